"""CPU checks of MinHash near-duplicate removal (include/snx.h "MinHash near-duplicate removal"): the hashlib restatement
(tests/minhash_reference.py) that the GPU suite (test_gpu_minhash.py) holds csrc/minhash.hip to is itself held to what the
reference's MinHashDeduplicator produced (tests/golden/g16, tools/make_golden_minhash.py); the host half of snx.minhash
(need, code-point CSR, message length, validators); the C ABI's presence and argument checks; and the CLI round trip with
the two GPU calls replaced by the restatement."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import minhash_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16 = os.path.join(ROOT, "tests", "golden", "g16")


@pytest.fixture(scope="module")
def g16():
    with open(os.path.join(G16, "rows.json"), encoding="utf-8") as f:
        rec = json.load(f)
    rec["rows"] = [tuple(r) for r in rec["rows"]]
    rec["signatures"] = dict(np.load(os.path.join(G16, "signatures.npz")))
    return rec


def test_restatement_reproduces_the_reference(g16):
    rows = g16["rows"]
    assert len(rows) == 48 and [tuple(s) for s in g16["settings"]] == [(128, 0.8, 3), (128, 0.5, 3), (100, 0.8, 2),
                                                                         (16, 1.0, 5)]
    for num_perm, threshold, ngram in g16["settings"]:
        dup, sig = R.deduplicate(rows, num_perm, threshold, ngram)
        want = g16["signatures"][f"p{num_perm}_n{ngram}"]
        assert sig.dtype == np.uint32 and sig.shape == (len(rows), num_perm, 4) and np.array_equal(sig, want)
        kept = g16["kept"][f"{num_perm},{threshold},{ngram}"]
        assert np.flatnonzero(dup < 0).tolist() == kept
        assert 0 < len(kept) < len(rows)                     # every setting drops something and keeps something
        for i in np.flatnonzero(dup >= 0):                   # a dropped row names an earlier kept row
            assert dup[i] < i and dup[dup[i]] == -1


def test_need_matches_is_the_float_comparison():
    from snx.minhash import need_matches
    for num_perm in (16, 100, 128):
        for threshold in (0, 0.5, 0.8, 1.0, 1.01):
            need = need_matches(num_perm, threshold)
            for m in range(num_perm + 1):
                assert (m / num_perm >= threshold) == (m >= need), (num_perm, threshold, m)
            assert need == R.need_matches(num_perm, threshold)
    assert need_matches(128, 0.8) == 103 and need_matches(128, 0) == 0 and need_matches(128, 1.01) == 129
    assert need_matches(100, 0.8) == 80 and need_matches(16, 1.0) == 16 and need_matches(16, float("nan")) == 17
    with pytest.raises(ValueError, match="need_matches"):
        need_matches(0, 0.5)


EDGE = ["", "a", "ab", "abc", "abcd", "aé한\U0001F600я", "İSTANBUL İ", "  padded text \t\n", "zzzzzzzz"]


def test_code_point_csr_of_the_edge_strings():
    from snx.minhash import code_point_csr, longest_message_bytes
    ptr, cps = code_point_csr(EDGE)
    assert ptr.dtype == np.int64 and cps.dtype == np.int32
    low = [t.lower().strip() for t in EDGE]
    assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in low])]).tolist()
    assert cps.tolist() == [ord(c) for t in low for c in t]
    assert len(low[6]) == len(EDGE[6]) + 2                   # each İ lowers to two code points
    assert low[7] == "padded text"
    # the longest message: prefix digits + underscore + the longest n-gram's UTF-8 bytes, rows shorter than n as a whole
    for n in (1, 2, 3, 5, 12):
        grams = set().union(*(R.ngrams(t, n) for t in low))
        want = max(len(g.encode()) for g in grams)
        assert longest_message_bytes(ptr, cps, n, 128) == 4 + want, n
        assert longest_message_bytes(ptr, cps, n, 10) == 2 + want
    e_ptr, e_cps = code_point_csr([])
    assert e_ptr.tolist() == [0] and e_cps.size == 0 and longest_message_bytes(e_ptr, e_cps, 3, 128) == 4
    assert longest_message_bytes(*code_point_csr(["\U0001F600" * 20]), 12, 128) == 52
    assert longest_message_bytes(*code_point_csr(["ab"]), 3, 128) == 6


def test_validators_name_their_caller():
    from snx.minhash import first_match, greedy_dedup, minhash_signatures, signature_inputs
    with pytest.raises(ValueError, match="minhash_signatures: texts must be strings"):
        signature_inputs(["a", 3])
    with pytest.raises(ValueError, match="minhash_signatures: .*lone surrogate"):
        signature_inputs(["ok", "bad \ud800 text"])
    with pytest.raises(ValueError, match=r"minhash_signatures: num_perm must be in \[1, 256\]"):
        signature_inputs(["a"], num_perm=257)
    with pytest.raises(ValueError, match="minhash_signatures: num_perm must be an int"):
        signature_inputs(["a"], num_perm=12.0)
    with pytest.raises(ValueError, match="minhash_signatures: ngram_size must be >= 1"):
        signature_inputs(["a"], ngram_size=0)
    # 13 four-byte code points: "127_" + 52 bytes = 56 > 55; twelve of them fit (52), and so do 51 + 4 = 55 ASCII bytes
    with pytest.raises(ValueError, match="minhash_signatures: the longest message .* has 56 bytes"):
        signature_inputs(["\U0001F600" * 13], num_perm=128, ngram_size=13)
    signature_inputs(["\U0001F600" * 13], num_perm=128, ngram_size=12)
    signature_inputs(["x" * 60], num_perm=128, ngram_size=51)
    with pytest.raises(ValueError, match="has 56 bytes"):
        signature_inputs(["x" * 60], num_perm=128, ngram_size=52)
    signature_inputs(["x" * 60], num_perm=100, ngram_size=52)   # prefixes of two digits: 55 bytes
    with pytest.raises(ValueError, match="minhash_signatures: runs on a GPU"):
        minhash_signatures(["a"], device="cpu")
    import torch
    with pytest.raises(ValueError, match="greedy_dedup: signatures must be uint32"):
        greedy_dedup(torch.zeros((2, 4, 4), dtype=torch.int32), 3)      # not on a GPU
    with pytest.raises(ValueError, match="first_match: signatures must be uint32"):
        first_match(np.zeros((2, 4, 4), np.uint32), None, 3)


def test_c_abi_section_and_argument_checks():
    from snx import asmcheck, fn
    from snx._lib import SIGNATURES
    text = open(os.path.join(ROOT, "include", "snx.h")).read()
    assert "---- MinHash near-duplicate removal (csrc/minhash.hip)" in text
    assert "#define SNX_MINHASH_MSG_MAX 55" in text and "#define SNX_MINHASH_PERM_MAX 256" in text
    for n in ("snx_minhash_signatures", "snx_minhash_dedup_workspace_bytes", "snx_minhash_dedup",
              "snx_minhash_first_match"):
        assert re.search(r"\b%s\(" % n, text) and n in SIGNATURES, n
    assert set(asmcheck.GUARDED["minhash.hip"]) == {"mh_sig_kernel", "mh_match_kernel", "mh_resolve_kernel"}
    one = C.c_void_p(256)
    sigs, dedup, first = fn("snx_minhash_signatures"), fn("snx_minhash_dedup"), fn("snx_minhash_first_match")
    size = fn("snx_minhash_dedup_workspace_bytes")
    assert sigs(one, one, 4, 3, 257, one, None) == -2 and sigs(one, one, 4, 0, 128, one, None) == -2
    assert sigs(one, one, -1, 3, 128, one, None) == -2 and sigs(None, one, 4, 3, 128, one, None) == -3
    assert sigs(None, None, 0, 3, 128, None, None) == 0      # nothing to do
    assert size(0, 128) == 0 and size(10, 0) == 0 and size(10, 257) == 0
    # compacted low words [P][n rounded to 64] + kept list + key keepers + one block's state
    assert size(1000, 128) >= 128 * 1024 * 4 + 2 * 1000 * 4 + 128 * 512 * 4 + 512 * 512 // 8
    assert size(1000, 128) < 2 * (128 * 1024 * 4 + 128 * 512 * 4)
    assert dedup(one, 10, 128, 103, None, one, one, size(10, 128) - 1, None) == -3       # workspace too small
    assert dedup(one, 10, 128, 103, None, one, None, 0, None) == -3
    assert dedup(None, 10, 128, 103, None, one, one, size(10, 128), None) == -3
    assert dedup(one, 10, 300, 103, None, one, one, 1 << 30, None) == -2
    assert dedup(None, 0, 128, 103, None, None, None, 0, None) == 0
    assert first(one, 65536, one, 4, 128, 103, one, None) == -2
    assert first(None, 2, one, 4, 128, 103, one, None) == -3 and first(one, 2, None, 4, 128, 103, one, None) == -3
    assert first(None, 0, None, 0, 128, 103, None, None) == 0


def test_exact_deduplicator_and_keys():
    from collections import namedtuple
    from src.preprocessing.cleaners import MinHashDeduplicator
    from src.preprocessing.cleaners.deduplicator import ExactDeduplicator, exact_groups, pair_key
    T = namedtuple("T", "query positive")
    rows = [T("A cat", "x"), T(" A cat ", "x "), T("a cat", "x"), T("A cat", "y"), T("A cat", "x")]
    d = ExactDeduplicator()
    assert d.deduplicate(rows) == [rows[0], rows[2], rows[3]]     # strips, keeps case, does not join the two texts
    assert d.is_duplicate("a cat ", " x") and not d.is_duplicate("b", "x") and d.is_duplicate("b", "x")
    d.clear()
    assert not d.is_duplicate("A cat", "x")
    assert pair_key(" A Cat", "X ") == "a cat|||x"
    assert exact_groups([tuple(r) for r in rows]).tolist() == [0, 0, 0, 3, 0]
    m = MinHashDeduplicator()
    assert (m.num_perm, m.threshold, m.ngram_size) == (128, 0.8, 3)
    import inspect
    assert [str(p) for p in inspect.signature(MinHashDeduplicator.__init__).parameters.values()] == [
        "self", "num_perm: 'int' = 128", "threshold: 'float' = 0.8", "ngram_size: 'int' = 3"]


def _stub_gpu(monkeypatch):
    """snx.minhash's two GPU calls replaced by the restatement, on CPU tensors."""
    import torch
    from snx import minhash as M

    def signatures(texts, num_perm=128, ngram_size=3, device="cuda"):
        M.signature_inputs(texts, num_perm, ngram_size)
        return torch.from_numpy(R.signatures(texts, num_perm, ngram_size).view(np.int32))

    def dedup(sig, need, exact_group=None):
        return torch.from_numpy(R.greedy(sig.numpy().view(np.uint32), need, exact_group))

    monkeypatch.setattr(M, "minhash_signatures", signatures)
    monkeypatch.setattr(M, "greedy_dedup", dedup)


def test_cli_round_trip(tmp_path, monkeypatch, capsys, g16):
    import torch
    if not torch.cuda.is_available():
        _stub_gpu(monkeypatch)
    from src.train.cli import dedup_triplets
    rows = g16["rows"]
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    lines = [json.dumps({"query": q, "positive": p, "negative": f"neg {i}", "source": "g16"}, ensure_ascii=False)
             for i, (q, p) in enumerate(rows)]
    cut = 20
    (src / "train_000.jsonl").write_text("".join(x + "\n" for x in lines[:cut]) + "\n", encoding="utf-8")   # a blank line
    (src / "train_001.jsonl").write_text("\n".join(lines[cut:]), encoding="utf-8")                         # no final newline
    report = tmp_path / "report.jsonl"
    out = dedup_triplets.main(["--input-pattern", str(src / "train_*.jsonl"), "--output-dir", str(dst), "--report",
                               str(report), "--device", "cuda:0"])
    want, _ = R.deduplicate(rows)
    kept = np.flatnonzero(want < 0).tolist()
    assert kept == g16["kept"]["128,0.8,3"]
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == out and out["rows_in"] == len(rows) and out["rows_kept"] == len(kept)
    keys = [R.pair_key(q, p) for q, p in rows]
    exact = sum(1 for i, d in enumerate(want) if d >= 0 and keys[d] == keys[i])
    assert exact > 0 and out["exact_duplicates"] == exact
    assert out["minhash_duplicates"] == len(rows) - len(kept) - exact > 0
    assert (dst / "train_000.jsonl").read_text(encoding="utf-8").splitlines() == [lines[i] for i in kept if i < cut]
    assert (dst / "train_001.jsonl").read_text(encoding="utf-8").splitlines() == [lines[i] for i in kept if i >= cut]
    rep = [json.loads(x) for x in report.read_text().splitlines()]
    assert [r["row"] for r in rep] == list(range(len(rows)))
    assert [-1 if r["duplicate_of"] is None else r["duplicate_of"]["row"] for r in rep] == want.tolist()
    for r in rep:
        i = r["row"]
        assert (r["file"], r["line"]) == (("train_000.jsonl", i) if i < cut else ("train_001.jsonl", i - cut))
    with pytest.raises(ValueError, match="output-dir"):
        dedup_triplets.main(["--input-pattern", str(src / "train_*.jsonl"), "--output-dir", str(src)])
    with pytest.raises(FileNotFoundError):
        dedup_triplets.main(["--input-pattern", str(src / "none_*.jsonl"), "--output-dir", str(dst)])
