"""CPU checks of the corpus preparation (snx.textprep's host half, src.preprocessing.mlm_data, the CLI
src.train.cli.prepare_mlm_data): the plain-Python restatement (tests/textprep_reference.py) against what the reference's
own functions produced (tests/golden/g25_mlm_data), and the host code around the device stages with those stages replaced
by the restatement at their function boundary (``mlm_data.batch_stage``, ``mlm_data.dedup_stage``)."""
import gzip
import hashlib
import json
import os
import random

import numpy as np
import pytest

from tests import textprep_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = os.path.join(ROOT, "tests", "golden", "g25_mlm_data")


def load_g25(name: str):
    with gzip.open(os.path.join(G25, name), "rt", encoding="ascii") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases():
    return load_g25("cases.json.gz")


@pytest.fixture(scope="module")
def pipe():
    return load_g25("pipeline.json.gz")


# ---------------------------------------------------------------------------------- the device stages, restated
def host_batch_stage(doc_ptr, doc_cps, min_length, min_korean_ratio, device):
    from snx.textprep import code_point_csr, csr_texts
    from src.preprocessing.mlm_data import ValidBatch
    docs = csr_texts(doc_ptr, doc_cps)
    rows, doc, hangul, pieces = [], [], [], []
    for d, text in enumerate(docs):
        seg = R.segment(text)
        pieces.append(len(seg))
        for p in seg:
            if R.is_valid(len(p), R.hangul_count(p), min_length, min_korean_ratio):
                rows.append(p)
                doc.append(d)
                hangul.append(R.hangul_count(p))
    ptr, cps = code_point_csr(rows)
    digests = np.array([R.sha256_words(p) for p in rows], dtype=np.uint32).reshape(len(rows), 8)
    return ValidBatch(ptr, cps, np.array(hangul, dtype=np.int32), np.array(doc, dtype=np.int32),
                      np.array(pieces, dtype=np.int64), digests)


def host_dedup_stage(digests):
    if not digests:
        return np.zeros(0, dtype=np.int64)
    return np.array(R.first_equal(list(np.concatenate(digests))), dtype=np.int64)


@pytest.fixture
def host_stages(monkeypatch):
    from src.preprocessing import mlm_data
    monkeypatch.setattr(mlm_data, "batch_stage", host_batch_stage)
    monkeypatch.setattr(mlm_data, "dedup_stage", host_dedup_stage)
    return mlm_data


# ------------------------------------------------------------------------------------ the restatement and the golden
def test_the_restatement_equals_every_case_of_the_golden(cases):
    assert len(cases["documents"]) >= 330 and len(cases["grid"]) >= 6
    n = 0
    for (min_length, ratio), lists in zip(cases["grid"], cases["paragraphs"]):
        assert len(lists) == len(cases["documents"])
        for doc, want in zip(cases["documents"], lists):
            assert R.valid_paragraphs(doc, min_length, ratio) == want, (doc, min_length, ratio)
            n += len(want)
    assert n > 3000                                          # the golden is not a list of empty lists
    for text, hexdigest in cases["known_sha256"].items():
        assert "".join("%08x" % w for w in R.sha256_words(text)) == hexdigest
    assert cases["known_sha256"][""].startswith("e3b0c442") and cases["known_sha256"][""].endswith("7852b855")
    assert cases["known_sha256"]["가\n나"].startswith("a9017b3b") and cases["known_sha256"]["가\n나"].endswith("d7289e3f")


def test_the_white_space_list_is_pythons_isspace():
    want = {c for c in range(0x110000) if chr(c).isspace()}
    got = {c for lo, hi in R.SPACE_RANGES for c in range(lo, hi + 1)}
    assert got == want
    assert all(R.is_space(c) for c in want) and not any(R.is_space(c) for c in (0x08, 0x0E, 0x1B, 0x21, 0x200B, 0x2060))


def test_ratio_is_pythons_division_not_the_rational_or_the_multiplied_form():
    assert R.is_valid(10, 1, 0, 0.1) and R.is_valid(20, 2, 0, 0.1) and R.is_valid(30, 3, 0, 0.1)
    from fractions import Fraction
    assert not Fraction(1, 10) >= Fraction(0.1)              # the rational form drops (10, 1): the float 0.1 is above 1/10
    # the multiplied form h >= ratio * len agrees with the division at 0.1 for every len <= 120; it differs at these two
    assert 55 / 100 >= 0.55 and not 55 >= 0.55 * 100 and R.is_valid(100, 55, 0, 0.55)
    assert 7 / 100 >= 0.07 and not 7 >= 0.07 * 100 and R.is_valid(100, 7, 0, 0.07)
    assert R.is_valid(0, 0, 0, 0.0) and not R.is_valid(0, 0, 0, 0.1) and not R.is_valid(4, 4, 5, 0.0)


def test_the_restatement_reproduces_the_pipeline_golden(pipe):
    for run in ("main", "single"):
        g = pipe[run]
        unique, train, val, tb, vb, stats = R.pipeline(g["sources"], g["min_length"], g["min_korean_ratio"],
                                                       g["val_ratio"], g["seed"])
        assert [R.sha256_words(p) for p in g["valid"]] == \
            [tuple(int(h[8 * j:8 * j + 8], 16) for j in range(8)) for h in g["valid_sha256"]]
        assert (unique, train, val) == (g["unique"], g["train"], g["val"])
        assert hashlib.sha256(tb).hexdigest() == g["files"]["train"]["sha256"] and len(tb) == g["files"]["train"]["bytes"]
        assert hashlib.sha256(vb).hexdigest() == g["files"]["val"]["sha256"] and len(vb) == g["files"]["val"]["bytes"]
        assert stats == g["stats"]
    assert len(pipe["main"]["valid"]) > len(pipe["main"]["unique"]) > 20 and len(pipe["main"]["val"]) >= 1
    s = pipe["single"]
    assert int(len(s["unique"]) * (1 - s["val_ratio"])) == 0 and len(s["train"]) == 1 and s["val"] == []


# ----------------------------------------------------------------------------------------------- the host tail
def test_shuffling_indices_is_shuffling_the_paragraphs(pipe):
    from src.preprocessing.mlm_data import split_indices
    for run in ("main", "single"):
        g = pipe[run]
        tr, va = split_indices(len(g["unique"]), g["val_ratio"], g["seed"])
        assert [g["unique"][i] for i in tr] == g["train"] and [g["unique"][i] for i in va] == g["val"]
    random.seed(7)
    rows = [f"row {i}" for i in range(1000)]
    shuffled = rows.copy()
    random.shuffle(shuffled)
    tr, va = split_indices(1000, 0.05, 7)
    assert [rows[i] for i in tr + va] == shuffled and len(tr) == 950


def test_the_host_tail_reproduces_the_goldens_files_and_stats(pipe, tmp_path):
    from src.preprocessing.mlm_data import finish_corpus, line_bytes, write_corpus
    for run in ("main", "single"):
        g = pipe[run]
        unique = g["unique"]
        corpus = finish_corpus(unique, [len(p) for p in unique], [R.hangul_count(p) for p in unique], g["val_ratio"],
                               g["seed"])
        assert corpus.train == g["train"] and corpus.val == g["val"] and corpus.stats == g["stats"]
        out = tmp_path / run
        write_corpus(corpus, str(out))
        for name in ("train", "val"):
            data = (out / f"{name}.txt").read_bytes()
            assert hashlib.sha256(data).hexdigest() == g["files"][name]["sha256"]
            assert data == line_bytes(getattr(corpus, name))
    assert line_bytes(["가\n나\r다\u2028라"]) == "가 나\r다\u2028라\n".encode("utf-8")      # only U+000A is replaced
    empty = finish_corpus([], [], [])
    assert empty.train == [] and empty.val == [] and empty.stats["total"] == 0


def test_python_mirrors_the_kernels_constants_and_the_header_declares_the_section():
    import re
    from snx import _abi, textprep as tx
    src = open(os.path.join(ROOT, "opensearch-neural-pre-train_amd", "csrc", "textprep.hip"), encoding="utf-8").read()
    assert int(re.search(r"constexpr int TX_THREADS = (\d+);", src)[1]) == tx.TILE
    assert re.search(r"constexpr int TX_TILE = TX_THREADS;", src)
    assert 1 << int(re.search(r"constexpr int64_t TX_DEDUP_MAX = 1ll << (\d+);", src)[1]) == tx.FIRST_EQUAL_MAX
    assert (tx.HANGUL_LO, tx.HANGUL_HI) == (R.HANGUL_LO, R.HANGUL_HI) == (0xAC00, 0xD7AF)
    names = {n for n in _abi.PROTOTYPES if n.startswith("snx_tx_")}
    assert names == {"snx_tx_segment_count", "snx_tx_segment_meta", "snx_tx_segment_fill", "snx_tx_sha256_rows",
                     "snx_tx_first_equal_workspace_bytes", "snx_tx_first_equal"}
    from snx._lib import fn
    assert fn("snx_tx_first_equal_workspace_bytes")(1000) == 4 * (2048 + 1000)
    assert fn("snx_tx_first_equal_workspace_bytes")(0) == 0
    assert fn("snx_tx_first_equal")(None, -1, None, None, 0, None) == -2           # refused on the host, no launch
    assert fn("snx_tx_segment_count")(None, None, 3, None, None, None) == -3
    assert fn("snx_tx_sha256_rows")(None, None, 0, None, None) == 0


# ------------------------------------------------------------------------------------------ packer and pipeline
def test_code_point_csr_keeps_the_text_as_it_is_and_refuses_a_lone_surrogate():
    from snx.textprep import LoneSurrogateError, code_point_csr, csr_texts
    texts = ["  UPPER 가\n", "", "\U0001f600a"]
    ptr, cps = code_point_csr(texts)
    assert ptr.tolist() == [0, 10, 10, 12] and ptr.dtype == np.int64 and cps.dtype == np.int32
    assert cps.tolist() == [ord(ch) for t in texts for ch in t]
    assert csr_texts(ptr, cps) == texts
    with pytest.raises(LoneSurrogateError, match="text 2") as e:
        code_point_csr(["ok", "가", "bad \ud800 text", "\udfff"])
    assert e.value.index == 2 and isinstance(e.value, ValueError)
    with pytest.raises(ValueError, match="strings"):
        code_point_csr(["a", 3])


def test_argument_checks_raise_before_any_launch():
    import torch
    from snx import textprep as tx
    with pytest.raises(ValueError, match="min_length"):
        tx.valid_mask(torch.tensor([3]), torch.tensor([1]), 1.5, 0.3)
    with pytest.raises(ValueError, match="one size"):
        tx.valid_mask(torch.tensor([3, 4]), torch.tensor([1]), 1, 0.3)
    with pytest.raises(ValueError, match="uint32"):
        tx.first_equal(torch.zeros((4, 8), dtype=torch.int32))              # not on a GPU
    with pytest.raises(ValueError, match="uint32"):
        tx.first_equal(np.zeros((4, 8), dtype=np.uint32))
    with pytest.raises(ValueError, match="ptr int64"):
        tx.sha256_rows(np.zeros(2, dtype=np.int32), np.zeros(0, dtype=np.int32))
    # the mask itself is plain torch and runs anywhere: Python's decision on the CPU too
    got = tx.valid_mask(torch.tensor([10, 20, 30, 10, 0]), torch.tensor([1, 2, 3, 0, 0]), 0, 0.1).tolist()
    assert got == [True, True, True, False, False]


def test_prepare_mlm_corpus_with_host_stages_equals_the_golden_at_every_batch_size(pipe, host_stages):
    for run in ("main", "single"):
        g = pipe[run]
        results = []
        for batch in (1, 700, 1 << 24):
            c = host_stages.prepare_mlm_corpus(g["sources"], g["min_length"], g["min_korean_ratio"], g["val_ratio"],
                                               g["seed"], batch_code_points=batch, device="cpu")
            assert (c.train, c.val, c.stats) == (g["train"], g["val"], g["stats"])
            assert (c.valid, c.unique) == (len(g["valid"]), len(g["unique"]))
            assert c.documents == sum(len(s) for s in g["sources"]) == len(c.report)
            assert sum(r["valid"] for r in c.report) == c.valid and sum(r["kept"] for r in c.report) == c.unique
            assert sum(r["pieces"] for r in c.report) == c.pieces >= c.valid
            results.append(c)
        assert results[0].report == results[1].report == results[2].report


def test_a_lone_surrogate_names_the_source_and_the_document(host_stages):
    with pytest.raises(ValueError, match=r"mc4, document 1.*lone surrogate"):
        host_stages.prepare_mlm_corpus([["가나다"], ["fine", "bad \udc00"]], source_names=["wiki", "mc4"], device="cpu",
                                       batch_code_points=4)
    with pytest.raises(ValueError, match="val_ratio"):
        host_stages.prepare_mlm_corpus([["가"]], val_ratio=1.0, device="cpu")


# ------------------------------------------------------------------------------------------------------ the CLI
def _write_sources(tmp_path, sources):
    a = tmp_path / "a_wiki.jsonl"
    with open(a, "w", encoding="utf-8") as f:
        for i, doc in enumerate(sources[0]):
            f.write(json.dumps({"id": i, "text": doc}, ensure_ascii=bool(i % 2)) + "\n")
            if i == 3:
                f.write("\n")                                # a blank line is no document
    half = len(sources[1]) // 2
    for name, docs in (("b_mc4_0.jsonl", sources[1][:half]), ("b_mc4_1.jsonl", sources[1][half:])):
        with open(tmp_path / name, "w", encoding="utf-8") as f:
            for doc in docs:
                f.write(json.dumps({"body": doc, "text": 7}) + "\n")
    return str(a), str(tmp_path / "b_mc4_*.jsonl")


def test_cli_parsing():
    from src.train.cli.prepare_mlm_data import parse_args
    a = parse_args(["--input", "x.jsonl"])
    assert (a.input, a.max_docs, a.output_dir, a.min_length, a.korean_ratio, a.val_ratio, a.seed, a.text_field) == \
        (["x.jsonl"], [0], "data/mlm_korean", 50, 0.3, 0.05, 42, "text")
    a = parse_args(["--input", "w", "--max-docs", "5", "--input", "m", "--input", "z", "--korean-ratio", "0.5"])
    assert a.input == ["w", "m", "z"] and a.max_docs == [5, 0, 0] and a.korean_ratio == 0.5
    with pytest.raises(SystemExit):
        parse_args(["--input", "w", "--max-docs", "1", "--max-docs", "2"])
    with pytest.raises(SystemExit):
        parse_args([])


def test_cli_reads_jsonl_and_txt_and_counts_max_docs(tmp_path):
    from src.train.cli.prepare_mlm_data import read_documents
    p = tmp_path / "d.jsonl"
    p.write_text('{"text": "one"}\n\n{"other": "x"}\n{"text": 5}\n{"text": "four\\r\\n"}\n["text"]\n', encoding="utf-8")
    assert list(read_documents(str(p))) == ["one", "", "", "four\r\n", ""]
    assert list(read_documents(str(p), "other")) == ["", "x", "", "", ""]
    assert list(read_documents(str(p), "text", 2)) == ["one", ""]
    (tmp_path / "t2.txt").write_bytes("둘\r\n\r\n끝".encode("utf-8"))
    (tmp_path / "t1.txt").write_bytes("하나\n\n문단\n".encode("utf-8"))
    assert list(read_documents(str(tmp_path / "t*.txt"))) == ["하나\n\n문단\n", "둘\r\n\r\n끝"]      # sorted, CR kept
    assert list(read_documents(str(tmp_path / "t*.txt"), max_docs=1)) == ["하나\n\n문단\n"]
    with pytest.raises(FileNotFoundError):
        list(read_documents(str(tmp_path / "none*.txt")))


def test_cli_writes_the_goldens_files_and_prints_the_stats(pipe, host_stages, tmp_path, capsys):
    from src.train.cli import prepare_mlm_data as cli
    g = pipe["main"]
    a, b = _write_sources(tmp_path, g["sources"])
    out = tmp_path / "out"
    report = tmp_path / "report.jsonl"
    summary = cli.main(["--input", a, "--input", b, "--text-field", "text", "--output-dir", str(out), "--report",
                        str(report), "--device", "cpu"])
    # the second source keeps its text in "body": under --text-field text it is all empty documents
    assert summary["documents"] == sum(len(s) for s in g["sources"]) and summary["unique"] < len(g["unique"])
    capsys.readouterr()
    with open(tmp_path / "a_body.jsonl", "w", encoding="utf-8") as f:
        for doc in g["sources"][0]:
            f.write(json.dumps({"body": doc}) + "\n")
    summary = cli.main(["--input", str(tmp_path / "a_body.jsonl"), "--input", b, "--text-field", "body", "--output-dir",
                        str(out), "--report", str(report), "--device", "cpu", "--batch-code-points", "500"])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == summary
    for name in ("train", "val"):
        assert hashlib.sha256((out / f"{name}.txt").read_bytes()).hexdigest() == g["files"][name]["sha256"]
    assert (summary["train"], summary["val"], summary["unique"], summary["valid"]) == \
        (len(g["train"]), len(g["val"]), len(g["unique"]), len(g["valid"]))
    assert summary["mean_length"] == g["stats"]["mean_length"]
    assert summary["mean_korean_ratio"] == g["stats"]["mean_korean_ratio"]
    rows = [json.loads(line) for line in open(report, encoding="utf-8")]
    assert len(rows) == summary["documents"] and sum(r["kept"] for r in rows) == summary["unique"]
    assert [r["source"] for r in rows] == [0] * len(g["sources"][0]) + [1] * len(g["sources"][1])


def test_cli_max_docs_takes_the_first_documents_of_its_source(pipe, host_stages, tmp_path, capsys):
    from src.train.cli import prepare_mlm_data as cli
    g = pipe["main"]
    a, _ = _write_sources(tmp_path, g["sources"])
    summary = cli.main(["--input", a, "--max-docs", "4", "--output-dir", str(tmp_path / "o"), "--device", "cpu"])
    want = R.pipeline([g["sources"][0][:4]], 50, 0.3, 0.05, 42)
    assert summary["documents"] == 4 and summary["unique"] == len(want[0])
    assert (tmp_path / "o" / "train.txt").read_bytes() == want[3]


def test_cli_exits_with_status_1_when_nothing_valid_remains(host_stages, tmp_path, capsys):
    from src.train.cli import prepare_mlm_data as cli
    (tmp_path / "latin.txt").write_text("no hangul here at all, however long the paragraph may be\n\nshort", encoding="utf-8")
    with pytest.raises(SystemExit) as e:
        cli.main(["--input", str(tmp_path / "latin.txt"), "--output-dir", str(tmp_path / "o"), "--device", "cpu"])
    assert e.value.code == 1
    assert "No valid paragraphs" in capsys.readouterr().err and not (tmp_path / "o" / "train.txt").exists()
