"""GPU checks of the corpus preparation (csrc/textprep.hip, include/snx.h "Corpus preparation"): snx.textprep,
src.preprocessing.mlm_data and the CLI.  Every comparison is equality: the segmentation against the plain-Python
restatement (tests/textprep_reference.py, itself held to the golden by tests/test_textprep_host.py) and against what the
reference's own functions produced (tests/golden/g25_mlm_data), the digests against hashlib, the dedup against a dict."""
import hashlib
import json
import random

import numpy as np
import pytest
import torch

from tests import textprep_reference as R
from tests.test_textprep_host import _write_sources, load_g25

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    return load_g25("cases.json.gz")


@pytest.fixture(scope="module")
def pipe():
    return load_g25("pipeline.json.gz")


def check_segmentation(docs, dev):
    """Pieces, their documents and their Hangul counts of one call equal the restatement's; -> the pieces."""
    from snx import textprep as tx
    seg = tx.segment_paragraphs(docs, dev)
    want = [R.segment(d) for d in docs]
    flat = [p for w in want for p in w]
    assert int(seg.par_ptr[0]) == 0 and int(seg.par_ptr[-1]) == seg.par_cps.numel() and seg.n_docs == len(docs)
    got = tx.paragraph_texts(seg.par_ptr, seg.par_cps)
    assert len(got) == len(flat)
    for i, (g, w) in enumerate(zip(got, flat)):
        assert g == w, (i, g[:80], w[:80])
    assert seg.par_doc.tolist() == [d for d, w in enumerate(want) for _ in w]
    assert seg.par_hangul.tolist() == [R.hangul_count(p) for p in flat]
    assert seg.lengths.tolist() == [len(p) for p in flat]
    return flat


# ------------------------------------------------------------------------------------------------ 1. segmentation
def test_segmentation_of_the_golden_documents_in_one_call(cases, dev):
    from snx import textprep as tx
    docs = cases["documents"]
    flat = check_segmentation(docs, dev)
    every = [p for lst in cases["paragraphs"][cases["grid"].index([0, 0.0])] for p in lst]
    assert flat == every                                     # the reference's own pieces, no filter
    seg = tx.segment_paragraphs(docs, dev)
    for (min_length, ratio), lists in zip(cases["grid"], cases["paragraphs"]):
        keep = torch.nonzero(tx.valid_mask(seg.lengths, seg.par_hangul, min_length, ratio)).flatten()
        assert tx.paragraph_texts(seg.par_ptr, seg.par_cps, keep) == [p for lst in lists for p in lst]


def test_segmentation_edge_documents(dev):
    docs = ["", "가", " ", "a", " \t\u3000\n\n\x0b\x0c\r\x1c\x1d\x1e\x1f\x85\xa0\u1680\u2000\u200a\u2028\u2029\u202f\u205f",
            "가\n나", "가\n\n나", "가\n\n\n나", "가\n\n\n\n나", "가\n\n\n\n\n\n\n나", "가\n \n나", "가\r\n\r\n나",
            "\t \t가", "가\t \t나", "가 \t", "\n", "\n\n", "\n\n\n", "가\n", "\n가", "\n\n가\n\n", "가\u200b\n\n\u200b"]
    flat = check_segmentation(docs, dev)
    assert "가 나" in flat and "가\n \n나" in flat and "가\r\n\r\n나" in flat and flat.count("나") == 4
    assert check_segmentation([], dev) == []
    assert check_segmentation([""], dev) == []
    assert check_segmentation(["", "", ""], dev) == []
    assert check_segmentation(["가", "", "나\n\n다"], dev) == ["가", "나", "다"]     # an empty document between two


def test_no_state_crosses_from_one_document_into_the_next(dev):
    docs = []
    for tail in ("\n", " ", "\t", "\n\n", " \n", "\u3000"):
        for head in ("\n", " ", "\t", "\n\n", "\n ", "\u3000"):
            docs += ["가나" + tail, head + "다라"]
    docs += ["가\n", "\n", "\n나", " ", " ", " 다", "라 ", "", " 마"]
    flat = check_segmentation(docs, dev)
    assert "가나" in flat and "다라" in flat and len(flat) == 2 * 36 + 5


def test_features_at_every_offset_across_two_tiles(dev):
    from snx.textprep import TILE
    assert TILE == 256
    features = ["   ", "\n\n", "\n\n\n", " \n\n ", "\u3000 \n", " \t ", "\n", "\n \n", "a \n\n\n\n b"]
    docs = ["가" * a + f + "나" * 3 for f in features for a in range(2 * TILE + 3)]
    docs += ["가" * a + f for f in ("\u3000 \n", "\n\n", " ") for a in range(TILE - 2, TILE + 3)]    # the feature ends the document
    flat = check_segmentation(docs, dev)
    assert "가" * TILE + " " + "나" * 3 in flat and "가" * (TILE - 1) in flat


def test_a_long_document_with_paragraphs_longer_than_a_tile(dev):
    from snx.textprep import TILE
    rng = random.Random(5)
    parts = []
    while sum(len(p) for p in parts) < 200_000:
        words = ["".join(chr(rng.randint(0xAC00, 0xD7AF)) for _ in range(rng.randint(1, 9))) for _ in range(rng.randint(1, 400))]
        parts.append(rng.choice(["", " ", "\u3000"]) + rng.choice([" ", "  ", "\t ", "\n", " \n"]).join(words) +
                     rng.choice(["", " ", " \t", "\n"]))
    doc = "".join(p + rng.choice(["\n\n", "\n\n\n", "\n\n\n\n\n"]) for p in parts)
    flat = check_segmentation(["가\n\n", doc, "\n\n나"], dev)
    assert len(doc) >= 200_000 and max(len(p) for p in flat) > 4 * TILE and len(flat) > 50
    ws_only = " \t\n\n\u3000 \n" * 300                      # white space only, several tiles
    assert check_segmentation([ws_only, "가"], dev) == ["가"]


# ------------------------------------------------------------------------------------------------ 2. validity
def test_validity_is_pythons_division_for_every_length_up_to_120(dev):
    from snx import textprep as tx
    docs, counts = [], []
    for n in range(1, 121):
        for h in range(n + 1):
            docs.append("가" * h + "a" * (n - h))
            counts.append((n, h))
    seg = tx.segment_paragraphs(docs, dev)
    assert list(zip(seg.lengths.tolist(), seg.par_hangul.tolist())) == counts
    start = {n: (n - 1) * (n + 2) // 2 for n in range(1, 122)}        # the rows of length n are start[n] .. start[n + 1]
    # 0.1, 0.3 and 1/3 with the rational form's misses (10, 1), (20, 2), (30, 3); 0.55 and 0.07 are where the multiplied
    # form h >= ratio * len differs from the division at these lengths: (100, 55) and (100, 7)
    for ratio in (0.1, 0.3, 1 / 3, 0.55, 0.07, 0.0, 1.0):
        got = tx.valid_mask(seg.lengths, seg.par_hangul, 0, ratio).tolist()
        assert got == [h / n >= ratio for n, h in counts] == [R.is_valid(n, h, 0, ratio) for n, h in counts], ratio
        for n in range(1, 121):                              # min_length equal to len, and to len + 1
            a, b = start[n], start[n + 1]
            assert counts[a] == (n, 0) and counts[b - 1] == (n, n)
            at_len = tx.valid_mask(seg.lengths[a:b], seg.par_hangul[a:b], n, ratio).tolist()
            assert at_len == got[a:b], (n, ratio)
            assert not tx.valid_mask(seg.lengths[a:b], seg.par_hangul[a:b], n + 1, ratio).any(), (n, ratio)
    at = {c: i for i, c in enumerate(counts)}
    m = tx.valid_mask(seg.lengths, seg.par_hangul, 0, 0.1).tolist()
    assert m[at[(10, 1)]] and m[at[(20, 2)]] and m[at[(30, 3)]] and not m[at[(11, 1)]]
    assert tx.valid_mask(seg.lengths, seg.par_hangul, 0, 0.55).tolist()[at[(100, 55)]]
    assert tx.valid_mask(seg.lengths, seg.par_hangul, 0, 0.07).tolist()[at[(100, 7)]]
    assert tx.valid_mask(seg.lengths, seg.par_hangul, 50, 0.0).tolist() == [n >= 50 for n, _ in counts]


def test_the_hangul_range_is_the_references(dev):
    from snx import textprep as tx
    docs = ["\uabff", "가", "힣", "\ud7af", "\ud7b0", "\uabff가힣\ud7af\ud7b0a"]
    seg = tx.segment_paragraphs(docs, dev)
    assert seg.par_hangul.tolist() == [0, 1, 1, 1, 0, 3]
    assert tx.valid_mask(seg.lengths, seg.par_hangul, 1, 1.0).tolist() == [False, True, True, True, False, False]


# ------------------------------------------------------------------------------------------------- 3. SHA-256
def _digests(texts, dev):
    from snx import textprep as tx
    ptr, cps = tx.code_point_csr(texts)
    d = tx.sha256_rows(ptr, cps, dev)
    assert d.dtype == torch.uint32 and tuple(d.shape) == (len(texts), 8)
    return ["".join("%08x" % w for w in row) for row in d.view(torch.int32).cpu().numpy().view(np.uint32).tolist()]


def _want(texts):
    return [hashlib.sha256(t.encode("utf-8")).hexdigest() for t in texts]


def test_sha256_at_the_block_and_padding_edges(dev):
    texts = ["a" * n for n in (0, 1, 55, 56, 63, 64, 65, 119, 120, 128)]
    texts += ["a" * 62 + "가" + "b", "a" * 63 + "가" + "b"]                          # 3 bytes from 62 and from 63
    texts += ["a" * s + "\U0001f600" + "b" * 5 for s in (61, 62, 63)]               # 4 bytes from 61, 62, 63
    texts += ["a" * 63 + "\xe9", "a" * 55 + "\xe9", "a" * 54 + "\xe9"]              # 2 bytes over the block / padding edge
    texts += ["", "가\n나", "a\xe9가\U0001f600\u044f" * 7, "\U0001f600" * 16, "가" * 21 + "a", "\u07ff\u0800\uffff\U00010000\U0010ffff\x7f\x80"]
    got = _digests(texts, dev)
    assert got == _want(texts)
    at = texts.index("")
    assert got[at] == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
    assert got[texts.index("가\n나")].startswith("a9017b3b") and got[texts.index("가\n나")].endswith("d7289e3f")
    assert _digests([], dev) == [] and _digests([""], dev) == [got[at]]


def test_sha256_of_rows_of_very_different_lengths_and_of_one_megabyte(dev):
    rng = random.Random(11)
    alphabet = "ab \n\xe9\u07ff가힣\uffff\U0001f600\U0010ffff"
    texts = ["".join(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 3, 20, 64, 300, 5000]))) for _ in range(200)]
    texts[7] = "가나다 abc \U0001f600" * 60_000                 # about 1 MB of UTF-8, in a wave with short rows
    assert len(texts[7].encode("utf-8")) > 1_000_000
    assert _digests(texts, dev) == _want(texts)


def test_sha256_refuses_what_is_no_scalar_value(dev):
    from snx import textprep as tx
    with pytest.raises(ValueError, match="scalar"):
        tx.sha256_rows(np.array([0, 1], dtype=np.int64), np.array([0xD800], dtype=np.int32), dev)
    with pytest.raises(ValueError, match="ptr must"):
        tx.sha256_rows(np.array([0, 5], dtype=np.int64), np.array([65], dtype=np.int32), dev)


# --------------------------------------------------------------------------------------------------- 4. dedup
def _first(rows: np.ndarray, dev):
    from snx import textprep as tx
    d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint32).view(np.int32)).to(dev).view(torch.uint32)
    first = tx.first_equal(d)
    assert first.dtype == torch.int32 and first.numel() == rows.shape[0]
    return first.cpu().numpy()


def test_first_equal_small_and_degenerate(dev):
    assert _first(np.zeros((0, 8), np.uint32), dev).tolist() == []
    assert _first(np.full((1, 8), 0xFFFFFFFF, np.uint32), dev).tolist() == [0]
    assert _first(np.full((1000, 8), 0xDEADBEEF, np.uint32), dev).tolist() == [0] * 1000
    assert _first(np.zeros((1000, 8), np.uint32), dev).tolist() == [0] * 1000
    distinct = np.arange(8 * 5000, dtype=np.uint32).reshape(5000, 8)
    assert _first(distinct, dev).tolist() == list(range(5000))


def test_first_equal_compares_all_256_bits(dev):
    rng = np.random.default_rng(3)
    base = rng.integers(0, 2 ** 32, size=(64, 8), dtype=np.uint64).astype(np.uint32)
    rows, want = [], []
    for b in base:
        for w in range(8):                                   # eight rows that agree with b in seven words each
            r = b.copy()
            r[w] ^= np.uint32(1 << (w * 3))
            rows.append(r)
        rows.append(b.copy())
        rows.append(b.copy())                                # and one true duplicate
    rows = np.stack(rows)
    want = R.first_equal(rows)
    assert _first(rows, dev).tolist() == want
    assert sum(1 for i, f in enumerate(want) if f != i) == 64
    low = np.zeros((16, 8), np.uint32)                       # rows that differ in ONE word only, each word in turn
    for w in range(8):
        low[2 * w, w], low[2 * w + 1, w] = 1, 2
    assert _first(low, dev).tolist() == list(range(16))


def test_first_equal_far_apart_and_random_against_a_dict(dev):
    rng = np.random.default_rng(4)
    n = 200_000
    rows = rng.integers(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    src = rng.integers(0, n, size=n)
    dup = rng.random(n) < 0.3
    rows[dup] = rows[src[dup]]                               # 30 % copies of other rows, earlier or later
    rows[150_000] = rows[50_000]                             # 100,000 rows apart
    rows[199_999] = rows[0]
    want = R.first_equal([r.tobytes() for r in rows])
    got = _first(rows, dev)
    assert got.tolist() == want
    assert got[199_999] == got[0] and got[150_000] == got[50_000] and (got != np.arange(n)).mean() > 0.2
    assert np.array_equal(_first(rows, dev), got)            # run to run


def test_first_equal_from_texts(dev):
    from snx import textprep as tx
    texts = ["가나다", "abc", "가나다", "", "abc ", "", "가나다", "\U0001f600"]
    ptr, cps = tx.code_point_csr(texts)
    assert tx.first_equal(tx.sha256_rows(ptr, cps, dev)).tolist() == [0, 1, 0, 3, 4, 3, 0, 7]


# ---------------------------------------------------------------------------------------------- 5. end to end
def test_prepare_mlm_corpus_equals_the_golden_whatever_the_batch_size(pipe, dev):
    from src.preprocessing.mlm_data import line_bytes, prepare_mlm_corpus
    for run in ("main", "single"):
        g = pipe[run]
        reports = []
        for batch in (1, 3000, 1 << 24):                     # every document its own batch .. one batch for all
            c = prepare_mlm_corpus(g["sources"], g["min_length"], g["min_korean_ratio"], g["val_ratio"], g["seed"],
                                   batch_code_points=batch, device=dev)
            assert c.train == g["train"] and c.val == g["val"] and c.stats == g["stats"]
            assert (c.valid, c.unique) == (len(g["valid"]), len(g["unique"]))
            for name in ("train", "val"):
                data = line_bytes(getattr(c, name))
                assert hashlib.sha256(data).hexdigest() == g["files"][name]["sha256"]
            reports.append(c.report)
        assert reports[0] == reports[1] == reports[2]


def test_the_cli_writes_the_goldens_files(pipe, dev, tmp_path, capsys):
    from src.train.cli import prepare_mlm_data as cli
    g = pipe["main"]
    with open(tmp_path / "a_body.jsonl", "w", encoding="utf-8") as f:
        for doc in g["sources"][0]:
            f.write(json.dumps({"body": doc}) + "\n")
    _, b = _write_sources(tmp_path, g["sources"])
    out = tmp_path / "out"
    summary = cli.main(["--input", str(tmp_path / "a_body.jsonl"), "--input", b, "--text-field", "body", "--output-dir",
                        str(out), "--device", str(dev), "--report", str(tmp_path / "r.jsonl")])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    for name in ("train", "val"):
        assert hashlib.sha256((out / f"{name}.txt").read_bytes()).hexdigest() == g["files"][name]["sha256"]
    assert (summary["train"], summary["val"], summary["valid"]) == (len(g["train"]), len(g["val"]), len(g["valid"]))
    assert summary["mean_length"] == g["stats"]["mean_length"]
    assert summary["mean_korean_ratio"] == g["stats"]["mean_korean_ratio"]
    (tmp_path / "latin.txt").write_text("nothing here is hangul, however long the paragraph may turn out to be", encoding="utf-8")
    with pytest.raises(SystemExit) as e:
        cli.main(["--input", str(tmp_path / "latin.txt"), "--output-dir", str(tmp_path / "o2"), "--device", str(dev)])
    assert e.value.code == 1
