"""GPU checks of the character n-gram TF-IDF step (csrc/tfidf.hip, include/snx.h "Character n-gram TF-IDF"):
snx.retrieval.TfidfIndex, src.train.mining.tfidf and the CLI over it.

Small shapes against the plain-Python restatement (tests/tfidf_reference.py): keys, counts, feature ids and nnz are compared
exactly; weights within 1 fp32 ulp, which holds because they are computed in float64 and rounded once (a float64 sum of
squares in another order, or another libm's logarithm, moves the float64 value by parts in 10^16 and so its fp32 rounding by
at most one step).  Then tests/golden/g17_tfidf end to end: what scikit-learn and the reference's miner produced."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import tfidf_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G17 = os.path.join(ROOT, "tests", "golden", "g17_tfidf")

EDGE = [
    "a",                                                     # L == 3: the trigram is the whole padded word
    "ab cd",                                                 # no window across the space
    "aaaa",                                                  # repeated keys in one row
    "",
    " \t\n  ",                                               # whitespace only
    "\U0010FFFF x\U0001F600y \U0010FFFF\U0010FFFF\U0010FFFF\U0010FFFF",    # the largest code point and a non-BMP one
    "Hello  World\tfoo\nBAR  a b",
    "한국어 검색 엔진 의 검색",
    "İstanbul ΑΣ Straße",                                    # lower() changes the length; final sigma
    "the cat and the hat and the bat",
    "x",
    "a a a a a a a a",                                       # the blank between two words counts for both
]
QUERIES = ["the cat", "zzz qqq", "", "a", "검색", "HELLO world", "\U0010FFFF", "ψψ", "hat  bat\tthe", " \n"]
RANGES = [(1, 1), (2, 3), (3, 3), (1, 3)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g17():
    return R.load_g17(G17)


def _ulps32(a, b) -> int:
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.size == 0:
        return 0
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _split(cnt, *flat):
    ptr = np.concatenate([[0], np.cumsum(cnt.cpu().numpy())])
    host = [x.cpu().numpy() for x in flat]
    return [tuple(h[ptr[i]:ptr[i + 1]] for h in host) for i in range(len(ptr) - 1)]


def _check_counts(texts, ngram_range, dev):
    from snx.retrieval import row_counts, word_rows
    cnt, keys, counts = row_counts(*word_rows(texts), ngram_range, dev)
    assert cnt.dtype == torch.long and keys.dtype == torch.long and counts.dtype == torch.int32
    rows = _split(cnt, keys, counts)
    assert len(rows) == len(texts)
    for t, (k, c) in zip(texts, rows):
        rk, rc = R.row_counts(t, ngram_range)
        assert np.array_equal(k, rk) and np.array_equal(c, rc), (t[:40], ngram_range)
    return cnt, keys, counts


def _check_rows(texts, triple, model, ngram_range, sublinear=True):
    cnt, fid, w = triple
    assert cnt.dtype == torch.long and fid.dtype == torch.int32 and w.dtype == torch.float32
    rows = _split(cnt, fid, w)
    assert len(rows) == len(texts)
    for t, (f, x) in zip(texts, rows):
        rf, rw = R.transform_row(t, model, ngram_range, sublinear)
        assert np.array_equal(f, rf), (t[:40], ngram_range)
        assert (x > 0).all() and _ulps32(x, rw.astype(np.float32)) <= 1, (t[:40], ngram_range)


def _check_index(tf, corpus, ngram_range, max_features, sublinear=True):
    m = R.fit(corpus, ngram_range, max_features)
    assert np.array_equal(tf.feature_keys.cpu().numpy(), m["keys"])
    assert np.array_equal(tf.doc_freq.cpu().numpy(), m["doc_freq"]) and tf.doc_freq.dtype == torch.int32
    assert np.array_equal(tf.total_count.cpu().numpy(), m["total"])
    assert tf.idf.dtype == torch.float64 and np.array_equal(tf.idf.cpu().numpy(), m["idf"])      # bit-equal
    assert tf.feature_ngrams() == [R.key_ngram(k) for k in m["keys"].tolist()]
    _check_rows(corpus, tf.doc_rows(), m, ngram_range, sublinear)
    return m


def _check_search(tf, m, corpus, queries, k, ngram_range):
    """The hits against float64 cosines of the restatement's rows, within (nnz_q + 2) * 2^-24."""
    scores, docs, _, _ = tf.search_texts(queries, k)
    scores, docs = scores.cpu().numpy(), docs.cpu().numpy()
    F = max(m["keys"].size, 1)
    dense = lambda rows: np.stack([np.bincount(f, weights=w, minlength=F) for f, w in rows]) if rows else np.zeros((0, F))
    qr = R.transform(queries, m, ngram_range)
    cos = dense(qr) @ dense(R.transform(corpus, m, ngram_range)).T
    for q in range(len(queries)):
        tol = R.mining_tolerance(len(qr[q][0]))
        n = int((docs[q] >= 0).sum())
        assert n == min(k, int((cos[q] > 0).sum())) and (docs[q, n:] == -1).all() and (scores[q, n:] == 0).all()
        d, s = docs[q, :n], scores[q, :n]
        assert len(set(d.tolist())) == n and (s > 0).all()
        assert (np.abs(s.astype(np.float64) - cos[q, d]) <= tol).all()
        assert all(s[i] > s[i + 1] or (s[i] == s[i + 1] and d[i] < d[i + 1]) for i in range(n - 1))
        rest = np.setdiff1d(np.arange(len(corpus)), d)
        if n == k and rest.size:
            assert cos[q, rest].max() <= float(s[-1]) + tol


# ------------------------------------------------------------------------------------------------ 1. row counts
@pytest.mark.parametrize("ngram_range", RANGES)
def test_row_counts_edge_rows(dev, ngram_range):
    cnt, _, _ = _check_counts(EDGE + QUERIES, ngram_range, dev)
    assert cnt[3] == 0 and cnt[4] == 0                       # the empty and the whitespace-only row


def test_row_counts_at_and_beyond_the_lds_capacity(dev):
    """A row exactly at the LDS form's capacity, one code point beyond it, and one beyond it by a factor of three: the
    workspace form gives what the LDS form gives."""
    from snx.retrieval import lds_row_capacity, row_counts, word_rows
    rng = np.random.default_rng(5)
    cap = lds_row_capacity((2, 3))
    assert cap == 2046

    def text(n):
        words, left = [], n
        while left > 0:
            L = min(left, int(rng.integers(1, 9)))
            words.append("".join(rng.choice(list("abc한\U0001F600"), L)))
            left -= L + 1
        t = " ".join(words)
        return t if len(t) == n else t + "d" * (n - len(t))
    texts = ["short one", text(cap), text(cap + 1), "", text(3 * cap + 7), text(cap - 1), "aa"]
    assert [len(" ".join(t.split())) for t in texts[1:6]] == [cap, cap + 1, 0, 3 * cap + 7, cap - 1]
    a = _check_counts(texts, (2, 3), dev)
    b = row_counts(*word_rows(texts), (2, 3), dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))     # two runs, the same bits
    _check_counts([text(3 * lds_row_capacity((1, 3)) + 1), text(lds_row_capacity((1, 3))), "a b"], (1, 3), dev)
    # one long row of a single repeated word: every run is long
    _check_counts(["ab " * 3000], (2, 3), dev)


# ------------------------------------------------------------------------------------------------ 2. fit and transform
@pytest.mark.parametrize("ngram_range", RANGES)
@pytest.mark.parametrize("sublinear", [True, False])
def test_index_against_the_restatement(dev, ngram_range, sublinear):
    from snx.retrieval import TfidfIndex
    tf = TfidfIndex(dev, ngram_range=ngram_range, max_features=None, sublinear_tf=sublinear)
    tf.fit_add(EDGE[:5])
    tf.fit_add(EDGE[5:])                                     # two batches are one corpus
    tf.build()
    m = _check_index(tf, EDGE, ngram_range, None, sublinear)
    triple = tf.query_rows(QUERIES)
    _check_rows(QUERIES, triple, m, ngram_range, sublinear)
    unknown = ngram_range[0] >= 2                            # from 1-grams on, "zzz qqq" holds the blank every word holds
    assert triple[0][2] == 0 and triple[0][9] == 0 and (triple[0][1] == 0) == unknown    # empty; blank; unknown n-grams
    again = tf.query_rows(QUERIES)
    assert all(torch.equal(x, y) for x, y in zip(triple, again))             # two runs, the same bits
    if sublinear:
        _check_search(tf, m, EDGE, QUERIES, 4, ngram_range)
        scores, docs, rank, tscore = tf.search_texts(QUERIES, 3, targets=torch.zeros(len(QUERIES), dtype=torch.int32,
                                                                                      device=dev))
        if unknown:
            assert (docs[1] == -1).all() and (scores[1] == 0).all() and int(rank[1]) == 0    # no known n-gram: no hit
        assert (docs[2] == -1).all() and rank.shape == (len(QUERIES),) and tscore.dtype == torch.float32


def test_max_features_above_equal_and_below_the_distinct_keys(dev):
    from snx.retrieval import TfidfIndex
    distinct = R.fit(EDGE, (2, 3), None)["distinct"]
    for mf in (distinct + 5, distinct, distinct - 1, distinct // 2, 3, 1):
        tf = TfidfIndex(dev, max_features=mf)
        tf.fit_add(EDGE)
        m = _check_index(tf.build(), EDGE, (2, 3), mf)
        assert m["keys"].size == min(mf, distinct) == tf.index.V
        _check_rows(QUERIES, tf.query_rows(QUERIES), m, (2, 3))
    # the tie rule at the cut on the device: b, c and d once each, the cut through them keeps the lowest keys
    tf = TfidfIndex(dev, ngram_range=(1, 1), max_features=4)
    tf.fit_add(["b c d a a a"])
    assert tf.build().feature_ngrams() == [" ", "a", "b", "c"] and tf.total_count.tolist() == [12, 3, 1, 1]


def test_tiny_corpora_and_a_feature_in_every_document(dev):
    from snx.retrieval import TfidfIndex
    for corpus in (["the cat sat"], ["the cat sat", "the dog"], ["the cat", "the hat", "the bat"]):
        tf = TfidfIndex(dev)
        tf.fit_add(corpus)
        m = _check_index(tf.build(), corpus, (2, 3), 30000)
        assert (m["doc_freq"] == len(corpus)).any()          # idf = log(1) + 1 = 1 exactly
        assert (tf.idf[tf.doc_freq == len(corpus)] == 1.0).all()
        _check_search(tf, m, corpus, ["the", "cat", "dog hat", "zzz"], 2, (2, 3))
    with pytest.raises(ValueError):
        TfidfIndex(dev, ngram_range=(2, 4))
    with pytest.raises(ValueError):
        TfidfIndex(dev, max_features=0)
    with pytest.raises(RuntimeError):
        TfidfIndex(dev).query_rows(["a"])


def test_c_interface_refuses_bad_shapes(dev):
    from snx._lib import fn
    assert fn("snx_tfidf_row_counts")(None, None, 1, 1, 0, 2, None, None, None, None, 0, None) == -2
    assert fn("snx_tfidf_row_counts")(None, None, 1, 1, 2, 4, None, None, None, None, 0, None) == -2
    assert fn("snx_tfidf_row_counts")(None, None, 1, 1, 3, 2, None, None, None, None, 0, None) == -2
    assert fn("snx_tfidf_row_counts")(None, None, 1, 1, 2, 3, None, None, None, None, 0, None) == -3
    assert fn("snx_tfidf_counts_workspace_bytes")(2046, 2, 3) == 0
    assert fn("snx_tfidf_counts_workspace_bytes")(2047, 2, 3) == 64 * 8192 * 8
    assert fn("snx_tfidf_weights")(None, None, None, 1, None, None, 0, None, 0, None, None, None, None) == -2


# ------------------------------------------------------------------------------------------------ 3. g17 end to end
@pytest.fixture(scope="module")
def g17_index(dev, g17):
    from snx.retrieval import TfidfIndex
    tf = TfidfIndex(dev, ngram_range=(2, 3), max_features=g17["max_features"], sublinear_tf=True)
    tf.fit_add(g17["corpus"])
    return tf.build()


def test_g17_features_idf_and_weights(g17, g17_index):
    a, tf = g17["arrays"], g17_index
    assert tf.feature_ngrams() == g17["features"]
    assert np.array_equal(tf.idf.cpu().numpy(), a["idf"])    # bit-equal
    cnt, fid, w = tf.doc_rows()
    assert np.array_equal(np.concatenate([[0], np.cumsum(cnt.cpu().numpy())]), a["corpus_indptr"])
    assert np.array_equal(fid.cpu().numpy(), a["corpus_indices"])
    assert _ulps32(w.cpu().numpy(), a["corpus_data"].astype(np.float32)) <= 1


def test_g17_scores_within_the_fmaf_bound(g17, g17_index):
    from src.train.mining.tfidf import read_records
    a = g17["arrays"]
    recs = [read_records(f) for f in g17["input_files"]]
    queries = [recs[s][i].get("query", "") for s, i in g17["need"]]
    cnt, _, _ = g17_index.query_rows(queries)
    assert np.array_equal(cnt.cpu().numpy(), a["nnz_q"])
    scores, docs, _, _ = g17_index.search_texts(queries, g17["top_k"])
    scores, docs = scores.cpu().numpy().astype(np.float64), docs.cpu().numpy()
    worst = 0.0
    for r in range(len(queries)):
        live = docs[r] >= 0
        assert int(live.sum()) == min(g17["top_k"], int((a["scores"][r] > 0).sum()))
        gap = np.abs(scores[r, live] - a["scores"][r, docs[r, live]])
        worst = max(worst, float(gap.max()) if gap.size else 0.0)
        assert (gap <= R.mining_tolerance(a["nnz_q"][r])).all(), (r, gap.max())
    print(f"g17: largest |fp32 score - float64 score| = {worst:.3e}")


def test_g17_mining_output_and_cli(dev, g17, tmp_path, capsys):
    from snx.retrieval import TfidfIndex
    from src.train.cli import mine_tfidf_negatives as cli
    from src.train.mining.tfidf import collect_shard_files, mine_tfidf_negatives
    src = tmp_path / "in"
    shutil.copytree(os.path.join(G17, "input"), src)
    files = collect_shard_files(str(src))
    tf = TfidfIndex(dev, max_features=g17["max_features"])
    out = mine_tfidf_negatives(files, tf, output_dir=str(tmp_path / "out"), max_corpus=g17["max_corpus"],
                               top_k=g17["top_k"], batch_size=g17["batch_size"], fit_batch=128)
    seen = R.check_mining_output(g17, str(tmp_path / "out"), out["shards"])
    assert out["failed"] == seen["zero"] == 5 and out["corpus"] == g17["max_corpus"]
    capsys.readouterr()
    summary = cli.main(["--data-dir", str(src), "--output-dir", str(tmp_path / "cli"), "--max-corpus", str(g17["max_corpus"]),
                        "--max-features", str(g17["max_features"]), "--top-k", str(g17["top_k"]), "--device", str(dev)])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == summary and summary["features"] == g17["max_features"]
    assert {k: summary[k] for k in ("total", "already_had_negative", "added", "failed")} == \
        {k: out[k] for k in ("total", "already_had_negative", "added", "failed")}
    for n in g17["shards"]:                                  # the batch size changes nothing
        assert open(tmp_path / "cli" / n, "rb").read() == open(tmp_path / "out" / n, "rb").read()
