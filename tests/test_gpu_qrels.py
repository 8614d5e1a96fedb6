"""GPU checks of scoring against qrels (csrc/qrels.hip, include/snx.h "relevance judgments") against the numpy
restatement tests/qrels_reference.py, which the host suite (test_qrels_host.py) holds to the reference project's own
outputs (tests/golden/g14_qrels.json).  Integers and fp32 / float64 bits are compared exactly; the only bound is the
bootstrap intervals' n * 2^-52 against the reference's recorded intervals, derived in test_qrels_host.interval_bound.

"The tolerance tests/test_gpu_hybrid.py uses for g13" is exact equality (it compares the g13 values by their hex
images), so the first-relevant metrics over g14's lists are compared to the recorded values with ==."""
import json
import os

import numpy as np
import pytest
import torch

from tests import qrels_reference as Q
from tests.test_gpu_retrieval import _index, _long_query_corpus, _to_device
from tests.test_qrels_host import GOLDEN_DIR, OURS, REPORT, golden_qrels, interval_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(a):
    a = np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _int_rows(rng, n, V, max_nnz, top=3):
    """Rows with small-integer weights 1 .. top over terms [0, V): equal scores are certain."""
    out = []
    for _ in range(n):
        t = np.sort(rng.choice(V, size=int(rng.integers(1, max_nnz + 1)), replace=False))
        out.append((t, rng.integers(1, top + 1, len(t)).astype(np.float64)))
    return out


V, ND, NQ = 64, 3000, 40
LONELY = V - 1                                     # a term no query holds: docs with only this term score 0 everywhere


@pytest.fixture(scope="module")
def corpus(dev):
    from snx.retrieval import SparseIndex
    rng = np.random.default_rng(14)
    docs = _int_rows(rng, ND, V - 1, 6)
    queries = _int_rows(rng, NQ, V - 1, 5)
    docs[1000] = docs[2000] = docs[10]             # three equal rows: equal scores for every query, ids on both sides
    docs[40] = docs[41] = docs[2999] = (np.array([LONELY]), np.array([2.0]))
    queries[5] = (np.zeros(0, np.int64), np.zeros(0))                         # a query without terms
    queries[0] = (docs[10][0][:1], np.array([3.0]))                           # certainly matches the equal rows
    queries[7] = (docs[10][0][:1], np.array([2.0]))
    relevant = [sorted(rng.choice(ND, int(rng.integers(1, 7)), replace=False).tolist()) for _ in range(NQ)]
    relevant[0] = [1000]                           # equal score: non-relevant doc 10 in front, non-relevant 2000 behind
    relevant[1] = [40, 41, 2999]                   # every relevant doc scores 0
    relevant[2] = []
    relevant[3] = [-2, 17, 1500, ND, ND + 5]       # ids outside [0, nd)
    relevant[4] = sorted(rng.choice(ND, 400, replace=False).tolist())
    relevant[5] = [3, 4]                           # the empty query: nothing scores
    relevant[6] = sorted(rng.choice(ND, 300, replace=False).tolist() + [ND + 1])
    relevant[7] = [10, 1000, 2000]                 # all three equal rows relevant: the lowest id is the best
    # Planted hits, so that the ranked lists certainly hold relevant docs: a doc with every term of query qi at the top
    # weight 3 reaches the highest score any doc can have for qi (3 * the sum of the query's weights), so it is in
    # front of every doc that does not tie with it.  One such relevant doc for each query from 8 on, three for query 4.
    for qi in range(8, NQ):
        docs[100 + qi] = (queries[qi][0], np.full(len(queries[qi][0]), 3.0))
        relevant[qi] = sorted(set(relevant[qi]) | {100 + qi})
    for d in (200, 201, 202):
        docs[d] = (queries[4][0], np.full(len(queries[4][0]), 3.0))
    relevant[4] = sorted(set(relevant[4]) | {200, 201, 202})
    idx = SparseIndex(V, dev)
    for s in range(0, ND, 1024):
        idx.add(*_to_device(docs[s:s + 1024], dev))
    idx.build()
    S = Q.scores(queries, docs, V)
    return idx, _to_device(queries, dev, np.random.default_rng(1)), relevant, S, docs, queries


# ------------------------------------------------------------------------------------------------ first relevant
def test_first_relevant_equals_the_reference_and_the_single_target_minimum(dev, corpus):
    idx, q, relevant, S, _, _ = corpus
    assert S[0, 10] == S[0, 1000] == S[0, 2000] > 0 and (S[1, [40, 41, 2999]] == 0).all() and (S[5] == 0).all()
    assert len(np.unique(S[4][S[4] > 0])) < 40                                 # ties everywhere
    want = Q.first_relevant(S, relevant)
    got = [x.cpu().numpy() for x in idx.first_relevant(*q, relevant)]
    assert [g.dtype for g in got] == [np.int32, np.float32, np.int32, np.int32]
    for name, g, w in zip(("doc", "score", "rank", "nrel"), got, want):
        assert np.array_equal(_bits(g), _bits(w)), name
    doc, score, rank, nrel = got
    assert doc[0] == 1000 and rank[0] == 1 + int((S[0] > S[0, 1000]).sum()) + int((S[0, :1000] == S[0, 1000]).sum())
    assert rank[0] >= 2                                                        # doc 10 ties and comes first
    assert doc[1] == -1 and rank[1] == 0 and score[1] == 0 and nrel[1] == 3
    assert doc[2] == -1 and rank[2] == 0 and nrel[2] == 0
    assert nrel[3] == 2 and doc[3] in (17, 1500, -1)
    assert nrel[4] == len(relevant[4]) >= 400 and nrel[6] == 300 and rank[4] == 1
    assert doc[5] == -1 and rank[5] == 0 and nrel[5] == 2
    assert doc[7] == 10
    # the minimum over each row of the single-target rank of the exact search, on the same index
    width = max(len(r) for r in relevant)
    best = np.zeros(NQ, np.int64)
    for j in range(width):
        tgt = np.asarray([r[j] if j < len(r) and 0 <= r[j] < ND else 0 for r in relevant], np.int32)
        live = np.asarray([j < len(r) and 0 <= r[j] < ND for r in relevant])
        _, _, rk, ts = idx.search(*q, 1, targets=torch.from_numpy(tgt).to(dev))
        rk, ts = rk.cpu().numpy().astype(np.int64), ts.cpu().numpy()
        use = live & (rk > 0)
        best = np.where(use & ((best == 0) | (rk < best)), rk, best)
        hit = live & (tgt == doc)
        assert np.array_equal(_bits(ts[hit]), _bits(score[hit]))               # bit-equal to what the search ranks
    assert np.array_equal(best, rank.astype(np.int64))
    # independent of chunk_docs
    for chunk in (37, 1000, 32768):
        again = [x.cpu().numpy() for x in idx.first_relevant(*q, relevant, chunk_docs=chunk)]
        for g, a in zip(got, again):
            assert np.array_equal(_bits(g), _bits(a)), chunk
    # the CSR form of the rows gives the same
    from snx.retrieval import relevance_csr
    pair = relevance_csr(relevant, NQ, ND, dev)
    for g, a in zip(got, idx.first_relevant(*q, pair)):
        assert np.array_equal(_bits(g), _bits(a.cpu().numpy()))
    with pytest.raises(ValueError):
        idx.first_relevant(*q, relevant, chunk_docs=32769)
    with pytest.raises(ValueError):
        idx.first_relevant(*q, relevant[:-1])


def test_first_relevant_with_a_query_longer_than_one_staging_group(dev):
    docs, queries, V = _long_query_corpus()                 # 300 terms in query 0, query 1 empty
    idx = _index(docs, V, dev)
    S = Q.scores(queries, docs, V)
    relevant = [[0, 5, 120, 299], [4], list(range(0, 300, 3))]                # doc 0 is empty
    want = Q.first_relevant(S, relevant)
    got = [x.cpu().numpy() for x in idx.first_relevant(*_to_device(queries, dev), relevant, chunk_docs=128)]
    for name, g, w in zip(("doc", "score", "rank", "nrel"), got, want):
        assert np.array_equal(_bits(g), _bits(w)), name
    assert got[2][0] > 0 and got[2][1] == 0


def test_first_rank_in_a_list_is_the_whole_corpus_rank_when_it_fits(dev, corpus):
    from snx.retrieval import ranked_relevance
    idx, q, relevant, _, _, _ = corpus
    _, _, rank, _ = idx.first_relevant(*q, relevant)
    for k in (10, 100):
        first = ranked_relevance(idx.search(*q, k)[1], relevant, ND, (1, 5, 10))[0]
        want = torch.where(rank <= k, rank, torch.zeros_like(rank))
        assert torch.equal(first, want), k


# ------------------------------------------------------------------------------------------------ ranked lists
def _check_ranked(docs, relevant, nd, cutoffs):
    from snx.retrieval import ranked_relevance
    first, hits, dcg = ranked_relevance(docs, relevant, nd, cutoffs)
    w_first, w_hits, w_dcg = Q.ranked_relevance(docs.cpu().numpy(), relevant, nd, cutoffs)
    assert first.dtype == hits.dtype == torch.int32 and dcg.dtype == torch.float64
    assert np.array_equal(first.cpu().numpy(), w_first)
    assert np.array_equal(hits.cpu().numpy(), w_hits)
    assert np.array_equal(_bits(dcg.cpu().numpy()), _bits(w_dcg))
    return first.cpu().numpy(), hits.cpu().numpy(), dcg.cpu().numpy()


def test_ranked_relevance_on_search_fusion_and_seismic_outputs(dev, corpus):
    from snx.retrieval import SeismicIndex, SparseIndex, fuse_ranked
    idx, q, relevant, _, docs, _ = corpus
    s100, d100, _, _ = idx.search(*q, 100)
    first, hits, _ = _check_ranked(d100, relevant, ND, (1, 5, 10))
    assert (first[8:] > 0).all() and int(hits[4, 1]) >= 3                      # the planted docs (see the fixture)
    _check_ranked(d100, relevant, ND, (3, 50, 100))
    _check_ranked(d100, relevant, ND, (100,))
    _check_ranked(d100, relevant, ND, (1, 2, 3, 4, 5, 6, 7, 8))
    # a second retriever over halved doc rows, fused with the first
    other = SparseIndex(V, dev)
    other.add(*_to_device([(t[::2], w[::2]) for t, w in docs], dev))
    other.build()
    s2, d2, _, _ = other.search(*q, 100)
    fused = fuse_ranked([(d100, s100), (d2, s2)], "rrf", 50, k=60)[1]
    _check_ranked(fused, relevant, ND, (1, 5, 10, 50))
    seis = SeismicIndex(idx, n_postings=200, cluster_ratio=0.2, summary_prune_ratio=0.5).search(*q, 10)[1]
    _check_ranked(seis, relevant, ND, (1, 5, 10))
    _check_ranked(idx.search_two_phase(*q, 10)[1], relevant, ND, (1, 5, 10))


def test_ranked_relevance_list_ends_long_lists_and_repeats(dev):
    rng = np.random.default_rng(7)
    nq, R, nd = 200, 4096, 6000
    docs = np.stack([rng.permutation(nd)[:R] for _ in range(nq)]).astype(np.int32)
    for i in range(nq):                                                        # ragged ends, entries behind the end
        if i % 3 == 0:
            docs[i, int(rng.integers(0, R)):] = -1
        if i % 5 == 0:
            docs[i, int(rng.integers(0, R))] = -1                              # what follows is not part of the list
        if i % 7 == 0:
            docs[i, 70] = docs[i, 2]                                           # a repeated id counts at every position
        if i % 11 == 0:
            docs[i, 5] = nd + 3                                                # outside the corpus: never relevant
    relevant = [sorted(rng.choice(nd + 10, int(rng.integers(0, 600)), replace=False).tolist()) for _ in range(nq)]
    relevant[0] = []
    relevant[7] = docs[7, [2, 64, 127, 128, 4095]].tolist()
    d = torch.from_numpy(docs).to(dev)
    _check_ranked(d, relevant, nd, (1, 5, 10, 64, 65, 1000, 4095, 4096))
    _check_ranked(d, relevant, nd, (10,))
    _check_ranked(d[:, :1].contiguous(), relevant, nd, (1,))
    _check_ranked(d[:, :63].contiguous(), relevant, nd, (1, 63))
    from snx.retrieval import ranked_relevance
    for bad in ((0, 5), (5, 5), (10, 5), (1, 4097), (), tuple(range(1, 10)), (1.0,)):
        with pytest.raises(ValueError):
            ranked_relevance(d, relevant, nd, bad)
    with pytest.raises(ValueError):
        ranked_relevance(torch.zeros((2, 4097), dtype=torch.int32, device=dev), [[], []], nd)


def test_first_relevant_metrics_over_the_golden_lists_equal_the_recorded_values(dev):
    from snx.retrieval import ranked_relevance
    from src.train.eval import qrels_metrics
    g = golden_qrels()
    nd = g["num_docs"]
    nrel = [sum(1 for d in r if 0 <= d < nd) for r in g["relevant"]]
    for name, m in g["methods"].items():
        lists = torch.tensor(m["lists"], dtype=torch.int32, device=dev)
        first, hits, dcg = ranked_relevance(lists, g["relevant"], nd, (1, 5, 10))
        assert first.cpu().tolist() == m["hit_ranks"], name
        out = qrels_metrics(first, hits, dcg, nrel, (1, 5, 10))
        for ours, ref in zip(OURS, REPORT):
            print(name, ours, out[ours], float.fromhex(m["metrics"][ref]))
            assert out[ours] == float.fromhex(m["metrics"][ref]), (name, ours)


# ------------------------------------------------------------------------------------------------ bootstrap
def test_bootstrap_means_are_the_fixed_order_bit_for_bit(dev):
    from snx.retrieval import bootstrap_indices, bootstrap_means
    rng = np.random.default_rng(5)
    for n, M, nb in ((1, 1, 3), (63, 2, 50), (64, 16, 50), (65, 3, 50), (1000, 5, 200), (20000, 4, 6)):
        v = rng.random((n, M))
        v[:, 0] = rng.integers(0, 2, n)
        idx = bootstrap_indices(n, nb, 42)
        got = bootstrap_means(v, n_bootstrap=nb, seed=42, device=dev)
        assert got.dtype == torch.float64 and tuple(got.shape) == (nb, M)
        want = Q.bootstrap_means(v, idx)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (n, M)
        again = bootstrap_means(torch.from_numpy(v).to(dev), indices=idx)
        assert torch.equal(got, again)                                         # and from run to run
    one = bootstrap_means(rng.random(100), n_bootstrap=10, device=dev)
    assert tuple(one.shape) == (10, 1)


def test_bootstrap_intervals_equal_the_reference_within_the_derived_bound(dev):
    from src.train.eval import bootstrap_confidence_interval, first_relevant_values
    g = golden_qrels()
    for name, m in g["methods"].items():
        vals = first_relevant_values(m["hit_ranks"], k=10)
        n = vals.shape[0]
        assert 0.0 <= vals.min() and vals.max() <= 1.0
        bound = interval_bound(n)                                              # n * 2^-52, from n
        got = bootstrap_confidence_interval(vals[:, [0, 3, 4]], n_bootstrap=g["n_bootstrap"], confidence=g["confidence"],
                                            seed=g["seed"], device=dev)
        for ci, key in zip(got, ("recall@1", "mrr", "ndcg@10")):
            for x in ("point_estimate", "lower", "upper"):
                want = float.fromhex(m["ci"][key][x])
                print(name, key, x, ci[x], want, abs(ci[x] - want), bound)
                assert abs(ci[x] - want) <= bound, (name, key, x)
        single = bootstrap_confidence_interval(vals[:, 3], device=dev)
        assert single == got[1]


# ------------------------------------------------------------------------------------------------ CLI
def test_eval_benchmark_cli_end_to_end(dev, tmp_path, capsys):
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.cli import eval_benchmark as E
    from src.train.cli.mine_negatives import load_model
    from src.train.data.collator import create_tokenizer
    from src.train.eval import BenchmarkEvaluator, first_relevant_values, load_benchmark_dir
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(dict(
        vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
        local_attention=16, pad_token_id=999)))
    torch.manual_seed(5)
    (tmp_path / "ckpt").mkdir()
    torch.save(SPLADEModernBERT(model_name=str(mdir)).state_dict(), tmp_path / "ckpt" / "model.pt")
    argv = ["--checkpoint", str(tmp_path / "ckpt" / "model.pt"), "--model-name", str(mdir), "--tokenizer", "hash:1000",
            "--benchmark-dir", GOLDEN_DIR, "--query-max-length", "16", "--doc-max-length", "32", "--batch-size", "8",
            "--bootstrap", "100", "--report", str(tmp_path / "report.json")]
    lines = E.main(argv)
    printed = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert printed == json.loads(json.dumps(lines))
    rows = [x for x in lines if "method" in x]
    tests = [x for x in lines if "test" in x]
    assert [x["method"] for x in rows] == list(E.METHODS) and len(tests) == 10
    assert tests[0]["test"] == "sparse_vs_bm25" and tests[-1]["test"] == "two_phase_vs_seismic"
    assert all(set(t) == {"test", "statistic", "p_value", "significant"} for t in tests)
    keys = {"method", "num_docs", "top_k", "num_queries", "wall_s", "ci", *OURS,
            *(f"{a}@{c}" for a in ("recall_frac", "ndcg_multi") for c in (1, 5, 10))}
    for x in rows:
        assert set(x) == keys | ({"first_relevant"} if x["method"] == "sparse" else set()), x["method"]
        assert x["num_queries"] == 7 and x["num_docs"] == 12 and x["top_k"] == 10 and x["wall_s"] > 0
        assert set(x["ci"]) == {"recall@1", "mrr", "ndcg@10"}
        for key, ci in x["ci"].items():
            assert set(ci) == {"point_estimate", "lower", "upper"}
            assert ci["lower"] <= ci["point_estimate"] <= ci["upper"] and abs(ci["point_estimate"] - x[key]) < 1e-12
        assert 0 <= x["recall@1"] <= x["recall@5"] <= x["recall@10"] <= 6 / 7   # q5's relevant doc is not in the corpus
    report = json.load(open(tmp_path / "report.json"))["metrics"]
    assert list(report) == list(E.METHODS)
    for x in rows:
        assert report[x["method"]] == {**{r: x[o] for o, r in zip(OURS, REPORT)}, "num_queries": 7}
    assert rows[1]["recall@10"] > 0                                            # BM25 finds docs on lexical overlap
    # the sparse line's mrr, recomputed from first_relevant over the same encoding
    args = E.parse_args(argv)
    data = load_benchmark_dir(GOLDEN_DIR)
    ev = BenchmarkEvaluator(create_tokenizer("hash:1000"), data, device=str(dev), query_max_length=16, doc_max_length=32,
                            batch_size=8)
    index, queries = ev.encode(load_model(args, dev))
    _, _, rank, nrel = index.first_relevant(*queries, data.relevant)
    assert nrel.cpu().tolist() == [1, 2, 1, 1, 0, 1, 1]
    assert rows[0]["mrr"] == float(np.mean(first_relevant_values(rank, k=10)[:, 3]))
    r = rank.cpu().numpy()
    assert rows[0]["first_relevant"]["found"] == int((r > 0).sum())
    assert rows[0]["first_relevant"]["mrr_full"] >= rows[0]["mrr"]
    few = E.main(argv[:-4] + ["--methods", "bm25,sparse", "--bootstrap", "0", "--max-queries", "3"])
    assert [x.get("method", x.get("test")) for x in few] == ["bm25", "sparse", "bm25_vs_sparse"]
    assert all("ci" not in x for x in few) and few[0]["num_queries"] == 3
