"""GPU checks of the term-expansion evaluation (csrc/expansion.hip, include/snx.h "term-expansion evaluation") against the
restatement tests/expansion_reference.py, which the host suite (test_expansion_host.py) holds to the reference project's
own outputs (tests/golden/g20_expansion).  Everything is equality: positions, counts and the bits of the float64 folds --
the device only counts and adds table entries.  The one bound is the bootstrap interval's n * 2^-52 of
tests/test_gpu_qrels.py::test_bootstrap_intervals_equal_the_reference_within_the_derived_bound (`bound =
interval_bound(n)`, tests/test_qrels_host.interval_bound), which holds for values in [-1, 1] as it does for [0, 1]."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import expansion_reference as R
from tests.test_expansion_host import dec, golden, golden_rows
from tests.test_qrels_host import interval_bound

pytestmark = pytest.mark.gpu
NAMES = ("rank", "nranked", "first", "hits", "dcg")
DTYPES = [np.int32, np.int32, np.int32, np.int32, np.float64]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(a):
    a = np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def run(dev, case, max_k, cuts, slices=0):
    from snx.expansion import graded_metrics
    rep, ex, ptr, tok, grade, rel = case
    out = graded_metrics(torch.from_numpy(rep).to(dev), torch.from_numpy(ex).to(dev), (ptr, tok, grade, rel), cuts,
                         max_k=max_k, slices=slices)
    return [x.cpu().numpy() for x in out]


def check(dev, case, max_k, cuts, slices=(0, 1, 2, 7)):
    want = R.metrics(*case, max_k, list(cuts))
    for s in slices:
        got = run(dev, case, max_k, cuts, s)
        assert [g.dtype for g in got] == DTYPES
        for name, g, w in zip(NAMES, got, want):
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (name, s, max_k, cuts)
    return want


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("width", [1, 3, 63, 64, 65, 257, 1027, 4100])
def test_every_width_three_misaligned_rows_every_slicing(dev, width):
    case = R.grid_case(np.random.default_rng(width), 3, width, [5, 0, 9])
    check(dev, case, 5, (1, 3, 5, 8))


@pytest.mark.parametrize("B", [1, 70])
def test_batch_sizes(dev, B):
    for width in (65, 1027):
        case = R.grid_case(np.random.default_rng(B + width), B, width, [3, 10, 1, 0])
        check(dev, case, 20, (5, 10, 20), slices=(0, 2))


def test_judgments_per_row_straddle_the_lds_chunk(dev):
    rng = np.random.default_rng(64)
    case = R.grid_case(rng, 7, 1027, [0, 1, 2, 63, 64, 65, 200], top=30)
    assert np.diff(case[2]).tolist() == [0, 1, 2, 63, 64, 65, 200]
    check(dev, case, 100, (5, 10, 20, 50, 100))
    want = check(dev, case, 1027, (5, 10, 100, 500, 1027))                     # uncut lists: long folds in the finalize
    assert (want[0] > 0).sum() > 200 and (want[3][:, -1] > 60).any()
    none = (case[0], case[1], np.zeros(8, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    want = check(dev, none, 100, (5, 10))
    assert want[0].shape == (0,) and (want[1] > 0).all() and not want[2].any() and not want[4].any()


@pytest.mark.parametrize("max_k", [1, 5, 100, 257, 264])
def test_max_k(dev, max_k):
    case = R.grid_case(np.random.default_rng(max_k), 3, 257, [40, 7, 12], top=9)
    want = check(dev, case, max_k, (5, 10, 300), slices=(0, 3))
    assert want[0].max() <= max_k and want[1].max() <= min(max_k, 257)


@pytest.mark.parametrize("cuts", [(7,), (1, 2, 3, 5, 8, 13, 21, 34), (2, 10, 1000)])
def test_cutoffs_one_eight_and_above_max_k(dev, cuts):
    case = R.grid_case(np.random.default_rng(len(cuts)), 4, 300, [30, 2, 0, 64], top=12)
    want = check(dev, case, 10, cuts, slices=(0, 2))
    if cuts[-1] > 10:                                                          # above max_k: the whole cut list
        at10 = R.metrics(*case, 10, [10])
        assert np.array_equal(want[3][:, -1], at10[3][:, 0]) and np.array_equal(_bits(want[4][:, -1]), _bits(at10[4][:, 0]))


def test_full_width_once(dev):
    rng = np.random.default_rng(50368)
    rep = np.zeros((2, 50368), np.float32)
    for b in range(2):
        on = rng.choice(50368, 300, replace=False)
        rep[b, on] = rng.integers(1, 60, 300).astype(np.float32) / 4           # ties among the 300
    ex = np.zeros(50368, np.uint8)
    ex[:7] = 1
    on = np.nonzero(rep[0])[0]
    tok = np.concatenate([on[:6], [50367, 3, 12345], np.nonzero(rep[1])[0][:9]])
    case = (rep, ex, np.array([0, 9, 18]), tok, np.arange(18) % 4, np.ones(18, np.int64))
    want = check(dev, case, 100, (5, 10, 20, 50, 100), slices=(0, 1, 7))
    assert (want[0] > 0).sum() >= 4


def test_a_block_of_more_than_2_31_entries(dev):
    """Row offsets past 2^31 elements: only the first and the last row hold anything, and only they are judged."""
    from snx.expansion import graded_metrics
    B, width = 42700, 50368
    assert B * width > 2 ** 31
    rng = np.random.default_rng(31)
    rep = torch.zeros((B, width), device=dev)
    rows = np.zeros((2, width), np.float32)
    for r in range(2):
        on = rng.choice(width, 200, replace=False)
        rows[r, on] = rng.integers(1, 40, 200).astype(np.float32)
    rep[0] = torch.from_numpy(rows[0]).to(dev)
    rep[B - 1] = torch.from_numpy(rows[1]).to(dev)
    ex = np.zeros(width, np.uint8)
    ex[:7] = 1
    tok = np.concatenate([np.nonzero(rows[0])[0][:8], np.nonzero(rows[1])[0][:8]])
    grade, rel = np.arange(16) % 4, np.ones(16, np.int64)
    ptr = np.full(B + 1, 8, np.int64)
    ptr[0], ptr[B] = 0, 16
    got = [x.cpu().numpy() for x in graded_metrics(rep, torch.from_numpy(ex).to(dev), (ptr, tok, grade, rel), [10, 100])]
    want = R.metrics(rows, ex, np.array([0, 8, 16]), tok, grade, rel, 100, [10, 100])
    assert np.array_equal(got[0], want[0]) and (want[0][:8] > 0).any() and (want[0][8:] > 0).any()
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(_bits(g[[0, B - 1]]), _bits(w)) and not g[1:B - 1].any()


# ------------------------------------------------------------------------------------------------ value classes
def test_ties_straddle_the_cut_and_the_special_values(dev):
    width = 70
    rep = np.zeros((6, width), np.float32)
    rep[0, :] = 2.0                                            # all positive; ids 10 and 12 lead, the rest in id order
    rep[0, 10:13] = 5.0
    rep[1, :] = 0.0                                            # all zero
    rep[2, :] = -3.0                                           # negatives and -0.0
    rep[2, ::2] = np.float32(-0.0)
    rep[3, :] = 1.0
    rep[3, 20] = np.nan                                        # a NaN entry: not ranked, the others undisturbed
    rep[3, 21] = np.inf
    rep[4, [3, 30, 31, 32, 33, 60]] = [9.0, 4.0, 4.0, 4.0, 4.0, 1.0]   # a tie of four straddling max_k = 3
    rep[5, :] = 7.0                                            # every positive entry excluded below
    ex = np.zeros(width, np.uint8)
    ex[[0, 11]] = 1
    rows = [[0, 1, 10, 11, 12, 13, 69, 70, -1], [0, 5], [0, 1, 2], [19, 20, 21, 22, 0], [3, 30, 31, 32, 33, 60, 59], [1, 69]]
    ptr = np.cumsum([0] + [len(r) for r in rows])
    tok = np.array([t for r in rows for t in r])
    grade = np.array([(i % 3) + 1 for i in range(len(tok))])
    rel = np.ones(len(tok), np.int64)
    case = (rep, ex, ptr, tok, grade, rel)
    rank, nranked, first, hits, dcg = check(dev, case, 3, (1, 3), slices=(0, 1, 2, 7))
    assert rank[:9].tolist() == [0, 3, 1, 0, 2, 0, 0, 0, 0] and nranked.tolist() == [3, 0, 0, 3, 3, 3]
    assert rank[14:19].tolist() == [0, 0, 1, 0, 0]                             # inf first; NaN and the excluded id unranked
    assert rank[19:26].tolist() == [1, 2, 3, 0, 0, 0, 0]                       # the tie is cut between ids 31 and 32
    rank, nranked, *_ = check(dev, case, 70, (1, 70), slices=(0, 3))
    assert rank[:9].tolist() == [0, 3, 1, 0, 2, 12, 68, 0, 0] and nranked.tolist() == [68, 0, 0, 67, 6, 68]
    assert rank[14:19].tolist() == [19, 0, 1, 20, 0]
    all_ex = (rep, np.ones(width, np.uint8), ptr, tok, grade, rel)
    rank, nranked, first, hits, dcg = check(dev, all_ex, 70, (5,), slices=(0, 2))
    assert not rank.any() and not nranked.any() and not first.any() and not hits.any() and not dcg.any()


def test_judged_ranks_and_the_ranking_list(dev):
    from snx.expansion import judged_ranks
    from src.evaluation import RankingMetrics
    case = R.grid_case(np.random.default_rng(9), 5, 300, [12, 0, 70, 3, 1], top=20)
    rep, ex, ptr, tok, grade, rel = case
    want = R.metrics(*case, 25, [25])
    for s in (0, 1, 4):
        rank, nranked = judged_ranks(torch.from_numpy(rep).to(dev), torch.from_numpy(ex).to(dev), ptr, tok, 25, slices=s)
        assert np.array_equal(rank.cpu().numpy(), want[0]) and np.array_equal(nranked.cpu().numpy(), want[1])
    rows_a, _ = golden_rows()
    m = RankingMetrics(R.StubTokenizer())
    exm = R.excluded_mask(R.SPECIAL_IDS, R.V)
    for i in (0, 6, 7, 8):                                                     # more than, fewer than max_k positives; none
        for top_k in (None, 1, 100, 1000):
            want_ids = R.ranking(rows_a[i], exm, R.V if top_k is None else top_k)
            got = m._sparse_to_ranking(torch.from_numpy(rows_a[i]).to(dev), top_k)
            assert [t for t, _ in got] == want_ids and [w for _, w in got] == [float(rows_a[i, t]) for t in want_ids]


# ------------------------------------------------------------------------------------------------ golden
def test_g20_rows_through_graded_metrics_and_the_mirror_equal_the_golden(dev):
    from src.evaluation import EvaluationDataset, GradedRelevance, RankingMetrics
    g = golden()
    rows_a, rows_b = golden_rows()
    ds = EvaluationDataset(queries=[GradedRelevance.from_dict(q) for q in g["queries"]], name="g20")
    wide = RankingMetrics(R.StubTokenizer(), k_values=list(R.K_WIDE))
    want = dec(g["single"])
    dev_rows = torch.from_numpy(rows_a).to(dev)
    for i in range(R.NQ):
        got = wide.evaluate_single_query(dev_rows[i], ds[i], max_k=R.MAX_K)
        assert got == want[i] and list(got) == list(want[i]), i
        assert type(got["first_relevant_rank"]) is type(want[i]["first_relevant_rank"])
    assert wide.evaluate_single_query(torch.from_numpy(rows_a[8]), ds[8], max_k=R.MAX_K) == want[8]    # a host row is moved
    batch = wide._batch_metrics(dev_rows, list(ds), R.MAX_K)                   # one call over all 40 rows
    assert batch == want
    plain = RankingMetrics(R.StubTokenizer())
    for rows, name in ((rows_a, "evaluate_a"), (rows_b, "evaluate_b")):
        res = plain.evaluate(R.stub_model(rows).to(dev), ds, batch_size=R.BATCH_SIZE)
        assert res.per_query_metrics == dec(g[name]["per_query_metrics"]), name
        d = res.to_dict()
        d.pop("per_query_metrics")
        assert json.loads(json.dumps(d, default=float)) == dec(g[name]["aggregate"]), name
        assert res.num_queries == R.NQ
    # fp16 rows are cast, as the mirror documents
    assert wide._batch_metrics(dev_rows.half(), list(ds), R.MAX_K) == want     # multiples of 1/8 below 2048: exact in fp16


def test_comparison_on_the_device_path_against_the_golden(dev):
    from src.evaluation import EvaluationResult, ModelComparison
    g = golden()
    a, b = dec(g["evaluate_a"]["per_query_metrics"]), dec(g["evaluate_b"]["per_query_metrics"])
    want = dec(g["comparison"]["metrics_compared"])
    bound = interval_bound(R.NQ)                                               # n * 2^-52 (tests/test_gpu_qrels.py)
    for metric, w in want.items():
        sa, sb = [q[metric] for q in a], [q[metric] for q in b]
        assert max(abs(x - y) for x, y in zip(sa, sb)) <= 1.0
        ci = ModelComparison.bootstrap_confidence_interval(sa, sb)
        assert list(ci) == ["mean_diff", "ci_lower", "ci_upper", "confidence", "significant"]
        for key in ("mean_diff", "ci_lower", "ci_upper"):
            print(metric, key, ci[key], w["bootstrap_ci"][key], abs(ci[key] - w["bootstrap_ci"][key]), bound)
            assert abs(ci[key] - w["bootstrap_ci"][key]) <= bound, (metric, key)
        assert ci["significant"] is w["bootstrap_ci"]["significant"] and ci["confidence"] == 0.95
    cmp_ = ModelComparison.compare_models(EvaluationResult(per_query_metrics=a), EvaluationResult(per_query_metrics=b),
                                          "ckpt_a", "ckpt_b")
    assert list(cmp_.metrics_compared) == list(want) and all("error" not in v for v in cmp_.metrics_compared.values())
    assert cmp_.summary() == g["comparison"]["summary"]
    with pytest.warns(UserWarning, match="Different number of queries"):
        assert ModelComparison.compare_models(EvaluationResult(per_query_metrics=a), EvaluationResult()).metrics_compared == {}


# ------------------------------------------------------------------------------------------------ the native model
def test_native_model_rows_through_evaluate_equal_the_restatement(dev, tmp_path):
    from src.evaluation import EvaluationDataset, RankingMetrics
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.data.collator import create_tokenizer
    torch.manual_seed(5)
    model = SPLADEModernBERT(config=dict(vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2,
                                         num_attention_heads=4, local_attention=16, pad_token_id=999)).to(dev)
    tok = create_tokenizer("hash:1000")
    word_of = {}
    for i in range(20000):                                                     # a word for every id of the hash tokenizer
        word_of.setdefault(tok.encode(f"t{i}", add_special_tokens=False)[0], f"t{i}")
    sources = [f"term{i} term{i + 1}" for i in range(11)]
    m = RankingMetrics(tok, k_values=[1, 5, 20])
    ex = R.excluded_mask(sorted(m.special_token_ids), 1000)
    enc = tok(sources)
    with torch.no_grad():
        first, _ = model.eval()(enc["input_ids"].to(dev), enc["attention_mask"].to(dev))
    first = first.float().cpu().numpy()
    pairs = []
    for i, src in enumerate(sources):                                          # judged tokens placed by a first forward
        order = R.ranking(first[i], ex, 1000)
        assert len(order) > 40
        zero = [v for v in range(6, 999) if first[i, v] == 0][0]
        pairs.append({"source": src, "domain": ["legal", "medical"][i % 2],
                      "synonyms": {"exact": [word_of[order[0]], f"{word_of[order[1]]} {word_of[order[2]]}"],
                                   "partial": [word_of[order[3]], word_of[order[39]]],
                                   "related": [word_of[order[14]], word_of[zero]]}})
    ds = EvaluationDataset.from_synonym_pairs(pairs)
    seen = []

    class Recording(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, ids, mask):
            rep, tw = self.inner(ids, mask)
            seen.append(rep.detach().float().cpu().numpy())
            return rep, tw

    res = m.evaluate(Recording(model), ds, batch_size=4)
    rows = np.concatenate(seen)
    assert rows.shape == (11, 1000) and [len(s) for s in seen] == [4, 4, 3] and (rows > 0).sum() > 100
    resolve = R.resolver(tok)
    want = [R.single_query(rows[i], sorted(m.special_token_ids), resolve, ds[i].to_dict(), [1, 5, 20], 20) for i in range(11)]
    assert res.per_query_metrics == want
    assert sum(w["mrr"] > 0 for w in want) >= 6                                # the judged tokens are in the lists


def test_eval_expansion_cli_end_to_end(dev, tmp_path, capsys):
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.cli import eval_expansion as E
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(dict(
        vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
        local_attention=16, pad_token_id=999)))
    for name, seed in (("a.pt", 5), ("b.pt", 6)):
        torch.manual_seed(seed)
        torch.save(SPLADEModernBERT(model_name=str(mdir)).state_dict(), tmp_path / name)
    pairs = [{"source": f"term{i} term{i + 1}", "domain": ["legal", "medical"][i % 2],
              "synonyms": {"exact": [f"term{i}"], "partial": [f"term{i + 1}", "two words"], "related": [f"other{i}"]}}
             for i in range(6)]
    (tmp_path / "pairs.json").write_text(json.dumps(pairs))
    argv = ["--checkpoint", str(tmp_path / "a.pt"), "--compare", str(tmp_path / "b.pt"), "--model-name", str(mdir),
            "--tokenizer", "hash:1000", "--synonym-pairs", str(tmp_path / "pairs.json"), "--k-values", "5,20",
            "--batch-size", "4", "--report", str(tmp_path / "report.json")]
    lines = E.main(argv)
    printed = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == len(printed) == 3 and printed[0]["checkpoint"].endswith("a.pt") and printed[0]["dataset"] == "pairs"
    for line in printed[:2]:
        assert line["num_queries"] == 6 and "per_query_metrics" not in line
        assert sorted(line["recall_at_k"]) == sorted(line["ndcg_at_k"]) == ["20", "5"]
        assert sorted(line["domain_metrics"]) == ["legal", "medical"] and 0.0 <= line["mrr"] <= 1.0
    assert list(printed[2]["metrics_compared"]) == ["mrr", "ndcg@5", "ndcg@10", "ndcg@20"]
    assert set(printed[2]["metrics_compared"]["mrr"]) == {"model_a_mean", "model_b_mean", "paired_t_test", "bootstrap_ci"}
    report = json.loads((tmp_path / "report.json").read_text())
    assert [len(x) for x in report["per_query_metrics"]] == [6, 6] and report["k_values"] == [5, 20]
    assert printed[0]["mrr"] == float(np.mean([q["mrr"] for q in report["per_query_metrics"][0]]))
    only = E.main(argv[:2] + argv[4:-2] + ["--domain", "legal"])
    assert len(only) == 1 and only[0]["num_queries"] == 3 and only[0]["dataset"] == "pairs_legal"


# ------------------------------------------------------------------------------------------------ errors
def test_bad_arguments_are_refused_before_any_launch(dev):
    from snx import fn
    from snx.expansion import graded_metrics, judged_ranks
    rep = torch.ones((2, 64), device=dev)
    ex = torch.zeros(64, dtype=torch.uint8, device=dev)
    j = [[(1, 3, True)], []]
    for kw, msg in ((dict(k_values=[]), "cutoffs"), (dict(k_values=list(range(1, 10))), "cutoffs"),
                    (dict(k_values=[5, 5]), "ascend"), (dict(k_values=[0, 5]), "ascend"), (dict(k_values=[5], max_k=0), "max_k"),
                    (dict(k_values=[5], slices=-1), "slices"), (dict(k_values=[5.0]), "cutoffs")):
        with pytest.raises(ValueError, match=msg):
            graded_metrics(rep, ex, j, **kw)
    for bad_rep in (rep.double(), rep[:, ::2], rep[0], rep.cpu()):
        with pytest.raises(ValueError, match="rep must be"):
            graded_metrics(bad_rep, ex, j, [5])
    with pytest.raises(ValueError, match="excluded"):
        graded_metrics(rep, ex[:63].contiguous(), j, [5])
    with pytest.raises(ValueError, match="repeated"):
        judged_ranks(rep, ex, [0, 2, 2], [4, 4], 5)
    # the C entry point itself: the error code comes back and nothing was launched (the outputs keep their sentinel)
    out = [torch.full((n,), -7, dtype=torch.int32, device=dev) for n in (1, 2, 2, 2)]
    dcg = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    ptr = torch.tensor([0, 1, 1], device=dev)
    tok = torch.tensor([1], dtype=torch.int32, device=dev)
    u8 = torch.ones(1, dtype=torch.uint8, device=dev)
    gain = torch.ones((3, 8), dtype=torch.float64, device=dev)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731

    def call(B=2, V=64, max_k=8, cuts=(5,), G=8, ws_bytes=4096):
        host = (C.c_int32 * len(cuts))(*cuts)
        return fn("snx_expansion_metrics")(p(rep), B, V, p(ex), p(ptr), p(tok), p(u8), p(u8), 1, max_k,
                                           C.cast(host, C.c_void_p), len(cuts), p(gain), G, 0, p(out[0]), p(out[1]),
                                           p(out[2]), p(out[3]), p(dcg), p(ws), ws_bytes, None)
    assert call(cuts=(5, 3)) == -3 and call(V=0) == -2 and call(max_k=0) == -2 and call(G=4) == -3 and call(ws_bytes=4) == -3
    torch.cuda.synchronize()
    assert all((o == -7).all() for o in out) and (dcg == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert out[0].tolist() == [2] and out[1].tolist() == [8, 8] and out[2].tolist() == [2, 0] and dcg.tolist() == [1.0, 0.0]
