"""GPU checks of the exact L2 nearest neighbours and the information-gain filter over them (csrc/infogain.hip, include/snx.h
"exact L2 nearest neighbours"; snx.infogain, src.information_gain, src.train.cli.filter_synonyms).

The distance is a defined chain, so parity is equality: with the rational restatement of the chain on tiny shapes, and
with numpy on data whose every step is exact (integers times 2^-3: ties abound, and the order (d2, id) is checked with
them).  On random floats the numpy chain multiplies and adds where the device fuses, one rounding per step on either side:
|d2 - ref| <= D 2^-52 ref.  The golden pipeline compares with what the reference produced (tests/golden/g19_infogain): the
float64 entropies differ by about d (D + 4) 2^-52 ~ 1e-10, so an fp32 value can differ only at a rounding boundary: one
fp32 ulp for an entropy, two ulps of the larger entropy for their difference."""
import json
import os

import numpy as np
import pytest
import torch

from tests import infogain_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G19 = os.path.join(ROOT, "tests", "golden", "g19_infogain")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g19():
    return R.load_g19(G19)


def _grid(shape, seed):
    """Integers in [-8, 8] times 2^-3: differences, squares and sums of up to 4096 of them are exact in float64."""
    return (np.random.default_rng(seed).integers(-8, 9, size=shape) / 8.0).astype(np.float32)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _knn(index, q, k, **kw):
    d2, ids = index.knn(q, k, **kw)
    assert d2.dtype == torch.float64 and ids.dtype == torch.int32 and d2.shape == ids.shape == (q.shape[0], k)
    return d2.cpu().numpy(), ids.cpu().numpy()


def _expect(q, corpus, k, d2=None):
    """(d2 [nq, k], ids [nq, k]) under (d2 ascending, id ascending), padded with +inf / -1."""
    full = R.d2_plain(q, corpus) if d2 is None else d2
    nq, n = full.shape
    want_d = np.full((nq, k), np.inf)
    want_i = np.full((nq, k), -1, dtype=np.int32)
    for i in range(nq):
        o = R.knn_order(full[i])[:k]
        want_d[i, :o.size], want_i[i, :o.size] = full[i, o], o
    return want_d, want_i


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("D", [1, 3, 33, 100])
def test_chain_is_the_abi_bit_for_bit(dev, D):
    from snx.infogain import L2Index
    rng = np.random.default_rng(D)
    corpus = rng.standard_normal((9, D)).astype(np.float32)
    q = rng.standard_normal((5, D)).astype(np.float32)
    q[3] = corpus[6]                                          # a query copied from the corpus
    exact = np.array([[R.d2_fma(q[i], corpus[r]) for r in range(9)] for i in range(5)])
    got_d, got_i = _knn(L2Index(corpus, dev), q, 9)
    want_d, want_i = _expect(q, corpus, 9, exact)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(_bits(got_d), _bits(want_d))
    assert got_i[3, 0] == 6 and _bits(got_d[3, 0]) == 0       # exactly +0.0 at rank 1


# ------------------------------------------------------------------------------------------------ exact data, ties, padding
@pytest.mark.parametrize("nq", [1, 65])
@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_exact_data_order_and_padding(dev, nq, n):
    from snx.infogain import L2Index
    for D in (7, 8):                                          # the scalar and the 16-byte loads
        corpus, q = _grid((n, D), 100 * n + D), _grid((nq, D), 100 * n + D + 1)
        q[0] = corpus[n // 2]
        corpus[n - 1] = corpus[0]                             # an exact duplicate: a tie for every query (n > 1)
        index = L2Index(corpus, dev)
        full = R.d2_plain(q, corpus)
        for k in (1, 11, 50, 256):
            got_d, got_i = _knn(index, q, k)
            want_d, want_i = _expect(q, corpus, k, full)
            assert np.array_equal(got_i, want_i), (D, k)
            assert np.array_equal(_bits(got_d), _bits(want_d)), (D, k)
            if k > n:
                assert (got_i[:, n:] == -1).all() and np.isposinf(got_d[:, n:]).all()


# ------------------------------------------------------------------------------------------------ the selection paths
@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_selection_paths_splits_and_query_slices(dev, order):
    """n = 4096, D = 4, k = 8.  Rows by descending distance: every row beats the threshold and every list is compacted over
    and over.  Ascending: the first tile fills the list and nothing follows.  Rows equal to the nearest one sit on both
    sides of the split boundaries of chunk_rows 128 and 1024; chunk_rows and the query slices change no bit."""
    from snx.infogain import L2Index
    n, D, k, nq = 4096, 4, 8, 65
    corpus = _grid((n, D), 7)
    norm = (corpus.astype(np.float64) ** 2).sum(axis=1)
    o = np.argsort(norm, kind="stable")
    corpus = corpus[o[::-1] if order == "descending" else o].copy()
    near = corpus[-1] if order == "descending" else corpus[0]
    q = (near[None] + _grid((nq, D), 8) / 8.0).astype(np.float32)        # a step of at most 2^-3: the corpus order is the queries'
    for r in (127, 128, 1023, 1024, 2047, 2048):
        corpus[r] = near
    full = R.d2_plain(q, corpus)
    want_d, want_i = _expect(q, corpus, k, full)
    assert all(len({127, 128, 1023, 1024} & set(want_i[i].tolist())) >= 2 for i in range(nq))
    index = L2Index(corpus, dev)
    for chunk_rows in (0, 128, 1024):
        got_d, got_i = _knn(index, q, k, chunk_rows=chunk_rows)
        assert np.array_equal(got_i, want_i), chunk_rows       # the lowest id first among equals
        assert np.array_equal(_bits(got_d), _bits(want_d)), chunk_rows
        a_d, a_i = _knn(index, q[:1], k, chunk_rows=chunk_rows)
        b_d, b_i = _knn(index, q[1:], k, chunk_rows=chunk_rows)
        assert np.array_equal(np.concatenate([a_i, b_i]), want_i)
        assert np.array_equal(_bits(np.concatenate([a_d, b_d])), _bits(want_d))
    s_d, s_i = _knn(index, q, k, query_slice=1)
    assert np.array_equal(s_i, want_i) and np.array_equal(_bits(s_d), _bits(want_d))


# ------------------------------------------------------------------------------------------------ random floats
@pytest.fixture(scope="module")
def floats():
    rng = np.random.default_rng(11)
    corpus = rng.standard_normal((2000, 768)).astype(np.float32)
    q = rng.standard_normal((50, 768)).astype(np.float32)
    q[:10] = corpus[5:15] + np.float32(0.01) * q[:10]
    return corpus, q, R.d2_plain(q, corpus)


def test_random_floats_within_one_rounding_per_step(dev, floats):
    from snx.infogain import L2Index
    corpus, q, full = floats
    k, bound = 51, 768 * 2.0 ** -52
    s = np.sort(full, axis=1)[:, :k + 1]
    assert ((s[:, 1:] - s[:, :-1]) > 2 * bound * s[:, 1:]).all()          # the reference's order is decided
    want_d, want_i = _expect(q, corpus, k, full)
    got_d, got_i = _knn(L2Index(corpus, dev), q, k)
    worst = float((np.abs(got_d - want_d) / want_d).max())
    print(f"d2 against the numpy float64 chain: worst relative difference {worst:.3g}, bound {bound:.3g}")
    assert np.array_equal(got_i, want_i)
    assert worst <= bound


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("D", [1, 33, 768])
def test_gather_sorted_equals_the_search(dev, D):
    from snx.infogain import L2Index
    rng = np.random.default_rng(D)
    n = 300
    corpus = rng.standard_normal((n, D)).astype(np.float32)
    index = L2Index(corpus, dev)
    for m in (1, 3):
        t = rng.standard_normal((m, D)).astype(np.float32)
        t[0] = corpus[17]
        all_d, all_i = _knn(index, t, 256)
        lookup = [dict(zip(all_i[i].tolist(), _bits(all_d[i]).tolist())) for i in range(m)]
        for K in (1, 2, 50, 256):
            nb = np.stack([rng.permutation(all_i[i])[:K] for i in range(m)]).astype(np.int32)
            if K > 1:
                nb[:, rng.choice(K, size=max(1, K // 5), replace=False)] = -1           # skipped slots
            got = index.gather_sorted(t, nb)
            assert got.dtype == torch.float64 and got.shape == (m, K)
            got = got.cpu().numpy()
            for i in range(m):
                want = sorted(lookup[i][j] for j in nb[i].tolist() if j >= 0)
                filled = len(want)
                assert _bits(got[i, :filled]).tolist() == want, (m, K, i)               # ascending; the search's bits
                assert np.isposinf(got[i, filled:]).all()
    with pytest.raises(ValueError):
        index.gather_sorted(corpus[:2], np.full((2, 3), n, dtype=np.int32))


# ------------------------------------------------------------------------------------------------ the golden pipeline
def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _close_to_golden(got, want, name):
    """Entropies within 1 fp32 ulp, IG within 2 ulps of the larger entropy; returns how many values are not bit-equal."""
    (ig, h_t, h_c), (g_ig, g_t, g_c) = got, want
    assert all(x.dtype == np.float32 for x in got), name
    for x, y, what in ((h_t, g_t, "h_target"), (h_c, g_c, "h_cond")):
        assert (np.abs(x.astype(np.float64) - y.astype(np.float64)) <= _ulp32(y)).all(), (name, what)
    big = np.maximum(_ulp32(g_t), _ulp32(g_c))
    assert (np.abs(ig.astype(np.float64) - g_ig.astype(np.float64)) <= 2 * big).all(), (name, "ig")
    return sum(int((x.view(np.uint32) != y.view(np.uint32)).sum()) for x, y in zip(got, want))


def _config(case, **kw):
    from src.information_gain import InformationGainConfig
    return InformationGainConfig(k_entropy=case["k_entropy"], k_neighborhood=case["k_neighborhood"],
                                 percentile_threshold=case["percentile"], min_ig_absolute=case["min_ig_absolute"],
                                 normalize_embeddings=case["normalize"], **kw)


def _golden(g19, name):
    a = g19["arrays"]
    return a[f"{name}/ig"], a[f"{name}/h_target"], a[f"{name}/h_cond"]


def test_golden_pipeline(dev, g19):
    from src.information_gain import (InformationGainFilter, analyze_ig_distribution, compute_adaptive_threshold,
                                      compute_information_gain, compute_information_gain_batch, filter_synonym_pairs)
    off = 0
    for case in g19["cases"]:
        corpus, src, tgt, _ = R.build_case(case)
        name, want = case["name"], _golden(g19, case["name"])
        got = compute_information_gain_batch(src, tgt, corpus, _config(case))
        off += _close_to_golden(got, want, name)
        small = compute_information_gain_batch(src, tgt, corpus, _config(case, batch_size=7))
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, small)), name
        for method, t in case["thresholds"].items():
            assert repr(compute_adaptive_threshold(got[0], method=method, percentile=case["percentile"])) == t, (name, method)
        pairs = [tuple(p) for p in case["pairs"]]
        results = filter_synonym_pairs(pairs, src, tgt, corpus, _config(case))
        assert [r.is_filtered for r in results] == case["flags"], name
        assert [r.filter_reason for r in results] == case["reasons"], name
        assert analyze_ig_distribution(results) == case["distribution"], name
        if f"{name}/single" in g19["arrays"]:
            single = g19["arrays"][f"{name}/single"]
            d, D = case["D"], case["D"]
            for i in range(single.shape[0]):
                one = np.array(compute_information_gain(src[i], tgt[i], corpus, _config(case)))
                tol = d * (D + 4) * 2.0 ** -52 + 8 * np.spacing(np.abs(single[i]).max())
                assert (np.abs(one - single[i]) <= 2 * tol).all(), (name, i)
        if name == g19["filter_case"]:
            f = InformationGainFilter(_config(case, use_faiss=False)).fit(corpus)
            fr = f.filter_pairs(pairs, src, tgt)
            cls = tuple(np.array([getattr(r, a) for r in fr], dtype=np.float32)
                        for a in ("information_gain", "target_entropy", "conditional_entropy"))
            a = g19["arrays"]
            off += _close_to_golden(cls, (a["filter/ig"], a["filter/h_target"], a["filter/h_cond"]), "filter")
            # IndexFlatL2's convention: squared distances as fp32, ids int64, over the rows fit kept
            kept = R.normalize_rows(corpus) if case["normalize"] else corpus
            q = R.normalize_rows(tgt[1:2])[0]
            d2, ids = f.get_knn_faiss(q, 5)
            full = R.d2_plain(q[None], kept)[0]
            o = R.knn_order(full)[:5]
            assert d2.dtype == np.float32 and ids.dtype == np.int64 and ids.tolist() == o.tolist()
            assert (np.abs(d2.astype(np.float64) - full[o]) <= np.spacing(full[o].astype(np.float32))).all()
    print(f"golden pipeline: {off} fp32 values are not bit-equal to the reference's")


def test_single_query_functions(dev):
    """knn_entropy_kl skips the nearest row when the query is in the reference set, knn_entropy_batch never does, and
    get_knn_indices is the order (d2, id)."""
    from src.information_gain import _log_volume_unit_ball, get_knn_indices, knn_entropy_batch, knn_entropy_kl
    rng = np.random.default_rng(3)
    ref = rng.standard_normal((100, 8)).astype(np.float32)
    q = rng.standard_normal((5, 8)).astype(np.float32)
    q[2] = ref[40]
    dist = np.sqrt(np.sort(R.d2_plain(q, ref), axis=1))
    batch = knn_entropy_batch(q, ref, k=5)
    want = R.kl_entropy(dist[:, 5], 8, 100, 5)
    assert batch.dtype == np.float32 and (np.abs(batch - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    for i in range(5):
        one = knn_entropy_kl(q[i], ref, k=5)
        rho = dist[i, 5] if i == 2 else dist[i, 4]
        ref_one = float(R.kl_entropy(rho, 8, 100, 5))
        # d ln(rho) moves by d (D + 4) 2^-52 with the chain's roundings; eight roundings of the sums on either side
        assert isinstance(one, float) and abs(one - ref_one) <= 8 * 12 * 2.0 ** -52 + 8 * np.spacing(abs(ref_one))
        ids = get_knn_indices(q[i], ref, 10)
        assert ids.dtype == np.int64 and ids.tolist() == R.knn_order(R.d2_plain(q[i:i + 1], ref)[0])[:10].tolist()
    assert knn_entropy_kl(q[0], ref[:1], k=5) == 0.0 and not knn_entropy_batch(q, ref[:1], k=5).any()
    assert len(get_knn_indices(q[0], ref[:3], 10)) == 3
    assert abs(_log_volume_unit_ball(3) - np.log(4 / 3 * np.pi)) < 1e-12


def test_cli_report_equals_the_golden(dev, g19, tmp_path, capsys):
    from src.train.cli.filter_synonyms import main
    case = next(c for c in g19["cases"] if c["kinds"] == ["corpus"])
    corpus, _, _, rows = R.build_case(case)
    terms = [f"t{i}" for i in range(case["n"])]
    pairs = [{"source": s, "target": t, "similarity": sim, "category": "cluster"} for s, t, sim in case["pairs"]]
    pairs.insert(3, {"source": "t1", "target": "absent"})
    pairs.append({"source": "nowhere", "target": "nothing", "similarity": 0.9})
    np.save(tmp_path / "E.npy", corpus)
    (tmp_path / "terms.json").write_text(json.dumps(terms))
    (tmp_path / "pairs.json").write_text(json.dumps(pairs))
    summary = main(["--pairs", str(tmp_path / "pairs.json"), "--embeddings", str(tmp_path / "E.npy"), "--terms",
                    str(tmp_path / "terms.json"), "--output-dir", str(tmp_path / "out"), "--k-entropy",
                    str(case["k_entropy"]), "--k-neighborhood", str(case["k_neighborhood"]), "--percentile-threshold",
                    str(case["percentile"]), "--min-ig-absolute", str(case["min_ig_absolute"]), "--batch-size", "16"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {k: v for k, v in line.items() if k != "seconds"} == {k: v for k, v in summary.items() if k != "seconds"}
    assert (summary["terms"], summary["dim"], summary["total_pairs"], summary["scored_pairs"], summary["skipped_pairs"]) == (
        case["n"], case["D"], case["m"] + 2, case["m"], 2)
    assert summary["filtered_pairs"] == sum(case["flags"]) and summary["kept_pairs"] == case["m"] - sum(case["flags"])
    assert repr(summary["threshold"]) == case["thresholds"]["percentile"]
    with open(tmp_path / "out" / "ig_report.json") as f:
        report = json.load(f)
    assert [(s["source"], s["target"], s["missing"]) for s in report["skipped"]] == [
        ("t1", "absent", ["absent"]), ("nowhere", "nothing", ["nowhere", "nothing"])]
    assert [(r["source"], r["target"], r["similarity"]) for r in report["results"]] == [tuple(p) for p in case["pairs"]]
    assert [r["is_filtered"] for r in report["results"]] == case["flags"]
    assert [r["filter_reason"] for r in report["results"]] == case["reasons"]
    assert report["distribution"] == case["distribution"]
    got = tuple(np.array([r[a] for r in report["results"]], dtype=np.float32)
                for a in ("information_gain", "target_entropy", "conditional_entropy"))
    _close_to_golden(got, _golden(g19, case["name"]), "cli")
