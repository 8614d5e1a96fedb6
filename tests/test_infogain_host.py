"""Host checks of the information-gain filter (include/snx.h "exact L2 nearest neighbours", src.information_gain): the
numpy restatement of the five rules (tests/infogain_reference.py) against what the reference's src/information_gain.py
produced (tests/golden/g19_infogain, written by tools/make_golden_infogain.py; nothing of the reference is read at test
time), the package's host half -- thresholds, decisions, distribution statistics, psi and ln V_d without scipy -- and the
argument checks that need no GPU."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from tests import infogain_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G19 = os.path.join(ROOT, "tests", "golden", "g19_infogain")


@pytest.fixture(scope="module")
def g19():
    return R.load_g19(G19)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _golden(g19, name):
    a = g19["arrays"]
    return a[f"{name}/ig"], a[f"{name}/h_target"], a[f"{name}/h_cond"]


def _config(case):
    from src.information_gain import InformationGainConfig
    return InformationGainConfig(k_entropy=case["k_entropy"], k_neighborhood=case["k_neighborhood"],
                                 percentile_threshold=case["percentile"], min_ig_absolute=case["min_ig_absolute"],
                                 normalize_embeddings=case["normalize"])


# ------------------------------------------------------------------------------------------------ the restatement
def test_golden_covers_the_shape_classes_and_edge_cases(g19):
    shapes = {(c["n"], c["D"], c["m"]) for c in g19["cases"]}
    assert {(300, 48, 64), (70, 33, 30), (40, 1024, 12), (5, 7, 6), (2000, 768, 50)} <= shapes
    assert any(c["n"] == 1 for c in g19["cases"])
    assert any(c["n"] < c["k_neighborhood"] and c["n"] > c["k_entropy"] for c in g19["cases"])
    assert any(1 < c["n"] <= c["k_entropy"] for c in g19["cases"])
    kinds = set().union(*(c["kinds"] for c in g19["cases"]))
    assert kinds == {"corpus", "fresh_target", "near", "fresh_source", "dup"}
    assert all(all(c["restatement_bit_equal"]) for c in g19["cases"])
    assert any(c["flags"].count(True) not in (0, len(c["flags"])) for c in g19["cases"])


def test_restatement_equals_the_reference_bit_for_bit(g19):
    for case in g19["cases"]:
        corpus, src, tgt, _ = R.build_case(case)
        got = R.information_gain(src, tgt, corpus, case["k_entropy"], case["k_neighborhood"], case["normalize"])
        for x, y, what in zip(got, _golden(g19, case["name"]), ("ig", "h_target", "h_cond")):
            assert x.dtype == np.float32 and np.array_equal(_bits(x), _bits(y)), (case["name"], what)


def test_fma_restatement_is_one_rounding_per_step():
    assert R.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60      # a product no double holds
    assert R.fma(3.0, 3.0, 1.0) == 10.0
    q = np.array([0.1, -0.7, 0.3], dtype=np.float32)
    assert R.d2_fma(q, q.copy()) == 0.0
    c = np.array([0.2, 0.5, -0.9], dtype=np.float32)
    plain = float(R.d2_plain(q[None], c[None])[0, 0])
    assert abs(R.d2_fma(q, c) - plain) <= 3 * 2.0 ** -52 * plain


# ------------------------------------------------------------------------------------------------ the package's host half
def test_thresholds_flags_and_reasons_equal_the_reference(g19):
    from src.information_gain import compute_adaptive_threshold, compute_percentile_threshold, decide_pairs
    for case in g19["cases"]:
        ig, h_t, h_c = _golden(g19, case["name"])
        for method, want in case["thresholds"].items():
            got = compute_adaptive_threshold(ig, method=method, percentile=case["percentile"])
            assert isinstance(got, float) and repr(got) == want, (case["name"], method)
        thr = compute_percentile_threshold(ig, case["percentile"])
        pairs = [tuple(p) for p in case["pairs"]]
        results = decide_pairs(pairs, ig, h_t, h_c, thr, _config(case), "percentile")
        assert [r.is_filtered for r in results] == case["flags"], case["name"]
        assert [r.filter_reason for r in results] == case["reasons"], case["name"]
        assert [(r.source, r.target, r.similarity) for r in results] == pairs
        assert [r.information_gain for r in results] == ig.astype(np.float64).tolist()
    with pytest.raises(ValueError):
        compute_adaptive_threshold(np.zeros(3, dtype=np.float32), method="mean")


def test_distribution_statistics_equal_the_reference(g19):
    from src.information_gain import InformationGainResult, analyze_ig_distribution
    for case in g19["cases"]:
        ig, h_t, h_c = _golden(g19, case["name"])
        results = [InformationGainResult(s, t, float(ig[i]), float(h_t[i]), float(h_c[i]), sim, case["flags"][i])
                   for i, (s, t, sim) in enumerate(case["pairs"])]
        got = analyze_ig_distribution(results)
        assert list(got) == list(case["distribution"]) and got == case["distribution"], case["name"]


def test_psi_and_log_volume_without_scipy(g19):
    from snx.infogain import digamma_int, log_volume_unit_ball
    psi = g19["arrays"]["psi"]
    assert psi.shape == (256,)
    for k in range(1, 257):
        got = digamma_int(k)
        assert abs(got - psi[k - 1]) <= np.spacing(abs(psi[k - 1])), k
        assert got == R.digamma_int(k)
    lo, hi = g19["lnv_d"]
    lnv = g19["arrays"]["lnv"]
    assert (lo, hi, lnv.shape) == (1, 4096, (4096,))                                        # every D the ABI admits
    for d in range(lo, hi + 1):
        got, want = log_volume_unit_ball(d), lnv[d - lo]
        assert abs(got - want) <= np.spacing(abs(want)), d
    with pytest.raises(ValueError):
        digamma_int(0)


def test_degenerate_sizes_give_zeros():
    from snx.infogain import entropy_ks
    assert entropy_ks(1, 10, 50) == (0, 1, 0)
    assert entropy_ks(0, 10, 50)[0] < 1 and entropy_ks(0, 10, 50)[2] < 1
    assert entropy_ks(2, 10, 50) == (1, 2, 1) and entropy_ks(300, 10, 50) == (10, 50, 10)
    assert entropy_ks(300, 10, 1) == (10, 1, 0) and entropy_ks(300, 0, 50) == (0, 50, 0)
    rng = np.random.default_rng(0)
    one, m = rng.standard_normal((1, 7)).astype(np.float32), rng.standard_normal((4, 7)).astype(np.float32)
    for n_rows, ke, kn in ((one, 10, 50), (m, 0, 50), (m, 10, 1)):
        got = R.information_gain(m, m[::-1], n_rows, ke, kn)
        if ke == 0 or n_rows.shape[0] == 1:
            assert all(x.dtype == np.float32 and not x.any() for x in got)
        else:
            assert not got[2].any() and got[1].all() and np.array_equal(got[0], got[1])


def test_argument_checks_need_no_gpu():
    from snx import fn
    from snx.infogain import DIM_MAX, K_MAX, L2Index, check_ig_ks, check_k, check_rows
    assert (K_MAX, DIM_MAX) == (256, 4096)
    assert check_k(256, "t") == 256
    for bad in (0, 257, True, 2.0):
        with pytest.raises(ValueError):
            check_k(bad, "t")
    ok = np.zeros((3, 5), dtype=np.float32)
    assert check_rows(ok, "t", "x", 5).shape == (3, 5)
    for bad in (np.zeros((3, 4097), dtype=np.float32), np.zeros((3, 0), dtype=np.float32), np.zeros(5, dtype=np.float32),
                ok.astype(np.float64), np.array([[1.0, np.inf]], dtype=np.float32),
                np.array([[np.nan, 0.0]], dtype=np.float32)):
        with pytest.raises(ValueError):
            check_rows(bad, "t", "x")
        with pytest.raises(ValueError):
            L2Index(bad)                                     # refused before any device is touched
    with pytest.raises(ValueError):
        check_rows(ok, "t", "x", 6)
    assert check_ig_ks(255, 256) == (255, 256)
    for ke, kn in ((256, 50), (10, 257), (-1, 50), (10, True)):
        with pytest.raises(ValueError):
            check_ig_ks(ke, kn)
    # the C ABI refuses the same before any launch
    one = C.c_void_p(256)
    knn, gather = fn("snx_l2_knn"), fn("snx_l2_gather_sorted")
    assert knn(one, 1, one, 1, 4, 257, 0, one, one, one, 1 << 20, None) == -2
    assert knn(one, 1, one, 1, 4, 0, 0, one, one, one, 1 << 20, None) == -2
    assert knn(one, 1, one, 1, 4097, 1, 0, one, one, one, 1 << 20, None) == -2
    assert knn(one, 1, one, 1, 4, 1, -1, one, one, one, 1 << 20, None) == -2
    assert knn(None, 1, one, 1, 4, 1, 0, one, one, one, 1 << 20, None) == -3
    assert knn(one, 1, one, 1, 4, 1, 0, one, one, one, 0, None) == -3                     # workspace too small
    assert knn(one, 0, one, 1, 4, 1, 0, one, one, None, 0, None) == 0                      # no query: nothing to do
    assert gather(one, 1, one, 1, 4, one, 257, one, None) == -2
    assert gather(one, 1, one, 1, 4097, one, 1, one, None) == -2
    assert gather(one, 1, one, 1, 4, None, 1, one, None) == -3
    ws = fn("snx_l2_knn_workspace_bytes")
    assert ws(1, 1000, 257, 0) == 0 and ws(1, 1000, 8, 0) > 0
    # the workspace grows with nq * k * splits, never with nq * n
    assert ws(64, 1 << 20, 8, 1 << 20) == ws(64, 1 << 10, 8, 1 << 10)
    assert ws(128, 4096, 8, 1024) == 2 * ws(64, 4096, 8, 1024)


def test_abi_is_declared_bound_and_guarded():
    from snx import asmcheck
    from snx._lib import SIGNATURES
    with open(os.path.join(ROOT, "include", "snx.h")) as f:
        header = f.read()
    assert "exact L2 nearest neighbours" in header and re.search(r"#define SNX_L2_KMAX 256\b", header)
    for name in ("snx_l2_knn_workspace_bytes", "snx_l2_knn", "snx_l2_gather_sorted"):
        assert name in SIGNATURES and re.search(r"\b%s\(" % name, header)
    assert set(asmcheck.GUARDED["infogain.hip"]) == {"l2_search_kernel", "l2_merge_kernel", "l2_gather_kernel"}


def test_mirror_has_the_reference_names_and_defaults():
    import src.information_gain as M
    for name in ("InformationGainConfig", "InformationGainResult", "knn_entropy_kl", "knn_entropy_batch", "get_knn_indices",
                 "compute_information_gain", "compute_information_gain_batch", "compute_percentile_threshold",
                 "compute_adaptive_threshold", "filter_synonym_pairs", "InformationGainFilter", "analyze_ig_distribution"):
        assert hasattr(M, name), name
    assert dataclasses.asdict(M.InformationGainConfig()) == dict(
        k_entropy=10, k_neighborhood=50, percentile_threshold=10.0, min_ig_absolute=0.0, batch_size=1000, use_faiss=True,
        normalize_embeddings=True, verbose=False)
    assert [f.name for f in dataclasses.fields(M.InformationGainResult)] == [
        "source", "target", "information_gain", "target_entropy", "conditional_entropy", "similarity", "is_filtered",
        "filter_reason"]
    f = M.InformationGainFilter()
    with pytest.raises(RuntimeError):
        f.filter_pairs([], np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32))
    with pytest.raises(RuntimeError):
        f.get_knn_faiss(np.zeros(4, np.float32), 1)


def test_cli_arguments():
    from src.train.cli.filter_synonyms import parse_args
    a = parse_args(["--pairs", "p.json", "--embeddings", "E.npy", "--terms", "t.json", "--output-dir", "o"])
    assert (a.k_entropy, a.k_neighborhood, a.percentile_threshold, a.min_ig_absolute, a.method, a.no_normalize,
            a.batch_size) == (10, 50, 10.0, 0.0, "percentile", False, 1000)
    with pytest.raises(SystemExit):
        parse_args(["--pairs", "p.json", "--embeddings", "E.npy", "--terms", "t.json", "--output-dir", "o", "--method", "x"])
