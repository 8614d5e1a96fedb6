"""CPU checks of the IVF-Flat dense retrieval (include/snx.h "IVF-Flat dense retrieval"): the numpy stand-in
tests/ivf_reference.py is held to the definition by brute force on dyadic data (where fp32 dot products are exact in any
order), its k-means step to hand-worked centroids, and the miner (src.preprocessing.miners) driven by the stand-ins to the
reference's own results (tests/golden/g22_miner/miner.json, written by tools/make_golden_miner.py).  Every check is run
again with a one-line fault planted in the stand-in and must fail then."""
import ctypes as C
import dataclasses
import json
import os
import re
from typing import Any, Dict, Optional

import numpy as np
import pytest

from tests import dense_reference as DR
from tests import ivf_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "g22_miner", "miner.json")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _dyadic(rng, n, D):
    return (rng.integers(-8, 9, size=(n, D)) / 8.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the definition
def definition(E, Cn, Q, nprobe, lo, hi, exclude=None, ceiling=None):
    """The header's definition by brute force: list(d) and P(q) by argmax / lexsort with ties to the lowest list, then the
    exact dense band search with every doc outside the probed lists excluded."""
    ids = np.arange(Cn.shape[0])
    doc_list = np.array([ids[np.lexsort((ids, -row))][0] for row in R.scores64(E, Cn)], np.int64)
    probed = [ids[np.lexsort((ids, -row))][:nprobe] for row in R.scores64(Q, Cn)]
    S = DR.exact_scores(Q, E)
    ex = []
    for q in range(Q.shape[0]):
        out = set(np.flatnonzero(~np.isin(doc_list, probed[q])).tolist())
        if exclude is not None:
            out |= set(exclude[q])
        ex.append(sorted(out))
    return doc_list, np.stack(probed).astype(np.int32), DR.search_band(S, lo, hi, ex, ceiling)


def _case(seed=0, nd=90, nq=7, D=6, nlist=5):
    rng = np.random.default_rng(seed)
    E, Q, Cn = _dyadic(rng, nd, D), _dyadic(rng, nq, D), _dyadic(rng, nlist, D)
    Cn[3] = Cn[1]                                            # duplicate centroids: list 3 stays empty, ties go to list 1
    E[10] = Cn[1]
    Q[2] = Cn[1]                                             # a doc and a query certainly tied between lists 1 and 3
    return E, Q, Cn


def _standin(E, Cn, fault=None, batches=1):
    idx = R.NumpyIvfFlatIndex(E.shape[1], Cn.shape[0], fault=fault).set_centroids(Cn)
    for part in np.array_split(E, batches):
        idx.add(part)
    return idx.build()


def check_lists_and_probe(fault=None):
    E, Q, Cn = _case()
    idx = _standin(E, Cn, fault, batches=3)
    doc_list, probed, _ = definition(E, Cn, Q, 3, 0, 1)
    st = idx.structure()
    assert np.array_equal(st["list_ptr"], np.concatenate([[0], np.cumsum(np.bincount(doc_list, minlength=5))]))
    assert st["list_ptr"][4] == st["list_ptr"][3]            # the duplicate centroid's list is empty
    for c in range(5):
        assert np.array_equal(st["list_doc"][st["list_ptr"][c]:st["list_ptr"][c + 1]], np.flatnonzero(doc_list == c))
    sc, lists = idx.probe(Q, 3)
    assert np.array_equal(lists, probed)
    assert np.array_equal(_bits(sc), _bits(np.take_along_axis(DR.exact_scores(Q, Cn), probed.astype(np.int64), 1)))


def check_search_and_band(fault=None):
    E, Q, Cn = _case(1)
    idx = _standin(E, Cn, fault)
    S = DR.exact_scores(Q, E)
    for nprobe in (1, 3, 5):
        for k in (1, 10, 200):                               # 200: more than the probed lists hold -> unused slots
            sc, dc = idx.search(Q, k, nprobe=nprobe)
            _, _, (rs, rd, rf) = definition(E, Cn, Q, nprobe, 0, k)
            assert np.array_equal(dc, rd) and np.array_equal(_bits(sc), _bits(rs))
            assert ((dc == -1) == (np.arange(k)[None, :] >= rf[:, None])).all()
    rs, rd, _, _ = DR.search(S, 10)
    sc, dc = idx.search(Q, 10, nprobe=5)                     # every list probed: the exact search
    assert np.array_equal(dc, rd) and np.array_equal(_bits(sc), _bits(rs))
    rng = np.random.default_rng(2)
    excl = [sorted(rng.choice(90, size=n, replace=False).tolist()) for n in (0, 40, 90, 0, 5, 0, 40)]
    mid = [float(np.sort(S[q])[::-1][20]) for q in range(7)]
    ceil = [np.inf, np.inf, np.inf, mid[3], mid[4], -np.inf, mid[6]]
    for lo, hi in ((0, 1), (2, 9), (5, 60)):
        for ex, ce in ((excl, None), (None, ceil), (excl, ceil)):
            got = idx.search_band(Q, lo, hi, exclude=ex, ceiling=ce, nprobe=2)
            _, _, want = definition(E, Cn, Q, 2, lo, hi, ex, ce)
            assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1])
            assert np.array_equal(_bits(got[0]), _bits(want[0]))
    pairs = np.array([[0, 5], [6, 89], [2, 10]])
    assert np.array_equal(_bits(idx.pair_scores(Q, pairs)), _bits(S[pairs[:, 0], pairs[:, 1]]))


def check_ties_across_lists(fault=None):
    # two lists whose docs all score 0.5 for the one query; list 0 is walked first and holds the HIGHER doc ids
    Cn = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    E = np.array([[0, 1, 0.5]] * 6 + [[1, 0, 0.5]] * 6, np.float32)         # docs 0-5 in list 1, docs 6-11 in list 0
    Q = np.array([[0, 0, 1]], np.float32)                    # tied between the centroids: probes list 0, then list 1
    idx = _standin(E, Cn, fault)
    assert idx.probe(Q, 2)[1].tolist() == [[0, 1]]
    sc, dc = idx.search(Q, 4, nprobe=2)
    assert dc.tolist() == [[0, 1, 2, 3]] and sc.tolist() == [[0.5] * 4]
    assert idx.search(Q, 4, nprobe=1)[1].tolist() == [[6, 7, 8, 9]]


def test_stand_in_satisfies_the_definition():
    check_lists_and_probe()
    check_search_and_band()
    check_ties_across_lists()


def test_planted_faults_in_the_stand_in_are_caught():
    with pytest.raises(AssertionError):
        check_lists_and_probe("tie_high")
    with pytest.raises(AssertionError):
        check_ties_across_lists("carry_threshold")
    with pytest.raises(AssertionError):
        check_search_and_band("fill_slots")
    with pytest.raises(AssertionError):
        check_miner_skips_unfilled_slots("fill_slots")


# ------------------------------------------------------------------------------------------------ k-means
def test_kmeans_step_by_hand():
    X = np.array([[2, 0], [0, 1], [4, 0], [0, 3], [1, -1], [-1, 1], [3, 4]], np.float32)
    lists = np.array([0, 1, 0, 1, 2, 2, 4])
    prev = np.array([[9, 9], [9, 9], [9, 9], [0.5, -0.25], [9, 9]], np.float32)
    got = R.kmeans_update(X, lists, prev)
    want = np.array([[1, 0], [0, 1], [0, 0], [0.5, -0.25], [np.float32(np.float64(3) / 5), np.float32(np.float64(4) / 5)]],
                    np.float32)                              # mean (3, 0) / 3; (0, 2) / 2; zero mean; empty: kept; (3, 4) / 5
    assert np.array_equal(_bits(got), _bits(want))
    # more members than one segment of the sum: (1026 * 3, 1026 * 4) / 1026 -> (0.6, 0.8) again
    big = np.tile(np.array([[3, 4]], np.float32), (R.KM_SEG + 2, 1))
    one = R.kmeans_update(big, np.zeros(len(big), np.int64), np.zeros((1, 2), np.float32))
    assert np.array_equal(_bits(one), _bits(want[4:5]))


def test_kmeans_on_separated_clusters_and_nlist_clamp():
    rng = np.random.default_rng(3)
    axes = np.eye(4, dtype=np.float32)[:3] * 8
    X = np.concatenate([axes[c] + rng.integers(-1, 2, size=(20, 4)) for c in range(3)]).astype(np.float32)
    X = X[rng.permutation(len(X))]
    c = R.kmeans(X, 3, 10, 2)                                # seed 2: the initial rows come from three different clusters
    assert sorted(np.argmax(c, axis=1).tolist()) == [0, 1, 2] and (c.max(axis=1) > 0.95).all()
    assert np.array_equal(_bits(c), _bits(R.kmeans(X, 3, 10, 2))) and not np.array_equal(c, R.kmeans(X, 3, 0, 2))
    idx = R.NumpyIvfFlatIndex(4, 100, nprobe=100)
    idx.add(X[:5])
    idx.build()
    assert idx.nlist == 5 and idx.nprobe == 5 and idx.list_ptr[-1] == 5


# ------------------------------------------------------------------------------------------------ the miner
@dataclasses.dataclass
class Triplet:
    query: str
    positive: str
    negative: Optional[str] = None
    pair_type: str = "unknown"
    difficulty: str = "medium"
    source: str = ""
    metadata: Dict[str, Any] = dataclasses.field(default_factory=dict)


def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        g = json.load(f)
    table = {t: np.asarray(row, np.float32) / 4 for t, row in zip(g["texts"], g["embeddings_times_4"])}
    return g, (lambda texts: np.stack([table[t] for t in texts]))


def run_golden_cases(make_miner):
    """Every recorded case of the golden through a miner built by ``make_miner(encode)`` -> nothing; asserts equality."""
    g, encode = golden()
    miner = make_miner(encode)
    for case in g["cases"]:
        kw = case["kwargs"]
        if case["kind"] == "mine_negatives":
            got = [dataclasses.asdict(r) for r in miner.mine_negatives(case["queries"], case["positives"], **kw)]
        else:
            got = [dataclasses.asdict(t) for t in miner.mine_for_triplets([Triplet(**t) for t in case["triplets"]], **kw)]
        assert got == case["results"], (case["kind"], kw)


def _cpu_miner(encode, index_type, fault=None, **kw):
    from src.preprocessing.miners import BGEM3HardNegativeMiner
    g, _ = golden()
    classes = {"flat": DR.NumpyDenseIndex,
               "ivf": lambda dim, nlist, device, nprobe=1: R.NumpyIvfFlatIndex(dim, nlist, device, nprobe=nprobe, fault=fault)}
    miner = BGEM3HardNegativeMiner(device="cpu", encode=encode, index_classes=classes)
    miner.build_index(list(g["documents"]), index_type=index_type, **kw)
    return miner


def test_miner_on_the_stand_ins_reproduces_the_reference_results():
    g, _ = golden()
    assert len(g["cases"]) == 6 and any(len(r["negatives"]) < c["kwargs"]["num_negatives"]
                                        for c in g["cases"] if c["kind"] == "mine_negatives" for r in c["results"])
    run_golden_cases(lambda encode: _cpu_miner(encode, "flat"))
    nd = len(g["documents"])
    run_golden_cases(lambda encode: _cpu_miner(encode, "ivf", nlist=4, nprobe=4))     # every list probed: the flat result
    miner = _cpu_miner(golden()[1], "ivf", nlist=1000, nprobe=1)
    assert miner._index.nlist == nd                          # clamped, as the reference clamps it
    miner.clear_index()
    with pytest.raises(RuntimeError):
        miner.mine_negatives(["q"], ["p"])
    with pytest.raises(ValueError):
        miner.build_index(["a"], index_type="hnsw")
    from src.preprocessing.miners import BGEM3HardNegativeMiner
    with pytest.raises(FileNotFoundError):                   # a model name is never resolved
        BGEM3HardNegativeMiner(device="cpu").build_index(["a"])


def check_miner_skips_unfilled_slots(fault=None):
    g, encode = golden()
    miner = _cpu_miner(encode, "ivf", fault=fault, nlist=4, nprobe=1)
    idx = miner._index
    res = miner.mine_negatives(g["cases"][0]["queries"], g["cases"][0]["positives"], num_negatives=5, min_score=-1.0,
                               max_score=2.0)
    q = np.stack([encode([t])[0] for t in g["cases"][0]["queries"]])
    probed = idx.probe(q, 1)[1][:, 0]
    assert (idx.list_ptr[1:] - idx.list_ptr[:-1]).max() < len(g["documents"])          # some slot stays unfilled
    for r, c in zip(res, probed):
        inside = {g["documents"][d] for d in idx.list_doc[idx.list_ptr[c]:idx.list_ptr[c + 1]]}
        assert set(r.negatives) <= inside and r.positive not in r.negatives


def test_miner_skips_unfilled_slots():
    check_miner_skips_unfilled_slots()


def test_mine_dense_negatives_takes_the_ivf_stand_in(tmp_path):
    from src.train.mining.dense import mine_dense_negatives
    from tests.test_dense_host import mine_case
    emb, tix, files = mine_case(tmp_path)
    kw = dict(k=2, rank_start=1, rank_end=3)
    flat = mine_dense_negatives(files, str(tmp_path / "flat"), emb, tix, DR.NumpyDenseIndex(2), **kw)
    ivf = mine_dense_negatives(files, str(tmp_path / "ivf"), emb, tix, R.NumpyIvfFlatIndex(2, 3, nprobe=3, niter=2), **kw)
    assert flat == ivf
    for name in ("train_0.jsonl", "train_1.jsonl"):
        assert (tmp_path / "flat" / name).read_text() == (tmp_path / "ivf" / name).read_text()
    one = mine_dense_negatives(files, str(tmp_path / "one"), emb, tix, R.NumpyIvfFlatIndex(2, 3, nprobe=1, niter=2), **kw)
    assert one["records"] == flat["records"] and one["band_fill"] <= flat["band_fill"]


# ------------------------------------------------------------------------------------------------ header, ABI, CLI
NAMES = ["snx_ivf_build_workspace_bytes", "snx_ivf_build", "snx_ivf_kmeans_update", "snx_ivf_search_workspace_bytes",
         "snx_ivf_search"]


def test_header_and_ctypes_table_name_the_ivf_entry_points():
    import snx
    from snx import asmcheck
    from snx._lib import SIGNATURES
    text = open(os.path.join(ROOT, "include", "snx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, text) and n in SIGNATURES, n
    assert "ref:src/preprocessing/miners/bge_m3_miner.py:91-136, 166-249" in text
    assert not [n for n in snx.verify_exports() if n in NAMES]
    assert set(asmcheck.GUARDED["ivf.hip"]) == {"iv_scan_kernel", "iv_merge_kernel"}


def test_workspace_and_shape_errors_come_from_the_host():
    from snx import fn
    size, build_size = fn("snx_ivf_search_workspace_bytes"), fn("snx_ivf_build_workspace_bytes")
    big = size(4096, 1_000_000, 1000, 8, 100, 2000, 0)
    assert 0 < big < 4096 * 1_000_000 * 4 // 50              # far below the [nq, nd] fp32 matrix
    assert size(4096, 4_000_000, 1000, 8, 100, 2000, 0) == big              # more docs in lists as long: the same
    assert size(4096, 1_000_000, 1000, 8, 100, 2000, 128) > big             # finer splits: more candidate lists
    for bad in ((0, 10, 4, 1, 10, 10, 0), (4, -1, 4, 1, 10, 0, 0), (4, 10, 0, 1, 10, 10, 0), (4, 10, 4, 5, 10, 10, 0),
                (4, 10, 4, 1, 0, 10, 0), (4, 10, 4, 1, 1025, 10, 0), (4, 10, 4, 1, 10, 11, 0), (4, 10, 4, 1, 10, 10, 64),
                (4, 10, 65537, 1, 10, 10, 0)):
        assert size(*bad) == 0, bad
    assert build_size(1000, 7) > 0 and build_size(-1, 7) == 0 and build_size(10, 0) == 0 and build_size(10, 65537) == 0
    buf, ibuf = (C.c_float * 64)(), (C.c_int64 * 64)()
    p, ip = C.cast(buf, C.c_void_p), C.cast(ibuf, C.c_void_p)
    search, build, update = fn("snx_ivf_search"), fn("snx_ivf_build"), fn("snx_ivf_kmeans_update")

    def s(nq=2, D=8, nd=4, nlist=2, max_list=4, nprobe=1, lo=0, hi=1, split=0, q=p, out=ip, ws=p, ws_bytes=1 << 24, ex=None):
        return search(q, nq, D, p, ip, ip, nd, nlist, max_list, ip, nprobe, ex, None, None, lo, hi, split, out, p, None, ws,
                      ws_bytes, None)
    for kw in (dict(D=0), dict(D=4097), dict(nlist=0), dict(nprobe=0), dict(nprobe=3), dict(lo=-1), dict(lo=1, hi=1),
               dict(hi=1025), dict(split=100), dict(max_list=5), dict(nq=-1)):
        assert s(**kw) == -2, kw
    for kw in (dict(q=None), dict(out=None), dict(ws=None), dict(ws_bytes=16), dict(ex=ip)):
        assert s(**kw) == -3, kw
    assert s(nq=0, ws=None, ws_bytes=0) == 0                 # no queries: nothing to do
    assert build(ip, 4, 0, p, 8, ip, ip, p, p, 1 << 20, None) == -2 and build(ip, 4, 2, p, 0, ip, ip, p, p, 1 << 20, None) == -2
    assert build(ip, 4, 2, p, 8, None, ip, p, p, 1 << 20, None) == -3 and build(ip, 4, 2, p, 8, ip, ip, p, p, 0, None) == -3
    assert build(ip, 4, 2, None, 8, ip, ip, p, p, 1 << 20, None) == -3
    assert update(p, 4, 0, ip, ip, 2, p, p, None) == -2 and update(p, 4, 8, ip, ip, 0, p, p, None) == -2
    assert update(p, 4, 8, None, ip, 2, p, p, None) == -3 and update(p, 4, 8, ip, ip, 2, p, None, None) == -3


def test_ivf_index_validates_its_arguments_without_a_gpu():
    from snx.retrieval import IVF_NLIST_MAX, K_MAX, IvfFlatIndex
    for dim in (0, 4097, 1.5, True, "8"):
        with pytest.raises(ValueError):
            IvfFlatIndex(dim, 4, "cpu")
    for nlist in (0, IVF_NLIST_MAX + 1, 2.0, True):
        with pytest.raises(ValueError):
            IvfFlatIndex(8, nlist, "cpu")
    for nprobe in (0, 5, True, 1.0):
        with pytest.raises(ValueError):
            IvfFlatIndex(8, 4, "cpu", nprobe=nprobe)
    with pytest.raises(ValueError):
        IvfFlatIndex(8, 4096, "cpu", nprobe=K_MAX + 1)
    with pytest.raises(ValueError):
        IvfFlatIndex(8, 4, "cpu", niter=-1)
    idx = IvfFlatIndex(8, 4, "cpu", nprobe=4)
    for call in (lambda: idx.search(None, 1), lambda: idx.search_band(None, 0, 1), lambda: idx.pair_scores(None, None),
                 lambda: idx.structure(), lambda: idx.probe(None)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):
        idx.build()                                          # neither centroids nor docs


def test_cli_arguments():
    from src.train.cli import teacher_scores
    base = ["mine", "--embeddings", "e.npy", "--text-index", "t.json"]
    a = teacher_scores.parse_args(base)
    assert (a.index, a.nlist, a.nprobe) == ("flat", 100, 1)
    a = teacher_scores.parse_args(base + ["--index", "ivf", "--nlist", "64", "--nprobe", "8"])
    assert (a.index, a.nlist, a.nprobe) == ("ivf", 64, 8)
    for bad in (["--index", "hnsw"], ["--nprobe", "0"], ["--nlist", "4", "--nprobe", "5"]):
        with pytest.raises(SystemExit):
            teacher_scores.parse_args(base + bad)


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="no hipcc")
def test_scan_kernel_resources_leave_two_workgroups_per_cu():
    """The compiler's own figures for iv_scan_kernel: no scratch, and registers and LDS that let two workgroups (launch
    bounds 256 x 2: two waves per SIMD of 512 registers a lane, 160 KiB of LDS a CU) run side by side, as dn_search_kernel."""
    from snx import asmcheck
    asm = asmcheck.compile_asm(os.path.join(asmcheck.CSRC, "ivf.hip"))
    block = re.search(r"\.amdhsa_kernel \S*iv_scan_kernel\S*\n(.*?)\.end_amdhsa_kernel", asm, re.S)[1]
    got = {k: int(re.search(r"\.amdhsa_%s (\d+)" % k, block)[1])
           for k in ("group_segment_fixed_size", "private_segment_fixed_size", "next_free_vgpr")}
    print(got)
    assert got["private_segment_fixed_size"] == 0
    assert 2 * got["group_segment_fixed_size"] <= 160 * 1024
    assert 2 * ((got["next_free_vgpr"] + 7) // 8 * 8) <= 512
