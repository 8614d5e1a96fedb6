#!/usr/bin/env python3
"""Write tests/golden/g19_infogain/ by RUNNING the reference's src/information_gain.py (it needs numpy and scipy).

    python tools/make_golden_infogain.py --reference <checkout of the reference project>

The inputs of every case come from tests/infogain_reference.py ``build_case`` (a deterministic generator), so the fixture
holds the case specifications and what the reference answered.  Data only:

  g19.json     per case: the specification, the thresholds of the three methods (repr of the float), the filter flags and
               reasons of filter_synonym_pairs, analyze_ig_distribution; the CLI case's pairs by term name
  arrays.npz   per case ``<name>/ig|h_target|h_cond`` (fp32, compute_information_gain_batch); ``<name>/single`` (float64
               [m, 3], compute_information_gain pair by pair) where recorded; ``filter/...`` the same three arrays through
               InformationGainFilter.fit + filter_pairs; ``psi`` = scipy's digamma(1 .. 256) and ``lnv`` = the
               reference's log unit-ball volume at d = 1 .. 4096 (``lnv_d`` = [first, last])

Cases: the five shape classes n x D x pairs = 300x48x64, 70x33x30, 40x1024x12, 5x7x6, 2000x768x50; targets that are corpus
rows and targets that are not; a target a small step from its source; sources outside the corpus; n < k_neighborhood
(40), n <= k_entropy (5), n = 1; an exact duplicate pair of corpus rows in the interior of a neighbourhood.

The tool refuses to write unless, on the reference's own float64 distances (scipy's cdist): the relative gap between ranks
K and K + 1 of every source's distances exceeds 1e-9; the distance that rho reads is either tied exactly with a neighbour
in the order or more than 1e-9 (relative) away from it; and no IG lies within 4 fp32 ulps of a threshold, other than the
order statistics that define it."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import infogain_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g19_infogain")
MIXED = ["corpus", "fresh_target", "near", "fresh_source", "dup"]
CASES = [
    dict(name="a_300x48", n=300, D=48, m=64, seed=1, kinds=MIXED, k_entropy=10, k_neighborhood=50, normalize=True,
         percentile=10.0, min_ig_absolute=-100.0, single=4),
    dict(name="b_70x33", n=70, D=33, m=30, seed=2, kinds=MIXED, k_entropy=10, k_neighborhood=50, normalize=False,
         percentile=10.0, min_ig_absolute=0.0, single=3),
    dict(name="c_40x1024", n=40, D=1024, m=12, seed=3, kinds=MIXED, k_entropy=10, k_neighborhood=50, normalize=True,
         percentile=10.0, min_ig_absolute=0.0, single=0),
    dict(name="d_5x7", n=5, D=7, m=6, seed=4, kinds=MIXED[:4], k_entropy=10, k_neighborhood=50, normalize=True,
         percentile=10.0, min_ig_absolute=0.0, single=2),
    dict(name="e_2000x768", n=2000, D=768, m=50, seed=5, kinds=MIXED, k_entropy=10, k_neighborhood=50, normalize=True,
         percentile=10.0, min_ig_absolute=-100.0, single=0),
    dict(name="f_1x7", n=1, D=7, m=3, seed=6, kinds=["corpus", "fresh_target", "fresh_source"], k_entropy=10,
         k_neighborhood=50, normalize=True, percentile=10.0, min_ig_absolute=0.0, single=0),
    dict(name="g_300x48_k3", n=300, D=48, m=64, seed=9, kinds=MIXED, k_entropy=3, k_neighborhood=8, normalize=True,
         percentile=25.0, min_ig_absolute=-6.0, single=0),
    dict(name="h_cli_120x32", n=120, D=32, m=40, seed=8, kinds=["corpus"], k_entropy=10, k_neighborhood=50,
         normalize=True, percentile=10.0, min_ig_absolute=-100.0, single=0),
]
FILTER_CASE = "a_300x48"
LNV_D = list(range(1, 4097))
GAP = 1e-9


def load_reference(root: str):
    spec = importlib.util.spec_from_file_location("ref_information_gain", os.path.join(root, "src", "information_gain.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def check_conditioning(case, corpus, src, tgt):
    """The assertions on the reference's own float64 distances."""
    from scipy.spatial.distance import cdist
    if case["normalize"]:
        corpus, src, tgt = R.normalize_rows(corpus), R.normalize_rows(src), R.normalize_rows(tgt)
    n = corpus.shape[0]
    k1 = min(case["k_entropy"], n - 1)
    K = min(case["k_neighborhood"], n)
    k2 = min(min(case["k_entropy"], case["k_neighborhood"] - 1), K - 1)

    def apart(sorted_d, pos, what):
        for o in (pos - 1, pos + 1):
            if 0 <= o < sorted_d.shape[0]:
                x, y = sorted_d[pos], sorted_d[o]
                assert x == y or abs(x - y) > GAP * max(x, y), f"{case['name']}: {what}: near tie {x!r} / {y!r}"

    ds = cdist(src, corpus, metric="euclidean")
    dt = cdist(tgt, corpus, metric="euclidean")
    smallest = np.inf
    for i in range(src.shape[0]):
        s = np.sort(ds[i])
        if K < n:
            gap = (s[K] - s[K - 1]) / s[K]
            assert gap > GAP, f"{case['name']}: pair {i}: neighbourhood boundary gap {gap!r}"
            smallest = min(smallest, gap)
        if k1 >= 1:
            apart(np.sort(dt[i]), min(k1, n - 1), f"pair {i} marginal rho")
        if k2 >= 1:
            nb = np.argsort(ds[i])[:K]
            c = np.sort(cdist(tgt[i:i + 1], corpus[nb], metric="euclidean")[0])
            apart(c, k2 if c[0] < 1e-10 else k2 - 1, f"pair {i} conditional rho")
    return smallest


def check_thresholds(case, ig, thresholds):
    s = np.sort(ig.astype(np.float64))
    pos = (len(s) - 1) * case["percentile"] / 100.0
    bracket = {float(s[int(np.floor(pos))]), float(s[int(np.ceil(pos))])}
    for method, t in thresholds.items():
        for v in ig.astype(np.float64).tolist():
            if v == t or (method == "percentile" and v in bracket):
                continue
            assert abs(v - t) > 4 * max(ulp32(v), ulp32(t)), f"{case['name']}: IG {v!r} within 4 ulps of {method} {t!r}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    from scipy.special import digamma
    arrays, recorded = {}, []
    for case in CASES:
        corpus, src, tgt, rows = R.build_case(case)
        cfg = ref.InformationGainConfig(k_entropy=case["k_entropy"], k_neighborhood=case["k_neighborhood"],
                                        percentile_threshold=case["percentile"], min_ig_absolute=case["min_ig_absolute"],
                                        normalize_embeddings=case["normalize"], use_faiss=False)
        gap = check_conditioning(case, corpus, src, tgt)
        ig, h_t, h_c = ref.compute_information_gain_batch(src, tgt, corpus, cfg)
        assert ig.dtype == h_t.dtype == h_c.dtype == np.float32
        mine = R.information_gain(src, tgt, corpus, case["k_entropy"], case["k_neighborhood"], case["normalize"])
        same = [bool(np.array_equal(x.view(np.uint32), y.view(np.uint32))) for x, y in zip(mine, (ig, h_t, h_c))]
        name = case["name"]
        arrays[f"{name}/ig"], arrays[f"{name}/h_target"], arrays[f"{name}/h_cond"] = ig, h_t, h_c
        thresholds = {m: ref.compute_adaptive_threshold(ig, method=m, percentile=case["percentile"])
                      for m in ("percentile", "otsu", "mad")}
        check_thresholds(case, ig, thresholds)
        pairs = [(f"s{i}" if a < 0 else f"t{a}", f"x{i}" if b < 0 else f"t{b}", round(0.5 + 0.007 * i, 3))
                 for i, (a, b) in enumerate(rows)]
        results = ref.filter_synonym_pairs(pairs, src, tgt, corpus, cfg)
        assert [r.information_gain for r in results] == ig.astype(np.float64).tolist()
        if case["single"]:
            arrays[f"{name}/single"] = np.array([ref.compute_information_gain(src[i], tgt[i], corpus, cfg)
                                                 for i in range(case["single"])], dtype=np.float64)
        recorded.append({**case, "pairs": [list(p) for p in pairs],
                         "thresholds": {m: repr(float(t)) for m, t in thresholds.items()},
                         "flags": [bool(r.is_filtered) for r in results],
                         "reasons": [r.filter_reason for r in results],
                         "distribution": ref.analyze_ig_distribution(results),
                         "boundary_gap": None if not np.isfinite(gap) else float(gap), "restatement_bit_equal": same})
        print(f"{name}: restatement bit-equal {same}, smallest boundary gap {gap:.3g}, "
              f"filtered {sum(r.is_filtered for r in results)}/{len(results)}")
        if name == FILTER_CASE:                               # the class path: the corpus is normalised in fit and again
            f = ref.InformationGainFilter(cfg).fit(corpus)
            fr = f.filter_pairs(pairs, src, tgt)
            arrays["filter/ig"] = np.array([r.information_gain for r in fr], dtype=np.float32)
            arrays["filter/h_target"] = np.array([r.target_entropy for r in fr], dtype=np.float32)
            arrays["filter/h_cond"] = np.array([r.conditional_entropy for r in fr], dtype=np.float32)
    arrays["psi"] = np.array([float(digamma(k)) for k in range(1, 257)], dtype=np.float64)
    arrays["lnv"] = np.array([float(ref._log_volume_unit_ball(d)) for d in LNV_D], dtype=np.float64)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "g19.json"), "w", encoding="utf-8") as f:
        json.dump({"source": "ref:src/information_gain.py compute_information_gain_batch, filter_synonym_pairs, "
                             "InformationGainFilter, analyze_ig_distribution",
                   "numpy": np.__version__, "filter_case": FILTER_CASE, "lnv_d": [LNV_D[0], LNV_D[-1]], "cases": recorded}, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(OUT, "arrays.npz"), **arrays)
    print(f"wrote {OUT}: {len(recorded)} cases")


if __name__ == "__main__":
    main()
