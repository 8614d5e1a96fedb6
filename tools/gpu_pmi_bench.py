#!/usr/bin/env python3
"""Co-occurrence counting and PMI: the GPU path at 2,000, 100,000 and 640,000 synthetic documents, and the Python loop at
2,000 -- the restatement's (tests/pmi_reference.py), or with ``--reference DIR`` the reference's own
CooccurrenceMatrixBuilder and compute_pmi_matrix (it needs scipy and tqdm; the checkout is only read on the machine that
has it, nothing here needs it on a GPU machine).

    python tools/gpu_pmi_bench.py [--docs 2000,100000,640000] [--cpu-docs 2000] [--window-type sentence] [--reference DIR]

Synthetic documents: 3 .. 6 sentences of 8 .. 24 tokens drawn from a Zipf law over 120,000 terms, closed by one of ``.!?``.
The GPU side is src.pmi.CooccurrenceMatrixBuilder (the reference's defaults: sentence windows, min_term_freq 5, symmetric)
and PMICalculator.compute_pmi_matrix, timed in three parts that each end in a device synchronise or a copy to the host:
``host`` (tokenising, interning, the vocabulary, the id rows), ``count`` (snx.cooc.cooccurrence and the copy of the CSR to
the host) and ``pmi_matrix``.  One JSON line per size; nothing is asserted about speed."""
import argparse
import importlib.util
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

TERMS = 120000


def synth(n_docs: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    weights = 1.0 / np.arange(1, TERMS + 1) ** 1.1
    cum = np.cumsum(weights / weights.sum())
    words = np.array([f"w{i}" for i in range(TERMS)])
    docs = []
    for _ in range(n_docs):
        parts = []
        for _ in range(int(rng.integers(3, 7))):
            ids = np.searchsorted(cum, rng.random(int(rng.integers(8, 25))))
            parts.append(" ".join(words[np.minimum(ids, TERMS - 1)]) + ".!?"[int(rng.integers(0, 3))])
        docs.append(" ".join(parts))
    return docs


def gpu_run(docs, window_type: str, device: str):
    import torch
    from snx import cooc
    from src.pmi import CooccurrenceConfig, CooccurrenceMatrixBuilder, PMICalculator, WindowType
    cfg = CooccurrenceConfig(window_type=WindowType(window_type))
    out = {}
    for part in (docs[:2000], docs):                          # a small first pass warms up
        b = CooccurrenceMatrixBuilder(cfg, device=device)
        t0 = time.perf_counter()
        ptr, ids, w = b.prepare(part)
        t1 = time.perf_counter()
        V = len(b.get_vocabulary())
        csr = cooc.cooccurrence(ptr, ids, V, window_size=w, symmetric=cfg.symmetric, normalize=cfg.normalize, device=device)
        data, indices, indptr = csr.numpy()
        t2 = time.perf_counter()
        calc = PMICalculator(csr, b.get_term_frequencies(), b.get_vocabulary(), csr.total_windows, device=device)
        t3 = time.perf_counter()
        m = calc.compute_pmi_matrix()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        out = {"vocab": V, "windows": csr.total_windows, "tokens": int(ptr[-1]), "nnz": csr.nnz,
               "host_s": round(t1 - t0, 3), "count_s": round(t2 - t1, 3), "fit_s": round(t2 - t0, 3),
               "pmi_matrix_s": round(t4 - t3, 3)}
        del b, csr, calc, m
        torch.cuda.empty_cache()
    return out


def restatement_run(docs, window_type: str):
    from tests import pmi_reference as R
    t0 = time.perf_counter()
    vocab, tf, _, rows, w = R.build(docs, window_type, 10, 5, TERMS)
    indptr, indices, data, _, total = R.cooccurrence(rows, len(vocab), w, True, False)
    t1 = time.perf_counter()
    marg, tot = R.marginals_total(vocab, tf, data, 0.75)
    row = np.repeat(np.arange(len(vocab)), np.diff(indptr))
    for i in range(indices.size):
        R.pmi_cell(data[i], marg[row[i]], marg[indices[i]], tot, len(vocab), 1.0, True, 2.0, 1)
    t2 = time.perf_counter()
    return {"what": "the restatement's loops (tests/pmi_reference.py)", "vocab": len(vocab), "windows": total,
            "nnz": int(indices.size), "fit_s": round(t1 - t0, 3), "pmi_matrix_s": round(t2 - t1, 3)}


def reference_run(docs, window_type: str, root: str):
    for pkg in ("src", "src.pmi"):
        mod = types.ModuleType(pkg)
        mod.__path__ = []
        sys.modules[pkg] = mod
    mods = {}
    for leaf in ("cooccurrence", "pmi_calculator"):
        spec = importlib.util.spec_from_file_location(f"src.pmi.{leaf}", os.path.join(root, "src", "pmi", f"{leaf}.py"))
        mods[leaf] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[leaf]
        spec.loader.exec_module(mods[leaf])
    co, pc = mods["cooccurrence"], mods["pmi_calculator"]
    t0 = time.perf_counter()
    b = co.CooccurrenceMatrixBuilder(co.CooccurrenceConfig(window_type=co.WindowType(window_type)))
    b.fit(docs, show_progress=False)
    t1 = time.perf_counter()
    calc = pc.PMICalculator(b.get_cooccurrence_matrix(), b.get_term_frequencies(), b.get_vocabulary(),
                            b.get_stats().total_windows)
    t2 = time.perf_counter()
    calc.compute_pmi_matrix()
    t3 = time.perf_counter()
    return {"what": "the reference's CooccurrenceMatrixBuilder and compute_pmi_matrix", "vocab": len(b.get_vocabulary()),
            "windows": b.get_stats().total_windows, "nnz": b.get_stats().total_cooccurrences,
            "fit_s": round(t1 - t0, 3), "pmi_matrix_s": round(t3 - t2, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=str, default="2000,100000,640000", help="GPU sizes; empty: no GPU side")
    ap.add_argument("--cpu-docs", type=int, default=2000, help="0: no CPU side")
    ap.add_argument("--window-type", choices=("sentence", "paragraph", "sliding"), default="sentence")
    ap.add_argument("--reference", type=str, default=None, help="time the reference's own loop instead of the restatement's")
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    sizes = [int(x) for x in args.docs.split(",") if x]
    docs = synth(max(sizes + [args.cpu_docs]))
    if sizes:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("gpu_pmi_bench: the GPU side needs a GPU (--docs '' times the CPU side alone)")
    for n in sizes:
        print(json.dumps({"bench": "pmi_gpu", "docs": n, "window_type": args.window_type,
                          **gpu_run(docs[:n], args.window_type, args.device)}), flush=True)
    if args.cpu_docs:
        run = reference_run(docs[:args.cpu_docs], args.window_type, args.reference) if args.reference else \
            restatement_run(docs[:args.cpu_docs], args.window_type)
        print(json.dumps({"bench": "pmi_cpu", "docs": args.cpu_docs, "window_type": args.window_type, **run}), flush=True)


if __name__ == "__main__":
    main()
