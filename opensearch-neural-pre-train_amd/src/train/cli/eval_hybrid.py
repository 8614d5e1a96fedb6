"""A checkpoint against the BM25 baseline and the hybrid rows of the reference's benchmark, offline
(snx.retrieval.Bm25Index / fuse_ranked).

    python -m src.train.cli.eval_hybrid --checkpoint outputs/train_v33/final_model --val-file data/val.jsonl \\
        [--sweep] [--dense-run dense.npz | --dense-embeddings emb.npz [--dense-index flat|flat2|graph --ef 0 --degree 32]]

One JSON line per method: ``sparse`` (the model's exact search), ``bm25`` (BM25 over the same token ids: the model's
tokenizer, the evaluator's truncation and vocabulary filter; not OpenSearch's analyzer) and ``bm25_sparse_rrf``.
``--sweep`` adds the reference's grid over BM25 + sparse (ref:benchmark/hybrid_searcher.py:575-620): linear alpha 0.3 /
0.4 / 0.5 and weighted RRF 0.4 / 0.6.  ``--dense-run`` takes a dense retriever's top lists produced elsewhere -- an .npz
with ``docs`` int [nq, R] (ids in the evaluator's doc order, -1: unused) and ``scores`` float [nq, R] -- and adds
``dense``, ``bm25_dense_rrf``, ``dense_sparse_rrf`` and ``triple_rrf``: the seven rows of
ref:scripts/run_7way_benchmark.py (the dense encoder itself is not part of this project).  ``--dense-embeddings`` takes
the embeddings instead -- an .npz with ``docs`` fp32 [nd, D] and ``queries`` fp32 [nq, D] in the evaluator's corpus order
-- and runs the reference's SemanticSearcher (inner product, ref:benchmark/searchers.py:97-127) here, exactly, on
snx.retrieval.DenseIndex at the retrieval depth; the two flags exclude each other.  ``--dense-index graph`` searches an
snx.retrieval.GraphIndex instead (``--degree`` links per doc, a beam of ``--ef`` entries, 0: max(100, retrieval depth)),
the approximate search in the role of the reference's HNSW field (ref:benchmark/index_manager.py:98-110; not FAISS's
graph); its ``dense`` line also carries ``recall_vs_exact@10`` and ``recall_vs_exact@depth`` against the flat search of the
same run and ``mean_iterations``.  ``--dense-index flat2`` is the flat search through a bf16 first pass
(``DenseIndex.search_two_phase(exact=True)``): the same lists bit for bit, and the ``dense`` line adds
``certified_fraction``, the share of the queries whose list the first pass alone proved exact.  Every retriever contributes
its top 100 (--retrieval-k) and a fused list returns the top 10.  Each line carries the metrics, the mean union size of
fused rows and the paired t-test against ``bm25``.  One process (not torchrun)."""
from __future__ import annotations

import argparse
import json
from typing import List, Optional, Tuple

RRF_K = 60                   # ref:benchmark/hybrid_searcher.py:621-631
RETRIEVAL_K = 100
SWEEP = [("bm25_sparse_linear_0.3", "linear", {"alpha": 0.3}), ("bm25_sparse_linear_0.4", "linear", {"alpha": 0.4}),
         ("bm25_sparse_linear_0.5", "linear", {"alpha": 0.5}),
         ("bm25_sparse_weighted_rrf", "weighted_rrf", {"k": RRF_K, "weights": (0.4, 0.6)})]


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="BM25 baseline and hybrid rank fusion against exact sparse retrieval (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--checkpoint", type=str, default=None,
                    help="checkpoint directory holding model.pt, or a model.pt file (default: random init)")
    ap.add_argument("--model-name", type=str, default="skt/A.X-Encoder-base")
    ap.add_argument("--tokenizer", type=str, default=None, help="tokenizer dir or hash:<vocab> (default: --model-name)")
    ap.add_argument("--val-file", type=str, default="data/v29.0_kd/val.jsonl")
    ap.add_argument("--max-queries", type=int, default=2000)
    ap.add_argument("--max-docs", type=int, default=50000)
    ap.add_argument("--query-max-length", type=int, default=64)
    ap.add_argument("--doc-max-length", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--retrieval-k", type=int, default=RETRIEVAL_K, help="depth of every retriever's list")
    ap.add_argument("--rrf-k", type=float, default=RRF_K)
    ap.add_argument("--k1", type=float, default=1.2)
    ap.add_argument("--b", type=float, default=0.75)
    ap.add_argument("--sweep", action="store_true", help="the reference's linear / weighted-RRF grid over BM25 + sparse")
    ap.add_argument("--dense-run", type=str, default=None, help=".npz with docs [nq, R] and scores [nq, R] of a dense run")
    ap.add_argument("--dense-embeddings", type=str, default=None,
                    help=".npz with docs [nd, D] and queries [nq, D] (fp32, corpus order): the dense search runs here")
    ap.add_argument("--dense-index", choices=("flat", "flat2", "graph"), default="flat",
                    help="how --dense-embeddings is searched: exactly, exactly through a bf16 first pass, or through the "
                         "graph index")
    ap.add_argument("--ef", type=int, default=0, help="graph: beam entries (0: max(100, --retrieval-k))")
    ap.add_argument("--degree", type=int, default=32, help="graph: links per doc (even)")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON lines to this file")
    args = ap.parse_args(argv)
    if args.dense_run and args.dense_embeddings:
        ap.error("--dense-run and --dense-embeddings exclude each other")
    if not 1 <= args.retrieval_k <= 1024:
        ap.error("--retrieval-k must lie in [1, 1024]")
    if args.dense_index != "flat" and not args.dense_embeddings:
        ap.error(f"--dense-index {args.dense_index} needs --dense-embeddings")
    if not (args.ef == 0 or args.retrieval_k <= args.ef <= 1024) or not 2 <= args.degree <= 64 or args.degree % 2:
        ap.error("need --ef 0 or --retrieval-k <= --ef <= 1024, and an even --degree in [2, 64]")
    if not args.rrf_k >= 0 or not args.k1 >= 0 or not 0 <= args.b <= 1:
        ap.error("need --rrf-k >= 0, --k1 >= 0 and --b in [0, 1]")
    return args


def rows(args: argparse.Namespace) -> List[Tuple[str, Optional[str], dict, Tuple[str, ...]]]:
    """[(name, fusion method | None, its parameters, the retrievers in list order)] in print order."""
    rrf = {"k": args.rrf_k}
    out = [("sparse", None, {}, ("sparse",)), ("bm25", None, {}, ("bm25",)),
           ("bm25_sparse_rrf", "rrf", rrf, ("bm25", "sparse"))]
    if args.sweep:
        out += [(name, method, dict(params), ("bm25", "sparse")) for name, method, params in SWEEP]
    if args.dense_run or args.dense_embeddings:
        out += [("dense", None, {}, ("dense",)), ("bm25_dense_rrf", "rrf", rrf, ("bm25", "dense")),
                ("dense_sparse_rrf", "rrf", rrf, ("dense", "sparse")),
                ("triple_rrf", "rrf", rrf, ("bm25", "dense", "sparse"))]       # ref:benchmark/hybrid_searcher.py:517-521
    return out


def load_dense_run(path: str, nq: int, nd: int, depth: int, device):
    """-> (docs int32 [nq, R'], scores fp32 [nq, R'], R' = min(R, depth)) on ``device``; ids outside [0, nd) end a list."""
    import numpy as np
    import torch
    z = np.load(path)
    docs, scores = np.asarray(z["docs"]), np.asarray(z["scores"])
    if docs.ndim != 2 or docs.shape != scores.shape or docs.shape[0] != nq or docs.shape[1] < 1:
        raise ValueError(f"{path}: docs and scores must both be [{nq}, R]")
    docs = np.where((docs >= 0) & (docs < nd), docs, -1)[:, :depth].astype(np.int32)
    return torch.from_numpy(docs).to(device), torch.from_numpy(scores[:, :depth].astype(np.float32)).to(device)


def list_recall(docs, exact, k: int) -> float:
    """Mean share of the first ``k`` docs of every ``exact`` list that the same query's ``docs`` list holds in its first
    ``k``; a query without an exact doc counts as 1."""
    import torch
    a, b = docs[:, :k].long(), exact[:, :k].long()
    if not b.shape[0]:
        return 1.0
    hit = ((b[:, :, None] == a[:, None, :]) & (b[:, :, None] >= 0)).any(2).sum(1).double()
    want = (b >= 0).sum(1).double()
    return float(torch.where(want > 0, hit / want.clamp(min=1), torch.ones_like(want)).mean())


def search_dense_embeddings(path: str, nq: int, nd: int, depth: int, device, dense_index: str = "flat", ef: int = 0,
                            degree: int = 32):
    """The dense top lists from embeddings -> (docs int32 [nq, depth], scores fp32 [nq, depth], extra fields of the
    ``dense`` line) on ``device`` (unused slots -1 / 0 when depth > nd).  ``flat``: an exact inner-product search of every
    query over every doc.  ``flat2``: the same lists from ``search_two_phase(exact=True)``; the extra field is the
    certified fraction.  ``graph``: snx.retrieval.GraphIndex with ``degree`` links and a beam of ``ef`` entries (0:
    max(100, depth)); the extra fields are its recall against the flat lists and the mean iteration count."""
    import numpy as np
    import torch
    from snx.retrieval import DenseIndex, GraphIndex
    z = np.load(path)
    docs, queries = np.asarray(z["docs"]), np.asarray(z["queries"])
    if docs.ndim != 2 or queries.ndim != 2 or docs.shape[0] != nd or queries.shape != (nq, docs.shape[1]):
        raise ValueError(f"{path}: need docs [{nd}, D] and queries [{nq}, D]")
    index = DenseIndex(int(docs.shape[1]), device)
    index.add(torch.from_numpy(np.ascontiguousarray(docs, dtype=np.float32)).to(device))
    index.build()
    q = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).to(device)
    if dense_index == "flat2":
        scores, ids, cert = index.search_two_phase(q, depth, exact=True)
        return ids, scores, {"dense_index": "flat2", "certified_fraction": float(cert.double().mean()) if nq else 0.0}
    scores, ids, _, _ = index.search(q, depth)
    if dense_index == "flat":
        return ids, scores, {}
    ef = ef or max(100, depth)
    graph = GraphIndex(int(docs.shape[1]), device, degree=degree, knn=2 * degree, ef=ef)
    graph.add(index.emb)
    graph.build()
    g_scores, g_ids = graph.search(q, depth)
    extra = {"dense_index": "graph", "ef": ef, "degree": degree, "recall_vs_exact@10": list_recall(g_ids, ids, 10),
             f"recall_vs_exact@{depth}": list_recall(g_ids, ids, depth),
             "mean_iterations": float(graph.last_iterations.double().mean()) if nq else 0.0}
    return g_ids, g_scores, extra


def list_ranks(docs, targets):
    """1-based position of each query's target in its list (the list ends at the first negative id), 0 = absent."""
    import torch
    live = torch.cumsum((docs < 0).int(), 1) == 0
    hit = live & (docs == targets[:, None].to(docs.dtype))
    pos = torch.argmax(hit.int(), 1) + 1
    return torch.where(hit.any(1), pos, torch.zeros_like(pos)).cpu().tolist()


def main(argv: Optional[List[str]] = None) -> List[dict]:
    args = parse_args(argv)
    import torch
    from snx.retrieval import fuse_ranked
    from src.train.cli.mine_negatives import load_model
    from src.train.data.collator import create_tokenizer
    from src.train.eval import (RETRIEVAL_SIZE, MidTrainingEvaluator, bm25_index, hybrid_params, metrics_from_ranks,
                                paired_t_test)
    device = torch.device("cuda:0")
    tokenizer = create_tokenizer(args.tokenizer or args.model_name)
    model = load_model(args, device)
    ev = MidTrainingEvaluator(tokenizer, args.val_file, max_queries=args.max_queries, max_docs=args.max_docs,
                              device=str(device), query_max_length=args.query_max_length,
                              doc_max_length=args.doc_max_length, batch_size=args.batch_size)
    index, queries = ev.encode(model)
    if queries is None:
        raise ValueError(f"{args.val_file}: no queries or no docs to evaluate")
    nq, nd, depth = len(ev.corpus.queries), len(ev.corpus.docs), args.retrieval_k
    targets = torch.tensor(ev.corpus.targets, dtype=torch.int32, device=device)
    bm, bm_queries = bm25_index(ev, index.V, hybrid_params({"k1": args.k1, "b": args.b}))
    found = {}                                                   # retriever -> (docs, scores) at the retrieval depth
    s, d, _, _ = index.search(*queries, depth)
    found["sparse"] = (d, s)
    s, d, _, _ = bm.index.search(*bm_queries, depth)
    found["bm25"] = (d, s)
    if args.dense_run:
        found["dense"] = load_dense_run(args.dense_run, nq, nd, depth, device)
    dense_extra = {}
    if args.dense_embeddings:
        d, s, dense_extra = search_dense_embeddings(args.dense_embeddings, nq, nd, depth, device, args.dense_index,
                                                    args.ef, args.degree)
        found["dense"] = (d, s)
    ranks, totals = {}, {}
    for name, method, params, members in rows(args):
        if method is None:
            ranks[name] = list_ranks(found[members[0]][0], targets)
        else:
            same = max(found[m][0].shape[1] for m in members)    # lists of one width: pad with unused slots
            lists = [(torch.nn.functional.pad(found[m][0], (0, same - found[m][0].shape[1]), value=-1),
                      torch.nn.functional.pad(found[m][1], (0, same - found[m][1].shape[1]))) for m in members]
            _, _, rank, total = fuse_ranked(lists, method, RETRIEVAL_SIZE, targets=targets, **params)
            ranks[name], totals[name] = rank.cpu().tolist(), float(total.double().mean())
    lines = []
    out = open(args.out, "w") if args.out else None
    try:
        for name, method, params, members in rows(args):
            t = paired_t_test(ranks[name], ranks["bm25"])
            line = dict(method=name, fusion=method, retrievers=list(members), num_queries=nq, num_docs=nd,
                        retrieval_k=depth, **{k: (list(v) if isinstance(v, tuple) else v) for k, v in params.items()},
                        **metrics_from_ranks(ranks[name]))
            if method is not None:
                line["total"] = totals[name]
            if name == "dense":
                line.update(dense_extra)
            # json has no nan: a t-test without variation (bm25 against itself) is written as null
            line.update(vs_bm25_statistic=None if t["statistic"] != t["statistic"] else t["statistic"],
                        vs_bm25_p=None if t["p_value"] != t["p_value"] else t["p_value"],
                        vs_bm25_significant=t["significant"])
            lines.append(line)
            text = json.dumps(line)
            print(text, flush=True)
            if out:
                out.write(text + "\n")
    finally:
        if out:
            out.close()
    return lines


if __name__ == "__main__":
    main()
