"""Mid-training retrieval evaluation: ``MidTrainingEvaluator``.

The reference CLI imports this class (ref:src/train/cli/train_v33_ddp.py:46-49, built at :629-644, run every 5 epochs at
:679-697) from a module that is absent from the reference tree.  Here it is built on the native path: the model's own
forward encodes a small fixed corpus taken from the validation triplets, ``ops.sparse_topk`` applies the inference
encoder's vocabulary filter on the device, and ``snx.retrieval.SparseIndex`` scores every query against every doc
exactly on the GPU.  The metrics are those of ref:benchmark/metrics.py:52-99 over single-target hit ranks.

Scoring is the plain dot product of the sparse vectors -- SPLADE's own score and that of OpenSearch's ``neural_sparse``
query -- not the saturation function of the ``rank_feature`` query the reference benchmark's searcher sends
(ref:benchmark/searchers.py:155-188).  Ties rank the lower doc id first.

``load_benchmark_dir``, ``qrels_metrics`` and ``bootstrap_confidence_interval`` score a benchmark directory with qrels
(several relevant docs per query) the way the reference's benchmark runner does; the evaluator above keeps its
single-positive protocol."""
from __future__ import annotations

import logging
from dataclasses import dataclass
from itertools import islice
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

logger = logging.getLogger(__name__)

RETRIEVAL_SIZE = 10          # ref:benchmark/config.py:44
QUERY_TOP_K = 64             # NeuralSparseSearcher's query encoding, ref:benchmark/searchers.py:161
METRIC_KEYS = ("recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10")


@dataclass
class EvalCorpus:
    queries: List[str]
    docs: List[str]
    targets: List[int]          # doc id of each query's positive
    forced: int                 # positives kept although the corpus already held max_docs docs


def _negatives(rec: dict) -> List[str]:
    negs = rec.get("negatives")
    if isinstance(negs, list):
        return [n for n in negs if isinstance(n, str)]
    neg = rec.get("negative")
    return [neg] if isinstance(neg, str) else []


def build_eval_corpus(records: Iterable[dict], max_queries: int, max_docs: int) -> EvalCorpus:
    """The first ``max_queries`` records are the queries.  Docs: their positives, then their negatives, then positives and
    negatives of later records, up to ``max_docs``; deduplicated by exact text (first occurrence keeps the id).  Every
    chosen query's positive is in the corpus even past ``max_docs``; it is the query's one relevant doc."""
    it = iter(records)
    chosen = list(islice(it, max(0, int(max_queries))))
    docs: List[str] = []
    ids: Dict[str, int] = {}

    def add(text: str, force: bool = False) -> Optional[int]:
        if text in ids:
            return ids[text]
        if not force and len(docs) >= max_docs:
            return None
        ids[text] = len(docs)
        docs.append(text)
        return ids[text]

    targets, forced = [], 0
    for rec in chosen:
        if rec["positive"] not in ids and len(docs) >= max_docs:
            forced += 1
        targets.append(add(rec["positive"], force=True))
    for rec in chosen:
        for n in _negatives(rec):
            add(n)
    for rec in it:
        if len(docs) >= max_docs:
            break
        add(rec["positive"])
        for n in _negatives(rec):
            add(n)
    return EvalCorpus([rec["query"] for rec in chosen], docs, targets, forced)


def metrics_from_ranks(ranks: Sequence[int], k: int = RETRIEVAL_SIZE) -> Dict[str, float]:
    """Full 1-based target ranks (0 = score 0, a miss) -> recall@1/5/10, mrr@10, ndcg@10 with the formulas of
    ref:benchmark/metrics.py:52-99 over the top-``k`` retrieval (a target ranked below ``k`` is not retrieved)."""
    hit = [int(r) if 1 <= int(r) <= k else None for r in ranks]
    n = len(hit)
    out = {f"recall@{c}": (sum(1 for h in hit if h is not None and h <= c) / n if n else 0.0) for c in (1, 5, 10)}
    rr = [1.0 / h if h is not None else 0.0 for h in hit]
    out["mrr@10"] = float(np.mean(rr)) if rr else 0.0
    idcg = 1.0
    nd = [(1.0 / np.log2(h + 1)) / idcg if h is not None and h <= 10 else 0.0 for h in hit]
    out["ndcg@10"] = float(np.mean(nd)) if nd else 0.0
    return out


def _idf_tensor(query_idf) -> Optional[torch.Tensor]:
    if query_idf is None:
        return None
    return torch.as_tensor(query_idf, dtype=torch.float32).detach().contiguous()


def cat_query_rows(batches):
    """(vals, ids, cnt) batches -> one triple.  IDF rows are as wide as their batch is long, so the batches are padded to
    one width first (weight 0, id -1 in the unused slots); batches of one width are joined as they are."""
    cap = max(b[0].shape[1] for b in batches)
    pad = lambda x, v: torch.nn.functional.pad(x, (0, cap - x.shape[1]), value=v)   # noqa: E731
    return (torch.cat([pad(b[0], 0.0) for b in batches]), torch.cat([pad(b[1], -1) for b in batches]),
            torch.cat([b[2] for b in batches]))


class MidTrainingEvaluator:
    """Retrieval quality of the model being trained, on a fixed corpus built from ``val_file`` (a triplet JSONL read by
    ``load_training_data``, or ``synthetic:N[:k]``).  ``evaluate(model)`` -> recall@1/5/10, mrr@10, ndcg@10,
    num_queries, num_docs, avg_nnz_q, avg_nnz_d; with ``seismic`` / ``two_phase`` / ``hybrid`` (parameter dicts, see
    seismic_params / two_phase_params / hybrid_params) also the seismic_* / two_phase_* keys of seismic_eval /
    two_phase_eval and the bm25_* / hybrid_* / *_p keys of hybrid_eval (BM25 under the same tokenizer, BM25 + sparse
    fusion, paired t-tests).  Queries keep their top
    64 terms, docs every term that survives the inference encoder's filter (ref:benchmark/indexer.py:59); retrieval
    size 10.  ``query_idf`` ([V] fp32): doc-only mode -- the queries are not encoded, their rows are idf[token] once per
    distinct kept token (snx.idf.idf_query_rows), the way OpenSearch queries an inference-free model; docs unchanged."""

    def __init__(self, tokenizer, val_file: str, max_queries: int = 200, max_docs: int = 1000, device: str = "cuda",
                 query_max_length: int = 64, doc_max_length: int = 256, batch_size: int = 64,
                 seismic: Optional[dict] = None, two_phase: Optional[dict] = None, hybrid: Optional[dict] = None,
                 query_idf=None):
        from benchmark.encoders import special_token_ids
        from src.train.data import load_training_data
        self.query_idf = _idf_tensor(query_idf)
        self.seismic = seismic_params(seismic) if seismic is not None else None
        self.two_phase = two_phase_params(two_phase) if two_phase is not None else None
        self.hybrid = hybrid_params(hybrid) if hybrid is not None else None
        self._bm25 = None                    # (Bm25Index, query rows): the corpus is fixed, built once per evaluator
        self.tokenizer = tokenizer
        self.device = torch.device(device)
        self.query_max_length, self.doc_max_length = int(query_max_length), int(doc_max_length)
        self.batch_size = max(1, int(batch_size))
        ds = load_training_data([val_file])
        self.corpus = build_eval_corpus((ds[i] for i in range(len(ds))), max_queries, max_docs)
        if self.corpus.forced:
            logger.info(f"eval corpus: {self.corpus.forced} query positive(s) kept past max_docs={max_docs} "
                        f"({len(self.corpus.docs)} docs)")
        self._token_lookup = list(tokenizer.convert_ids_to_tokens(list(range(tokenizer.vocab_size))))
        self._special = special_token_ids(tokenizer)
        self._allowed: Optional[torch.Tensor] = None
        self.last_ranks: Optional[List[int]] = None
        logger.info(f"eval corpus: {len(self.corpus.queries)} queries, {len(self.corpus.docs)} docs from {val_file}")

    def _allowed_mask(self, V: int) -> torch.Tensor:
        from benchmark.encoders import allowed_token_mask
        if self._allowed is None or self._allowed.numel() != V:
            self._allowed = allowed_token_mask(self._token_lookup, self._special, V).to(self.device)
        return self._allowed

    def _encode(self, model, texts: List[str], max_length: int, top_k: Optional[int]):
        """Batches of (vals, ids, cnt) from ops.sparse_topk over the model's sparse_repr."""
        from snx import ops
        for s in range(0, len(texts), self.batch_size):
            enc = self.tokenizer(texts[s:s + self.batch_size], padding=True, truncation=True, max_length=max_length,
                                 return_tensors="pt")
            rep, _ = model(enc["input_ids"].to(self.device), enc["attention_mask"].to(self.device))
            rep = rep.float().contiguous()
            vals, ids, cnt, _ = ops.sparse_topk(rep, self._allowed_mask(rep.shape[1]),
                                                None if top_k is None else min(top_k, rep.shape[1]))
            yield vals, ids, cnt

    def _idf_queries(self, V: int):
        """Batches of (vals, ids, cnt) query rows from the token ids alone: idf[token], the model is not run."""
        from snx.idf import idf_query_rows
        idf = self.query_idf.to(self.device)
        if idf.numel() != V:
            raise ValueError(f"query_idf holds {idf.numel()} entries, the model's vocabulary {V}")
        for s in range(0, len(self.corpus.queries), self.batch_size):
            enc = self.tokenizer(self.corpus.queries[s:s + self.batch_size], padding=True, truncation=True,
                                 max_length=self.query_max_length, return_tensors="pt")
            yield idf_query_rows(enc["input_ids"].to(self.device), enc["attention_mask"].to(self.device),
                                 self._allowed_mask(V), idf)

    def encode(self, model):
        """The corpus through ``model`` -> (SparseIndex over the docs, built when there are queries, or None; the query
        rows (vals, ids, cnt) or None).  The model's training mode is restored."""
        from snx.retrieval import SparseIndex
        c = self.corpus
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                index = None
                for vals, ids, cnt in self._encode(model, c.docs, self.doc_max_length, None):
                    if index is None:
                        index = SparseIndex(vals.shape[1], self.device)
                    index.add(vals, ids, cnt)
                if getattr(self, "query_idf", None) is not None and index is not None:
                    qb = list(self._idf_queries(index.V))
                else:
                    qb = list(self._encode(model, c.queries, self.query_max_length, QUERY_TOP_K))
                queries = None
                if qb and index is not None:
                    index.build()
                    queries = cat_query_rows(qb)
        finally:
            model.train(was_training)
        return index, queries

    def evaluate(self, model) -> Dict[str, float]:
        c = self.corpus
        index, queries = self.encode(model)
        ranks: List[int] = []
        avg_q = 0.0
        extra: Dict[str, float] = {}
        if queries is not None:
            targets = torch.tensor(c.targets, dtype=torch.int32, device=self.device)
            _, docs, rank, _ = index.search(*queries, RETRIEVAL_SIZE, targets=targets)
            ranks = rank.cpu().tolist()
            avg_q = float(queries[2].double().mean())
            if self.seismic is not None:
                extra = seismic_eval(index, queries, targets, docs, self.seismic)[0]
            if self.two_phase is not None:
                extra.update(two_phase_eval(index, queries, targets, docs, self.two_phase)[0])
            if self.hybrid is not None:
                if self._bm25 is None:
                    self._bm25 = bm25_index(self, index.V, self.hybrid)
                extra.update(hybrid_eval(index, queries, targets, *self._bm25, self.hybrid)[0])
        else:
            if self.seismic is not None:
                extra = {f"seismic_{k}": 0.0 for k in METRIC_KEYS + ("overlap@5", "postings_frac")}
            if self.two_phase is not None:
                extra.update({f"two_phase_{k}": 0.0 for k in METRIC_KEYS + ("overlap@5", "postings_frac")})
            if self.hybrid is not None:
                extra.update({k: 0.0 for k in HYBRID_KEYS})
        avg_d = index.nnz / index.num_docs if index is not None and index.num_docs else 0.0
        self.last_ranks = ranks
        out = metrics_from_ranks(ranks)
        out.update(num_queries=float(len(c.queries)), num_docs=float(len(c.docs)), avg_nnz_q=avg_q, avg_nnz_d=avg_d)
        out.update(extra)
        return out


SEISMIC_DEFAULTS = {"n_postings": 300, "cluster_ratio": 0.1, "summary_prune_ratio": 0.4, "top_n": 10,
                    "heap_factor": 1.0}


def seismic_params(p: dict) -> dict:
    """The five SEISMIC parameters (snx.retrieval.SeismicIndex), missing ones at their defaults."""
    bad = set(p) - set(SEISMIC_DEFAULTS)
    if bad:
        raise ValueError(f"seismic: unknown parameter(s) {sorted(bad)}; known: {list(SEISMIC_DEFAULTS)}")
    return {**SEISMIC_DEFAULTS, **p}


def overlap_at(ann_docs, exact_docs, k: int = 5) -> float:
    """ref:scripts/neural_sparse_search_aws.py:1205-1215 (_recall_at_k), averaged over queries: |ANN top k & exact top
    k| / |exact top k|, 0 for a query whose exact list is empty.  Rows are doc ids, -1 = unused slot."""
    vals = []
    for a, e in zip(np.asarray(ann_docs), np.asarray(exact_docs)):
        es = {int(d) for d in e[:k] if d >= 0}
        vals.append(len(es & {int(d) for d in a[:k] if d >= 0}) / len(es) if es else 0.0)
    return float(np.mean(vals)) if vals else 0.0


def cut_postings(index, queries, top_n: int) -> torch.Tensor:
    """int64 [nq]: postings of the exact index under each query's top_n terms by (weight desc, term asc)."""
    vals, ids, cnt = queries
    live = torch.arange(vals.shape[1], device=vals.device)[None, :] < cnt.long()[:, None]
    key = torch.where(live, ids.long(), torch.full_like(ids, index.V, dtype=torch.long))
    o1 = torch.sort(key, dim=1, stable=True)[1]
    w1 = torch.where(torch.gather(live, 1, o1), torch.gather(vals, 1, o1), torch.zeros_like(vals))
    o2 = torch.sort(-w1, dim=1, stable=True)[1]
    t = torch.gather(torch.gather(ids.long(), 1, o1), 1, o2)[:, :top_n]
    ok = torch.gather(torch.gather(live, 1, o1), 1, o2)[:, :top_n]
    lens = index.term_ptr[t.clamp(0, index.V - 1) + 1] - index.term_ptr[t.clamp(0, index.V - 1)]
    return torch.where(ok, lens, torch.zeros_like(lens)).sum(1)


def seismic_eval(index, queries, targets, exact_docs, params: dict, six=None):
    """SEISMIC over the exact index's corpus -> (metrics, info).  metrics: seismic_recall@1/5/10, seismic_mrr@10,
    seismic_ndcg@10 (the ANN ranks), seismic_overlap@5 (against ``exact_docs``), seismic_postings_frac (docs scored over
    the exact postings of the Q_cut terms, summed over queries).  info: the SeismicIndex, build_s, search_s and the
    counters' means.  ``six``: an index already built with ``params``' index settings."""
    import time
    from snx.retrieval import SeismicIndex
    p = seismic_params(params)
    if six is None:
        six = SeismicIndex(index, p["n_postings"], p["cluster_ratio"], p["summary_prune_ratio"])
    torch.cuda.synchronize(index.device)
    t0 = time.perf_counter()
    _, docs, rank, _, stats = six.search(*queries, RETRIEVAL_SIZE, top_n=p["top_n"], heap_factor=p["heap_factor"],
                                         targets=targets)
    torch.cuda.synchronize(index.device)
    search_s = time.perf_counter() - t0
    out = {f"seismic_{k}": v for k, v in metrics_from_ranks(rank.cpu().tolist()).items()}
    out["seismic_overlap@5"] = overlap_at(docs.cpu().numpy(), exact_docs.cpu().numpy(), 5)
    total = int(cut_postings(index, queries, p["top_n"]).sum())
    out["seismic_postings_frac"] = float(stats["postings_scored"].sum()) / total if total else 0.0
    info = {"index": six, "build_s": six.build_seconds, "search_s": search_s}
    info.update({k: float(v.double().mean()) for k, v in stats.items()})
    return out, info


# OpenSearch's neural_sparse_two_phase_processor as the reference configures it (ref:benchmark/index_manager.py:197-238)
TWO_PHASE_DEFAULTS = {"prune_type": "max_ratio", "prune_value": 0.4, "expansion_rate": 5.0, "max_window_size": 10000}


def two_phase_params(p: dict) -> dict:
    """The four two-phase parameters (snx.retrieval.SparseIndex.search_two_phase), missing ones at their defaults."""
    bad = set(p) - set(TWO_PHASE_DEFAULTS)
    if bad:
        raise ValueError(f"two_phase: unknown parameter(s) {sorted(bad)}; known: {list(TWO_PHASE_DEFAULTS)}")
    return {**TWO_PHASE_DEFAULTS, **p}


def two_phase_eval(index, queries, targets, exact_docs, params: dict, doc_prune=None):
    """Two-phase search over the exact index's corpus -> (metrics, info).  metrics: two_phase_recall@1/5/10,
    two_phase_mrr@10, two_phase_ndcg@10 (the two-phase ranks), two_phase_overlap@5 (against ``exact_docs``),
    two_phase_postings_frac (posting-list lengths under the Q_high terms over those under all query terms, summed over
    queries).  ``doc_prune`` = (prune_type, value): the search runs on ``index.pruned(...)`` (ingest-time pruning) and
    doc_postings_frac = pruned nnz / nnz is added.  info: the index searched, search_s and the counters' means."""
    import time
    p = two_phase_params(params)
    out = {}
    searched = index
    if doc_prune is not None:
        searched = index.pruned(*doc_prune)
        out["doc_postings_frac"] = searched.nnz / index.nnz if index.nnz else 0.0
    torch.cuda.synchronize(index.device)
    t0 = time.perf_counter()
    _, docs, rank, _, stats = searched.search_two_phase(*queries, RETRIEVAL_SIZE, targets=targets, **p)
    torch.cuda.synchronize(index.device)
    search_s = time.perf_counter() - t0
    out.update({f"two_phase_{k}": v for k, v in metrics_from_ranks(rank.cpu().tolist()).items()})
    out["two_phase_overlap@5"] = overlap_at(docs.cpu().numpy(), exact_docs.cpu().numpy(), 5)
    total = int(stats["postings_all"].sum())
    out["two_phase_postings_frac"] = float(stats["postings_high"].sum()) / total if total else 0.0
    info = {"index": searched, "search_s": search_s}
    info.update({k: float(v.double().mean()) for k, v in stats.items()})
    return out, info


# ---- BM25 baseline, hybrid fusion and the significance test (ref:benchmark/hybrid_searcher.py, ref:benchmark/metrics.py)
# fusion method, RRF constant, linear weight and per-retriever depth: ref:benchmark/hybrid_searcher.py:621-631; k1 / b:
# OpenSearch's BM25 defaults
HYBRID_DEFAULTS = {"method": "rrf", "k": 60, "alpha": 0.4, "retrieval_k": 100, "k1": 1.2, "b": 0.75}
HYBRID_KEYS = tuple(f"bm25_{k}" for k in METRIC_KEYS) + tuple(f"hybrid_{k}" for k in METRIC_KEYS) + \
    ("hybrid_total", "sparse_vs_bm25_p", "hybrid_vs_sparse_p")


def hybrid_params(p: dict) -> dict:
    """The six hybrid parameters (snx.retrieval.Bm25Index / fuse_ranked), missing ones at their defaults."""
    bad = set(p) - set(HYBRID_DEFAULTS)
    if bad:
        raise ValueError(f"hybrid: unknown parameter(s) {sorted(bad)}; known: {list(HYBRID_DEFAULTS)}")
    out = {**HYBRID_DEFAULTS, **p}
    if out["method"] not in ("rrf", "weighted_rrf", "linear"):
        raise ValueError(f"hybrid: unknown method {out['method']!r}")
    if not 1 <= int(out["retrieval_k"]) <= 1024:
        raise ValueError("hybrid: retrieval_k must be in [1, 1024]")
    return out


def fusion_kwargs(p: dict) -> dict:
    """The parameters ``fuse_ranked`` takes for ``p['method']``."""
    return {"alpha": p["alpha"]} if p["method"] == "linear" else {"k": p["k"]}


def _betacf(a: float, b: float, x: float) -> float:
    """Continued fraction of the incomplete beta function (modified Lentz), float64."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 10000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def betainc(a: float, b: float, x: float) -> float:
    """Regularised incomplete beta function I_x(a, b), float64 (continued fraction on the side where it converges fast)."""
    import math
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, 1.0 - x) / b


def paired_t_test(ranks_a: Sequence[int], ranks_b: Sequence[int], k: int = RETRIEVAL_SIZE) -> Dict[str, float]:
    """ref:benchmark/metrics.py:149-177 over target ranks: reciprocal hit ranks (a rank of 0 or above ``k`` is not
    retrieved and counts 0.0), then the paired two-sided t-test -> statistic, p_value, significant (p < 0.05).  The
    Student-t tail is I_{df / (df + t^2)}(df / 2, 1 / 2) with ``betainc`` above (no scipy).  Fewer than two pairs or all
    differences equal to 0: nan, not significant -- what the reference returns."""
    if len(ranks_a) != len(ranks_b):
        raise ValueError("Result lists must have same length for paired test")
    rr = [np.array([1.0 / int(r) if 1 <= int(r) <= k else 0.0 for r in ranks], np.float64) for ranks in (ranks_a, ranks_b)]
    d = rr[0] - rr[1]
    n = len(d)
    t, p = float("nan"), float("nan")
    if n >= 2:
        mean = float(np.mean(d))
        var = float(np.sum((d - np.mean(d)) ** 2) / (n - 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = float(np.float64(mean) / np.sqrt(np.float64(var) / n))
        if np.isfinite(t):
            df = float(n - 1)
            p = betainc(0.5 * df, 0.5, df / (df + t * t))
        elif not np.isnan(t):
            p = 0.0
    return {"statistic": t, "p_value": p, "significant": bool(p < 0.05)}


def bm25_index(ev: "MidTrainingEvaluator", V: int, params: dict):
    """The BM25 index over the evaluator's docs and the queries' rows (vals, ids, cnt), tokenized as the encoder sees them
    (the evaluator's truncation and vocabulary filter).  Independent of the model."""
    from snx.retrieval import Bm25Index
    bm = Bm25Index(V, ev.device, k1=params["k1"], b=params["b"])
    allowed = ev._allowed_mask(V)

    def batches(texts, max_length):
        for s in range(0, len(texts), ev.batch_size):
            enc = ev.tokenizer(texts[s:s + ev.batch_size], padding=True, truncation=True, max_length=max_length,
                               return_tensors="pt")
            yield enc["input_ids"].to(ev.device), enc["attention_mask"].to(ev.device)
    for ids, mask in batches(ev.corpus.docs, ev.doc_max_length):
        bm.add_tokens(ids, mask, allowed)
    bm.build()
    rows = [bm.query_rows(ids, mask, allowed) for ids, mask in batches(ev.corpus.queries, ev.query_max_length)]
    cap = max(r[0].shape[1] for r in rows)
    pad = lambda x: torch.nn.functional.pad(x, (0, cap - x.shape[1]))            # noqa: E731
    return bm, (torch.cat([pad(r[0]) for r in rows]), torch.cat([pad(r[1]) for r in rows]), torch.cat([r[2] for r in rows]))


def hybrid_eval(index, queries, targets, bm, bm_queries, params: dict):
    """BM25 and BM25 + sparse fusion over the exact index's corpus -> (metrics, info).  metrics: bm25_* and hybrid_* (the
    five METRIC_KEYS each: BM25's ranks; the ranks after fusing the two retrievers' top ``retrieval_k`` lists, list 0 =
    BM25, returning RETRIEVAL_SIZE), hybrid_total (mean union size), sparse_vs_bm25_p and hybrid_vs_sparse_p (paired
    t-tests over reciprocal hit ranks).  info: the rank lists and the two searches' (docs, scores) lists."""
    from snx.retrieval import fuse_ranked
    p = hybrid_params(params)
    rk = int(p["retrieval_k"])
    b_s, b_d, b_rank, _ = bm.index.search(*bm_queries, rk, targets=targets)
    s_s, s_d, s_rank, _ = index.search(*queries, rk, targets=targets)
    _, _, h_rank, total = fuse_ranked([(b_d, b_s), (s_d, s_s)], p["method"], RETRIEVAL_SIZE, targets=targets,
                                      **fusion_kwargs(p))
    ranks = {"bm25": b_rank.cpu().tolist(), "sparse": s_rank.cpu().tolist(), "hybrid": h_rank.cpu().tolist()}
    out = {f"bm25_{k}": v for k, v in metrics_from_ranks(ranks["bm25"]).items()}
    out.update({f"hybrid_{k}": v for k, v in metrics_from_ranks(ranks["hybrid"]).items()})
    out["hybrid_total"] = float(total.double().mean()) if total.numel() else 0.0
    out["sparse_vs_bm25_p"] = paired_t_test(ranks["sparse"], ranks["bm25"])["p_value"]
    out["hybrid_vs_sparse_p"] = paired_t_test(ranks["hybrid"], ranks["sparse"])["p_value"]
    return out, {"ranks": ranks, "bm25": (b_d, b_s), "sparse": (s_d, s_s)}


# ---- benchmarks with qrels: several relevant docs per query (ref:benchmark/hf_data_loader.py, ref:benchmark/hf_runner.py,
# ref:benchmark/metrics.py:180-215; snx.retrieval "relevance judgments")
QRELS_CUTOFFS = (1, 5, 10)
REPORT_KEYS = {"recall@1": "recall_at_1", "recall@5": "recall_at_5", "recall@10": "recall_at_10", "mrr": "mrr",
               "ndcg@10": "ndcg_at_10"}                      # the key names of ref:benchmark/metrics.py:36-49


@dataclass
class BenchmarkData:
    query_ids: List[str]
    queries: List[str]
    doc_ids: List[str]
    docs: List[str]
    titles: List[str]
    relevant: List[List[int]]   # per query: positions in ``docs`` of its relevant docs, ascending
    judged: List[int]           # per query: qrels with score > 0, those naming a doc outside the corpus included


def load_benchmark_dir(path: str, max_queries: Optional[int] = None) -> BenchmarkData:
    """A BEIR/MTEB-style directory -- ``corpus.jsonl`` (``_id``, ``text``, optional ``title``), ``queries.jsonl`` (``_id``,
    ``text``), ``qrels.jsonl`` (``query-id``, ``corpus-id``, ``score``) -- read by the rules of the reference's local
    loader (ref:benchmark/hf_data_loader.py:401-459): a qrel counts when ``score > 0``; the queries are those with a
    counting qrel, in order of first appearance in ``qrels.jsonl``; ``max_queries`` (None or 0: all) truncates that
    order; a corpus ``_id`` seen twice keeps its first position and its last text.  A relevant id that is not in the
    corpus is kept out of the query's row, but the query stays: it can then only miss."""
    import json
    import os
    doc_pos: Dict[str, int] = {}
    docs: List[str] = []
    titles: List[str] = []
    with open(os.path.join(path, "corpus.jsonl"), encoding="utf-8") as f:
        for line in f:
            if not line.strip():
                continue
            d = json.loads(line)
            i = doc_pos.setdefault(d["_id"], len(docs))
            if i == len(docs):
                docs.append(d["text"])
                titles.append(d.get("title", ""))
            else:
                docs[i], titles[i] = d["text"], d.get("title", "")
    text_of: Dict[str, str] = {}
    with open(os.path.join(path, "queries.jsonl"), encoding="utf-8") as f:
        for line in f:
            if line.strip():
                q = json.loads(line)
                text_of[q["_id"]] = q["text"]
    rel: Dict[str, List[str]] = {}
    with open(os.path.join(path, "qrels.jsonl"), encoding="utf-8") as f:
        for line in f:
            if line.strip():
                r = json.loads(line)
                if r["score"] > 0:
                    rel.setdefault(r["query-id"], []).append(r["corpus-id"])
    qids = list(rel)
    if max_queries:
        qids = qids[:max_queries]
    unknown = [q for q in qids if q not in text_of]
    if unknown:
        raise ValueError(f"{path}: qrels.jsonl names {len(unknown)} query id(s) that queries.jsonl lacks, first {unknown[0]!r}")
    rows = [sorted({doc_pos[d] for d in rel[q] if d in doc_pos}) for q in qids]
    return BenchmarkData(qids, [text_of[q] for q in qids], list(doc_pos), docs, titles, rows, [len(rel[q]) for q in qids])


class BenchmarkEvaluator(MidTrainingEvaluator):
    """The evaluator's encoding path (``encode``, and ``bm25_index`` over it) for a ``BenchmarkData`` instead of a
    validation file; ``relevant`` holds the qrels rows.  It does not score by itself: see src.train.cli.eval_benchmark."""

    def __init__(self, tokenizer, data: BenchmarkData, device: str = "cuda", query_max_length: int = 64,
                 doc_max_length: int = 256, batch_size: int = 64, query_idf=None):
        from benchmark.encoders import special_token_ids
        self.seismic = self.two_phase = self.hybrid = self._bm25 = None
        self.query_idf = _idf_tensor(query_idf)
        self.tokenizer = tokenizer
        self.device = torch.device(device)
        self.query_max_length, self.doc_max_length = int(query_max_length), int(doc_max_length)
        self.batch_size = max(1, int(batch_size))
        self.corpus = EvalCorpus(list(data.queries), list(data.docs), [], 0)
        self.relevant = [list(r) for r in data.relevant]
        self._token_lookup = list(tokenizer.convert_ids_to_tokens(list(range(tokenizer.vocab_size))))
        self._special = special_token_ids(tokenizer)
        self._allowed = None
        self.last_ranks = None

    def evaluate(self, model):
        raise NotImplementedError("BenchmarkEvaluator encodes; src.train.cli.eval_benchmark scores against the qrels")


def first_relevant_values(first_rank, k: int = RETRIEVAL_SIZE) -> np.ndarray:
    """Per-query values float64 [nq, 5] under the first-relevant rule, columns recall@1, recall@5, recall@10, reciprocal
    rank, ndcg@10 (ref:benchmark/metrics.py:52-99 per query): ``first_rank`` is the 1-based rank of the first relevant
    doc, 0 = none; a rank beyond the list depth ``k`` is a miss."""
    r = np.asarray(first_rank.cpu() if isinstance(first_rank, torch.Tensor) else first_rank, dtype=np.int64).reshape(-1)
    hit = (r >= 1) & (r <= int(k))
    safe = np.where(hit, r, 1)
    out = np.zeros((r.size, 5), np.float64)
    for j, c in enumerate((1, 5, 10)):
        out[:, j] = hit & (r <= c)
    out[:, 3] = np.where(hit, 1.0 / safe, 0.0)
    out[:, 4] = np.where(hit & (r <= 10), 1.0 / np.log2(safe + 1), 0.0)
    return out


def qrels_metrics(first_rank, hits, dcg, nrel, cutoffs: Sequence[int] = QRELS_CUTOFFS, k: int = RETRIEVAL_SIZE
                  ) -> Dict[str, float]:
    """Metrics of ranked lists against qrels, from the outputs of ``snx.retrieval.ranked_relevance`` (``first_rank``
    [nq], ``hits`` / ``dcg`` [nq, ncut] at ``cutoffs``) and the row sizes ``nrel`` [nq] (``first_relevant``'s fourth
    output).  The reference's five numbers under its first-relevant rule (ref:benchmark/hf_runner.py:191-215 into
    ref:benchmark/metrics.py): recall@1/5/10, mrr, ndcg@10, a rank beyond the list depth ``k`` being a miss.  And per
    cutoff c the two standard multi-relevant numbers it lacks: recall_frac@c = mean of hits / nrel (0 for an empty row),
    ndcg_multi@c = mean of dcg / idcg, idcg = the left-fold prefix sum of the same discount table over min(nrel, c)
    positions.  Plus num_queries."""
    from snx.retrieval import discount_table
    cpu = lambda x: np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)      # noqa: E731
    cuts = [int(c) for c in cutoffs]
    hits = cpu(hits).astype(np.float64).reshape(-1, len(cuts))
    dcg = cpu(dcg).astype(np.float64).reshape(-1, len(cuts))
    nrel = cpu(nrel).astype(np.int64).reshape(-1)
    vals = first_relevant_values(first_rank, k)
    nq = vals.shape[0]
    if hits.shape[0] != nq or nrel.size != nq:
        raise ValueError("qrels_metrics: first_rank, hits, dcg and nrel must describe the same queries")
    mean = lambda x: float(np.mean(x)) if nq else 0.0                             # noqa: E731
    out = {name: mean(vals[:, j]) for j, name in enumerate(REPORT_KEYS)}
    ideal = np.concatenate([[0.0], np.cumsum(discount_table(max(cuts)))]) if cuts else np.zeros(1)
    for j, c in enumerate(cuts):
        out[f"recall_frac@{c}"] = mean(np.where(nrel > 0, hits[:, j] / np.maximum(nrel, 1), 0.0))
        idcg = ideal[np.minimum(nrel, c)]
        out[f"ndcg_multi@{c}"] = mean(np.where(idcg > 0, dcg[:, j] / np.where(idcg > 0, idcg, 1.0), 0.0))
    out["num_queries"] = nq
    return out


def interval_from_means(per_query_values, means, confidence: float = 0.95) -> Dict[str, float]:
    """The arithmetic of ref:benchmark/metrics.py:208-215 over resample means already formed: point_estimate = the mean
    of the values, lower / upper = the (1 -+ confidence) / 2 percentiles of ``means`` (numpy's linear interpolation)."""
    v = np.asarray(per_query_values, np.float64).reshape(-1)
    m = np.asarray(means, np.float64).reshape(-1)
    return {"point_estimate": float(np.mean(v)), "lower": float(np.percentile(m, (1 - confidence) / 2 * 100)),
            "upper": float(np.percentile(m, (1 + confidence) / 2 * 100))}


def bootstrap_confidence_interval(per_query_values, n_bootstrap: int = 1000, confidence: float = 0.95, seed: int = 42,
                                  device=None):
    """ref:benchmark/metrics.py:180-215 for a metric that is the mean of per-query values (all five of the reference's
    are): the ``n_bootstrap`` resample means come from ``snx.retrieval.bootstrap_means`` on the GPU -- the reference's
    own resamples for ``seed`` 42 -- and the percentiles are taken on the host.  ``per_query_values`` [n] -> {point_estimate,
    lower, upper}; [n, M] (M <= 16, one launch) -> a list of M such dicts."""
    from snx.retrieval import bootstrap_means
    v = per_query_values.detach().cpu().numpy() if isinstance(per_query_values, torch.Tensor) else per_query_values
    v = np.asarray(v, np.float64)
    means = bootstrap_means(v, n_bootstrap=n_bootstrap, seed=seed, device=device).cpu().numpy()
    if v.ndim == 1:
        return interval_from_means(v, means[:, 0], confidence)
    return [interval_from_means(v[:, m], means[:, m], confidence) for m in range(v.shape[1])]
