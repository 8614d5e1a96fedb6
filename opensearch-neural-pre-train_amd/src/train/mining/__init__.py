"""Hard-negative mining with the model's own sparse index (self-mining, the ANCE / SPLADE++ loop).

The reference makes its multi-negative files offline from BGE-M3 embeddings and a dense search
(ref:scripts/mine_multi_negatives.py).  Here the trained SPLADE model retrieves over its own training corpus on the GPU
and its hard misses become the next round's negatives:

  corpus     docs = unique texts of ``positive`` / ``negative`` / ``negatives[]`` in first-occurrence order over the
             sorted input files; queries = unique ``query`` texts, each with the doc ids of ALL its positives
  encoding   the model's forward (no_grad, bf16 autocast), then ``ops.sparse_topk`` with the inference encoder's
             vocabulary filter: docs keep every surviving term, queries their top ``query_top_k``; batches are the
             texts sorted by (token length, id) cut into ``batch_size`` -- fixed by the corpus, never by the rank count
  search     ``SparseIndex.search_band``: ranks [rank_start, rank_end) of the docs that score > 0, are not a positive of
             the query, and (with ``max_score_ratio`` r) score < fp32(r) * min over the query's positives of s(q, p)
  assignment k negatives per record from its query's band (``first``: rank order; ``random``: drawn without
             replacement by a generator keyed on (seed, query id)); a short band repeats its last negative, an empty
             one falls back to the record's own negatives that are not positives of the query, else the record is
             written unchanged

With N ranks, doc batch b is encoded on rank b % N, the packed rows are all-gathered and every rank builds the same
index in doc-id order; query batches are split the same way and rank 0 writes.  The output is byte-identical for any N."""
from __future__ import annotations

import glob
import json
import logging
import os
import shutil
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

logger = logging.getLogger(__name__)

META_KEYS = ("pair_type", "difficulty", "source")          # ref:scripts/mine_multi_negatives.py:339-341
TEACHER_KEYS = ("teacher_pos_score", "teacher_neg_score", "teacher_neg_scores")
QUERY_TOP_K = 64                                         # NeuralSparseSearcher's query encoding, as the evaluator


@dataclass
class MiningCorpus:
    files: List[str]
    docs: List[str]
    queries: List[str]
    positives: List[List[int]]                           # per query: ascending doc ids of all its positives
    records: List[dict] = field(repr=False)
    rec_file: List[int] = field(repr=False)              # index into files
    rec_query: List[int] = field(repr=False)
    rec_pos: List[int] = field(repr=False)
    rec_negs: List[List[int]] = field(repr=False)        # doc ids of the record's original negatives, in order


def record_negatives(rec: dict) -> List[str]:
    """The original negative texts of a record: ``negative`` and then ``negatives[]``."""
    out = []
    if isinstance(rec.get("negative"), str):
        out.append(rec["negative"])
    if isinstance(rec.get("negatives"), list):
        out.extend(n for n in rec["negatives"] if isinstance(n, str))
    return out


def expand_files(patterns: Sequence[str]) -> List[str]:
    files = set()
    for p in patterns:
        files.update(glob.glob(p))
    return sorted(files)


def build_corpus(files: Sequence[str]) -> MiningCorpus:
    """Read the JSONL shards (sorted paths) through ``load_training_data`` and number docs and queries."""
    from src.train.data import load_training_data
    files = sorted(files)
    ds = load_training_data([glob.escape(f) for f in files])
    docs: List[str] = []
    doc_id: Dict[str, int] = {}
    queries: List[str] = []
    query_id: Dict[str, int] = {}
    pos_sets: List[set] = []

    def did(text: str) -> int:
        i = doc_id.get(text)
        if i is None:
            i = doc_id[text] = len(docs)
            docs.append(text)
        return i

    records, rec_file, rec_query, rec_pos, rec_negs = [], [], [], [], []
    for i in range(len(ds)):
        rec = ds[i]
        p = did(rec["positive"])
        negs = [did(t) for t in record_negatives(rec)]
        q = query_id.get(rec["query"])
        if q is None:
            q = query_id[rec["query"]] = len(queries)
            queries.append(rec["query"])
            pos_sets.append(set())
        pos_sets[q].add(p)
        records.append(rec)
        rec_file.append(ds.index[i][0])
        rec_query.append(q)
        rec_pos.append(p)
        rec_negs.append(negs)
    return MiningCorpus(list(files), docs, queries, [sorted(s) for s in pos_sets], records, rec_file, rec_query,
                        rec_pos, rec_negs)


def length_batches(lengths: Sequence[int], batch_size: int) -> List[List[int]]:
    """Ids sorted by (length, id), cut into batches of ``batch_size``: a function of the corpus alone."""
    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    bs = max(1, int(batch_size))
    return [order[s:s + bs] for s in range(0, len(order), bs)]


def token_lengths(tokenizer, texts: Sequence[str], max_length: int, chunk: int = 1024) -> List[int]:
    out: List[int] = []
    for s in range(0, len(texts), chunk):
        enc = tokenizer(list(texts[s:s + chunk]), padding=True, truncation=True, max_length=max_length,
                        return_tensors="pt")
        out.extend(enc["attention_mask"].sum(dim=1).tolist())
    return out


def f32(x) -> float:
    """An fp32 value as the shortest decimal that reads back to the same fp32 bits (what the JSON files hold)."""
    return float(str(np.float32(x)))


def sample_band(n_found: int, k: int, sample: str, seed: int, query_id: int) -> List[int]:
    """Positions (ascending) taken from a band of ``n_found`` docs: the first k, or k drawn without replacement by a
    generator keyed on (seed, query id)."""
    m = min(int(k), int(n_found))
    if sample == "first" or m == n_found:
        return list(range(m))
    if sample != "random":
        raise ValueError(f"sample must be 'first' or 'random', not {sample!r}")
    rng = np.random.Generator(np.random.PCG64([int(seed) & 0xFFFFFFFF, int(query_id)]))
    return sorted(int(i) for i in rng.choice(n_found, size=m, replace=False))


def assign_record(rec: dict, positives: Sequence[int], orig_negs: Sequence[int], band: Sequence[Tuple[int, float]],
                  k: int, sample: str, seed: int, query_id: int, docs: Sequence[str], pos_score: float,
                  score_of, teacher_scores: str = "none") -> Tuple[dict, str]:
    """One output record and its status: "full", "padded" (a short band, last negative repeated), "fallback" (empty
    band: the record's own negatives that are not positives of the query) or "unchanged" (nothing to take).
    ``band``: the query's (doc id, score) in rank order; ``score_of(doc)``: s(q, doc) for an original negative."""
    picks = [band[i] for i in sample_band(len(band), k, sample, seed, query_id)]
    status = "full" if len(picks) >= k else "padded"
    if not picks:
        pos = set(positives)
        seen, picks = set(), []
        for d in orig_negs:
            if d not in pos and d not in seen:
                seen.add(d)
                picks.append((d, score_of(d)))
        picks = picks[:k]
        status = "fallback"
        if not picks:
            return rec, "unchanged"
    while len(picks) < k:                                    # the collator's own padding rule
        picks.append(picks[-1])
    out = {"query": rec["query"], "positive": rec["positive"], "negatives": [docs[d] for d, _ in picks],
           "miner_pos_score": f32(pos_score), "miner_neg_scores": [f32(s) for _, s in picks]}
    if teacher_scores == "self":
        out["teacher_pos_score"] = out["miner_pos_score"]
        out["teacher_neg_scores"] = list(out["miner_neg_scores"])
    for key in META_KEYS:
        if key in rec:
            out[key] = rec[key]
    return out, status


def copy_val_files(patterns: Sequence[str], output_dir: str) -> List[str]:
    """ref:scripts/mine_multi_negatives.py:357-372: copy every matching file, keeping one that is already there."""
    out = []
    for src in expand_files(patterns):
        dst = os.path.join(output_dir, os.path.basename(src))
        if not os.path.exists(dst):
            shutil.copy2(src, dst)
            logger.info(f"Copied val file: {dst}")
        out.append(dst)
    return out


# ------------------------------------------------------------------------------------------------ device side
def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


def _all_gather(obj, dist, world):
    if dist is None:
        return [obj]
    out = [None] * world
    dist.all_gather_object(out, obj)                         # pickled through the backend (the host for gloo)
    return out


def _encode(model, tokenizer, texts, max_length, top_k, allowed, device):
    from snx import ops
    from snx.retrieval import pack_rows
    enc = tokenizer(list(texts), padding=True, truncation=True, max_length=max_length, return_tensors="pt")
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        rep, _ = model(enc["input_ids"].to(device), enc["attention_mask"].to(device))
    rep = rep.float().contiguous()
    V = rep.shape[1]
    vals, ids, cnt, _ = ops.sparse_topk(rep, allowed, None if top_k is None else min(int(top_k), V))
    return vals, ids, cnt, pack_rows(vals, ids, cnt, V)


def _doc_csr(pieces, n: int):
    """[(doc ids, counts, terms, weights)] in any order -> counts / terms / weights in doc-id order."""
    ids = np.concatenate([p[0] for p in pieces]) if pieces else np.zeros(0, np.int64)
    cnt = np.concatenate([p[1] for p in pieces]) if pieces else np.zeros(0, np.int64)
    terms = np.concatenate([p[2] for p in pieces]) if pieces else np.zeros(0, np.int32)
    w = np.concatenate([p[3] for p in pieces]) if pieces else np.zeros(0, np.float32)
    if ids.size != n or not np.array_equal(np.sort(ids), np.arange(n)):
        raise RuntimeError("mining: the gathered doc batches do not cover the corpus exactly once")
    starts = np.cumsum(cnt) - cnt
    order = np.argsort(ids, kind="stable")
    c = cnt[order]
    s = starts[order]
    base = np.repeat(np.cumsum(c) - c, c)
    idx = np.repeat(s, c) + (np.arange(int(c.sum())) - base)
    return c, terms[idx], w[idx]


def mine_negatives(model, tokenizer, input_files: Sequence[str], output_dir: str, *, k: int = 7, rank_start: int = 10,
                   rank_end: int = 50, query_max_length: int = 64, doc_max_length: int = 256, batch_size: int = 64,
                   query_top_k: int = QUERY_TOP_K, max_score_ratio: Optional[float] = None, sample: str = "first",
                   seed: int = 0, teacher_scores: str = "none", chunk_docs: int = 0,
                   val_patterns: Sequence[str] = (), device="cuda") -> Dict:
    """Mine ``k`` negatives per record of ``input_files`` and write one file per shard (same name) to ``output_dir``
    (rank 0).  Returns the summary: records, queries, docs, avg_nnz_d, avg_nnz_q, band_fill, padded, fallback,
    unchanged (every rank returns it)."""
    from benchmark.encoders import allowed_token_mask, special_token_ids
    from snx.retrieval import K_MAX, SparseIndex
    k, rank_start, rank_end = int(k), int(rank_start), int(rank_end)
    if k < 1 or not 0 <= rank_start < rank_end <= K_MAX:
        raise ValueError(f"mining: need k >= 1 and 0 <= rank_start < rank_end <= {K_MAX}")
    if sample not in ("first", "random") or teacher_scores not in ("none", "self"):
        raise ValueError("mining: sample is 'first' or 'random', teacher_scores 'none' or 'self'")
    if max_score_ratio is not None and not float(max_score_ratio) > 0:
        raise ValueError("mining: max_score_ratio must be > 0")
    dist, rank, world = _dist()
    device = torch.device(device)
    corpus = build_corpus(input_files)
    c = corpus
    nd, nq = len(c.docs), len(c.queries)
    V = int(getattr(model, "vocab_size", tokenizer.vocab_size))
    allowed = allowed_token_mask(tokenizer.convert_ids_to_tokens(list(range(tokenizer.vocab_size))),
                                 special_token_ids(tokenizer), V).to(device)
    was_training = model.training
    model.eval()
    try:
        # docs: batch b on rank b % N, gathered, one index in doc-id order on every rank
        mine = []
        for b, ids in enumerate(length_batches(token_lengths(tokenizer, c.docs, doc_max_length), batch_size)):
            if b % world != rank:
                continue
            _, _, _, (cnt, terms, w) = _encode(model, tokenizer, [c.docs[i] for i in ids], doc_max_length, None,
                                               allowed, device)
            mine.append((np.asarray(ids, np.int64), cnt.cpu().numpy(), terms.cpu().numpy(), w.cpu().numpy()))
        pieces = [p for part in _all_gather(mine, dist, world) for p in part]
        dc, dt, dw = _doc_csr(pieces, nd)
        index = SparseIndex(V, device)
        index.add_csr(torch.from_numpy(dc).to(device), torch.from_numpy(dt).to(device), torch.from_numpy(dw).to(device))
        index.build()
        # queries: the same split; search the local ones
        q_extra: List[set] = [set() for _ in range(nq)]          # original negatives: scored for the fallback
        for q, negs in zip(c.rec_query, c.rec_negs):
            q_extra[q].update(negs)
        local = []
        for b, ids in enumerate(length_batches(token_lengths(tokenizer, c.queries, query_max_length), batch_size)):
            if b % world != rank:
                continue
            vals, qids, cnt, _ = _encode(model, tokenizer, [c.queries[i] for i in ids], query_max_length, query_top_k,
                                         allowed, device)
            local.append((ids, vals, qids, cnt))
        out_local = []
        if local:
            qlist = [i for part in local for i in part[0]]
            q_vals, q_ids, q_cnt = (torch.cat([part[j] for part in local]) for j in (1, 2, 3))
            pair_rows = [(r, d) for r, q in enumerate(qlist) for d in c.positives[q]]
            n_pos = len(pair_rows)
            pair_rows += [(r, d) for r, q in enumerate(qlist) for d in sorted(q_extra[q])]
            pairs = torch.tensor(pair_rows, dtype=torch.int64, device=device).reshape(-1, 2)
            ps = index.pair_scores(q_vals, q_ids, q_cnt, pairs).cpu().numpy()
            ceiling = None
            if max_score_ratio is not None:
                mins = np.full(len(qlist), np.inf, np.float32)
                np.minimum.at(mins, np.asarray([r for r, _ in pair_rows[:n_pos]], np.int64), ps[:n_pos])
                ceil = (np.float32(max_score_ratio) * mins).astype(np.float32)
                ceil[mins == 0] = np.inf
                ceiling = torch.from_numpy(ceil).to(device)
            scores, docs, found = index.search_band(q_vals, q_ids, q_cnt, rank_start, rank_end,
                                                    exclude=[c.positives[q] for q in qlist], ceiling=ceiling,
                                                    chunk_docs=chunk_docs)
            out_local.append((np.asarray(qlist, np.int64), docs.cpu().numpy(), scores.cpu().numpy(),
                              found.cpu().numpy(), np.asarray(pair_rows, np.int64).reshape(-1, 2), ps,
                              int(q_cnt.long().sum())))
        gathered = [p for part in _all_gather(out_local, dist, world) for p in part]
    finally:
        model.train(was_training)

    bands: Dict[int, List[Tuple[int, float]]] = {}
    pscore: Dict[Tuple[int, int], float] = {}
    q_nnz = 0
    fill = 0
    for qlist, docs, scores, found, pr, ps, nnz in gathered:
        q_nnz += nnz
        for r, q in enumerate(qlist.tolist()):
            f = int(found[r])
            fill += f
            bands[q] = [(int(docs[r, j]), float(scores[r, j])) for j in range(f)]
        for (r, d), s in zip(pr.tolist(), ps.tolist()):
            pscore[(int(qlist[r]), d)] = s
    counts = {"full": 0, "padded": 0, "fallback": 0, "unchanged": 0}
    if rank == 0:
        os.makedirs(output_dir, exist_ok=True)
        if teacher_scores == "none":
            logger.info("mining: teacher scores are not written (the old ones belong to the old negatives): MarginMSE "
                        "is inactive on this data; --teacher-scores self writes the miner's own")
        handles = [open(os.path.join(output_dir, os.path.basename(f)), "w", encoding="utf-8") for f in c.files]
        try:
            for i, rec in enumerate(c.records):
                q = c.rec_query[i]
                out, st = assign_record(rec, c.positives[q], c.rec_negs[i], bands.get(q, []), k, sample, seed, q,
                                        c.docs, pscore[(q, c.rec_pos[i])], lambda d, q=q: pscore[(q, d)],
                                        teacher_scores)
                counts[st] += 1
                handles[c.rec_file[i]].write(json.dumps(out, ensure_ascii=False) + "\n")
        finally:
            for h in handles:
                h.close()
        copy_val_files(val_patterns, output_dir)
    else:
        for i in range(len(c.records)):                      # the same counts on every rank, nothing written
            q = c.rec_query[i]
            band = bands.get(q, [])
            counts["full" if len(band) >= k else "padded" if band else
                   "fallback" if any(d not in c.positives[q] for d in c.rec_negs[i]) else "unchanged"] += 1
    summary = {"records": len(c.records), "queries": nq, "docs": nd,
               "avg_nnz_d": float(index.nnz / nd) if nd else 0.0, "avg_nnz_q": float(q_nnz / nq) if nq else 0.0,
               "band_fill": float(fill / (nq * (rank_end - rank_start))) if nq else 0.0,
               "padded": counts["padded"], "fallback": counts["fallback"], "unchanged": counts["unchanged"]}
    logger.info("mining: " + " | ".join(f"{key}={v:.4g}" if isinstance(v, float) else f"{key}={v}"
                                       for key, v in summary.items()))
    return summary
