"""Teacher scores and dense hard-negative mining from cached teacher embeddings (BGE-M3 in the reference), on the GPU.

Embeddings arrive as the reference's cache, an ``.npy`` array [n, D] plus a JSON map ``md5(text)[:16] -> row``
(ref:scripts/mine_multi_negatives.py:45-64); ``write_teacher_cache`` writes that cache from any encoder (the CLI hands it
``src.model.teachers.BGEM3Teacher.encode``).  Everything from the arrays onward is on ``snx.retrieval.DenseIndex``
(csrc/dense.hip):

  write_teacher_scores   ref:scripts/precompute_teacher_scores.py:162-224 through ``pair_scores``: every record gets
                         ``teacher_pos_score`` / ``teacher_neg_score`` as round(float(s), 6), one output file per shard; a
                         missing negative scores 0.0; a record whose query or positive is not in the cache is written
                         unchanged.  Extension: a record with ``negatives[]`` also gets ``teacher_neg_scores``.
  mine_dense_negatives   ref:scripts/mine_multi_negatives.py:225-353 through ``search_band`` over ``build_corpus``'s docs:
                         ranks [rank_start, rank_end) of the docs that are not a positive of the query, then the picking
                         and padding rules of the sparse miner (``sample_band``, ``assign_record``).  Output keys are the
                         reference's: ``negatives``, ``teacher_pos_score``, ``teacher_neg_scores`` (rounded to 6) and the
                         meta keys.

One deliberate deviation: a query's positives (ALL of them, over every record of the query) are excluded BEFORE ranking,
as in the sparse miner, so the band always holds rank_end - rank_start non-positives when the corpus has them; the
reference ranks first and skips the record's own positive INSIDE ranks [rank_start, rank_end), which shortens the band
and lets a positive of another record of the same query through.  Docs without an embedding stay out of the index; a
record whose query has no embedding is written unchanged.

Both functions run in a single process (no rank split: the search is one GPU's work) and take the index object as a
parameter -- an empty ``DenseIndex(dim, device)``, which they fill -- so that a numpy stand-in with the same methods
drives them on the CPU (tests/dense_reference.py)."""
from __future__ import annotations

import hashlib
import json
import logging
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import META_KEYS, assign_record, build_corpus

logger = logging.getLogger(__name__)


def text_hash(text: str) -> str:
    """The cache key of a text: md5(utf-8)[:16]."""
    return hashlib.md5(text.encode("utf-8")).hexdigest()[:16]


def load_teacher_cache(embeddings_npy: str, text_index_json: str) -> Tuple[np.ndarray, Dict[str, int]]:
    """The reference's embedding cache -> (embeddings fp32 [n, D], text hash -> row)."""
    emb = np.load(embeddings_npy, mmap_mode="r")
    if emb.ndim != 2:
        raise ValueError(f"{embeddings_npy}: expected a [n, D] array, got shape {emb.shape}")
    with open(text_index_json, "r") as f:
        text_to_idx = {str(h): int(i) for h, i in json.load(f).items()}
    if text_to_idx and not 0 <= min(text_to_idx.values()) <= max(text_to_idx.values()) < emb.shape[0]:
        raise ValueError(f"{text_index_json}: rows must lie in [0, {emb.shape[0]})")
    return emb, text_to_idx


def collect_unique_texts(input_files: Sequence[str]) -> Tuple[List[str], Dict[str, int]]:
    """The unique texts of the shards in first-occurrence order and the map text hash -> row
    (ref:scripts/precompute_teacher_scores.py:49-86: ``query``, ``positive``, ``negative`` of every record; here also the
    entries of a ``negatives`` list, which ``write_teacher_scores`` reads).  Files in sorted order; only strings count."""
    seen: Dict[str, int] = {}
    texts: List[str] = []
    for path in sorted(input_files):
        for item in _read(path):
            if not isinstance(item, dict):
                continue
            negs = item["negatives"] if isinstance(item.get("negatives"), list) else []
            for text in [item.get("query"), item.get("positive"), item.get("negative")] + list(negs):
                if not isinstance(text, str):
                    continue
                h = text_hash(text)
                if h not in seen:
                    seen[h] = len(texts)
                    texts.append(text)
    return texts, seen


def shard_range(n: int, num_shards: int, shard_index: int) -> Tuple[int, int]:
    """Rows [begin, end) of shard ``shard_index`` of ``num_shards`` contiguous, near-equal parts of ``n`` rows."""
    if num_shards < 1 or not 0 <= shard_index < num_shards:
        raise ValueError("need num_shards >= 1 and 0 <= shard_index < num_shards")
    return n * shard_index // num_shards, n * (shard_index + 1) // num_shards


def write_teacher_cache(input_files: Sequence[str], output_dir: str, encode, dim: int, num_shards: int = 1,
                        shard_index: int = 0) -> Tuple[int, int]:
    """Encode the unique texts of the shards into the cache ``load_teacher_cache`` reads: ``text_index.json`` and
    ``embeddings.npy`` fp32 [n, dim] -- or, for ``num_shards > 1``, this shard's rows as ``embeddings.part{i}.npy``
    (``merge_teacher_cache`` joins them).  ``encode(texts) -> array-like [len(texts), dim]``, rows in input order.
    Returns (unique texts, rows written)."""
    texts, seen = collect_unique_texts(input_files)
    b, e = shard_range(len(texts), int(num_shards), int(shard_index))
    emb = np.zeros((0, dim), np.float32)
    if e > b:
        emb = np.ascontiguousarray(_to_host(encode(texts[b:e])), dtype=np.float32)
    if emb.shape != (e - b, dim):
        raise ValueError(f"teacher cache: the encoder returned shape {emb.shape}, expected {(e - b, dim)}")
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "text_index.json"), "w") as f:
        json.dump(seen, f)
    name = "embeddings.npy" if int(num_shards) == 1 else f"embeddings.part{int(shard_index)}.npy"
    np.save(os.path.join(output_dir, name), emb)
    return len(texts), e - b


def merge_teacher_cache(output_dir: str) -> int:
    """Join ``embeddings.part{0..k-1}.npy`` of a sharded run into ``embeddings.npy``; the rows must match
    ``text_index.json``.  Returns the rows."""
    parts = []
    while os.path.exists(os.path.join(output_dir, f"embeddings.part{len(parts)}.npy")):
        parts.append(np.load(os.path.join(output_dir, f"embeddings.part{len(parts)}.npy")))
    if not parts:
        raise FileNotFoundError(f"{output_dir}: no embeddings.part0.npy")
    emb = np.concatenate(parts, axis=0).astype(np.float32, copy=False)
    with open(os.path.join(output_dir, "text_index.json")) as f:
        n = len(json.load(f))
    if emb.shape[0] != n:
        raise ValueError(f"{output_dir}: the parts hold {emb.shape[0]} rows, text_index.json names {n} (a shard is missing)")
    np.save(os.path.join(output_dir, "embeddings.npy"), emb)
    return n


def _to_index(index, a: np.ndarray):
    """A numpy array as the index takes it: a tensor on its device (DenseIndex), or the array itself (a stand-in)."""
    dev = getattr(index, "device", None)
    if dev is None:
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _to_host(x) -> np.ndarray:
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _rows(embeddings, rows: Sequence[int]) -> np.ndarray:
    dim = int(embeddings.shape[1])
    if not len(rows):
        return np.zeros((0, dim), np.float32)
    return np.ascontiguousarray(np.asarray(embeddings[np.asarray(rows, np.int64)], dtype=np.float32))


def _r6(x) -> float:
    return round(float(x), 6)


def _read(path: str) -> List[dict]:
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            try:
                out.append(json.loads(line.strip()))
            except json.JSONDecodeError:
                continue
    return out


def write_teacher_scores(input_files: Sequence[str], output_dir: str, embeddings, text_to_idx: Dict[str, int],
                         index) -> int:
    """Teacher scores for every record of ``input_files`` (one output file per shard, same name).  ``index``: an empty
    dense index; it receives the cache rows that any record names as a positive or negative.  Returns the records scored."""
    files = sorted(input_files)
    shards = [_read(f) for f in files]

    def row(text):
        return text_to_idx.get(text_hash(text)) if isinstance(text, str) else None

    def neg_texts(item) -> List:
        return [n for n in item["negatives"]] if isinstance(item.get("negatives"), list) else []

    doc_rows = set()
    for items in shards:
        for item in items:
            for text in [item.get("positive", ""), item.get("negative")] + neg_texts(item):
                r = row(text)
                if r is not None:
                    doc_rows.add(r)
    doc_rows = sorted(doc_rows)
    local = {r: i for i, r in enumerate(doc_rows)}
    index.add(_to_index(index, _rows(embeddings, doc_rows)))
    index.build()
    os.makedirs(output_dir, exist_ok=True)
    total = 0
    for path, items in zip(files, shards):
        q_local: Dict[int, int] = {}
        pairs: List[Tuple[int, int]] = []
        plan = []                                                # per record: None | (pos, neg | None, [negs | None])
        for item in items:
            q, p = row(item.get("query", "")), row(item.get("positive", ""))
            if q is None or p is None:
                plan.append(None)
                continue
            qi = q_local.setdefault(q, len(q_local))

            def pair(r):
                if r is None:
                    return None
                pairs.append((qi, local[r]))
                return len(pairs) - 1

            neg = pair(row(item["negative"])) if item.get("negative") else None
            plan.append((pair(p), neg, [pair(row(n)) for n in neg_texts(item)]))
        scores = np.zeros(0, np.float32)
        if pairs:
            qemb = _rows(embeddings, list(q_local))              # insertion order = local query row
            scores = _to_host(index.pair_scores(_to_index(index, qemb),
                                                _to_index(index, np.asarray(pairs, np.int64).reshape(-1, 2))))
        with open(os.path.join(output_dir, os.path.basename(path)), "w", encoding="utf-8") as fout:
            for item, pl in zip(items, plan):
                if pl is not None:
                    pos, neg, negs = pl
                    item["teacher_pos_score"] = _r6(scores[pos])
                    item["teacher_neg_score"] = _r6(scores[neg]) if neg is not None else 0.0
                    if isinstance(item.get("negatives"), list):
                        item["teacher_neg_scores"] = [_r6(scores[i]) if i is not None else 0.0 for i in negs]
                    total += 1
                fout.write(json.dumps(item, ensure_ascii=False) + "\n")
    return total


def mine_dense_negatives(input_files: Sequence[str], output_dir: str, embeddings, text_to_idx: Dict[str, int], index, *,
                         k: int = 7, rank_start: int = 10, rank_end: int = 50, sample: str = "first", seed: int = 0,
                         chunk_docs: int = 0, two_phase: Optional[Tuple[float, bool]] = None) -> Dict:
    """Mine ``k`` negatives per record from ranks [rank_start, rank_end) of the teacher's dense search and write one file
    per shard to ``output_dir``.  ``index``: an empty dense index; it receives the embedded docs of the corpus.  Returns
    the summary: records, queries, docs, indexed_docs, band_fill, padded, fallback, unchanged.  ``two_phase``:
    (expansion, exact) sends the band search through ``DenseIndex.search_band_two_phase`` -- with ``exact`` the files are
    those of the plain search -- and the summary gains ``certified_fraction``, the share of the queries whose band the
    bf16 pass alone proved exact."""
    from snx.retrieval import K_MAX
    k, rank_start, rank_end = int(k), int(rank_start), int(rank_end)
    if k < 1 or not 0 <= rank_start < rank_end <= K_MAX:
        raise ValueError(f"dense mining: need k >= 1 and 0 <= rank_start < rank_end <= {K_MAX}")
    if sample not in ("first", "random"):
        raise ValueError("dense mining: sample is 'first' or 'random'")
    c = build_corpus(input_files)
    doc_row = [text_to_idx.get(text_hash(t)) for t in c.docs]
    kept = [d for d, r in enumerate(doc_row) if r is not None]   # index doc id -> corpus doc id
    local = {d: i for i, d in enumerate(kept)}
    index.add(_to_index(index, _rows(embeddings, [doc_row[d] for d in kept])))
    index.build()
    q_row = [text_to_idx.get(text_hash(t)) for t in c.queries]
    qs = [q for q, r in enumerate(q_row) if r is not None]       # search row -> corpus query id
    q_search = {q: i for i, q in enumerate(qs)}
    bands: Dict[int, List[Tuple[int, float]]] = {}
    pscore: Dict[Tuple[int, int], float] = {}
    fill, certified = 0, 0.0
    if qs:
        qemb = _to_index(index, _rows(embeddings, [q_row[q] for q in qs]))
        wanted: List[set] = [set() for _ in c.queries]           # docs whose s(q, d) the records need
        for i, q in enumerate(c.rec_query):
            wanted[q].add(c.rec_pos[i])
            wanted[q].update(c.rec_negs[i])
        pairs = [(q_search[q], local[d], q, d) for q in qs for d in sorted(wanted[q]) if d in local]
        if pairs:
            ps = _to_host(index.pair_scores(qemb, _to_index(index, np.asarray([p[:2] for p in pairs], np.int64))))
            for (_, _, q, d), s in zip(pairs, ps.tolist()):
                pscore[(q, d)] = s
        exclude = [[local[d] for d in c.positives[q] if d in local] for q in qs]
        if two_phase is None:
            band = index.search_band(qemb, rank_start, rank_end, exclude=exclude, ceiling=None, chunk_docs=chunk_docs)
        else:
            *band, cert = index.search_band_two_phase(qemb, rank_start, rank_end, exclude=exclude, ceiling=None,
                                                      expansion=two_phase[0], exact=two_phase[1], chunk_docs=chunk_docs)
            certified = float(_to_host(cert).mean())
        scores, docs, found = (_to_host(x) for x in band)
        for i, q in enumerate(qs):
            f = int(found[i])
            fill += f
            bands[q] = [(kept[int(docs[i, j])], float(scores[i, j])) for j in range(f)]
    counts = {"full": 0, "padded": 0, "fallback": 0, "unchanged": 0}
    os.makedirs(output_dir, exist_ok=True)
    handles = [open(os.path.join(output_dir, os.path.basename(f)), "w", encoding="utf-8") for f in c.files]
    try:
        for i, rec in enumerate(c.records):
            q = c.rec_query[i]
            out, st = rec, "unchanged"
            if q in q_search:
                pos = pscore.get((q, c.rec_pos[i]), rec.get("teacher_pos_score", 0.0))
                got, st = assign_record(rec, c.positives[q], c.rec_negs[i], bands[q], k, sample, seed, q, c.docs, pos,
                                        lambda d, q=q: pscore.get((q, d), 0.0))
                if st != "unchanged":                            # the miner's fp32 decimals read back to the same fp32
                    out = {"query": rec["query"], "positive": rec["positive"], "negatives": got["negatives"],
                           "teacher_pos_score": _r6(np.float32(got["miner_pos_score"])),
                           "teacher_neg_scores": [_r6(np.float32(s)) for s in got["miner_neg_scores"]]}
                    for key in META_KEYS:
                        if key in rec:
                            out[key] = rec[key]
            counts[st] += 1
            handles[c.rec_file[i]].write(json.dumps(out, ensure_ascii=False) + "\n")
    finally:
        for h in handles:
            h.close()
    nq = len(qs)
    summary = {"records": len(c.records), "queries": len(c.queries), "docs": len(c.docs), "indexed_docs": len(kept),
               "band_fill": float(fill / (nq * (rank_end - rank_start))) if nq else 0.0, "padded": counts["padded"],
               "fallback": counts["fallback"], "unchanged": counts["unchanged"]}
    if two_phase is not None:
        summary["certified_fraction"] = certified
    logger.info("dense mining: " + " | ".join(f"{key}={v:.4g}" if isinstance(v, float) else f"{key}={v}"
                                             for key, v in summary.items()))
    return summary
