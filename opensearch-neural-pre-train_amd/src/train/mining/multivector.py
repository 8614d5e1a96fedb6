"""Multi-vector (MaxSim) and lexical teacher scores for the records of a training set, straight from the encoder.

``write_teacher_scores`` (dense.py) reads single vectors from a cache on disk.  A multi-vector cannot be cached that way (a
256-token text is 512 KB in bf16), so here the scorer sits directly behind the forward: per chunk of records the chunk's
unique texts are encoded once (``encode_mv``: ``BGEM3Teacher.encode_multivector``), the (query, positive) and (query,
negative) pairs are scored over that store (``scorer``: ``snx.teacher.maxsim_pairs``) and the store is dropped.  The dense
score of ``mode="dense+colbert"`` is the CLS cosine of the same forward.  A mode with "sparse" takes all its scores from one
forward too: ``encode_mv`` is then ``BGEM3Teacher.encode_m3`` and ``lex_scorer`` (``snx.teacher.lexical_pairs``) scores the
lexical weights.  The fields written are those of
``write_teacher_scores`` -- ``teacher_pos_score``, ``teacher_neg_score`` and, for a record with ``negatives[]``,
``teacher_neg_scores``, each round(float(s), 6) -- so the trainer reads the output unchanged.  A record without a string
query and positive is written unchanged; a missing negative scores 0.0."""
from __future__ import annotations

import json
import os
from typing import Callable, Dict, List, Optional, Sequence

from .dense import _r6, _read

MV_MODES = ("colbert", "dense+colbert", "sparse", "dense+sparse", "sparse+colbert", "dense+sparse+colbert")


def _score_chunk(items: List[dict], encode_mv: Callable, scorer: Callable, mode: str, weights,
                 lex_scorer: Optional[Callable] = None) -> int:
    """Adds the score fields to the scoreable records of ``items`` in place; returns how many there were."""
    import torch
    from src.model.teachers.bge_m3 import combine_modes, combine_scores, mode_weights
    row: Dict[str, int] = {}
    pair_q: List[int] = []
    pair_d: List[int] = []

    def pair(q: int, text):
        if not isinstance(text, str):
            return None
        pair_q.append(q)
        pair_d.append(row.setdefault(text, len(row)))
        return len(pair_q) - 1

    plan = []                                                    # per record: None | (pos, neg | None, [negs | None])
    for item in items:
        if not isinstance(item, dict) or not isinstance(item.get("query"), str) or not isinstance(item.get("positive"), str):
            plan.append(None)
            continue
        q = row.setdefault(item["query"], len(row))
        negs = item["negatives"] if isinstance(item.get("negatives"), list) else []
        plan.append((pair(q, item["positive"]), pair(q, item.get("negative")), [pair(q, n) for n in negs]))
    if not pair_q:
        return 0
    pq, pd = torch.tensor(pair_q), torch.tensor(pair_d)

    def dense_of(emb):
        return (emb[pq.to(emb.device)] * emb[pd.to(emb.device)]).sum(dim=-1)

    if "sparse" in mode:
        emb, mv_ptr, mv, lex_ptr, lex_ids, lex_w = encode_mv(list(row))
        by_mode = {"sparse": lex_scorer(lex_ptr, lex_ids, lex_w, pq, pd).to(torch.float32)}
        if "dense" in mode:
            by_mode["dense"] = dense_of(emb).to(by_mode["sparse"].device)
        if "colbert" in mode:
            by_mode["colbert"] = scorer(mv, mv_ptr, pq, pd).to(torch.float32).to(by_mode["sparse"].device)
        scores = combine_modes(by_mode, mode_weights(weights))
    else:
        emb, mv_ptr, mv = encode_mv(list(row))
        scores = scorer(mv, mv_ptr, pq, pd).to(torch.float32)
        if mode == "dense+colbert":
            scores = combine_scores(dense_of(emb).to(scores.device), scores, mode_weights(weights, pair=True))
    scores = scores.cpu().tolist()
    done = 0
    for item, pl in zip(items, plan):
        if pl is None:
            continue
        pos, neg, negs = pl
        item["teacher_pos_score"] = _r6(scores[pos])
        item["teacher_neg_score"] = _r6(scores[neg]) if neg is not None else 0.0
        if isinstance(item.get("negatives"), list):
            item["teacher_neg_scores"] = [_r6(scores[i]) if i is not None else 0.0 for i in negs]
        done += 1
    return done


def write_multivector_scores(input_files: Sequence[str], output_dir: str, encode_mv: Callable, scorer: Callable,
                             mode: str = "colbert", weights=(1.0, 1.0), chunk_records: int = 256,
                             lex_scorer: Optional[Callable] = None) -> int:
    """Teacher scores for every record of ``input_files`` (one output file per shard, same name), ``chunk_records``
    records per forward-and-score round.  ``encode_mv(texts) -> (emb [n, H], mv_ptr [n + 1], mv [rows, H])``;
    ``scorer(mv, mv_ptr, pair_q, pair_d) -> [npairs]``.  ``mode``: "colbert", or "dense+colbert" with ``weights`` =
    (w_dense, w_colbert).  A mode with "sparse" ("sparse", "dense+sparse", "sparse+colbert", "dense+sparse+colbert"):
    ``encode_mv(texts)`` returns ``encode_m3``'s six values, ``lex_scorer(lex_ptr, ids, w, pair_q, pair_d) -> [npairs]``
    is required and ``weights`` may be (w_dense, w_sparse, w_colbert) or a dict by mode.  Returns the records scored."""
    if mode not in MV_MODES:
        raise ValueError(f"multi-vector scores: mode is one of {MV_MODES}")
    if "sparse" in mode and lex_scorer is None:
        raise ValueError("multi-vector scores: a sparse mode needs lex_scorer")
    if int(chunk_records) < 1:
        raise ValueError("multi-vector scores: chunk_records must be positive")
    os.makedirs(output_dir, exist_ok=True)
    total = 0
    for path in sorted(input_files):
        items = _read(path)
        with open(os.path.join(output_dir, os.path.basename(path)), "w", encoding="utf-8") as fout:
            for at in range(0, len(items), int(chunk_records)):
                chunk = items[at:at + int(chunk_records)]
                total += _score_chunk(chunk, encode_mv, scorer, mode, weights, lex_scorer)
                for item in chunk:
                    fout.write(json.dumps(item, ensure_ascii=False) + "\n")
    return total


def default_ncand(rank_end: int) -> int:
    """Candidates per query of the centroid pass when the caller names none: four times the band's end, at least 128."""
    return min(max(4 * int(rank_end), 128), 1024)


def mine_multivector_negatives(input_files: Sequence[str], output_dir: str, encode_mv: Callable, index, *, k: int = 7,
                               rank_start: int = 10, rank_end: int = 50, chunk_texts: int = 256,
                               chunk_docs: int = 0, index_type: str = "exact", ncentroids: int = 1024,
                               ncand: int = 0, nbits: int = 0, nprobe: int = 0, k_sim: int = 4, reps: int = 16,
                               d_proj: int = 16, fde_seed: int = 0) -> Dict:
    """Hard negatives under the late-interaction teacher: per record ``k`` negatives from ranks [rank_start, rank_end) of
    the MaxSim search of its query over the corpus, the unique positives of the shards, with the query's own positives
    (all of them, over every record of the query) excluded before ranking.  ``encode_mv(texts) -> (emb, mv_ptr, mv)``
    (``BGEM3Teacher.encode_multivector``) encodes the corpus ``chunk_texts`` texts at a time into ``index``, an empty
    ``snx.retrieval.MultiVectorIndex`` or a stand-in with its ``add`` / ``build`` / ``search_band`` / ``pair_scores``, and
    then the queries.  The records written are ``mine_dense_negatives``': ``negatives[]``, ``teacher_pos_score``,
    ``teacher_neg_scores`` (the MaxSim values, rounded to 6) and the meta keys; a short band repeats its last negative.  A
    record without a string query and positive, with a query of one token or with an empty band is written unchanged.
    ``index_type="centroid"``: the band comes from ``index.search_band_two_phase`` over ``ncand`` candidates of the
    centroid-interaction pass (0: ``default_ncand(rank_end)``), after ``index.train_centroids(ncentroids)``; the negatives
    are then approximate, their scores and the positives' still exact.  ``nbits`` 1, 2 or 4 (centroid only; 0: uncompressed):
    the store is then residual-compressed (``index.compress(nbits)``), the bf16 rows are released and every score, the
    positives' included, is the packed form's.  ``nprobe`` 1 .. 64 (centroid only; 0: every document is walked): the
    candidates come from the documents in the ``nprobe`` best centroid lists of each query row
    (``search_band_two_phase(..., nprobe=nprobe)``).  ``index_type="fde"``: no centroids; the candidates come from a dense
    search over MUVERA fixed-dimensional encodings (``index.set_fde(FdeEncoder(dim, k_sim, reps, d_proj, device, fde_seed))``,
    then ``search_band_two_phase(..., fde=True)``), the scores exact as for "centroid".  ``index_type="token"``: token
    retrieval over the compressed store (``index.search_band_tokens(..., nprobe)`` after ``train_centroids`` and
    ``compress(nbits)``); it needs ``nbits`` 1, 2 or 4 and ``nprobe`` 1 .. 64 and takes no ``ncand``; the negatives' scores
    are then token retrieval's x(q, d) (include/snx.h), the positives' the packed form's.  Returns the counts: records, queries, docs, store_rows, store_bytes, band_fill, padded, unchanged."""
    import torch
    from . import META_KEYS
    k, rank_start, rank_end, chunk_texts = int(k), int(rank_start), int(rank_end), int(chunk_texts)
    if k < 1 or not 0 <= rank_start < rank_end <= 1024 or chunk_texts < 1:
        raise ValueError("multi-vector mining: need k >= 1, 0 <= rank_start < rank_end <= 1024 and chunk_texts >= 1")
    if index_type not in ("exact", "centroid", "fde", "token"):
        raise ValueError('multi-vector mining: index_type is "exact", "centroid", "fde" or "token"')
    token = index_type == "token"
    if token and int(ncand):
        raise ValueError('multi-vector mining: index_type="token" has no candidate list; ncand must be 0')
    ncand = int(ncand) or default_ncand(rank_end)
    if index_type != "exact" and not token and not rank_end <= ncand <= 1024:
        raise ValueError("multi-vector mining: need rank_end <= ncand <= 1024")
    if int(nbits) not in (0, 1, 2, 4) or (int(nbits) and index_type not in ("centroid", "token")) or (token and not int(nbits)):
        raise ValueError('multi-vector mining: nbits is 0, or 1, 2 or 4 with index_type="centroid"; "token" needs 1, 2 or 4')
    if isinstance(nprobe, bool) or not isinstance(nprobe, int) or not 0 <= nprobe <= 64 or \
            (nprobe and index_type not in ("centroid", "token")) or (token and not nprobe):
        raise ValueError('multi-vector mining: nprobe is 0, or 1 .. 64 with index_type="centroid"; "token" needs 1 .. 64')
    probed = {"nprobe": nprobe} if nprobe else ({"fde": True} if index_type == "fde" else {})
    files = sorted(input_files)
    shards = [_read(f) for f in files]
    docs: Dict[str, int] = {}
    queries: Dict[str, int] = {}
    positives: List[set] = []
    for items in shards:
        for item in items:
            if isinstance(item, dict) and isinstance(item.get("query"), str) and isinstance(item.get("positive"), str):
                q = queries.setdefault(item["query"], len(queries))
                if q == len(positives):
                    positives.append(set())
                positives[q].add(docs.setdefault(item["positive"], len(docs)))
    doc_texts, query_texts = list(docs), list(queries)
    rows = nbytes = 0
    for s in range(0, len(doc_texts), chunk_texts):
        _, ptr, mv = encode_mv(doc_texts[s:s + chunk_texts])
        index.add(mv, ptr)
        rows += int(mv.shape[0])
        nbytes += int(mv.shape[0]) * int(mv.shape[1]) * mv.element_size()
    index.build()
    if index_type in ("centroid", "token") and doc_texts:
        index.train_centroids(int(ncentroids))
        if int(nbits):
            index.compress(int(nbits))
    if index_type == "fde" and doc_texts:
        from snx.retrieval import FdeEncoder
        index.set_fde(FdeEncoder(index.dim, int(k_sim), int(reps), int(d_proj), index.device, seed=int(fde_seed)))
    bands: Dict[int, List] = {}                                  # query -> [(doc, score)] in rank order
    pscore: Dict = {}                                            # (query, positive) -> score
    fill = 0
    for s in range(0, len(query_texts), chunk_texts):
        _, ptr, mv = encode_mv(query_texts[s:s + chunk_texts])
        ptr = [int(v) for v in torch.as_tensor(ptr).tolist()]
        kept = [i for i in range(len(ptr) - 1) if ptr[i + 1] > ptr[i]]   # a query of one token has no row: unchanged
        if not kept or not doc_texts:
            continue
        qptr = [ptr[i] for i in kept] + [ptr[-1]]
        exclude = [sorted(positives[s + i]) for i in kept]
        if token:
            sc, dd, found = index.search_band_tokens(mv, qptr, rank_start, rank_end, nprobe, exclude=exclude)
        elif index_type != "exact":
            sc, dd, found = index.search_band_two_phase(mv, qptr, rank_start, rank_end, ncand, exclude=exclude,
                                                        chunk_docs=chunk_docs, **probed)
        else:
            sc, dd, found = index.search_band(mv, qptr, rank_start, rank_end, exclude=exclude, chunk_docs=chunk_docs)
        sc, dd, found = sc.cpu().tolist(), dd.cpu().tolist(), found.cpu().tolist()
        pairs = [(j, d) for j, i in enumerate(kept) for d in sorted(positives[s + i])]
        ps = index.pair_scores(mv, qptr, torch.tensor(pairs, dtype=torch.long, device=mv.device)).cpu().tolist()
        for (j, d), v in zip(pairs, ps):
            pscore[(s + kept[j], d)] = v
        for j, i in enumerate(kept):
            bands[s + i] = [(dd[j][r], sc[j][r]) for r in range(found[j])]
            fill += found[j]
    counts = {"full": 0, "padded": 0, "unchanged": 0}
    os.makedirs(output_dir, exist_ok=True)
    for path, items in zip(files, shards):
        with open(os.path.join(output_dir, os.path.basename(path)), "w", encoding="utf-8") as fout:
            for item in items:
                q = queries.get(item.get("query")) if isinstance(item, dict) and isinstance(item.get("query"), str) and \
                    isinstance(item.get("positive"), str) else None
                picks = bands.get(q, [])[:k]
                out, st = item, "unchanged"
                if picks:
                    st = "full" if len(picks) >= k else "padded"
                    picks = picks + [picks[-1]] * (k - len(picks))
                    out = {"query": item["query"], "positive": item["positive"], "negatives": [doc_texts[d] for d, _ in picks],
                           "teacher_pos_score": _r6(pscore[(q, docs[item["positive"]])]),
                           "teacher_neg_scores": [_r6(v) for _, v in picks]}
                    for key in META_KEYS:
                        if key in item:
                            out[key] = item[key]
                counts[st] += 1
                fout.write(json.dumps(out, ensure_ascii=False) + "\n")
    nb = len(bands)
    return {"records": sum(len(x) for x in shards), "queries": len(queries), "docs": len(docs), "store_rows": rows,
            "store_bytes": nbytes, "band_fill": float(fill / (nb * (rank_end - rank_start))) if nb else 0.0,
            "padded": counts["padded"], "unchanged": counts["unchanged"]}
