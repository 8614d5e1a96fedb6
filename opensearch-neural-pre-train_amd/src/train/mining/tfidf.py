"""Lexical hard negatives by character n-gram TF-IDF: the first mining step of the reference
(ref:scripts/mine_hard_negatives.py), which fills the ``negative`` field of raw triplets before any model or teacher
exists.  The corpus is the unique non-empty positives of the shards in file order, up to ``max_corpus``
(ref:mine_hard_negatives.py:85-119); every record without a negative is searched against it by cosine over tf-idf rows and
receives the best hit whose text differs from its own positive, with ``difficulty = "hard"``
(ref:mine_hard_negatives.py:262-388).  The index is a parameter: ``snx.retrieval.TfidfIndex`` on a GPU, or any object with
``fit_add(texts)``, ``build()`` and ``search_texts(texts, k) -> (scores, docs, ...)`` (unused slots: doc -1).

One deliberate difference: the index never returns a document that shares no n-gram with the query, so a record whose only
candidates would score 0 counts as ``failed``; the reference ranks all documents and hands such a record a zero-cosine
document in arbitrary order."""
from __future__ import annotations

import json
import logging
import os
import re
import tempfile
from typing import Dict, List, Optional, Sequence

import numpy as np

logger = logging.getLogger(__name__)

STAT_KEYS = ("total", "already_had_negative", "added", "failed")
_SHARD = re.compile(r"^train_shard_.*\.jsonl$")


def parse_shard_range(shard_range: str, num_shards: int) -> List[int]:
    """"all", "A-B" (inclusive) or "N" -> shard indices."""
    if shard_range == "all":
        return list(range(num_shards))
    if "-" in shard_range:
        a, b = shard_range.split("-", 1)
        return list(range(int(a), int(b) + 1))
    return [int(shard_range)]


def collect_shard_files(data_dir: str, shard_range: str = "all") -> List[str]:
    """The ``train_shard_*.jsonl`` files of ``data_dir`` in sorted order, restricted to ``shard_range``."""
    shards = sorted(os.path.join(data_dir, f) for f in os.listdir(data_dir) if _SHARD.match(f))
    if not shards:
        raise FileNotFoundError(f"No train_shard_*.jsonl files in {data_dir}")
    picked = []
    for i in parse_shard_range(shard_range, len(shards)):
        if 0 <= i < len(shards):
            picked.append(shards[i])
        else:
            logger.warning("Shard index %d out of range (max %d)", i, len(shards) - 1)
    return picked


def read_records(path: str) -> List[dict]:
    """The records of a JSONL shard; blank and malformed lines are skipped."""
    out = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            try:
                out.append(json.loads(line))
            except json.JSONDecodeError:
                continue
    return out


def build_positive_corpus(shard_files: Sequence[str], max_corpus: int) -> List[str]:
    """Unique non-empty ``positive`` texts in file order, at most ``max_corpus``; reading stops once the cap is reached."""
    seen, corpus = set(), []
    for path in shard_files:
        if len(corpus) >= max_corpus:
            break
        with open(path, encoding="utf-8") as f:
            for line in f:
                if len(corpus) >= max_corpus:
                    break
                line = line.strip()
                if not line:
                    continue
                try:
                    rec = json.loads(line)
                except json.JSONDecodeError:
                    continue
                pos = rec.get("positive", "")
                if pos and pos not in seen:
                    seen.add(pos)
                    corpus.append(pos)
    return corpus


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def write_records(records: Sequence[dict], out_path: str) -> None:
    """One JSON object per line through a temporary file in the target's directory and a rename."""
    folder = os.path.dirname(os.path.abspath(out_path))
    os.makedirs(folder, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=folder, prefix=".tmp_", suffix=".jsonl")
    try:
        with os.fdopen(fd, "w", encoding="utf-8") as f:
            for rec in records:
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")
        os.replace(tmp, out_path)
    except Exception:
        os.unlink(tmp)
        raise


def mine_shard(shard_file: str, index, corpus: Sequence[str], *, top_k: int = 10, batch_size: int = 1000,
               output_dir: Optional[str] = None, dry_run: bool = False) -> Dict[str, int]:
    """Fill the missing negatives of one shard from a built ``index`` over ``corpus``; -> its stats."""
    records = read_records(shard_file)
    stats = dict.fromkeys(STAT_KEYS, 0)
    stats["total"] = len(records)
    need = [i for i, rec in enumerate(records) if not rec.get("negative")]
    stats["already_had_negative"] = len(records) - len(need)
    if not need:
        return stats
    k = min(int(top_k), len(corpus))
    for b0 in range(0, len(need), int(batch_size)):
        batch = need[b0:b0 + int(batch_size)]
        docs = None
        if k >= 1:
            docs = _host(index.search_texts([records[i].get("query", "") for i in batch], k)[1])
        for j, i in enumerate(batch):
            positive = records[i].get("positive", "")
            negative = None
            for d in (docs[j] if docs is not None else ()):
                if d >= 0 and corpus[int(d)] != positive:     # -1: fewer than k documents share an n-gram with the query
                    negative = corpus[int(d)]
                    break
            if negative:
                records[i]["negative"] = negative
                records[i]["difficulty"] = "hard"
                stats["added"] += 1
            else:
                stats["failed"] += 1
    if not dry_run:
        out = shard_file if output_dir is None else os.path.join(output_dir, os.path.basename(shard_file))
        write_records(records, out)
    return stats


def mine_tfidf_negatives(shard_files: Sequence[str], index, *, output_dir: Optional[str] = None, max_corpus: int = 50000,
                         top_k: int = 10, batch_size: int = 1000, dry_run: bool = False, fit_batch: int = 65536) -> dict:
    """The whole step over ``shard_files``: corpus, fit and build of ``index`` (handed over empty), then every shard.
    ``output_dir=None`` rewrites the shards in place.  -> the summed stats, with ``corpus`` (its size) and ``shards`` (the
    per-shard stats in order)."""
    shard_files = list(shard_files)
    corpus = build_positive_corpus(shard_files, int(max_corpus))
    for b0 in range(0, len(corpus), int(fit_batch)):
        index.fit_add(corpus[b0:b0 + int(fit_batch)])
    if corpus:
        index.build()
    per_shard = [mine_shard(f, index, corpus, top_k=top_k, batch_size=batch_size, output_dir=output_dir, dry_run=dry_run)
                 for f in shard_files]
    out = {key: sum(s[key] for s in per_shard) for key in STAT_KEYS}
    out["corpus"] = len(corpus)
    out["shards"] = per_shard
    return out
