"""MLM corpus preparation (ref:scripts/prepare_korean_mlm_data.py): raw documents to the ``train.txt`` / ``val.txt`` that
``src.train.cli.pretrain_mlm`` reads, one paragraph per line.

The device does the streaming over code points (snx.textprep): blank runs, paragraph cuts, strip, Hangul count, the
validity filter, SHA-256 of every valid paragraph and the first-occurrence dedup over the whole corpus.  Documents go to the
device in batches bounded by code points; invalid paragraphs are discarded per batch, the valid ones wait on the host as
code points and their digests accumulate on the device (32 bytes each); the dedup runs once at the end over all of them
in input order, so the result does not depend on the batch size.  The host keeps what the reference does with Python's own
``random`` and ``sum``: shuffle, split, write, statistics (``finish_corpus``)."""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

DEFAULT_BATCH_CODE_POINTS = 1 << 24    # 64 MiB of code points a batch


@dataclass
class ValidBatch:
    """What one batch of documents leaves behind: its valid paragraphs as a host CSR of code points, per paragraph the
    Hangul count and the document (index in the batch), per document the pieces before the filter, and the digests."""
    ptr: np.ndarray                    # int64 [v + 1]
    cps: np.ndarray                    # int32
    hangul: np.ndarray                 # int32 [v]
    doc: np.ndarray                    # int32 [v]
    doc_pieces: np.ndarray             # int64 [documents of the batch]
    digests: object                    # uint32 [v, 8]: a tensor on the device (a numpy array from a host stage)


@dataclass
class MlmCorpus:
    train: List[str]
    val: List[str]
    stats: Dict[str, float]
    documents: int = 0
    pieces: int = 0
    valid: int = 0
    unique: int = 0
    report: List[Dict[str, int]] = field(default_factory=list)   # per input document, in input order


def batch_stage(doc_ptr: np.ndarray, doc_cps: np.ndarray, min_length: int, min_korean_ratio: float, device) -> ValidBatch:
    """One batch of documents, packed as a CSR of code points, on the GPU: segment, filter, hash the valid paragraphs."""
    import torch
    from snx import textprep as tx
    seg = tx.segment_csr(doc_ptr, doc_cps, device)
    keep = torch.nonzero(tx.valid_mask(seg.lengths, seg.par_hangul, min_length, min_korean_ratio)).flatten()
    ptr, cps = tx.gather_rows(seg.par_ptr, seg.par_cps, keep)
    digests = tx.sha256_rows(ptr, cps)
    doc_pieces = torch.bincount(seg.par_doc.long(), minlength=doc_ptr.size - 1)
    return ValidBatch(ptr.cpu().numpy(), cps.cpu().numpy(), seg.par_hangul[keep].cpu().numpy(),
                      seg.par_doc[keep].cpu().numpy(), doc_pieces.cpu().numpy(), digests)


def dedup_stage(digests: list) -> np.ndarray:
    """The digests of all batches in input order -> first [n]: the smallest index with the same digest."""
    import torch
    from snx import textprep as tx
    if not digests:
        return np.zeros(0, dtype=np.int64)
    return tx.first_equal(torch.cat(digests)).cpu().numpy().astype(np.int64)


def split_indices(n: int, val_ratio: float, seed: int) -> Tuple[List[int], List[int]]:
    """The reference's ``split_train_val`` (ref:prepare_korean_mlm_data.py:220-239) on the indices 0 .. n-1:
    ``random.shuffle`` permutes positions, so shuffling indices gives the permutation it gives the paragraphs."""
    random.seed(seed)
    order = list(range(n))
    random.shuffle(order)
    cut = max(1, int(n * (1 - val_ratio)))
    return order[:cut], order[cut:]


def line_bytes(paragraphs: Iterable[str]) -> bytes:
    """The file ``save_lines`` writes (ref:prepare_korean_mlm_data.py:242-252): U+000A becomes U+0020, nothing else."""
    return "".join(p.replace("\n", " ") + "\n" for p in paragraphs).encode("utf-8")


def finish_corpus(unique: Sequence[str], lengths: Sequence[int], hangul: Sequence[int], val_ratio: float = 0.05,
                  seed: int = 42) -> MlmCorpus:
    """The host-only tail (rules 6-8): shuffle and split the deduplicated paragraphs, and the reference's statistics
    (ref:prepare_korean_mlm_data.py:255-274): both means are Python ``sum`` in train-then-val order over the total."""
    n = len(unique)
    if len(lengths) != n or len(hangul) != n:
        raise ValueError("finish_corpus: one length and one Hangul count per paragraph")
    if n == 0:
        return MlmCorpus([], [], {"total": 0, "train": 0, "val": 0, "mean_length": 0, "mean_korean_ratio": 0})
    tr, va = split_indices(n, val_ratio, seed)
    lengths, hangul = [int(x) for x in lengths], [int(x) for x in hangul]
    order = tr + va
    stats = {"total": n, "train": len(tr), "val": len(va),
             "mean_length": sum(lengths[i] for i in order) / n,
             "mean_korean_ratio": sum((hangul[i] / lengths[i] if lengths[i] else 0.0) for i in order) / n}
    return MlmCorpus([unique[i] for i in tr], [unique[i] for i in va], stats)


def write_corpus(corpus: MlmCorpus, output_dir: str) -> None:
    import os
    os.makedirs(output_dir, exist_ok=True)
    for name, rows in (("train.txt", corpus.train), ("val.txt", corpus.val)):
        with open(os.path.join(output_dir, name), "wb") as f:
            f.write(line_bytes(rows))


def _batches(sources, batch_code_points: int) -> Iterator[List[Tuple[int, int, str]]]:
    """(source, index in the source, text) of every document, cut into batches of at most ``batch_code_points`` code points
    (a longer document is a batch of its own)."""
    batch, size = [], 0
    for s, docs in enumerate(sources):
        for i, text in enumerate(docs):
            if not isinstance(text, str):
                raise ValueError(f"prepare_mlm_corpus: source {s}, document {i}: not a string")
            if batch and size + len(text) > batch_code_points:
                yield batch
                batch, size = [], 0
            batch.append((s, i, text))
            size += len(text)
    if batch:
        yield batch


def kept_paragraphs(parts: Sequence[ValidBatch], is_first: np.ndarray) -> Tuple[List[str], List[int], List[int]]:
    """The first occurrences among the valid paragraphs of all batches -> (texts, lengths, Hangul counts), in input order.
    Only these become ``str``."""
    from snx.textprep import csr_texts
    unique: List[str] = []
    lengths: List[int] = []
    hangul: List[int] = []
    at = 0
    for vb in parts:
        v = vb.hangul.size
        rows = np.nonzero(is_first[at:at + v])[0]
        at += v
        lens = vb.ptr[rows + 1] - vb.ptr[rows]
        if rows.size:
            out_ptr = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
            src = np.repeat(vb.ptr[rows] - out_ptr[:-1], lens) + np.arange(int(out_ptr[-1]), dtype=np.int64)
            unique += csr_texts(out_ptr, vb.cps[src])
        lengths += lens.tolist()
        hangul += vb.hangul[rows].tolist()
    return unique, lengths, hangul


def prepare_mlm_corpus(sources: Sequence[Iterable[str]], min_length: int = 50, min_korean_ratio: float = 0.3,
                       val_ratio: float = 0.05, seed: int = 42, batch_code_points: int = DEFAULT_BATCH_CODE_POINTS,
                       device="cuda", source_names: Optional[Sequence[str]] = None) -> MlmCorpus:
    """``sources``: iterables of documents (``str``), concatenated in order as the reference concatenates Wikipedia and
    mC4 (ref:prepare_korean_mlm_data.py:337).  -> the train and val paragraphs, the statistics and the counts."""
    from snx.textprep import LoneSurrogateError, code_point_csr
    if isinstance(min_length, bool) or not isinstance(min_length, (int, np.integer)):
        raise ValueError("prepare_mlm_corpus: min_length must be an int")
    if not 0.0 <= float(val_ratio) < 1.0:
        raise ValueError("prepare_mlm_corpus: val_ratio must be in [0, 1)")
    if isinstance(batch_code_points, bool) or int(batch_code_points) < 1:
        raise ValueError("prepare_mlm_corpus: batch_code_points must be >= 1")
    names = list(source_names) if source_names is not None else [f"source {s}" for s in range(len(sources))]
    parts: List[ValidBatch] = []
    digests = []
    report: List[Dict[str, int]] = []
    doc_of: List[np.ndarray] = []                            # per valid paragraph: its document among all documents
    for batch in _batches(sources, int(batch_code_points)):
        try:
            doc_ptr, doc_cps = code_point_csr([t for _, _, t in batch], "prepare_mlm_corpus")
        except LoneSurrogateError as e:
            s, i, _ = batch[e.index]
            raise ValueError(f"prepare_mlm_corpus: {names[s]}, document {i}: the text holds a lone surrogate "
                             "(U+D800..U+DFFF), which has no UTF-8 form") from None
        vb = batch_stage(doc_ptr, doc_cps, int(min_length), float(min_korean_ratio), device)
        valid_per_doc = np.bincount(vb.doc, minlength=len(batch))
        doc_of.append(vb.doc.astype(np.int64) + len(report))
        for (s, i, _), p, v in zip(batch, vb.doc_pieces.tolist(), valid_per_doc.tolist()):
            report.append({"source": s, "document": i, "pieces": int(p), "valid": int(v), "kept": 0})
        parts.append(vb)
        digests.append(vb.digests)
    first = dedup_stage(digests)
    n_valid = int(first.size)
    is_first = first == np.arange(n_valid, dtype=np.int64)
    unique, lengths, hangul = kept_paragraphs(parts, is_first)
    if doc_of:
        for d in np.concatenate(doc_of)[is_first].tolist():
            report[d]["kept"] += 1
    corpus = finish_corpus(unique, lengths, hangul, val_ratio, seed)
    corpus.documents, corpus.pieces = len(report), sum(r["pieces"] for r in report)
    corpus.valid, corpus.unique, corpus.report = n_valid, len(unique), report
    return corpus
