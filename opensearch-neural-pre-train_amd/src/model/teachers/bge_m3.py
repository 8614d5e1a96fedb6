"""BGE-M3 dense teacher for knowledge distillation (ref:src/model/teachers/bge_m3.py) on the native encoder.

The reference wraps ``SentenceTransformer("BAAI/bge-m3")``; here the XLM-RoBERTa forward and CLS pooling run in
``snx.teacher.TeacherEncoder`` (csrc/teacher.hip) and the model is read from a LOCAL directory -- a model name is never
resolved.  Methods, argument names, defaults and return values are the reference's; ``get_batch_soft_labels`` encodes all
documents of the batch in one call instead of one call per query (same values)."""
from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from snx.teacher import (DEFAULT_BATCH_TOKENS, TeacherEncoder, lexical_pairs, lexical_pairs_torch, maxsim_pairs,
                         maxsim_pairs_torch)

SCORE_MODES = ("dense", "colbert", "dense+colbert", "sparse", "dense+sparse", "sparse+colbert", "dense+sparse+colbert")


def combine_scores(dense, colbert, weights: Tuple[float, float] = (1.0, 1.0)):
    """(w_dense * dense + w_colbert * colbert) / (w_dense + w_colbert): the weighted mean of the two teacher scores."""
    w_dense, w_colbert = float(weights[0]), float(weights[1])
    if w_dense < 0 or w_colbert < 0 or w_dense + w_colbert <= 0:
        raise ValueError("combine_scores: the weights must be non-negative and not both zero")
    return (w_dense * dense + w_colbert * colbert) / (w_dense + w_colbert)


def combine_modes(scores: Dict[str, torch.Tensor], weights: Dict[str, float]):
    """The weighted mean of the teacher scores present: sum_m weights[m] * scores[m] / sum_m weights[m] over the modes m of
    ``scores`` ("dense", "sparse", "colbert"); ``combine_scores``' weight rules: non-negative, not all zero."""
    if not scores or any(m not in weights for m in scores):
        raise ValueError("combine_modes: every score needs a weight, and there must be one score at least")
    w = {m: float(weights[m]) for m in scores}
    if any(v < 0 for v in w.values()) or sum(w.values()) <= 0:
        raise ValueError("combine_modes: the weights must be non-negative and not all zero")
    return sum(w[m] * scores[m] for m in scores) / sum(w.values())


def mode_weights(weights, pair: bool = False):
    """``get_ranking_scores``' ``weights`` as ``combine_modes``' dict: (w_dense, w_colbert), (w_dense, w_sparse, w_colbert) or
    a dict by mode, a missing weight 1.  ``pair``: as ``combine_scores``' (w_dense, w_colbert) instead."""
    if isinstance(weights, dict):
        w = {m: float(weights.get(m, 1.0)) for m in ("dense", "sparse", "colbert")}
    elif len(weights) == 3:
        w = {"dense": float(weights[0]), "sparse": float(weights[1]), "colbert": float(weights[2])}
    elif len(weights) == 2:
        w = {"dense": float(weights[0]), "sparse": 1.0, "colbert": float(weights[1])}
    else:
        raise ValueError("weights: (w_dense, w_colbert), (w_dense, w_sparse, w_colbert) or a dict by mode")
    return (w["dense"], w["colbert"]) if pair else w


def lexical_scores(lex_ptr, ids: torch.Tensor, w: torch.Tensor, pair_q, pair_d) -> torch.Tensor:
    """The native scorer for lexical weights on a GPU; a CPU encoder's go through the float64 restatement."""
    if w.device.type == "cuda":
        return lexical_pairs(lex_ptr, ids, w, pair_q, pair_d)
    return lexical_pairs_torch(lex_ptr, ids, w, pair_q, pair_d).to(torch.float32)


def maxsim_scores(mv: torch.Tensor, mv_ptr, pair_q, pair_d) -> torch.Tensor:
    """The native scorer for a store on a GPU; a CPU encoder's store goes through the float64 restatement."""
    if mv.device.type == "cuda":
        return maxsim_pairs(mv, mv_ptr, pair_q, pair_d)
    return maxsim_pairs_torch(mv, mv_ptr, pair_q, pair_d).to(torch.float32)


def _load_tokenizer(model_dir: str):
    try:
        from transformers import AutoTokenizer
    except ImportError as e:
        raise ImportError("BGEM3Teacher: pass tokenizer=..., or install transformers to read the one in model_dir") from e
    return AutoTokenizer.from_pretrained(model_dir, local_files_only=True)


class BGEM3Teacher(nn.Module):
    """BGE-M3 as teacher model: dense embeddings, soft labels for contrastive distillation, ranking scores.

    ``model_dir``: a local HF / sentence-transformers directory (``TeacherEncoder.from_pretrained``), or a ready
    ``TeacherEncoder``.  ``tokenizer``: an HF tokenizer, or ``"gpu:DIR"`` / ``"unigram:DIR"`` for the native Unigram tokenizer
    of ``DIR/tokenizer.json`` (snx.unigram) on the teacher's GPU / in plain Python; default: the one stored in ``model_dir``."""

    def __init__(self, model_dir: Union[str, TeacherEncoder] = "BAAI/bge-m3", device: str = "cuda", max_length: int = 512,
                 normalize_embeddings: bool = True, tokenizer=None, precision: str = "bf16",
                 batch_tokens: int = DEFAULT_BATCH_TOKENS):
        super().__init__()
        self.model_name = model_dir if isinstance(model_dir, str) else None
        self.device = device
        self.max_length = max_length
        self.normalize_embeddings = normalize_embeddings
        self.batch_tokens = batch_tokens
        if isinstance(model_dir, TeacherEncoder):
            self.model = model_dir.to(device)
            if tokenizer is None:
                raise ValueError("BGEM3Teacher: a ready TeacherEncoder needs tokenizer=...")
        else:
            self.model = TeacherEncoder.from_pretrained(model_dir, device=device, precision=precision)
        if isinstance(tokenizer, str):
            if not tokenizer.startswith(("gpu:", "unigram:")):
                raise ValueError("BGEM3Teacher: a tokenizer given by name must be gpu:DIR or unigram:DIR")
            from src.train.data.collator import create_tokenizer
            tokenizer = create_tokenizer(tokenizer, device=self.model.device)
        self.tokenizer = tokenizer if tokenizer is not None else _load_tokenizer(model_dir)

    @torch.no_grad()
    def encode(self, texts: Union[str, List[str]], batch_size: int = 32, show_progress: bool = False) -> torch.Tensor:
        """Texts -> dense embeddings [num_texts, hidden] on ``device``."""
        if isinstance(texts, str):
            texts = [texts]
        return self.model.encode(texts, self.tokenizer, batch_size=None, max_length=self.max_length,
                                 batch_tokens=self.batch_tokens, normalize=self.normalize_embeddings)

    @torch.no_grad()
    def compute_similarity(self, query_embeds: torch.Tensor, doc_embeds: torch.Tensor) -> torch.Tensor:
        """Cosine similarity matrix [batch_size, num_docs]."""
        if self.normalize_embeddings:
            query_embeds = F.normalize(query_embeds, p=2, dim=-1)
            doc_embeds = F.normalize(doc_embeds, p=2, dim=-1)
        return torch.mm(query_embeds, doc_embeds.t())

    @torch.no_grad()
    def get_ranking_scores(self, queries: List[str], documents: List[str], batch_size: int = 32, mode: str = "dense",
                           weights=(1.0, 1.0)) -> torch.Tensor:
        """Teacher scores of query-document pairs [num_pairs].  ``mode``: "dense" (the CLS cosine, the reference's
        score), "colbert" (MaxSim over the multi-vector rows), "sparse" (lexical matching over the lexical weights) or
        several joined by "+": their weighted mean.  ``weights``: (w_dense, w_colbert), (w_dense, w_sparse, w_colbert) or a
        dict by mode; a weight that is not given is 1.  The colbert modes need a model directory with
        ``colbert_linear.pt``, the sparse modes one with ``sparse_linear.pt``."""
        assert len(queries) == len(documents), "Must have same number of queries and docs"
        if mode not in SCORE_MODES:
            raise ValueError(f"get_ranking_scores: mode must be one of {SCORE_MODES}")
        if mode == "dense":
            query_embeds = self.encode(queries, batch_size=batch_size)
            doc_embeds = self.encode(documents, batch_size=batch_size)
            return (query_embeds * doc_embeds).sum(dim=-1)
        n = len(queries)
        pair_q, pair_d = torch.arange(n), torch.arange(n, 2 * n)
        if "sparse" not in mode:
            emb, mv_ptr, mv = self.encode_multivector(list(queries) + list(documents))
            colbert = maxsim_scores(mv, mv_ptr, pair_q, pair_d)
            if mode == "colbert":
                return colbert
            return combine_scores((emb[:n] * emb[n:]).sum(dim=-1), colbert, mode_weights(weights, pair=True))
        if "colbert" in mode and not self.model.has_multivector:
            raise ValueError("teacher: this encoder has no multi-vector head (no colbert_linear.pt in the model directory)")
        emb, mv_ptr, mv, lex_ptr, lex_ids, lex_w = self.encode_m3(list(queries) + list(documents))
        scores = {"sparse": lexical_scores(lex_ptr, lex_ids, lex_w, pair_q, pair_d)}
        if "dense" in mode:
            scores["dense"] = (emb[:n] * emb[n:]).sum(dim=-1)
        if "colbert" in mode:
            scores["colbert"] = maxsim_scores(mv, mv_ptr, pair_q, pair_d)
        return combine_modes(scores, mode_weights(weights))

    @torch.no_grad()
    def encode_m3(self, texts: List[str]):
        """Texts -> (dense embeddings, mv_ptr, multi-vector rows | None, lex_ptr, lex_ids, lex_w) of one forward
        (``TeacherEncoder.encode_m3``)."""
        return self.model.encode_m3(texts, self.tokenizer, max_length=self.max_length, batch_tokens=self.batch_tokens)

    @torch.no_grad()
    def compute_lexical_scores(self, queries: List[str], documents_per_query: List[List[str]]) -> List[torch.Tensor]:
        """Lexical matching scores: per query one fp32 tensor [len(documents_per_query[i])].  Every distinct text is
        encoded once."""
        assert len(queries) == len(documents_per_query), "Must have one document list per query"
        row: Dict[str, int] = {}
        for t in list(queries) + [d for docs in documents_per_query for d in docs]:
            row.setdefault(t, len(row))
        pairs = [(row[q], row[d]) for q, docs in zip(queries, documents_per_query) for d in docs]
        if not pairs:
            return [torch.zeros(0, device=self.model.device) for _ in queries]
        _, _, _, lex_ptr, lex_ids, lex_w = self.encode_m3(list(row))
        scores = lexical_scores(lex_ptr, lex_ids, lex_w, torch.tensor([p[0] for p in pairs]),
                                torch.tensor([p[1] for p in pairs]))
        return list(torch.split(scores, [len(docs) for docs in documents_per_query]))

    @torch.no_grad()
    def encode_multivector(self, texts: List[str]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Texts -> (dense embeddings [n, hidden], mv_ptr [n + 1], multi-vector rows) of one forward
        (``TeacherEncoder.encode_multivector``)."""
        return self.model.encode_multivector(texts, self.tokenizer, max_length=self.max_length,
                                             batch_tokens=self.batch_tokens)

    @torch.no_grad()
    def compute_multivector_scores(self, queries: List[str], documents_per_query: List[List[str]]) -> List[torch.Tensor]:
        """MaxSim (late-interaction) scores: per query one fp32 tensor [len(documents_per_query[i])].  Every distinct text
        is encoded once."""
        assert len(queries) == len(documents_per_query), "Must have one document list per query"
        row: Dict[str, int] = {}
        for t in list(queries) + [d for docs in documents_per_query for d in docs]:
            row.setdefault(t, len(row))
        pairs = [(row[q], row[d]) for q, docs in zip(queries, documents_per_query) for d in docs]
        if not pairs:
            return [torch.zeros(0, device=self.model.device) for _ in queries]
        _, mv_ptr, mv = self.encode_multivector(list(row))
        scores = maxsim_scores(mv, mv_ptr, torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs]))
        return list(torch.split(scores, [len(docs) for docs in documents_per_query]))

    @torch.no_grad()
    def get_soft_labels(self, query: str, positive_doc: str, negative_docs: List[str],
                        temperature: float = 2.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(softmax over [positive, *negatives] at ``temperature``, raw similarities)."""
        query_embed = self.encode(query)
        doc_embeds = self.encode([positive_doc] + negative_docs)
        similarities = self.compute_similarity(query_embed, doc_embeds).squeeze(0)
        return F.softmax(similarities / temperature, dim=-1), similarities

    @torch.no_grad()
    def get_batch_soft_labels(self, queries: List[str], positive_docs: List[str], negative_docs: List[List[str]],
                              temperature: float = 2.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """Soft labels of a batch of triplets -> (soft_labels, raw_scores), both [batch_size, 1 + num_neg]."""
        batch_size = len(queries)
        docs = [[positive_docs[i]] + (list(negative_docs[i]) if negative_docs else []) for i in range(batch_size)]
        width = len(docs[0]) if docs else 0
        if any(len(d) != width for d in docs):
            raise ValueError("get_batch_soft_labels: every query needs the same number of negatives")
        query_embeds = self.encode(queries)
        doc_embeds = self.encode([t for d in docs for t in d]).reshape(batch_size, width, -1)
        if self.normalize_embeddings:
            query_embeds = F.normalize(query_embeds, p=2, dim=-1)
            doc_embeds = F.normalize(doc_embeds, p=2, dim=-1)
        raw_scores = torch.bmm(doc_embeds, query_embeds.unsqueeze(-1)).squeeze(-1)
        return F.softmax(raw_scores / temperature, dim=-1), raw_scores

    @torch.no_grad()
    def get_in_batch_soft_labels(self, queries: List[str], documents: List[str], temperature: float = 2.0) -> torch.Tensor:
        """Row-wise softmax of the full query x document similarity matrix [batch_size, batch_size]."""
        similarity = self.compute_similarity(self.encode(queries), self.encode(documents))
        return F.softmax(similarity / temperature, dim=-1)

    def to(self, device: str) -> "BGEM3Teacher":
        """Move the teacher to ``device``."""
        self.device = device
        self.model = self.model.to(device)
        return self


def create_bge_m3_teacher(model_dir: str = "BAAI/bge-m3", device: str = "cuda", max_length: int = 512,
                          tokenizer=None) -> BGEM3Teacher:
    """Factory of the reference; ``model_dir`` must be a local directory."""
    return BGEM3Teacher(model_dir=model_dir, device=device, max_length=max_length, tokenizer=tokenizer)


class KDLossWithBGEM3(nn.Module):
    """Knowledge distillation against the teacher: KL(teacher || student) on in-batch soft labels plus MSE on raw scores,
    total = kl_weight * T^2 * kl + mse_weight * mse."""

    def __init__(self, teacher: BGEM3Teacher, kl_weight: float = 1.0, mse_weight: float = 0.5, temperature: float = 2.0):
        super().__init__()
        self.teacher = teacher
        self.kl_weight = kl_weight
        self.mse_weight = mse_weight
        self.temperature = temperature

    def forward(self, student_scores: torch.Tensor, queries: List[str], documents: List[str]) -> Dict[str, torch.Tensor]:
        """``student_scores`` [batch_size, batch_size] -> {'total', 'kl', 'mse'}."""
        with torch.no_grad():
            teacher_scores = self.teacher.compute_similarity(self.teacher.encode(queries), self.teacher.encode(documents))
            teacher_soft_labels = F.softmax(teacher_scores / self.temperature, dim=-1)
        student_log_probs = F.log_softmax(student_scores / self.temperature, dim=-1)
        kl_loss = F.kl_div(student_log_probs, teacher_soft_labels, reduction="batchmean")
        mse_loss = F.mse_loss(student_scores, teacher_scores)
        total_loss = self.kl_weight * (self.temperature ** 2) * kl_loss + self.mse_weight * mse_loss
        return {"total": total_loss, "kl": kl_loss, "mse": mse_loss}
