"""BGE-M3 dense teacher for knowledge distillation (ref:src/model/teachers/bge_m3.py) on the native encoder.

The reference wraps ``SentenceTransformer("BAAI/bge-m3")``; here the XLM-RoBERTa forward and CLS pooling run in
``snx.teacher.TeacherEncoder`` (csrc/teacher.hip) and the model is read from a LOCAL directory -- a model name is never
resolved.  Methods, argument names, defaults and return values are the reference's; ``get_batch_soft_labels`` encodes all
documents of the batch in one call instead of one call per query (same values)."""
from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from snx.teacher import DEFAULT_BATCH_TOKENS, TeacherEncoder


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
    def get_ranking_scores(self, queries: List[str], documents: List[str], batch_size: int = 32) -> torch.Tensor:
        """Teacher scores of query-document pairs [num_pairs]."""
        assert len(queries) == len(documents), "Must have same number of queries and docs"
        query_embeds = self.encode(queries, batch_size=batch_size)
        doc_embeds = self.encode(documents, batch_size=batch_size)
        return (query_embeds * doc_embeds).sum(dim=-1)

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
