"""Graded evaluation of term expansion (ref:src/evaluation/ranking_metrics.py): Recall@K, MRR and nDCG@K of a source term's
judged synonyms (grade 3 exact, 2 partial, 1 related) in the model's own ranking of the vocabulary, per query, aggregated,
per domain, and compared between two checkpoints.

What runs where.  The device (snx.expansion, csrc/expansion.hip) finds where each judged id falls in the ranking of its
row -- a count over the row, no sort, no per-element copy to the host -- and folds the gains; one call and one copy back
per batch.  The host keeps the reference's rules the device does not see: a token counts only when it encodes to exactly
one id; the recall / MRR set is the distinct resolved ids of tokens with grade >= min_grade, while DCG reads the id -> grade
map in which a later token overwrites an earlier one of the same id; IDCG comes from all judgments, resolved or not;
first_relevant_rank is int(1 / mrr); means and medians are numpy's.  The ranking itself (include/snx.h): entries with
weight > 0 that are not special ids, weight descending, ties lowest id first, cut after max_k."""
from __future__ import annotations

import json
import math
import warnings
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Set, Tuple, Union

import numpy as np
import torch

GRADES = (0, 1, 2, 3)
SAMPLE_DATASET = Path(__file__).resolve().parents[3] / "tests" / "golden" / "g20_expansion" / "sample_dataset.json"


@dataclass
class GradedRelevance:
    """The judgments of one source term: token -> grade (3 exact synonym, 2 partial, 1 related, 0 not relevant)."""
    query: str
    relevance_judgments: Dict[str, int]
    domain: Optional[str] = None

    def __post_init__(self):
        for token, grade in self.relevance_judgments.items():
            if grade not in GRADES:
                raise ValueError(f"Invalid relevance grade {grade} for token '{token}'. Must be 0, 1, 2, or 3.")

    def get_relevant_tokens(self, min_grade: int = 1) -> Set[str]:
        return {t for t, g in self.relevance_judgments.items() if g >= min_grade}

    def get_tokens_by_grade(self, grade: int) -> Set[str]:
        return {t for t, g in self.relevance_judgments.items() if g == grade}

    def ideal_ranking(self, k: Optional[int] = None) -> List[Tuple[str, int]]:
        """(token, grade) by grade descending (stable: equal grades keep the dict's order), the first ``k``."""
        best = sorted(self.relevance_judgments.items(), key=lambda item: item[1], reverse=True)
        return best if k is None else best[:k]

    def to_dict(self) -> Dict:
        return {"query": self.query, "relevance_judgments": self.relevance_judgments, "domain": self.domain}

    @classmethod
    def from_dict(cls, data: Dict) -> "GradedRelevance":
        return cls(query=data["query"], relevance_judgments=data["relevance_judgments"], domain=data.get("domain"))


@dataclass
class EvaluationDataset:
    queries: List[GradedRelevance]
    name: str = "evaluation_dataset"
    version: str = "1.0"

    def __len__(self) -> int:
        return len(self.queries)

    def __iter__(self):
        return iter(self.queries)

    def __getitem__(self, idx: int) -> GradedRelevance:
        return self.queries[idx]

    def filter_by_domain(self, domain: str) -> "EvaluationDataset":
        return EvaluationDataset(queries=[q for q in self.queries if q.domain == domain], name=f"{self.name}_{domain}",
                                 version=self.version)

    def get_domains(self) -> Set[str]:
        return {q.domain for q in self.queries if q.domain is not None}

    def statistics(self) -> Dict:
        grades = [g for q in self.queries for g in q.relevance_judgments.values()]
        return {"num_queries": len(self.queries), "total_judgments": len(grades),
                "avg_judgments_per_query": len(grades) / len(self.queries) if self.queries else 0,
                "grade_distribution": {g: grades.count(g) for g in GRADES}, "domains": list(self.get_domains())}

    def save(self, path: Union[str, Path]) -> None:
        data = {"name": self.name, "version": self.version, "queries": [q.to_dict() for q in self.queries]}
        with open(Path(path), "w", encoding="utf-8") as f:
            json.dump(data, f, ensure_ascii=False, indent=2)

    @classmethod
    def load(cls, path: Union[str, Path]) -> "EvaluationDataset":
        with open(Path(path), "r", encoding="utf-8") as f:
            data = json.load(f)
        return cls(queries=[GradedRelevance.from_dict(q) for q in data["queries"]],
                   name=data.get("name", "evaluation_dataset"), version=data.get("version", "1.0"))

    @classmethod
    def from_synonym_pairs(cls, synonym_data: List[Dict], name: str = "auto_generated") -> "EvaluationDataset":
        """One query per record {"source", "synonyms": {"exact": [...], "partial": [...], "related": [...]}, "domain"?}:
        exact -> 3, partial -> 2, related -> 1; a token named twice keeps the grade of the later list."""
        queries = []
        for item in synonym_data:
            lists = item.get("synonyms", {})
            judgments = {}
            for key, grade in (("exact", 3), ("partial", 2), ("related", 1)):
                for token in lists.get(key, []):
                    judgments[token] = grade
            queries.append(GradedRelevance(query=item["source"], relevance_judgments=judgments, domain=item.get("domain")))
        return cls(queries=queries, name=name)


@dataclass
class EvaluationResult:
    per_query_metrics: List[Dict] = field(default_factory=list)
    recall_at_k: Dict[int, float] = field(default_factory=dict)
    mrr: float = 0.0
    ndcg_at_k: Dict[int, float] = field(default_factory=dict)
    mean_first_relevant_rank: float = 0.0
    median_first_relevant_rank: float = 0.0
    num_queries: int = 0
    domain_metrics: Dict[str, Dict] = field(default_factory=dict)

    def summary(self) -> str:
        bar = "=" * 60
        out = [bar, "Evaluation Results Summary", bar, f"Number of queries: {self.num_queries}", "", "Recall@K:"]
        out += [f"  Recall@{k}: {v:.4f}" for k, v in sorted(self.recall_at_k.items())]
        out += ["", f"MRR: {self.mrr:.4f}", "", "nDCG@K:"]
        out += [f"  nDCG@{k}: {v:.4f}" for k, v in sorted(self.ndcg_at_k.items())]
        out += ["", f"Mean first relevant rank: {self.mean_first_relevant_rank:.2f}",
                f"Median first relevant rank: {self.median_first_relevant_rank:.2f}"]
        if self.domain_metrics:
            out += ["", "Per-Domain Results:"]
            for domain, m in self.domain_metrics.items():
                out += [f"  {domain}:", f"    MRR: {m.get('mrr', 0):.4f}"]
                out += [f"    nDCG@{k}: {v:.4f}" for k, v in sorted(m.get("ndcg_at_k", {}).items())]
        out.append(bar)
        return "\n".join(out)

    def to_dict(self) -> Dict:
        return {"per_query_metrics": self.per_query_metrics, "recall_at_k": self.recall_at_k, "mrr": self.mrr,
                "ndcg_at_k": self.ndcg_at_k, "mean_first_relevant_rank": self.mean_first_relevant_rank,
                "median_first_relevant_rank": self.median_first_relevant_rank, "num_queries": self.num_queries,
                "domain_metrics": self.domain_metrics}


def _gain(grade: int, position: int) -> float:
    return (2 ** grade - 1) / math.log2(position + 1)


class RankingMetrics:
    DEFAULT_K_VALUES = [5, 10, 20, 50, 100]
    SPECIAL_ATTRS = ("pad_token_id", "cls_token_id", "sep_token_id", "unk_token_id", "mask_token_id", "bos_token_id",
                     "eos_token_id")

    def __init__(self, tokenizer, k_values: Optional[List[int]] = None, special_tokens: Optional[Set[str]] = None):
        self.tokenizer = tokenizer
        self.k_values = k_values or self.DEFAULT_K_VALUES
        self.special_token_ids = self._get_special_token_ids(special_tokens)
        self._token_id_cache: Dict[str, Optional[int]] = {}
        self._excluded: Dict[Tuple[int, str], torch.Tensor] = {}

    # ------------------------------------------------------------------------------------------------ tokens
    def _get_special_token_ids(self, special_tokens: Optional[Set[str]] = None) -> Set[int]:
        ids = {getattr(self.tokenizer, a, None) for a in self.SPECIAL_ATTRS} - {None}
        ids.update(getattr(self.tokenizer, "additional_special_tokens_ids", ()))
        for token in special_tokens or ():
            ids.update(self.tokenizer.encode(token, add_special_tokens=False))
        return ids

    def _get_token_id(self, token: str) -> Optional[int]:
        """The id of a token that encodes to exactly one id; a token of several pieces (or none) has no id."""
        if token not in self._token_id_cache:
            ids = self.tokenizer.encode(token, add_special_tokens=False)
            self._token_id_cache[token] = ids[0] if len(ids) == 1 else None
        return self._token_id_cache[token]

    def _relevant_ids(self, ground_truth: GradedRelevance, min_grade: int = 1) -> Set[int]:
        ids = {self._get_token_id(t) for t in ground_truth.get_relevant_tokens(min_grade)}
        return ids - {None}

    def _grade_of(self, ground_truth: GradedRelevance) -> Dict[int, int]:
        out = {}
        for token, grade in ground_truth.relevance_judgments.items():
            tid = self._get_token_id(token)
            if tid is not None:
                out[tid] = grade                               # a later token of the same id overwrites
        return out

    # ------------------------------------------------------------------------------------------------ device side
    def _excluded_mask(self, V: int, device: torch.device) -> torch.Tensor:
        key = (V, str(device))
        if key not in self._excluded:
            ex = torch.zeros(V, dtype=torch.uint8)
            inside = [t for t in self.special_token_ids if 0 <= t < V]
            if inside:
                ex[torch.tensor(inside, dtype=torch.long)] = 1
            self._excluded[key] = ex.to(device)
        return self._excluded[key]

    @staticmethod
    def _rows_on_gpu(rows: torch.Tensor) -> torch.Tensor:
        rows = rows.detach()
        if rows.device.type != "cuda":
            rows = rows.to("cuda")                             # the kernels run on a GPU; there is no host path
        return rows.to(torch.float32).contiguous()

    def _sparse_to_ranking(self, sparse_repr: torch.Tensor, top_k: Optional[int] = None) -> List[Tuple[int, float]]:
        """[(token id, weight)] of the ranked entries, weight descending (ties lowest id first), at most ``top_k``
        (None: all of them).  snx.ops.sparse_topk with the special ids disallowed; it reports the survivors in id order
        when no more than ``top_k`` survive, and the host orders them then."""
        from snx.ops import sparse_topk
        row = self._rows_on_gpu(sparse_repr.reshape(1, -1))
        V = row.shape[1]
        if top_k is not None and min(top_k, V) <= 0:
            return []
        k = None if top_k is None or top_k > 16384 else int(top_k)
        vals, ids, cnt, srt = sparse_topk(row, 1 - self._excluded_mask(V, row.device), k)
        n = int(cnt[0])
        pairs = list(zip(ids[0, :n].tolist(), vals[0, :n].tolist()))
        if not int(srt[0]):
            pairs.sort(key=lambda p: (-p[1], p[0]))
        return pairs if top_k is None else pairs[:top_k]

    def _batch_metrics(self, rows: torch.Tensor, ground_truths: List[GradedRelevance], max_k: int) -> List[Dict]:
        """The per-query dicts of ``rows`` [B, V]: one graded_metrics call (per 8 cutoffs) and one copy back."""
        from snx.expansion import CUTOFFS_MAX, graded_metrics
        rows = self._rows_on_gpu(rows)
        B, V = rows.shape
        cuts = sorted(set(int(k) for k in self.k_values))
        if cuts and cuts[0] < 1:
            raise ValueError("k_values must be >= 1")
        judged, rel_ids = [], []
        for gt in ground_truths:
            rel = self._relevant_ids(gt)
            judged.append([(tid, g, tid in rel) for tid, g in self._grade_of(gt).items()])
            rel_ids.append(rel)
        excluded = self._excluded_mask(V, rows.device)
        nranked = first = None
        hits: Dict[int, np.ndarray] = {}
        dcg: Dict[int, np.ndarray] = {}
        for s in range(0, max(len(cuts), 1), CUTOFFS_MAX):
            part = cuts[s:s + CUTOFFS_MAX] or [int(max_k)]
            _, nr, fr, h, d = graded_metrics(rows, excluded, judged, part, max_k=int(max_k))
            back = torch.cat([nr.double(), fr.double(), h.double().reshape(-1), d.reshape(-1)]).cpu().numpy()
            nranked, first = back[:B].astype(np.int64), back[B:2 * B].astype(np.int64)
            hh = back[2 * B:2 * B + B * len(part)].reshape(B, len(part)).astype(np.int64)
            dd = back[2 * B + B * len(part):].reshape(B, len(part))
            for c, k in enumerate(part):
                hits[k], dcg[k] = hh[:, c], dd[:, c]
        out = []
        for b, gt in enumerate(ground_truths):
            m = {"query": gt.query, "domain": gt.domain, "num_ranked_tokens": int(nranked[b])}
            for k in self.k_values:
                m[f"recall@{k}"] = int(hits[int(k)][b]) / len(rel_ids[b]) if rel_ids[b] else 0.0
            m["mrr"] = 1.0 / int(first[b]) if first[b] else 0.0
            m["first_relevant_rank"] = int(1 / m["mrr"]) if m["mrr"] > 0 else float("inf")
            for k in self.k_values:
                idcg = self.compute_idcg(gt, k)
                m[f"ndcg@{k}"] = float(dcg[int(k)][b]) / idcg if idcg != 0 else 0.0
            out.append(m)
        return out

    # ------------------------------------------------------------------------------------------------ over a ranking list
    def compute_recall_at_k(self, ranking: List[Tuple[int, float]], ground_truth: GradedRelevance, k: int,
                            min_grade: int = 1) -> float:
        wanted = self._relevant_ids(ground_truth, min_grade)
        if not wanted:
            return 0.0
        return len(wanted & {tid for tid, _ in ranking[:k]}) / len(wanted)

    def compute_mrr(self, ranking: List[Tuple[int, float]], ground_truth: GradedRelevance, min_grade: int = 1) -> float:
        wanted = self._relevant_ids(ground_truth, min_grade)
        for position, (tid, _) in enumerate(ranking, start=1):
            if tid in wanted:
                return 1.0 / position
        return 0.0

    def compute_dcg(self, ranking: List[Tuple[int, float]], ground_truth: GradedRelevance, k: int) -> float:
        grade_of = self._grade_of(ground_truth)
        total = 0.0
        for position, (tid, _) in enumerate(ranking[:k], start=1):
            grade = grade_of.get(tid, 0)
            if grade > 0:
                total += _gain(grade, position)
        return total

    def compute_idcg(self, ground_truth: GradedRelevance, k: int) -> float:
        total = 0.0
        for position, (_, grade) in enumerate(ground_truth.ideal_ranking(k), start=1):
            if grade > 0:
                total += _gain(grade, position)
        return total

    def compute_ndcg(self, ranking: List[Tuple[int, float]], ground_truth: GradedRelevance, k: int) -> float:
        idcg = self.compute_idcg(ground_truth, k)
        return self.compute_dcg(ranking, ground_truth, k) / idcg if idcg != 0 else 0.0

    # ------------------------------------------------------------------------------------------------ evaluation
    def _default_max_k(self) -> int:
        return max(self.k_values) if self.k_values else 100

    def evaluate_single_query(self, sparse_repr: torch.Tensor, ground_truth: GradedRelevance,
                              max_k: Optional[int] = None) -> Dict:
        """``evaluate``'s path at one row: sparse_repr [V]."""
        max_k = self._default_max_k() if max_k is None else max_k
        return self._batch_metrics(sparse_repr.reshape(1, -1), [ground_truth], max_k)[0]

    def evaluate(self, model: torch.nn.Module, eval_dataset: EvaluationDataset, batch_size: int = 32,
                 device: Optional[torch.device] = None) -> EvaluationResult:
        if device is None:
            device = next(model.parameters()).device
        model.eval()
        queries = list(eval_dataset)
        per_query: List[Dict] = []
        for s in range(0, len(queries), batch_size):
            batch = queries[s:s + batch_size]
            enc = self.tokenizer([q.query for q in batch], padding=True, truncation=True, max_length=64,
                                 return_tensors="pt")
            enc = {k: v.to(device) for k, v in enc.items()}
            with torch.no_grad():
                sparse, _ = model(enc["input_ids"], enc["attention_mask"])
            per_query.extend(self._batch_metrics(sparse, batch, self._default_max_k()))
        return self._aggregate_metrics(per_query)

    def _aggregate_metrics(self, per_query_metrics: List[Dict]) -> EvaluationResult:
        result = EvaluationResult(per_query_metrics=per_query_metrics, num_queries=len(per_query_metrics))
        if not per_query_metrics:
            return result

        def mean_of(rows, key):
            return np.mean([m[key] for m in rows])

        for k in self.k_values:
            result.recall_at_k[k] = mean_of(per_query_metrics, f"recall@{k}")
        result.mrr = mean_of(per_query_metrics, "mrr")
        for k in self.k_values:
            result.ndcg_at_k[k] = mean_of(per_query_metrics, f"ndcg@{k}")
        found = [m["first_relevant_rank"] for m in per_query_metrics if m["first_relevant_rank"] != float("inf")]
        if found:
            result.mean_first_relevant_rank = np.mean(found)
            result.median_first_relevant_rank = np.median(found)
        for domain in {m.get("domain") for m in per_query_metrics if m.get("domain")}:
            rows = [m for m in per_query_metrics if m.get("domain") == domain]
            result.domain_metrics[domain] = {
                "num_queries": len(rows), "mrr": mean_of(rows, "mrr"),
                "recall_at_k": {k: mean_of(rows, f"recall@{k}") for k in self.k_values},
                "ndcg_at_k": {k: mean_of(rows, f"ndcg@{k}") for k in self.k_values}}
        return result


def _paired_t(diffs: np.ndarray) -> Tuple[float, float]:
    """Two-sided paired t-test without scipy: t = mean / sqrt(var / n) with the n - 1 variance, and the Student-t tail
    I_{df / (df + t^2)}(df / 2, 1 / 2) through src.train.eval.betainc."""
    from src.train.eval import betainc
    n = diffs.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = float(np.mean(diffs) / np.sqrt(np.sum((diffs - np.mean(diffs)) ** 2) / (n - 1) / n))
    if np.isnan(t):
        return t, float("nan")
    if np.isinf(t):
        return t, 0.0
    df = float(n - 1)
    return t, betainc(0.5 * df, 0.5, df / (df + t * t))


@dataclass
class ModelComparison:
    """Paired statistics between two checkpoints evaluated on the same queries."""
    model_a_name: str
    model_b_name: str
    metrics_compared: Dict[str, Dict] = field(default_factory=dict)

    @staticmethod
    def paired_t_test(scores_a: List[float], scores_b: List[float], alpha: float = 0.05) -> Dict:
        if len(scores_a) != len(scores_b):
            raise ValueError("Score lists must have same length")
        if len(scores_a) < 2:
            return {"t_statistic": None, "p_value": None, "significant": False, "error": "Insufficient samples for t-test"}
        diffs = [a - b for a, b in zip(scores_a, scores_b)]
        try:
            from scipy import stats
            t_stat, p_value = stats.ttest_rel(scores_a, scores_b)
        except ImportError:
            t_stat, p_value = _paired_t(np.asarray(diffs, dtype=np.float64))
        return {"t_statistic": float(t_stat), "p_value": float(p_value), "significant": p_value < alpha,
                "mean_diff": float(np.mean(scores_a) - np.mean(scores_b)), "std_diff": float(np.std(diffs))}

    @staticmethod
    def bootstrap_confidence_interval(scores_a: List[float], scores_b: List[float], n_bootstrap: int = 10000,
                                      confidence: float = 0.95, seed: int = 42) -> Dict:
        """Interval of the mean difference over ``n_bootstrap`` resamples.  The resamples are the reference's for ``seed``
        (snx.retrieval.bootstrap_indices), their means are formed on the GPU (snx.retrieval.bootstrap_means), the
        percentiles on the host."""
        from snx.retrieval import bootstrap_means
        diffs = np.array(scores_a) - np.array(scores_b)
        means = bootstrap_means(diffs, n_bootstrap=n_bootstrap, seed=seed).cpu().numpy()[:, 0]
        alpha = 1 - confidence
        lower = np.percentile(means, 100 * (alpha / 2))
        upper = np.percentile(means, 100 * (1 - alpha / 2))
        return {"mean_diff": float(np.mean(diffs)), "ci_lower": float(lower), "ci_upper": float(upper),
                "confidence": confidence, "significant": not (lower <= 0 <= upper)}

    @classmethod
    def compare_models(cls, result_a: EvaluationResult, result_b: EvaluationResult, model_a_name: str = "Model A",
                       model_b_name: str = "Model B", metrics: Optional[List[str]] = None) -> "ModelComparison":
        """Default metrics: mrr and ndcg@5 / 10 / 20.  A metric whose scores cannot be compared (ValueError, TypeError)
        is recorded as {"error": ...}; a missing library or GPU is not such a case and raises."""
        comparison = cls(model_a_name=model_a_name, model_b_name=model_b_name)
        if metrics is None:
            metrics = ["mrr"] + [f"ndcg@{k}" for k in (5, 10, 20)]
        rows_a, rows_b = result_a.per_query_metrics, result_b.per_query_metrics
        if len(rows_a) != len(rows_b):
            warnings.warn(f"Different number of queries: {len(rows_a)} vs {len(rows_b)}")
            return comparison
        for metric in metrics:
            try:
                a = [q.get(metric, 0) for q in rows_a]
                b = [q.get(metric, 0) for q in rows_b]
                comparison.metrics_compared[metric] = {
                    "model_a_mean": float(np.mean(a)), "model_b_mean": float(np.mean(b)),
                    "paired_t_test": cls.paired_t_test(a, b), "bootstrap_ci": cls.bootstrap_confidence_interval(a, b)}
            except (ValueError, TypeError) as e:
                comparison.metrics_compared[metric] = {"error": str(e)}
        return comparison

    def summary(self) -> str:
        bar = "=" * 70
        out = [bar, f"Model Comparison: {self.model_a_name} vs {self.model_b_name}", bar]
        for metric, r in self.metrics_compared.items():
            if "error" in r:
                out.append(f"\n{metric}: ERROR - {r['error']}")
                continue
            t, ci = r["paired_t_test"], r["bootstrap_ci"]
            out += [f"\n{metric.upper()}:", f"  {self.model_a_name}: {r['model_a_mean']:.4f}",
                    f"  {self.model_b_name}: {r['model_b_mean']:.4f}", f"  Difference: {t['mean_diff']:.4f}"]
            if t.get("t_statistic") is not None:
                out.append(f"  Paired t-test: t={t['t_statistic']:.3f}, p={t['p_value']:.4f}{'*' if t['significant'] else ''}")
            out.append(f"  95% CI: [{ci['ci_lower']:.4f}, {ci['ci_upper']:.4f}]{'*' if ci['significant'] else ''}")
        out += ["", "* indicates statistically significant difference (p < 0.05)", bar]
        return "\n".join(out)


def create_korean_legal_medical_eval_dataset() -> EvaluationDataset:
    """The reference's sample dataset (15 source terms of the legal, medical and general domains, graded synonyms each).
    Its judgment lists are data: they are kept as the fixture tools/make_golden_expansion.py records
    (tests/golden/g20_expansion/sample_dataset.json) and loaded from there."""
    if not SAMPLE_DATASET.exists():
        raise FileNotFoundError(f"{SAMPLE_DATASET} is missing: the sample dataset ships as that fixture "
                                "(tools/make_golden_expansion.py writes it)")
    return EvaluationDataset.load(SAMPLE_DATASET)
