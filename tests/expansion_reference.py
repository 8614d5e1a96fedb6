"""NumPy / Python restatement of the term-expansion evaluation (include/snx.h "term-expansion evaluation"), the
deterministic case builder of tests/golden/g20_expansion and the stub tokenizer and model that the golden tool
(tools/make_golden_expansion.py) and the tests share.

Three layers, each in plain loops:
  ranking / metrics     the ABI text: which entries are ranked, their order, positions, the counts and the fold
  single_query          the per-query numbers of the reference's RankingMetrics.evaluate_single_query, from the ranking
                        above plus the host rules (token resolution, the two id sets, IDCG, int(1 / mrr))
  build_rows / build_queries, StubTokenizer, StubModel     the g20 inputs
"""
import math

import numpy as np

V = 512
NQ = 40
MAX_K = 100
K_DEFAULT = [5, 10, 20, 50, 100]
K_WIDE = [5, 10, 20, 50, 100, 150]                 # the largest exceeds MAX_K
PAD, CLS, SEP, UNK, MASK = 0, 1, 2, 3, 4
ADDITIONAL_SPECIAL = [5, 6]
SPECIAL_IDS = [PAD, CLS, SEP, UNK, MASK] + ADDITIONAL_SPECIAL
DOMAINS = ["legal", "medical", "general"]
NO_DOMAIN_QUERY = 11
BATCH_SIZE = 25                                    # evaluate(): two batches, 25 and 15 queries


# ------------------------------------------------------------------------------------------------ the ABI text
def gain(g: int, p: int) -> float:
    return (2 ** g - 1) / math.log2(p + 1)


def ranking(row, excluded, max_k: int):
    """Ids of the ranked entries (row > 0 and not excluded) by weight descending, ties lowest id first, cut after max_k."""
    row = np.asarray(row, dtype=np.float32)
    ids = [v for v in range(row.shape[0]) if row[v] > 0 and not excluded[v]]
    ids.sort(key=lambda v: (-float(row[v]), v))
    return ids[:max_k]


def metrics(rep, excluded, j_ptr, j_tok, j_grade, j_rel, max_k: int, cutoffs):
    """-> rank int32 [nj], nranked int32 [B], first int32 [B], hits int32 [B, ncut], dcg float64 [B, ncut]."""
    rep = np.asarray(rep, dtype=np.float32)
    B, width = rep.shape
    ncut = len(cutoffs)
    rank = np.zeros(len(j_tok), np.int32)
    nranked = np.zeros(B, np.int32)
    first = np.zeros(B, np.int32)
    hits = np.zeros((B, ncut), np.int32)
    dcg = np.zeros((B, ncut), np.float64)
    for b in range(B):
        order = ranking(rep[b], excluded, max_k)
        pos = {v: p + 1 for p, v in enumerate(order)}
        nranked[b] = len(order)
        judged = []
        for i in range(int(j_ptr[b]), int(j_ptr[b + 1])):
            t = int(j_tok[i])
            rank[i] = pos.get(t, 0) if 0 <= t < width else 0
            if rank[i]:
                judged.append((int(rank[i]), int(j_grade[i]), bool(j_rel[i])))
        judged.sort()
        rel_pos = [p for p, _, r in judged if r]
        first[b] = rel_pos[0] if rel_pos else 0
        for c, k in enumerate(cutoffs):
            hits[b, c] = sum(1 for p in rel_pos if p <= k)
            acc = 0.0
            for p, g, _ in judged:
                if g > 0 and p <= k:
                    acc = acc + gain(g, p)
            dcg[b, c] = acc
    return rank, nranked, first, hits, dcg


# ------------------------------------------------------------------------------------------------ the per-query numbers
def excluded_mask(special_ids, width: int) -> np.ndarray:
    ex = np.zeros(width, np.uint8)
    for s in special_ids:
        if 0 <= s < width:
            ex[s] = 1
    return ex


def judgment_rows(judgments: dict, resolve):
    """(id, grade, rel) of every resolved id: the grade map in which a later token overwrites an earlier one of the same
    id, and membership in the set of ids of tokens with grade >= 1 -- two different things."""
    grade_of, rel_ids = {}, set()
    for tok, g in judgments.items():
        i = resolve(tok)
        if i is None:
            continue
        grade_of[i] = g
        if g >= 1:
            rel_ids.add(i)
    return [(i, g, i in rel_ids) for i, g in grade_of.items()], rel_ids


def ideal_dcg(judgments: dict, k: int) -> float:
    grades = sorted(judgments.values(), reverse=True)[:k]              # stable; only the grades matter
    acc = 0.0
    for i, g in enumerate(grades):
        if g > 0:
            acc = acc + gain(g, i + 1)
    return acc


def single_query(row, special_ids, resolve, query: dict, k_values, max_k: int) -> dict:
    width = len(row)
    rows, rel_ids = judgment_rows(query["relevance_judgments"], resolve)
    ptr = np.array([0, len(rows)])
    tok = np.array([r[0] for r in rows], np.int64)
    rank, nranked, first, hits, dcg = metrics(np.asarray(row)[None, :], excluded_mask(special_ids, width), ptr, tok,
                                              [r[1] for r in rows], [r[2] for r in rows], max_k, list(k_values))
    out = {"query": query["query"], "domain": query.get("domain"), "num_ranked_tokens": int(nranked[0])}
    for c, k in enumerate(k_values):
        out[f"recall@{k}"] = int(hits[0, c]) / len(rel_ids) if rel_ids else 0.0
    out["mrr"] = 1.0 / int(first[0]) if first[0] else 0.0
    out["first_relevant_rank"] = int(1 / out["mrr"]) if out["mrr"] > 0 else float("inf")
    for c, k in enumerate(k_values):
        idcg = ideal_dcg(query["relevance_judgments"], k)
        out[f"ndcg@{k}"] = float(dcg[0, c]) / idcg if idcg != 0 else 0.0
    return out


# ------------------------------------------------------------------------------------------------ stubs
class StubTokenizer:
    """Words ``w<i>`` and ``a<i>`` (an alias) encode to the single id i, ``q<i>`` (a query text) to i as well, a word
    joined with ``+`` to one id per part; anything else to the unknown id.  Ids may exceed the vocabulary."""
    pad_token_id, cls_token_id, sep_token_id, unk_token_id, mask_token_id = PAD, CLS, SEP, UNK, MASK
    bos_token_id = None
    eos_token_id = None
    additional_special_tokens_ids = list(ADDITIONAL_SPECIAL)

    def encode(self, text, add_special_tokens=False):
        ids = []
        for word in str(text).split():
            for part in word.split("+"):
                ids.append(int(part[1:]) if part[:1] in "waq" and part[1:].isdigit() else UNK)
        return [CLS] + ids + [SEP] if add_special_tokens else ids

    def __call__(self, texts, padding=True, truncation=True, max_length=64, return_tensors="pt"):
        import torch
        rows = [self.encode(t, add_special_tokens=True)[:max_length] for t in texts]
        width = max(len(r) for r in rows)
        ids = torch.full((len(rows), width), PAD, dtype=torch.long)
        mask = torch.zeros((len(rows), width), dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r, dtype=torch.long)
            mask[i, :len(r)] = 1
        return {"input_ids": ids, "attention_mask": mask}


def stub_model(rows):
    """A module whose forward returns (rows[i], None) for the query text ``q<i>`` (its id sits behind the CLS token)."""
    import torch

    class StubModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))
            self.register_buffer("rows", torch.as_tensor(np.asarray(rows, dtype=np.float32)))

        def forward(self, input_ids, attention_mask):
            return self.rows[input_ids[:, 1]], None

    return StubModel()


def resolver(tokenizer):
    def resolve(token):
        ids = tokenizer.encode(token, add_special_tokens=False)
        return ids[0] if len(ids) == 1 else None
    return resolve


# ------------------------------------------------------------------------------------------------ the g20 inputs
def build_rows(variant: int = 0) -> np.ndarray:
    """rows fp32 [NQ, V]: the positive weights of a row are distinct multiples of 1/8 (no ties), the rest 0 or negative.
    ``variant`` 1 is the second checkpoint of the comparison: the same generator from other seeds."""
    rows = np.zeros((NQ, V), np.float32)
    for i in range(NQ):
        rng = np.random.default_rng(1000 * (variant + 1) + i)
        npos = 30 if i == 6 else 0 if i == 7 else int(rng.integers(130, 300))
        vals = (rng.permutation(V) + 1).astype(np.float32) / np.float32(8)
        chosen = rng.choice(V, size=npos, replace=False)
        rows[i, chosen] = vals[chosen]
        rest = np.setdiff1d(np.arange(V), chosen)
        neg = rng.choice(rest, size=min(20, len(rest)), replace=False)
        rows[i, neg] = -vals[neg]
        if i != 7:
            rows[i, ADDITIONAL_SPECIAL[0]] = 80.0                     # a special id at the very top: masking matters
    return rows


def build_queries(rows) -> list:
    """The judgments, placed by the ranking of ``rows`` (variant 0).  Dict order is part of the cases."""
    ex = excluded_mask(SPECIAL_IDS, V)
    out = []
    for i in range(NQ):
        rng = np.random.default_rng(77 + i)
        order = ranking(rows[i], ex, V)
        zero = [v for v in range(7, V) if rows[i, v] == 0]
        at = lambda p: f"w{order[p - 1]}"                              # noqa: E731  the token at position p
        if i == 0:
            j = {}
        elif i == 1:
            j = {f"w{order[0]}+w{order[1]}": 3, "w9+w10": 2, "zzz yyy": 1}
        elif i == 2:
            j = {f"w{ADDITIONAL_SPECIAL[0]}": 3, at(4): 2, at(30): 1}
        elif i == 3:
            j = {at(2): 3, f"a{order[1]}": 0, at(12): 2}
        elif i == 4:
            j = {f"a{order[1]}": 0, at(2): 3, at(12): 2}
        elif i == 5:
            j = {f"w{zero[0]}": 3, f"w{zero[1]}": 1, at(7): 1}
        elif i == 6:
            j = {at(1): 1, at(len(order) - 1): 3, at(len(order)): 2, f"w{zero[0]}": 3}
        elif i == 7:
            j = {"w20": 3, "w21": 2}
        elif i == 8:
            j = {at(3): 0, at(93): 2, at(110): 3, at(101): 3}
        elif i == 9:
            j = {at(99): 3, at(100): 1, at(102): 2, f"w{order[9]}+w{order[10]}": 3}
        elif i == 10:
            j = {f"w{V + 88}": 2, at(5): 3, at(60): 1}
        else:
            j = {}
            n = int(rng.integers(3, 12))
            for p in sorted(set(int(x) for x in rng.integers(1, min(len(order), 160) + 1, size=n))):
                j[at(p)] = int(rng.integers(0, 4))
            j[f"w{zero[int(rng.integers(0, len(zero)))]}"] = int(rng.integers(1, 4))
            if i % 4 == 0:
                j[f"w{order[0]}+w{order[2]}"] = 3
            if i % 5 == 0:
                j = dict(reversed(list(j.items())))
        out.append({"query": f"q{i}", "relevance_judgments": j,
                    "domain": None if i == NO_DOMAIN_QUERY else DOMAINS[i % 3]})
    return out


def grid_case(rng, B: int, width: int, counts, top: int = 4):
    """Small-integer rows (ties abound) with NaN, -0.0 and negatives, an exclusion mask, and judgments of ``counts[b]``
    distinct ids per row, a few of them outside [0, width)."""
    rep = rng.integers(-1, top + 1, size=(B, width)).astype(np.float32)
    rep[rep == -1] = np.float32(-0.0) if width % 2 else np.float32(-1.5)
    if width > 2:
        rep[rng.integers(0, B), rng.integers(0, width)] = np.nan
    ex = (rng.random(width) < 0.1).astype(np.uint8)
    ptr, tok, grade, rel = [0], [], [], []
    for b in range(B):
        n = int(counts[b % len(counts)])
        pool = np.concatenate([np.arange(width), [-3, -1, width, width + 5, 2 ** 31 - 1]])
        ids = rng.permutation(pool)[:n] if n <= len(pool) else pool
        tok.extend(int(x) for x in ids)
        grade.extend(int(x) for x in rng.integers(0, 4, size=len(ids)))
        rel.extend(int(x) for x in rng.integers(0, 2, size=len(ids)))
        ptr.append(len(tok))
    return rep, ex, np.array(ptr, np.int64), np.array(tok, np.int64), np.array(grade, np.int64), np.array(rel, np.int64)
