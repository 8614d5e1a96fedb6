"""The contract of include/snx.h "Character n-gram TF-IDF" restated in plain Python and numpy, for the tests: the
``char_wb`` analyzer, the exact n-gram key, the fit with the project's tie rule at the ``max_features`` cut, the
sublinear tf-idf rows in float64 rounded to fp32 once, and the index's score and order (fp32 multiply-add over the shared
features ascending; score descending, ties lowest doc id, only scores > 0).  ``NumpyTfidfIndex`` is the stand-in on which
the miner's host logic runs without a GPU."""
from collections import Counter
from typing import List, Optional, Sequence

import numpy as np


def analyze(text: str, ngram_range=(2, 3)) -> List[str]:
    """The n-grams of a text, with repeats, as the contract lists them."""
    lo, hi = ngram_range
    out = []
    for w in text.lower().split():
        w = " " + w + " "
        L = len(w)
        for n in range(lo, hi + 1):
            if L <= n:
                out.append(w)
                break
            out.extend(w[i:i + n] for i in range(L - n + 1))
    return out


def ngram_key(g: str) -> int:
    return sum((ord(c) + 1) << s for c, s in zip(g, (42, 21, 0)))


def key_ngram(k: int) -> str:
    return "".join(chr(c - 1) for c in ((k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF) if c)


def row_counts(text: str, ngram_range=(2, 3)):
    """(keys int64 ascending, counts int32) of one text."""
    c = Counter(ngram_key(g) for g in analyze(text, ngram_range))
    keys = sorted(c)
    return np.array(keys, dtype=np.int64), np.array([c[k] for k in keys], dtype=np.int32)


def fit(texts: Sequence[str], ngram_range=(2, 3), max_features: Optional[int] = 30000) -> dict:
    total, df = Counter(), Counter()
    for t in texts:
        keys, counts = row_counts(t, ngram_range)
        for k, c in zip(keys.tolist(), counts.tolist()):
            total[k] += c
            df[k] += 1
    keys = sorted(total)
    if max_features is not None and max_features < len(keys):
        keys = sorted(sorted(keys, key=lambda k: (-total[k], k))[:max_features])     # ties at the cut: lowest key
    dfa = np.array([df[k] for k in keys], dtype=np.int32)
    idf = np.log((1.0 + np.float64(len(texts))) / (1.0 + dfa.astype(np.float64))) + 1.0
    return {"keys": np.array(keys, dtype=np.int64), "total": np.array([total[k] for k in keys], dtype=np.int64),
            "doc_freq": dfa, "idf": idf, "n_docs": len(texts), "distinct": len(total)}


def transform_row(text: str, model: dict, ngram_range=(2, 3), sublinear_tf: bool = True):
    """(feature ids int32 ascending, weights float64 of unit norm) of one text; unknown n-grams dropped."""
    keys, counts = row_counts(text, ngram_range)
    pos = np.searchsorted(model["keys"], keys)
    ok = (pos < model["keys"].size)
    ok[ok] &= model["keys"][pos[ok]] == keys[ok]
    fid, c = pos[ok].astype(np.int32), counts[ok].astype(np.float64)
    u = (np.log(c) + 1.0 if sublinear_tf else c) * model["idf"][fid]
    return fid, (u / np.sqrt(np.sum(u * u)) if fid.size else u)


def transform(texts: Sequence[str], model: dict, ngram_range=(2, 3), sublinear_tf: bool = True):
    return [transform_row(t, model, ngram_range, sublinear_tf) for t in texts]


def dense32(rows, F: int) -> np.ndarray:
    m = np.zeros((len(rows), max(F, 1)), dtype=np.float32)
    for i, (fid, w) in enumerate(rows):
        m[i, fid] = w.astype(np.float32)
    return m


def scores32(q32: np.ndarray, d32: np.ndarray) -> np.ndarray:
    """s(q, d) [nq, nd] fp32: acc = fp32(q_f * d_f + acc) over the features ascending (the product of two fp32 is exact in
    float64; the sum is rounded to float64 and then to fp32, which differs from one fmaf rounding only in rare double
    rounding cases -- the tests compare scores within a tolerance, not bit for bit)."""
    acc = np.zeros((q32.shape[0], d32.shape[0]), dtype=np.float32)
    for f in np.flatnonzero(q32.any(0) & d32.any(0)):
        acc = (q32[:, f].astype(np.float64)[:, None] * d32[:, f].astype(np.float64)[None, :]
               + acc.astype(np.float64)).astype(np.float32)
    return acc


def top_k(scores: np.ndarray, k: int):
    """(scores [nq, k] fp32, docs [nq, k] int32): score descending, ties lowest doc id, only > 0; unused 0 / -1."""
    nq, nd = scores.shape
    out_s = np.zeros((nq, k), dtype=np.float32)
    out_d = np.full((nq, k), -1, dtype=np.int32)
    for q in range(nq):
        order = np.lexsort((np.arange(nd), -scores[q].astype(np.float64)))
        order = [d for d in order if scores[q, d] > 0][:k]
        out_s[q, :len(order)] = scores[q, order]
        out_d[q, :len(order)] = order
    return out_s, out_d


class NumpyTfidfIndex:
    """The host stand-in of snx.retrieval.TfidfIndex: fit_add / build / search_texts with numpy results."""

    def __init__(self, ngram_range=(2, 3), max_features: Optional[int] = 30000, sublinear_tf: bool = True):
        self.ngram_range, self.max_features, self.sublinear_tf = tuple(ngram_range), max_features, sublinear_tf
        self.texts: List[str] = []
        self.model = None

    def fit_add(self, texts):
        self.texts.extend(texts)
        self.model = None

    def build(self):
        self.model = fit(self.texts, self.ngram_range, self.max_features)
        self.rows = transform(self.texts, self.model, self.ngram_range, self.sublinear_tf)
        self.d32 = dense32(self.rows, self.model["keys"].size)
        return self

    @property
    def num_docs(self):
        return len(self.texts)

    def search_texts(self, texts, k, targets=None):
        q = dense32(transform(texts, self.model, self.ngram_range, self.sublinear_tf), self.model["keys"].size)
        s, d = top_k(scores32(q, self.d32), k)
        return s, d, None, None


# ------------------------------------------------------------------------------------------------ the g17 fixture
def cli_flags_of(path: str) -> dict:
    """{'--flag': {'type', 'default', 'action'}} of every add_argument(...) in a module's parse_args(), read as TEXT through
    ``ast`` (type and default as source, so that Path('x') and 50_000 compare by meaning)."""
    import ast
    with open(path, encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "parse_args")
    out = {}
    for node in ast.walk(fn):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            out[ast.literal_eval(node.args[-1])] = {key: ast.unparse(kw[key]) if key in kw else None
                                                    for key in ("type", "default", "action")}
    return out


def load_g17(folder: str) -> dict:
    import json
    import os
    with open(os.path.join(folder, "meta.json"), encoding="utf-8") as f:
        g = json.load(f)
    g["arrays"] = dict(np.load(os.path.join(folder, "arrays.npz")))
    g["folder"] = folder
    g["input_files"] = [os.path.join(folder, "input", n) for n in g["shards"]]
    g["expected_lines"] = []
    for n in g["shards"]:
        with open(os.path.join(folder, "expected", n), encoding="utf-8") as f:
            g["expected_lines"].append(f.read().split("\n")[:-1])
    g["expected"] = [[json.loads(line) for line in lines] for lines in g["expected_lines"]]
    corpus, seen = [], set()                                  # the unique positives in file order, up to the cap
    for recs in g["expected"]:
        for rec in recs:
            p = rec.get("positive", "")
            if p and p not in seen and len(corpus) < g["max_corpus"]:
                seen.add(p)
                corpus.append(p)
    g["corpus"] = corpus
    return g


def mining_tolerance(nnz_q: int) -> float:
    """(nnz_q + 2) * 2^-24: an fp32 multiply-add chain over nnz_q products of unit vectors, plus the two weight roundings."""
    return (int(nnz_q) + 2) * 2.0 ** -24


def check_mining_output(g: dict, out_dir: str, stats: Sequence[dict]) -> dict:
    """The four conditions on a mining output over the g17 shards (host stand-in and GPU alike); -> counts."""
    import json
    import os
    scores, nnz_q, corpus = g["arrays"]["scores"], g["arrays"]["nnz_q"], g["corpus"]
    doc_of = {t: i for i, t in enumerate(corpus)}
    ours_lines = []
    for n in g["shards"]:
        with open(os.path.join(out_dir, n), encoding="utf-8") as f:
            ours_lines.append(f.read().split("\n")[:-1])
    need = {(s, i): r for r, (s, i) in enumerate(g["need"])}
    n_close = n_zero = 0
    failed = [0] * len(g["shards"])
    for s, lines in enumerate(ours_lines):
        assert len(lines) == len(g["expected_lines"][s])
        for i, line in enumerate(lines):
            if (s, i) not in need:                            # 4: had a negative: byte for byte
                assert line == g["expected_lines"][s][i], (s, i)
                continue
            r, rec, ref = need[(s, i)], json.loads(line), g["expected"][s][i]
            positive = rec.get("positive", "")
            adm = np.array([t != positive for t in corpus])
            top = np.sort(scores[r][adm])[::-1]
            best, second, tol = float(top[0]), float(top[1]), mining_tolerance(nnz_q[r])
            if best <= 0.0:                                   # 3: nothing shares an n-gram with the query
                assert not rec.get("negative"), (s, i, rec)
                n_zero += 1
                failed[s] += 1
                continue
            assert bool(rec.get("negative")) == bool(ref.get("negative")), (s, i)
            assert rec["negative"] != positive and rec["difficulty"] == "hard", (s, i)       # 1
            got = float(scores[r][doc_of[rec["negative"]]])
            assert got >= best - tol, (s, i, got, best, tol)
            if best - second > tol:                           # 2
                assert rec["negative"] == ref["negative"], (s, i)
            else:
                n_close += 1
            rest = {k: v for k, v in rec.items() if k not in ("negative", "difficulty")}
            assert rest == {k: v for k, v in ref.items() if k not in ("negative", "difficulty")}, (s, i)
    assert n_close <= 0.05 * len(g["need"])
    for s, (st, ref) in enumerate(zip(stats, g["stats"])):
        assert st["total"] == ref["total"] and st["already_had_negative"] == ref["already_had_negative"], (st, ref)
        assert st["failed"] == failed[s] and st["added"] + st["failed"] == ref["added"] + ref["failed"], (st, ref)
    return {"close": n_close, "zero": n_zero}
