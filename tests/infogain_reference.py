"""Plain numpy restatement of the information-gain contract (include/snx.h "exact L2 nearest neighbours" and the five rules
of src/information_gain.py), for the tests.  It imports nothing from the package.

Distances here are the reference's own: float64, difference form, one multiply and one add per step (``d2_plain``), which
is what scipy's cdist computes; with them the three fp32 arrays equal the goldens bit for bit.  ``d2_fma`` restates the
device's chain exactly -- one rounding per step -- with rationals, for tiny shapes."""
import math
from fractions import Fraction

import numpy as np

EULER_GAMMA = 0.5772156649             # the estimator's ten-digit constant
EPS = 1e-10


def normalize_rows(x: np.ndarray) -> np.ndarray:
    """Rule 1: x / (norm(x, axis=1, keepdims=True) + 1e-10) in fp32 numpy."""
    return x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-10)


def d2_plain(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """float64 [m, n]: acc = acc + t * t for j ascending from 0, t = (double)a[i, j] - (double)b[r, j]."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    for j in range(a.shape[1]):
        t = a64[:, j, None] - b64[None, :, j]
        acc = acc + t * t
    return acc


def fma(x: float, y: float, z: float) -> float:
    """fma(x, y, z) rounded once: the exact rational value, then Python's correctly rounded int / int division."""
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def d2_fma(q: np.ndarray, c: np.ndarray) -> float:
    """The ABI's chain for one pair of fp32 rows."""
    acc = 0.0
    for x, y in zip(q.tolist(), c.tolist()):               # fp32 -> Python float is exact
        t = float(np.float64(x) - np.float64(y))
        acc = fma(t, t, acc)
    return acc


def knn_order(d2_row: np.ndarray) -> np.ndarray:
    """Corpus ids under (d2 ascending, id ascending)."""
    return np.lexsort((np.arange(d2_row.shape[0]), d2_row))


def digamma_int(k: int) -> float:
    """psi(k), integer k >= 1: -gamma + sum_{i<k} 1/i."""
    return math.fsum([-0.5772156649015329] + [1.0 / i for i in range(1, k)])


def log_volume_unit_ball(d: int) -> float:
    return (d / 2) * float(np.log(np.pi)) - math.lgamma(d / 2 + 1)


def kl_entropy(rho, d: int, n_ref: int, k: int):
    rho = np.maximum(np.asarray(rho, dtype=np.float64), EPS)
    return d * np.log(rho) + np.log(n_ref) + log_volume_unit_ball(d) + EULER_GAMMA - digamma_int(k)


def information_gain(sources, targets, corpus, k_entropy=10, k_neighborhood=50, normalize=True, d2=d2_plain):
    """Rules 1-5 -> (ig, h_target, h_conditional), fp32 [m]."""
    src, tgt, cor = (np.asarray(x, dtype=np.float32) for x in (sources, targets, corpus))
    if normalize:
        src, tgt, cor = normalize_rows(src), normalize_rows(tgt), normalize_rows(cor)
    m, (n, d) = src.shape[0], cor.shape
    h_t = np.zeros(m, dtype=np.float32)
    h_c = np.zeros(m, dtype=np.float32)
    k1 = min(k_entropy, n - 1)                                           # rule 2
    if k1 >= 1:
        dist = np.sqrt(np.sort(d2(tgt, cor), axis=1))
        h_t = kl_entropy(dist[:, min(k1, n - 1)], d, n, k1).astype(np.float32)
    K = min(k_neighborhood, n)                                           # rule 3
    k2 = min(min(k_entropy, k_neighborhood - 1), K - 1)                  # rule 4
    if k2 >= 1:
        ds = d2(src, cor)
        for i in range(m):
            nb = knn_order(ds[i])[:K]
            dist = np.sqrt(np.sort(d2(tgt[i:i + 1], cor[nb])[0]))
            rho = dist[k2] if dist[0] < EPS else dist[k2 - 1]
            h_c[i] = kl_entropy(rho, d, K, k2)
    return h_t - h_c, h_t, h_c                                           # rule 5


# ------------------------------------------------------------------------------------------------ the golden cases' inputs
def synth(shape, seed: int) -> np.ndarray:
    """Deterministic fp32 values in [-1, 1): splitmix64 of the element index, the top 24 bits.  The golden cases are built
    from it, so the fixture stores what the reference answered and not what it was asked."""
    size = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(size, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) / 2.0 ** 23 - 1.0).astype(np.float32).reshape(shape)


def build_case(spec):
    """(corpus [n, D], sources [m, D], targets [m, D], rows) of a golden case.  ``rows[i]`` = (a, b): the corpus rows behind
    pair i's source and target, -1 where the vector is not a corpus row.  Pair kinds, cycled: ``corpus`` (both are corpus
    rows), ``fresh_target`` (a target outside the corpus), ``near`` (the target a small step from its source),
    ``fresh_source`` (a source outside the corpus), ``dup`` (a source next to corpus row 1, whose exact duplicate sits at
    row n // 2: a tie in the interior of the neighbourhood)."""
    n, D, m, seed = spec["n"], spec["D"], spec["m"], spec["seed"]
    corpus = synth((n, D), seed)
    if "dup" in spec["kinds"]:
        assert n >= 4
        corpus[n // 2] = corpus[1]
    fresh, noise = synth((2 * m, D), seed + 1000), synth((m, D), seed + 2000)
    src, tgt, rows = np.empty((m, D), np.float32), np.empty((m, D), np.float32), []
    for i in range(m):
        kind = spec["kinds"][i % len(spec["kinds"])]
        a, b = (7 * i + 1) % n, (11 * i + 3) % n
        if kind == "corpus":
            src[i], tgt[i] = corpus[a], corpus[b]
        elif kind == "fresh_target":
            src[i], tgt[i], b = corpus[a], fresh[i], -1
        elif kind == "near":
            src[i], tgt[i], b = corpus[a], corpus[a] + np.float32(2.0 ** -10) * noise[i], -1
        elif kind == "fresh_source":
            src[i], tgt[i], a = fresh[m + i], corpus[b], -1
        elif kind == "dup":
            src[i], tgt[i], a = corpus[1] + np.float32(2.0 ** -8) * noise[i], corpus[b], -1
        else:
            raise ValueError(kind)
        rows.append((a, b))
    return corpus, src, tgt, rows


def load_g19(path):
    """tests/golden/g19_infogain -> the JSON dict with ``arrays`` (the npz as a dict) added."""
    import json
    import os
    with open(os.path.join(path, "g19.json"), encoding="utf-8") as f:
        g = json.load(f)
    with np.load(os.path.join(path, "arrays.npz")) as z:
        g["arrays"] = {k: z[k] for k in z.files}
    return g
