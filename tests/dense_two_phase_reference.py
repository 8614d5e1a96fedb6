"""Plain numpy restatement of the "two-phase dense retrieval" section of include/snx.h: the tests' reference for
csrc/dense_two_phase.hip.

bf16 rounding is round to nearest even on the fp32 bits; the three norms are float64 left folds over ascending j (every
square is exact in float64); the exact score is tests/dense_reference.py's chain; the candidates are the k1 best of a
GIVEN approximate score matrix (the hardware's accumulation order inside v_mfma_f32_32x32x16_bf16 is not restated: the
certificate has to hold for any order, and the host tests simulate several); the certificate is the header's."""
import math

import numpy as np

from tests import dense_reference as DR

K_MAX = 1024


def dp(D: int) -> int:
    return (D + 31) // 32 * 32


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 (finite) -> bf16 bits uint16, round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def prepare(X: np.ndarray):
    """[n, D] fp32 -> (bits [n, Dp] uint16, norm2, hat2, res2 float64 [n])."""
    X = np.ascontiguousarray(X, np.float32)
    n, D = X.shape
    bits = np.zeros((n, dp(D)), np.uint16)
    bits[:, :D] = bf16_bits(X)
    x, xh = X.astype(np.float64), bf16_value(bits[:, :D]).astype(np.float64)
    sums = np.zeros((3, n), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(D):
            e = x[:, j] - xh[:, j]
            sums[0] += x[:, j] * x[:, j]
            sums[1] += xh[:, j] * xh[:, j]
            sums[2] += e * e
    return bits, sums[0], sums[1], sums[2]


def doc_maxima(norm2, hat2, res2):
    """(N, Nhat, R): the maxima over the docs of the square roots; no doc: zeros."""
    return tuple(float(np.sqrt(v.max())) if v.size else 0.0 for v in (norm2, hat2, res2))


def epsilon(D: int, q_norm2: float, q_hat2: float, q_res2: float, N: float, Nh: float, R: float) -> float:
    """The header's eps: s(q, d) <= a(q, d) + eps for every doc d."""
    n_q, nh_q, r_q = math.sqrt(q_norm2), math.sqrt(q_hat2), math.sqrt(q_res2)
    m23, m24 = 2 * dp(D) * 2.0 ** -23, D * 2.0 ** -24
    g23, g24 = m23 / (1.0 - m23), m24 / (1.0 - m24)
    eps = n_q * R + r_q * Nh + g23 * nh_q * Nh + g24 * n_q * N
    return eps * (1.0 + 2.0 ** -20) + D * 2.0 ** -100 * (1.0 + nh_q + Nh)


def approx_scores(Qh: np.ndarray, Eh: np.ndarray, order: str = "ascending") -> np.ndarray:
    """A simulated phase-1 matrix: the exact fp32 products of the bf16 values, accumulated in fp32 in the given order
    ("ascending" and "descending" in j, or "pairwise": a balanced tree), then + 0.0."""
    Qh, Eh = np.asarray(Qh, np.float32), np.asarray(Eh, np.float32)
    P = Qh[:, None, :] * Eh[None, :, :]                       # 8-bit significands: every product is exact in fp32
    D = P.shape[2]
    if order == "pairwise":
        while P.shape[2] > 1:
            if P.shape[2] % 2:
                P = np.concatenate([P, np.zeros(P.shape[:2] + (1,), np.float32)], 2)
            P = P[:, :, 0::2] + P[:, :, 1::2]
        acc = P[:, :, 0]
    else:
        acc = np.zeros(P.shape[:2], np.float32)
        for j in (range(D) if order == "ascending" else range(D - 1, -1, -1)):
            acc = acc + P[:, :, j]
    return acc.astype(np.float32) + np.float32(0.0)


def candidates(A: np.ndarray, k1: int):
    """-> (cand_doc [nq, k1] int32, cand_approx [nq, k1] fp32): approximate score descending, ties lowest doc first."""
    approx, docs, _, _ = DR.search(A, k1)
    return docs, approx


def rescore(S: np.ndarray, cand_doc: np.ndarray, cand_approx: np.ndarray, eps, lo: int, hi: int, exclude=None,
            ceiling=None):
    """Phase 2 over the exact score matrix ``S`` [nq, nd] -> (scores, docs, found, certified bool [nq]).  ``eps`` [nq]:
    the bound of each query (non-finite: never certified)."""
    nq, nd = S.shape
    k1 = cand_doc.shape[1]
    assert 0 <= lo < hi <= k1
    w = hi - lo
    scores, docs = np.zeros((nq, w), np.float32), np.full((nq, w), -1, np.int32)
    found, cert = np.zeros(nq, np.int32), np.zeros(nq, bool)
    for q in range(nq):
        c = cand_doc[q][cand_doc[q] >= 0].astype(np.int64)
        ok = np.ones(len(c), bool)
        if exclude is not None and len(exclude[q]):
            ok &= ~np.isin(c, np.asarray(list(exclude[q]), np.int64))
        if ceiling is not None:
            with np.errstate(invalid="ignore"):
                ok &= S[q, c] < np.float32(ceiling[q])
        adm = c[ok]
        order = adm[np.lexsort((adm, -S[q, adm].astype(np.float64)))]
        band = order[lo:hi]
        found[q] = len(band)
        docs[q, :len(band)] = band
        scores[q, :len(band)] = S[q, band]
        finite = np.isfinite(S[q, c]).all() and np.isfinite(cand_approx[q][:len(c)]).all() and np.isfinite(eps[q])
        if not finite:
            cert[q] = False
        elif nd <= k1:
            cert[q] = True
        else:
            cert[q] = len(order) >= hi and float(S[q, order[hi - 1]]) > float(cand_approx[q, k1 - 1]) + float(eps[q])
    return scores, docs, found, cert


def query_eps(Q: np.ndarray, E: np.ndarray) -> np.ndarray:
    """eps of every query row against the docs E; +inf (never certified) for a query with a non-finite norm or with
    n_q N or nhat_q Nhat above 2^127."""
    _, qn, qh, qr = prepare(Q)
    N, Nh, R = doc_maxima(*prepare(E)[1:])
    def in_range(i):                                          # no product or partial sum of either pass can overflow fp32
        return np.isfinite([qn[i], qh[i], qr[i]]).all() and math.sqrt(qn[i]) * N <= 2.0 ** 127 and \
            math.sqrt(qh[i]) * Nh <= 2.0 ** 127
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array([epsilon(Q.shape[1], qn[i], qh[i], qr[i], N, Nh, R) if in_range(i) else np.inf
                         for i in range(Q.shape[0])], np.float64)


def search_k1(nd: int, k: int, expansion: float) -> int:
    return max(k, min(nd, K_MAX, math.ceil(k * expansion)))


def band_k1(nd: int, hi: int, longest: int, expansion: float) -> int:
    return max(hi, min(nd, K_MAX, math.ceil((hi + longest) * expansion)))


def band_two_phase(Q, E, lo, hi, k1, exclude=None, ceiling=None, exact=False, order="ascending", S=None):
    """The whole search on the host -> (scores, docs, found, certified); ``S``: the exact chain matrix, if at hand."""
    Q, E = np.asarray(Q, np.float32), np.asarray(E, np.float32)
    S = DR.chain_scores(Q, E) if S is None else S
    D = Q.shape[1]
    A = approx_scores(bf16_value(prepare(Q)[0][:, :D]), bf16_value(prepare(E)[0][:, :D]), order)
    cd, ca = candidates(A, k1)
    scores, docs, found, cert = rescore(S, cd, ca, query_eps(Q, E), lo, hi, exclude, ceiling)
    if exact:
        s2, d2, f2 = DR.search_band(S, lo, hi, exclude, ceiling)
        scores[~cert], docs[~cert], found[~cert] = s2[~cert], d2[~cert], f2[~cert]
    return scores, docs, found, cert


# ---------------------------------------------------------------------------------------------------------------- fixtures
def grid_fixture(nd: int, D: int, nq: int, k: int, seed: int):
    """Operands on the grid of multiples of 1/8 in [-1, 1] (exact in bf16; every product is a multiple of 1/64 and every
    partial sum is exact in fp32 in any order) with a planted top k: dims 0 and 1 of every query are 1; the k planted docs
    (at random ids) hold (1, 1) there and every other doc (-1, -1); all other entries are in {-1/8, 0, 1/8}.  A planted
    doc scores at least 2 - (D - 2) / 64 and any other at most -2 + (D - 2) / 64, so for D <= 100 the k-th score lies more
    than 0.9 above every later one -- far above eps, which is below 0.01 here -- and every row is certified whenever
    k1 > k.  Ties among the other docs are frequent.  -> (Q [nq, D], E [nd, D]) fp32."""
    assert 3 <= D <= 100 and k < nd
    rng = np.random.RandomState(seed)
    Q = rng.randint(-1, 2, size=(nq, D)).astype(np.float32) / 8
    E = rng.randint(-1, 2, size=(nd, D)).astype(np.float32) / 8
    Q[:, :2] = 1.0
    E[:, :2] = -1.0
    E[rng.permutation(nd)[:k], :2] = 1.0
    return Q, E


def adversarial_fixture(nd: int = 200, D: int = 32, seed: int = 5):
    """One query against 64 docs that share one bf16 image (all ones) and differ below bf16 precision: twin i holds
    1 + i 2^-16 in dim 0, so a = 32 for all of them and s = 32 + i 2^-16 exactly.  The twins sit at ascending ids, the
    best ones last, so a phase 1 that keeps fewer than 64 keeps the WRONG ones; every other doc scores below 9.
    -> (Q [1, D], E [nd, D], twin ids [64])."""
    rng = np.random.RandomState(seed)
    E = (rng.randint(-2, 3, size=(nd, D)).astype(np.float32) / 8)
    ids = np.sort(rng.permutation(nd)[:64])
    E[ids] = 1.0
    E[ids, 0] = (1.0 + np.arange(64) * 2.0 ** -16).astype(np.float32)
    return np.ones((1, D), np.float32), E, ids
