"""Exact L2 nearest neighbours and the information-gain scores of synonym pairs on the GPU (csrc/infogain.hip,
include/snx.h "exact L2 nearest neighbours"): the distance work of the reference's second synonym filter
(ref:src/information_gain.py:156-195, 291-372), a float64 cdist against the whole corpus and one argsort per pair there.

``L2Index`` holds the corpus on the device.  ``information_gain`` turns (source, target) embedding pairs into the three
fp32 arrays of ``compute_information_gain_batch``: two searches and one gather per batch of pairs on the device, then the
Kozachenko-Leonenko formula in float64 numpy over one value per pair.  Normalisation is the caller's (src.information_gain
does it on the host with numpy, as the reference writes it)."""
import math
from typing import Tuple

import numpy as np
import torch

from ._abi import CONSTANTS
from ._lib import call
from .ops import _p, _stream
from .retrieval._common import cuda_device, slices, step_bytes_mean, workspace

K_MAX = CONSTANTS["SNX_L2_KMAX"]
DIM_MAX = 4096
EULER_GAMMA = 0.5772156649             # the reference's constant in the estimator, ten digits (ref:information_gain.py:149)
EPS = 1e-10                            # a distance below it means "the query is in the reference set"
_WS_BUDGET = 1 << 30                   # bytes of search workspace per launch
_EULER = 0.5772156649015329            # Euler-Mascheroni to float64, for psi


# ------------------------------------------------------------------------------------------------ the estimator's constants
def digamma_int(k: int) -> float:
    """psi(k) at an integer k >= 1: -gamma + sum_{i<k} 1/i, summed exactly and rounded once."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
        raise ValueError("digamma_int: k must be an int >= 1")
    return math.fsum([-_EULER] + [1.0 / i for i in range(1, int(k))])


# Stirling's tail for x >= 13 and the rational for [2, 3) of the Cephes library's lgam (Moshier; netlib cephes/cprob/gamma.c)
_LG_A = (8.11614167470508450300e-4, -5.95061904284301438324e-4, 7.93650340457716943945e-4, -2.77777777730099687205e-3,
         8.33333333333331927722e-2)
_LG_B = (-1.37825152569120859100e3, -3.88016315134637840924e4, -3.31612992738871184744e5, -1.16237097492762307383e6,
         -1.72173700820839662146e6, -8.53555664245765465627e5)
_LG_C = (-3.51815701436523470549e2, -1.70642106651881159223e4, -2.20528590553854454839e5, -1.13933444367982507207e6,
         -2.53252307177582951285e6, -2.01889141433532773231e6)
_LS2PI = 0.91893853320467274178        # ln sqrt(2 pi)


def _horner(x: float, coef, monic: bool = False) -> float:
    r = x + coef[0] if monic else coef[0]
    for c in coef[1:]:
        r = r * x + c
    return r


def log_gamma(x: float) -> float:
    """ln Gamma(x) for x >= 1 in the Cephes form that scipy's gammaln evaluates: at every x = d / 2 + 1, d in [1, 4096], the
    bits are gammaln's (tools/make_golden_infogain.py records them), so ln V_d is the reference's number.  math.lgamma is
    not: the two differ by up to 12 ulps at half-integers, and ln V_d, a difference, by up to 8."""
    x = float(x)
    if not x >= 1.0:
        raise ValueError("log_gamma: x must be >= 1")
    if x < 13.0:
        z, p, u = 1.0, 0.0, x
        while u >= 3.0:                                      # down to [2, 3), the product of the steps in z
            p -= 1.0
            u = x + p
            z *= u
        while u < 2.0:
            z /= u
            p += 1.0
            u = x + p
        if u == 2.0:
            return math.log(z)
        u = x + (p - 2.0)
        return math.log(z) + u * _horner(u, _LG_B) / _horner(u, _LG_C, monic=True)
    q = (x - 0.5) * math.log(x) - x + _LS2PI
    if x > 1.0e8:
        return q
    p = 1.0 / (x * x)
    if x >= 1000.0:
        return q + ((7.9365079365079365079365e-4 * p - 2.7777777777777777777778e-3) * p + 0.0833333333333333333333) / x
    return q + _horner(p, _LG_A) / x


def log_volume_unit_ball(d: int) -> float:
    """ln V_d = (d / 2) ln(pi) - ln Gamma(d / 2 + 1) (ref:information_gain.py:84-97)."""
    return (d / 2) * float(np.log(np.pi)) - log_gamma(d / 2 + 1)


def kl_entropy(rho, d: int, n_ref: int, k: int):
    """The Kozachenko-Leonenko value of one point (ref:information_gain.py:144-151) in float64, the terms added in the
    reference's order; ``rho`` float64 (any shape) is clamped at EPS first."""
    rho = np.maximum(np.asarray(rho, dtype=np.float64), EPS)
    return d * np.log(rho) + np.log(n_ref) + log_volume_unit_ball(d) + EULER_GAMMA - digamma_int(k)


# ------------------------------------------------------------------------------------------------ validation (no GPU)
def check_k(k, who: str, name: str = "k") -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= K_MAX:
        raise ValueError(f"{who}: {name} must be an int in [1, {K_MAX}]")
    return int(k)


def check_rows(x, who: str, name: str, dim=None) -> np.ndarray:
    """``x`` -> fp32 C-contiguous numpy [m, D] with 1 <= D <= 4096 and every value finite."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.ndim != 2 or x.dtype != np.float32:
        raise ValueError(f"{who}: {name} must be fp32 [m, D]")
    if not 1 <= x.shape[1] <= DIM_MAX:
        raise ValueError(f"{who}: {name} must have 1 <= D <= {DIM_MAX} columns")
    if dim is not None and x.shape[1] != dim:
        raise ValueError(f"{who}: {name} must be fp32 [m, {dim}]")
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: {name} has at most 2^31 - 1 rows")
    if x.size and not bool(np.isfinite(x).all()):
        raise ValueError(f"{who}: {name} must be finite")
    return np.ascontiguousarray(x)


# ------------------------------------------------------------------------------------------------ the index
class L2Index:
    """The corpus of term embeddings on the GPU, uploaded once.

        index = L2Index(corpus)                       # fp32 [n, D], finite
        d2, ids = index.knn(queries, k)               # float64 / int32 [nq, k], on the device
        d2 = index.gather_sorted(targets, nb_ids)     # float64 [m, K], each row ascending

    d2 is the float64 chain ``acc = fma(t, t, acc)``, ``t = (double)q[j] - (double)c[j]``, j ascending from +0.0; the order
    is d2 ascending, ties lowest corpus id first; unused slots hold id -1 and +inf.  Results are bit-reproducible and do not
    depend on ``chunk_rows`` or on how the queries are sliced."""

    def __init__(self, corpus, device="cuda"):
        e = check_rows(corpus, "L2Index", "corpus")
        self.device = cuda_device(device)
        if self.device.type != "cuda":
            raise ValueError("L2Index: runs on a GPU")
        self.n, self.dim = int(e.shape[0]), int(e.shape[1])
        self.emb = torch.from_numpy(e).to(self.device)

    def _queries(self, x, who: str, name: str) -> torch.Tensor:
        return torch.from_numpy(check_rows(x, f"L2Index.{who}", name, self.dim)).to(self.device)

    def knn(self, queries, k: int, chunk_rows: int = 0, query_slice: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ``k`` nearest corpus rows of every query -> (d2 float64 [nq, k], ids int32 [nq, k])."""
        k = check_k(k, "L2Index.knn")
        chunk_rows, query_slice = int(chunk_rows), int(query_slice)
        if not 0 <= chunk_rows < 2 ** 31 or query_slice < 0:
            raise ValueError("L2Index.knn: chunk_rows and query_slice must be >= 0 (0: default)")
        q = self._queries(queries, "knn", "queries")
        nq, dev, sizing = int(q.shape[0]), self.device, "snx_l2_knn_workspace_bytes"
        d2 = torch.empty((nq, k), dtype=torch.float64, device=dev)
        ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
        step = step_bytes_mean(sizing, _WS_BUDGET, nq, self.n, k, chunk_rows)
        step = min(step, query_slice) if query_slice else step
        with torch.cuda.device(dev):
            for s, m in slices(nq, step):
                ws, ws_bytes = workspace(sizing, dev, m, self.n, k, chunk_rows)
                call("snx_l2_knn", _p(q[s:]), m, _p(self.emb), self.n, self.dim, k, chunk_rows, _p(ids[s:]), _p(d2[s:]),
                     _p(ws), ws_bytes, _stream())
        return d2, ids

    def gather_sorted(self, targets, nb_ids) -> torch.Tensor:
        """d2(targets[i], corpus[nb_ids[i, r]]) for every r, each row sorted ascending -> float64 [m, K]; an id < 0 is
        skipped and leaves a +inf at the row's end."""
        t = self._queries(targets, "gather_sorted", "targets")
        nb = nb_ids if isinstance(nb_ids, torch.Tensor) else torch.as_tensor(np.asarray(nb_ids))
        if nb.dim() != 2 or nb.shape[0] != t.shape[0] or nb.is_floating_point() or not 1 <= nb.shape[1] <= K_MAX:
            raise ValueError(f"L2Index.gather_sorted: nb_ids must be int [{t.shape[0]}, K] with 1 <= K <= {K_MAX}")
        if nb.numel() and int(nb.max()) >= self.n:
            raise ValueError(f"L2Index.gather_sorted: ids must be < {self.n} (negative: skipped)")
        nb = nb.clamp(min=-1).to(self.device, torch.int32).contiguous()
        m, K = int(nb.shape[0]), int(nb.shape[1])
        out = torch.empty((m, K), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            call("snx_l2_gather_sorted", _p(t), m, _p(self.emb), self.n, self.dim, _p(nb), K, _p(out), _stream())
        return out


# ------------------------------------------------------------------------------------------------ information gain
def entropy_ks(n: int, k_entropy: int, k_neighborhood: int) -> Tuple[int, int, int]:
    """(k of the marginal entropy, K rows of a neighbourhood, k of the conditional entropy) for a corpus of ``n`` rows
    (ref:information_gain.py:176, 356, 360-364 with knn_entropy_kl's own clamp)."""
    k1 = min(k_entropy, n - 1)
    K = min(k_neighborhood, n)
    k2 = min(min(k_entropy, k_neighborhood - 1), K - 1)
    return k1, K, k2


def check_ig_ks(k_entropy, k_neighborhood, who: str = "information_gain") -> Tuple[int, int]:
    for v, name in ((k_entropy, "k_entropy"), (k_neighborhood, "k_neighborhood")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
            raise ValueError(f"{who}: {name} must be an int >= 0")
    if int(k_entropy) + 1 > K_MAX or int(k_neighborhood) > K_MAX:
        raise ValueError(f"{who}: needs k_entropy < {K_MAX} and k_neighborhood <= {K_MAX}")
    return int(k_entropy), int(k_neighborhood)


def information_gain(index: L2Index, sources, targets, k_entropy: int = 10, k_neighborhood: int = 50,
                     batch_size: int = 1000) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(information_gain, target_entropy, conditional_entropy), fp32 [m], of the pairs sources[i] -> targets[i] against the
    corpus of ``index`` (all three already normalised, or not, by the caller).

    Per batch of ``batch_size`` pairs: ``knn(targets, k + 1)`` gives rho of the marginal entropy (position min(k, n - 1), no
    self-exclusion), ``knn(sources, K)`` the neighbourhood, ``gather_sorted`` the target's ascending distances to it, from
    which rho of the conditional entropy is position k when the smallest is below 1e-10 and k - 1 otherwise.  Device memory
    does not grow with the number of pairs."""
    k_entropy, k_neighborhood = check_ig_ks(k_entropy, k_neighborhood)
    if isinstance(batch_size, bool) or int(batch_size) < 1:
        raise ValueError("information_gain: batch_size must be >= 1")
    src = check_rows(sources, "information_gain", "sources", index.dim)
    tgt = check_rows(targets, "information_gain", "targets", index.dim)
    if src.shape[0] != tgt.shape[0]:
        raise ValueError("information_gain: one target per source")
    m, n, d = int(src.shape[0]), index.n, index.dim
    k1, K, k2 = entropy_ks(n, k_entropy, k_neighborhood)
    h_t = np.zeros(m, dtype=np.float32)
    h_c = np.zeros(m, dtype=np.float32)
    for s in range(0, m, int(batch_size)):
        e = min(m, s + int(batch_size))
        if k1 >= 1:
            d2, _ = index.knn(tgt[s:e], k1 + 1)
            h_t[s:e] = kl_entropy(np.sqrt(d2[:, k1].cpu().numpy()), d, n, k1).astype(np.float32)
        if k2 >= 1:
            _, ids = index.knn(src[s:e], K)
            dist = np.sqrt(index.gather_sorted(tgt[s:e], ids).cpu().numpy())
            rho = np.where(dist[:, 0] < EPS, dist[:, k2], dist[:, k2 - 1])
            h_c[s:e] = kl_entropy(rho, d, K, k2).astype(np.float32)
    return h_t - h_c, h_t, h_c
