"""The IDF line (csrc/idf.hip, include/snx.h "IDF"): document frequencies on the GPU, the IDF table and its exchange
format, the penalty weights of the IDF-aware FLOPS term, the inference-free ("doc-only") query, and the autograd
binding of the loss with that penalty.

Logarithms and exponentials are evaluated on the host in float64 and rounded once to fp32: the tables have V entries."""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import Iterable, Optional

import numpy as np
import torch

from ._lib import call, fn
from .loss import _f32c
from .ops import _chk, _p, _stream

SMOOTHINGS = ("bm25", "standard", "smooth")
V_MAX = 1 << 20                       # snx_idf_doc_freq: the presence bitmap is V bits of LDS
META_KEYS = ("vocab_size", "num_docs", "smoothing", "tokenizer_name", "dtype", "byte_order")


def _token_rows(input_ids, attention_mask, what: str):
    if not (isinstance(input_ids, torch.Tensor) and isinstance(attention_mask, torch.Tensor)) or input_ids.dim() != 2 or \
            attention_mask.shape != input_ids.shape or input_ids.is_floating_point() or attention_mask.is_floating_point():
        raise ValueError(f"{what}: input_ids and attention_mask must be int tensors [n, S] of one shape")
    if input_ids.device.type != "cuda" or attention_mask.device != input_ids.device:
        raise ValueError(f"{what}: input_ids and attention_mask must live on one GPU")
    if input_ids.shape[1] < 1:
        raise ValueError(f"{what}: rows need at least one position")
    return input_ids.to(torch.long).contiguous(), attention_mask.to(torch.long).contiguous()


def doc_freq(input_ids: torch.Tensor, attention_mask: torch.Tensor, V: int, out: Optional[torch.Tensor] = None,
             num_docs: int = 0, count: Optional[torch.Tensor] = None):
    """Document frequencies of token rows (snx_idf_doc_freq; the counting loop of ref:tools/idf-compute/src/main.rs:160-176).
    ``input_ids`` / ``attention_mask`` [n, S] int on one GPU.  -> (df [V] int64, num_docs + n).  ``out`` (int64 [V]) is added
    to, so batches accumulate; a fresh zeroed table otherwise.  A row counts once for each distinct id in [0, V) at a
    position whose mask is non-zero; other ids are ignored; no cap on S.  EVERY row is a document, also one with no counted
    position: the reference counts every non-empty text, and what is empty is decided before tokenising
    (src/train/cli/compute_idf.py skips empty fields).  ``count``: optional device int64 [1], also incremented by n."""
    V = int(V)
    if not 1 <= V <= V_MAX:
        raise ValueError(f"doc_freq: V must be in [1, {V_MAX}]")
    ids, mask = _token_rows(input_ids, attention_mask, "doc_freq")
    dev = ids.device
    if out is None:
        out = torch.zeros(V, dtype=torch.int64, device=dev)
    else:
        _chk(out, torch.int64, "out", (V,))
        if out.device != dev:
            raise ValueError("doc_freq: out must live on the tokens' GPU")
    if count is not None:
        _chk(count, torch.int64, "count", (1,))
    n, S = int(ids.shape[0]), int(ids.shape[1])
    with torch.cuda.device(dev):
        call("snx_idf_doc_freq", _p(ids), _p(mask), n, S, V, _p(out), _p(count), _stream())
    return out, int(num_docs) + n


def idf_from_counts(doc_freq_counts, num_docs: int, smoothing: str = "bm25") -> np.ndarray:
    """idf [V] fp32 from document frequencies: float64 on the host, one rounding.
    bm25: ln(1 + (N - df + 0.5) / (df + 0.5)); standard: ln(N / (df + 1)) (ref:tools/idf-compute/src/main.rs:199-205);
    smooth: ln((N + 1) / (df + 1)) + 1 (ref:tests/test_korean_neural_sparse.py:110)."""
    if smoothing not in SMOOTHINGS:
        raise ValueError(f"unknown smoothing {smoothing!r}; choose from {SMOOTHINGS}")
    df = np.asarray(doc_freq_counts, dtype=np.float64)
    n = np.float64(num_docs)
    if smoothing == "bm25":
        v = np.log(1.0 + (n - df + 0.5) / (df + 0.5))
    elif smoothing == "standard":
        with np.errstate(divide="ignore"):
            v = np.log(n / (df + 1.0))
    else:
        v = np.log((n + 1.0) / (df + 1.0)) + 1.0
    return v.astype(np.float32)


class IdfTable:
    """Document frequencies accumulated on the GPU and the IDF weights derived from them.

        t = IdfTable(V, device, tokenizer_name="...")
        t.fit_tokens(input_ids, attention_mask)          # per batch
        w = t.idf("bm25")                                # numpy fp32 [V]
        t.save("out/idf")                                # out/idf.bin + out/idf.json, the reference's exchange format
        IdfTable.load("out/idf")                         # -> (numpy fp32 [V], metadata dict)
    """

    def __init__(self, vocab_size: int, device="cuda", tokenizer_name: str = ""):
        self.vocab_size = int(vocab_size)
        if not 1 <= self.vocab_size <= V_MAX:
            raise ValueError(f"IdfTable: vocab_size must be in [1, {V_MAX}]")
        self.device = torch.device(device)
        self.tokenizer_name = str(tokenizer_name)
        self.num_docs = 0
        self.df: Optional[torch.Tensor] = None

    def fit_tokens(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> "IdfTable":
        self.df, self.num_docs = doc_freq(input_ids.to(self.device), attention_mask.to(self.device), self.vocab_size,
                                          out=self.df, num_docs=self.num_docs)
        return self

    def doc_freq_host(self) -> np.ndarray:
        if self.df is None:
            return np.zeros(self.vocab_size, dtype=np.int64)
        return self.df.cpu().numpy()

    def idf(self, smoothing: str = "bm25") -> np.ndarray:
        return idf_from_counts(self.doc_freq_host(), self.num_docs, smoothing)

    def save(self, path_without_ext, smoothing: str = "bm25") -> dict:
        return save_idf(path_without_ext, self.idf(smoothing), self.num_docs, smoothing, self.tokenizer_name)

    @staticmethod
    def load(path_without_ext):
        return load_idf(path_without_ext)

    def to_pt(self, path, smoothing: str = "bm25") -> str:
        return idf_to_pt(self.idf(smoothing), path)

    def save_idf_json(self, path, tokenizer, smoothing: str = "bm25") -> int:
        return save_idf_json(path, self.idf(smoothing), tokenizer)


def save_idf(path_without_ext, idf, num_docs: int, smoothing: str, tokenizer_name: str) -> dict:
    """``.bin``: little-endian f32 x vocab_size; ``.json``: the six keys of ref:tools/idf-compute/src/main.rs:224-231 -- what
    ref:tools/idf-compute/load_idf.py reads (np.fromfile(bin, float32, count=vocab_size)).  Extensions are set the way
    that loader does (``Path.with_suffix``)."""
    w = np.ascontiguousarray(np.asarray(idf, dtype=np.float32))
    if w.ndim != 1:
        raise ValueError("save_idf: idf must be [V]")
    base = Path(path_without_ext)
    if base.parent != Path(""):
        base.parent.mkdir(parents=True, exist_ok=True)
    meta = {"vocab_size": int(w.shape[0]), "num_docs": int(num_docs), "smoothing": str(smoothing),
            "tokenizer_name": str(tokenizer_name), "dtype": "float32", "byte_order": "little_endian"}
    with open(base.with_suffix(".bin"), "wb") as f:
        f.write(w.astype("<f4").tobytes())
    with open(base.with_suffix(".json"), "w") as f:
        json.dump(meta, f, indent=2)
    return meta


def load_idf(path_without_ext):
    """-> (idf numpy fp32 [V], metadata) from ``.bin`` + ``.json`` (a ``.pt`` file is read through torch.load)."""
    base = Path(path_without_ext)
    if base.suffix == ".pt":
        w = torch.load(str(base), map_location="cpu")
        w = w.detach().to(torch.float32).numpy()
        return w, {"vocab_size": int(w.shape[0])}
    with open(base.with_suffix(".json")) as f:
        meta = json.load(f)
    if meta.get("dtype", "float32") != "float32" or meta.get("byte_order", "little_endian") != "little_endian":
        raise ValueError(f"{base}.json: only little-endian float32 tables are supported")
    V = int(meta["vocab_size"])
    w = np.fromfile(str(base.with_suffix(".bin")), dtype="<f4", count=V)
    if w.shape[0] != V:
        raise ValueError(f"{base}.bin holds {w.shape[0]} values, metadata says {V}")
    return w.astype(np.float32), meta


def idf_to_pt(idf, path) -> str:
    """The ``.pt`` form of ref:tools/idf-compute/load_idf.py:27-32: one fp32 tensor [V]."""
    out = Path(path).with_suffix(".pt")
    torch.save(torch.from_numpy(np.ascontiguousarray(np.asarray(idf, dtype=np.float32))), str(out))
    return str(out)


def save_idf_json(path, idf, tokenizer) -> int:
    """token string -> weight, the ``idf.json`` a doc-only model ships (ref:tests/test_korean_neural_sparse.py:94-122).
    Ids the tokenizer has no string for are left out; -> the number of entries written."""
    w = np.asarray(idf, dtype=np.float32)
    toks = tokenizer.convert_ids_to_tokens(list(range(int(w.shape[0]))))
    table = {t: float(v) for t, v in zip(toks, w.tolist()) if isinstance(t, str)}
    with open(path, "w", encoding="utf-8") as f:
        json.dump(table, f, ensure_ascii=False)
    return len(table)


def penalty_weights(idf, alpha: float = 4.0, special_ids: Iterable[int] = (), special_penalty: float = 100.0,
                    stopword_ids: Iterable[int] = (), stopword_penalty: float = 15.0) -> torch.Tensor:
    """The per-token weights of the IDF-aware FLOPS penalty (ref:docs/concepts/04-loss-functions.md §5 "V26",
    ref:scripts/test_idf_math.py:61-126), float64 on the host, returned as fp32 [V] (CPU):
      idf_norm = (idf - min_real) / (max_real - min_real + 1e-8)   min / max over the non-special ids
      w        = exp(-alpha * idf_norm)
      w[stop] *= stopword_penalty                                  (test_idf_math.py:123-126)
      w[special] = special_penalty                                 (docs §5)
    The defaults are the reference's V26 values."""
    v = np.asarray(idf.detach().cpu().numpy() if isinstance(idf, torch.Tensor) else idf, dtype=np.float64)
    if v.ndim != 1 or v.shape[0] < 1:
        raise ValueError("penalty_weights: idf must be [V]")
    V = v.shape[0]
    special = np.unique(np.asarray(list(special_ids), dtype=np.int64))
    stop = np.unique(np.asarray(list(stopword_ids), dtype=np.int64))
    for name, a in (("special_ids", special), ("stopword_ids", stop)):
        if a.size and (a.min() < 0 or a.max() >= V):
            raise ValueError(f"penalty_weights: {name} outside [0, {V})")
    real = np.ones(V, dtype=bool)
    real[special] = False
    if not real.any():
        raise ValueError("penalty_weights: every id is special")
    lo, hi = v[real].min(), v[real].max()
    w = np.exp(-np.float64(alpha) * ((v - lo) / (hi - lo + 1e-8)))
    w[stop] *= np.float64(stopword_penalty)
    w[special] = np.float64(special_penalty)
    return torch.from_numpy(w.astype(np.float32))


def idf_query_rows(input_ids: torch.Tensor, attention_mask: torch.Tensor, allowed: torch.Tensor, idf: torch.Tensor):
    """Inference-free query rows: the (vals, ids, cnt) triple every ``SparseIndex`` search takes.  The ids are the distinct
    counted ids of ``term_counts`` (ascending), the weight is idf[id] ONCE per distinct id, whatever its count
    (ref:tests/test_korean_neural_sparse.py:417-427); unused slots carry id -1 and weight 0.  Sparse rows hold weights > 0
    (``pack_rows``), so an id with idf <= 0 -- "standard" smoothing at df = N -- leaves the row: it could add nothing (0) or
    only push a score down (< 0), and OpenSearch's sparse fields take positive weights."""
    from .retrieval.hybrid import term_counts
    _chk(allowed, torch.uint8, "allowed")
    _chk(idf, torch.float32, "idf", (int(allowed.numel()),))
    allowed = allowed * (idf > 0).to(torch.uint8)
    term, _tf, cnt, _len = term_counts(input_ids, attention_mask, allowed)
    vals = idf[term.clamp_min(0).long()]
    vals = torch.where(term >= 0, vals, torch.zeros((), dtype=torch.float32, device=vals.device))
    return vals.contiguous(), term, cnt


def idf_query_dense(input_ids: torch.Tensor, attention_mask: torch.Tensor, allowed: torch.Tensor,
                    idf: torch.Tensor) -> torch.Tensor:
    """q [B, V] fp32 (snx_idf_query_dense): q[b, id] = idf[id] for every id of row b at a masked-in position with
    allowed[id] != 0, zero elsewhere -- the anchor of a doc-only training step.  One launch, no memset."""
    ids, mask = _token_rows(input_ids, attention_mask, "idf_query_dense")
    dev = ids.device
    _chk(allowed, torch.uint8, "allowed")
    if allowed.dim() != 1 or allowed.numel() < 1 or allowed.device != dev:
        raise ValueError("idf_query_dense: allowed must be uint8 [V] on the tokens' GPU")
    V = int(allowed.numel())
    _chk(idf, torch.float32, "idf", (V,))
    if idf.device != dev:
        raise ValueError("idf_query_dense: idf must live on the tokens' GPU")
    B, S = int(ids.shape[0]), int(ids.shape[1])
    q = torch.empty((B, V), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("snx_idf_query_dense", _p(ids), _p(mask), _p(allowed), _p(idf), B, S, V, _p(q), _stream())
    return q


def flops_workspace(V: int, device) -> torch.Tensor:
    nbytes = int(fn("snx_idf_flops_workspace_bytes")(int(V)))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)     # 8-byte aligned


def idf_flops_fwd(x: torch.Tensor, w: torch.Tensor, beta: float, lam: float = 0.0, loss: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None):
    """P(x) = sum_j w_j |a_j| + beta * sum_j w_j a_j^2 over the column means a of ``x`` [R, V] fp32 (snx_idf_flops_fwd).
    -> (out3 = {sum t1, sum t2, P} fp32 on the device, workspace).  ``loss`` (fp32 [1] or 0-d): loss += fp32(lam * P) in
    place.  The workspace's first V floats are the means (``flops_means``) the backward reads."""
    _chk(x, torch.float32, "x")
    if x.dim() != 2:
        raise ValueError("idf_flops_fwd: x must be [R, V]")
    R, V = int(x.shape[0]), int(x.shape[1])
    _chk(w, torch.float32, "w", (V,))
    if loss is not None:
        _chk(loss, torch.float32, "loss")
        if loss.numel() != 1:
            raise ValueError("idf_flops_fwd: loss must hold one element")
    if ws is None:
        ws = flops_workspace(V, x.device)
    out3 = torch.empty(3, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        call("snx_idf_flops_fwd", _p(x), R, V, _p(w), float(beta), float(lam), _p(ws), _p(out3), _p(loss), _stream())
    return out3, ws


def flops_means(ws: torch.Tensor, V: int) -> torch.Tensor:
    """The column means a forward left in its workspace: fp32 [V] (a view)."""
    return ws.view(torch.float32)[:int(V)]


def idf_flops_bwd_accum(dx: torch.Tensor, ws: torch.Tensor, w: torch.Tensor, beta: float, lam: float,
                        g: torch.Tensor) -> torch.Tensor:
    """dx [R, V] += g * lam * w_j * (sign(a_j) + 2 beta a_j) / R, in place (snx_idf_flops_bwd_accum); ``g`` a device fp32
    scalar, ``ws`` the forward's workspace.  ``dx`` may be a row range of a larger contiguous buffer."""
    _chk(dx, torch.float32, "dx")
    if dx.dim() != 2:
        raise ValueError("idf_flops_bwd_accum: dx must be [R, V]")
    R, V = int(dx.shape[0]), int(dx.shape[1])
    _chk(w, torch.float32, "w", (V,))
    _chk(g, torch.float32, "g")
    with torch.cuda.device(dx.device):
        call("snx_idf_flops_bwd_accum", _p(dx), R, V, _p(ws), _p(w), float(beta), float(lam), _p(g), _stream())
    return dx


class SpladeLossIdfFn(torch.autograd.Function):
    """(q [B,V], p [Bp,V], n [B*k,V]) -> (loss 0-d, scalars [18]): SPLADELossV33 with its three FLOPS terms replaced by the
    IDF-aware penalty P.  scalars = the nine of snx.loss.SpladeLossFn (its flops_* stay the UNWEIGHTED sums the base kernel
    reports) followed by {l1, l2, P} for q, p, n (zeros for a side whose lambda is 0).
    Forward: snx_loss_fwd with lambda_q = lambda_d = lambda_neg = 0, then snx_idf_flops_fwd per side with a non-zero lambda
    in the fixed order q, p (the own rows [label_off, label_off + B)), n, each adding fp32(lambda * P) to the loss.
    Backward: snx_loss_bwd into ONE buffer with three adjacent row ranges, as SpladeLossFn, then snx_idf_flops_bwd_accum
    on the matching ranges -- the ranges stay adjacent views of one storage (snx/encoder.py _gather_rows)."""

    @staticmethod
    def forward(ctx, q, p, n, w, tpos, tneg, hp, beta, k, label_off, bf16_mm, tscores=None):
        if not q.is_cuda:
            raise RuntimeError("SPLADELossIDF (snx backend) needs GPU tensors; there is no CPU fallback")
        q, p, n = _f32c(q), _f32c(p), _f32c(n)
        B, V = q.shape
        Bp = p.shape[0]
        if p.shape[1] != V or n.shape != (B * k, V):
            raise ValueError(f"loss: inconsistent shapes q{tuple(q.shape)} p{tuple(p.shape)} n{tuple(n.shape)} k={k}")
        _chk(w, torch.float32, "penalty_weights", (V,))
        tp = _f32c(tpos) if tpos is not None else None
        tn = _f32c(tneg).view(-1) if tneg is not None else None
        if tp is not None and (tp.numel() != B or tn is None or tn.numel() != B * k):
            raise ValueError("teacher score shapes must be [B] and [B,k]")
        hp = tuple(float(x) for x in hp)
        if len(hp) == 5:
            hp = hp + (0.0, 1.0)
        lams = hp[1:4]
        ts = _f32c(tscores) if (tscores is not None and hp[5] > 0) else None
        if ts is not None and tuple(ts.shape) != (B, B):
            raise ValueError(f"teacher_scores must be [B, B] = [{B}, {B}], got {tuple(ts.shape)}")
        dims = (C.c_int32 * 6)(B, Bp, k, V, label_off, int(bf16_mm))
        hpa = (C.c_float * 7)(hp[0], 0.0, 0.0, 0.0, *hp[4:])
        ws = torch.empty(fn("snx_loss_workspace_bytes")(B, Bp, k, V), dtype=torch.uint8, device=q.device)
        out = torch.zeros(18, dtype=torch.float32, device=q.device)
        call("snx_loss_fwd", _p(q), _p(p), _p(n), _p(tp), _p(tn), _p(ts), hpa, dims, _p(ws), _p(out), _stream())
        sides = (q, p[label_off:label_off + B], n)
        pws = [None, None, None]
        for s in range(3):
            if lams[s] != 0.0:
                pws[s] = flops_workspace(V, q.device)
                call("snx_idf_flops_fwd", _p(sides[s]), int(sides[s].shape[0]), V, _p(w), float(beta), lams[s],
                     _p(pws[s]), _p(out[9 + 3 * s:]), _p(out), _stream())
        ctx.save_for_backward(q, p, n, ws, w, *[x for x in pws if x is not None])
        ctx.have = [x is not None for x in pws]
        ctx.dims, ctx.hp, ctx.use_kd = dims, hpa, int(ts is not None)
        ctx.lams, ctx.beta, ctx.label_off = lams, float(beta), int(label_off)
        loss = out[0].clone()
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, gloss, _gs):
        q, p, n, ws, w, *rest = ctx.saved_tensors
        rest = list(rest)
        pws = [rest.pop(0) if h else None for h in ctx.have]
        g = gloss.to(torch.float32).contiguous().view(1)
        B, Bp, V = q.shape[0], p.shape[0], q.shape[1]
        g_all = torch.empty((B + Bp + n.shape[0], V), dtype=torch.float32, device=q.device)
        dq, dp, dn = g_all[:B], g_all[B:B + Bp], g_all[B + Bp:]
        call("snx_loss_bwd", _p(q), _p(p), _p(n), _p(g), ctx.hp, ctx.dims, _p(ws), ctx.use_kd, _p(dq), _p(dp), _p(dn),
             _stream())
        targets = (dq, dp[ctx.label_off:ctx.label_off + B], dn)
        for s in range(3):
            if pws[s] is not None:
                call("snx_idf_flops_bwd_accum", _p(targets[s]), int(targets[s].shape[0]), V, _p(pws[s]), _p(w),
                     ctx.beta, ctx.lams[s], _p(g), _stream())
        return dq, dp, dn, None, None, None, None, None, None, None, None, None


def splade_loss_idf(q, p, n, w, hp, k: int, beta: float = 0.3, tpos: Optional[torch.Tensor] = None,
                    tneg: Optional[torch.Tensor] = None, label_off: int = 0, bf16_mm: bool = False,
                    tscores: Optional[torch.Tensor] = None):
    """``snx.loss.splade_loss`` with the IDF-aware FLOPS penalty: hp as there (its lambdas weigh P(q), P(pos), P(neg)),
    ``w`` the fp32 [V] penalty weights on the device.  -> (loss, scalars [18])."""
    return SpladeLossIdfFn.apply(q, p, n, w, tpos, tneg, tuple(hp), float(beta), int(k), int(label_off), bool(bf16_mm),
                                 tscores)
