"""Exact restatement of the weight-gradient ("TN") GEMM family (csrc/gemm.hip: the 128x128 token-split kernel and
tn128_reduce_kernel; csrc/gemm_tn256.hip: the 256x256 persistent kernel and tn256_reduce_kernel; csrc/gemm_tn.h), the
case tables, a restatement of both launch plans, and a per-element check whose acceptance SETS follow from the one place
the family rounds.  Plain torch / numpy on the CPU; sibling of tests/gemm_reference.py, whose guarded buffers and
check_guarded it reuses.

The operation.  dW_out[n,k] = dW0[n,k] + sum_m dY[m,n'] X[m,k], bf16 operands, fp32 result.  For
snx_gemm_tn_accum_interleaved and `interleaved = 1` in a group, n' is the column of dY that holds natural row n: dY's
columns come in the interleaved GeGLU order (per 64 columns: 32 of a, then 32 of g), column n' belongs to natural row
src_rows(N)[n'] (geglu_src_row of csrc/elementwise.hip; _natural in tests/test_gpu_ops.py states the inverse).  The
product of two bf16 values is exact in fp32; the only rounding is fp32 addition -- inside the MFMA, along a workgroup's
K-steps, across slabs or atomics, and the final `+=`.

Two input families, as in the NT reference.
  exact     dY and X are multiples of 2^-3 with |.| <= 1/2 (gemm_reference's three row classes -- symmetric, non-negative,
            large-only -- dealt per token row), dW0 a multiple of 2^-6 with |dW0| <= 64.  With M <= 8,448 every product,
            partial sum, slab and result is a multiple of 2^-6 below 2^12 (twice the sum on top of dW0: below 2^13): exact
            in fp32 in ANY order.  ONE admissible value per element, formed as an integer matrix product in float32 (the
            host test asserts that it equals the float64 one).  The check assumes nothing about the MFMA, the summation
            tree or the order in which atomics arrive, so it holds bit for bit with "det_reduce" 0 as well.
  random    0.1 randn for dY, randn for X and dW0 (what tests/test_gpu_ops.py uses), M <= 1,408.  S = the float64 sum,
            Abs = |dW0| + sum |dy||x|, delta = gamma_n Abs + (M + 1) 2^-52 Abs with gamma_n = n 2^-24 / (1 - n 2^-24)
            (Higham, Accuracy and Stability, 4.2) and n = M + c + 8, c = the number of partials the plan adds into that
            element's tile (slabs or splits, or 1 for a direct flush; a ragged rest counts as one more).  The accepted
            set is the fp32 values inside [S - delta, S + delta].
            ASSUMPTION (MFMA-ADD): each of the MFMA's additions errs by at most 2^-24 of its result, in whatever order
            it adds; the products of two bf16 values are exact.  The guides do not state the MFMA's internal order or
            rounding; nothing else about the hardware's sum is assumed.
            M <= 1,408 keeps 8 M^2 2^-24 <= 1: delta stays below an eighth of a mean term, the set cannot swallow a
            dropped or doubled token row (asserted when a case is built).

Guards.  dW lives inside a larger fp32 buffer with GUARD_ROWS = 128 rows of the NaN sentinel before and after, its body
pre-filled with dW0.  dY and X carry 128 rows of bf16 NaN before row 0 and after row M - 1: a row multiplied that should
not be poisons the tile.  The workspace is exactly workspace_bytes() = snx_gemm_tn_workspace_bytes() bytes of the fp32
NaN sentinel followed by a guard of the same sentinel: a reduce that reads a slab nobody wrote turns dW into NaN, a flush
past the advertised size shows in the guard.

Launch arithmetic restated.  tn128_plan (tn_pick_splits / tn128_plan of gemm.hip), tn256_plan (tn256_schedule, item_at,
contributor_of, tail_contributors and the reduce's `sb < se` skip of gemm_tn256.hip: what every workgroup multiplies,
which slab it writes, which slabs the reduce adds), workspace_bytes (tn_group_ws_bytes) and dispatch (launch_tn_group).
The case tables state the class of every row and ASSERT it through the plans at import.
tests/test_tn_reference_host.py ties the plans to the library (workspace bytes, to the byte, on every row and a sweep of
M = 1..9,000), proves that writes and reads of the slabs agree, and that the reference admits fp32 emulations of both trees
and rejects the planted faults.

Measured on an MI355X with the kernels of commit e0eeae8 plus the M < 64 dispatch fix that arrives with this file (no
kernel arithmetic changes), over all cases of tests/test_gpu_tn_per_element.py.  Nothing fell outside its set:
    form      family   elements     pinned to one value
    256x256   exact    87,588,864   100 %, met bit for bit with "det_reduce" 1 and with float atomics
              random    1,245,184   0 % (every set wider than two adjacent fp32 values)
    128x128   exact     3,588,096   100 %
              random      638,976   0 %
34 tests, 207 launches, 5.0 s for the file, 0.47 s for the slowest test.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests import gemm_reference as G

BF16 = G.BF16
U32 = G.U32
GUARD_ROWS = G.GUARD_ROWS
SENT_F32 = G.SENT_F32
guarded, check_guards, check_guarded, cdiv, _raw = G.guarded, G.check_guards, G.check_guarded, G.cdiv, G._raw
M_EXACT_MAX = 8448
M_RANDOM_MAX = 1408
TAIL_PCT = 95                       # csrc/config.h tn256_tail_pct
SLAB256 = 256 * 256 * 4
SLAB128 = 128 * 128 * 4


def norm_group(group):
    """((N, K) or (N, K, interleaved), ...) -> ((N, K, 0 / 1), ...)"""
    out = tuple((int(p[0]), int(p[1]), int(bool(p[2])) if len(p) > 2 else 0) for p in group)
    assert 1 <= len(out) <= 4 and all(N % 128 == 0 and K % 128 == 0 and N > 0 and K > 0 for N, K, _ in out)
    return out


def src_rows(N):
    """natural Wi row held by interleaved row / dY column n' (geglu_src_row with I = N / 2), as an int64 array"""
    n = np.arange(N)
    return np.where((n & 63) < 32, 32 * (n >> 6) + (n & 31), N // 2 + 32 * (n >> 6) + (n & 31))


# ----------------------------------------------------------------------------- launch arithmetic, restated
def tn_pick_splits(tiles, M):
    max_splits = max(1, cdiv(M, 256))
    best, best_fill, s = 1, 0.0, 1
    while s <= max_splits and s <= 32 and tiles * s <= 8 * 512:
        w = tiles * s
        fill = w / float(cdiv(w, 512) * 512)
        if fill > best_fill + 0.02:
            best_fill, best = fill, s
        s += 1
    return best


def tn128_plan(group, M):
    """128x128 kernel: output tiles of the group, token splits, rows per split (whole 64-row steps), rows of the last
    split; slabs = splits where the ordered reduction needs a workspace (more than one split), else 0 (direct flush)"""
    group = norm_group(group)
    tiles = sum((N // 128) * (K // 128) for N, K, _ in group)
    splits = tn_pick_splits(tiles, M)
    rows = cdiv(cdiv(M, splits), 64) * 64
    splits = cdiv(M, rows)
    return SimpleNamespace(form="128", tiles=tiles, splits=splits, rows=rows, last=M - (splits - 1) * rows,
                           slabs=splits if splits > 1 else 0)


def tiles256(group):
    """[(problem, n0, k0)] in the tile order of decode()"""
    out = []
    for p, (N, K, _) in enumerate(norm_group(group)):
        tk = cdiv(K, 256)
        out += [(p, (t // tk) * 256, (t % tk) * 256) for t in range(cdiv(N, 256) * tk)]
    return out


@functools.lru_cache(maxsize=None)
def _sched(ntiles, nsteps, nwg):
    """tn256_schedule's scalars: (P, nmain, main_len, tail_len, tail_u, slabs), None where the kernel declines"""
    if ntiles > nwg:
        return None
    P = nwg // ntiles
    nmain = P * ntiles
    wt = nwg - nmain
    tail_len = nsteps * wt * TAIL_PCT // (100 * nwg) if wt > 0 else 0
    main_len = nsteps - tail_len
    tail_u = cdiv(ntiles * tail_len, wt) if wt > 0 else 0
    if tail_u <= 0:
        tail_len, main_len = 0, nsteps
    mt = max(_tail_contributors(t, tail_len, tail_u) for t in range(ntiles))
    return P, nmain, main_len, tail_len, tail_u, P + mt


def _tail_contributors(tile, tail_len, tail_u):
    if tail_len <= 0:
        return 0
    return ((tile + 1) * tail_len - 1) // tail_u - (tile * tail_len) // tail_u + 1


def tn256_plan(group, M, reserved=0):
    """What gemm_tn256.hip makes of a group over the whole K-steps of M token rows on 256 - reserved (rounded up to 8)
    workgroups; None where the group has more 256-tiles than workgroups (the 128x128 kernel takes it) or M holds no
    whole K-step.  items[L] = [(tile, sb, se)] of logical workgroup L (item_at, walked as the kernel walks it);
    writes[(contributor, tile)] = [L, ...] from contributor_of (the host test asserts one writer per slab);
    reads[tile] = the slab indices the reduce adds, in its order (non-empty main pieces, then tail_contributors)."""
    group = norm_group(group)
    nwg = 256 - cdiv(reserved, 8) * 8
    M64 = M & ~63
    tl = tiles256(group)
    ntiles, nsteps = len(tl), M64 // 64
    sc = _sched(ntiles, nsteps, nwg) if M64 >= 64 else None
    if sc is None:
        return None
    P, nmain, main_len, tail_len, tail_u, slabs = sc

    def item_at(L, it):
        if L < nmain:
            if it > 0:
                return None
            p = L // ntiles
            sb, se = p * main_len // P, (p + 1) * main_len // P
            return (L - p * ntiles, sb, se) if sb < se else None
        if tail_len <= 0:
            return None
        U = ntiles * tail_len
        ub = (L - nmain) * tail_u
        ue = min(U, ub + tail_u)
        if ub >= ue:
            return None
        tile = ub // tail_len + it
        lo, hi = max(ub, tile * tail_len), min(ue, (tile + 1) * tail_len)
        if lo >= hi:
            return None
        return tile, main_len + lo - tile * tail_len, main_len + hi - tile * tail_len

    def contributor_of(L, tile):
        return L // ntiles if L < nmain else P + (L - nmain) - (tile * tail_len) // tail_u

    items, writes = {}, {}
    for L in range(nwg):
        its, it = [], 0
        while True:
            o = item_at(L, it)
            if o is None:
                break
            its.append(o)
            writes.setdefault((contributor_of(L, o[0]), o[0]), []).append(L)
            it += 1
        items[L] = its
    nonempty = [p for p in range(P) if p * main_len // P < (p + 1) * main_len // P]
    tc = [_tail_contributors(t, tail_len, tail_u) for t in range(ntiles)]
    reads = {t: nonempty + [P + c for c in range(tc[t])] for t in range(ntiles)}
    tails = [items[L] for L in range(nmain, nwg)]
    half = sum(1 for p, n0, k0 in tl if n0 + 256 > group[p][0] or k0 + 256 > group[p][1])
    return SimpleNamespace(form="256", group=group, M=M, M64=M64, nwg=nwg, tiles=tl, ntiles=ntiles, nsteps=nsteps, P=P,
                           nmain=nmain, spare=nwg - nmain, main_len=main_len, tail_len=tail_len, tail_u=tail_u,
                           empty=P - len(nonempty), longest=max(se - sb for v in items.values() for _, sb, se in v),
                           tc_min=min(tc), tc_max=max(tc), span=max((len(v) for v in tails), default=0),
                           idle=sum(1 for v in tails if not v), slabs=slabs, half_outside=half, rest=M - M64,
                           items=items, writes=writes, reads=reads)


def workspace_bytes(group, M):
    """tn_group_ws_bytes: the maximum over reserved = 0, 8, ..., 128 of the 256-form slabs (none below one whole K-step),
    and the 128-form slabs when it splits the token range"""
    group = norm_group(group)
    need, M64, ntiles = 0, M & ~63, len(tiles256(group))
    if M64 >= 64:
        for r in range(0, 129, 8):
            sc = _sched(ntiles, M64 // 64, 256 - r)
            if sc is not None:
                need = max(need, sc[5] * ntiles * SLAB256)
    p = tn128_plan(group, M)
    if p.splits > 1:
        need = max(need, p.splits * p.tiles * SLAB128)
    return need


def dispatch(group, M, tn256=1, tn256_min_m=8192, reserved=0):
    """launch_tn_group: the plan that runs -- the 256 form from "tn256_min_m" rows on where the range holds one whole
    K-step and the group fits the workgroups, else the 128x128 kernel"""
    if tn256 and M >= tn256_min_m and (M & ~63) >= 64:
        p = tn256_plan(group, M, reserved)
        if p is not None:
            return p
    return tn128_plan(group, M)


def partial_counts(group, M, plan):
    """per problem an int array [N, K] in NATURAL row order: the number of partials the plan adds into the element"""
    group = norm_group(group)
    out = [np.full((N, K), max(plan.splits, 1) if plan.form == "128" else 0, dtype=np.int64) for N, K, _ in group]
    if plan.form == "256":
        for t, (p, n0, k0) in enumerate(plan.tiles):
            out[p][n0:n0 + 256, k0:k0 + 256] = len(plan.reads[t]) + (1 if plan.rest else 0)
        for p, (N, K, inter) in enumerate(group):
            if inter:
                nat = np.empty_like(out[p])
                nat[src_rows(N)] = out[p]
                out[p] = nat
    return out


# ----------------------------------------------------------------------------- cases
def _bf16_guarded(mid):
    buf, view = guarded(mid.shape[0], mid.shape[1], BF16)
    view.copy_(mid.to(BF16))
    return buf


@functools.lru_cache(maxsize=3)
def build_case(family, group, M):
    """inputs and the float64 side of one (family, group, M).  Per problem p: dY[p], X[p] = guarded bf16 buffers (NaN rows
    around the M token rows; dY's columns in the interleaved order where the problem says so), dW0[p] fp32 [N, K], and
      exact   want[p] = THE fp32 result, sum32[p] = the float32 integer product it was formed from (times 64)
      random  S[p], Abs[p] (float64), natural row order"""
    group = norm_group(group)
    assert family in ("exact", "random")
    g = torch.Generator().manual_seed(7919 * M + sum((i + 1) * (1009 * N + K + inter) for i, (N, K, inter) in enumerate(group))
                                      + (3 if family == "exact" else 0))
    c = SimpleNamespace(family=family, group=group, M=M, dY=[], X=[], dW0=[], want=[], sum32=[], S=[], Abs=[])
    if family == "exact":
        assert M <= M_EXACT_MAX and 16 * M < 2 ** 24
    else:
        assert M <= M_RANDOM_MAX and 8 * M * M * U32 <= 1, "random family: 8 M^2 2^-24 <= 1"
    for N, K, inter in group:
        if family == "exact":
            dy, x = G._exact_matrix(g, M, N), G._exact_matrix(g, M, K)
            dw0 = torch.randint(-4096, 4097, (N, K), generator=g).to(torch.float32) / 64.0
        else:
            dy, x = 0.1 * torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
            dw0 = torch.randn(N, K, generator=g)
        dy, x = dy.to(BF16), x.to(BF16)
        nat = dy[:, torch.from_numpy(np.argsort(src_rows(N)))] if inter else dy     # natural row n <- column n' of dY
        if family == "exact":
            s32 = (nat.float() * 8).t().contiguous() @ (x.float() * 8)              # integers below 2^24: exact, any order
            c.sum32.append(s32)
            c.want.append(dw0 + s32 / 64.0)                                          # multiples of 2^-6 below 2^12: exact
            assert float(c.want[-1].abs().max()) < 4096 and float(s32.abs().max()) < 2 ** 24
        else:
            d64, x64 = nat.double(), x.double()
            c.S.append((dw0.double() + d64.t() @ x64).numpy())
            c.Abs.append((dw0.double().abs() + d64.abs().t() @ x64.abs()).numpy())
        c.dY.append(_bf16_guarded(dy))
        c.X.append(_bf16_guarded(x))
        c.dW0.append(dw0)
    return c


def operands(c, p):
    """the M token rows of problem p's guarded operands: (dY, X) bf16"""
    return c.dY[p][GUARD_ROWS:GUARD_ROWS + c.M], c.X[p][GUARD_ROWS:GUARD_ROWS + c.M]


def expected(c, plan, launches=1):
    """per problem (lo, hi) float64 [N, K]: exact family lo = hi = dW0 + launches x sum; random family the fp32 values inside
    [S - delta, S + delta] (one launch)"""
    out = []
    if c.family == "exact":
        for dw0, s32 in zip(c.dW0, c.sum32):
            v = (dw0 + launches * (s32 / 64.0)).double().numpy()
            out.append((v, v))
        return out
    assert launches == 1
    for S, Abs, cnt in zip(c.S, c.Abs, partial_counts(c.group, c.M, plan)):
        n = c.M + cnt + 8
        delta = (n * U32 / (1 - n * U32) + (c.M + 1) * 2.0 ** -52) * Abs
        lo, hi = G.f32_up(S - delta), G.f32_down(S + delta)
        assert bool((lo <= hi).all())
        out.append((lo, hi))
    return out


def guarded_dw(dw0, device="cpu"):
    """(guarded fp32 buffer whose body holds dW0, view of the body)"""
    buf, mid = guarded(dw0.shape[0], dw0.shape[1], torch.float32, device)
    mid.copy_(dw0)
    return buf, mid


def workspace(nbytes, device="cpu"):
    """exactly nbytes of the fp32 NaN sentinel + GUARD_ROWS x 256 sentinel words behind them, as one int32 tensor"""
    assert nbytes % 4 == 0
    return torch.full((nbytes // 4 + GUARD_ROWS * 256,), SENT_F32, dtype=torch.int32, device=device)


def check_workspace(ws, nbytes, what):
    bad = (ws[nbytes // 4:] != SENT_F32).nonzero()
    assert bad.numel() == 0, f"{what}: {len(bad)} words written behind the advertised {nbytes} workspace bytes, first at +{int(bad[0])}"


# ----------------------------------------------------------------------------- case tables
SMALL_LAYER = ((768, 256), (768, 256, 1), (256, 384), (256, 256))
LAYER_149M = ((2304, 768), (2304, 768, 1), (768, 1152), (768, 768))
ATOM = "atomics"                    # the row also runs with "det_reduce" 0
RND = "random"                      # the row also runs the random family
RND_ATOM = "random atomics"         # ... and the random family with "det_reduce" 0
# 256x256 form, forced with "tn256" 1 and "tn256_min_m" 1: (group, M, reserved CUs, expected plan fields, marks).  A plan
# of None = the 256 form declines; form "128" = launch_tn_group does not offer the range to it.
CASES_256 = (
    (((256, 256),), 128, 0, dict(ntiles=1, P=256, empty=254, spare=0, tail_len=0), (RND,)),
    (((256, 256),), 64, 0, dict(ntiles=1, P=256, empty=255, spare=0, longest=1), ()),
    (((128, 128),), 192, 0, dict(ntiles=1, half_outside=1, empty=253), (ATOM, RND, RND_ATOM)),
    (((512, 512),), 320, 0, dict(ntiles=4, P=64, empty=59, spare=0), (RND,)),
    (((768, 384, 1),), 1061, 0, dict(ntiles=6, P=42, empty=26, spare=4, tail_len=0, half_outside=3, rest=37), (ATOM, RND)),
    (((768, 384),), 1088, 24, dict(ntiles=6, P=38, nwg=232, half_outside=3), (ATOM,)),
    (SMALL_LAYER, 1024, 0, dict(ntiles=9, P=28, empty=12), (ATOM, RND)),
    (((768, 1152), (384, 128, 1)), 640, 8, dict(ntiles=17, nwg=248, half_outside=5), (ATOM,)),
    (((2560, 2560),), 320, 0, dict(ntiles=100, P=2, tail_len=1, tail_u=2, span=2, idle=6, tc_min=1, tc_max=1), (ATOM,)),
    (((2304, 2048),), 384, 128, dict(ntiles=72, P=1, nwg=128, tail_len=2, tc_min=1, tc_max=2, idle=8), ()),
    (((2304, 3840),), 512, 0, dict(ntiles=135, P=1, tail_len=3, tail_u=4, tc_min=1, tc_max=2), ()),
    (LAYER_149M, 1408, 128, dict(ntiles=78, tail_len=8, span=3), (ATOM,)),
    (((2304, 3840),), 192, 128, None, ()),
    (((128, 128),), 1, 0, "128", (ATOM, RND)),
    (((128, 128),), 63, 0, "128", (ATOM, RND)),
)
# one row at the DEFAULT switches ("tn256" 1, "tn256_min_m" 8192), exact family
CASE_DEFAULT = (((768, 384),), 8192 + 64 + 37, 0, dict(ntiles=6, P=42, tail_len=1, rest=37, spare=4))
# 128x128 kernel ("tn256" 0): (group, M, expected plan fields, marks)
CASES_128 = (
    (((128, 128),), 1, dict(tiles=1, splits=1, last=1), (RND,)),
    (((128, 128),), 63, dict(tiles=1, splits=1, last=63), (ATOM,)),
    (((128, 128),), 65, dict(tiles=1, splits=1, last=65), (RND, RND_ATOM)),
    (((768, 384),), 300, dict(tiles=18, splits=2, rows=192, last=108), (ATOM, RND)),
    (((768, 384, 1),), 257, dict(last=65), (ATOM, RND)),
    (SMALL_LAYER, 777, dict(tiles=34, splits=4, last=9), (ATOM,)),
    (((128, 128),), 3000, dict(tiles=1, splits=10), ()),
)


def _assert_tables():
    for group, M, res, want, _ in CASES_256:
        plan = dispatch(group, M, 1, 1, res)
        if want is None:
            assert tn256_plan(group, M, res) is None and plan.form == "128" and (M & ~63) >= 64, (group, M)
        elif want == "128":
            assert M < 64 and plan.form == "128" and plan.slabs == 0 and workspace_bytes(group, M) == 0, (group, M)
        else:
            got = {k: getattr(plan, k) for k in want}
            assert plan.form == "256" and got == want, (group, M, res, got, want)
    group, M, res, want = CASE_DEFAULT
    plan = dispatch(group, M, 1, 8192, res)
    assert plan.form == "256" and {k: getattr(plan, k) for k in want} == want, (group, M, vars(plan))
    for group, M, want, _ in CASES_128:
        plan = tn128_plan(group, M)
        assert {k: getattr(plan, k) for k in want} == want, (group, M, vars(plan), want)


_assert_tables()
