"""Host-side proof of tests/gemm_reference.py (no GPU): the reference admits what the kernels' cast points can produce and
rejects what they cannot.

a. Conformance.  simulate() restates the kernels' cast points on the CPU -- fp32 accumulation of the exact products in
   32-wide chunks, ascending and again with k shuffled, bf16 by torch's own cast (independent of bf16_round), the epilogues
   in numpy float32, gelu_f / gelu_grad_f by the float32 emulation gelu_emul -- and must fall inside the acceptance sets
   of every case of the three tables, every legal epilogue, both families (workload-sized cases: SAMPLE_ROWS rows spread
   over the whole height; a row's results depend on that row alone).  gelu_emul with its reciprocal and exponential moved
   by -1, 0, +1 ulp stays inside the tabulated intervals for all finite bf16 inputs, and the erfc fit's error is re-measured
   in float64 against the figure csrc/common.h states.
b. Planted faults.  FAULTS names, per fault, the families that must reject it; the test asserts exactly that set.
c. Width of the acceptance sets, from the reference alone.  Exact family: every store, residual and RoPE element has ONE
   admissible value, and the sums hit round-to-even ties.  Random family: share of store elements that admit more than
   two adjacent bf16 values, per K, over the committed cases (computed by this file; no kernel involved):
       K     64      128     192     256     320     384     768     1152
       worst 0.569 % 1.562 % 2.045 % 3.423 % 4.651 % 6.090 % 16.495 % 29.845 %
   (the large cases, where the share is not the noise of a few hundred elements: 0.46 % at K = 64, 1.2 % at K = 128; it
   grows with K because gamma_n does: n = K + 8)
   cap: 2 % up to K = 128; above, WIDE_CAP[K] = the worst share above plus a quarter of it.
d. Coverage.  Every class of the issue's table occurs for every epilogue that admits it, read off the case tables
   through nt256_plan and pipe_plan, whose own arithmetic is checked to deal every 64-row unit exactly once.
"""
import numpy as np
import pytest
import torch

from tests import gemm_reference as R

SAMPLE_ROWS = 192
WIDE_CAP = {64: 0.02, 128: 0.02, 192: 0.02556, 256: 0.04279, 320: 0.05814, 384: 0.07613, 768: 0.20619, 1152: 0.37306}
ALL_CASES = ([("128", M, N, K, 0, f) for M, N, K, fams in R.CASES_128 for f in fams]
             + [("256", M, N, K, res, f) for M, N, K, res, _ in R.CASES_256 for f in R.B_]
             + [("pipe", M, N, 768, res, "exact") for M, N, res, *_ in R.CASES_PIPE])


def _case(form, M, N, K, fam):
    c = R.build_case(fam, M, N, K)
    if M > 2 * SAMPLE_ROWS:
        rows = np.unique(np.concatenate([np.arange(64), np.linspace(0, M - 1, SAMPLE_ROWS - 64).astype(np.int64)]))
        c = R.subcase(c, rows)
    return c


# ----------------------------------------------------------------------------- the simulation
def simulate(c, entry, rope_cols=None, shuffle=False, fault=None):
    """{output name: guarded buffer} of one entry point, with the kernels' cast points and optionally one planted fault"""
    f32 = np.float32
    M, N, K = c.M, c.N, c.K
    A, B = c.A.float(), c.B.float()
    ks = torch.arange(K - 64 if fault == "drop_last_ktile" else K)
    if shuffle:
        ks = ks[torch.randperm(len(ks), generator=torch.Generator().manual_seed(K))]
    acc = torch.zeros(M, N)
    for k0 in range(0, len(ks), 32):
        idx = ks[k0:k0 + 32]
        acc += A[:, idx] @ B[:, idx].t()
    if fault == "stale_ktile":                                  # rows 0..63: K-tile 1 taken from the stage that still holds tile 0
        r = slice(0, min(64, M))
        acc[r] += A[r, 0:64] @ B[:, 0:64].t() - A[r, 64:128] @ B[:, 64:128].t()
    if fault == "truncate":
        cc = R.bf16_trunc(acc.double().numpy())
    else:
        cc = R.to_np(acc.to(R.BF16))
    out = {}

    def put(name, val, dtype=R.BF16):
        buf, mid = R.guarded(M, val.shape[1], dtype)
        mid.copy_(torch.from_numpy(np.ascontiguousarray(val)).to(dtype))
        out[name] = buf
        return buf

    def gelu(a):
        if fault == "tanh_gelu":
            a32 = a.astype(f32)
            g = (f32(0.5) * a32 * (f32(1) + np.tanh(f32(0.7978845608) * (a32 + f32(0.044715) * a32 * a32 * a32)))).astype(np.float64)
            return g, R.gelu_emul(a)[1]
        g, d = R.gelu_emul(a)
        return g, (d * 1.01 if fault == "gelu_grad_1pct" else d)

    if entry == "store":
        if fault == "narrow_shift4":
            cc[M // 2] = np.roll(cc[M // 2], 4)
        buf = put("C", cc)
        if fault == "row_past_m":
            buf[R.GUARD_ROWS + M] = buf[R.GUARD_ROWS + M - 1]
        if fault == "chunk_unwritten":
            R._raw(buf)[R.GUARD_ROWS + M // 2, :8] = R.SENT_BF16
    elif entry == "resid":
        h = c.Hin.numpy()
        if fault == "resid_before_round":
            put("Hout", (h + acc.numpy()).astype(np.float64), torch.float32)
        else:
            put("Hout", (h + cc.astype(f32)).astype(np.float64), torch.float32)
    elif entry in ("rope", "rope_rows"):
        pos = c.pos.numpy().astype(np.int64).copy()
        if fault == "clamped_pos":
            pos[0] = pos[M - 1]
        cs = c.tab.numpy()[pos]
        cos, sin = cs[:, None, :, 0], cs[:, None, :, 1]
        if fault == "sin_sign":
            sin = -sin
        rc = rope_cols + 64 if fault == "rope_past_cols" else rope_cols
        res = cc.copy()
        if rc:
            v = cc[:, :rc].astype(f32).reshape(M, rc // 64, 2, 32)
            if fault == "pair_16":                              # (d, d + 16) inside each half instead of (d, d + 32)
                v = v.reshape(M, rc // 64, 2, 2, 16).transpose(0, 1, 3, 2, 4).reshape(M, rc // 64, 2, 32)
            x1, x2 = v[:, :, 0], v[:, :, 1]
            lo, hi = x1 * cos - x2 * sin, x2 * cos + x1 * sin
            r = np.stack((lo, hi), axis=2)
            if fault == "pair_16":
                r = r.reshape(M, rc // 64, 2, 2, 16).transpose(0, 1, 3, 2, 4)
            res[:, :rc] = R.to_np(torch.from_numpy(np.ascontiguousarray(r.reshape(M, rc))).to(R.BF16))
        put("C", res)
    elif entry == "geglu_fwd":
        v = cc.reshape(M, N // 64, 2, 32)
        a, g = (v[:, :, 1], v[:, :, 0]) if fault == "halves_swapped" else (v[:, :, 0], v[:, :, 1])
        G = R.to_np(torch.from_numpy(gelu(a)[0]).float().to(R.BF16))
        put("U", cc)
        put("Y", (G * g).reshape(M, N // 2))
    else:
        u = R.to_np(c.U).reshape(M, N // 32, 2, 32)
        a, g = (u[:, :, 1], u[:, :, 0]) if fault == "halves_swapped" else (u[:, :, 0], u[:, :, 1])
        dy = cc.reshape(M, N // 32, 32)
        ge, gr = gelu(a)
        G = R.to_np(torch.from_numpy(ge).float().to(R.BF16))
        t = dy * g
        if fault != "dyg_not_rounded":
            t = R.to_np(torch.from_numpy(t).float().to(R.BF16))
        da = (t.astype(f32) * gr.astype(f32)).astype(np.float64)
        put("dU", np.stack((da, dy * G), axis=2).reshape(M, 2 * N))
    return out


def _check(c, entry, outs, rope_cols=None, what=""):
    exp = R.expected(c, entry, rope_cols)
    assert set(exp) == set(outs)
    return {k: R.check_guarded(outs[k], exp[k], f"{what} {entry} {k}") for k in exp}


# ----------------------------------------------------------------------------- roundings and the gelu table
def test_bf16_round_is_exact_including_ties():
    f = float.fromhex
    x = np.array([1.0, f("0x1.01p0"), f("0x1.03p0"), f("0x1.0100000000001p0"), f("0x1.00fffffffffffp0"), -f("0x1.01p0"),
                  f("0x1.ffp3"), 0.0, -0.0, f("0x1.fe8p-100"), f("0x1.0100001p0"), f("0x1.7fp5")])
    want = np.array([1.0, 1.0, f("0x1.04p0"), f("0x1.02p0"), 1.0, -1.0, 16.0, 0.0, -0.0, f("0x1.fep-100"), f("0x1.02p0"),
                     f("0x1.80p5")])
    assert np.array_equal(R.bf16_round(x), want)
    # 0x1.0100001p0 lies above the tie; fp32 (24 bits) would first round it ONTO the tie 0x1.01p0 and then down to even
    assert float(torch.tensor(f("0x1.0100000001p0"), dtype=torch.float64).float().to(R.BF16)) == 1.0
    assert R.bf16_round(np.array([f("0x1.0100000001p0")]))[0] == f("0x1.02p0")
    # every fp32 value torch can round: same result as torch's own RNE cast, ties of both parities included
    g = torch.Generator().manual_seed(1)
    v = torch.cat([torch.randn(200000, generator=g) * 10 ** torch.randint(-8, 9, (200000,), generator=g).float(),
                   (torch.arange(-70000, 70000).float() + 0.5) / 128.0])
    assert np.array_equal(R.bf16_round(v.double().numpy()), v.to(R.BF16).double().numpy())
    _, every = R.all_bf16()
    keep = np.abs(every) >= R.BF16_MIN
    assert np.array_equal(R.bf16_round(every[keep]), every[keep])
    o = R.bf16_ord(np.sort(every[keep]))
    assert bool(np.all(np.diff(o) >= 0)) and int((np.diff(o) == 0).sum()) == 0
    with pytest.raises(AssertionError):
        R.bf16_round(np.array([1e-40]))


def test_gelu_fit_error_against_what_common_h_states():
    """csrc/common.h: "3.5e-9 absolute error before fp32 rounding".  In float64 that figure is met by h = erfc / 2 with the
    decimal constants (to its two digits); with the constants rounded to fp32, as the kernel holds them, the error of h is
    2.2e-8 at x = 0.  The table uses the per-input error of the formula with the fp32 constants, not the stated figure."""
    from scipy.special import erfc
    _, x = R.all_bf16()
    true_h = 0.5 * erfc(np.abs(x) / np.sqrt(2.0))
    dec = np.abs(R.gelu_fit_f64(x, R.POLY_DEC, 0.23164189, -0.72134752)[0] - true_h).max()
    f32 = np.abs(R.gelu_fit_f64(x)[0] - true_h).max()
    print(f"erfc / 2 fit in float64 over all finite bf16 inputs: decimal constants {dec:.3e}, fp32 constants {f32:.3e}")
    assert dec <= R.FIT * 1.05 and f32 <= 7 * R.FIT


def test_gelu_emulation_stays_inside_the_table_for_all_bf16_inputs():
    tab = R.gelu_table()
    _, x = R.all_bf16()
    o = R.bf16_ord(x) + 0x7F7F
    worst = [0.0, 0.0]
    for drcp in (-1, 0, 1):
        for dexp in (-1, 0, 1):
            g, d = R.gelu_emul(x, drcp, dexp)
            G = R.bf16_round(np.where(np.abs(g) < R.BF16_MIN, 0.0, g))
            assert bool(np.all((G >= tab.g_lo[o]) & (G <= tab.g_hi[o]))), (drcp, dexp)
            assert bool(np.all((d >= tab.d_lo[o]) & (d <= tab.d_hi[o]))), (drcp, dexp)
            nz = tab.err_g[o] > 0
            worst[0] = max(worst[0], float((np.abs(g - tab.gelu[o])[nz] / tab.err_g[o][nz]).max()))
            worst[1] = max(worst[1], float((np.abs(d - tab.grad[o]) / tab.err_d[o]).max()))
    print(f"gelu_emul +-1 ulp: worst error / half-width gelu {worst[0]:.3f}, gelu' {worst[1]:.3f}")
    # the table decides: in GELU's interesting range almost every input has ONE admissible G
    near = np.abs(x) <= 4.0
    one = R.widths(tab.g_lo[o], tab.g_hi[o])[near] == 1
    assert one.mean() > 0.99
    # and it is not so wide that tanh-GELU or a 1 % error in GELU' would fit
    a = x[(np.abs(x) > 0.5) & (np.abs(x) < 3.0)]
    oa = R.bf16_ord(a) + 0x7F7F
    assert bool(np.all(tab.err_d[oa] < 1e-5)) and bool(np.all(tab.err_g[oa] < 1e-5))


# ----------------------------------------------------------------------------- launch arithmetic
@pytest.mark.parametrize("M,N,K,res,classes", R.CASES_256)
def test_nt256_plan_deals_every_unit_once_and_the_table_names_its_class(M, N, K, res, classes):
    p = R.nt256_plan(M, N, K, res)
    seen = np.zeros((4 * p.tm, p.tn), dtype=np.int64)
    for wg, mine in p.tiles.items():
        assert 0 <= wg < p.nwg
        for m0, n0, u in mine:
            assert m0 % 64 == 0 and n0 % 256 == 0 and 1 <= u <= 4
            seen[m0 // 64:m0 // 64 + u, n0 // 256] += 1
    assert bool((seen == 1).all()), "a 64-row unit dealt twice or never"
    assert set(classes) <= p.classes, (sorted(p.classes), classes)
    assert M * K * 2 < 2 ** 32 and N * K * 2 < 2 ** 32 and N % 64 == 0          # what snx_launch_nt256 takes


def test_tile_order_is_a_bijection():
    for tm, tn, cg in ((17, 2, 2), (9, 5, 5), (24, 3, 2), (1, 1, 1), (20, 8, 3), (7, 9, 4)):
        order = (tm, tn, R.cdiv(tm, 8), cg)
        assert sorted(R.tile_of(order, p) for p in range(tm * tn)) == [(m, n) for m in range(tm) for n in range(tn)]


@pytest.mark.parametrize("M,N,res,nwg,empty,most", R.CASES_PIPE)
def test_pipe_plan_matches_the_table(M, N, res, nwg, empty, most):
    p = R.pipe_plan(M, N, 768, res)
    assert (p.nwg, p.empty, p.most) == (nwg, empty, most) and sum(p.counts) == p.ntiles
    assert R.pipe_plan(M + 64, N, 768, res) is None and R.pipe_plan(M, N, 704, res) is None


def test_coverage_of_the_class_table():
    mid = {"resid", "geglu_bwd"}
    seen = {e: set() for e in R.ENTRIES}
    for M, N, K, fams in R.CASES_128:
        nk = K // 64
        for e in R.legal_entries(N):
            for fam in fams:
                form = ("nk<5" if nk < 5 else "nk=5" if nk == 5 else "nk>=6") if e in mid else f"nk{min(nk, 3)}"
                seen[e] |= {(fam, form), (fam, f"nk {nk}"), (fam, "narrow" if N % 8 else "wide"), (fam, f"M {M}"), (fam, f"N {N}")}
                if N % 64 and not N % 8:
                    seen[e].add((fam, "partial span"))
                if R.column_group(M, N, K, 128, 1.8e6) < R.cdiv(N, 128):
                    seen[e].add((fam, "column groups"))
    for fam in R.B_:
        for e in R.ENTRIES:
            want = {"nk<5", "nk=5", "nk>=6"} if e in mid else {"nk1", "nk2", "nk3"}
            want |= {"wide", "column groups", "M 1", "M 65", "M 129", "M 200"} | {f"nk {n}" for n in (1, 2, 3, 4, 5, 6, 12)}
            if e in ("store", "resid"):
                want |= {"narrow", "partial span"} | {f"N {n}" for n in (4, 12, 68, 132, 8, 72, 200)}
            if e == "geglu_bwd":
                want |= {f"N {n}" for n in (32, 96, 160)}
            want |= {f"N {n}" for n in (64, 192, 384, 2304)}
            missing = {w for w in want if (fam, w) not in seen[e]}
            assert not missing, (fam, e, sorted(missing))
    assert any(K == 2304 for _, _, K, f in R.CASES_128 if "exact" in f) and any(K == 1152 for _, _, K, f in R.CASES_128 if "random" in f)
    got = set()
    for M, N, K, res, classes in R.CASES_256:
        got |= set(classes)
        assert R.legal_entries(N, "256") == R.ENTRIES                 # all six entries run on every 256x256 case
    assert {"single ragged tile", "fewer tiles than workgroups, tile order", "tile order", "column runs",
            "one round, nothing left", "rounds plus leftovers", "two rounds", "nk 1", "nk 2", "u 1", "u 2", "u 3", "u 4",
            "N % 256 = 64", "N % 256 = 128", "N % 256 = 192"} <= got
    assert {(e, m) for *_, e, m in R.CASES_PIPE} >= {(7, 1), (5, 1), (0, 1), (0, 2), (0, 3)}


# ----------------------------------------------------------------------------- a. conformance
@pytest.mark.parametrize("form,M,N,K,res,fam", ALL_CASES)
def test_simulated_cast_points_fall_inside_the_acceptance_sets(form, M, N, K, res, fam):
    c = _case(form, M, N, K, fam)
    entries = ("geglu_bwd",) if form == "pipe" else R.legal_entries(N, form)
    for e in entries:
        rcs = (R.rope_cols_of(N) if form == "128" else [N - 64]) if e in ("rope", "rope_rows") else [None]
        for rc in rcs:
            for shuffle in (False, True):
                st = _check(c, e, simulate(c, e, rc, shuffle), rc, f"{fam} {M}x{N}x{K} rope_cols {rc} shuffled {shuffle}")
                if fam == "exact" and e in ("store", "resid", "rope", "rope_rows"):
                    assert all(s.single == 1.0 for s in st.values())


# ----------------------------------------------------------------------------- b. planted faults
# fault -> (entry, shape, rope_cols, families that must reject it).  truncation and the unrounded residual need inexact
# sums or ties: both families have them; the exact family's small integers hide nothing else either.
FAULTS = {
    "drop_last_ktile": ("store", (200, 192, 320), None, R.B_),
    "stale_ktile": ("store", (200, 192, 320), None, R.B_),
    "truncate": ("store", (200, 192, 320), None, R.B_),
    "resid_before_round": ("resid", (200, 192, 320), None, R.B_),
    "sin_sign": ("rope", (200, 192, 320), 128, R.B_),
    "pair_16": ("rope", (200, 192, 320), 128, R.B_),
    "rope_past_cols": ("rope", (200, 192, 320), 128, R.B_),
    "clamped_pos": ("rope", (200, 192, 320), 128, R.B_),
    "halves_swapped": ("geglu_fwd", (200, 192, 320), None, R.B_),
    "tanh_gelu": ("geglu_fwd", (200, 192, 320), None, R.B_),
    "gelu_grad_1pct": ("geglu_bwd", (200, 192, 320), None, R.B_),
    "dyg_not_rounded": ("geglu_bwd", (200, 192, 320), None, R.B_),
    "row_past_m": ("store", (200, 192, 320), None, R.B_),
    "chunk_unwritten": ("store", (200, 192, 320), None, R.B_),
    "narrow_shift4": ("store", (65, 12, 128), None, R.B_),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_rejected_by_the_named_families(fault):
    entry, (M, N, K), rc, named = FAULTS[fault]
    caught = []
    for fam in R.B_:
        c = R.build_case(fam, M, N, K)
        _check(c, entry, simulate(c, entry, rc), rc, "clean")     # the same run without the fault passes
        try:
            _check(c, entry, simulate(c, entry, rc, fault=fault), rc, fault)
        except AssertionError as err:
            caught.append(fam)
            print(f"{fault} / {fam}: {str(err)[:160]}")
    assert tuple(caught) == tuple(named), (fault, caught)
    if fault == "halves_swapped":                                # the backward reads the saved u the same way
        c = R.build_case("exact", M, N, K)
        with pytest.raises(AssertionError):
            _check(c, "geglu_bwd", simulate(c, "geglu_bwd", fault=fault), None, fault)


# ----------------------------------------------------------------------------- c. widths
@pytest.mark.parametrize("form,M,N,K,res,fam", ALL_CASES)
def test_width_of_the_acceptance_sets(form, M, N, K, res, fam):
    c = _case(form, M, N, K, fam)
    w = R.widths(c.c_lo, c.c_hi)
    if fam == "exact":
        assert bool((w == 1).all())
        lo, hi, _ = R.ep_resid(c.c_lo, c.c_hi, c.Hin.numpy())
        assert np.array_equal(lo, hi)
        if N % 64 == 0:
            lo, hi = R.ep_rope(c.c_lo, c.c_hi, c.tab, c.pos, N)
            assert np.array_equal(lo, hi)
        if K >= 128 and M * N >= 4096:                               # round-to-even ties really occur
            scaled = np.abs(c.S) / 2.0 ** (np.floor(np.log2(np.maximum(np.abs(c.S), 2.0 ** -20))) - 8)
            ties = (scaled % 1.0) == 0.5
            assert ties.mean() > 0.01, ties.mean()
    else:
        share = float((w > 2).mean())
        print(f"random {M}x{N}x{K}: {share:.3%} of store elements admit more than two values")
        assert share <= WIDE_CAP[K], (share, WIDE_CAP[K])
