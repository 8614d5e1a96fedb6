"""The NT GEMM family against the float64 reference of tests/gemm_reference.py, per element: all six entry points
(snx_gemm_nt_bf16, _resid, _rope, _rope_rows, _geglu_fwd, _geglu_bwd) in the three kernel forms -- the 128x128 kernel
(nt256 off, nt_pipe 0), the 256x256 persistent kernel forced onto every eligible shape (snx_nt256_configure(2, 1)) and the
pipelined GeGLU backward (nt_pipe 2 and 1, nt_pipe_min_m 1) -- in both input families.  The C entry points are called as
the snx.ops wrappers call them, but into guarded buffers: 128 guard rows of a NaN sentinel before and after every output,
the output itself pre-filled with it.  Every switch is restored on the way out of the block that set it (Switches).

Per run: guards untouched, every element written and finite and inside its acceptance set; columns >= rope_cols are
c's own set; rope and rope_rows give the same bits; a second run gives the same bits.  In the exact family store,
residual, RoPE and u have ONE admissible value: those runs are bit-for-bit checks with no assumption about the MFMA.
tests/test_gemm_reference_host.py proves on the CPU that the reference admits the kernels' cast points and rejects the
planted faults, and that the case tables reach every class (through nt256_plan / pipe_plan, asserted again here).

Which case is there for which seam: gemm_reference.CASES_128 / CASES_256 / CASES_PIPE and their comments.  Read from
gemm_nt256.hip before the table was committed: a short tile of u units keeps the whole tile's LDS image (DMA source rows
remapped, rows past 32 u and past M re-read a valid row), stores are guarded by row < M and by the wave-uniform
col0 < N, so every shape with M >= 1, N % 64 == 0, K % 64 == 0 is inside what the kernel supports -- (200, 192, 128) is
four one-unit tiles on four workgroups, 252 workgroups return at once.

The chain test runs Wqkv + RoPE -> Wo + residual -> Wi + GeGLU forward -> Wo backward + GeGLU' on 200 rows (H = 256,
I = 384), each stage fed the previous KERNEL's output and judged against the reference evaluated at those inputs.

Measured on an MI355X when this file was added (kernels of commit f602ce6): 187 tests, every element of every output
inside its acceptance set, every exact-family store, residual, RoPE and u element equal to the reference bit for bit in
all three forms, rope = rope_rows and run = rerun everywhere; the shares per form and epilogue stand in the docstring
of tests/gemm_reference.py.  The whole file takes 70 s, the slowest test 2.8 s.
"""
import functools

import pytest
import torch

from tests import gemm_reference as R

pytestmark = pytest.mark.gpu
SWITCHES = ("nt256", "nt256_min_m", "nt_pipe", "nt_pipe_min_m")
FORMS = {"128": dict(nt256=0, nt_pipe=0), "256": dict(nt256=2, nt256_min_m=1, nt_pipe=0),
         "pipe2": dict(nt256=0, nt_pipe=2, nt_pipe_min_m=1), "pipe1": dict(nt256=0, nt_pipe=1, nt_pipe_min_m=1)}
OUT_DTYPE = {"C": R.BF16, "Hout": torch.float32, "U": R.BF16, "Y": R.BF16, "dU": R.BF16}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=2)
def _case(family, M, N, K):
    return R.build_case(family, M, N, K, theta=(10000.0, 160000.0)[(M + N // 64) % 2])


@functools.lru_cache(maxsize=2)
def _device_inputs(family, M, N, K):
    c = _case(family, M, N, K)
    d = {k: getattr(c, k).cuda() for k in ("A", "B", "Hin", "U", "pos", "tab")}
    d["rows"] = d["tab"][d["pos"].long()].contiguous()            # what snx_rope_rows resolves: tab[pos], [M, 32, 2]
    return d


class Switches:
    """one kernel form (and a CU reservation) for the duration of a block; everything back in place afterwards"""

    def __init__(self, form, reserved=0):
        self.form, self.reserved = form, reserved

    def __enter__(self):
        import snx
        from snx._lib import fn
        self.saved = {k: snx.config(k) for k in SWITCHES}
        self.saved_reserved = fn("snx_get_reserved_cus")()
        try:
            f = FORMS[self.form]
            if "nt256" in f:
                assert fn("snx_nt256_configure")(f["nt256"], f.get("nt256_min_m", 0)) == 0
            snx.configure(**{k: v for k, v in f.items() if k.startswith("nt_pipe")})
            assert fn("snx_set_reserved_cus")(self.reserved) == 0
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        import snx
        from snx._lib import fn
        fn("snx_set_reserved_cus")(self.saved_reserved)
        fn("snx_nt256_configure")(self.saved["nt256"], self.saved["nt256_min_m"])
        snx.configure(**self.saved)
        return False


def _launch(entry, d, M, N, K, rope_cols=None):
    """one entry point into fresh guarded buffers, as snx.ops calls it -> {output name: guarded buffer on the device}"""
    from snx._lib import call
    from snx.ops import _p, _stream
    dev = d["A"].device
    A, B = _p(d["A"]), _p(d["B"])
    shapes = {"store": {"C": N}, "resid": {"Hout": N}, "rope": {"C": N}, "rope_rows": {"C": N},
              "geglu_fwd": {"U": N, "Y": N // 2}, "geglu_bwd": {"dU": 2 * N}}[entry]
    bufs = {k: R.guarded(M, cols, OUT_DTYPE[k], dev) for k, cols in shapes.items()}
    o = {k: _p(v[1]) for k, v in bufs.items()}
    if entry == "store":
        call("snx_gemm_nt_bf16", A, B, o["C"], M, N, K, _stream())
    elif entry == "resid":
        call("snx_gemm_nt_resid", A, B, _p(d["Hin"]), o["Hout"], M, N, K, _stream())
    elif entry == "rope":
        call("snx_gemm_nt_rope", A, B, o["C"], _p(d["tab"]), _p(d["pos"]), rope_cols, M, N, K, _stream())
    elif entry == "rope_rows":
        call("snx_gemm_nt_rope_rows", A, B, o["C"], _p(d["tab"]), _p(d["pos"]), _p(d["rows"]), rope_cols, M, N, K, _stream())
    elif entry == "geglu_fwd":
        call("snx_gemm_nt_geglu_fwd", A, B, o["U"], o["Y"], M, N, K, _stream())
    else:
        call("snx_gemm_nt_geglu_bwd", A, B, _p(d["U"]), o["dU"], M, N, K, _stream())
    return {k: v[0] for k, v in bufs.items()}


class Tally:
    def __init__(self):
        self.n = self.one = self.two = self.low = self.wide = 0

    def add(self, st):
        self.n += st.n
        self.one += st.single * st.n
        self.two += st.two * st.n
        self.low += st.two_lo * st.two * st.n
        self.wide += st.wide * st.n

    def __str__(self):
        return (f"{self.n} elements, one {self.one / self.n:.3%}, two {self.two / self.n:.3%} "
                f"(low {self.low / max(self.two, 1):.1%}), wider {self.wide / self.n:.3%}"
                f" | {self.n} {self.one:.0f} {self.two:.0f} {self.low:.0f}")


def _run_and_check(c, d, entry, rope_cols, what, tally, again=True):
    """run, check against the reference, run again for the same bits; returns the raw bits of the outputs"""
    M, N, K = c.M, c.N, c.K
    outs = _launch(entry, d, M, N, K, rope_cols)
    twice = _launch(entry, d, M, N, K, rope_cols) if again else None
    torch.cuda.synchronize()
    exp = R.expected(c, entry, rope_cols)
    assert set(exp) == set(outs)
    for k, buf in outs.items():
        st = R.check_guarded(buf.cpu(), exp[k], f"{what} {entry} {k}")
        tally.add(st)
        if c.family == "exact" and (entry in ("store", "resid", "rope", "rope_rows") or k == "U"):
            assert st.single == 1.0                          # pinned to one value: this was a bit-for-bit check
        if again:
            assert torch.equal(R._raw(buf), R._raw(twice[k])), f"{what} {entry} {k}: a second run gave other bits"
    return outs


def _all_entries(c, d, entries, rope_cols_list, what):
    for e in entries:
        tally = Tally()
        if e == "rope_rows":
            continue
        if e != "rope":
            _run_and_check(c, d, e, None, what, tally)
        plain = _launch("store", d, c.M, c.N, c.K)["C"] if e == "rope" else None
        for rc in rope_cols_list if e == "rope" else []:
            a = _run_and_check(c, d, "rope", rc, f"{what} rope_cols {rc}", tally)
            assert torch.equal(R._raw(a["C"])[:, rc:], R._raw(plain)[:, rc:]), f"{what} rope_cols {rc}: columns >= rope_cols are not c"
            b = _run_and_check(c, d, "rope_rows", rc, f"{what} rope_cols {rc}", tally, again=False)
            assert torch.equal(R._raw(a["C"]), R._raw(b["C"])), f"{what} rope_cols {rc}: rope and rope_rows differ"
        print(f"{what} {e}: {tally}")


@pytest.mark.parametrize("M,N,K,family", [(M, N, K, f) for M, N, K, fams in R.CASES_128 for f in fams])
def test_128_kernel_per_element(dev, M, N, K, family):
    c, d = _case(family, M, N, K), _device_inputs(family, M, N, K)
    with Switches("128"):
        _all_entries(c, d, R.legal_entries(N), R.rope_cols_of(N) if N % 64 == 0 else [], f"128x128 {family} {M}x{N}x{K}")


@pytest.mark.parametrize("entry", R.ENTRIES[:2] + R.ENTRIES[2:3] + R.ENTRIES[4:])
@pytest.mark.parametrize("M,N,K,reserved,classes,family",
                         [(*case, f) for case in R.CASES_256 for f in R.B_])
def test_256_kernel_per_element(dev, M, N, K, reserved, classes, family, entry):
    from snx._lib import fn
    plan = R.nt256_plan(M, N, K, reserved)
    assert set(classes) <= plan.classes, (sorted(plan.classes), classes)
    c, d = _case(family, M, N, K), _device_inputs(family, M, N, K)
    rc = (N - 64, 64, N, 0)[(M + reserved) % 4]
    with Switches("256", reserved):
        assert fn("snx_get_reserved_cus")() == 256 - plan.nwg
        _all_entries(c, d, (entry, "rope_rows") if entry == "rope" else (entry,), [rc, N - 64] if M < 3000 else [rc],
                     f"256x256 {family} {M}x{N}x{K} reserved {reserved}")


@pytest.mark.parametrize("form", ["pipe2", "pipe1"])
@pytest.mark.parametrize("M,N,reserved,nwg,empty,most", R.CASES_PIPE)
def test_pipelined_geglu_backward_per_element(dev, M, N, reserved, nwg, empty, most, form):
    p = R.pipe_plan(M, N, 768, reserved)
    assert (p.nwg, p.empty, p.most) == (nwg, empty, most)
    c, d = _case("exact", M, N, 768), _device_inputs("exact", M, N, 768)
    with Switches(form, reserved):
        _all_entries(c, d, ("geglu_bwd",), [], f"pipelined ({form}) exact {M}x{N}x768 reserved {reserved}")


def test_pipelined_geglu_backward_random_family(dev):
    for M, N in ((384, 384), (1024, 512)):
        c, d = _case("random", M, N, 768), _device_inputs("random", M, N, 768)
        assert R.pipe_plan(M, N, 768) is not None
        for form in ("pipe2", "pipe1"):
            with Switches(form):
                _all_entries(c, d, ("geglu_bwd",), [], f"pipelined ({form}) random {M}x{N}x768")


@pytest.mark.parametrize("form", ["128", "256"])
def test_chain_of_a_layer(dev, form):
    """Wqkv + RoPE -> Wo + residual -> Wi + GeGLU forward -> Wo backward + GeGLU', each stage on the previous kernel's output"""
    T, H, I = 200, 256, 384
    g = torch.Generator().manual_seed(5)
    bf = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(R.BF16)      # noqa: E731
    x, wqkv, wo, wi, wob = bf(T, H), bf(3 * H, H, scale=0.05), bf(H, H, scale=0.05), bf(2 * I, H, scale=0.05), bf(I, H, scale=0.05)
    hin = torch.randn(T, H, generator=g)
    pos = torch.randint(0, R.MAX_POS, (T,), generator=g, dtype=torch.int32)
    pos[0], pos[T // 2] = R.MAX_POS - 1, 0
    tally = Tally()

    def stage(entry, c, rope_cols=None):
        d = {k: getattr(c, k).cuda() for k in ("A", "B", "Hin", "U", "pos", "tab") if getattr(c, k) is not None}
        outs = _run_and_check(c, d, entry, rope_cols, f"chain ({form}) {entry}", tally)
        return {k: v[R.GUARD_ROWS:R.GUARD_ROWS + T].cpu() for k, v in outs.items()}

    with Switches(form):
        qkv = stage("rope", R.case_of(x, wqkv, pos=pos, theta=160000.0), 2 * H)["C"]
        hout = stage("resid", R.case_of(qkv[:, 2 * H:].contiguous(), wo, Hin=hin))["Hout"]
        fwd = stage("geglu_fwd", R.case_of(hout.to(R.BF16), wi))
        stage("geglu_bwd", R.case_of(hout.to(R.BF16), wob, U=fwd["U"]))
    print(f"chain ({form}): {tally}")
