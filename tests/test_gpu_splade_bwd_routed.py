"""snx_splade_bwd / snx_splade_bwd_tw against the exact routed float64 reference, per element (bounds and their
derivation: tests/splade_bwd_reference.py).  The backward takes the packed keys as an INPUT, so the tests write the
routing themselves and make every coefficient an exact bf16 value; what remains is fp32 summation order and one bf16
rounding, and a dropped, duplicated or misrouted entry is orders of magnitude outside the bound.  All shapes are small
(T <= 1,301 rows); tests/test_splade_bwd_reference_host.py checks, without a GPU, that the cases hold what their
comments say.  Needs a real MI355X:  pytest -m gpu."""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import splade_bwd_reference as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _seq_lens(n):
    return [(7 * i * i + 3) % 40 + 1 for i in range(n)]


_TW = dict(tokens="spread")
CASES = {
    # the four H / 256 instantiations of every gather (token direction included)
    **{f"H{H}": dict(lens=[5, 70, 33], V=300, H=H, seed=H, **_TW) for H in (256, 512, 768, 1024)},
    # the 8-sequences-at-a-time sweep of the dE / db kernel: one batch, a partial one, a full one, two, three
    **{f"nseq{n}": dict(lens=_seq_lens(n), V=97, H=256, seed=n, **_TW) for n in (1, 7, 8, 9, 17)},
    # more sequences than the 256 threads of the panel gather's item table: two sequences per thread, 38 batches of the sweep
    "nseq300": dict(lens=[i % 3 + 1 for i in range(300)], V=9, H=256, seed=300),
    # 8-row waves and 32-row workgroups of the dE kernel
    **{f"V{V}": dict(lens=[3, 40, 17], V=V, H=256, seed=V) for V in (1, 7, 9)},
    **{f"V{V}": dict(lens=[3, 40, 17], V=V, H=256, seed=V, **_TW) for V in (33, 777)},
    # the bucket kernel's per-wave vocabulary range steps from 64 to 128 and waves fall idle
    **{f"V{V}": dict(lens=[3, 40, 17], V=V, H=256, seed=V, **_TW) for V in (1024, 1025)},
    # 64 panels of 65 terms: every 64-entry chunk of the one-row bucket (about 3,700 entries) straddles a panel end
    "V4100": dict(lens=[40, 3, 17], V=4100, H=256, seed=41, routing=["one_row", "round_robin", "random"], **_TW),
    # packed sequences, max_seqlen above the longest
    "packed": dict(lens=[1, 3, 8, 9, 64, 65, 200], V=333, H=512, seed=7, max_seqlen=256, **_TW),
    # buckets of exactly 63 / 64 / 65 / 128 entries, a bucket of every term, round robin, two sequences without an active entry
    "routing": dict(lens=[130, 20, 9, 12, 6], V=777, H=256, seed=9,
                    routing=["counts", "one_row", "round_robin", "masked", "gzero"]),
    # token direction: coincident and non-coincident entries, masked tokens, one-token sequences
    "tw_mixed": dict(lens=[1, 64, 37, 9, 1], V=211, H=768, seed=13, tokens="spread", coincide=0.5),
    # every token takes one column: 1,301 tokens, two chunks of the counting sort (Hd dyadic: that column's sum is exact)
    "tw_one_col": dict(lens=[600, 500, 1, 200], V=50, H=256, seed=15, tokens="one_col", hd_dyadic=True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    kw = dict(CASES[name])
    ms = kw.pop("max_seqlen", None)
    case = R.make_case(**kw)
    case.max_seqlen = ms or case.max_len
    case.exact_tok = bool(kw.get("hd_dyadic"))
    return case, R.reference_of(case)          # the reference also refuses keys that route outside their sequence


def _run(dev, case, max_seqlen=None, entry="auto"):
    """One call of the C ABI, the way test_splade_bwd makes it -> (dHd, dW, db) on the device; dHd pre-filled with NaN.
    entry: "auto" (snx_splade_bwd_tw when the case has a token direction, else snx_splade_bwd), "plain" (snx_splade_bwd)
    or "tw_null" (snx_splade_bwd_tw with g_tw = NULL)."""
    from snx._lib import check, fn
    from snx.ops import _p, _stream
    ms = max_seqlen or case.max_seqlen
    assert ms >= case.max_len
    T, B, V, H = case.T, case.B, case.V, case.H
    d = lambda a: a.to(dev).contiguous()
    g, keys, Hd, W, cu = d(case.g), d(case.keys), d(case.Hd), d(case.W), d(case.cu)
    dHd = torch.full((T, H), float("nan"), dtype=BF16, device=dev)
    dW, db = d(case.dW0).clone(), d(case.db0).clone()
    scratch = torch.empty(fn("snx_splade_bwd_scratch_bytes")(B, ms, V), dtype=torch.uint8, device=dev)
    if entry == "plain" or (entry == "auto" and case.g_tw is None):
        check(fn("snx_splade_bwd")(_p(g), _p(keys), _p(Hd), _p(W), _p(cu), _p(dHd), _p(dW), _p(db), _p(scratch), T, B, ms,
                                   V, H, _stream()), "snx_splade_bwd")
    else:
        g_tw = None if entry == "tw_null" else d(case.g_tw)
        tkeys = d(case.tkeys)
        tws = torch.empty(fn("snx_splade_tw_scratch_bytes")(T, V), dtype=torch.uint8, device=dev)
        check(fn("snx_splade_bwd_tw")(_p(g), _p(keys), _p(g_tw), _p(tkeys), _p(Hd), _p(W), _p(cu), _p(dHd), _p(dW), _p(db),
                                      _p(scratch), _p(tws), T, B, ms, V, H, _stream()), "snx_splade_bwd_tw")
    torch.cuda.synchronize()
    return dHd, dW, db


def _check(name, out, case, ref):
    ratios = R.check_routed(*out, ref, case.dW0, case.db0, what=name, token_sums_exact=case.exact_tok)
    print(f"{name}: worst err / bound ratio dHd {ratios['dHd']:.3g} dW {ratios['dW']:.3g} db {ratios['db']:.3g}")
    return ratios


def _same_bits(a, b, what, ratios):
    for n, x, y in zip(("dHd", "dW", "db"), a, b):
        xi = x.view(torch.int16) if x.dtype == BF16 else x.view(torch.int32)
        yi = y.view(torch.int16) if y.dtype == BF16 else y.view(torch.int32)
        assert torch.equal(xi, yi), (f"{what}: {n} differs in {int((xi != yi).sum())} elements "
                                     f"(worst err / bound ratio of the default form {ratios})")


@pytest.mark.parametrize("name", list(CASES))
def test_routed_backward_per_element(dev, name):
    case, ref = _case(name)
    _check(name, _run(dev, case), case, ref)


@pytest.mark.parametrize("name", ["routing", "packed", "V4100", "V1025", "tw_mixed", "H1024"])
def test_launch_forms_on_the_same_data(dev, name):
    """The panel gather (default panel count, one panel) and the wave-per-row gather give the same bits; so do the
    vocabulary-ordered buckets with max_seqlen declared as the true maximum and as 1024 (more than 64 KiB of LDS: the
    opt-in); first-come buckets (max_seqlen = 1025) sum in another order and stay inside the bounds."""
    import snx
    case, ref = _case(name)
    base = _run(dev, case)
    ratios = _check(name, base, case, ref)
    panels = snx.config("splade_dh_panels")
    try:
        for p in (0, 1):
            snx.configure(splade_dh_panels=p)
            _same_bits(_run(dev, case), base, f"{name}: splade_dh_panels={p} against {panels}", ratios)
    finally:
        snx.configure(splade_dh_panels=panels)
    assert snx.config("splade_dh_panels") == panels
    for ms in (case.max_len, 1024):
        _same_bits(_run(dev, case, max_seqlen=ms), base, f"{name}: max_seqlen={ms} against {case.max_seqlen}", ratios)
    _check(f"{name}, first-come buckets", _run(dev, case, max_seqlen=1025), case, ref)


@pytest.mark.parametrize("name", ["tw_mixed", "tw_one_col"])
def test_null_token_gradient_is_the_sparse_backward_bit_for_bit(dev, name):
    case, _ = _case(name)
    ref = R.splade_bwd_reference(case.g, case.keys, None, None, case.Hd, case.W, case.cu, case.dW0, case.db0)
    plain = _run(dev, case, entry="plain")
    ratios = R.check_routed(*plain, ref, case.dW0, case.db0, what=f"{name}, snx_splade_bwd")
    print(f"{name}, sparse direction alone: worst err / bound ratio {ratios}")
    _same_bits(_run(dev, case, entry="tw_null"), plain, f"{name}: g_tw = NULL against snx_splade_bwd", ratios)


def test_end_to_end_keys_of_the_forward_with_an_irregular_mask(dev):
    """keys and token keys from decoder_splade_fwd (holes, left padding, one valid row, a fully masked sequence: its keys
    and its token keys are 0xFFFF, value 0 at row / column 0, as include/snx.h states for both forms of the forward), g and
    g_tw built from the decoded logits by the exact-coefficient builder"""
    from snx import ops
    B, S, V, K = 6, 64, 1000, 256
    T = B * S
    gen = torch.Generator().manual_seed(77)
    mask = (torch.rand(B, S, generator=gen) < 0.7).long()
    mask[1, : S // 3] = 0
    mask[1, S // 3:] = 1
    mask[2] = 0
    mask[2, S // 2] = 1
    mask[3] = 0
    Hd = torch.randn(T, K, generator=gen).to(BF16)
    W = (torch.randn(V, K, generator=gen) * 0.05).to(BF16)
    bias = torch.randn(V, generator=gen) * 0.3
    cu = torch.arange(B + 1, dtype=torch.int32) * S
    _, keys, _, tkeys = ops.decoder_splade_fwd_tw(Hd.to(dev), W.to(dev), bias.to(dev), cu.to(dev), mask.reshape(-1).to(dev), S)
    keys, tkeys = keys.cpu(), tkeys.cpu()
    assert (keys[3] == 0xFFFF).all() and (tkeys.view(B, S)[3] == 0xFFFF).all()
    x, _ = R.decode_keys(keys)
    g, _ = R.build_exact_g(x, gen)
    assert (g[3] != 0).sum() > V // 2                       # x = 0 with g != 0, on the key value 0 of the forward
    g_tw = R.build_exact_g_tw(g, keys, tkeys, cu, gen)
    case = SimpleNamespace(lens=None, cu=cu, B=B, T=T, V=V, H=K, max_len=S, max_seqlen=S, g=g, keys=keys, g_tw=g_tw,
                             tkeys=tkeys, Hd=Hd, W=W, dW0=torch.randn(V, K, generator=gen), db0=torch.randn(V, generator=gen),
                             exact_tok=False)
    ref = R.reference_of(case)
    assert (ref.row_entries.view(B, S)[mask == 0] == 0).all() and (ref.row_entries > 0).sum() > T // 3
    _check("end to end", _run(dev, case), case, ref)
