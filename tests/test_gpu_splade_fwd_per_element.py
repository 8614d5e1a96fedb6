"""The fused decoder GEMM + SPLADE tail forward against the exact host reference (tests/splade_fwd_reference.py), per
element, in BOTH kernel forms -- the 128x128 kernel (snx.configure(dec256=0)) and the 256x192 persistent kernel forced
onto tiny batches (dec256=1, dec256_min_t=1) -- and through all three entry forms: snx_decoder_splade_fwd,
snx_decoder_splade_fwd_rec with token_keys, snx_decoder_splade_fwd_flags with SNX_FWD_NO_TOKEN_WEIGHTS and only
snx_splade_head_scratch_bytes_notw(T) bytes of scratch.  Every output starts as a sentinel (NaN, 0x5A5A5A5A, scratch
0xA5 with a guard zone behind it); under NO_TOKEN_WEIGHTS token_weights and token_keys must come back untouched.  That
the asked-for form really ran is read off the scratch buffer: the 256x192 form writes its row tables behind the row
maxima, the 128x128 kernel never touches that region.

Exact class: keys and token_keys equal the reference BIT FOR BIT, sparse and token_weights are the float64 log1p of the
reported bits within 2 fp32 ulp (exact zeros where the bits are 0), and the outputs of the two forms and of all entry
forms are equal bit for bit.  Generic class (random normal inputs, K <= 256): the interval checker with its 5 % cap on
ambiguous entries.  tests/test_splade_fwd_reference_host.py proves on the CPU, case by case, that the reference rejects
the planted faults.

Which case is there for which seam (cases: splade_fwd_reference.CASES; every case runs under both forms unless said):
  counts       valid rows per sequence 0 (first, between, last, and a zero-length sequence), 1, 31, 32, 33, 63, 64, 65, 127,
               128, 129, 257, 300 with all-ones, right-padded, left-padded, holey and one-row-in-the-middle masks (list
               position != sequence position); a sequence across both wave rows (> 128) and across two tiles (> 256); 44
               sub-tiles (not a multiple of 8); T above cu[-1]; max_seqlen equal to and above the longest; V = 385; nseq 16
  one_row_x20  20 sequences of one valid row: every sub-tile of a wave is another sequence (a flush per sub-tile), 31
               padded repeats per sub-tile; max_seqlen 3 (64-row chunks) and 65 (128-row chunks); V = 192
  two_tiles    2,400 valid rows x V = 3,100 (second vocabulary block, > 1,536), K = 64: 10 x 17 tiles = 9 blocks of 4 x 8,
               so the workgroups of one XCD take two tiles in a row; with K = 64 a tile is two half-steps against a ring of
               five slots, i.e. the request stream runs up to two tiles ahead and parks at its end.  (Read before it was
               run: ld_advance steps the tile whenever ld_h + 1 == nh, for any nh >= 1, the MFMA stream consumes slots in
               the same order, and a parked stream re-requests the last half-step into slots that are no longer read.)
  no_valid     no valid row in the batch: the 256x192 kernel returns before its first request (sub-tile count 0, so
               next_tile finds nothing); keys come from the memset and the finalize pass
  nseq65       65 short sequences: more than one round of groups per XCD in the 128x128 kernel's work order; V = 129
  v1 ... v777  vocabulary edges V = 1, 95, 96, 97, 127, 128, 129 (nseq65), 191, 192 (one_row_x20), 193, 385 (counts), 777:
               tiles half and wholly outside V in both forms; nseq 1 (v1, v127), 7 (partial group), 9 (more than one
               group); K = 64, 128, 256, 768 (v777), 1152 (v193); max_seqlen on both sides of 64 (v1: 40 and 128)
  v65600       V above 65,535 (no token keys: the recording entry point must refuse), K = 64, two short sequences
  groups       two calls over one token buffer as csrc/model.hip makes them on the 128x128 form (cu_seqlens + 0 with a
               short max_seqlen and finalize = 0, then cu_seqlens + 5 with finalize = 1, sparse / keys offset by 5 V):
               equal to the single call, token_weights and token_keys included
  gen64/128/256  generic class, ragged and holey masks

Value-0 keys: both forms write 0x0000FFFF (include/snx.h); the 128x128 kernel canonicalises in its final store.

Measured on an MI355X when this file was added: 19 cases + the two-call test = 148 forwards, 2,238,868 output elements
checked; every case ran under BOTH forms (the two-call test under the 128x128 form alone, as the model makes those calls),
K = 64 included: the 256x192 form took it (its row tables were written) and gave the reference's bits.  Exact class: every
key and token key equal to the reference and equal between the forms and the entry forms.  Worst error over the 2-ulp
log1p bound: sparse 0.265, token_weights 0.256.  Largest ambiguous share in the generic class: 4.675 % of the (b, v)
entries and 1.724 % of the tokens (gen256; 0.9 % / 0.5 % at K = 128, 0.7 % / 0.5 % at K = 64).  The whole file takes 3 s.
"""
import ctypes as C

import pytest
import torch

from tests import splade_fwd_reference as R

pytestmark = pytest.mark.gpu
SNX_FWD_NO_TOKEN_WEIGHTS = 2
KEY_SENTINEL = 0x5A5A5A5A
GUARD = 4096
FORMS = {"128x128": dict(dec256=0), "256x192": dict(dec256=1, dec256_min_t=1)}
ENTRIES = ("plain", "rec", "notw")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gpu_inputs(dev):
    cache = {}

    def get(name):
        if name not in cache:
            c = R.build_case(name)
            cache[name] = {k: getattr(c, k).to(dev) for k in ("Hd", "W", "bias", "cu", "mask")}
        return cache[name]
    return get


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(c, d, form, entry, calls):
    """One forward under `form` through `entry`.  calls: [(first sequence, sequences, max_seqlen, finalize)].  Returns
    (sparse, keys, tw, tkeys) on the device; tw / tkeys are None where the entry does not produce them."""
    import snx
    from snx._lib import check, fn
    from snx.ops import _p, _stream
    dev = d["Hd"].device
    T, V, K, B = c.T, c.V, c.K, c.B
    nan = float("nan")
    sparse = torch.full((B, V), nan, dtype=torch.float32, device=dev)
    keys = torch.full((B, V), KEY_SENTINEL, dtype=torch.int32, device=dev)
    tw = torch.full((T,), nan, dtype=torch.float32, device=dev)
    tkeys = torch.full((T,), KEY_SENTINEL, dtype=torch.int32, device=dev)
    full, tables = fn("snx_splade_head_scratch_bytes")(T, V), fn("snx_splade_head_scratch_bytes_notw")(T)
    need = tables if entry == "notw" else full
    scratch = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    saved = {k: snx.config(k) for k in ("dec256", "dec256_min_t")}
    try:
        snx.configure(**FORMS[form])
        for sb, ns, msl, fin in calls:
            cu = C.c_void_p(d["cu"].data_ptr() + 4 * sb)
            sp, ky = C.c_void_p(sparse.data_ptr() + 4 * sb * V), C.c_void_p(keys.data_ptr() + 4 * sb * V)
            head = (_p(d["Hd"]), _p(d["W"]), _p(d["bias"]), cu, _p(d["mask"]), sp, ky)
            if entry == "plain":
                assert fin == 1
                check(fn("snx_decoder_splade_fwd")(*head, _p(tw), _p(scratch), T, ns, msl, V, K, _stream()), "fwd")
            elif entry == "ex":
                check(fn("snx_decoder_splade_fwd_ex")(*head, _p(tw), _p(scratch), T, ns, msl, V, K, fin, _stream()), "fwd_ex")
            elif entry == "rec":
                check(fn("snx_decoder_splade_fwd_rec")(*head, _p(tw), _p(tkeys), _p(scratch), T, ns, msl, V, K, fin,
                                                       _stream()), "fwd_rec")
            else:
                check(fn("snx_decoder_splade_fwd_flags")(*head, _p(tw), _p(tkeys), _p(scratch), T, ns, msl, V, K, fin,
                                                         SNX_FWD_NO_TOKEN_WEIGHTS, _stream()), "fwd_flags")
        torch.cuda.synchronize()
    finally:
        snx.configure(**saved)
    assert bool((scratch[need:] == 0xA5).all()), "wrote behind the scratch buffer"
    touched = bool((scratch[need - tables:need] != 0xA5).any())      # the row tables of the 256x192 form
    assert touched == (form == "256x192"), f"asked for the {form} form, row tables written: {touched}"
    if entry == "notw":
        assert bool(torch.isnan(tw).all()), "token_weights written under SNX_FWD_NO_TOKEN_WEIGHTS"
        assert bool((tkeys == KEY_SENTINEL).all()), "token_keys written under SNX_FWD_NO_TOKEN_WEIGHTS"
        return sparse, keys, None, None
    if entry != "rec":
        assert bool((tkeys == KEY_SENTINEL).all()), "token_keys written without being asked for"
        return sparse, keys, tw, None
    return sparse, keys, tw, tkeys


def _check_runs(c, runs):
    """runs: {label: outputs}.  Every run against the reference; in the exact class all runs bit-equal to each other."""
    worst = dict(sparse=0.0, tw=0.0, amb_cols=0.0, amb_toks=0.0, checked=0)
    for label, (sp, ky, tw, tk) in runs.items():
        o = R.check_forward(c.ref, ky, sp, tw, tk, f"{c.name} {label}")
        worst["sparse"] = max(worst["sparse"], o.sparse_ratio)
        worst["tw"] = max(worst["tw"], o.tw_ratio)
        worst["amb_cols"], worst["amb_toks"] = max(worst["amb_cols"], o.amb_cols), max(worst["amb_toks"], o.amb_toks)
        worst["checked"] += o.checked
        # what the statistical tests of tests/test_gpu_ops.py also hold: sparse IS log1p of the key's value, on the device
        val = ((ky.to(torch.int64) & 0xFFFFFFFF) >> 16 << 16).to(torch.int32).view(torch.float32)
        assert torch.equal(_bits(torch.log1p(val)), _bits(sp)), f"{c.name} {label}: sparse is not log1p(value(keys))"
    if c.exact:
        labels = list(runs)
        first = runs[labels[0]]
        for label in labels[1:]:
            sp, ky, tw, tk = runs[label]
            assert torch.equal(ky, first[1]) and torch.equal(_bits(sp), _bits(first[0])), f"{c.name}: {label} != {labels[0]}"
        tws = [(l, r[2]) for l, r in runs.items() if r[2] is not None]
        for l, t in tws[1:]:
            assert torch.equal(_bits(t), _bits(tws[0][1])), f"{c.name}: token_weights of {l} != {tws[0][0]}"
        tks = [(l, r[3]) for l, r in runs.items() if r[3] is not None]
        for l, t in tks[1:]:
            assert torch.equal(t, tks[0][1]), f"{c.name}: token_keys of {l} != {tks[0][0]}"
    print(f"{c.name}: {len(runs)} runs ({', '.join(runs)}), {worst['checked']} elements checked, worst error / bound "
          f"sparse {worst['sparse']:.3f} token_weights {worst['tw']:.3f}, ambiguous columns {worst['amb_cols']:.3%} "
          f"tokens {worst['amb_toks']:.3%}")


@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_per_element_both_forms_all_entries(dev, gpu_inputs, name):
    from snx._lib import CONSTANTS, fn
    from snx.ops import _p, _stream
    c, d = R.build_case(name), gpu_inputs(name)
    assert c.K % 64 == 0 and c.T * c.K * 2 < 2 ** 32 and c.V * c.K * 2 < 2 ** 32      # what snx_launch_decoder256 accepts
    rec = c.spec.get("rec", True)
    runs = {}
    for form in FORMS:
        for msl in c.spec["msl"]:
            assert msl >= c.longest
            for entry in ENTRIES:
                if entry == "rec" and not rec:
                    continue
                runs[f"{form}/max_seqlen {msl}/{entry}"] = _run(c, d, form, entry, [(0, c.B, msl, 1)])
    if not rec:                                             # the column tag has 16 bits: refused before anything is launched
        buf = torch.zeros(max(c.T, 64), dtype=torch.int32, device=dev)
        scratch = torch.empty((fn("snx_splade_head_scratch_bytes")(c.T, c.V),), dtype=torch.uint8, device=dev)
        sp, ky, _, _ = next(iter(runs.values()))
        rc = fn("snx_decoder_splade_fwd_rec")(_p(d["Hd"]), _p(d["W"]), _p(d["bias"]), _p(d["cu"]), _p(d["mask"]),
                                              _p(sp.clone()), _p(ky.clone()), _p(buf.view(torch.float32)), _p(buf), _p(scratch),
                                              c.T, c.B, c.longest, c.V, c.K, 1, _stream())
        assert rc == CONSTANTS["SNX_E_SHAPE"]
    _check_runs(c, runs)


def test_two_group_calls_equal_the_single_call(dev, gpu_inputs):
    """csrc/model.hip on the 128x128 form: one call per sequence group over ONE token buffer, the last one finalises."""
    c, d = R.build_case("groups"), gpu_inputs("groups")
    sb = c.spec["split"]
    short, longest = max(c.lens[:sb]), max(c.lens[sb:])
    assert short <= 64 < longest                            # 64-row chunks in the first call, 128-row chunks in the second
    calls = [(0, sb, short, 0), (sb, c.B - sb, longest, 1)]
    runs = {}
    for entry in ("ex", "rec", "notw"):
        runs[f"128x128/one call/{entry}"] = _run(c, d, "128x128", entry, [(0, c.B, c.longest, 1)])
        runs[f"128x128/two calls/{entry}"] = _run(c, d, "128x128", entry, calls)
    _check_runs(c, runs)
