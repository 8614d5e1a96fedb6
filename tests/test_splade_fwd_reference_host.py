"""The exact forward reference of the SPLADE head and its checker (tests/splade_fwd_reference.py), proven on the CPU against
the case table that tests/test_gpu_splade_fwd_per_element.py runs on the GPU: (a) a simulation of the kernels' cast points
-- two forms with different summation orders and the row bookkeeping of the form they stand for -- is accepted in every
case (exact class: bit-equal; generic class: inside the intervals and under the ambiguity cap), (b) every planted fault
that applies to a case is rejected there, each output planted on its own, except what NOT_CLAIMED lists with the reason,
and what is listed is really not seen, (c) the builder's conditions and the ambiguity cap hold with the reference alone.

The simulated forms.  "128": fp32 accumulation over ascending 32-wide k blocks; a sequence's candidates are its valid rows,
tagged with their sequence positions (decoder_splade_kernel).  "256": descending 16-wide k blocks; the candidates are the
positions of the compacted list of valid rows, the last 32-row sub-tile padded with repeats of the last valid row at later
list positions, and a finalize step maps list positions to sequence positions (decoder256.hip)."""
import functools

import numpy as np
import pytest
import torch

from tests import splade_fwd_reference as R

F64 = torch.float64
PRI = 1 << 18                                               # priorities and tags stay below it


# ----------------------------------------------------------------------------------------------- the simulation
@functools.lru_cache(maxsize=8)
def _acc32(name, form):
    c = R.build_case(name)
    blk, order = (32, 1) if form == "128" else (16, -1)
    h, w = c.Hd.to(torch.float32), c.W.to(torch.float32)
    acc = torch.zeros(c.T, c.V, dtype=torch.float32)
    for k0 in list(range(0, c.K, blk))[::order]:
        acc = acc + h[:, k0:k0 + blk] @ w[:, k0:k0 + blk].t()
    return acc


def _lost_subtile(c):
    """the planted 'one sub-tile lost': the first 32 list positions of the sequence with the most valid rows"""
    return int(np.argmax(c.nvalid))


def simulate(name, form, fault=None):
    """-> keys [B, V], tkeys [T] (int64), sparse, tw (fp32) of the simulated form with one planted fault"""
    c = R.build_case(name)
    T, V, B = c.T, c.V, c.B
    acc = _acc32(name, form)
    bias = c.bias if fault == "bias_unrounded" else R.rbf_bias(c.bias)
    x = acc + bias[None, :]
    vb = R.value_bits_f32(x, truncate=fault == "truncate")
    cu = [int(v) for v in c.cu]
    keys = torch.full((B, V), R.EMPTY_KEY, dtype=torch.int64)
    for b in range(B):
        s0, ln = cu[b], cu[b + 1] - cu[b]
        vp = torch.nonzero(c.mask[s0:s0 + ln]).flatten()
        if fault == "mask_ignored" or (fault == "masked_seq_nonzero" and vp.numel() == 0):
            vp = torch.arange(ln)
        n = vp.numel()
        src, tag, rep = s0 + vp, (vp if form == "128" else torch.arange(n)), vp
        pri = 2 * (PRI - tag)                               # the lower tag wins a tie
        if fault == "tie_later_row":
            pri = 2 * tag
        if fault == "list_position":                        # (256) finalize forgotten
            rep = tag
        if form == "256" and n % 32 and n:
            npad = 32 - n % 32
            ptag = n + torch.arange(npad)
            src = torch.cat([src, (s0 + vp[-1]).repeat(npad)])
            rep = torch.cat([rep, ln + ptag])               # whatever the list holds behind its end: modelled as no row of
                                                            # the sequence (a stale entry that names the right row shows nowhere)
            pri = torch.cat([pri, 2 * (PRI - ptag) if fault != "pad_wins" else torch.full((npad,), 2 * (PRI - n + 1) + 1)])
            tag = torch.cat([tag, ptag])
        if fault == "rows_past_end" and cu[b + 1] < T:      # the next sequence's first row (or the first trailing row)
            src = torch.cat([src, torch.tensor([cu[b + 1]])])
            rep = torch.cat([rep, torch.tensor([ln])])
            pri = torch.cat([pri, torch.tensor([2 * (PRI - ln)])])
            tag = torch.cat([tag, torch.tensor([ln])])
        if fault == "subtile_lost" and b == _lost_subtile(c):
            keep = torch.arange(src.numel()) >= 32
            src, rep, pri = src[keep], rep[keep], pri[keep]
        if src.numel() == 0:
            continue
        vals = vb[src]
        win = torch.from_numpy(((vals << 20) | pri[:, None]).numpy().argmax(0))
        m = vals.max(0).values
        keys[b] = torch.where(m > 0, (m << 16) | ((0xFFFF - rep[win]) & 0xFFFF), torch.full_like(m, R.EMPTY_KEY))
    if fault == "seq_shift":
        keys = torch.roll(keys, 1, 0)
    if fault == "last_col_dropped":
        keys[:, V - 1] = R.EMPTY_KEY
    # token half
    live = torch.zeros(T, dtype=torch.bool)
    live[:cu[-1]] = c.mask[:cu[-1]] != 0
    if fault == "mask_ignored_tok":
        live[:cu[-1]] = True
    tv = vb
    col = torch.arange(V)
    if fault == "last_col_dropped_tok":
        tv = vb.clone()
        tv[:, V - 1] = 0
    if fault == "col_past_v_tok":                           # a column V built from row V - 1 of W and a stale bias
        tv = torch.cat([vb, R.value_bits_f32(x[:, V - 1:] + 8.0)], 1)
        col = torch.arange(V + 1)
    pri = (PRI - col) if fault != "tie_higher_col" else col
    win = torch.from_numpy(((tv << 20) | pri[None, :]).numpy().argmax(1))
    m = tv.max(1).values
    tkeys = torch.where(live & (m > 0), (m << 16) | ((0xFFFF - col[win]) & 0xFFFF), torch.full_like(m, R.EMPTY_KEY))
    if fault == "relu_missing_tok":                         # the row maximum of the signed logits
        raw = R.raw_bits_f32(x)
        neg = live & (m == 0) & (raw >= 0x8000).all(1)      # every logit negative: the largest = the smallest bits
        nwin = torch.from_numpy(raw.numpy().argmin(1))
        tkeys = torch.where(neg, (raw.min(1).values << 16) | (0xFFFF - nwin), tkeys)
    if fault == "subtile_lost_tok":
        b = _lost_subtile(c)
        vp = torch.nonzero(c.mask[cu[b]:cu[b + 1]]).flatten()[:32]
        tkeys[cu[b] + vp] = R.EMPTY_KEY
    sparse = torch.log1p(R.bits_value(keys >> 16).to(torch.float32))
    tw = torch.log1p(R.bits_value(tkeys >> 16).to(torch.float32))
    return keys, tkeys, sparse, tw


def _check(name, form, fault=None):
    c = R.build_case(name)
    keys, tkeys, sparse, tw = simulate(name, form, fault)
    rec = c.spec.get("rec", True)
    return R.check_forward(c.ref, keys, sparse, tw, tkeys if rec else None, f"{name}/{form}/{fault}")


# fault -> the simulated form it is planted in
FAULTS = {
    "mask_ignored": "128", "mask_ignored_tok": "128", "rows_past_end": "128", "tie_later_row": "128", "tie_higher_col": "128",
    "pad_wins": "256", "list_position": "256", "bias_unrounded": "128", "truncate": "256", "last_col_dropped": "128",
    "last_col_dropped_tok": "256", "col_past_v_tok": "256", "relu_missing_tok": "128", "seq_shift": "256",
    "masked_seq_nonzero": "128", "subtile_lost": "256", "subtile_lost_tok": "256",
}


def applicable(name, fault):
    """structural: does the case contain what the fault acts on at all"""
    c = R.build_case(name)
    rec = c.spec.get("rec", True)
    masked_rows = any(nv < ln for nv, ln in zip(c.nvalid, c.lens))
    if fault in ("tie_higher_col", "relu_missing_tok", "col_past_v_tok", "last_col_dropped_tok"):
        return rec and sum(c.nvalid) > 0                    # seen through the token keys (or a live token's weight)
    if fault in ("mask_ignored", "mask_ignored_tok"):
        return masked_rows
    if fault == "masked_seq_nonzero":
        return any(nv == 0 and ln > 0 for nv, ln in zip(c.nvalid, c.lens))
    if fault == "rows_past_end":
        return c.B > 1 or c.T > int(c.cu[-1])
    if fault == "seq_shift":
        return c.B > 1 and sum(c.nvalid) > 0
    if fault == "tie_later_row":
        return max(c.nvalid) >= 2
    if fault == "pad_wins":
        return any(nv % 32 for nv in c.nvalid)
    if fault == "list_position":                            # some valid row whose list position is not its sequence position
        return any(bool((vp != torch.arange(vp.numel())).any()) for _, _, vp in c.ref.rows)
    return sum(c.nvalid) > 0


# (case, fault) pairs that apply by shape and that the reference nevertheless cannot see, with the reason
_EXACT = [n for n in R.CASES if R.CASES[n]["kind"] == "exact"]
NOT_CLAIMED = {
    # relu on the token side shows only on a live token whose every logit is negative: the cases built with a strictly
    # negative bias and a zero row (allneg), and the one-column case
    **{(n, "relu_missing_tok"): "no live token with only negative logits"
       for n in R.CASES if not (R.CASES[n].get("allneg") or n == "v1")},
    ("gen64", "last_col_dropped_tok"): "random bias, 777 columns: column V - 1 is no live token's only arg-max",
    ("gen128", "last_col_dropped_tok"): "random bias, 777 columns: column V - 1 is no live token's only arg-max",
    ("v1", "bias_unrounded"): "one column: the unrounded bias moves a logit only at a tie between 2 and 4 that goes down; no maximum is one",
    ("v1", "mask_ignored"): "one column: none of the 7 masked rows exceeds the maximum of the 33 valid ones",
    ("v1", "tie_higher_col"): "one column",
    ("v1", "tie_later_row"): "33 rows, one column: no two valid rows share the maximum",
    ("v1", "pad_wins"): "the last valid row does not attain the maximum of the only column",
}


@pytest.mark.parametrize("name", list(R.CASES))
def test_builder_conditions_and_cap_with_the_reference_alone(name):
    c = R.build_case(name)
    ref = c.ref
    out = R.check_forward(ref, ref.keys, ref.sparse.to(torch.float32), ref.tw.to(torch.float32),
                          ref.tkeys if c.spec.get("rec", True) else None, name)
    print(f"{name}: T {c.T} B {c.B} V {c.V} K {c.K} valid {c.nvalid} conditions {c.stats} ambiguous columns "
          f"{out.amb_cols:.3%} tokens {out.amb_toks:.3%}")
    assert out.amb_cols <= R.AMBIGUOUS_CAP and out.amb_toks <= R.AMBIGUOUS_CAP
    if c.exact:
        assert out.amb_cols == 0 and out.amb_toks == 0
        assert int(c.cu[-1]) + c.spec.get("tail", 0) == c.T and not bool(c.mask[int(c.cu[-1]):].any())


@pytest.mark.parametrize("form", ["128", "256"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_clean_simulation_is_accepted(name, form):
    c = R.build_case(name)
    out = _check(name, form)
    keys, tkeys, _, _ = simulate(name, form)
    if c.exact:                                             # bit-equal, said once more without the checker
        assert torch.equal(keys, c.ref.keys)
        assert c.ref.tkeys is None or torch.equal(tkeys, c.ref.tkeys)
    assert out.sparse_ratio <= 1.0 and out.tw_ratio <= 1.0


def _detected(name, fault):
    try:
        _check(name, FAULTS[fault], fault)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("name", list(R.CASES))
def test_each_case_detects_its_planted_faults(name, fault):
    if not applicable(name, fault) or (name, fault) in NOT_CLAIMED:
        return
    assert _detected(name, fault), f"{name}: planted fault {fault} passes the checker"


def test_what_is_not_claimed_is_really_not_detected():
    for (name, fault), why in NOT_CLAIMED.items():
        if applicable(name, fault):
            assert not _detected(name, fault), f"stale NOT_CLAIMED entry: {name} detects {fault} ({why})"


def test_rounding_helper_rounds_once_to_nearest_even():
    """_rne_bf16_value against exhaustive neighbours: ties go to the even significand, and a value a hair off the tie that
    fp32 would first round ONTO the tie is still rounded by its true position"""
    one = 1.0
    ulp = 2.0 ** -7                                          # bf16 spacing in [1, 2)
    x = np.array([one + 0.5 * ulp, one + 1.5 * ulp, one + 0.5 * ulp + 2.0 ** -30, one + 1.5 * ulp - 2.0 ** -30, -3.0, 0.0])
    want = np.array([one, one + 2 * ulp, one + ulp, one + ulp, -3.0, 0.0])
    assert (R._rne_bf16_value(x) == want).all()
    through_f32 = torch.tensor(x, dtype=F64).to(torch.float32).to(torch.bfloat16).to(F64).numpy()
    assert through_f32[2] == one                             # the double rounding the helper avoids
