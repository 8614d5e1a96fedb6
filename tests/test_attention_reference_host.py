"""The float64 attention reference and its per-element bounds (tests/attention_reference.py), proven on the CPU against
the case table of tests/test_gpu_attention_per_element.py: (a) a float64 simulation of the kernels' cast points stays
inside the bounds in every case and tensor, (b) every case detects every planted fault that applies to it, in the forward
AND in the backward where the fault exists in both, by at least 10x in at least one element -- except what NOT_CLAIMED
lists per direction, with the reason, (c) every case contains what its comment says."""
import functools
import math

import pytest
import torch

from tests import attention_reference as R
from tests import test_gpu_attention_per_element as G

BF16 = torch.bfloat16
F64 = torch.float64
NEG_BIG = -1.0e30
LOG2E = 1.4426950408889634

MUTANTS = ("window+1", "window-1", "mask_ignored", "clamped_edge", "no_rescale", "delta_zero", "heads_swapped", "dk_dv_exchanged")
FWD_MUTANTS = ("window+1", "window-1", "mask_ignored", "clamped_edge", "no_rescale", "heads_swapped")
BWD_MUTANTS = ("window+1", "window-1", "mask_ignored", "clamped_edge", "delta_zero", "heads_swapped", "dk_dv_exchanged")


def rb(x):
    """float64 -> nearest bf16 value, as float64"""
    return x.to(torch.float32).to(BF16).to(F64)


def r32(x):
    return x.to(torch.float32).to(F64)


def applicable(case, mutant):
    if mutant == "window+1":
        return case.window >= 0
    if mutant == "window-1":
        return case.window >= 1
    if mutant == "mask_ignored":
        return bool((case.mask == 0).any())
    if mutant == "clamped_edge":
        return any(n % 64 for n in case.lens)
    return case.heads >= 2 if mutant == "heads_swapped" else True


def _sim_units(case, mutant):
    """like R._units, with the planted fault applied to the visibility; clamped_edge appends the rows between the sequence
    end and the next multiple of 64 as visible copies of the last row.  Yields (sl, h, n, rows [m] -> source row, vis [m, m])."""
    window = case.window + (mutant == "window+1") - (mutant == "window-1")
    cu = case.cu.tolist()
    for b in range(case.B):
        n = cu[b + 1] - cu[b]
        msk = case.mask[cu[b]:cu[b + 1]]
        if mutant == "mask_ignored":
            msk = torch.ones_like(msk)
        rows = torch.arange(n)
        if mutant == "clamped_edge":
            m = (n + 63) // 64 * 64
            rows = torch.arange(m).clamp(max=n - 1)
            msk = torch.cat([msk, torch.ones(m - n, dtype=msk.dtype)])
        vis = R.visibility(rows.numel(), msk, window)
        for h in range(case.heads):
            yield slice(cu[b], cu[b + 1]), h, n, rows, vis


def _swap_heads(x, case, thirds):
    """heads 0 and 1 of ONE token (the last valid one) exchanged in every third of x [T, thirds heads 64]"""
    t = int(torch.nonzero(case.mask)[-1])
    v = x.view(case.T, thirds, case.heads, 64)
    v[t, :, [0, 1]] = v[t, :, [1, 0]]
    return x


def simulate_forward(case, mutant=None):
    """The online softmax of the kernels in float64 with their cast points: key tiles of 64 over the tile range of each
    16-row group as the RESIDENT kernel takes it (the streaming kernel takes the range of its 64-row tile: the extra tiles
    are wholly out of band, their weights are wiped by the first real tile or are 0 after it, the results are the same), scores in the log2 domain, masked scores NEG_BIG, p~ = 2^(t - m) summed unrounded into l and rounded to
    bf16 as the operand of the P V product, accumulator and l rescaled by 2^(m_old - m_new); out rounded to bf16, lse to
    fp32.  -> (out [T, heads 64], lse [heads, T]) float64."""
    T, H = case.T, case.heads
    x = case.qkv.to(F64).view(T, 3, H, 64)
    out, lse = torch.zeros(T, H, 64, dtype=F64), torch.zeros(H, T, dtype=F64)
    window = case.window + (mutant == "window+1") - (mutant == "window-1")
    for sl, h, n, rows, vis in _sim_units(case, mutant):
        q, k, v = x[sl, 0, h], x[sl, 1, h][rows], x[sl, 2, h][rows]
        vis = vis[:n]
        m_keys = rows.numel()
        t = torch.where(vis, (R.SCALE * (q @ k.t())) * LOG2E, torch.full((n, m_keys), NEG_BIG, dtype=F64))
        row_lo = torch.arange(n) // 16 * 16
        j_lo, j_hi = torch.zeros(n, dtype=torch.int64), torch.full((n,), (m_keys - 1) // 64)
        if window >= 0:
            j_lo = (row_lo - window).clamp(min=0) // 64
            j_hi = (row_lo + 15 + window).clamp(max=m_keys - 1) // 64
        m_run, l_run, o = torch.full((n,), NEG_BIG, dtype=F64), torch.zeros(n, dtype=F64), torch.zeros(n, 64, dtype=F64)
        for j in range((m_keys + 63) // 64):
            ks = slice(64 * j, min(64 * j + 64, m_keys))
            act = (j >= j_lo) & (j <= j_hi)
            m_new = torch.maximum(m_run, t[:, ks].max(dim=1).values)
            alpha = torch.exp2(m_run - m_new)
            p = torch.exp2(t[:, ks] - m_new[:, None])
            l_new = l_run * alpha + p.sum(dim=1)
            o_new = (o if mutant == "no_rescale" else o * alpha[:, None]) + rb(p) @ v[ks]
            m_run, l_run = torch.where(act, m_new, m_run), torch.where(act, l_new, l_run)
            o = torch.where(act[:, None], o_new, o)
        out[sl, h] = rb(o / l_run[:, None])
        lse[h, sl] = r32((m_run + torch.log2(l_run)) / LOG2E)
    out = out.view(T, H * 64)
    if mutant == "heads_swapped":
        _swap_heads(out, case, 1)
        t = int(torch.nonzero(case.mask)[-1])
        lse[[0, 1], t] = lse[[1, 0], t]
    return out, lse


def simulate_backward(case, out_in, lse_in, mutant=None):
    """The backward's cast points in float64: P = exp(s - lse_in) and dS = P (dP - delta) rounded to bf16 as operands, the
    three gradients rounded to bf16.  -> dqkv [T, 3 heads 64] float64."""
    T, H = case.T, case.heads
    x = case.qkv.to(F64).view(T, 3, H, 64)
    dO_all, o_all, lse_all = case.dout.to(F64).view(T, H, 64), out_in.to(F64).view(T, H, 64), lse_in.to(F64)
    d = torch.zeros(T, 3, H, 64, dtype=F64)
    for sl, h, n, rows, vis in _sim_units(case, mutant):
        q, k, v = x[sl, 0, h][rows], x[sl, 1, h][rows], x[sl, 2, h][rows]
        dO, o, l_ = dO_all[sl, h][rows], o_all[sl, h][rows], lse_all[h, sl][rows]
        P = torch.where(vis, torch.exp(R.SCALE * (q @ k.t()) - l_[:, None]), torch.zeros((), dtype=F64))
        delta = torch.zeros_like(l_) if mutant == "delta_zero" else (dO * o).sum(dim=1)
        dS = rb(P * (dO @ v.t() - delta[:, None]))
        d[sl, 0, h] = rb(R.SCALE * (dS @ k))[:n]
        d[sl, 1, h] = rb(R.SCALE * (dS.t() @ q))[:n]
        d[sl, 2, h] = rb(rb(P).t() @ dO)[:n]
    if mutant == "dk_dv_exchanged":
        d = d[:, [0, 2, 1]].contiguous()
    d = d.view(T, 3 * H * 64)
    return _swap_heads(d, case, 3) if mutant == "heads_swapped" else d


@functools.lru_cache(maxsize=None)
def _worst(name, mutant=None):
    """worst err / bound ratio per tensor of the simulated kernel (with one planted fault) in a case of the GPU file"""
    case, fref, out_in, lse_in, bref = G._case(name)
    r = {}
    if mutant is None or mutant in FWD_MUTANTS:
        r.update(R.forward_ratios(*simulate_forward(case, mutant), fref))
    if mutant is None or mutant in BWD_MUTANTS:
        r.update(R.backward_ratios(simulate_backward(case, out_in, lse_in, mutant), bref))
    return r


DIRECTIONS = {"fwd": ("out", "lse"), "bwd": ("dQ", "dK", "dV")}


def directions(mutant):
    return [d for d, muts in (("fwd", FWD_MUTANTS), ("bwd", BWD_MUTANTS)) if mutant in muts]


@pytest.mark.parametrize("name", list(G.CASES))
def test_correct_rounding_stays_inside_the_bounds(name):
    r = _worst(name)
    print(f"{name}: simulated cast points, worst err / bound ratio {r}")
    assert set(r) == {"out", "lse", "dQ", "dK", "dV"} and all(v < 1.0 for v in r.values()), r


def test_reference_equals_float64_autograd():
    """a second opinion on the reference: softmax attention by autograd in float64 (dense, -inf masking) gives the reference's
    forward and, at out_in = out and lse_in = lse unrounded, its backward"""
    case = R.make_case([70, 5, 33], 2, 8, "holes", seed=3)
    fref = R.forward_reference(case)
    bref = R.backward_reference(case, fref.out, fref.lse)
    x = case.qkv.to(F64).view(case.T, 3, 2, 64).clone().requires_grad_(True)
    outs = []
    for sl, h, _, _, _, vis in R._units(case):
        s = R.SCALE * (x[sl, 0, h] @ x[sl, 1, h].t())
        outs.append((sl, h, torch.softmax(torch.where(vis, s, torch.full_like(s, -math.inf)), dim=1) @ x[sl, 2, h]))
    rows = ~fref.novis
    loss = 0
    for sl, h, o in outs:
        keep = rows[sl]
        assert ((o - fref.out.view(case.T, 2, 64)[sl, h])[keep].abs() <= 1e-13).all()
        loss = loss + (o[keep] * case.dout.to(F64).view(case.T, 2, 64)[sl, h][keep]).sum()
    loss.backward()
    assert ((x.grad.reshape(case.T, -1) - bref.dqkv).abs() <= 1e-12 * (1 + bref.dqkv.abs())).all()
    assert fref.novis.sum() == 0 or (bref.dqkv.view(case.T, 3, -1)[fref.novis, 0] == 0).all()


# Which planted faults each case is SHOWN to detect (err / bound >= 10 in at least one element of the simulated kernel),
# per direction: the forward and the backward are separate kernels and separate GPU tests.  Every applicable (mutant,
# direction) is claimed unless NOT_CLAIMED excepts it: "mutant" = both directions, "mutant/fwd" or "mutant/bwd" = one.
_ONE_TILE = "no_rescale"       # needs a maximum that rises from one key tile to the next
NOT_CLAIMED = {
    # one sequence of two tiles (65 tokens), its second tile a single key
    "seams64_w-1": (_ONE_TILE,), "seams64_w8": (_ONE_TILE,), "seams64_groups": (_ONE_TILE,), "seams64_w64": (), "seams64_w65": (),
    # window 0: a row is one key.  A masked token is then seen by nobody but itself (a row without a visible key: don't-care
    # in the forward, dO = 0 in the backward), and the copies past the sequence end are outside every band
    **{n: (_ONE_TILE, "mask_ignored", "clamped_edge") for n in G.CASES if G.CASES[n]["window"] == 0},
    # the mirror image of peaked_up: the maximum stands in the FIRST tile, nothing is ever rescaled; the copies of the last row
    # carry the LOWEST scores of every row: weights of e^-30 in the forward (the backward sees the last query's copies in dK, dV)
    "peaked_down": (_ONE_TILE, "clamped_edge/fwd"),
}
# no sequence of seams64 has two tokens 65 or 66 apart (65 tokens at the most): windows 64 + 1 and 65 +- 1 change nothing there;
# the seam windows are decided on `tiles` and `stream` (and 63 +- 1, 64 - 1 on seams64 too)
NOT_CLAIMED["seams64_w64"] += ("window+1",)
NOT_CLAIMED["seams64_w65"] += ("window+1", "window-1")


def claimed(name, mutant, direction):
    ex = NOT_CLAIMED.get(name, ())
    return applicable(G._case(name)[0], mutant) and mutant not in ex and f"{mutant}/{direction}" not in ex


@pytest.mark.parametrize("name,mutant", [(n, m) for n in G.CASES for m in MUTANTS])
def test_each_case_detects_its_planted_faults(name, mutant):
    todo = [d for d in directions(mutant) if claimed(name, mutant, d)]
    if not todo:
        return
    r = _worst(name, mutant)
    print(f"{name}, {mutant}: worst err / bound ratio {r}")
    for d in todo:
        assert max(r[t] for t in DIRECTIONS[d]) >= 10.0, (name, mutant, d, r)


def test_what_is_not_claimed_is_really_not_detected():
    """an exception that the case WOULD detect is a stale entry: every listed (mutant, direction) that applies stays below 10"""
    for name, ex in NOT_CLAIMED.items():
        for e in ex:
            mutant, _, d = e.partition("/")
            if not applicable(G._case(name)[0], mutant):
                continue
            r = _worst(name, mutant)
            for dd in ([d] if d else directions(mutant)):
                assert max(r[t] for t in DIRECTIONS[dd]) < 10.0, (name, e, dd, r)


# ----------------------------------------------------------------------------- (c) the cases hold what their comments say
def _first_tile_masked_for_a_valid_query(case):
    """a valid query whose first key tile (of its 16-row group's tile range, as the resident kernels take it; the streaming
    kernels start no later) holds no valid key"""
    cu = case.cu.tolist()
    for b in range(case.B):
        m = case.mask[cu[b]:cu[b + 1]]
        for i in torch.nonzero(m).flatten().tolist():
            lo = max(i // 16 * 16 - case.window, 0) // 64 if case.window >= 0 else 0
            if not m[64 * lo:64 * lo + 64].any():
                return True
    return False


def test_the_families_stand_on_both_sides_of_every_seam():
    lens = set(sum((f["lens"] for f in G.FAMILIES.values()), []))
    for seam in (16, 32, 64, 128, 192, 256):
        assert {seam - 1, seam, seam + 1} <= lens, seam
    assert {1, 2, 511, 513} <= lens and max(lens) == 513
    for fam, ms in (("seams64", 256), ("stream", 1024)):                    # max_seqlen declared above the longest sequence
        assert G.FAMILIES[fam]["max_seqlen"] == ms > max(G.FAMILIES[fam]["lens"])
    windows = {kw["window"] for kw in G.CASES.values()}
    assert {-1, 0, 1, 8, 63, 64, 65, 128} <= windows
    for fam in G.FAMILIES:
        assert {G.CASES[f"{fam}_w{w}"]["window"] for w in (-1, 0, 8, 63, 64, 65)} == {-1, 0, 8, 63, 64, 65}
    assert all(sum(kw["lens"]) <= 2500 and kw["heads"] in (2, 3) for kw in G.CASES.values())


def test_unit_counts_leave_dead_slots():
    s = G.FAMILIES["seams64"]
    units = len(s["lens"]) * s["heads"]
    assert units == 33 and units % 4 and units % 8            # streaming blocks are dealt over 8 XCDs: 7 dead blocks per tile
    for name, tiles in (("seams64_groups", {1, 2}), ("tiles_groups", {2, 3, 4}), ("mixed_groups_w64", {1, 4, 5})):
        kw = G.CASES[name]
        ntu = [(ml + 63) // 64 for _, _, ml in kw["groups"]]
        assert set(ntu) == tiles
        for (s0, n, ml), t in zip(kw["groups"], ntu):
            assert max(kw["lens"][s0:s0 + n]) <= ml
        if name == "seams64_groups":                           # 30 units in workgroups of 4, 3 units in workgroups of 2
            assert [(n * kw["heads"]) % (4 // t) for (_, n, _), t in zip(kw["groups"], ntu)] == [2, 1]
    kinds = sorted(ml for _, _, ml in G.CASES["mixed_groups_w64"]["groups"])
    assert kinds[0] <= 64 < kinds[1] <= 256 < kinds[2]


def test_every_recipe_meets_a_resident_and_a_streaming_case():
    for recipe in R.RECIPES:
        names = [n for n, kw in G.CASES.items() if kw["recipe"] == recipe]
        assert any(n in G.RESIDENT for n in names) and any(max(G.CASES[n]["lens"]) > 256 for n in names), recipe


@pytest.mark.parametrize("name", list(G.CASES))
def test_the_masks_hold_what_the_recipes_say(name):
    case, fref, out_in, lse_in, _ = G._case(name)
    cu = case.cu.tolist()
    seqs = [case.mask[cu[b]:cu[b + 1]] for b in range(case.B)]
    assert all(int(m.sum()) >= 1 for m in seqs)
    assert (case.dout.view(case.T, -1)[case.mask == 0] == 0).all()
    assert (out_in[fref.novis] == 0).all() and (lse_in[:, fref.novis] == 0).all()
    long = max(case.lens) > 65
    if case.recipe in ("left", "mix") and long:
        assert _first_tile_masked_for_a_valid_query(case)
        assert any(int(torch.nonzero(m)[0]) >= 64 for m in seqs)
    if case.recipe == "right":
        assert any(int(m.sum()) == 1 and m.numel() > 1 for m in seqs)                       # one valid token
    if case.recipe == "mix":                                                                # a masked tail and a masked head
        assert any(m[0] == 1 and m[-1] == 0 for m in seqs) and any(m[0] == 0 and m[-1] == 1 for m in seqs)
    if case.recipe == "right" and long:
        assert any((int(m.sum()) + 63) // 64 < (m.numel() + 63) // 64 for m in seqs)        # a wholly masked trailing tile
    if case.recipe in ("holes", "mix"):
        assert any(((m[1:-1] == 0) & (m[:-2] == 1) & (m[2:] == 1)).any() for m in seqs if m.numel() > 2)
    if case.recipe == "alternate":
        assert all(abs(int(m.sum()) * 2 - m.numel()) <= 1 for m in seqs)
    if case.recipe == "holes" and case.window == 0:
        assert fref.novis.sum() >= 3                           # rows without a visible key: the holes themselves
    if case.recipe == "ones":
        assert (case.mask == 1).all() and not fref.novis.any()


def test_the_peaked_cases_are_sharp_and_their_maximum_moves_as_said():
    for name, last in (("peaked_up", True), ("peaked_down", False)):
        case = G._case(name)[0]
        for sl, h, q, k, v, vis in R._units(case):
            n = q.shape[0]
            z = R.SCALE * (q @ k.t())
            top = z.argmax(dim=1)
            assert (z.max(dim=1).values - z.min(dim=1).values).min() > 30         # e^-30: the far end of a row is nothing
            assert torch.softmax(z, dim=1).max(dim=1).values.mean() > 0.15        # against 1 / n < 0.02 for a flat row
            if n > 64:
                tile = top // 64
                assert (tile == ((n - 1) // 64 if last else 0)).float().mean() > 0.9
                if last:                                       # the maximum of the keys seen so far rises in EVERY tile
                    run = torch.stack([z[:, :64 * j + 64].max(dim=1).values for j in range((n + 63) // 64)], dim=1)
                    assert ((run[:, 1:] > run[:, :-1]).all(dim=1)).float().mean() > 0.9
