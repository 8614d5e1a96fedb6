"""The float64 reference of the routed SPLADE-head backward and its per-element check, proven on the CPU: the reference
is autograd's answer, an fp32 summation in any order stays inside the derived bounds, and every planted local fault --
the kind that the global cos / rel criterion lets through -- violates them."""
import pytest
import torch

from tests import splade_bwd_reference as R

BF16 = torch.bfloat16
F64 = torch.float64


def test_reference_equals_float64_autograd():
    """Autograd of log1p(relu(logits)).max over the rows (and over the columns, for token_weights) in float64, the routing
    taken from that arg-max.  Hd, W and the bias are small dyadic numbers, so the float64 logits ARE bf16 values (multiples
    of 1/16 below 16) and the keys can carry them; g comes from the exact-coefficient builder, so the coefficient's bf16
    rounding in the reference changes nothing and the two answers differ by float64 rounding alone."""
    gen = torch.Generator().manual_seed(5)
    lens = torch.tensor([7, 1, 12, 5])
    B, V, H = 4, 37, 8
    T = int(lens.sum())
    cu = torch.zeros(B + 1, dtype=torch.int64)
    cu[1:] = lens.cumsum(0)
    Hd = (torch.randint(-8, 9, (T, H), generator=gen).to(F64) / 4).requires_grad_(True)
    W = (torch.randint(-2, 3, (V, H), generator=gen).to(F64) / 4).requires_grad_(True)
    bias = (torch.randint(-16, 17, (V,), generator=gen).to(F64) / 16).requires_grad_(True)
    mask = torch.ones(T, dtype=F64)
    mask[2] = mask[9] = 0.0
    logits = Hd @ W.t() + bias
    assert (logits.detach().to(BF16).to(F64) == logits.detach()).all()
    sc = torch.log1p(torch.relu(logits)) * mask[:, None]
    per_seq = [sc[cu[b]:cu[b + 1]].max(dim=0) for b in range(B)]
    sparse = torch.stack([m.values for m in per_seq])
    row = torch.stack([m.indices for m in per_seq])
    mt = sc.max(dim=1)
    keys = R.encode_keys(torch.expm1(sparse.detach()).to(BF16).to(F64), row)
    xt = torch.expm1(mt.values.detach()).to(BF16).to(F64)
    tkeys = torch.where(xt > 0, R.encode_keys(xt, mt.indices), torch.full((T,), 0xFFFF, dtype=torch.int32))
    x, _ = R.decode_keys(keys)
    at_row = torch.stack([torch.relu(logits.detach())[cu[b] + row[b], torch.arange(V)] * mask[cu[b] + row[b]] for b in range(B)])
    assert (x == at_row).all()                                       # expm1(log1p(.)) came back to the bf16 logit
    g, _ = R.build_exact_g(x, gen)
    g_tw = R.build_exact_g_tw(g, keys, tkeys, cu, gen)
    assert R.token_routing(g, keys, tkeys, cu).same.sum() >= 3       # coincident entries are part of the case
    ((sparse * g.to(F64)).sum() + (mt.values * g_tw.to(F64)).sum()).backward()
    dW0, db0 = torch.randn(V, H, generator=gen), torch.randn(V, generator=gen)
    ref = R.splade_bwd_reference(g, keys, g_tw, tkeys, Hd.detach(), W.detach(), cu, dW0, db0)
    for name, got, want, mag in (("dHd", ref.dHd, Hd.grad, ref.dHd_mag), ("dW", ref.dW - dW0.to(F64), W.grad, ref.dW_mag),
                                 ("db", ref.db - db0.to(F64), bias.grad, ref.db_mag)):
        assert ((got - want).abs() <= 1e-13 * mag).all(), name
    assert (ref.row_entries > 0).sum() > 5 and (ref.row_entries[mask == 0] == 0).all()


def _emulate_fp32(case, gen, drop_entry=None, shift_entry=None, skip_seq=None):
    """The kernels' arithmetic in plain fp32, one addition at a time in a SHUFFLED order: coefficient = bf16 of the fp32
    quotient, products of two bf16 values, fp32 running sums, dHd rounded to bf16 once.  The keyword arguments plant one
    fault each."""
    f32 = torch.float32
    x, row = R.decode_keys(case.keys)
    c = torch.where(x > 0, (case.g / (1.0 + x).to(f32)).to(BF16).to(f32), torch.zeros((), dtype=f32))
    cu = case.cu.to(torch.int64)
    ent = [(int(cu[b] + row[b, v]), v, float(c[b, v])) for b in range(case.B) for v in range(case.V)
           if c[b, v] != 0 and b != skip_seq]
    if drop_entry is not None:
        ent.pop(drop_entry)
    if shift_entry is not None:
        t, v, cc = ent[shift_entry]
        b = int(torch.searchsorted(cu, t, right=True) - 1)
        ent[shift_entry] = (t + 1 if t + 1 < cu[b + 1] else t - 1, v, cc)
    if case.g_tw is not None:
        r = R.token_routing(case.g, case.keys, case.tkeys, cu)
        d = (1.0 + r.x).to(f32)
        gs = r.gs.to(f32)
        ct = ((gs + case.g_tw) / d).to(BF16).to(f32) - (gs / d).to(BF16).to(f32)
        ct = torch.where(r.live & (case.g_tw != 0), ct, torch.zeros((), dtype=f32))
        ent += [(t, int(r.v[t]), float(ct[t])) for t in range(case.T) if ct[t] != 0 and int(r.seq[t]) != skip_seq]
    Hd, W = case.Hd.to(f32), case.W.to(f32)
    dH = torch.zeros(case.T, case.H, dtype=f32)
    dW, db = case.dW0.clone(), case.db0.clone()
    for i in torch.randperm(len(ent), generator=gen).tolist():
        t, v, cc = ent[i]
        dH[t] += cc * W[v]
    for i in torch.randperm(len(ent), generator=gen).tolist():
        t, v, cc = ent[i]
        dW[v] += cc * Hd[t]
        db[v] += cc
    return dH, dW, db


@pytest.fixture(scope="module")
def small():
    case = R.make_case([9, 1, 30, 4, 17], 48, 128, seed=11, routing=["random", "random", "one_row", "round_robin", "random"],
                       tokens="spread")
    return case, R.reference_of(case)


def test_fp32_sums_in_a_shuffled_order_stay_inside_the_bounds(small):
    case, ref = small
    gen = torch.Generator().manual_seed(2)
    for _ in range(3):
        dH, dW, db = _emulate_fp32(case, gen)
        ratios = R.check_routed(dH.to(BF16), dW, db, ref, case.dW0, case.db0, what="emulation")
        # the summation term alone (before the bf16 rounding) uses a small part of its bound
        s = ((dH.to(F64) - ref.dHd).abs() / (R.gamma(ref.dHd_n.to(F64))[:, None] * ref.dHd_mag).clamp(min=1e-300)).max()
        print("fp32 emulation, worst err / bound ratio:", ratios, "summation term of dHd alone:", float(s))
        assert max(ratios.values()) <= 1.0 and float(s) <= 1.0


@pytest.mark.parametrize("fault", ["entry_dropped", "entry_one_row_off", "vocabulary_row_dropped", "sequence_skipped"])
def test_planted_faults_violate_the_bounds(small, fault):
    case, ref = small
    gen = torch.Generator().manual_seed(3)
    kw = {"entry_dropped": dict(drop_entry=17), "entry_one_row_off": dict(shift_entry=40),
          "sequence_skipped": dict(skip_seq=3)}.get(fault, {})
    dH, dW, db = _emulate_fp32(case, gen, **kw)
    dH = dH.to(BF16)
    if fault == "vocabulary_row_dropped":
        v = int(torch.nonzero(ref.col_entries > 0)[5])
        dW[v], db[v] = case.dW0[v], case.db0[v]
    with pytest.raises(AssertionError, match="bound violated, worst err / bound ratio") as ei:
        R.check_routed(dH, dW, db, ref, case.dW0, case.db0, what=fault)
    print(ei.value)
    msg = str(ei.value)
    if fault == "vocabulary_row_dropped":
        assert "dW: bound violated" in msg and "db: bound violated" in msg and "dHd: bound violated" not in msg
    elif fault == "entry_one_row_off":                                # the column's coefficient sum does not move
        assert "dHd: bound violated" in msg and "dW: bound violated" in msg and "db: bound violated" not in msg
    else:
        assert all(f"{n}: bound violated" in msg for n in ("dHd", "dW", "db"))


def test_exact_requirements_are_enforced(small):
    """an unwritten (NaN) row, a non-zero row without an entry, a touched idle column"""
    case, ref = small
    gen = torch.Generator().manual_seed(4)
    dH, dW, db = _emulate_fp32(case, gen)
    dH = dH.to(BF16)
    empty = int(torch.nonzero(ref.row_entries == 0)[0])
    bad = dH.clone()
    bad[empty, 3] = float("nan")
    with pytest.raises(AssertionError, match="not written"):
        R.check_routed(bad, dW, db, ref, case.dW0, case.db0)
    bad = dH.clone()
    bad[empty, 3] = 2.0 ** -60
    with pytest.raises(AssertionError, match="not exact zeros"):
        R.check_routed(bad, dW, db, ref, case.dW0, case.db0)
    g2 = case.g.clone()
    g2[:, 7] = 0.0                                                   # an idle column (tokens may still name it: none do)
    r2 = R.splade_bwd_reference(g2, case.keys, None, None, case.Hd, case.W, case.cu, case.dW0, case.db0)
    assert r2.col_entries[7] == 0
    dW2 = r2.dW.float()
    dW2[7, 0] += 2.0 ** -20
    with pytest.raises(AssertionError, match="differ from their initial values"):
        R.check_routed(r2.dHd.to(BF16), dW2, r2.db.float(), r2, case.dW0, case.db0)


def test_the_builder_makes_every_coefficient_exact():
    gen = torch.Generator().manual_seed(9)
    x = R.pick_x((12000,), gen)
    assert x.min() >= 2.0 ** -6 and x.max() < 16
    g, c = R.build_exact_g(x, gen)
    assert ((g / (1.0 + x).float()).to(BF16).to(F64) == c).all()
    assert (g == 0).float().mean() < 0.2 and (g < 0).any() and (g > 0).any()
    # logits of a real forward may be tiny: the product then has no exact fp32 form and the entry is switched off
    g2, c2 = R.build_exact_g(torch.tensor([2.0 ** -30, 2.0 ** -9, 0.0], dtype=F64), gen, zero_frac=0.0)
    assert g2[0] == 0 and g2[1] != 0 and g2[2] != 0 and c2[2] == 0


def test_the_gpu_cases_hold_what_they_are_meant_to():
    """tests/test_gpu_splade_bwd_routed.py: the token-direction cases really contain masked tokens, coincident and
    non-coincident entries, and more tokens of one column than one chunk of the counting sort holds; the routing case has
    its buckets of exactly 63, 64, 65 and 128 entries, a bucket of several hundred and two sequences without an entry"""
    from tests.test_gpu_splade_bwd_routed import _case
    case, ref = _case("tw_mixed")
    r = R.token_routing(case.g, case.keys, case.tkeys, case.cu)
    active = r.live & (case.g_tw != 0)
    assert (~r.live).sum() >= 10 and (active & r.same).sum() >= 10 and (active & ~r.same).sum() >= 10
    assert r.same[0] or not r.live[0]                       # a one-token sequence's entry always coincides
    case, ref = _case("tw_one_col")
    assert int(ref.tok_col_entries.max()) > 1024 and (ref.tok_col_entries > 0).sum() == 1
    case, ref = _case("routing")
    assert ref.row_entries[:4].tolist() == [63, 64, 65, 128]
    lo, hi = int(case.cu[3]), int(case.cu[5])
    assert (ref.row_entries[lo:hi] == 0).all() and int(ref.row_entries.max()) > 600
    case, ref = _case("V4100")
    assert int(ref.row_entries.max()) > 3000
    g, x = case.g, R.decode_keys(case.keys)[0]
    assert ((x == 0) & (g != 0)).any() and ((x > 0) & (g == 0)).any() and (g < 0).any()
