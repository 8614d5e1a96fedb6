"""Host-side proof of tests/tn_reference.py (no GPU): the restated plans are the library's, they are consistent with
themselves, the tables reach every class, and the reference admits what the kernels' trees can produce and rejects what
they cannot.

a. Plans against the library.  workspace_bytes == snx_gemm_tn_workspace_bytes, to the byte, on every table row and for
   M = 1..9,000 on three groups (the only exported figure that depends on tn_pick_splits, tn128_plan, tn256_schedule and
   tail_contributors at once; host code, no launch).
b. Plan consistency, every table row and a sweep of (tiles, K-steps, workgroups): the items of all workgroups partition
   ntiles x nsteps exactly once; contributor_of is injective per tile; its range is exactly what the reduce adds (the
   non-empty pieces, then tail_contributors); no index reaches `slabs`.
c. Class coverage, read off the tables through the plans.
d. Emulations.  emulate() walks the plan of a case in fp32 -- per contribution the token ranges it multiplies, summed
   range by range, contributions added to dW0 in reduce order -- with two inner orders (whole 64-row K-steps ascending;
   32-row half-steps, second half first, rows reversed) and once with every partial of a tile arriving in a shuffled order
   (float atomics).  All must equal the exact family's one value and lie inside the random family's sets.
e. Planted faults.  FAULTS names, per fault, a row where it can occur and the families that must reject it; "rejected" =
   at least one element leaves its set (non-finite counts), the count is printed.  Measured here, elements outside their
   set, exact / random family:
       256 form, 512 x 512, M = 320 (262,144 elements, 65,536 per tile)        128 form, 768 x 384, M = 300 (16,384 per tile)
       drop_seam_step     65,536 /  65,511                                      16,384 / 16,380
       double_seam_step   65,536 /  65,511                                      16,384 / 16,380
       drop_half_step     65,536 /  65,497                                      16,384 / 16,371
       drop_last_row     157,976 / 258,455        overwrite 262,106 / 262,052   overwrite 294,887 / 294,829
   and on the rows where only they can occur: rest_dropped 32,768 / 32,564, rest_twice 65,536 / 65,175, half_tile_shifted
   32,768 / 32,728, tail_skipped 65,536 / 65,504, tail_to_neighbour 131,072 / 131,009, inter_twice and inter_none 270,300 /
   270,167, swap_nk 260,360 / 261,078; a NaN guard row or an unwritten slab: every element of the tile.
   bf16_product cannot occur in the exact family (every product of two multiples of 1/8 up to 1/2 is a bf16 value): the
   test asserts that it is ADMITTED there, and rejected in the random family.
"""
import numpy as np
import pytest
import torch

from tests import tn_reference as T

GR = T.GUARD_ROWS
ROWS_256 = [(g, M, res) for g, M, res, _, _ in T.CASES_256]
SWEEP_GROUPS = (((768, 384),), T.SMALL_LAYER, T.LAYER_149M)


# ----------------------------------------------------------------------------- a. plans against the library
def _lib_bytes(group, M):
    from snx import fn
    from snx.ops import TnProblem
    group = T.norm_group(group)
    arr = (TnProblem * len(group))(*[TnProblem(0, 0, 0, N, K, inter, 0) for N, K, inter in group])
    return int(fn("snx_gemm_tn_workspace_bytes")(arr, len(group), M))


def test_workspace_bytes_equal_the_library_on_every_row():
    rows = [(g, M) for g, M, *_ in T.CASES_256] + [T.CASE_DEFAULT[:2]] + [(g, M) for g, M, *_ in T.CASES_128]
    for g, M in rows:
        assert T.workspace_bytes(g, M) == _lib_bytes(g, M), (g, M)
    assert max(T.workspace_bytes(g, M) for g, M in rows) == 106168320          # the 101 MB of the largest row


@pytest.mark.parametrize("group", SWEEP_GROUPS)
def test_workspace_bytes_equal_the_library_over_m(group):
    bad = [M for M in range(1, 9001) if T.workspace_bytes(group, M) != _lib_bytes(group, M)]
    assert not bad, (group, bad[:10])


def test_small_m_is_refused_by_nothing_on_the_host():
    """the defect this file arrived with: "tn256_min_m" <= M < 64 advertised 0 workspace bytes and then demanded P x ntiles
    slabs (SNX_E_ARG before any launch).  The host-visible half: 0 bytes are advertised and the plan that runs needs none."""
    for M in (1, 32, 63):
        assert _lib_bytes(((128, 128),), M) == 0
        p = T.dispatch(((128, 128),), M, 1, 1, 0)
        assert p.form == "128" and p.slabs == 0


# ----------------------------------------------------------------------------- b. plan consistency
def _check_plan(p):
    seen = np.zeros((p.ntiles, p.nsteps), dtype=np.int64)
    for L, its in p.items.items():
        for tile, sb, se in its:
            assert 0 <= sb < se <= p.nsteps and 0 <= tile < p.ntiles
            seen[tile, sb:se] += 1
    assert (seen == 1).all(), "the items do not partition ntiles x nsteps exactly once"
    per_tile = {}
    for (c, tile), Ls in p.writes.items():
        assert len(Ls) == 1, f"slab ({c}, {tile}) has writers {Ls}"            # contributor_of injective per tile
        assert 0 <= c < p.slabs, "a contributor index reaches `slabs`"
        per_tile.setdefault(tile, []).append(c)
    for t in range(p.ntiles):
        assert sorted(per_tile.get(t, [])) == p.reads[t], (t, sorted(per_tile.get(t, [])), p.reads[t])
        assert p.reads[t] == sorted(set(p.reads[t]))
    # the reduce's fixed order is token order: ascending contributor = ascending K-steps (pieces, then the tail by id)
    rng = {k: next((sb, se) for tile, sb, se in p.items[v[0]] if tile == k[1]) for k, v in p.writes.items()}
    for t in range(p.ntiles):
        ends = [rng[(c, t)] for c in p.reads[t]]
        assert all(a[1] == b[0] for a, b in zip(ends, ends[1:])) and ends[0][0] == 0 and ends[-1][1] == p.nsteps


def test_plans_are_consistent_on_every_row():
    for g, M, res in ROWS_256 + [T.CASE_DEFAULT[:3]]:
        p = T.tn256_plan(g, M, res)
        if p is not None:
            _check_plan(p)


def test_plans_are_consistent_over_a_sweep():
    n = 0
    for tiles_n in (1, 2, 3, 6, 9, 17, 78, 100, 128, 135, 200, 256):
        group = ((256 * tiles_n, 256),)
        for res in (0, 8, 24, 64, 128):
            for steps in list(range(1, 41)) + [129, 576]:
                p = T.tn256_plan(group, 64 * steps, res)
                assert (p is None) == (tiles_n > 256 - res)
                if p is not None:
                    _check_plan(p)
                    n += 1
    assert n > 2000


def test_128_plan_covers_every_row_once():
    for M in list(range(1, 1200)) + [3000, 8293, 36864]:
        for tiles in (1, 18, 34, 306, 540):
            group = ((128 * tiles, 128),)
            p = T.tn128_plan(group, M)
            assert p.rows % 64 == 0 and (p.splits - 1) * p.rows < M <= p.splits * p.rows and 1 <= p.last <= p.rows


# ----------------------------------------------------------------------------- c. class coverage
def test_tables_reach_every_class():
    plans = [T.dispatch(g, M, 1, 1, res) for g, M, res in ROWS_256]
    p256 = [p for p in plans if p.form == "256"]
    groups = [T.norm_group(g) for g, *_ in T.CASES_256]
    classes = {
        "one tile, P = 256, all but one or two pieces empty": any(p.ntiles == 1 and p.P == 256 and p.empty >= 254 for p in p256),
        "a tile three quarters outside": any(p.group == ((128, 128, 0),) for p in p256),
        "empty main pieces, no spare workgroups": any(p.empty and not p.spare for p in p256),
        "spare workgroups with tail_len 0": any(p.spare and p.tail_len == 0 for p in p256),
        "K = 128 mod 256": any(K % 256 == 128 for p in p256 for _, K, _ in p.group),
        "N = 128 mod 256": any(N % 256 == 128 for p in p256 for N, _, _ in p.group),
        "ragged rest": any(p.rest for p in p256),
        "fewer workgroups (reserved CUs)": {p.nwg for p in p256} >= {256, 248, 232, 128},
        "the small model's layer group": any(p.ntiles == 9 and p.P == 28 and p.empty == 12 for p in p256),
        "interleaved problem not the first": any(len(g) > 1 and g[-1][2] and not g[0][2] for g in groups),
        "interleaved problem inside a group of four": any(len(g) == 4 and g[1][2] for g in groups),
        "P = 2 with a tail": any(p.P == 2 and p.tail_len for p in p256),
        "P = 1": any(p.P == 1 for p in p256),
        "a tail workgroup spans 2 tiles": any(p.span == 2 for p in p256),
        "a tail workgroup spans 3 tiles": any(p.span == 3 for p in p256),
        "idle tail workgroups beside working ones": any(p.idle and p.tail_len for p in p256),
        "tiles with 1 and with 2 tail contributors": any((p.tc_min, p.tc_max) == (1, 2) for p in p256),
        "items of several K-steps": any(p.longest >= 4 for p in p256),
        "the 256 form declines": any(p.form == "128" and w is None for p, (*_, w, _) in zip(plans, T.CASES_256)),
        "fewer rows than one K-step": sum(p.form == "128" and w == "128" for p, (*_, w, _) in zip(plans, T.CASES_256)) >= 2,
    }
    assert all(classes.values()), [k for k, v in classes.items() if not v]
    d = T.dispatch(*T.CASE_DEFAULT[:2], 1, 8192, 0)
    assert d.form == "256" and d.tail_len == 1 and d.rest and T.CASE_DEFAULT[1] >= 8192
    p128 = [T.tn128_plan(g, M) for g, M, *_ in T.CASES_128]
    c128 = {
        "one split, direct flush, fewer rows than a step": any(p.splits == 1 and p.last < 64 for p in p128),
        "one split, a step and one row": any(p.splits == 1 and p.last == 65 for p in p128),
        "slabs with a ragged last split": any(p.splits == 2 and p.last % 64 for p in p128),
        "last split = one whole step + 1 row": any(p.splits > 1 and p.last == 65 for p in p128),
        "last split shorter than a step": any(p.splits > 1 and p.last < 64 for p in p128),
        "tile_end decode over 4 problems": any(len(g) == 4 for g, *_ in T.CASES_128),
        "one tile, 10 splits": any(p.tiles == 1 and p.splits == 10 for p in p128),
        "interleaved": any(x[2] for g, *_ in T.CASES_128 for x in T.norm_group(g)),
    }
    assert all(c128.values()), [k for k, v in c128.items() if not v]
    # coverage of modes: the random family on three rows per table at least, atomics on the half-outside, ragged-rest and
    # one tail row, random atomics on one row per table
    for table, marks in ((T.CASES_256, [r[4] for r in T.CASES_256]), (T.CASES_128, [r[3] for r in T.CASES_128])):
        assert sum(T.RND in m for m in marks) >= 3 and sum(T.RND_ATOM in m for m in marks) >= 1
    for p, (*_, marks) in zip(plans, T.CASES_256):
        if p.form == "256" and (p.half_outside or p.rest):
            assert T.ATOM in marks
    assert any(T.ATOM in marks and p.form == "256" and p.tail_len for p, (*_, marks) in zip(plans, T.CASES_256))
    assert any(T.ATOM in r[3] and T.tn128_plan(r[0], r[1]).last % 64 for r in T.CASES_128)
    for g, M, *_, marks in T.CASES_256 + T.CASES_128:
        assert T.RND not in marks or M <= T.M_RANDOM_MAX


def test_exact_reference_is_the_float64_product():
    """the float32 integer product is THE value: equal to the float64 product of the same operands, on every row"""
    rows = [(g, M) for g, M, *_ in T.CASES_256] + [T.CASE_DEFAULT[:2]] + [(g, M) for g, M, *_ in T.CASES_128]
    for g, M in rows:
        c = T.build_case("exact", T.norm_group(g), M)
        for p, (N, K, inter) in enumerate(c.group):
            dy, x = T.operands(c, p)
            nat = dy[:, torch.from_numpy(np.argsort(T.src_rows(N)))] if inter else dy
            ref = c.dW0[p].double() + nat.double().t() @ x.double()
            assert torch.equal(c.want[p].double(), ref), (g, M, p)
            w = c.want[p]
            assert torch.equal(w * 64, (w * 64).round()) and float(w.abs().max()) < 4096
            two = (c.dW0[p] + 2 * (c.sum32[p] / 64.0)).double()
            assert torch.equal(two, c.dW0[p].double() + 2 * (nat.double().t() @ x.double()))


# ----------------------------------------------------------------------------- d. emulations
def contributions(c, plan):
    """per problem a list of regions (n0, n1, k0, k1) in the kernel's row order with their partials in reduce order; a
    partial = dict(ranges=[(r0, r1) token rows], ...)"""
    out = [[] for _ in c.group]
    if plan.form == "128":
        t = 0
        for p, (N, K, _) in enumerate(c.group):
            for n0 in range(0, N, 128):
                for k0 in range(0, K, 128):
                    parts = [dict(ranges=[(m, min(m + 64, min(c.M, (s + 1) * plan.rows)))
                                          for m in range(s * plan.rows, min(c.M, (s + 1) * plan.rows), 64)])
                             for s in range(plan.splits)]
                    out[p].append(dict(reg=(n0, n0 + 128, k0, k0 + 128), parts=parts))
                    t += 1
        assert t == plan.tiles
        return out
    rng = {(k[0], k[1]): next((sb, se) for tile, sb, se in plan.items[v[0]] if tile == k[1]) for k, v in plan.writes.items()}
    for t, (p, n0, k0) in enumerate(plan.tiles):
        N, K, _ = c.group[p]
        parts = [dict(ranges=[(64 * s, 64 * s + 64) for s in range(*rng[(ci, t)])], slab=ci) for ci in plan.reads[t]]
        if plan.rest:
            parts.append(dict(ranges=[(plan.M64, c.M)], rest=True))
        out[p].append(dict(reg=(n0, min(n0 + 256, N), k0, min(k0 + 256, K)), parts=parts, tile=t))
    return out


def plant(fault, c, plan, con):
    """edit the contributions to plant one fault; returns the flags emulate() needs"""
    flags = {}
    regs = [r for pr in con for r in pr]
    if fault == "drop_seam_step":                      # the first K-step of the second contributor of a tile is lost
        r = next(r for r in regs if len([q for q in r["parts"] if not q.get("rest")]) >= 2)
        r["parts"][1]["ranges"] = r["parts"][1]["ranges"][1:]
    elif fault == "double_seam_step":                  # ... or added by both neighbours
        r = next(r for r in regs if len([q for q in r["parts"] if not q.get("rest")]) >= 2)
        r["parts"][0]["ranges"] = r["parts"][0]["ranges"] + r["parts"][1]["ranges"][:1]
    elif fault == "drop_half_step":
        r0, r1 = regs[0]["parts"][0]["ranges"][0]
        assert r1 - r0 == 64
        regs[0]["parts"][0]["ranges"][0] = (r0, r0 + 32)
    elif fault == "drop_last_row":
        for r in regs:
            a, b = r["parts"][-1]["ranges"][-1]
            assert b == c.M
            r["parts"][-1]["ranges"][-1] = (a, b - 1)
    elif fault == "rest_dropped":
        assert plan.rest
        regs[-1]["parts"] = [q for q in regs[-1]["parts"] if not q.get("rest")]
    elif fault == "rest_twice":
        assert plan.rest
        regs[0]["parts"].append(regs[0]["parts"][-1])
    elif fault == "nan_guard_row":                     # one row past M - 1 multiplied in
        a, b = regs[0]["parts"][-1]["ranges"][-1]
        regs[0]["parts"][-1]["ranges"][-1] = (a, b + 1)
    elif fault == "guard_row_before":                  # ... or the one before row 0
        a, b = regs[0]["parts"][0]["ranges"][0]
        regs[0]["parts"][0]["ranges"][0] = (a - 1, b)
    elif fault == "empty_slab_added":
        assert plan.empty
        regs[-1]["parts"].insert(0, dict(nan=True))
    elif fault == "tail_skipped":
        r = next(r for r in regs if any(q.get("slab", -1) >= plan.P for q in r["parts"]))
        assert r["parts"][-1]["slab"] >= plan.P
        r["parts"].pop()
    elif fault == "tail_to_neighbour":
        i = next(i for i, r in enumerate(regs) if any(q.get("slab", -1) >= plan.P for q in r["parts"]))
        q = regs[i]["parts"].pop()
        regs[i + 1]["parts"].append(dict(q, src=regs[i]["reg"]))
    elif fault == "half_tile_shifted":                 # the half of a tile that lies outside K lands one tile over
        r = next(r for r in regs if r["reg"][3] - r["reg"][2] == 128)
        flags["shift"] = r
    elif fault in ("swap_nk", "inter_twice", "inter_none", "bf16_product", "overwrite"):
        flags[fault] = True
    else:
        raise KeyError(fault)
    return flags


def emulate(c, plan, order=0, atomics=False, fault=None):
    """fp32 emulation of the plan's summation tree -> per problem dW [N, K] (natural rows), float32 tensors"""
    con = contributions(c, plan)
    flags = plant(fault, c, plan, con) if fault else {}
    gen = torch.Generator().manual_seed(c.M)
    outs = []
    for p, (N, K, inter) in enumerate(c.group):
        dyb, xb = c.dY[p].float(), c.X[p].float()                              # guarded: token row m is row GR + m

        def term(r0, r1, reg):
            n0, n1, k0, k1 = reg
            pieces = [(r0, r1)] if order == 0 or r1 - r0 <= 32 else [(r0 + 32, r1), (r0, r0 + 32)]
            acc = None
            for a, b in pieces:
                rows = torch.arange(GR + a, GR + b)
                if order:
                    rows = rows.flip(0)
                d, x = dyb[rows][:, n0:n1], xb[rows][:, k0:k1]
                if flags.get("bf16_product"):
                    v = (d[:, :, None] * x[:, None, :]).to(T.BF16).float().sum(0)
                else:
                    v = d.t() @ x
                acc = v if acc is None else acc + v
            return acc

        perm = torch.from_numpy(T.src_rows(N)) if inter else torch.arange(N)
        out = torch.zeros(N, K) if flags.get("overwrite") else c.dW0[p][perm].clone()   # kernel row order
        for r in con[p]:
            n0, n1, k0, k1 = r["reg"]
            partials = []
            for q in r["parts"]:
                if q.get("nan"):
                    partials.append(torch.full((n1 - n0, k1 - k0), float("nan")))
                    continue
                acc = torch.zeros(n1 - n0, k1 - k0)
                for a, b in q["ranges"]:
                    acc = acc + term(a, b, q.get("src", r["reg"]))
                partials.append(acc)
            if atomics:
                partials = [partials[i] for i in torch.randperm(len(partials), generator=gen)]
            for acc in partials:
                if flags.get("swap_nk") and n1 - n0 == k1 - k0:
                    acc = acc.t()
                out[n0:n1, k0:k1] += acc
            if flags.get("shift") is r and n0 + 1 < N:
                tot = sum(partials)
                h = min(n1 - n0, N - n0 - 1)
                out[n0 + 1:n0 + 1 + h, 0:128] += tot[:h, :128]
        nat = torch.empty_like(out)
        if flags.get("inter_none"):
            nat = out
        elif flags.get("inter_twice"):
            nat[perm[perm]] = out
        else:
            nat[perm] = out
        outs.append(nat)
    return outs


def outside(c, plan, got):
    """elements outside their set, per problem"""
    n = []
    for (lo, hi), g in zip(T.expected(c, plan), got):
        v = g.double().numpy()
        n.append(int((~(np.isfinite(v) & (v >= lo) & (v <= hi))).sum()))
    return n


EMU_ROWS = ([("256", g, M, res) for g, M, res, _, _ in T.CASES_256 if sum(N * K for N, K, _ in T.norm_group(g)) * M < 1.3e9]
            + [("128", g, M, 0) for g, M, _, _ in T.CASES_128])


def _plan(form, g, M, res):
    return T.dispatch(g, M, 1, 1, res) if form == "256" else T.tn128_plan(g, M)


@pytest.mark.parametrize("form,group,M,res,family", [(*r, f) for r in EMU_ROWS for f in ("exact", "random")
                                                     if f == "exact" or r[2] <= T.M_RANDOM_MAX])
def test_emulations_are_admitted(form, group, M, res, family):
    c, plan = T.build_case(family, T.norm_group(group), M), _plan(form, group, M, res)
    for kw in (dict(order=0), dict(order=1), dict(order=0, atomics=True)):
        got = emulate(c, plan, **kw)
        assert outside(c, plan, got) == [0] * len(c.group), (kw, outside(c, plan, got))
        if family == "exact":
            assert all(torch.equal(a, b) for a, b in zip(got, c.want)), kw


def test_guarded_check_accepts_and_tallies():
    """the GPU file's path: a guarded buffer holding an emulation passes check_guarded; the exact family is all `single`"""
    g, M = ((768, 384, 1),), 257
    plan = T.tn128_plan(g, M)
    for family in ("exact", "random"):
        c = T.build_case(family, T.norm_group(g), M)
        buf, mid = T.guarded_dw(c.dW0[0])
        mid.copy_(emulate(c, plan)[0])
        st = T.check_guarded(buf, T.expected(c, plan)[0], family)
        assert st.n == 768 * 384 and (st.single == 1.0) == (family == "exact")
        buf[GR - 1, 5] = 1.0
        with pytest.raises(AssertionError, match="guard rows before"):
            T.check_guarded(buf, T.expected(c, plan)[0], family)
    ws = T.workspace(1024)
    T.check_workspace(ws, 1024, "ws")
    ws[256] = 0
    with pytest.raises(AssertionError, match="behind the advertised"):
        T.check_workspace(ws, 1024, "ws")


# ----------------------------------------------------------------------------- e. planted faults
B_ = ("exact", "random")
R512 = ("256", ((512, 512),), 320, 0)
R300 = ("128", ((768, 384),), 300, 0)
FAULTS = (
    ("drop_seam_step", R512, B_), ("drop_seam_step", R300, B_),
    ("double_seam_step", R512, B_), ("double_seam_step", R300, B_),
    ("drop_half_step", R512, B_), ("drop_half_step", R300, B_),
    ("drop_last_row", R512, B_), ("drop_last_row", ("128", ((768, 384, 1),), 257, 0), B_),
    ("drop_last_row", ("256", ((768, 384, 1),), 1061, 0), B_),
    ("rest_dropped", ("256", ((768, 384, 1),), 1061, 0), B_), ("rest_twice", ("256", ((768, 384, 1),), 1061, 0), B_),
    ("nan_guard_row", R512, B_), ("nan_guard_row", R300, B_), ("guard_row_before", R512, B_),
    ("nan_guard_row", ("128", ((128, 128),), 63, 0), B_),
    ("empty_slab_added", R512, B_), ("empty_slab_added", ("256", ((256, 256),), 64, 0), B_),
    ("tail_skipped", ("256", ((2560, 2560),), 320, 0), B_), ("tail_to_neighbour", ("256", ((2560, 2560),), 320, 0), B_),
    ("half_tile_shifted", ("256", ((768, 384),), 1088, 24), B_),
    ("swap_nk", R512, B_), ("swap_nk", ("128", ((128, 128),), 65, 0), B_),
    ("inter_twice", ("256", ((768, 384, 1),), 1061, 0), B_), ("inter_none", ("256", ((768, 384, 1),), 1061, 0), B_),
    ("inter_twice", ("128", ((768, 384, 1),), 257, 0), B_), ("inter_none", ("128", ((768, 384, 1),), 257, 0), B_),
    ("bf16_product", ("256", ((128, 128),), 192, 0), ("random",)),
    ("overwrite", R512, B_), ("overwrite", R300, B_),
)


@pytest.mark.parametrize("fault,row,families", FAULTS, ids=[f"{f}-{r[0]}-{r[2]}" for f, r, _ in FAULTS])
def test_planted_faults_are_rejected(fault, row, families):
    form, group, M, res = row
    plan = _plan(form, group, M, res)
    for family in B_:
        if family == "random" and M > T.M_RANDOM_MAX:
            continue
        c = T.build_case(family, T.norm_group(group), M)
        bad = sum(outside(c, plan, emulate(c, plan, fault=fault)))
        print(f"{fault} on {form} {group} M={M} {family}: {bad} of {sum(N * K for N, K, _ in c.group)} elements outside their set")
        assert (bad > 0) == (family in families), (fault, row, family, bad)
