"""Lexical teacher scores on the GPU (csrc/teacher_lex.hip, snx_teacher_forward_m3): head, unique kernel, pair scorer and the
whole path, each against float64 torch or plain Python computed here.  Bounds: an fp32 dot product of H terms and a bias,
1.01 (H + 2) 2^-24 (sum |h w| + |b|); a sum of m rounded non-negative products, 1.01 (m + 1) 2^-24 score; a max is exact."""
import ctypes as C
import functools

import pytest
import torch

from tests import teacher_helpers as TH

pytestmark = pytest.mark.gpu
DEV, UNUSED, EPS = "cuda:0", (0, 1, 2, 3), 2.0 ** -24


def _call(name, *args):
    from snx import fn
    from snx._lib import check
    check(fn(name)(*[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args],
                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


@pytest.mark.parametrize("H", (256, 512, 768, 1024))
@pytest.mark.parametrize("T", (1, 5, 259))
def test_token_weights_against_float64(T, H):
    gen = torch.Generator().manual_seed(100 * T + H)
    h, w, b = torch.randn(T, H, generator=gen), 0.1 * torch.randn(H, generator=gen), 0.25
    w[0] = 0.5
    h[0] = -h[0].abs() * w.sign()                                  # every product negative: relu gives exactly 0.0f
    h[1:2] = -0.5 * torch.nn.functional.one_hot(torch.tensor([0]), H)      # row 1, if there is one: -0.25 + b, exactly zero
    if T > 2:
        h[T - 1] = h[T - 1].abs() * w.sign()                       # every product positive
    ref = torch.relu(h.double() @ w.double() + b)
    bound = 1.01 * (H + 2) * EPS * ((h.double() * w.double()).abs().sum(dim=1) + b)
    out, dh, dw = torch.full((T + 8,), 7.0, device=DEV), h.to(DEV), w.to(DEV)
    _call("snx_teacher_token_weights", dh, dw, b, out, T, H)
    got = out.cpu().double()
    err = (got[:T] - ref).abs()
    print(f"token weights T={T} H={H}: max err {float(err.max()):.3e}, {float((err / bound).max()):.3f} of bound")
    assert bool((got[T:] == 7.0).all()) and bool((err <= bound).all())
    assert got[0] == 0.0 and (T < 2 or got[1] == 0.0) and (T < 3 or got[T - 1] > 1.0)


def _lex_dict(ids, tw):
    d = {}
    for v, x in zip(ids, tw):
        if v not in UNUSED and x > 0:
            d[v] = max(d.get(v, 0.0), x)
    return d


def test_unique_kernel_exact():
    gen, lens = torch.Generator().manual_seed(11), (1, 2, 3, 64, 65, 255, 256, 257, 1000, 4097)
    seqs = []
    for s, n in enumerate(lens):
        a, b = float(s + 1), float(len(lens) - s)                  # id 10 grows with s, id 11 falls: either neighbour has a
        plant = [(10, 9 * a), (11, b), (12, 5.0), (13, 0.0), (14, 0.0), (10, a), (11, 2 * b), (12, 5.0), (13, 0.0),   # larger one
                 (14, 3.0)] + [(u, 1e4) for u in UNUSED]            # max first / last / twice; all 0; 0 and > 0; unused
        fill = max(0, n - len(plant) - 1)
        rid = torch.randint(100, 100 + max(1, n // 3), (fill,), generator=gen).tolist()
        rw = (torch.rand(fill, generator=gen) * (torch.rand(fill, generator=gen) > 0.2)).tolist()
        seqs.append(plant + list(zip(rid, rw)) + [(11, 8 * b)] if n > len(plant) else plant[:n])
    seqs.append([(u, 1e4) for u in UNUSED + (0,)])                 # unused ids only: no term
    ids = torch.tensor([v for s in seqs for v, _ in s], dtype=torch.long)
    tw = torch.tensor([x for s in seqs for _, x in s], dtype=torch.float32)
    cu = torch.tensor([0] + [len(s) for s in seqs]).cumsum(0).tolist()
    tok = [(ids[a:b].tolist(), tw[a:b].tolist()) for a, b in zip(cu, cu[1:])]
    want = [_lex_dict(*t) for t in tok]
    for s in range(len(lens)):                                     # the trap is real: a max across the boundary differs
        o = s + 1 if s + 1 < len(lens) else s - 1
        both = _lex_dict(tok[s][0] + tok[o][0], tok[s][1] + tok[o][1])
        assert {v: both[v] for v in want[s]} != want[s]
    T, n = cu[-1], len(seqs)
    lex_id, cnt, lex_w = (torch.full((m + 4,), v, dtype=t, device=DEV) for m, v, t in
                          ((T, 77, torch.int32), (n, 77, torch.int32), (T, 7.0, torch.float32)))
    dids, dtw, dcu = ids.to(DEV), tw.to(DEV), torch.tensor(cu, dtype=torch.int32, device=DEV)
    _call("snx_lexical_unique", dids, dtw, dcu, (C.c_int32 * 4)(*UNUSED), 4, lex_id, lex_w, cnt, T, n, max(lens))
    gi, gw, gc = lex_id.cpu().tolist(), lex_w.cpu().tolist(), cnt.cpu().tolist()
    assert gi[T:] == [77] * 4 and gw[T:] == [7.0] * 4 and gc[n:] == [77] * 4 and gc[n - 1] == 0
    for s in range(n):
        a, b, k = cu[s], cu[s + 1], len(want[s])
        assert gc[s] == k and gi[a:a + k] == sorted(want[s]) and gw[a:a + k] == [want[s][v] for v in sorted(want[s])]
        assert gi[a + k:b] == [-1] * (b - a - k) and [str(x) for x in gw[a + k:b]] == ["0.0"] * (b - a - k)   # not -0.0f


def test_pair_scorer_against_float64():
    from snx.teacher import lexical_pairs
    gen, lens = torch.Generator().manual_seed(12), (0, 1, 63, 64, 65, 300)
    rows = []
    for L in lens:                                                 # row 2 i, and behind it a trap: its ids with weights of 1000
        ids = torch.randperm(600, generator=gen)[:L].sort().values
        rows += [(ids, torch.rand(L, generator=gen) + 0.5), (ids, torch.full((L,), 1000.0))]
    rows.append((10000 + torch.arange(64), torch.ones(64)))        # row 12: disjoint from all
    ptr = torch.tensor([0] + [len(r[0]) for r in rows]).cumsum(0).tolist()
    ids, w = torch.cat([r[0] for r in rows]).to(torch.int32), torch.cat([r[1] for r in rows])
    maps = [dict(zip(i.tolist(), x.double().tolist())) for i, x in rows]
    pairs = [(2 * i, 2 * j) for i in range(6) for j in range(6)] + [(2 * i, 12) for i in range(6)] + [(12, 2 * i) for i in range(6)]
    ref = torch.tensor([sum(x * maps[b][v] for v, x in maps[a].items() if v in maps[b]) for a, b in pairs], dtype=torch.float64)
    m = torch.tensor([len(maps[a].keys() & maps[b].keys()) for a, b in pairs], dtype=torch.float64)
    pq, pd = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    dids, dw = ids.to(DEV), w.to(DEV)
    got = lexical_pairs(ptr, dids, dw, pq, pd)
    err, bound = (got.double().cpu() - ref).abs(), 1.01 * (m + 1) * EPS * ref
    print(f"lexical pairs: {int((ref > 0).sum())} of {len(pairs)} positive, {float((err[ref > 0] / bound[ref > 0]).max()):.3f} of bound")
    assert int((m > 0).sum()) >= 16 and bool((err <= bound).all())  # disjoint rows, an empty side: bound 0, exactly 0.0f
    assert torch.equal(got, lexical_pairs(ptr, dids, dw, pq, pd))  # the same bits from call to call ...
    h = len(pairs) // 2                                            # ... and whatever else is in the pair list
    assert torch.equal(got, torch.cat([lexical_pairs(ptr, dids, dw, pq[:h], pd[:h]), lexical_pairs(ptr, dids, dw, pq[h:], pd[h:])]))


def _dense(ptr, ids, w, n, V):
    rows = torch.repeat_interleave(torch.arange(n), (ptr[1:] - ptr[:-1]).cpu())
    return torch.zeros(n, V, dtype=torch.float64).index_put((rows, ids.cpu().long()), w.cpu().double())


@functools.lru_cache(maxsize=None)
def _end_to_end_reference():
    """The golden batch through forward_torch and the sparse head in fp32, with emulated bf16 and in float64 -> per run the
    lexical weights as a dense [n, vocab] map and the pair scores; the head's bound; the pairs' shared terms.  All CPU."""
    from snx.teacher import (forward_torch, lexical_pairs_torch, lexical_weights_torch, random_sparse_head,
                             token_weights_torch)
    _, cfg, sd = TH.golden()
    ids, mask = TH.golden_reference("batch")[:2]
    sparse, n = random_sparse_head(cfg, 79), int(ids.shape[0])
    pq = torch.tensor([0] * n + list(range(n)) + [n - 1] * n)      # sequence 0 is <s> </s> and has no term: the last
    pd = torch.tensor(list(range(n)) * 3)                          # sequence is paired with all of them too
    out = []
    for params, emul in ((sd, False), (sd, True), ({k: v.double() for k, v in sd.items()}, False)):
        _, _, h = forward_torch(cfg, params, ids, mask, emulate_bf16=emul, return_hidden=True)
        tw = token_weights_torch(sparse, h)
        ptr, li, lw = lexical_weights_torch(ids, mask, tw, UNUSED)
        out.append((_dense(ptr, li, lw, n, cfg.vocab_size), lexical_pairs_torch(ptr, li, lw, pq, pd)))
    assert float((tw[mask.bool()] > 0).double().mean()) >= 1 / 3   # the comparison is not vacuous
    hw = (h.abs() @ sparse["weight"].double().reshape(-1).abs() + sparse["bias"].double().abs())[mask.bool()].max()
    shared = ((out[2][0] > 0).double() @ (out[2][0] > 0).double().t())[pq, pd]
    return sparse, ids, mask, pq, pd, out, float(1.01 * (cfg.hidden_size + 2) * EPS * hw), shared


@pytest.mark.parametrize("precision", ("bf16", "fp32"))
def test_encode_m3_end_to_end(precision):
    from snx.teacher import TeacherEncoder, lexical_pairs, random_colbert_head
    _, cfg, sd = TH.golden()
    sparse, ids, mask, pq, pd, ((w32, s32), (w16, s16), (w64, s64)), tw_bound, shared = _end_to_end_reference()
    enc = TeacherEncoder(cfg, sd, DEV, precision, colbert_head=random_colbert_head(cfg, 77), sparse_head=sparse)
    emb, mv_ptr, mv, lex_ptr, li, lw = enc.encode_tokens_m3(ids, mask, UNUSED)
    assert torch.equal(emb, enc.encode_tokens(ids, mask))          # the outputs of the other entry points, bit for bit
    assert all(torch.equal(x, y) for x, y in zip((emb, mv_ptr, mv), enc.encode_tokens_multivector(ids, mask)))
    bare = TeacherEncoder(cfg, sd, DEV, precision, sparse_head=sparse).encode_tokens_m3(ids, mask, UNUSED)
    assert bare[2] is None and all(torch.equal(x, y) for x, y in zip(bare[:1] + bare[3:], (emb, lex_ptr, li, lw)))
    gw, gs = _dense(lex_ptr, li, lw, len(ids), cfg.vocab_size), lexical_pairs(lex_ptr, li, lw, pq, pd).double().cpu()
    for name, got, x32, x16, x64, kernel in (("weights", gw, w32, w16, w64, tw_bound),
                                             ("scores", gs, s32, s16, s64, 1.01 * (shared + 1) * EPS * s64)):
        e_ref, e32 = float((x16 - x32).abs().max()), float((x32 - x64).abs().max())
        if precision == "bf16":
            to_emul, to_f32 = float((got - x16).abs().max()) / e_ref, float((got - x32).abs().max()) / e_ref
            print(f"end to end bf16 {name}: e_ref {e_ref:.3e}, {to_emul:.3f} e_ref to emulated, {to_f32:.3f} e_ref to fp32")
            assert to_emul <= 1.0 and to_f32 <= 2.0
        else:
            err, bound = (got - x64).abs(), 4.0 * e32 + kernel
            print(f"end to end fp32 {name}: e32 {e32:.3e}, err {float(err.max()):.3e}, {float((err / bound).max()):.3f} of bound")
            assert bool((err <= bound).all())
