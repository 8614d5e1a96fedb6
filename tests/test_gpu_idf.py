"""GPU checks of the IDF line (csrc/idf.hip, include/snx.h "IDF", snx/idf.py) against the restatement
tests/idf_reference.py.  Counts, means, query rows and the dense query matrix are held to equality; the float64 sums and
the fp32 gradient coefficients to bounds derived next to each assertion from the number formats, not from the results."""
import numpy as np
import pytest
import torch

from tests import idf_reference as R

pytestmark = pytest.mark.gpu

VS = [1, 63, 64, 65, 1027, 250002]
U = 2.0 ** -24                                   # unit roundoff of fp32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def token_rows(rng, n, S, V):
    """Rows with a hot id, ids < 0 and >= V, a row of one repeated token and a row with every position masked."""
    ids = rng.integers(-2, V + 3, size=(n, S), dtype=np.int64)
    hot = rng.random((n, S)) < 0.3
    ids[hot] = 0
    mask = (rng.random((n, S)) < 0.8).astype(np.int64)
    ids[0, :] = V - 1
    mask[0, :] = 1
    if n > 1:
        mask[1, :] = 0
    if n > 2:
        ids[2, :] = V + 1                                      # nothing countable, nothing masked
        mask[2, :] = 1
    return ids, mask


# ------------------------------------------------------------------------------------------------ doc_freq
def _doc_freq_case(dev, n, S, V, seed):
    from snx.idf import doc_freq
    rng = np.random.default_rng(seed)
    ids, mask = token_rows(rng, n, S, V)
    want, nd = R.doc_freq(ids, mask, V)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    got, got_n = doc_freq(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), V, count=count)
    assert got.dtype == torch.int64 and tuple(got.shape) == (V,)
    assert np.array_equal(got.cpu().numpy(), want), (n, S, V)
    assert got_n == nd == n and int(count) == n                # every row is a document, the fully masked one too
    return ids, mask, want, got


@pytest.mark.parametrize("S", [1, 7, 64, 300, 9000])
@pytest.mark.parametrize("V", VS)
def test_doc_freq_equals_the_restatement(dev, V, S):
    _doc_freq_case(dev, 257 if S <= 64 else 3, S, V, seed=V * 31 + S)


@pytest.mark.parametrize("n", [1, 3, 257])
def test_doc_freq_row_counts(dev, n):
    _doc_freq_case(dev, n, 64, 1027, seed=n)


def test_doc_freq_more_rows_than_workgroups(dev):
    """Rows beyond the launch's 2048 workgroups: a workgroup walks several documents and its hot-id table carries counts
    from one to the next."""
    _doc_freq_case(dev, 5000, 7, 65, seed=9)


def test_doc_freq_at_the_largest_vocabulary(dev):
    """V = 2^20: 128 KiB of bitmap, the launch that opts in to more than 64 KiB of LDS."""
    _doc_freq_case(dev, 5, 300, 1 << 20, seed=20)


def test_doc_freq_two_calls_accumulate(dev):
    from snx.idf import IdfTable, doc_freq
    V = 1027
    rng = np.random.default_rng(4)
    a, b = token_rows(rng, 70, 33, V), token_rows(rng, 5, 300, V)
    wa, na = R.doc_freq(*a, V)
    wb, nb = R.doc_freq(*b, V)
    df, nd = doc_freq(torch.from_numpy(a[0]).to(dev), torch.from_numpy(a[1]).to(dev), V)
    df2, nd = doc_freq(torch.from_numpy(b[0]).to(dev), torch.from_numpy(b[1]).to(dev), V, out=df, num_docs=nd)
    assert df2 is df and nd == na + nb == 75
    assert np.array_equal(df.cpu().numpy(), wa + wb)
    t = IdfTable(V, dev)
    t.fit_tokens(torch.from_numpy(a[0]), torch.from_numpy(a[1])).fit_tokens(torch.from_numpy(b[0]), torch.from_numpy(b[1]))
    assert t.num_docs == 75 and np.array_equal(t.doc_freq_host(), wa + wb)
    for sm in ("bm25", "standard", "smooth"):
        assert np.array_equal(_bits(t.idf(sm)), _bits(R.idf(wa + wb, 75, sm))), sm


def test_doc_freq_refuses_a_vocabulary_beyond_the_bitmap(dev):
    from snx.idf import doc_freq
    z = torch.zeros((1, 1), dtype=torch.long, device=dev)
    with pytest.raises(ValueError):
        doc_freq(z, z, (1 << 20) + 1)


# ------------------------------------------------------------------------------------------------ penalty
SHAPES = [(r, v) for r in (1, 3, 64, 70) for v in (1, 63, 64, 65, 257, 1027, 4100)] + [(64, 50368)]
BETA, LAM, G = 0.3, 0.013, 0.37


def penalty_inputs(R_, V, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R_, V)).astype(np.float32)
    x[rng.random((R_, V)) < 0.5] = 0.0
    x[:, ::5] = 0.0                                            # exact-zero columns
    if R_ >= 2 and V > 2:
        x[:, 2] = 0.0
        x[0, 2], x[1, 2] = 1.5, -1.5                           # a column that cancels to an exact zero mean
    w = np.exp(-4.0 * rng.random(V)).astype(np.float32)
    w[::7] = 0.0
    w[1::11] = 100.0
    return x, w


@pytest.fixture(scope="module")
def penalty_cases(dev):
    """Forward of every shape once: (x, w, out3, out3 of a second run, means, workspace) -- shared by the forward and
    backward tests and left unchanged."""
    from snx.idf import flops_means, idf_flops_fwd
    out = {}
    for (R_, V) in SHAPES:
        x, w = penalty_inputs(R_, V, R_ * 100003 + V)
        xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
        loss = torch.full((1,), 2.5, dtype=torch.float32, device=dev)
        o1, ws = idf_flops_fwd(xd, wd, BETA, LAM, loss=loss)
        o2, ws2 = idf_flops_fwd(xd, wd, BETA, LAM)
        out[(R_, V)] = dict(x=x, w=w, wd=wd, o1=o1.cpu().numpy(), o2=o2.cpu().numpy(), ws=ws,
                            mean=flops_means(ws, V).cpu().numpy(), mean2=flops_means(ws2, V).cpu().numpy(),
                            loss=float(loss))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"R{s[0]}-V{s[1]}")
def test_penalty_forward(penalty_cases, shape):
    R_, V = shape
    c = penalty_cases[shape]
    a = R.column_means_fp32(c["x"])
    assert np.array_equal(_bits(c["mean"]), _bits(a))                         # bit for bit
    s1, s2, P, a1, a2 = R.penalty(a, c["w"], BETA)
    b32 = float(np.float32(BETA))
    for name, got, want, mag in (("l1", c["o1"][0], s1, a1), ("l2", c["o1"][1], s2, a2), ("P", c["o1"][2], P, a1 + b32 * a2)):
        bound = V * 2.0 ** -52 * mag + 2.0 ** -24 * abs(want)                 # float64 accumulation + one fp32 rounding
        print(f"{name} R={R_} V={V} got={float(got)!r} want={want!r} err={abs(float(got) - want):.3e} bound={bound:.3e}")
        assert abs(float(got) - want) <= bound, (name, shape)
    assert np.array_equal(_bits(c["o1"]), _bits(c["o2"])) and np.array_equal(_bits(c["mean"]), _bits(c["mean2"]))
    # the loss scalar took fp32(lambda * P), one fp32 product and one fp32 sum
    add = np.float32(LAM) * np.float32(c["o1"][2])
    assert np.float32(c["loss"]) == np.float32(np.float32(2.5) + add)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"R{s[0]}-V{s[1]}")
def test_penalty_backward_accumulates_in_place(dev, penalty_cases, shape):
    from snx.idf import idf_flops_bwd_accum
    R_, V = shape
    c = penalty_cases[shape]
    rng = np.random.default_rng(V + R_)
    dx = rng.standard_normal((R_ + 2, V)).astype(np.float32)   # the block is a row range of a larger buffer
    buf = torch.from_numpy(dx).to(dev)
    g = torch.tensor([G], dtype=torch.float32, device=dev)
    idf_flops_bwd_accum(buf[1:R_ + 1], c["ws"], c["wd"], BETA, LAM, g)
    got = buf.cpu().numpy()
    assert np.array_equal(_bits(got[0]), _bits(dx[0])) and np.array_equal(_bits(got[-1]), _bits(dx[-1]))
    coef = R.penalty_grad_coef(c["mean"], c["w"], BETA, LAM, G, R_)
    want = dx[1:R_ + 1].astype(np.float64) + coef[None, :]
    # the kernel's expression (w * (sign + (2 beta) * a)) * ((g * lambda) / R) rounds SIX times in fp32 (2 beta is exact):
    # (2 beta) * a, sign + ., w * ., g * lambda, . / R, the last product; then the sum dx + coef rounds once
    bound = 6 * U * np.abs(coef)[None, :] + U * np.abs(want)
    err = np.abs(got[1:R_ + 1].astype(np.float64) - want)
    print(f"bwd R={R_} V={V} max err/bound={float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), shape
    zero = c["mean"] == 0
    assert zero.any()
    assert np.array_equal(_bits(got[1:R_ + 1][:, zero]), _bits(dx[1:R_ + 1][:, zero]))   # sign(0) = 0: untouched


# ------------------------------------------------------------------------------------------------ the loss
def _reps(rng, rows, V):
    x = rng.random((rows, V)).astype(np.float32)
    x[rng.random((rows, V)) < 0.7] = 0.0
    return x


@pytest.mark.parametrize("B,k,V,gathered", [(3, 1, 257, False), (8, 2, 1027, False), (4, 1, 50368, False),
                                            (3, 1, 257, True), (8, 2, 1027, True)])
def test_splade_loss_idf(dev, B, k, V, gathered):
    from snx.idf import splade_loss_idf
    from snx.loss import splade_loss
    rng = np.random.default_rng(B * 1000 + V + gathered)
    Bp, off = (2 * B, B) if gathered else (B, 0)
    q, p, n = _reps(rng, B, V), _reps(rng, Bp, V), _reps(rng, B * k, V)
    w = np.exp(-4.0 * rng.random(V)).astype(np.float32)
    w[::9] = 100.0
    lams = (0.011, 0.0031, 0.0029)
    hp = (2.0,) + lams + (0.0,)
    hp0 = (2.0, 0.0, 0.0, 0.0, 0.0)
    T = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)   # noqa: E731
    q0, p0, n0 = T(q), T(p), T(n)
    base, sc0 = splade_loss(q0, p0, n0, hp0, k, label_off=off)
    g0 = torch.autograd.grad(base * 0.5, (q0, p0, n0))
    q1, p1, n1 = T(q), T(p), T(n)
    wd = torch.from_numpy(w).to(dev)
    loss, sc = splade_loss_idf(q1, p1, n1, wd, hp, k, beta=BETA, label_off=off)
    assert tuple(sc.shape) == (18,)
    sc_h, sc0_h = sc.cpu().numpy(), sc0.cpu().numpy()
    assert np.array_equal(_bits(sc_h[1:9]), _bits(sc0_h[1:9]))            # flops_* stay the base kernel's unweighted values
    # loss = splade_loss(lambda = 0) + fp32(lambda_q P_q) + fp32(lambda_d P_p) + fp32(lambda_neg P_n), in that order
    want = np.float32(base.item())
    for s in range(3):
        want = np.float32(want + np.float32(np.float32(lams[s]) * np.float32(sc_h[11 + 3 * s])))
    assert np.float32(loss.item()) == want and np.float32(sc_h[0]) == want
    # the three P against the restatement, on the rows the kernel names
    sides = (q, p[off:off + B], n)
    means = []
    for s, x in enumerate(sides):
        a = R.column_means_fp32(x)
        means.append(a)
        s1, s2, P, a1, a2 = R.penalty(a, w, BETA)
        for got, wnt, mag in ((sc_h[9 + 3 * s], s1, a1), (sc_h[10 + 3 * s], s2, a2),
                              (sc_h[11 + 3 * s], P, a1 + float(np.float32(BETA)) * a2)):
            assert abs(float(got) - wnt) <= R.penalty_bound(V, mag, wnt), (s, got, wnt)
    # gradients = snx_loss_bwd's output + the coefficients, and the three are adjacent row ranges of ONE storage
    g1 = torch.autograd.grad(loss * 0.5, (q1, p1, n1))
    dq, dp, dn = g1
    assert dq.untyped_storage().data_ptr() == dp.untyped_storage().data_ptr() == dn.untyped_storage().data_ptr()
    assert dp.data_ptr() == dq.data_ptr() + dq.numel() * 4 and dn.data_ptr() == dp.data_ptr() + dp.numel() * 4
    assert dq.is_contiguous() and dp.is_contiguous() and dn.is_contiguous()
    rows = (slice(0, B), slice(off, off + B), slice(0, B * k))
    for s in range(3):
        got, b0 = g1[s].cpu().numpy().astype(np.float64), g0[s].cpu().numpy().astype(np.float64)
        Rs = sides[s].shape[0]
        coef = R.penalty_grad_coef(means[s], w, BETA, lams[s], 0.5, Rs)
        want_g = b0.copy()
        want_g[rows[s]] += coef[None, :]
        bound = U * np.abs(want_g)                                             # the sum's rounding
        bound[rows[s]] += 6 * U * np.abs(coef)[None, :]                        # six fp32 roundings of the coefficient
        assert (np.abs(got - want_g) <= bound).all(), s
        if gathered and s == 1:                                                # remote rows: the in-batch term alone
            assert np.array_equal(got[:off], b0[:off])


@pytest.mark.parametrize("B,k,V", [(3, 1, 257), (8, 2, 1027), (4, 1, 50368)])
def test_unit_weights_give_the_base_kernels_flops(dev, B, k, V):
    """w = 1: the penalty's quadratic sum is the base kernel's flops_* scalar, which is summed in fp32 -- V * 2^-24 * sum on
    top of the penalty's own bound."""
    from snx.idf import splade_loss_idf
    rng = np.random.default_rng(V)
    q, p, n = (torch.from_numpy(_reps(rng, r, V)).to(dev) for r in (B, B, B * k))
    w = torch.ones(V, dtype=torch.float32, device=dev)
    _, sc = splade_loss_idf(q, p, n, w, (2.0, 0.01, 0.01, 0.01, 0.0), k, beta=BETA)
    sc = sc.cpu().numpy().astype(np.float64)
    for s in range(3):
        l2, base = sc[10 + 3 * s], sc[2 + s]
        assert base > 0
        assert abs(l2 - base) <= R.penalty_bound(V, l2, l2) + V * U * l2, (s, l2, base)


# ------------------------------------------------------------------------------------------------ queries
@pytest.mark.parametrize("V", VS)
def test_query_rows_and_dense_equal_the_restatement(dev, V):
    from snx.idf import idf_query_dense, idf_query_rows
    rng = np.random.default_rng(V + 5)
    n, S = 9, 40
    ids, mask = token_rows(rng, n, S, V)
    ids[3, :] = ids[3, 0]                                      # duplicates
    ids[4, ::2] = ids[4, 1]
    allowed = (rng.random(V) < 0.8).astype(np.uint8)
    if V > 1:
        allowed[V - 1] = 1
        allowed[0] = 0                                         # the hot id is disallowed
    idf = (rng.random(V) * 9 + 0.1).astype(np.float32)
    idf[rng.random(V) < 0.1] = 0.0                             # weights a sparse row cannot hold
    idf[rng.random(V) < 0.05] = -0.25
    D = lambda a: torch.from_numpy(a).to(dev)                  # noqa: E731
    q = idf_query_dense(D(ids), D(mask), D(allowed), D(idf))
    assert np.array_equal(_bits(q.cpu().numpy()), _bits(R.query_dense(ids, mask, allowed, idf)))
    vals, term, cnt = idf_query_rows(D(ids), D(mask), D(allowed), D(idf))
    vals, term, cnt = vals.cpu().numpy(), term.cpu().numpy(), cnt.cpu().numpy()
    want = R.query_rows(ids, mask, allowed, idf)
    assert cnt[1] == 0                                         # every position masked
    for r, (terms, ws) in enumerate(want):
        assert cnt[r] == len(terms)
        assert term[r, :cnt[r]].tolist() == terms and (term[r, cnt[r]:] == -1).all()
        assert np.array_equal(_bits(vals[r, :cnt[r]]), _bits(np.asarray(ws, dtype=np.float32)))
        assert (vals[r, cnt[r]:] == 0).all()


def test_search_with_idf_rows(dev):
    from snx.idf import idf_query_rows
    from snx.retrieval import SparseIndex
    V, N, nq, S = 1027, 50, 6, 12
    rng = np.random.default_rng(50)
    idf = (rng.random(V) * 5 + 0.5).astype(np.float32)
    allowed = np.ones(V, dtype=np.uint8)
    allowed[:3] = 0
    ids = rng.integers(3, V, size=(nq, S), dtype=np.int64)
    ids[:, 3] = ids[:, 2]                                      # a repeated token weighs once
    ids[:, 0] = 1                                              # disallowed
    mask = np.ones((nq, S), dtype=np.int64)
    mask[:, -2:] = 0
    docs = np.zeros((N, V), dtype=np.float32)
    for d in range(N):
        t = rng.choice(V, size=30, replace=False)
        docs[d, t] = (rng.random(30) * 0.9 + 0.1).astype(np.float32)
    for i in range(nq):                                        # doc 7 i holds every token of query i, heavily
        docs[7 * i, ids[i, :S - 2]] = 2.0
    rows = R.query_rows(ids, mask, allowed, idf)
    sc = R.scores(rows, docs)
    order = np.sort(sc, axis=1)
    assert ((order[:, -1] - order[:, -2]) > 1e-3 * order[:, -1]).all()          # the construction separates the best
    cap = int((docs > 0).sum(1).max())
    dvals = np.zeros((N, cap), dtype=np.float32)
    dids = np.full((N, cap), -1, dtype=np.int32)
    dcnt = np.zeros(N, dtype=np.int32)
    for d in range(N):
        t = np.nonzero(docs[d])[0]
        dcnt[d] = len(t)
        dids[d, :len(t)] = t
        dvals[d, :len(t)] = docs[d, t]
    D = lambda a: torch.from_numpy(a).to(dev)                  # noqa: E731
    index = SparseIndex(V, dev)
    index.add(D(dvals), D(dids), D(dcnt))
    index.build()
    scores, got, _, _ = index.search(*idf_query_rows(D(ids), D(mask), D(allowed), D(idf)), 3)
    assert got[:, 0].cpu().numpy().tolist() == np.argmax(sc, axis=1).tolist() == [7 * i for i in range(nq)]
    best = sc.max(axis=1)
    # the index's score is a chain of at most S - 2 fp32 fmas over positive terms: one rounding each, relative to a
    # partial sum that never exceeds the result
    assert (np.abs(scores[:, 0].cpu().numpy().astype(np.float64) - best) <= S * U * best).all()
