"""CPU checks of the two-phase dense retrieval (include/snx.h "two-phase dense retrieval") on its numpy reference,
tests/dense_two_phase_reference.py: hand-worked cases pin the rounding and the norms, and the certificate is held to its
guarantee -- a certified row IS the brute-force result, ties included -- over a few hundred seeded cases whose approximate
scores are accumulated in three different orders, with and without exclusions and a ceiling."""
import itertools

import numpy as np
import pytest

from tests import dense_reference as DR
from tests import dense_two_phase_reference as R


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the reference by hand
def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8,
                  3.4e38, 1e-40, 0.0], np.float32)
    want = [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, np.inf, 1e-40, 0.0]
    got = R.bf16_value(R.bf16_bits(x))
    assert got[:6].tolist() == want[:6]
    assert abs(float(got[6]) - 1e-40) <= 2.0 ** -134 and got[7] == 0.0    # subnormals round on the same grid


def test_prepare_pads_to_32_and_folds_from_the_left():
    X = np.array([[1.0 + 2.0 ** -8, 3.0, -0.5, 0.0, 0.0], [2.0 ** 27, 1.0, 1.0, 1.0, 1.0]], np.float32)
    bits, n2, h2, r2 = R.prepare(X)
    assert bits.shape == (2, 32) and not bits[:, 5:].any()
    assert R.bf16_value(bits[0, :3]).tolist() == [1.0, 3.0, -0.5]
    assert n2[0] == (1.0 + 2.0 ** -8) ** 2 + 9.0 + 0.25 and h2[0] == 10.25 and r2[0] == 2.0 ** -16
    # a left fold: every 1 is lost against 2^54 (ulp 4); a tree that adds the ones first would return 2^54 + 4
    assert n2[1] == 2.0 ** 54 and h2[1] == 2.0 ** 54 and r2[1] == 0.0


def test_epsilon_by_hand():
    # D = 3 (Dp = 32): bf16-exact operands leave the two accumulation terms only
    m23, m24 = 64 * 2.0 ** -23, 3 * 2.0 ** -24
    want = (m23 / (1 - m23) * 2.0 * 5.0 + m24 / (1 - m24) * 2.0 * 5.0) * (1 + 2.0 ** -20) + 3 * 2.0 ** -100 * 8.0
    assert R.epsilon(3, 4.0, 4.0, 0.0, 5.0, 5.0, 0.0) == want
    # and the bf16 terms: n_q R + r_q Nhat
    assert R.epsilon(3, 4.0, 4.0, 1.0, 5.0, 5.0, 0.5) > 2.0 * 0.5 + 1.0 * 5.0


def test_candidates_break_approximate_ties_by_doc_id_and_pad():
    A = np.array([[1.0, 3.0, 3.0, -2.0, 3.0]], np.float32)
    docs, approx = R.candidates(A, 3)
    assert docs.tolist() == [[1, 2, 4]] and approx.tolist() == [[3.0, 3.0, 3.0]]
    docs, approx = R.candidates(A, 7)
    assert docs.tolist() == [[1, 2, 4, 0, 3, -1, -1]] and approx[0, 5:].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ soundness
def _operands(rng, nq, nd, D, mode):
    """fp32 operands: "normal" rows, or "clustered": half the docs are near copies of a few rows (differences around
    bf16 precision), so that phase 1 often orders the top wrongly."""
    Q = rng.standard_normal((nq, D)).astype(np.float32)
    E = rng.standard_normal((nd, D)).astype(np.float32)
    if mode == "clustered":
        src = rng.integers(0, 4, size=nd // 2)
        E[:nd // 2] = E[nd - 1 - src] * (1.0 + rng.standard_normal((nd // 2, D)).astype(np.float32) * np.float32(2e-3))
        Q[: nq // 2] = E[nd - 1 - rng.integers(0, 4, size=nq // 2)]      # queries that look straight at a cluster
    return Q, E


CASES = list(itertools.product((3, 32, 100), (1, 7, 50), (1, 2, 4), ("ascending", "descending", "pairwise")))


@pytest.mark.parametrize("D,k,expansion,order", CASES)
def test_a_certified_row_is_the_brute_force_result(D, k, expansion, order):
    """81 parameter sets x 4 seeded shapes x 6 queries, plain and band.  Returns nothing; the tally test below reads the
    same function."""
    _soundness(D, k, expansion, order)


def _soundness(D, k, expansion, order):
    tally = np.zeros(2, np.int64)
    for rep in range(4):
        rng = np.random.default_rng([D, k, expansion, rep, len(order)])
        nd, nq = int(rng.integers(40, 401)), 6
        Q, E = _operands(rng, nq, nd, D, "clustered" if rep % 2 else "normal")
        S = DR.chain_scores(Q, E)
        # plain top k
        k1 = R.search_k1(nd, k, expansion)
        sc, dc, fd, cert = R.band_two_phase(Q, E, 0, k, k1, order=order, S=S)
        ws, wd, _, _ = DR.search(S, k)
        for q in np.nonzero(cert)[0]:
            assert np.array_equal(dc[q], wd[q]) and np.array_equal(_bits(sc[q]), _bits(ws[q])), (nd, rep, q)
        tally += (int(cert.sum()), nq)
        # band: exclusion rows of 0-8 docs taken from the top of the ranking, a ceiling that cuts into it for half the rows
        hi, lo = k, k // 3
        exclude = [sorted(rng.choice(DR.ranked(S[q])[:3 * k + 8], size=int(rng.integers(0, 9)), replace=False).tolist())
                   for q in range(nq)]
        ceiling = np.array([np.sort(S[q])[-1 - (k // 2)] if q % 2 else np.inf for q in range(nq)], np.float32)
        k1 = R.band_k1(nd, hi, max(len(r) for r in exclude), expansion)
        sc, dc, fd, cert = R.band_two_phase(Q, E, lo, hi, k1, exclude, ceiling, order=order, S=S)
        ws, wd, wf = DR.search_band(S, lo, hi, exclude, ceiling)
        for q in np.nonzero(cert)[0]:
            assert np.array_equal(dc[q], wd[q]) and np.array_equal(_bits(sc[q]), _bits(ws[q])) and fd[q] == wf[q], \
                (nd, rep, q)
        tally += (int(cert.sum()), nq)
        # exact=True is the brute-force result on every row
        sc, dc, fd, _ = R.band_two_phase(Q, E, lo, hi, k1, exclude, ceiling, exact=True, order=order, S=S)
        assert np.array_equal(dc, wd) and np.array_equal(_bits(sc), _bits(ws)) and np.array_equal(fd, wf)
    return tally


def test_the_certificate_both_grants_and_refuses():
    """The property above is empty if nothing is certified, and weak if everything is."""
    wide = _soundness(100, 7, 4, "ascending")
    tight = _soundness(100, 7, 1, "ascending")
    assert wide[0] >= wide[1] // 4, wide
    assert tight[0] < wide[0] and tight[0] < tight[1], (tight, wide)


def test_uncertified_rows_do_differ_somewhere():
    """Phase 1 alone is NOT exact: on clustered docs with k1 = k some uncertified row differs from brute force."""
    rng = np.random.default_rng(11)
    Q, E = _operands(rng, 16, 300, 32, "clustered")
    S = DR.chain_scores(Q, E)
    _, dc, _, cert = R.band_two_phase(Q, E, 0, 7, 7, S=S)
    _, wd, _, _ = DR.search(S, 7)
    wrong = [q for q in range(16) if not np.array_equal(dc[q], wd[q])]
    assert wrong and not cert[wrong].any()


# ------------------------------------------------------------------------------------------------ fixtures
def test_adversarial_twins_are_never_certified():
    Q, E, ids = R.adversarial_fixture()
    S = DR.chain_scores(Q, E)
    assert np.array_equal(S[0, ids], (32.0 + np.arange(64) * 2.0 ** -16).astype(np.float32))   # the exact scores differ
    assert S[0].argsort()[-64:].tolist() == ids.tolist()                                     # ... and lead the ranking
    Eh = R.bf16_value(R.prepare(E)[0][:, :32])
    assert (Eh[ids] == 1.0).all()                                                            # one bf16 image
    k, k1 = 10, 20
    for order in ("ascending", "descending", "pairwise"):
        A = R.approx_scores(Q, Eh, order)
        assert (A[0, ids] == 32.0).all()
        sc, dc, fd, cert = R.band_two_phase(Q, E, 0, k, k1, order=order, S=S)
        assert not cert[0]
        assert dc[0].tolist() == ids[k1 - 1:k1 - 1 - k:-1].tolist()      # the best of the 20 lowest ids: not the top 10
        sc, dc, fd, cert = R.band_two_phase(Q, E, 0, k, k1, exact=True, order=order, S=S)
        ws, wd, _, _ = DR.search(S, k)
        assert not cert[0] and np.array_equal(dc, wd) and np.array_equal(_bits(sc), _bits(ws))
        assert dc[0].tolist() == ids[:-k - 1:-1].tolist()


@pytest.mark.parametrize("D", (3, 32, 100))
@pytest.mark.parametrize("k", (1, 10, 100))
def test_grid_fixture_certifies_every_row(D, k):
    nd, nq = 1000, 9
    Q, E = R.grid_fixture(nd, D, nq, k, seed=D + k)
    bq, _, _, rq = R.prepare(Q)
    be, _, _, re = R.prepare(E)
    assert not rq.any() and not re.any()                                  # the bf16 copy is exact
    S = DR.exact_scores(Q, E)
    for order in ("ascending", "descending", "pairwise"):                 # ... and so is every partial sum
        assert np.array_equal(_bits(R.approx_scores(Q, E, order)), _bits(S))
    assert np.array_equal(_bits(DR.chain_scores(Q, E)), _bits(S))
    k1 = R.search_k1(nd, k, 2)
    sc, dc, fd, cert = R.band_two_phase(Q, E, 0, k, k1, S=S)
    assert cert.all()                                                     # certified fraction exactly 1
    ws, wd, _, _ = DR.search(S, k)
    assert np.array_equal(dc, wd) and np.array_equal(_bits(sc), _bits(ws))
    cd, _ = R.candidates(S, k1)
    ties = sum(len(np.unique(S[q, cd[q]])) < k1 for q in range(nq))
    assert k1 < 4 or ties > 0                                             # approximate ties inside the candidates


def test_all_docs_as_candidates_are_certified_and_padded():
    rng = np.random.default_rng(3)
    Q, E = _operands(rng, 5, 50, 32, "normal")
    S = DR.chain_scores(Q, E)
    k1 = R.search_k1(50, 100, 4)
    assert k1 == 100
    sc, dc, fd, cert = R.band_two_phase(Q, E, 0, 100, k1, S=S)
    ws, wd, _, _ = DR.search(S, 100)
    assert cert.all() and (fd == 50).all() and (dc[:, 50:] == -1).all() and not sc[:, 50:].any()
    assert np.array_equal(dc, wd) and np.array_equal(_bits(sc), _bits(ws))


def test_an_overflowing_bf16_copy_is_never_certified():
    Q = np.full((1, 4), 1.0, np.float32)
    E = np.zeros((40, 4), np.float32)
    E[:, 0] = np.arange(40, dtype=np.float32)
    E[7, 1] = 3.4e38                                                      # finite in fp32, an infinity in bf16
    with np.errstate(over="ignore", invalid="ignore"):
        sc, dc, fd, cert = R.band_two_phase(Q, E, 0, 3, 6)
    assert not cert[0]


def test_operands_that_could_overflow_fp32_are_never_certified():
    """Every value and every score is finite, but n_q N = 2^128: the bound's premise (no product or partial sum leaves
    the fp32 range) is not given, so no row is certified -- not even with every doc a candidate."""
    Q = np.zeros((2, 4), np.float32)
    Q[0, 0], Q[1, 1] = 2.0 ** 64, 1.0
    E = np.zeros((40, 4), np.float32)
    E[:, 1] = np.arange(40, dtype=np.float32)
    E[3, 2] = 2.0 ** 64
    S = DR.chain_scores(Q, E)
    assert np.isfinite(S).all()
    # with every doc a candidate the second query, small enough (2^64 <= 2^127), is certified; the first never is
    for k1, want in ((6, [False, False]), (40, [False, True])):
        _, _, _, cert = R.band_two_phase(Q, E, 0, 3, k1, S=S)
        assert cert.tolist() == want
