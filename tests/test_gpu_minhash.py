"""GPU checks of MinHash near-duplicate removal (csrc/minhash.hip, include/snx.h "MinHash near-duplicate removal"):
snx.minhash, src.preprocessing.cleaners.MinHashDeduplicator and nothing else.

Every comparison is integer equality: signatures against the hashlib restatement (tests/minhash_reference.py) and against
what the reference's own class produced (tests/golden/g16); the matcher on signatures built directly as uint32 arrays, so
that the number of equal positions of every pair is known exactly."""
import json
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import minhash_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16 = os.path.join(ROOT, "tests", "golden", "g16")
Triplet = namedtuple("Triplet", "query positive")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g16():
    with open(os.path.join(G16, "rows.json"), encoding="utf-8") as f:
        rec = json.load(f)
    rec["rows"] = [tuple(r) for r in rec["rows"]]
    rec["signatures"] = dict(np.load(os.path.join(G16, "signatures.npz")))
    return rec


def _host(sig) -> np.ndarray:
    return sig.view(torch.int32).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. signatures
LONG = " ".join(f"word{i} é한" for i in range(40))            # > 256 n-grams: several staging passes of 64
EDGE = [
    "",                                                      # the single n-gram is the empty text
    "a", "ab", "abc", "abcd",                                # shorter than, exactly, one more than ngram_size 3
    "aé한\U0001F600я mixed 1-, 2-, 3- and 4-byte code points",
    "UPPER İSTANBUL İ case",                                 # lower() changes the length
    "   blanks at both ends \t\n",
    "zzzzzzzzzzzz",                                          # a set of one n-gram
    "\U0001F600\U0001F601\U0001F602\U0001F603\U0001F604\U0001F605\U0001F606\U0001F607\U0001F608\U0001F609"
    "\U0001F60A\U0001F60B\U0001F60C\U0001F60D",              # 14 four-byte code points
    "the quick brown fox jumps over the lazy dog 0123456789 ABCDEFGHIJ",
    LONG,
]
# (num_perm, ngram_size): prefixes of 1, 2 and 3 digits at 128; 100 and 16; ngram_size 12 of four-byte code points is a
# 52-byte message, 51 ASCII bytes behind "127_" the 55 that just fit
SIG_CASES = [(128, 3), (100, 3), (16, 3), (128, 2), (128, 5), (128, 12), (128, 51), (100, 52), (1, 1)]


@pytest.mark.parametrize("num_perm,ngram", SIG_CASES)
def test_signatures_equal_the_restatement(dev, num_perm, ngram):
    from snx.minhash import minhash_signatures
    texts = EDGE if ngram < 20 else [t for t in EDGE if len(t.encode()) == len(t)]     # ASCII only at 51 and 52
    got = minhash_signatures(texts, num_perm, ngram, device=dev)
    assert got.dtype == torch.uint32 and tuple(got.shape) == (len(texts), num_perm, 4) and got.device == dev
    want = R.signatures(texts, num_perm, ngram)
    assert np.array_equal(_host(got), want)


def test_signatures_equal_the_reference_and_are_deterministic(dev, g16):
    from snx.minhash import minhash_signatures
    texts = [f"{q} {p}" for q, p in g16["rows"]]
    for num_perm, ngram in ((128, 3), (100, 2), (16, 5)):
        got = minhash_signatures(texts, num_perm, ngram, device=dev)
        assert np.array_equal(_host(got), g16["signatures"][f"p{num_perm}_n{ngram}"])
        assert torch.equal(got.view(torch.int32), minhash_signatures(texts, num_perm, ngram, device=dev).view(torch.int32))


def test_signatures_of_no_row_one_row_and_an_over_long_ngram(dev):
    from snx.minhash import minhash_signatures
    assert tuple(minhash_signatures([], device=dev).shape) == (0, 128, 4)
    one = minhash_signatures(["just one row"], device=dev)
    assert np.array_equal(_host(one), R.signatures(["just one row"]))
    with pytest.raises(ValueError, match="minhash_signatures: the longest message .* has 56 bytes"):
        minhash_signatures(["\U0001F600" * 13], 128, 13, device=dev)


# ------------------------------------------------------------------------------------------------ 2. matcher
def _random(rng, n, P=128):
    return rng.integers(0, 2 ** 32, size=(n, P, 4), dtype=np.uint32)


def _differ(sig, positions):
    """A copy of one signature [P, 4] that differs from it at exactly ``positions``, in the MOST significant word only."""
    out = sig.copy()
    out[positions, 0] ^= np.uint32(0x80000000)
    return out


def _dedup(sig, need, dev, group=None):
    from snx.minhash import greedy_dedup
    got = greedy_dedup(torch.from_numpy(sig.view(np.int32)).to(dev).view(torch.uint32), need, group)
    assert got.dtype == torch.int32 and got.device == dev
    return got.cpu().numpy()


def test_exactly_need_matches_decide(dev):
    rng = np.random.default_rng(1)
    a = _random(rng, 1)[0]
    for equal, want in ((103, [-1, 0]), (102, [-1, -1])):
        sig = np.stack([a, _differ(a, np.arange(equal, 128))])
        assert _dedup(sig, 103, dev).tolist() == want
        assert R.greedy(sig, 103).tolist() == want


def test_low_words_alone_do_not_decide(dev):
    rng = np.random.default_rng(2)
    a = _random(rng, 1)[0]
    for word in (0, 1, 2):                                   # equal in the least significant word at every position
        b = a.copy()
        b[:, word] += np.uint32(1)
        assert _dedup(np.stack([a, b]), 103, dev).tolist() == [-1, -1]
    assert _dedup(np.stack([a, a]), 128, dev).tolist() == [-1, 0]


def test_identical_rows_keep_only_the_first(dev):
    from snx.minhash import DEDUP_BLOCK
    rng = np.random.default_rng(3)
    n = DEDUP_BLOCK + 90                                     # the second block finds row 0 among the kept rows
    sig = np.repeat(_random(rng, 1, 16), n, axis=0)
    assert _dedup(sig, 13, dev).tolist() == [-1] + [0] * (n - 1)


def _chain(rng):
    a = _random(rng, 1)[0]
    b = _differ(a, np.arange(0, 25))                         # a ~ b: 103 equal
    c = _differ(b, np.arange(103, 128))                      # b ~ c: 103 equal; a, c: positions 25 .. 102, 78 equal
    return a, b, c


def test_chain_inside_a_block_and_across_a_boundary(dev):
    from snx.minhash import DEDUP_BLOCK as B
    rng = np.random.default_rng(4)
    a, b, c = _chain(rng)
    assert _dedup(np.stack([a, b, c]), 103, dev).tolist() == [-1, 0, -1]        # b goes, so c stays
    assert _dedup(np.stack([b, a, c]), 103, dev).tolist() == [-1, 0, 0]         # b kept: both go
    sig = _random(rng, B + 2)
    sig[0], sig[B - 1], sig[B] = a, b, c                     # b is the block's last row, c the next block's first
    want = np.full(B + 2, -1)
    want[B - 1] = 0
    assert _dedup(sig, 103, dev).tolist() == want.tolist()
    sig[0], sig[B - 1] = b, a                                # b kept in the first block: c goes across the boundary
    want[B] = 0
    assert _dedup(sig, 103, dev).tolist() == want.tolist()
    assert R.greedy(sig, 103).tolist() == want.tolist()


def test_smallest_kept_row_and_exact_group_override(dev):
    from snx.minhash import DEDUP_BLOCK as B
    rng = np.random.default_rng(5)
    a = _random(rng, 1)[0]
    a2 = _differ(a, np.arange(0, 30))                        # 98 equal: a and a2 are both kept
    x = a.copy()
    x[:15] = a2[:15]                                         # 113 equal with a, 15 + 98 = 113 with a2
    near = np.stack([a2, a, x])
    assert _dedup(near, 103, dev).tolist() == [-1, -1, 0]
    far = _random(rng, B + 40)
    far[3], far[7], far[B + 20] = a2, a, x                   # the same through the kept rows of an earlier block
    want = np.full(B + 40, -1)
    want[B + 20] = 3
    assert _dedup(far, 103, dev).tolist() == want.tolist()
    # the exact key of a kept row comes first, whatever the signatures say
    assert _dedup(near, 103, dev, group=np.array([0, 1, 1])).tolist() == [-1, -1, 1]
    group = np.arange(B + 40)
    group[B + 20] = 7
    want[B + 20] = 7
    assert _dedup(far, 103, dev, group=group).tolist() == want.tolist()
    # a key alone drops a row; the key of a DROPPED row drops nothing
    r = _random(rng, 4)
    r[1] = _differ(r[0], np.arange(0, 5))                    # row 1 goes by signature and never becomes its key's keeper
    got = _dedup(r, 103, dev, group=np.array([0, 1, 1, 0]))
    assert got.tolist() == [-1, 0, -1, 0] and R.greedy(r, 103, np.array([0, 1, 1, 0])).tolist() == got.tolist()


@pytest.fixture(scope="module")
def planted():
    """2 * block + 1 rows of 16 positions with planted near and exact duplicates, and the restatement's answers for every
    prefix length the tests use."""
    from snx.minhash import DEDUP_BLOCK as B
    rng = np.random.default_rng(6)
    n = 2 * B + 1
    sig = _random(rng, n, 16)
    src = rng.integers(0, n, size=n)
    for i in rng.permutation(n)[: n // 3]:                   # a third of the rows copy an earlier row, 0 .. 5 positions off
        if src[i] < i:
            sig[i] = _differ(sig[src[i]], rng.permutation(16)[: rng.integers(0, 6)])
    group = np.arange(n)
    for i in rng.permutation(n)[: n // 10]:
        if src[i] < i:
            group[i] = group[src[i]]
    sizes = (B - 1, B, B + 1, 2 * B + 1)
    return sig, group, {m: (R.greedy(sig[:m], 13), R.greedy(sig[:m], 13, group[:m])) for m in sizes}


@pytest.mark.parametrize("blocks,extra", [(1, -1), (1, 0), (1, 1), (2, 1)])
def test_sizes_around_the_block(dev, planted, blocks, extra):
    from snx.minhash import DEDUP_BLOCK as B
    sig, group, want = planted
    m = blocks * B + extra
    plain, keyed = want[m]
    assert 0 < (plain >= 0).sum() < m and (plain != keyed).any()
    assert _dedup(sig[:m], 13, dev).tolist() == plain.tolist()
    assert _dedup(sig[:m], 13, dev, group=group[:m]).tolist() == keyed.tolist()
    if (blocks, extra) == (2, 1):                            # determinism: a second run gives the same answer
        assert _dedup(sig[:m], 13, dev, group=group[:m]).tolist() == keyed.tolist()


def test_need_zero_and_need_above_num_perm(dev):
    from snx.minhash import DEDUP_BLOCK as B
    rng = np.random.default_rng(7)
    sig = _random(rng, B + 5, 16)
    assert _dedup(sig, 0, dev).tolist() == [-1] + [0] * (B + 4)                  # every row matches row 0
    same = np.repeat(sig[:1], B + 5, axis=0)
    assert _dedup(same, 17, dev).tolist() == [-1] * (B + 5)                      # nothing goes by signature
    assert _dedup(same, 17, dev, group=np.zeros(B + 5, np.int64)).tolist() == [-1] + [0] * (B + 4)
    assert _dedup(sig[:0], 13, dev).tolist() == [] and _dedup(sig[:1], 13, dev).tolist() == [-1]


def test_first_match(dev):
    from snx.minhash import first_match
    rng = np.random.default_rng(8)
    kept = _random(rng, 300)
    q = _random(rng, 3)
    q[0] = _differ(kept[200], np.arange(0, 25))              # 103 with row 200 ...
    kept[77] = _differ(q[0], np.arange(100, 125))            # ... and with row 77: the smaller
    q[1] = _differ(kept[5], np.arange(0, 26))                # 102: none
    t = lambda x: torch.from_numpy(x.view(np.int32)).to(dev).view(torch.uint32)  # noqa: E731
    assert first_match(t(q), t(kept), 103).tolist() == [77, -1, -1]
    assert first_match(t(q), None, 103).tolist() == [-1, -1, -1]
    assert first_match(t(q), t(kept), 0).tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ 3. the class
@pytest.mark.parametrize("setting", [(128, 0.8, 3), (128, 0.5, 3), (100, 0.8, 2), (16, 1.0, 5)])
def test_deduplicator_gives_the_references_lists(dev, g16, setting):
    from src.preprocessing.cleaners import MinHashDeduplicator
    num_perm, threshold, ngram = setting
    rows = [Triplet(q, p) for q, p in g16["rows"]]
    want = g16["kept"][f"{num_perm},{threshold},{ngram}"]
    d = MinHashDeduplicator(num_perm=num_perm, threshold=threshold, ngram_size=ngram)
    d.device = dev
    assert d.deduplicate(rows) == [rows[i] for i in want]
    ref_dup, ref_sig = R.deduplicate(g16["rows"], num_perm, threshold, ngram)
    assert d.duplicate_of.dtype == np.int32 and d.duplicate_of.tolist() == ref_dup.tolist()
    assert np.array_equal(_host(d.signatures), ref_sig)
    # the batch's kept rows stay: every row of the batch is now a duplicate, a new pair is not
    assert all(d.is_duplicate(t.query, t.positive) for t in rows[:6])
    assert not d.is_duplicate("a pair nobody has seen", "and its positive text") and \
        d.is_duplicate("A pair nobody has seen ", " and its positive text")
    # incremental: the same sequence one row at a time, and again after clear()
    for _ in range(2):
        d.clear()
        assert [i for i, t in enumerate(rows) if not d.is_duplicate(t.query, t.positive)] == want
    assert d.deduplicate(rows) == [rows[i] for i in want]    # determinism
