"""Host side of the probed multi-vector candidate pass: the argument rules of ``nprobe`` on MultiVectorIndex and the miner,
and of the two C entry points, all refused before any launch.  No GPU."""
import ctypes as C

import pytest
import torch

D = 64


def _rows(n, seed=0):
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=-1, keepdim=True)


def test_nprobe_argument_errors_and_add_clears_the_lists(tmp_path):
    from snx.retrieval import MultiVectorIndex
    from src.train.mining.multivector import mine_multivector_negatives
    index = MultiVectorIndex(D, "cpu")
    index.add(_rows(5), [0, 2, 2, 5])
    index.build()
    index.centroids, index.codes = _rows(2), torch.zeros(5, dtype=torch.uint16)   # as an assignment leaves them
    q = _rows(3, 1)
    for nprobe in (-1, 65, 2.0, True, "4"):
        for bad in (lambda: index.candidates(q, [0, 3], 2, nprobe=nprobe),
                    lambda: index.search_two_phase(q, [0, 3], 1, 2, nprobe=nprobe),
                    lambda: index.search_band_two_phase(q, [0, 3], 0, 1, 2, nprobe=nprobe)):
            with pytest.raises(ValueError, match="nprobe"):
                bad()
    index.list_ptr, index.list_docs = torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    index.add(_rows(2), [0, 2])                                    # a later add invalidates the lists with the codes
    assert index.list_ptr is None and index.list_docs is None and index.codes is None
    for kw in ({"nprobe": 65, "index_type": "centroid"}, {"nprobe": -1, "index_type": "centroid"}, {"nprobe": 4}):
        with pytest.raises(ValueError, match="nprobe"):
            mine_multivector_negatives([], str(tmp_path), None, None, **kw)


def test_probed_abi_refuses_bad_arguments_before_any_launch():
    from snx._abi import CONSTANTS
    from snx._lib import fn
    E_SHAPE, E_ARG = CONSTANTS["SNX_E_SHAPE"], CONSTANTS["SNX_E_ARG"]
    dptr, qptr, p = (C.c_int64 * 2)(0, 4), (C.c_int64 * 2)(0, 3), 4096        # p: an aligned address no launch will read
    lists = (C.c_int64 * 9)(0, 1, 1, 2, 2, 3, 3, 4, 4)

    def run(nprobe=2, nc=8, dim=64, ncand=4, lp=lists, list_len=4, list_docs=p, ws_bytes=1 << 30, chunk=0):
        return fn("snx_mv_candidates_probed")(p, 4, dptr, 1, p, nc, p, 0, dim, 3, qptr, 1, None, None, ncand, chunk, lp,
                                              list_docs, list_len, nprobe, p, p, p, ws_bytes, None)
    assert [run(nprobe=n) for n in (0, -1, 65)] == [E_ARG] * 3
    assert [run(nc=0), run(nc=4097), run(ncand=0), run(ncand=1025), run(chunk=63)] == [E_ARG] * 5
    assert run(lp=(C.c_int64 * 9)(0, 1, 1, 2, 1, 3, 3, 4, 4)) == E_ARG             # not monotone
    assert run(lp=(C.c_int64 * 9)(1, 1, 1, 2, 2, 3, 3, 4, 4)) == E_ARG             # does not start at 0
    assert [run(list_len=5), run(list_len=3), run(lp=None), run(list_docs=None)] == [E_ARG] * 4
    assert [run(dim=96), run(dim=2048)] == [E_SHAPE] * 2 and run(ws_bytes=16) == E_ARG
    sizing = fn("snx_mv_candidates_probed_workspace_bytes")
    assert sizing(qptr, 1, 1, 8, 4, 0, 2) > 16 * 8 * 2
    assert [sizing(qptr, 1, 1, 8, 4, 0, n) for n in (0, 65)] == [0, 0] and sizing(qptr, 1, 1, 0, 4, 0, 2) == 0
    assert sizing((C.c_int64 * 2)(0, 0), 1, 1, 8, 4, 0, 2) == 0 and sizing(qptr, 1, 1, 8, 4, 63, 2) == 0
    build, bsize = fn("snx_mv_lists_build"), fn("snx_mv_lists_workspace_bytes")
    assert bsize(4, 8) > 0 and [bsize(-1, 8), bsize(4, 0), bsize(4, 4097)] == [0, 0, 0]
    assert [build(p, 4, dptr, 1, nc, p, p, p, 1 << 30, None) for nc in (0, 4097)] == [E_ARG] * 2
    assert build(p, 4, dptr, 1, 8, None, p, p, 1 << 30, None) == E_ARG and build(p, 4, dptr, 1, 8, p, p, p, 16, None) == E_ARG
    assert build(p, 4, (C.c_int64 * 2)(0, 5), 1, 8, p, p, p, 1 << 30, None) == E_ARG    # doc_ptr past the rows
