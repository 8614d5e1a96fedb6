"""Host side of the residual-compressed multi-vector store: the argument rules of MultiVectorIndex.compress and of the rows'
release, the miner's nbits, and snx_mv_rescore_residual's refusals before any launch.  No GPU."""
import ctypes as C

import pytest
import torch

from tests.test_mv_centroid_host import D, _rows


def _index(dtype=torch.bfloat16):
    from snx.retrieval import MultiVectorIndex
    index = MultiVectorIndex(D, "cpu")
    index.add(_rows(5).to(dtype), [0, 2, 2, 5])
    return index.build()


def test_compress_argument_errors():
    index = _index()
    with pytest.raises(RuntimeError, match="centroids"):
        index.compress(2)                                          # before the centroids exist
    index.centroids, index.codes = _rows(2).bfloat16(), torch.zeros(5, dtype=torch.uint16)
    for nbits in (0, 3, 8, 2.0, True):
        with pytest.raises(ValueError, match="nbits"):
            index.compress(nbits)
    cut, w = [-0.1, 0.0, 0.1], [-0.2, -0.05, 0.05, 0.2]
    for c, ww in ((cut[::-1], w), ([0.0, 0.0, 0.1], w), (cut[:2], w), (cut, w[:3]), (cut, None), (None, w),
                  ([float("nan")] + cut[1:], w)):
        with pytest.raises(ValueError):
            index.compress(2, c, ww)
    with pytest.raises(ValueError, match="GPU"):
        index.compress(2, cut, w)                                  # everything else is in order
    with pytest.raises(RuntimeError):
        index.decompress([0])
    fp32 = _index(torch.float32)
    fp32.centroids, fp32.codes = _rows(2), torch.zeros(5, dtype=torch.uint16)
    with pytest.raises(ValueError, match="fp32"):
        fp32.compress(2)


def test_released_rows_and_add():
    index, q = _index(), _rows(3, 1).bfloat16()
    index.centroids, index.codes = _rows(2).bfloat16(), torch.zeros(5, dtype=torch.uint16)
    index.residuals, index.nbits = torch.zeros(5, D // 4, dtype=torch.uint8), 2     # as compress(2, keep_rows=True) leaves them
    index.add(_rows(2).bfloat16(), [0, 2])                          # a later add clears the compression with the codes
    assert index.residuals is None and index.nbits == 0 and index.codes is None and index.cutoffs is None
    index.build()
    index.residuals, index.nbits, index.rows, index._parts = torch.zeros(7, D // 4, dtype=torch.uint8), 2, None, []
    assert index.built                                              # as compress(2) leaves them: the rows are gone
    for call in (lambda: index.search(q, [0, 3], 1), lambda: index.search_band(q, [0, 3], 0, 1),
                 lambda: index.train_centroids(2), lambda: index.set_centroids(_rows(2)), lambda: index.compress(2),
                 lambda: index.add(_rows(2).bfloat16(), [0, 2])):
        with pytest.raises(RuntimeError, match="keep_rows"):
            call()


def test_miner_refuses_bad_nbits(tmp_path):
    from src.train.mining.multivector import mine_multivector_negatives
    for kw in ({"nbits": 3, "index_type": "centroid"}, {"nbits": 2, "index_type": "exact"}):
        with pytest.raises(ValueError, match="nbits"):
            mine_multivector_negatives([], str(tmp_path), None, None, **kw)


def test_rescore_residual_refuses_on_the_host():
    from snx._lib import CONSTANTS, fn
    E_SHAPE, E_ARG = CONSTANTS["SNX_E_SHAPE"], CONSTANTS["SNX_E_ARG"]
    dptr, qptr, p = (C.c_int64 * 2)(0, 4), (C.c_int64 * 2)(0, 3), 4096        # p: an aligned address no launch will read

    def run(nbits=2, nc=8, f32=0, dim=64, ncand=4, lo=0, hi=2, codes=p, weights=p, out=p, ws_bytes=1 << 30, qp=qptr):
        return fn("snx_mv_rescore_residual")(codes, p, p, weights, nc, nbits, p, f32, dim, 4, dptr, 1, 3, qp, 1, p, ncand, lo,
                                             hi, out, p, p, None, p, ws_bytes, None)
    assert [run(nbits=b) for b in (0, 3, 8)] == [E_ARG] * 3
    assert [run(lo=-1), run(lo=2, hi=2), run(hi=5), run(ncand=0), run(ncand=1025)] == [E_ARG] * 5
    assert [run(nc=0), run(nc=4097), run(f32=1)] == [E_ARG] * 3
    assert [run(codes=None), run(weights=None), run(out=None)] == [E_ARG] * 3
    assert [run(dim=96), run(dim=2048)] == [E_SHAPE] * 2
    assert run(qp=(C.c_int64 * 2)(0, 0)) == E_ARG and run(ws_bytes=16) == E_ARG
    sizing = fn("snx_mv_rescore_residual_workspace_bytes")
    assert sizing(qptr, 1, 1, 8, 4) > 8 * 64 * 4 and sizing(qptr, 1, 1, 0, 4) == 0 and sizing(qptr, 1, 1, 8, 1025) == 0
    assert fn("snx_mv_residual_encode")(p, 1, p, p, 8, 64, 3, p, p, None) == E_ARG
    assert fn("snx_mv_residual_encode")(p, 1, p, p, 8, 96, 2, p, p, None) == E_SHAPE
