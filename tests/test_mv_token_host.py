"""Host side of multi-vector token retrieval: the argument rules of ``search_tokens`` / ``search_band_tokens`` and of the
miner's ``index_type="token"``, and the refusals of the two C entry points before any launch.  No GPU."""
import ctypes as C
import json

import pytest
import torch

from tests.test_mv_centroid_host import D, _rows, _StubIndex


def test_token_argument_errors_and_invalidation():
    from snx.retrieval import MultiVectorIndex
    q = _rows(3, 1).to(torch.bfloat16)
    index = MultiVectorIndex(D, "cpu")
    index.add(_rows(5).to(torch.bfloat16), [0, 2, 2, 5])
    index.build()
    index.centroids, index.codes = _rows(2).to(torch.bfloat16), torch.zeros(5, dtype=torch.uint16)
    for call in (lambda **kw: index.search_tokens(q, [0, 3], kw.get("k", 2), kw.get("nprobe", 2)),
                 lambda **kw: index.search_band_tokens(q, [0, 3], 0, kw.get("k", 2), kw.get("nprobe", 2))):
        with pytest.raises(RuntimeError, match=r"compress\(\)"):
            call()                                                 # not compressed
        for nprobe in (0, -1, 65, 2.0, True):
            with pytest.raises(ValueError, match="nprobe"):
                call(nprobe=nprobe)
        for k in (0, 1025):
            with pytest.raises(ValueError):
                call(k=k)
    with pytest.raises(ValueError):
        index.search_band_tokens(q, [0, 3], 2, 2, 2)
    index.residuals, index.nbits = torch.zeros(5, D // 8, dtype=torch.uint8), 1    # as compress() leaves them
    index.row_list_ptr = index.row_list = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        index.search_tokens(q, [0, 3], 2, 2)                       # compressed, but the search itself needs a GPU
    index.add(_rows(2).to(torch.bfloat16), [0, 2])                 # a later add invalidates the row lists
    assert index.row_list_ptr is None and index.row_list is None and index.residuals is None
    f32 = MultiVectorIndex(D, "cpu")
    f32.add(_rows(5), [0, 2, 2, 5])
    f32.build()
    with pytest.raises(ValueError, match="fp32"):
        f32.search_tokens(_rows(3, 1), [0, 3], 2, 2)


def test_token_abi_refuses_bad_arguments_before_any_launch():
    from snx._abi import CONSTANTS
    from snx._lib import fn
    E_SHAPE, E_ARG = CONSTANTS["SNX_E_SHAPE"], CONSTANTS["SNX_E_ARG"]
    dptr, qptr, p = (C.c_int64 * 2)(0, 4), (C.c_int64 * 2)(0, 3), 4096        # p: an aligned address no launch will read
    lists = (C.c_int64 * 9)(0, 1, 1, 2, 2, 3, 3, 4, 4)

    def run(nprobe=2, nc=8, nbits=2, f32=0, dim=64, lo=0, hi=4, dp=dptr, qp=qptr, lp=lists, q=p, bits=p, rl=p,
            ws_bytes=1 << 30):
        return fn("snx_mv_token_search")(p, bits, p, p, nc, nbits, q, f32, dim, 4, dp, 1, lp, rl, p, 3, qp, 1, None, None,
                                         nprobe, lo, hi, p, p, p, p, ws_bytes, None)
    assert [run(dim=96), run(dim=2048), run(dim=0)] == [E_SHAPE] * 3
    assert [run(nprobe=n) for n in (0, -1, 65)] == [E_ARG] * 3
    assert [run(nc=0), run(nc=4097), run(nbits=3), run(nbits=0), run(f32=1)] == [E_ARG] * 5
    assert [run(lo=-1), run(lo=4), run(hi=1025)] == [E_ARG] * 3
    assert [run(q=None), run(q=4100), run(bits=4104), run(rl=None), run(ws_bytes=16)] == [E_ARG] * 5
    assert run(lp=(C.c_int64 * 9)(0, 1, 1, 2, 1, 3, 3, 4, 4)) == E_ARG             # not monotone
    assert run(lp=(C.c_int64 * 9)(1, 1, 1, 2, 2, 3, 3, 4, 4)) == E_ARG             # does not start at 0
    assert run(lp=(C.c_int64 * 9)(0, 1, 1, 2, 2, 3, 3, 3, 3)) == E_ARG             # does not end at the row count
    assert run(dp=(C.c_int64 * 2)(0, 5)) == E_ARG and run(qp=(C.c_int64 * 2)(0, 4)) == E_ARG      # past the rows
    assert run(qp=(C.c_int64 * 2)(0, 0)) == E_ARG                                   # a query without rows
    sizing = fn("snx_mv_token_search_workspace_bytes")
    assert sizing(qptr, 1, 1, 4, 8, 2, 4) > 3 * 3 * 8
    assert [sizing(qptr, 1, 1, 4, 8, n, 4) for n in (0, 65)] == [0, 0]
    assert [sizing(qptr, 1, 1, 4, 0, 2, 4), sizing(qptr, 1, 1, 4, 4097, 2, 4), sizing(qptr, 1, 1, 4, 8, 2, 1025)] == [0] * 3
    assert sizing((C.c_int64 * 2)(0, 0), 1, 1, 4, 8, 2, 4) == 0 and sizing(qptr, 1, -1, 4, 8, 2, 4) == 0


class _TokenStub(_StubIndex):
    def compress(self, nbits):
        self.calls.append(("compress", nbits))

    def search_band_tokens(self, qmv, q_ptr, lo, hi, nprobe, exclude=None):
        self.calls.append(("token", lo, hi, nprobe))
        return self._band(len(q_ptr) - 1, lo, hi, exclude)


def test_mine_token_rules_and_layout(tmp_path):
    from src.train.mining.multivector import mine_multivector_negatives
    texts = {f"d{i}": _rows(2, 10 + i) for i in range(6)}
    texts.update({"qa": _rows(1, 40), "qb": _rows(2, 50)})
    recs = [{"query": "qa", "positive": "d0"}] + [{"query": "qb", "positive": f"d{i}"} for i in range(1, 6)]
    src = tmp_path / "in" / "train_0.jsonl"
    src.parent.mkdir()
    src.write_text("".join(json.dumps(r) + "\n" for r in recs))

    def encode_mv(batch):
        ptr = torch.tensor([0] + [len(texts[t]) for t in batch]).cumsum(0)
        return None, ptr, torch.cat([texts[t] for t in batch])

    outs = {}
    for kind, kw in (("exact", {}), ("token", {"nbits": 2, "nprobe": 4})):
        stub = _TokenStub()
        counts = mine_multivector_negatives([str(src)], str(tmp_path / kind), encode_mv, stub, k=2, rank_start=1,
                                            rank_end=3, index_type=kind, ncentroids=16, **kw)
        outs[kind] = (counts, (tmp_path / kind / "train_0.jsonl").read_text(), stub.calls)
    assert outs["exact"][:2] == outs["token"][:2]
    assert outs["token"][2] == [("train", 16), ("compress", 2), ("token", 1, 3, 4)]
    for kw in ({"nbits": 0, "nprobe": 4}, {"nbits": 3, "nprobe": 4}, {"nbits": 2, "nprobe": 0}, {"nbits": 2, "nprobe": 65},
               {"nbits": 2, "nprobe": 4, "ncand": 128}):
        with pytest.raises(ValueError):
            mine_multivector_negatives([str(src)], str(tmp_path / "x"), encode_mv, _TokenStub(), index_type="token", **kw)
