"""Host side of the fixed-dimensional encodings: FdeEncoder's argument rules and seeded operands, what MultiVectorIndex
refuses around fde=True, and the C entry points' refusals, all before any launch.  No GPU."""
import ctypes as C

import pytest
import torch

D = 64


def _rows(n, dtype=torch.bfloat16):
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(0))
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


@pytest.mark.parametrize("args", [(96, 2, 2, 16), (2048, 2, 2, 16), (64, 7, 1, 16), (64, -1, 1, 16), (64, 2, 0, 16),
                                  (64, 2, 33, 16), (64, 2, 2, 48), (64, 6, 2, 64), (64, 2.0, 2, 16), (64, True, 2, 16)])
def test_encoder_argument_ranges(args):
    from snx.retrieval import FdeEncoder
    with pytest.raises(ValueError):                            # (64, 6, 2, 64): fde_dim = 8192 > 4096
        FdeEncoder(*args, "cpu")


def test_seeded_operands_are_the_documented_recipe_and_fp32_rows_are_refused():
    from snx.retrieval import FdeEncoder
    enc = FdeEncoder(128, 3, 2, 32, "cpu", seed=5)
    planes = torch.randn(2, 3, 128, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    proj = (2 * torch.randint(0, 2, (2, 32, 128), generator=torch.Generator().manual_seed(6)) - 1).to(torch.bfloat16)
    assert enc.fde_dim == 2 * 8 * 32 and torch.equal(enc.planes, planes) and torch.equal(enc.proj, proj)
    assert set(enc.proj.float().unique().tolist()) == {-1.0, 1.0}
    given = FdeEncoder(128, 3, 2, 32, "cpu", planes=planes.float(), proj=proj)
    assert torch.equal(given.planes, planes) and given.planes.dtype == torch.bfloat16
    for bad in ({"planes": planes}, {"planes": planes[:1], "proj": proj}, {"planes": planes, "proj": proj * float("inf")}):
        with pytest.raises(ValueError):
            FdeEncoder(128, 3, 2, 32, "cpu", **bad)
    enc = FdeEncoder(D, 2, 2, 16, "cpu")
    with pytest.raises(ValueError, match="bf16"):
        enc.encode_documents(_rows(5, torch.float32), [0, 5])
    with pytest.raises(ValueError, match="ptr"):
        enc.encode_queries(_rows(5), [0, 6])
    with pytest.raises(ValueError, match="GPU"):
        enc.encode_documents(_rows(5), [0, 5])


def test_index_rules_around_fde():
    from snx.retrieval import FdeEncoder, MultiVectorIndex
    enc, q = FdeEncoder(D, 2, 2, 16, "cpu"), _rows(3)
    f32 = MultiVectorIndex(D, "cpu")
    f32.add(_rows(5, torch.float32), [0, 2, 5])
    with pytest.raises(ValueError, match="fp32"):
        f32.build().set_fde(enc)
    index = MultiVectorIndex(D, "cpu")
    index.add(_rows(5), [0, 2, 2, 5])
    with pytest.raises(RuntimeError, match="build"):
        index.set_fde(enc)
    with pytest.raises(ValueError, match="encoder"):
        index.build().set_fde(FdeEncoder(128, 2, 2, 16, "cpu"))
    with pytest.raises(RuntimeError, match="set_fde"):         # no centroids either: fde=True does not ask for them
        index.search_two_phase(q, [0, 3], 1, 2, fde=True)
    for bad in (lambda: index.candidates(q, [0, 3], 2, nprobe=2, fde=True),
                lambda: index.search_two_phase(q, [0, 3], 1, 2, nprobe=2, fde=True),
                lambda: index.search_band_two_phase(q, [0, 3], 0, 1, 2, nprobe=2, fde=True)):
        with pytest.raises(ValueError, match="nprobe"):
            bad()
    index.fde, index._fde_index = torch.zeros(3, enc.fde_dim), object()        # as set_fde leaves them
    index.add(_rows(2), [0, 2])                                # a later add invalidates the FDEs
    assert index.fde is None and index._fde_index is None


def test_fde_abi_refuses_bad_arguments_before_any_launch():
    from snx._abi import CONSTANTS
    from snx._lib import fn
    E_SHAPE, E_ARG = CONSTANTS["SNX_E_SHAPE"], CONSTANTS["SNX_E_ARG"]
    ptr, p = (C.c_int64 * 3)(0, 2, 5), 4096                    # p: an aligned address no launch will read
    sizing, packed_bytes = fn("snx_mv_fde_workspace_bytes"), fn("snx_mv_fde_packed_bytes")

    def run(dim=64, k_sim=2, reps=2, dp=16, mv_ptr=ptr, nrows=5, rows=p, packed=p, out=p, ws=p, ws_bytes=1 << 20):
        return fn("snx_mv_fde_encode")(rows, nrows, mv_ptr, 2, packed, dim, k_sim, reps, dp, 0, out, ws, ws_bytes, None)
    shapes = [dict(dim=96), dict(dim=2048), dict(k_sim=7), dict(k_sim=-1), dict(reps=0), dict(reps=33), dict(dp=48),
              dict(k_sim=6, reps=2, dp=64), dict(nrows=-1)]
    assert [run(**kw) for kw in shapes] == [E_SHAPE] * len(shapes)
    args = [dict(mv_ptr=(C.c_int64 * 3)(0, 3, 2)), dict(mv_ptr=(C.c_int64 * 3)(1, 2, 5)), dict(nrows=4), dict(mv_ptr=None),
            dict(rows=None), dict(packed=None), dict(out=None), dict(ws=None), dict(out=4100), dict(ws_bytes=8)]
    assert [run(**kw) for kw in args] == [E_ARG] * len(args)
    assert sizing(ptr, 2) >= 3 * 8 + 2 * 4 and sizing(ptr, 0) == 0 and sizing((C.c_int64 * 3)(0, 3, 2), 2) == 0
    assert packed_bytes(64, 2, 2, 16) == 3 * 64 * 64 and packed_bytes(1024, 0, 32, 64) == 32 * 3 * 1024 * 64
    assert [packed_bytes(96, 2, 2, 16), packed_bytes(64, 6, 2, 64), packed_bytes(64, 2, 2, 8)] == [0, 0, 0]
    pack = fn("snx_mv_fde_pack")
    assert pack(p, p, 64, 6, 2, 64, p, None) == E_SHAPE and pack(None, p, 64, 2, 2, 16, p, None) == E_ARG
    assert pack(p, None, 64, 2, 2, 16, p, None) == E_ARG and pack(p, p, 64, 2, 2, 16, 4100, None) == E_ARG
