"""Arena and weight-cache sizes of the three model runtimes (csrc/model.hip, csrc/f32_path.hip, csrc/teacher.hip), without a
GPU.  The plans are bump allocations over 256-byte boundaries (csrc/runtime.h); a caller allocates by these numbers and the
forward and backward place every buffer by the same plan, so a size that moves is an ABI change.  EXPECTED holds what the
library returned before the three files shared one allocator, recorded by running ``_sizes()`` against that build; 0 is the
answer for a geometry the runtime refuses (the tiny parity model runs on the fp32 path only)."""
import ctypes as C

import pytest

# vocab, hidden, inter, layers, heads, head_dim, global_every, window
MODELS = {
    "tiny_parity": (1000, 64, 96, 4, 4, 16, 3, 8),                # fp32 path only
    "one_layer": (300, 256, 128, 1, 4, 64, 3, 16),
    "shipped": (50368, 768, 1152, 22, 12, 64, 3, 64),
    "odd_inter": (1000, 256, 100, 2, 4, 64, 2, 16),               # fp32 path only: T * inter * 4 is no multiple of 256
    "inter_192": (1000, 256, 192, 2, 4, 64, 2, 16),               # bf16: T * inter * 2 is no multiple of 256 at odd T
}
# vocab, hidden, inter, layers, heads, head_dim, max_pos, type_vocab, pad_id
TEACHERS = {
    "golden": (300, 256, 512, 2, 4, 64, 300, 1, 1),
    "one_layer": (300, 768, 3072, 1, 12, 64, 300, 1, 1),
    "shipped": (250002, 1024, 4096, 24, 16, 64, 8194, 1, 1),
    "inter_192": (300, 256, 192, 3, 4, 64, 300, 1, 1),
}
SHAPES = ((1, 1, 1), (131, 3, 65), (16384, 64, 256))             # T, nseq, max_seqlen

# per geometry: the weight cache, then per shape the sizes in the order of _model_sizes / _teacher_sizes
EXPECTED = {
    "model": {
        "inter_192": [
            4050944, 13824, 21504, 21504, 21248, 52480, 23552, 33280, 8192, 1115392, 2073600, 2073600,
            2067200, 68616448, 1939968, 3183104, 1073152, 138086912, 257886720, 257886720, 257100288,
            227493120, 240046080, 395497472, 134217728],
        "odd_inter": [
            0, 0, 0, 0, 0, 0, 22784, 31744, 8192, 0, 0, 0, 0, 0, 1795584, 2894336, 1073152, 0, 0, 0, 0,
            0, 221958144, 359321600, 134217728],
        "one_layer": [
            1857536, 10496, 11520, 11520, 11264, 27648, 17152, 16128, 8192, 1052672, 1186816, 1186816,
            1184512, 134508544, 1822720, 1688576, 1073152, 131091968, 147869184, 147869184, 147607040,
            285796096, 227104768, 210327552, 134217728],
        "shipped": [
            520912896, 232192, 708352, 708352, 706048, 1796864, 454400, 1263104, 24576, 4479488,
            66286592, 66286592, 66010880, 138846208, 7857408, 113227776, 3219456, 497410560, 8227250688,
            8227250688, 8192778752, 882912256, 857243648, 14035484672, 402653184],
        "tiny_parity": [
            0, 0, 0, 0, 0, 0, 13312, 23808, 2048, 0, 0, 0, 0, 0, 581888, 1813248, 268288, 0, 0, 0, 0, 0,
            70176768, 224055296, 33554432],
    },
    "teacher": {
        "golden": [
            2103296, 5632, 8192, 674304, 1073152, 84279296, 134217728],
        "inter_192": [
            2171904, 5120, 6912, 590592, 905472, 73793536, 113246208],
        "one_layer": [
            14164992, 18944, 30720, 2422272, 4024320, 302907392, 503316480],
        "shipped": [
            604274688, 25088, 40960, 3229184, 5365760, 403832832, 671088640],
    },
}


def _model_sizes(geom):
    from snx import fn
    from snx.encoder import ModelDesc
    d = ModelDesc(*geom, 0, 0, 1e-5, 0.0)
    p = C.byref(d)
    out = [fn("snx_weight_cache_bytes")(p)]
    for T, nseq, maxlen in SHAPES:
        out += [fn("snx_model_workspace_bytes")(p, T, nseq, 0), fn("snx_model_workspace_bytes")(p, T, nseq, 1),
                fn("snx_model_workspace_bytes_fwd")(p, T, nseq, 1), fn("snx_model_workspace_bytes_fwd")(p, T, nseq, 3),
                fn("snx_model_bwd_workspace_bytes")(p, T, nseq, maxlen),
                fn("snx_model_workspace_bytes_f32")(p, T, nseq, 0), fn("snx_model_workspace_bytes_f32")(p, T, nseq, 1),
                fn("snx_model_bwd_workspace_bytes_f32")(p, T)]
    return [int(x) for x in out]


def _teacher_sizes(geom):
    from snx import fn
    from snx.teacher import TeacherDesc
    d = TeacherDesc(*geom, 0, 1e-5, 0.0)
    p = C.byref(d)
    out = [fn("snx_teacher_weight_cache_bytes")(p)]
    for T, nseq, _ in SHAPES:
        out += [fn("snx_teacher_workspace_bytes")(p, T, nseq, 0), fn("snx_teacher_workspace_bytes")(p, T, nseq, 1)]
    return [int(x) for x in out]


def _sizes():
    return {"model": {k: _model_sizes(g) for k, g in MODELS.items()},
            "teacher": {k: _teacher_sizes(g) for k, g in TEACHERS.items()}}


@pytest.mark.parametrize("name", list(MODELS))
def test_model_arena_and_cache_sizes_are_the_recorded_ones(name):
    got = _model_sizes(MODELS[name])
    assert got == EXPECTED["model"][name]
    bf16_ok = name not in ("tiny_parity", "odd_inter")
    assert all((x > 0) == bf16_ok for x in got[:1] + [v for i in range(len(SHAPES)) for v in got[1 + 8 * i:6 + 8 * i]])
    assert all(x > 0 and x % 256 == 0 for i in range(len(SHAPES)) for x in got[6 + 8 * i:9 + 8 * i])


@pytest.mark.parametrize("name", list(TEACHERS))
def test_teacher_arena_and_cache_sizes_are_the_recorded_ones(name):
    got = _teacher_sizes(TEACHERS[name])
    assert got == EXPECTED["teacher"][name]
    assert all(x > 0 and x % 256 == 0 for x in got)
