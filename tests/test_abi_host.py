"""CPU checks of the header reader (snx/_abi.py): the Python layer takes every prototype, struct and constant of the C ABI
from include/snx.h.  Representative prototypes, the struct layouts and all constants are written out here by hand, so a
reader that mistypes an argument, or a header edit that moves one, fails here and not on the device."""
import ctypes as C

import pytest

P, STR, I32, I64, F32, F64, SZ, INT = (C.c_void_p, C.c_char_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t,
                                       C.c_int)

PINNED = {
    "snx_version": (INT, []),                                                        # (void)
    "snx_build_flags": (STR, []),                                                    # const char* return
    "snx_configure": (INT, [STR, I32]),                                              # const char* argument
    "snx_adamw_clip_step": (INT, [P, P, P, P, I64, P, I64, I64, I64, P, P, P]),
    "snx_gemm_f32": (INT, [P, I64, I64, P, I64, I64, P, I64, P, I64, I32, I32, I32, I32, P]),       # int64_t strides
    "snx_cooc_pmi_cells": (INT, [P, P, P, I64, I64, P, F64, F64, F64, I32, I32, F64, P, P]),       # double arguments
    "snx_sparse_index_build": (INT, [P, P, P, I32, I32, I64, P, P, P, P, SZ, P]),                  # size_t argument
    "snx_seismic_search": (INT, [P, P, P, I32, I32] + [P] * 9 + [I32, I32, P, I32, I32, F32] + [P] * 6),   # 26 arguments
    "snx_model_backward_units_range_tw": (INT, [P] * 15 + [I32] * 7 + [P, P]),                     # two streams at the end
    "snx_idf_flops_fwd": (INT, [P, I32, I32, P, F32, F32, P, P, P, P]),                            # float arguments
    "snx_gemm_tn_workspace_bytes": (SZ, [P, I32, I32]),                              # size_t return, struct pointer
    "snx_param_count": (I32, [P]),                                                   # int32_t return
}

STRUCT_FIELDS = {
    "snx_model_desc": ["vocab", "hidden", "inter", "layers", "heads", "head_dim", "global_every", "window", "pad_id",
                       "reserved0", "ln_eps", "reserved1"],
    "snx_teacher_desc": ["vocab", "hidden", "inter", "layers", "heads", "head_dim", "max_pos", "type_vocab", "pad_id",
                         "reserved0", "ln_eps", "reserved1"],
    "snx_tn_problem": ["dY", "X", "dW", "N", "K", "interleaved", "reserved"],
}

CONSTANTS = {
    "SNX_E_SHAPE": -2, "SNX_E_ARG": -3, "SNX_FWD_SAVE_FOR_BACKWARD": 1, "SNX_FWD_NO_TOKEN_WEIGHTS": 2,
    "SNX_TEACHER_BF16": 0, "SNX_TEACHER_F32": 1,
    "SNX_PRUNE_MAX_RATIO": 0, "SNX_PRUNE_ABS_VALUE": 1, "SNX_PRUNE_TOP_K": 2, "SNX_PRUNE_ALPHA_MASS": 3,
    "SNX_FUSE_RRF": 0, "SNX_FUSE_WEIGHTED_RRF": 1, "SNX_FUSE_LINEAR": 2, "SNX_BOOTSTRAP_SEGMENT": 64,
    "SNX_MINHASH_MSG_MAX": 55, "SNX_MINHASH_PERM_MAX": 256, "SNX_TFIDF_LDS_KEYS": 4096, "SNX_COOC_LDS_TOKENS": 4096,
    "SNX_COOC_LOG2": 0, "SNX_COOC_LOGE": 1, "SNX_COOC_LOGB": 2, "SNX_L2_KMAX": 256,
}


def test_representative_prototypes_are_typed_as_the_header_declares_them():
    from snx import _abi, _lib
    assert _lib.SIGNATURES is _abi.PROTOTYPES
    for name, (res, args) in PINNED.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res, name
        assert list(got_args) == args, name
    assert len(_lib.SIGNATURES["snx_seismic_search"][1]) == 26


def test_every_prototype_of_the_header_is_parsed_and_nothing_else():
    from snx import _abi
    from tests.test_host_cpu import _header_functions
    names = set(_header_functions()) - set(_abi.STRUCTS)         # the name regex may pick a struct name up
    assert len(_abi.PROTOTYPES) == len(names)
    assert set(_abi.PROTOTYPES) == names


def test_struct_layouts():
    from snx import _abi
    from snx.encoder import ModelDesc
    from snx.ops import TnProblem
    from snx.teacher import TeacherDesc
    assert sorted(_abi.STRUCTS) == sorted(STRUCT_FIELDS)
    for (name, fields), cls in zip(STRUCT_FIELDS.items(), (ModelDesc, TeacherDesc, TnProblem)):
        assert cls is _abi.STRUCTS[name] and issubclass(cls, C.Structure)
        assert [f for f, _ in cls._fields_] == fields, name
    for cls in (ModelDesc, TeacherDesc):
        assert C.sizeof(cls) == 48
        assert [t for _, t in cls._fields_] == [I32] * 10 + [F32] * 2
        assert cls.ln_eps.offset == 40
    assert C.sizeof(TnProblem) == 40 and TnProblem.N.offset == 24
    assert [t for _, t in TnProblem._fields_] == [P] * 3 + [I32] * 4
    d = ModelDesc(50000, 768, 1152, 22, 12, 64, 3, 64, 49999, 0, 1e-5, 0.0)
    assert (d.vocab, d.window, d.pad_id) == (50000, 64, 49999) and abs(d.ln_eps - 1e-5) < 1e-12


def test_constants_and_the_python_names_they_feed():
    from snx import _abi, _lib, cooc, encoder, infogain, minhash, teacher
    from snx.retrieval import hybrid, qrels, sparse, tfidf
    assert _abi.CONSTANTS == CONSTANTS
    assert (minhash.MSG_MAX, minhash.PERM_MAX) == (55, 256)
    assert cooc.LDS_TOKENS == 4096 and (cooc.LOG2, cooc.LOGE, cooc.LOGB) == (0, 1, 2)
    assert tfidf.LDS_KEYS == 4096 and qrels.BOOTSTRAP_SEGMENT == 64 and infogain.K_MAX == 256
    assert sparse.PRUNE_TYPES == {"max_ratio": 0, "abs_value": 1, "top_k": 2, "alpha_mass": 3}
    assert hybrid.FUSE_METHODS == {"rrf": 0, "weighted_rrf": 1, "linear": 2}
    assert teacher.PRECISIONS == {"bf16": 0, "fp32": 1}
    assert (encoder.SNX_FWD_SAVE_FOR_BACKWARD, encoder.SNX_FWD_NO_TOKEN_WEIGHTS) == (1, 2)
    assert sorted(_lib._CODES) == [-3, -2]
    assert _lib._CODES[-2].startswith("SNX_E_SHAPE") and _lib._CODES[-3].startswith("SNX_E_ARG")


def test_parser_on_header_snippets():
    from snx._abi import SnxLibraryError, parse
    with pytest.raises(SnxLibraryError, match="snx_odd") as e:
        parse("int snx_fine(int32_t n);\nint snx_odd(const float* x, uint16_t n, hipStream_t stream);\n")
    assert "uint16_t" in str(e.value)
    with pytest.raises(SnxLibraryError, match="snx_ret"):
        parse("bool snx_ret(void);")
    with pytest.raises(SnxLibraryError, match="snx_pair"):
        parse("typedef struct snx_pair { int32_t a; long b; } snx_pair;")
    protos, structs, consts = parse(
        "/* call snx_fake(int x); to see nothing */\n"
        "#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
        "#define SNX_NEG (-2)\n#define SNX_POS 7\n#define SNX_GUARD_\n#define SNX_HEX 0x10\n"
        "typedef struct snx_s {\n  const void* p; /* [M] */\n  float* q;\n  int32_t a, b, c;\n  float e;\n} snx_s;\n"
        "size_t snx_split(const snx_s* s /*[host]*/,\n"
        "                 const char* key, const void* data,\n"
        "                 int64_t n, double x, hipStream_t stream);\n"
        "int snx_none();\nconst char* snx_name(void);\n")
    assert protos == {"snx_split": (SZ, [P, STR, P, I64, F64, P]), "snx_none": (INT, []), "snx_name": (STR, [])}
    assert consts == {"SNX_NEG": -2, "SNX_POS": 7}
    assert list(structs) == ["snx_s"]
    assert structs["snx_s"]._fields_ == [("p", P), ("q", P), ("a", I32), ("b", I32), ("c", I32), ("e", F32)]


def test_a_missing_header_is_named(tmp_path):
    from snx._abi import SnxLibraryError, load
    path = str(tmp_path / "include" / "snx.h")
    with pytest.raises(SnxLibraryError) as e:
        load(path)
    assert path in str(e.value)


def test_call_raises_with_the_entry_points_name():
    """snx_gemm_nt_bf16 refuses K % 64 != 0 on the host, before any launch: no GPU is needed to see the code."""
    import snx
    from snx._lib import SnxError, call, check, fn
    assert snx.call is call
    one = C.c_void_p(16)
    assert fn("snx_gemm_nt_bf16")(one, one, one, 128, 128, 100, None) == -2
    with pytest.raises(SnxError, match="snx_gemm_nt_bf16 failed: SNX_E_SHAPE"):
        call("snx_gemm_nt_bf16", one, one, one, 128, 128, 100, None)
    with pytest.raises(SnxError, match="snx_gemm_nt_bf16 failed: SNX_E_ARG"):
        call("snx_gemm_nt_bf16", None, one, one, 128, 128, 128, None)
    with pytest.raises(SnxError, match="snx_gemm_nt_bf16 failed: SNX_E_SHAPE"):
        check(-2, "snx_gemm_nt_bf16")
    assert call("snx_configure", b"nt256", snx.config("nt256")) is None
