"""CPU: the ctypes binding is derived from the C headers (``_lib.parse_header``).  The parser on a synthetic header, literal
pins on the real ones (typed here, not computed, so a parser regression cannot hide), and the constants."""
import ctypes as C

import pytest

from cvpr22_cross_modal_pseudo_labeling_amd import _lib

SYNTHETIC = """
/* int ovis_in_a_comment(short x); */
#ifndef OVIS_DEMO_H
#define OVIS_DEMO_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define OVIS_PLAIN 7
#define OVIS_NEGATIVE (-3)   /* a comment behind it */
// int ovis_in_a_line_comment(short x);
const char* ovis_name(void);
size_t ovis_empty();
int ovis_values(int a, long b, float c, size_t d, uint64_t e);
int ovis_pointers(const void* a, float* b, const double* c, int32_t* d, const int64_t* e, uint32_t* f, uint64_t* g,
                  const uint8_t* h, const float* const* i,
                  float** j);
int ovis_arrays(const float mean[3], float std[], void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    vp = C.c_void_p
    signatures, constants = _lib.parse_header(SYNTHETIC)
    assert signatures == {
        "ovis_name": (C.c_char_p, []),
        "ovis_empty": (C.c_size_t, []),
        "ovis_values": (C.c_int, [C.c_int, C.c_long, C.c_float, C.c_size_t, C.c_uint64]),
        "ovis_pointers": (C.c_int, [vp] * 10),      # a multi-line prototype
        "ovis_arrays": (C.c_int, [vp, vp, vp]),
    }
    assert constants == {"OVIS_PLAIN": 7, "OVIS_NEGATIVE": -3}   # the include guard has no value: not a constant


@pytest.mark.parametrize("line, names", [
    ("int ovis_bad(int n, short x);", ("ovis_bad", "parameter 1")),
    ("int ovis_bad(unsigned int n);", ("ovis_bad", "parameter 0")),
    ("int ovis_bad(char* text);", ("ovis_bad", "parameter 0")),
    ("int ovis_bad(struct item* p);", ("ovis_bad", "parameter 0")),
    ("int ovis_bad(int& n);", ("ovis_bad", "parameter 0")),
    ("short ovis_bad(int n);", ("ovis_bad", "return type")),
    ("void* ovis_bad(int n);", ("ovis_bad", "return type")),
    ("int ovis_bad(int (*callback)(int));", ()),       # not a prototype this parser reads: left over, refused
    ("typedef int ovis_t;", ()),
])
def test_parser_refuses_what_it_does_not_know(line, names):
    with pytest.raises(TypeError) as err:
        _lib.parse_header("int ovis_good(int n);\n" + line + "\n")
    for name in names:
        assert name in str(err.value)


def test_real_headers_literal_pins():
    i, l, f, vp = C.c_int, C.c_long, C.c_float, C.c_void_p
    s = _lib.SIGNATURES
    assert s["ovis_version"] == (C.c_char_p, [])
    assert s["ovis_nms_workspace_bytes"] == (C.c_size_t, [i])
    assert s["ovis_sample_fg_bg"][1][4] is C.c_uint64 and len(s["ovis_sample_fg_bg"][1]) == 9
    box = s["ovis_box_decode_f32"][1]
    assert [box[k] for k in (1, 3, 4)] == [l, l, l] and box[6:11] == [f] * 5 and len(box) == 16
    assert s["ovis_split_gemm_pair_gated_ws"] == (i, [vp, l, vp, l, vp, l, vp, l, vp, l, l] + [i] * 7 + [vp, C.c_size_t, i, vp])
    assert "ovis_split_gemm_pair_gated" not in s and "ovis_gate_split_pair_f32" not in s
    from cvpr22_cross_modal_pseudo_labeling_amd import _cpu

    assert _cpu.SIGNATURES["ovis_cpu_nms_f32"] == (i, [vp, vp, i, f, vp])
    assert _cpu.SIGNATURES["ovis_cpu_transform_images_u8"] == (i, [vp, l, vp, i, vp, vp, i, i, i, vp, i])
    assert _cpu.SIGNATURES["ovis_cpu_version"] == (C.c_char_p, [])
    assert _cpu.CONSTANTS == {"OVIS_CPU_OK": 0, "OVIS_CPU_EINVAL": -1, "OVIS_CPU_ERANGE": -3}


def test_constants_come_from_the_header():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    assert (_lib.OVIS_OK, _lib.OVIS_EINVAL, _lib.OVIS_ENOSPC, _lib.OVIS_ERANGE) == (0, -1, -2, -3)
    assert _lib.OVIS_BOX_DECODE_MAX_IMAGES == 16
    assert _lib.OVIS_VIEW_MERGE_MAX_SEGMENTS == 64 and _lib.OVIS_VIEW_MERGE_TILE_ROWS == 64
    assert _C.NMS_MAX_CANDIDATES == _lib.OVIS_NMS_MAX_CANDIDATES == 131072
    with pytest.raises(RuntimeError, match=r"OVIS_ERANGE \(problem size not supported by the kernel\)"):
        _lib.check(-3, "op")
    with pytest.raises(RuntimeError, match=r"OVIS_EINVAL \(bad size or null pointer\)"):
        _lib.check(-1, "op")
    with pytest.raises(RuntimeError, match="HIP error 700"):
        _lib.check(700, "op")
    _lib.check(0, "op")


def test_every_bound_symbol_takes_its_declared_types():
    """``load()`` sets restype / argtypes of every exported function to the derived table: a wrong argument count or a
    float for an int is refused by ctypes before anything is launched."""
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    with pytest.raises(C.ArgumentError):
        lib.ovis_nms_workspace_bytes(1.5)
    with pytest.raises(TypeError):
        lib.ovis_nms_workspace_bytes()
