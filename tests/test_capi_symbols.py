"""CPU: libgm3d_hip.so builds, loads without a GPU and exports exactly what include/gm3d.h declares
(no compute calls here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    txt = open(os.path.join(ROOT, "include", "gm3d.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gm3d_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", txt)}


def test_library_exports_every_declared_symbol():
    from gm3d_amd import build
    lib = ctypes.CDLL(build.build())
    decl = declared()
    assert len(decl) >= 11
    for name in decl:
        assert hasattr(lib, name), name
    from gm3d_amd import _capi
    assert set(_capi.SIGNATURES) == set(decl)
    for name, args in decl.items():
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert len(_capi.SIGNATURES[name]) == n, name
    assert _capi.lib.gm3d_abi_version() == 1
    assert b"invalid" in _capi.lib.gm3d_strerror(-1)


HEADER_TEXT = """
typedef void *gm3d_stream_t; /* hipStream_t */
#define GM3D_OK 0
/* a comment (with a parenthesis); int gm3d_not_declared(int x); */
int gm3d_version(void);
const char *gm3d_name(int code);   // line comment (also stripped)
int gm3d_every_kind(const void *p, float *q, const long long *ids, int n, float s, double d,
                    long long stride, gm3d_stream_t stream);
"""


def test_header_parser_maps_every_parameter_kind():
    from gm3d_amd import _capi
    c = ctypes
    assert _capi.parse_header(HEADER_TEXT) == {
        "gm3d_version": (c.c_int, []),
        "gm3d_name": (c.c_char_p, [c.c_int]),
        "gm3d_every_kind": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_float, c.c_double, c.c_longlong, c.c_void_p]),
    }


def test_header_parser_refuses_unknown_types():
    import pytest
    from gm3d_amd import _capi
    with pytest.raises(ImportError, match=r"gm3d_f.*unsigned"):
        _capi.parse_header("int gm3d_f(unsigned n);")
    with pytest.raises(ImportError, match=r"gm3d_g.*size_t"):
        _capi.parse_header("int gm3d_g(int n, size_t bytes, gm3d_stream_t stream);")
    with pytest.raises(ImportError, match=r"gm3d_h.*float"):
        _capi.parse_header("float gm3d_h(int n);")
    with pytest.raises(ImportError, match=r"gm3d_i.*void"):
        _capi.parse_header("void gm3d_i(int n);")


def test_signature_widths_come_from_the_header():
    """Pins that an argument-count check cannot see: a 64-bit stride, a double and a float, and the one string result."""
    from gm3d_amd import _capi
    assert _capi.SIGNATURES["gm3d_colsum_finish_batched"][2] is ctypes.c_longlong
    assert _capi.SIGNATURES["gm3d_bn_finalize"][1] is ctypes.c_double
    assert _capi.SIGNATURES["gm3d_attention_fwd"][6] is ctypes.c_float
    assert _capi.lib.gm3d_strerror.restype is ctypes.c_char_p
    assert _capi.lib.gm3d_abi_version.restype is ctypes.c_int
    assert _capi.lib.gm3d_bn_finalize.argtypes[1] is ctypes.c_double


def test_argument_errors_are_detected_before_any_launch():
    """NULL pointers / bad sizes return GM3D_EINVAL / EUNSUPPORTED on the host: safe without a GPU."""
    from gm3d_amd._capi import lib, GM3D_EINVAL, GM3D_EUNSUPPORTED
    assert lib.gm3d_fps(None, 1, 1024, 64, None, None, None) == GM3D_EINVAL
    one = ctypes.c_void_p(16)  # never dereferenced: the shape check fails first
    assert lib.gm3d_fps(one, 1, 100000, 64, one, None, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_knn(one, one, 1, 8, 2, 9, None, one, None) == GM3D_EINVAL          # k > N
    assert lib.gm3d_knn(one, one, 1, 1024, 2, 65, None, one, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_attention_fwd(one, one, None, 1, 129, 6, 0.125, 1, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_attention_fwd(one, one, None, 1, 64, 6, 0.125, 7, None) == GM3D_EINVAL
    assert lib.gm3d_chamfer_fwd(one, one, 1, 0, 32, one, one, one, one, None) == GM3D_EINVAL


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from gm3d_amd import ops
    with pytest.raises(RuntimeError):
        ops.fps(torch.zeros(1, 16, 3), 4)
    with pytest.raises(RuntimeError):
        ops.chamfer(torch.zeros(1, 32, 3), torch.zeros(1, 32, 3))
    with pytest.raises(RuntimeError):
        ops.attention(torch.zeros(1, 4, 3 * 6 * 64), 6, 0.125)
