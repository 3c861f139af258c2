"""ctypes binding of libgm3d_hip.so -- the C ABI declared in include/gm3d.h.

There is NO CPU fallback anywhere in this package: if the library is missing the
import fails loudly, and every op rejects non-GPU tensors.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GM3D_HIP_LIB") or os.path.join(_HERE, "lib", "libgm3d_hip.so")
HEADER = os.path.join(_HERE, "..", "include", "gm3d.h")

GM3D_OK, GM3D_EINVAL, GM3D_EUNSUPPORTED, GM3D_ELAUNCH = 0, -1, -2, -3
GM3D_F32, GM3D_BF16 = 0, 1

_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
           "gm3d_stream_t": ctypes.c_void_p}
_DECL = re.compile(r"^([A-Za-z_][A-Za-z0-9_ ]*?\**) *\b(gm3d_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", re.M)


def _ctype(c_type, func, table=_CTYPES):
    """The ctypes type of one C type as the header spells it (qualifiers and the parameter's name already removed)."""
    if "*" in c_type:
        return ctypes.c_void_p
    if c_type not in table:
        raise ImportError("gm3d_amd: %s: no ctypes mapping for the type %r in include/gm3d.h" % (func, c_type))
    return table[c_type]


def parse_header(text):
    """name -> (restype, argtypes) for every function that the header text declares."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    out = {}
    for ret, name, params in _DECL.findall(text):
        ret = " ".join(ret.replace("const", " ").split())
        restype = ctypes.c_char_p if ret == "char *" else _ctype(ret, name, {"int": ctypes.c_int})
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = p.replace("const", " ").replace("*", " * ").split()
            argtypes.append(_ctype(" ".join(words[:-1]), name))      # the last word is the parameter's name
        out[name] = (restype, argtypes)
    return out


with open(HEADER) as _f:
    _PARSED = parse_header(_f.read())
# name -> argtypes, derived from include/gm3d.h (tests/test_capi_symbols.py pins the parser)
SIGNATURES = {name: argtypes for name, (_, argtypes) in _PARSED.items()}


class Gm3dError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "gm3d_amd: %s not found. Build it with `python -m gm3d_amd.build` "
            "(hipcc, --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PARSED.items():
        fn = getattr(lib, name)  # AttributeError = ABI mismatch: fail loudly
        fn.argtypes = argtypes
        fn.restype = restype
    return lib


lib = _load()


def check(rc, what):
    if rc != GM3D_OK:
        raise Gm3dError("%s failed: %s (code %d)" % (what, lib.gm3d_strerror(rc).decode(), rc))
