"""Writes tests/golden/gemm_routes.json: which C-ABI entry point (or library call) every dense product of a shape / layout / dtype grid
reaches through gemm.mm and through the weight-gradient entries, with the launch's integer arguments.

No GPU: the operands are stand-in objects (shape, strides, dtype, is_cuda, data_ptr), `_launch` is replaced by a recorder, and the
library calls (`@`, torch.bmm) record themselves.  The table was written by this file AT THE COMMIT BEFORE gemm.route / gemm.wgrad
existed and must come out byte-identical from every later one (tests/test_gemm_routes_cpu.py): the weight-gradient entries are
looked up under their names of that commit first.

    python -m tests.golden.make_golden_gemm_routes
"""
import contextlib
import json
import os

import torch

MS = (64, 200, 3200, 3328, 4096, 4992, 8192, 8320, 32768, 65536, 262144)
# (N, K): every width of 8 .. 1536 the models use, paired the way the shape table, the ragged rules and the weight-stationary kernel
# tell them apart (the full cross product is a megabyte of table and adds no rule)
PAIRS = ((384, 384), (384, 1024), (384, 1152), (384, 1536), (1152, 384), (1536, 384), (768, 384), (256, 512), (128, 384), (1024, 384),
         (512, 256), (256, 128), (96, 384), (384, 96), (192, 192), (576, 192), (288, 96), (96, 288), (72, 72), (8, 8), (128, 8),
         (1536, 1536))
LAYOUTS = ("dense", "pitch+8", "pitch+4", "base+8B", "w pitch 0", "out pitch%8")
# every layout and the fp32 modes on a sub-grid: the layout rules do not depend on the shape table
SUB_MS = (200, 65536)
SUB_PAIRS = ((384, 384), (96, 384), (192, 192), (72, 72))
WG_RS = (48, 64, 512, 8192)
WG_PAIRS = ((128, 128), (96, 384), (384, 1536), (8, 72), (1024, 384))
WG_NBS = (None, 1, 4, 12)           # None: the 2-D entry

_events = []


def _dense(shape):
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= n
    return tuple(reversed(st))


class Fake:
    """what the routing code reads of a tensor, and the few methods the library tails call on one"""

    def __init__(self, shape, dtype, strides=None, ptr=4096):
        self.shape, self.dtype = tuple(shape), dtype
        self._st = tuple(strides) if strides is not None else _dense(self.shape)
        self._ptr = ptr
        self.is_cuda = True
        self.device = torch.device("cpu")           # what the code under test allocates beside the operands lands in host memory

    def dim(self):
        return len(self.shape)

    def stride(self, i=None):
        return self._st if i is None else self._st[i]

    def data_ptr(self):
        return self._ptr

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def is_contiguous(self):
        return self._st == _dense(self.shape)

    def unsqueeze(self, d):
        assert d == 0
        return Fake((1,) + self.shape, self.dtype, (self.shape[0] * self._st[0],) + self._st, self._ptr)

    def __getitem__(self, i):
        assert i == 0
        return Fake(self.shape[1:], self.dtype, self._st[1:], self._ptr)

    def view(self, *shape):
        assert self.is_contiguous() or shape == (1,) + self.shape
        return self.unsqueeze(0) if shape == (1,) + self.shape else Fake(shape, self.dtype, None, self._ptr)

    def transpose(self, a, b):
        sh, st = list(self.shape), list(self._st)
        sh[a], sh[b], st[a], st[b] = sh[b], sh[a], st[b], st[a]
        return Fake(sh, self.dtype, st, self._ptr)

    def t(self):
        return self.transpose(0, 1)

    def new_empty(self, *shape):
        return Fake(shape, self.dtype)

    def _same(self, *a, **k):
        return self
    detach = float = contiguous = to = copy_ = __add__ = _same

    def __matmul__(self, other):
        _events.append(["lib", {"op": "matmul"}, list(self.shape) + list(other.shape) + list(other.stride())])
        return Fake((self.shape[0], other.shape[1]), self.dtype)


def _launch(name, meta, fn, *args):
    _events.append([name, meta, [a for a in args if type(a) is int]])


def _bmm(a, b, out_dtype=None, out=None):
    _events.append(["lib", {"op": "bmm", "out_dtype": out_dtype is not None, "out": out is not None},
                    list(a.shape) + list(a.stride()) + list(b.shape)])
    return out if out is not None else Fake((a.shape[0], a.shape[1], b.shape[2]), torch.float32)


@contextlib.contextmanager
def recording(f32_own=False):
    """the package's launches and library products go to `_events` instead of a device"""
    from gm3d_amd import embed, fused, gemm
    saved = [(m, n, getattr(m, n)) for m in (gemm, embed, fused) for n in ("_launch", "_stream") if hasattr(m, n)]
    saved += [(torch, "bmm", torch.bmm), (gemm, "F32_OWN", gemm.F32_OWN)]
    try:
        for m, n, _ in saved[:-2]:
            setattr(m, n, _launch if n == "_launch" else (lambda: None))
        torch.bmm, gemm.F32_OWN = _bmm, f32_own
        yield
    finally:
        for m, n, v in saved:
            setattr(m, n, v)


def operands(M, N, K, layout, dtype):
    """x (M,K), w (N,K), bias (N) f32, out (M,N) in `layout`"""
    xs = {"pitch+8": (K + 8, 1), "pitch+4": (K + 4, 1)}.get(layout)
    x = Fake((M, K), dtype, xs, 4096 + (8 if layout == "base+8B" else 0))
    w = Fake((N, K), dtype, (0, 1) if layout == "w pitch 0" else None, 8192)
    out = Fake((M, N), dtype, (N + 4, 1) if layout == "out pitch%8" else None, 16384)
    return x, w, Fake((N,), torch.float32, None, 2048), out


def mm_case(M, N, K, layout, mode):
    """-> the events of gemm.mm(x, w, bias, out); mode: "bf16", "f32" (F32_OWN off), "f32own" """
    from gm3d_amd import gemm
    del _events[:]
    with recording(mode == "f32own"):
        gemm.mm(*operands(M, N, K, layout, torch.bfloat16 if mode == "bf16" else torch.float32))
    return list(_events)


def wgrad_case(R, N, K, nb, mode):
    """-> the events of the weight gradient dy^T @ x: 2-D (nb None) through embed.splitk_wgrad, batched through the stacks' entry"""
    from gm3d_amd import embed, fused, gemm
    dtype = torch.bfloat16 if mode == "bf16" else torch.float32
    del _events[:]
    with recording(mode == "f32own"):
        if nb is None:
            embed.splitk_wgrad(Fake((R, N), dtype, None, 4096), Fake((R, K), dtype, None, 8192))
        else:
            batched = getattr(fused, "_wgrad_batched", None) or gemm.wgrad
            batched(Fake((nb, R, N), dtype, None, 4096), Fake((nb, R, K), dtype, None, 8192), Fake((nb, N, K), torch.float32, None, 16384))
    return list(_events)


def mm_grid():
    for M in MS:
        for N, K in PAIRS:
            yield M, N, K, "dense", "bf16"
    for mode in ("bf16", "f32", "f32own"):
        for layout in (LAYOUTS if mode == "bf16" else ("dense", "pitch+4")):
            if (mode, layout) == ("bf16", "dense"):
                continue
            for M in SUB_MS:
                for N, K in (SUB_PAIRS if mode == "bf16" else SUB_PAIRS[:2]):
                    yield M, N, K, layout, mode


def wgrad_grid():
    for mode in ("bf16", "f32", "f32own"):
        for nb in (WG_NBS if mode == "bf16" else (None, 4)):
            for R in WG_RS:
                for N, K in (WG_PAIRS if mode == "bf16" else WG_PAIRS[:2]):
                    yield R, N, K, nb, mode


def generate():
    table = {}
    for M, N, K, layout, mode in mm_grid():
        table["mm %s %s %d %d %d" % (mode, layout, M, N, K)] = mm_case(M, N, K, layout, mode)
    for R, N, K, nb, mode in wgrad_grid():
        table["wgrad %s %s %d %d %d" % (mode, "2d" if nb is None else "nb%d" % nb, R, N, K)] = wgrad_case(R, N, K, nb, mode)
    return table


def dumps(table):
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in table.items()) + "\n}\n"


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_routes.json")
    with open(path, "w") as f:
        f.write(dumps(generate()))
    print(path, os.path.getsize(path))
