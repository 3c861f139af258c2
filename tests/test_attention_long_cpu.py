"""CPU: the C-ABI edges of gm3d_attention_long_fwd/bwd (gm3d_amd/csrc/attention_long.hip), in the manner of
tests/test_abi_limits_cpu.py -- the refused side answers on the host before any launch, so the pointers are never dereferenced and
no GPU is needed; with an empty batch the accepted side returns GM3D_OK right after the same checks -- and the committed bars table
of tests/test_gpu_attention_long.py."""
import ctypes
import importlib.util
import json
import os

import pytest

from tests import attention_long_cases as C
from tests import mattn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(16)      # never dereferenced: the shape check fails (or the empty batch returns) first


def _fwd(T, B=1, HD=32, dtype=0):
    from gm3d_amd._capi import lib
    return lib.gm3d_attention_long_fwd(ONE, None, ONE, ONE, B, T, 6, HD, 0.125, dtype, None)


def _bwd(T, B=1, HD=32, dtype=0):
    from gm3d_amd._capi import lib
    return lib.gm3d_attention_long_bwd(ONE, None, ONE, ONE, ONE, ONE, B, T, 6, HD, 0.125, dtype, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("HD", [16, 32, 64])
def test_accepted_and_refused_token_counts(call, dtype, HD):
    from gm3d_amd._capi import GM3D_EUNSUPPORTED, GM3D_OK
    for T in (513, 2048):
        assert call(T, B=0, HD=HD, dtype=dtype) == GM3D_OK, T
    for T in (512, 2049, 1, 128):      # T <= 512 belongs to gm3d_attention_masked_*: one owner per range
        assert call(T, HD=HD, dtype=dtype) == GM3D_EUNSUPPORTED, T
        assert call(T, B=0, HD=HD, dtype=dtype) == GM3D_EUNSUPPORTED, T


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_other_refusals(call):
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED
    assert call(513, HD=48) == GM3D_EUNSUPPORTED
    assert call(513, HD=128) == GM3D_EUNSUPPORTED
    assert call(513, dtype=2) == GM3D_EINVAL
    assert call(513, dtype=-1) == GM3D_EINVAL
    assert call(513, B=-1) == GM3D_EINVAL
    assert call(513, B=(2 ** 31 - 1) // 4 // 6 + 1) == GM3D_EUNSUPPORTED      # the B * H bound of gm3d_attention_masked_*


def test_null_tensors_are_invalid():
    from gm3d_amd._capi import GM3D_EINVAL, lib
    assert lib.gm3d_attention_long_fwd(None, None, ONE, ONE, 1, 513, 6, 32, 0.125, 0, None) == GM3D_EINVAL
    assert lib.gm3d_attention_long_fwd(ONE, None, ONE, None, 1, 513, 6, 32, 0.125, 0, None) == GM3D_EINVAL
    assert lib.gm3d_attention_long_bwd(ONE, None, ONE, None, ONE, ONE, 1, 513, 6, 32, 0.125, 0, None) == GM3D_EINVAL
    assert lib.gm3d_attention_long_bwd(ONE, None, ONE, ONE, ONE, None, 1, 513, 6, 32, 0.125, 0, None) == GM3D_EINVAL


def test_existing_entry_points_still_refuse_513():
    from gm3d_amd._capi import GM3D_EUNSUPPORTED, lib
    assert lib.gm3d_attention_masked_fwd(ONE, None, ONE, ONE, 1, 513, 6, 32, 0.125, 0, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_attention_masked_bwd(ONE, None, ONE, ONE, ONE, ONE, 1, 513, 6, 32, 0.125, 0, None) == GM3D_EUNSUPPORTED


def test_header_declares_the_entry_points_and_their_contract():
    txt = open(os.path.join(ROOT, "include", "gm3d.h")).read()
    flat = " ".join(txt.replace("\n * ", " ").split())      # comment lines joined, their leading " * " dropped
    assert "int gm3d_attention_long_fwd(const void *qkv, const unsigned *mask, void *out, float *lse, int B, int T, int H, int HD," in flat
    assert "int gm3d_attention_long_bwd(const void *qkv, const unsigned *mask, const void *out, const void *dout," in flat
    assert "513 <= T <= 2048" in flat
    assert "T <= 512 and T > 2048 are GM3D_EUNSUPPORTED" in flat
    assert "HD in {16,32,64}" in flat and "B * H <= (2^31 - 1) / 4" in flat
    assert "GM3D_EINVAL" in flat and "before any launch" in flat
    assert "no atomics, no zero-fill" in flat


def test_python_guards_follow_the_kernels():
    import inspect
    from gm3d_amd import masked_stack, point_transformer
    assert "<= 2048" in inspect.getsource(masked_stack.supported)
    assert "self.num_group + 1 > 2048" in inspect.getsource(point_transformer.PointTransformer.__init__)


# ------------------------------------------------------------------------------------------------------------ the bars table
@pytest.fixture(scope="module")
def committed():
    with open(C.TABLE) as f:
        return json.load(f)


def test_table_has_a_row_for_every_case(committed):
    ids = [C.case_id(c) for c in C.cases()]
    assert len(set(ids)) == len(ids)
    assert sorted(committed) == sorted(ids)
    for c in C.cases():
        row = committed[C.case_id(c)]
        assert sorted(row) == ["dk", "dq", "dv", "lse", "out"], C.case_id(c)
        assert all(0.0 <= v < float("inf") for v in row.values()), C.case_id(c)
        bar = C.bars(c, row)
        assert all(bar[k] >= R.BARS[c.dtype][k] and bar[k] >= 3.0 * row[k] for k in row)


def test_cases_cover_what_the_kernels_branch_on():
    cs = C.cases()
    assert {(c.T, c.hd) for c in cs} == set(C.SHAPES)
    assert {c.kind for c in cs} == set(C.KINDS) and {c.dtype for c in cs} == {"f32", "bf16"}
    assert {c.variant for c in cs} == {"base", "amp", "adv"} and {c.B for c in cs} == {3, 4}
    assert all(513 <= c.T <= 2048 for c in cs)
    assert any(c.T % 64 == 1 for c in cs) and any(c.T % 256 == 0 for c in cs) and any(c.T == 2048 for c in cs)


@pytest.mark.parametrize("c", [R.Case("base", "anti", 513, 16, 4, "f32"), R.Case("amp", "sparse", 513, 16, 4, "bf16")], ids=C.case_id)
def test_table_regenerates(c, committed):
    spec = importlib.util.spec_from_file_location("make_attention_long_bars",
                                                  os.path.join(ROOT, "tests", "golden", "make_attention_long_bars.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.row(c) == committed[C.case_id(c)]
