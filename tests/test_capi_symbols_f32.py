"""CPU: the fp32 MFMA GEMM family (csrc/gemm_f32.hip) is exported by the built library, declared in include/gm3d.h with the argument
counts _capi binds, rejects calls outside its contract on the host, and the switch that routes the fp32 step to it exists and is off."""
import ctypes

from tests.test_capi_symbols import declared

NEW = ("gm3d_gemm_tn_f32", "gm3d_gemm_nt_f32", "gm3d_gemm_nt_f32_splits", "gm3d_gemm_nt_f32_slab_rows")


def test_f32_gemm_symbols_are_exported_declared_and_bound():
    from gm3d_amd import build
    lib = ctypes.CDLL(build.build())
    from gm3d_amd import _capi
    decl = declared()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in decl, name
        assert len(_capi.SIGNATURES[name]) == len(decl[name].split(",")), name


def test_f32_gemm_contract_is_checked_before_any_launch():
    """M = 0, a negative pitch, a NULL operand: GM3D_EINVAL; a misaligned pointer: GM3D_EUNSUPPORTED -- on the host, no GPU needed."""
    from gm3d_amd._capi import lib, GM3D_EINVAL, GM3D_EUNSUPPORTED
    one = ctypes.c_void_p(16)          # never dereferenced
    assert lib.gm3d_gemm_tn_f32(one, one, None, one, 0, 8, 8, 8, 8, 8, None) == GM3D_EINVAL
    assert lib.gm3d_gemm_tn_f32(one, one, None, one, 8, 8, 8, -8, 8, 8, None) == GM3D_EINVAL
    assert lib.gm3d_gemm_tn_f32(one, one, None, one, 8, 8, 8, 8, 8, 7, None) == GM3D_EINVAL
    assert lib.gm3d_gemm_tn_f32(None, one, None, one, 8, 8, 8, 8, 8, 8, None) == GM3D_EINVAL
    assert lib.gm3d_gemm_tn_f32(ctypes.c_void_p(18), one, None, one, 8, 8, 8, 8, 8, 8, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_gemm_nt_f32(one, one, one, None, 1, 0, 8, 8, 8, 8, 8, 0, 0, 0, 1, 0, None) == GM3D_EINVAL
    assert lib.gm3d_gemm_nt_f32(one, one, one, None, 1, 64, 8, 8, -8, 8, 8, 0, 0, 0, 1, 0, None) == GM3D_EINVAL
    assert lib.gm3d_gemm_nt_f32(one, one, one, None, 1, 4096, 8, 8, 8, 8, 8, 0, 0, 0, 2, 0, None) == GM3D_EINVAL      # splits without part
    assert lib.gm3d_gemm_nt_f32(one, one, one, one, 1, 40, 8, 8, 8, 8, 8, 0, 0, 0, 3, 0, None) == GM3D_EINVAL         # an empty slab
    assert lib.gm3d_gemm_nt_f32(one, one, one, one, 1, 1 << 20, 8, 8, 8, 8, 8, 0, 0, 0, 65, 0, None) == GM3D_EUNSUPPORTED


def test_nt_f32_splits_is_a_pure_function_with_no_empty_slab():
    from gm3d_amd._capi import lib
    for batch in (1, 3, 12):
        for R in (1, 65, 512, 4100, 8192, 262144):
            for N, K in ((8, 3), (96, 384), (392, 130), (1536, 384)):
                s = lib.gm3d_gemm_nt_f32_splits(batch, R, N, K)
                assert s == lib.gm3d_gemm_nt_f32_splits(batch, R, N, K) and 1 <= s <= 64
                slab = lib.gm3d_gemm_nt_f32_slab_rows(R, s)
                assert slab % 32 == 0 and (s - 1) * slab < R <= s * slab, (batch, R, N, K, s, slab)
    assert lib.gm3d_gemm_nt_f32_splits(1, 4100, 8, 3) > 1


def test_switch_exists_and_is_off():
    from gm3d_amd import gemm
    assert gemm.F32_OWN is False
