"""CPU: the shape contract of the C ABI at its edges, in one table.

Every row names an entry point, the parameter its guard limits, the last value the guard accepts and the first value it refuses.
The refused side must return GM3D_EUNSUPPORTED on the host, before any launch: the pointers are never dereferenced, so this runs
without a GPU.  Where the entry point checks its shape before an early return for an empty batch (B = 0 or R = 0), the accepted
side is checked the same way: GM3D_OK, nothing launched.  Every accepted value is run on the GPU in tests/test_gpu_abi_edges.py.
"""
import ctypes
import math

import pytest

ONE = ctypes.c_void_p(16)      # never dereferenced: the shape check fails (or the empty batch returns) first


def _lib():
    from gm3d_amd._capi import lib
    return lib


def _fps(N, B=1):
    return _lib().gm3d_fps(ONE, B, N, 64, ONE, None, None)


def _gather_points_grad(M, B=1):
    return _lib().gm3d_gather_points_grad(ONE, ONE, B, 3, 2048, M, ONE, None)


def _knn_n(N, B=1):
    return _lib().gm3d_knn(ONE, ONE, B, N, 8, 32, None, ONE, None)


def _knn_k(k, B=1):
    return _lib().gm3d_knn(ONE, ONE, B, 1024, 8, k, None, ONE, None)


def _knn_group_n(N, B=1):
    return _lib().gm3d_knn_group(ONE, ONE, B, N, 8, 32, ONE, ONE, None, None)


def _chamfer_fwd(P, B=None):
    return _lib().gm3d_chamfer_fwd(ONE, ONE, P, 64, 48, ONE, ONE, ONE, ONE, None)


def _chamfer_bwd(P, B=None):
    return _lib().gm3d_chamfer_bwd(ONE, ONE, ONE, ONE, ONE, ONE, P, 64, 48, ONE, ONE, None)


def _attn_fwd(T, B=1, dtype=1):
    return _lib().gm3d_attention_fwd(ONE, ONE, None, B, T, 6, 0.125, dtype, None)


def _attn_bwd(T, B=1, dtype=1):
    return _lib().gm3d_attention_bwd(ONE, ONE, ONE, ONE, ONE, B, T, 6, 0.125, dtype, None)


def _mattn_fwd(T, B=1, HD=32, dtype=0):
    return _lib().gm3d_attention_masked_fwd(ONE, None, ONE, ONE, B, T, 6, HD, 0.125, dtype, None)


def _mattn_bwd(T, B=1, HD=32, dtype=0):
    return _lib().gm3d_attention_masked_bwd(ONE, None, ONE, ONE, ONE, ONE, B, T, 6, HD, 0.125, dtype, None)


def _radius(G, B=1):
    return _lib().gm3d_radius_mask_bits_m(ONE, None, 0, 0.5, B, G, ONE, None)


def _vote(V=10, T=65, cls_dim=40, dtype=0):
    return _lib().gm3d_cls_tail_vote(ONE, V, 4, T, 384, *([ONE] * 14), cls_dim, 1e-5, ONE, ONE, ONE, ONE, None, dtype, None)


def _partition(T, B=1):
    return _lib().gm3d_partition_visible(ONE, B, T, 16, ONE, ONE, ONE, ONE, ONE, ONE, None)


def _gather_inverse_s(S, B=1):
    return _lib().gm3d_gather_inverse(ONE, B, 1024, S, ONE, ONE, None)


def _gather_inverse_j(J, B=1):
    return _lib().gm3d_gather_inverse(ONE, B, J, 64, ONE, ONE, None)


def _back_project(Gf, B=1):
    return _lib().gm3d_back_project(ONE, ONE, B, 64, 8, Gf, ONE, None)


def _bias_gelu_fwd(C, R=1):
    return _lib().gm3d_bias_gelu_fwd(ONE, ONE, ONE, R, C, 0, None)


def _bias_gelu_bwd(C, R=1):
    return _lib().gm3d_bias_gelu_bwd(ONE, ONE, ONE, ONE, ONE, R, C, 0, None)


def _lin3_bwd(C, R=1):
    return _lib().gm3d_lin3_gelu_bwd(ONE, ONE, ONE, ONE, R, C, ONE, 0, None)


def _pn1_stats(C1, R=1):
    return _lib().gm3d_pn_layer1_bwd_stats(ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, R, C1, ONE, 0, None)


def _ln_plain_fwd(C, R=1):
    return _lib().gm3d_ln_plain_fwd(ONE, ONE, ONE, 1e-5, ONE, ONE, ONE, R, C, 0, None)


def _ln_plain_bwd(C, R=1):
    return _lib().gm3d_ln_plain_bwd(ONE, ONE, ONE, ONE, ONE, ONE, ONE, R, C, 0, None)


def _add_ln_fwd(C, R=1):
    return _lib().gm3d_add_ln_fwd(ONE, ONE, None, None, 1, None, ONE, ONE, 1e-5, ONE, ONE, ONE, ONE, R, C, 0, None)


def _add_ln_bwd(C, R=1):
    return _lib().gm3d_add_ln_bwd(ONE, None, ONE, ONE, ONE, ONE, None, 1, ONE, None, ONE, 2, R, C, 0, None)


def _nt_big(N, K, batch=1):
    return _lib().gm3d_gemm_nt_bf16_big(ONE, ONE, ONE, batch, 64, N, K, N, K, K, 64 * N, 64 * K, N * K, 1, 0, None)


# (id, call(value, **kw), last accepted, first refused, empty-batch keyword that returns after the guard or None, extra kwargs)
# The empty-batch keyword is given only where the guard runs before the entry point's early return for an empty batch.
LIMITS = [
    ("fps.N", _fps, 16384, 16385, "B", {}),                                      # guard in fps.hip
    ("gather_points_grad.M", _gather_points_grad, 16384, 16385, "B", {}),        # guard in fps.hip
    ("knn.N", _knn_n, 12288, 12289, "B", {}),                                    # guard in knn.hip
    ("knn.k", _knn_k, 64, 65, "B", {}),                                          # guard in knn.hip
    ("knn_group.N", _knn_group_n, 12288, 12289, "B", {}),                        # guard in knn.hip (shared knn_check)
    ("chamfer_fwd.P", _chamfer_fwd, 65535, 65536, None, {}),                     # guard in chamfer.hip (general kernel: grid.y = P)
    ("chamfer_bwd.P", _chamfer_bwd, 65535, 65536, None, {}),                     # guard in chamfer.hip
    ("attention_fwd.T.bf16", _attn_fwd, 128, 129, "B", {"dtype": 1}),            # guard in attention.hip
    ("attention_fwd.T.f32", _attn_fwd, 128, 129, "B", {"dtype": 0}),             # guard in attention.hip
    ("attention_bwd.T", _attn_bwd, 128, 129, "B", {}),                           # guard in attention.hip (shared attn_check)
    ("attention_masked_fwd.T.hd16", _mattn_fwd, 512, 513, "B", {"HD": 16}),      # guard in attention_masked.hip
    ("attention_masked_fwd.T.hd32", _mattn_fwd, 512, 513, "B", {"HD": 32}),      # guard in attention_masked.hip
    ("attention_masked_fwd.T.hd64", _mattn_fwd, 512, 513, "B", {"HD": 64}),      # guard in attention_masked.hip (f32 kernel)
    ("attention_masked_bwd.T.hd64", _mattn_bwd, 512, 513, "B", {"HD": 64}),      # guard in attention_masked.hip
    ("attention_masked_fwd.HD", lambda hd, B=1: _mattn_fwd(64, B=B, HD=hd), 64, 65, "B", {}),   # guard in attention_masked.hip
    # bf16 keeps the head in LDS, at most 160 KiB (launch_lds, common.hpp): refused after the empty-batch return
    ("attention_masked_fwd.T.hd64.bf16", _mattn_fwd, 480, 481, None, {"HD": 64, "dtype": 1}),
    ("attention_masked_bwd.T.hd64.bf16", _mattn_bwd, 256, 257, None, {"HD": 64, "dtype": 1}),
    ("attention_masked_bwd.T.hd32.bf16", _mattn_bwd, 480, 481, None, {"HD": 32, "dtype": 1}),
    ("attention_masked_fwd.T.hd32.bf16", _mattn_fwd, 512, 513, "B", {"HD": 32, "dtype": 1}),
    ("attention_masked_bwd.T.hd16.bf16", _mattn_bwd, 512, 513, "B", {"HD": 16, "dtype": 1}),
    ("radius_mask_bits.G", _radius, 8192, 8193, None, {}),                       # guard in attention_masked.hip (16 G bytes of LDS)
    ("cls_tail_vote.V", lambda v, **k: _vote(V=v), 16, 17, None, {}),           # guard in vote.hip
    ("cls_tail_vote.cls_dim", lambda v, **k: _vote(cls_dim=v), 256, 257, None, {}),   # guard in vote.hip
    ("partition_visible.T", _partition, 1024, 1025, "B", {}),                    # guard in gather.hip (one thread per token)
    ("gather_inverse.S", _gather_inverse_s, 4096, 4097, "B", {}),                # guard in gather.hip
    ("gather_inverse.J", _gather_inverse_j, 16384, 16385, "B", {}),              # guard in gather.hip
    ("back_project.Gf", _back_project, 8192, 8193, "B", {}),                     # guard in gather.hip
    ("bias_gelu_fwd.C", _bias_gelu_fwd, 8192, 8200, "R", {}),                    # guard in rowops.hip (C / 8 threads per row)
    ("bias_gelu_bwd.C", _bias_gelu_bwd, 8192, 8200, "R", {}),                    # guard in rowops.hip
    ("lin3_gelu_bwd.C", _lin3_bwd, 512, 520, None, {}),                          # guard in embed.hip
    ("pn_layer1_bwd_stats.C1", _pn1_stats, 256, 264, None, {}),                  # guard in embed.hip
    ("ln_plain_fwd.C", _ln_plain_fwd, 512, 516, "R", {}),                        # guard in rowops.hip (via gm3d_add_ln_fwd)
    ("ln_plain_bwd.C", _ln_plain_bwd, 512, 516, None, {}),                       # guard in rowops.hip (via gm3d_add_ln_bwd_acc)
    ("add_ln_fwd.C", _add_ln_fwd, 512, 516, "R", {}),                            # guard in rowops.hip
    ("add_ln_bwd.C", _add_ln_bwd, 512, 516, None, {}),                           # guard in rowops.hip
    # whole 128 x 384 tiles only: the first refused value is a multiple of 8 (what gm3d_gemm_nt_bf16 takes) that is not a whole tile
    ("gemm_nt_bf16_big.N", lambda n, batch=1: _nt_big(n, 384, batch), 128, 136, "batch", {}),      # guard in gemm_nt.hip (nt_launch)
    ("gemm_nt_bf16_big.K", lambda k, batch=1: _nt_big(128, k, batch), 384, 392, "batch", {}),      # guard in gemm_nt.hip (nt_launch)
]

# The lower ends and the alignment conditions of the same guards: refused values only.
REFUSED_ALSO = [
    ("attention_masked_fwd.HD=48", lambda: _mattn_fwd(64, HD=48)),                # guard in attention_masked.hip
    ("cls_tail_vote.T=1", lambda: _vote(T=1)),                                    # guard in vote.hip: the head max-pools T - 1 >= 1 tokens
    ("cls_tail_vote.C=256", lambda: _lib().gm3d_cls_tail_vote(ONE, 10, 4, 65, 256, *([ONE] * 14), 40, 1e-5, ONE, ONE, ONE, ONE,
                                                              None, 0, None)),   # guard in vote.hip
    ("bias_gelu_bwd.C%8", lambda: _bias_gelu_bwd(12)),                            # guard in rowops.hip
    ("lin3_gelu_bwd.C%8", lambda: _lin3_bwd(12)),                                 # guard in embed.hip (chan_ok)
    ("pn_layer1_bwd_stats.C1%8", lambda: _pn1_stats(204)),                        # guard in embed.hip (chan_ok)
    ("ln_plain_fwd.C%4", lambda: _ln_plain_fwd(98)),                              # guard in rowops.hip
    ("ln_plain_fwd.C<4", lambda: _ln_plain_fwd(3)),                              # guard in rowops.hip (C = 3 is EUNSUPPORTED, not EINVAL)
    ("add_ln_bwd.C%4", lambda: _add_ln_bwd(98)),                                  # guard in rowops.hip
    ("gemm_nt_bf16_big.K=128", lambda: _nt_big(128, 128)),                        # guard in gemm_nt.hip: a 128 x 128 tile is not a big one
    ("gemm_nt_bf16_big.N%8", lambda: _nt_big(132, 384)),                          # guard in gemm_nt.hip (shared with gm3d_gemm_nt_bf16)
]


@pytest.mark.parametrize("row", LIMITS, ids=[r[0] for r in LIMITS])
def test_first_refused_shape_is_refused_before_any_launch(row):
    from gm3d_amd._capi import GM3D_EUNSUPPORTED
    name, call, ok, refused, empty, kw = row
    assert refused > ok
    assert call(refused, **kw) == GM3D_EUNSUPPORTED, name


@pytest.mark.parametrize("row", [r for r in LIMITS if r[4]], ids=[r[0] for r in LIMITS if r[4]])
def test_last_accepted_shape_passes_the_guard(row):
    """With an empty batch the call returns right after its shape checks: the accepted side is OK without a launch."""
    from gm3d_amd._capi import GM3D_OK
    name, call, ok, refused, empty, kw = row
    assert call(ok, **{empty: 0}, **kw) == GM3D_OK, name


@pytest.mark.parametrize("row", REFUSED_ALSO, ids=[r[0] for r in REFUSED_ALSO])
def test_other_refused_shapes(row):
    from gm3d_amd._capi import GM3D_EUNSUPPORTED
    assert row[1]() == GM3D_EUNSUPPORTED, row[0]


def test_fp64_slice_reductions_keep_their_lds_tile_within_64_kib():
    """gm3d_pn_layer1_bwd_stats (q = 5 fp64 sums) and gm3d_lin3_gelu_bwd (q = 4) launch sl row slices of C / 8 threads with an
    sl * q * C * 8-byte LDS tile and set no LDS attribute, so the tile must fit the 64 KiB a launch gets by default.  sl is not
    exported, but the partial-row count is: ceil(R / sl) rows (R small enough that the 1024-workgroup cap does not bind)."""
    lib = _lib()
    R = 4000
    for kind, q, Cmax in ((4, 5, 256), (3, 4, 512)):
        for C in range(8, Cmax + 1, 8):
            rows = lib.gm3d_embed_partial_rows(kind, R, C)
            sl = math.ceil(R / rows)
            assert rows == math.ceil(R / sl), (kind, C)
            assert sl * q * C * 8 <= 64 * 1024, (kind, C, sl)
            assert sl * C // 8 <= 256, (kind, C, sl)      # __launch_bounds__(256)
    # the step's shapes keep their 8 slices: C1 = 128 (embed layer 1), C = 128 / 256 (lin3 of the position embeddings)
    assert lib.gm3d_embed_partial_rows(4, R, 128) == R // 8
    assert lib.gm3d_embed_partial_rows(3, R, 128) == R // 8 and lib.gm3d_embed_partial_rows(3, R, 256) == R // 8
    assert lib.gm3d_embed_partial_rows(4, R, 256) == R // 4 and lib.gm3d_embed_partial_rows(3, R, 512) == R // 4
    assert lib.gm3d_embed_partial_rows(4, 10 ** 6, 256) == 1024      # the workgroup cap


def test_table_covers_the_documented_limits():
    """The header states these limits in words; the table must carry the same numbers."""
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gm3d.h")).read()
    rows = {r[0]: r for r in LIMITS}
    assert "N <= 16384" in txt and rows["fps.N"][2] == 16384
    assert "1 <= T <= 128" in txt and rows["attention_fwd.T.bf16"][2] == 128
    assert "T <= 480 forward / T <= 256 backward for HD = 64" in txt and "T <= 480 backward for HD = 32" in txt
    assert rows["attention_masked_bwd.T.hd32.bf16"][2] == 480
    assert rows["attention_masked_fwd.T.hd64.bf16"][2] == 480 and rows["attention_masked_bwd.T.hd64.bf16"][2] == 256
    assert "T <= 1024" in txt and rows["partition_visible.T"][2] == 1024
    assert "S <= 4096, J <= 16384" in txt and rows["gather_inverse.S"][2] == 4096 and rows["gather_inverse.J"][2] == 16384
    assert "Gf <= 8192" in txt and rows["back_project.Gf"][2] == 8192
    assert re.search(r"C1 <= 256", txt) and rows["pn_layer1_bwd_stats.C1"][2] == 256
    assert "C <= 512" in txt and rows["lin3_gelu_bwd.C"][2] == 512
