// Soft-target cross-entropy (forward, backward) and point mixup for the classification fine-tune (gm3d_amd/losses.py): label
// smoothing in both conventions the reference uses, and Point-MAE_SA3D/engine_finetune.py:43-76 (mixup_point_cloud).  Every
// coefficient is read from device memory, so a captured step follows new draws; every sum runs in the order below, so a graph replay
// equals an eager call bit for bit.  No atomics, no hand-off between workgroups.
//
// The target row is t_ic = u + wa [c = ya_i] + wb [c = yb_i] (compact; coef = (wa, wb, u); without yb the wb term is absent), or a dense
// (B,C) f32 tensor.  All arithmetic is f32, also for bf16 logits.
//
// soft_ce_fwd_kernel: ONE workgroup of min(16, B) waves; wave w owns rows w, w + W, ...; lane l owns classes l, l + 64, ... of a row.
//   per lane, classes ascending:  m_l = max z_c;  butterfly (below) -> m
//                                 s_l = sum expf(z_c - m);  butterfly -> s;  lse = m + logf(s)
//                                 compact: d_l = sum (lse - z_c);  butterfly -> d
//                                          row_loss = (wa (lse - z[ya]) + wb (lse - z[yb])) + u d      (u d is left out when u == 0)
//                                 dense:   r_l = sum t_c (lse - z_c);  butterfly -> row_loss
//   every term is a product of a weight and the non-negative lse - z_c: there is no S lse - sum t z cancellation.
//   A label outside [0, C) makes that row's loss NaN (gm3d_cls_tail_fwd's rule); lse is still written.
//   The mean: the row losses stay in LDS; after the one barrier wave 0's lane l adds rows l, l + 64, ... ascending, butterfly, / B.
// butterfly: v = v (+ or max) shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1 -- every lane ends with the same bits.
//
// soft_ce_bwd_kernel: 4 waves per workgroup, one wave per row, lane l owns classes l, l + 64, ...: every element has one writer.
//   S = (C u + wa) + wb (compact; without yb: C u + wa) or the butterfly sum of the lane sums of t_c (dense, classes ascending);
//   e_l = sum expf(z_c - lse), classes ascending;  butterfly -> e;  p_c = expf(z_c - lse) / e.  lse is the shift that keeps expf in
//   range, and e is 1 up to the rounding of the forward's lse = m + logf(s) (half an ulp of lse: 1.5e-5 at |lse| = 300), which the
//   division takes out again;
//   t_c = (u + wa [c = ya]) + wb [c = yb];  dlogits_c = (dloss / B) (S p_c - t_c), rounded once to the logits' dtype.
//   A label outside [0, C) makes the row NaN, like its loss.
//
// mixup_points_kernel: one workgroup per output cloud b, out[b] = l x[b] + m x[perm[b]] with both products rounded separately and one
//   add (no FMA: the file is built with -ffp-contract=off, and the intrinsics say so again); thread 0 writes yb[b] = ya[perm[b]].
//   perm lives on the device and cannot be checked on the host: a value outside [0, B) reads nothing -- the cloud becomes NaN and its
//   yb -1, which the loss turns into NaN.
#include <math.h>

#include "common.hpp"

namespace gm3d {

constexpr int SCE_MAX_B = 4096, SCE_MAX_C = 1024, SCE_FWD_WAVES = 16, SCE_BWD_WAVES = 4, MIX_THREADS_MAX = 1024;

__device__ __forceinline__ float sce_sum(float v) {
#pragma unroll
    for (int o = GM3D_WAVE / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float sce_max(float v) {
#pragma unroll
    for (int o = GM3D_WAVE / 2; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

template <class T>
__global__ __launch_bounds__(SCE_FWD_WAVES* GM3D_WAVE) void soft_ce_fwd_kernel(const T* __restrict__ logits, int B, int C,
                                                                                const long long* __restrict__ ya,
                                                                                const long long* __restrict__ yb,
                                                                                const float* __restrict__ coef,
                                                                                const float* __restrict__ dense,
                                                                                float* __restrict__ row_loss, float* __restrict__ lse_out,
                                                                                float* __restrict__ loss) {
    __shared__ float rows[SCE_MAX_B];
    const int lane = threadIdx.x & (GM3D_WAVE - 1), wave = threadIdx.x / GM3D_WAVE, W = blockDim.x / GM3D_WAVE;
    float wa = 0.f, wb = 0.f, u = 0.f;
    if (!dense) {
        wa = coef[0];
        wb = coef[1];
        u = coef[2];
    }
    for (int i = wave; i < B; i += W) {
        const T* z = logits + (size_t)i * C;
        float m = -INFINITY;
        for (int c = lane; c < C; c += GM3D_WAVE) m = fmaxf(m, (float)z[c]);
        m = sce_max(m);
        float s = 0.f;
        for (int c = lane; c < C; c += GM3D_WAVE) s += expf((float)z[c] - m);
        s = sce_sum(s);
        const float lse = m + logf(s);
        float r;
        if (dense) {
            const float* t = dense + (size_t)i * C;
            float acc = 0.f;
            for (int c = lane; c < C; c += GM3D_WAVE) acc += t[c] * (lse - (float)z[c]);
            r = sce_sum(acc);
        } else {
            const long long a = ya[i], b = yb ? yb[i] : 0;
            if (a < 0 || a >= C || b < 0 || b >= C) {
                r = NAN;
            } else {
                r = wa * (lse - (float)z[a]);
                if (yb) r += wb * (lse - (float)z[b]);
                if (u != 0.f) {
                    float d = 0.f;
                    for (int c = lane; c < C; c += GM3D_WAVE) d += lse - (float)z[c];
                    r += u * sce_sum(d);
                }
            }
        }
        if (lane == 0) {
            rows[i] = r;
            row_loss[i] = r;
            lse_out[i] = lse;
        }
    }
    __syncthreads();
    if (wave == 0) {
        float acc = 0.f;
        for (int i = lane; i < B; i += GM3D_WAVE) acc += rows[i];
        acc = sce_sum(acc);
        if (lane == 0) loss[0] = acc / (float)B;
    }
}

template <class T>
__global__ __launch_bounds__(SCE_BWD_WAVES* GM3D_WAVE) void soft_ce_bwd_kernel(const T* __restrict__ logits, int B, int C,
                                                                                const long long* __restrict__ ya,
                                                                                const long long* __restrict__ yb,
                                                                                const float* __restrict__ coef,
                                                                                const float* __restrict__ dense,
                                                                                const float* __restrict__ lse_in,
                                                                                const float* __restrict__ dloss, T* __restrict__ dlogits) {
    const int lane = threadIdx.x & (GM3D_WAVE - 1);
    const int i = blockIdx.x * SCE_BWD_WAVES + threadIdx.x / GM3D_WAVE;
    if (i >= B) return;                                      // whole waves leave; no barrier in this kernel
    const T* z = logits + (size_t)i * C;
    T* dz = dlogits + (size_t)i * C;
    const float g = dloss[0] / (float)B, lse = lse_in[i];
    float e = 0.f;
    for (int c = lane; c < C; c += GM3D_WAVE) e += expf((float)z[c] - lse);
    e = sce_sum(e);
    if (dense) {
        const float* t = dense + (size_t)i * C;
        float S = 0.f;
        for (int c = lane; c < C; c += GM3D_WAVE) S += t[c];
        S = sce_sum(S);
        for (int c = lane; c < C; c += GM3D_WAVE) dz[c] = (T)(g * (S * (expf((float)z[c] - lse) / e) - t[c]));
        return;
    }
    const float wa = coef[0], wb = yb ? coef[1] : 0.f, u = coef[2];
    const long long a = ya[i], b = yb ? yb[i] : -1;
    const bool bad = a < 0 || a >= C || (yb && (b < 0 || b >= C));
    const float S = ((float)C * u + wa) + wb;
    for (int c = lane; c < C; c += GM3D_WAVE) {
        float t = u;
        if (c == a) t += wa;
        if (c == b) t += wb;
        dz[c] = (T)(bad ? NAN : g * (S * (expf((float)z[c] - lse) / e) - t));
    }
}

__global__ __launch_bounds__(MIX_THREADS_MAX) void mixup_points_kernel(const float* __restrict__ x, const long long* __restrict__ perm,
                                                                        const float* __restrict__ coef2,
                                                                        const long long* __restrict__ ya, float* __restrict__ out,
                                                                        long long* __restrict__ yb, int B, int N) {
    const int b = blockIdx.x;
    const long long p = perm[b];
    const bool ok = p >= 0 && p < B;
    const float l = coef2[0], m = coef2[1];
    const size_t n3 = (size_t)N * 3;
    const float* xa = x + (size_t)b * n3;
    const float* xb = x + (size_t)(ok ? p : 0) * n3;
    float* o = out + (size_t)b * n3;
    for (size_t e = threadIdx.x; e < n3; e += blockDim.x) o[e] = ok ? __fadd_rn(__fmul_rn(l, xa[e]), __fmul_rn(m, xb[e])) : NAN;
    if (threadIdx.x == 0 && yb) yb[b] = ok ? ya[p] : -1;
}

inline int sce_check(const void* logits, int B, int C, const long long* ya, const long long* yb, const float* coef, const float* dense,
                     int dtype) {
    if (!logits || B < 0 || C < 1 || (dtype != GM3D_F32 && dtype != GM3D_BF16)) return GM3D_EINVAL;
    const bool compact = ya || yb || coef;
    if (compact == (dense != nullptr)) return GM3D_EINVAL;               // exactly one form
    if (compact && (!ya || !coef)) return GM3D_EINVAL;
    if (B > SCE_MAX_B || C > SCE_MAX_C) return GM3D_EUNSUPPORTED;
    return GM3D_OK;
}

}  // namespace gm3d

extern "C" int gm3d_soft_ce_fwd(const void* logits, int B, int C, const long long* ya, const long long* yb, const float* coef,
                                const float* dense, float* row_loss, float* lse, float* loss, int dtype, gm3d_stream_t stream) {
    using namespace gm3d;
    const int rc = sce_check(logits, B, C, ya, yb, coef, dense, dtype);
    if (rc != GM3D_OK) return rc;
    if (!row_loss || !lse || !loss) return GM3D_EINVAL;
    if (B == 0) return GM3D_OK;
    const int waves = B < SCE_FWD_WAVES ? B : SCE_FWD_WAVES;
    return by_dtype(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_lds<soft_ce_fwd_kernel<T>>(dim3(1), dim3(waves * GM3D_WAVE), 0, stream, (const T*)logits, B, C, ya, yb, coef, dense,
                                                 row_loss, lse, loss);
    });
}

extern "C" int gm3d_soft_ce_bwd(const void* logits, int B, int C, const long long* ya, const long long* yb, const float* coef,
                                const float* dense, const float* lse, const float* dloss, void* dlogits, int dtype,
                                gm3d_stream_t stream) {
    using namespace gm3d;
    const int rc = sce_check(logits, B, C, ya, yb, coef, dense, dtype);
    if (rc != GM3D_OK) return rc;
    if (!lse || !dloss || !dlogits) return GM3D_EINVAL;
    if (B == 0) return GM3D_OK;
    return by_dtype(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_lds<soft_ce_bwd_kernel<T>>(dim3((B + SCE_BWD_WAVES - 1) / SCE_BWD_WAVES), dim3(SCE_BWD_WAVES * GM3D_WAVE), 0, stream,
                                                 (const T*)logits, B, C, ya, yb, coef, dense, lse, dloss, (T*)dlogits);
    });
}

extern "C" int gm3d_mixup_points(const float* x, int B, int N, const long long* perm, const float* coef2, const long long* ya,
                                 float* out, long long* yb, gm3d_stream_t stream) {
    using namespace gm3d;
    if (!x || !perm || !coef2 || !out || out == x || N < 1 || B < 0 || (ya == nullptr) != (yb == nullptr)) return GM3D_EINVAL;
    if (B == 0) return GM3D_OK;
    const int threads = N > MIX_THREADS_MAX / 3 ? MIX_THREADS_MAX : (N * 3 + GM3D_WAVE - 1) / GM3D_WAVE * GM3D_WAVE;
    return launch_lds<mixup_points_kernel>(dim3((unsigned)B), dim3(threads), 0, stream, x, perm, coef2, ya, out, yb, B, N);
}
