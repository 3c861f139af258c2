// Voting evaluation of the fine-tuned classifier (Point-MAE_SA3D/tools/runner_finetune.py:271-335 validate_vote, :399-461
// test_vote): the V vote clouds of a batch built in one launch, and the eval-mode classification head + vote mean + argmax +
// correct count in one launch.  See include/gm3d.h for the contracts.
#include "cls_pool.hpp"
#include "common.hpp"

using namespace gm3d;

namespace {

constexpr int VOTE_MAX_V = 16;
constexpr int TAIL_C = 384;          // trans_dim: the head's input is 2*C = 768
constexpr int TAIL_H = 256;          // hidden width of cls_head_finetune
constexpr int TAIL_THREADS = 256;
constexpr int TAIL_WAVES = TAIL_THREADS / 64;
constexpr int TAIL_C8 = TAIL_C / 8;                  // 8-element column chunks of one token row
constexpr int TAIL_TG = TAIL_THREADS / TAIL_C8;      // token groups of the max-pool (5 x 48 = 240 threads)

// out[(v*B + b), j, :] = points[b, fps_idx[b, subsets[v, j]], :] * scale[v, b, :] + shift[v, b, :]
// = index_select + gather_operation + PointcloudScaleAndTranslate (datasets/data_transforms.py:27-35) of every vote.
// Indices come from the device: one out of range gives a NaN point instead of a stray read.
__global__ __launch_bounds__(256) void vote_sample_kernel(const float* __restrict__ points, const int32_t* __restrict__ fps_idx,
                                                          const long long* __restrict__ subsets, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, int B, int N0, int P, int npoints,
                                                          long long total, float* __restrict__ out) {
#pragma clang fp contract(off)   // product and sum rounded separately, like torch.mul(...) + ... of the reference
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long vb = i / npoints;
        const int j = (int)(i - vb * npoints);
        const int v = (int)(vb / B), b = (int)(vb - (long long)v * B);
        const long long s = subsets[(size_t)v * npoints + j];
        float* o = out + i * 3;
        const int k = (s >= 0 && s < P) ? fps_idx[(size_t)b * P + s] : -1;
        if (k < 0 || k >= N0) {
            o[0] = o[1] = o[2] = __builtin_nanf("");
            continue;
        }
        const float* p = points + ((size_t)b * N0 + k) * 3;
        const float* sc = scale + vb * 3;
        const float* sh = shift + vb * 3;
        o[0] = p[0] * sc[0] + sh[0];
        o[1] = p[1] * sc[1] + sh[1];
        o[2] = p[2] * sc[2] + sh[2];
    }
}

struct HeadArgs {
    const float *W1, *b1, *g1, *be1, *rm1, *rv1;
    const float *W2, *b2, *g2, *be2, *rm2, *rv2;
    const float *W3, *b3;
};

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// out[v][o] = act(W[o,:] . in[v,:] + bias[o]) for every vote v < V and row o < rows (in / out in LDS, pitches K / TAIL_H).
// One wave per row: the 64 lanes read the weight row coalesced, each lane sums its columns k = lane + 64 i in order, then a
// fixed butterfly across the wave.  BatchNorm (eval): (y - running_mean) / sqrt(running_var + eps) * gamma + beta, ReLU.
template <int K>
__device__ void dense(const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ gam,
                      const float* __restrict__ bet, const float* __restrict__ rm, const float* __restrict__ rv, float eps, int rows,
                      const float* in, float* out, int V) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = wave; o < rows; o += TAIL_WAVES) {
        float acc[VOTE_MAX_V];
#pragma unroll
        for (int v = 0; v < VOTE_MAX_V; ++v) acc[v] = 0.0f;
        const float* w = W + (size_t)o * K;
#pragma unroll 2
        for (int i = 0; i < K / 64; ++i) {
            const int k = lane + 64 * i;
            const float wk = w[k];
#pragma unroll
            for (int v = 0; v < VOTE_MAX_V; ++v)
                if (v < V) acc[v] = fmaf(wk, in[v * K + k], acc[v]);
        }
        float bo = bias[o], sc = 1.0f, mu = 0.0f, sh = 0.0f;
        if (gam) {
            sc = gam[o] / sqrtf(rv[o] + eps);
            mu = rm[o];
            sh = bet[o];
        }
#pragma unroll
        for (int v = 0; v < VOTE_MAX_V; ++v) {
            if (v < V) {
                float y = wave_sum(acc[v]) + bo;
                if (gam) y = fmaxf((y - mu) * sc + sh, 0.0f);
                if (lane == 0) out[v * TAIL_H + o] = y;
            }
        }
    }
}

__device__ __forceinline__ float nanmax(float a, float b) { return (b > a || b != b) ? b : a; }   // torch.max: NaN wins

// One workgroup per cloud b; it holds all V votes of that cloud: pooled features, both hidden layers and the logits stay in
// LDS, the vote mean is a sum in vote order in one thread, and argmax / correct count follow in the same workgroup.
template <class T>
__global__ __launch_bounds__(TAIL_THREADS) void cls_tail_vote_kernel(const T* __restrict__ x, int V, int B, int T_, HeadArgs h,
                                                                     int cls_dim, float eps, const long long* __restrict__ labels,
                                                                     float* __restrict__ mean, long long* __restrict__ pred,
                                                                     unsigned long long* __restrict__ correct, float* __restrict__ votes) {
    extern __shared__ float lds[];
    float* feat = lds;                                  // V x 768, later V x 256 (second hidden layer)
    float* part = feat + V * 2 * TAIL_C;                // TAIL_TG x 384 partial maxima
    float* hid = part + TAIL_TG * TAIL_C;               // V x 256: first hidden layer, later the logits
    const int b = blockIdx.x, tid = threadIdx.x;

    // feature of every vote: [x[:, 0] ; max over tokens 1..T-1] (P/models/Point_MAE.py:575)
    for (int v = 0; v < V; ++v) {
        const T* xr = x + ((size_t)v * B + b) * (size_t)T_ * TAIL_C;
        if (tid < TAIL_C8 * TAIL_TG) {
            const int c8 = tid % TAIL_C8, g = tid / TAIL_C8;
            float m[8], r[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) m[i] = -INFINITY;
            for (int t = 1 + g; t < T_; t += TAIL_TG) {
                V8<T>::load(xr + (size_t)t * TAIL_C + c8 * 8, r);
#pragma unroll
                for (int i = 0; i < 8; ++i) m[i] = nanmax(m[i], r[i]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) part[g * TAIL_C + c8 * 8 + i] = m[i];
            if (g == 0) {
                V8<T>::load(xr + c8 * 8, r);
#pragma unroll
                for (int i = 0; i < 8; ++i) feat[v * 2 * TAIL_C + c8 * 8 + i] = r[i];
            }
        }
        __syncthreads();
        for (int c = tid; c < TAIL_C; c += TAIL_THREADS) {
            float m = part[c];
#pragma unroll
            for (int g = 1; g < TAIL_TG; ++g) m = nanmax(m, part[g * TAIL_C + c]);
            feat[v * 2 * TAIL_C + TAIL_C + c] = m;
        }
        __syncthreads();
    }

    // Linear 768->256, BN, ReLU, (Dropout = identity), Linear 256->256, BN, ReLU, (Dropout), Linear 256->cls_dim
    dense<2 * TAIL_C>(h.W1, h.b1, h.g1, h.be1, h.rm1, h.rv1, eps, TAIL_H, feat, hid, V);
    __syncthreads();
    dense<TAIL_H>(h.W2, h.b2, h.g2, h.be2, h.rm2, h.rv2, eps, TAIL_H, hid, feat, V);
    __syncthreads();
    dense<TAIL_H>(h.W3, h.b3, nullptr, nullptr, nullptr, nullptr, eps, cls_dim, feat, hid, V);
    __syncthreads();

    // vote mean: sum over v = 0..V-1 in order, then / V
    float* mrow = part;
    for (int o = tid; o < cls_dim; o += TAIL_THREADS) {
        float s = 0.0f;
        for (int v = 0; v < V; ++v) {
            const float l = hid[v * TAIL_H + o];
            if (votes) votes[((size_t)v * B + b) * cls_dim + o] = l;
            s += l;
        }
        s = s / (float)V;
        mean[(size_t)b * cls_dim + o] = s;
        mrow[o] = s;
    }
    __syncthreads();
    if (tid == 0) {                                     // argmax, ties -> lowest index, NaN wins (torch.max)
        int best = 0;
        float bv = mrow[0];
        for (int o = 1; o < cls_dim; ++o) {
            const float l = mrow[o];
            if (bv == bv && (l > bv || l != l)) {
                bv = l;
                best = o;
            }
        }
        pred[b] = best;
        if ((long long)best == labels[b]) atomicAdd(correct, 1ull);   // integer add: order-independent
    }
}

constexpr int POOL_MAX_T = 512;

// The same head and vote epilogue for the Point-M2AE classifiers (gm3d_amd/point_m2ae_cls.py): the feature of every vote is the
// pooling of cls_pool_l1_kernel (cls_pool.hpp) -- mode 0: mean + max (F = 384), mode 1: [mean ; max] (F = 768) -- bit for bit.
// One workgroup per cloud b.  A thread pools 8 adjacent channels of one vote (one 16-byte row load per token); each channel's sum
// still runs over t = 0..T-1 in order.  featout (V*B,F), when given, receives the pooled features (row v*B+b, like x).
template <class T>
__global__ __launch_bounds__(TAIL_THREADS) void cls_tail_vote_pool_kernel(const T* __restrict__ x, int V, int B, int T_, int mode,
                                                                          HeadArgs h, int cls_dim, float eps,
                                                                          const long long* __restrict__ labels, float* __restrict__ mean,
                                                                          long long* __restrict__ pred,
                                                                          unsigned long long* __restrict__ correct,
                                                                          float* __restrict__ votes, float* __restrict__ featout) {
    extern __shared__ float lds[];
    const int F = mode ? 2 * TAIL_C : TAIL_C;
    float* feat = lds;                                  // V x F, later V x 256 (second hidden layer), later the vote mean
    float* hid = feat + V * F;                          // V x 256: first hidden layer, later the logits
    const int b = blockIdx.x, tid = threadIdx.x;

    for (int i = tid; i < V * TAIL_C8; i += TAIL_THREADS) {
        const int v = i / TAIL_C8, c8 = i - v * TAIL_C8;
        const T* xr = x + ((size_t)v * B + b) * (size_t)T_ * TAIL_C + c8 * 8;
        float r[8];
        PoolAcc p[8];
        V8<T>::load(xr, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k].init(r[k]);
#pragma unroll 4   // several row loads in flight; the adds stay in token order
        for (int t = 0; t < T_; ++t) {
            V8<T>::load(xr + (size_t)t * TAIL_C, r);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k].add(r[k], t);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) pool_feature(feat + v * F, TAIL_C, c8 * 8 + k, mode, p[k].mean(T_), p[k].m);
    }
    __syncthreads();
    if (featout)
        for (int i = tid; i < V * F; i += TAIL_THREADS) {
            const int v = i / F;
            featout[((size_t)v * B + b) * F + (i - v * F)] = feat[i];
        }

    // Linear F->256, BN, ReLU, (Dropout = identity), Linear 256->256, BN, ReLU, (Dropout), Linear 256->cls_dim
    if (mode)
        dense<2 * TAIL_C>(h.W1, h.b1, h.g1, h.be1, h.rm1, h.rv1, eps, TAIL_H, feat, hid, V);
    else
        dense<TAIL_C>(h.W1, h.b1, h.g1, h.be1, h.rm1, h.rv1, eps, TAIL_H, feat, hid, V);
    __syncthreads();
    dense<TAIL_H>(h.W2, h.b2, h.g2, h.be2, h.rm2, h.rv2, eps, TAIL_H, hid, feat, V);
    __syncthreads();
    dense<TAIL_H>(h.W3, h.b3, nullptr, nullptr, nullptr, nullptr, eps, cls_dim, feat, hid, V);
    __syncthreads();

    // vote mean, argmax and count: the epilogue of cls_tail_vote_kernel (restated, that kernel stays as the Point-MAE tests pin it)
    float* mrow = feat;
    for (int o = tid; o < cls_dim; o += TAIL_THREADS) {
        float s = 0.0f;
        for (int v = 0; v < V; ++v) {
            const float l = hid[v * TAIL_H + o];
            if (votes) votes[((size_t)v * B + b) * cls_dim + o] = l;
            s += l;
        }
        s = s / (float)V;
        mean[(size_t)b * cls_dim + o] = s;
        mrow[o] = s;
    }
    __syncthreads();
    if (tid == 0) {                                     // argmax, ties -> lowest index, NaN wins (torch.max)
        int best = 0;
        float bv = mrow[0];
        for (int o = 1; o < cls_dim; ++o) {
            const float l = mrow[o];
            if (bv == bv && (l > bv || l != l)) {
                bv = l;
                best = o;
            }
        }
        pred[b] = best;
        if ((long long)best == labels[b]) atomicAdd(correct, 1ull);
    }
}

}  // namespace

extern "C" int gm3d_vote_sample(const float* points, const int32_t* fps_idx, const long long* subsets, const float* scale,
                                const float* shift, int B, int N0, int point_all, int npoints, int V, float* out,
                                gm3d_stream_t stream) {
    if (!points || !fps_idx || !subsets || !scale || !shift || !out) return GM3D_EINVAL;
    if (B < 1 || N0 < 1 || point_all < 1 || npoints < 1 || V < 1 || point_all > N0 || npoints > point_all) return GM3D_EINVAL;
    const long long total = (long long)V * B * npoints;
    if (total * 3 > (1LL << 40)) return GM3D_EUNSUPPORTED;
    const long long want = (total + 255) / 256;
    const int grid = (int)(want < 8192 ? want : 8192);
    return launch_lds<vote_sample_kernel>(dim3(grid), dim3(256), 0, stream, points, fps_idx, subsets, scale, shift, B, N0, point_all,
                                          npoints, total, out);
}

extern "C" int gm3d_cls_tail_vote(const void* x, int V, int B, int T, int C, const float* W1, const float* b1, const float* g1,
                                  const float* be1, const float* rm1, const float* rv1, const float* W2, const float* b2,
                                  const float* g2, const float* be2, const float* rm2, const float* rv2, const float* W3,
                                  const float* b3, int cls_dim, float eps, const long long* labels, float* mean, long long* pred,
                                  long long* correct, float* votes, int dtype, gm3d_stream_t stream) {
    if (!x || !W1 || !b1 || !g1 || !be1 || !rm1 || !rv1 || !W2 || !b2 || !g2 || !be2 || !rm2 || !rv2 || !W3 || !b3 || !labels ||
        !mean || !pred || !correct)
        return GM3D_EINVAL;
    if (V < 1 || B < 1 || T < 1 || cls_dim < 1) return GM3D_EINVAL;
    if (C != TAIL_C || T < 2 || cls_dim > TAIL_H || V > VOTE_MAX_V || (dtype != GM3D_F32 && dtype != GM3D_BF16)) return GM3D_EUNSUPPORTED;
    if (((uintptr_t)x & 15) != 0) return GM3D_EUNSUPPORTED;     // 16-byte row loads
    const HeadArgs h{W1, b1, g1, be1, rm1, rv1, W2, b2, g2, be2, rm2, rv2, W3, b3};
    const size_t lds = (size_t)(V * 2 * TAIL_C + TAIL_TG * TAIL_C + V * TAIL_H) * sizeof(float);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(correct);
    return by_dtype(dtype, [&](auto* t) {
        using E = std::remove_pointer_t<decltype(t)>;
        return launch_lds<cls_tail_vote_kernel<E>>(dim3(B), dim3(TAIL_THREADS), lds, stream, (const E*)x, V, B, T, h, cls_dim, eps, labels,
                                                   mean, pred, cnt, votes);
    });
}

extern "C" int gm3d_cls_tail_vote_pool(const void* x, int V, int B, int T, int C, int mode, const float* W1, const float* b1,
                                       const float* g1, const float* be1, const float* rm1, const float* rv1, const float* W2,
                                       const float* b2, const float* g2, const float* be2, const float* rm2, const float* rv2,
                                       const float* W3, const float* b3, int cls_dim, float eps, const long long* labels, float* mean,
                                       long long* pred, long long* correct, float* votes, float* feat, int dtype, gm3d_stream_t stream) {
    if (V < 1 || B < 0 || T < 1 || cls_dim < 1) return GM3D_EINVAL;
    if (C != TAIL_C || T > POOL_MAX_T || cls_dim > TAIL_H || V > VOTE_MAX_V || (mode != 0 && mode != 1) ||
        (dtype != GM3D_F32 && dtype != GM3D_BF16))
        return GM3D_EUNSUPPORTED;
    if (B == 0) return GM3D_OK;
    if (!x || !W1 || !b1 || !g1 || !be1 || !rm1 || !rv1 || !W2 || !b2 || !g2 || !be2 || !rm2 || !rv2 || !W3 || !b3 || !labels ||
        !mean || !pred || !correct)
        return GM3D_EINVAL;
    if (((uintptr_t)x & 15) != 0) return GM3D_EUNSUPPORTED;     // 16-byte row loads
    const HeadArgs h{W1, b1, g1, be1, rm1, rv1, W2, b2, g2, be2, rm2, rv2, W3, b3};
    const int F = mode ? 2 * TAIL_C : TAIL_C;
    const size_t lds = (size_t)(V * F + V * TAIL_H) * sizeof(float);     // 64 KiB at V = 16, F = 768
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(correct);
    return by_dtype(dtype, [&](auto* t) {
        using E = std::remove_pointer_t<decltype(t)>;
        return launch_lds<cls_tail_vote_pool_kernel<E>>(dim3(B), dim3(TAIL_THREADS), lds, stream, (const E*)x, V, B, T, mode, h, cls_dim,
                                                        eps, labels, mean, pred, cnt, votes, feat);
    });
}
