// Classification tail of the Point-M2AE classifiers (gm3d_amd/point_m2ae_cls.py): token pooling, the three-layer head
// Linear / BatchNorm (training or eval) / ReLU / Dropout x 2 + Linear, and the mean cross-entropy, forward in two launches and
// backward in two.  Every sum runs in a fixed order in one thread (or a fixed butterfly in one wave): no float atomics, so a
// graph replay reproduces an eager call bit for bit.  See include/gm3d.h for the contracts.
#include "cls_pool.hpp"
#include "common.hpp"

using namespace gm3d;

namespace {

constexpr int CT_C = 384;            // token width
constexpr int CT_H = 256;            // hidden width of the head
constexpr int CT_MAX_B = 128;
constexpr int CT_MAX_T = 512;
constexpr int POOL_THREADS = 256;    // forward 1 / backward 2: one workgroup per cloud (and per weight-gradient block)
constexpr int HEAD_THREADS = 1024;   // forward 2 / backward 1: the batch-coupled part (BatchNorm statistics) in ONE workgroup
constexpr int RB = 8;                // rows per thread in the dense products of the head workgroup

template <class T> __device__ __forceinline__ float ld(const T* p) { return (float)*p; }
template <class T> __device__ __forceinline__ void st(T* p, float v) { *p = (T)v; }

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// ---------------------------------------------------------------------------------------------------------------- forward 1
// Workgroup b: mean and max over the T tokens of every channel (argmax: first maximum; a NaN wins, like torch.max), the pooled
// feature f (mode 0: mean + max, width C; mode 1: [mean ; max], width 2C) and the first Linear h1 = f W1^T + b1 (pre-BatchNorm).
template <class T>
__global__ __launch_bounds__(POOL_THREADS) void cls_pool_l1_kernel(const T* __restrict__ x, int T_, int mode, const float* __restrict__ W1,
                                                                   const float* __restrict__ b1, float* __restrict__ feat,
                                                                   int* __restrict__ argmax, float* __restrict__ h1) {
    __shared__ float f[2 * CT_C];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int F = mode ? 2 * CT_C : CT_C;
    const T* xb = x + (size_t)b * T_ * CT_C;
    for (int c = tid; c < CT_C; c += POOL_THREADS) {
        PoolAcc p;
        p.init(ld(xb + c));
        for (int t = 0; t < T_; ++t) p.add(ld(xb + (size_t)t * CT_C + c), t);
        argmax[(size_t)b * CT_C + c] = p.am;
        pool_feature(f, CT_C, c, mode, p.mean(T_), p.m);
    }
    __syncthreads();
    for (int k = tid; k < F; k += POOL_THREADS) feat[(size_t)b * F + k] = f[k];
    // one wave per output row: lanes read the weight row coalesced, a fixed butterfly sums the lanes
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = wave; o < CT_H; o += POOL_THREADS / 64) {
        const float* w = W1 + (size_t)o * F;
        float acc = 0.0f;
        for (int k = lane; k < F; k += 64) acc = fmaf(w[k], f[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) h1[(size_t)b * CT_H + o] = acc + b1[o];
    }
}

struct BnArgs {
    const float *g, *be;
    float *rm, *rv;
    long long* nbt;
};

// BatchNorm statistics of the B x 256 pre-activations h (one thread per column, rows in order) -> stat[0..255] mean,
// stat[256..511] 1 / sqrt(var + eps); training: batch mean and biased variance, running statistics updated; eval: running ones.
__device__ void bn_stats(const float* __restrict__ h, int B, BnArgs bn, float eps, float momentum, int training, float* __restrict__ stat) {
    const int o = threadIdx.x;
    if (o < CT_H) {
        float mean, var;
        if (training) {
            float s = 0.0f;
            for (int b = 0; b < B; ++b) s += h[(size_t)b * CT_H + o];
            mean = s / (float)B;
            float q = 0.0f;
            for (int b = 0; b < B; ++b) {
                const float d = h[(size_t)b * CT_H + o] - mean;
                q = fmaf(d, d, q);
            }
            var = q / (float)B;
            bn.rm[o] = (1.0f - momentum) * bn.rm[o] + momentum * mean;
            bn.rv[o] = (1.0f - momentum) * bn.rv[o] + momentum * (var * (float)B / (float)(B - 1));
        } else {
            mean = bn.rm[o];
            var = bn.rv[o];
        }
        stat[o] = mean;
        stat[CT_H + o] = 1.0f / sqrtf(var + eps);
    }
    if (training && threadIdx.x == 0) bn.nbt[0] += 1;
}

// a = max(xhat * gamma + beta, 0) * dropout factor
__device__ __forceinline__ float bn_act(float h, const float* stat, const float* g, const float* be, const float* drop, size_t i, int o) {
    const float y = (h - stat[o]) * stat[CT_H + o] * g[o] + be[o];
    const float a = fmaxf(y, 0.0f);
    return drop ? a * drop[i] : a;
}

// out[b][o] = in[b][:] . W[o][:] + bias[o], b < B, o < N; in: B x 256 in LDS, W: N x 256 (16-byte aligned rows).
// A thread owns one column o and RB rows: the weight row is read once per row block, the LDS rows are broadcasts.
__device__ void dense256(const float* __restrict__ in, const float* __restrict__ W, const float* __restrict__ bias, int B, int N,
                         float* __restrict__ out) {
    const int nrb = (B + RB - 1) / RB;
    for (int item = threadIdx.x; item < N * nrb; item += HEAD_THREADS) {
        const int o = item % N, r0 = (item / N) * RB;
        float acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = 0.0f;
        const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)o * CT_H);
        for (int k4 = 0; k4 < CT_H / 4; ++k4) {
            const float4 w = w4[k4];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r0 + r < B) {
                    const float4 a = reinterpret_cast<const float4*>(in + (size_t)(r0 + r) * CT_H)[k4];
                    acc[r] = fmaf(w.x, a.x, acc[r]);
                    acc[r] = fmaf(w.y, a.y, acc[r]);
                    acc[r] = fmaf(w.z, a.z, acc[r]);
                    acc[r] = fmaf(w.w, a.w, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (r0 + r < B) out[(size_t)(r0 + r) * N + o] = acc[r] + bias[o];
    }
}

struct HeadFwd {
    const float *W2, *b2, *W3, *b3;
    BnArgs bn1, bn2;
    const float* drop;        // (2,B,256) or NULL
    const long long* labels;  // (B) or NULL
    float* h;                 // (2,B,256): h1 (written by forward 1), h2
    float* stats;             // (4,256)
    float* logits;            // (B,cls_dim)
    float* loss;              // (1) or NULL
};

// ---------------------------------------------------------------------------------------------------------------- forward 2
// The batch-coupled rest in one workgroup: BatchNorm 1 (+ running statistics), ReLU, Dropout, Linear 2, BatchNorm 2, ReLU,
// Dropout, Linear 3, cross-entropy.  The activations (B x 256) live in LDS; h2 goes to global memory (saved for backward).
__global__ __launch_bounds__(HEAD_THREADS) void cls_head_fwd_kernel(int B, int cls_dim, float eps, float momentum, int training, HeadFwd a) {
    extern __shared__ float lds[];
    float* act = lds;                     // B x 256
    float* rowl = act + (size_t)B * CT_H; // B per-row losses
    const int tid = threadIdx.x;
    const float* drop1 = (training && a.drop) ? a.drop : nullptr;
    const float* drop2 = (training && a.drop) ? a.drop + (size_t)B * CT_H : nullptr;
    float* h1 = a.h;
    float* h2 = a.h + (size_t)B * CT_H;
    bn_stats(h1, B, a.bn1, eps, momentum, training, a.stats);
    __syncthreads();
    for (int i = tid; i < B * CT_H; i += HEAD_THREADS) act[i] = bn_act(h1[i], a.stats, a.bn1.g, a.bn1.be, drop1, i, i % CT_H);
    __syncthreads();
    dense256(act, a.W2, a.b2, B, CT_H, h2);
    __syncthreads();
    bn_stats(h2, B, a.bn2, eps, momentum, training, a.stats + 2 * CT_H);
    __syncthreads();
    for (int i = tid; i < B * CT_H; i += HEAD_THREADS) act[i] = bn_act(h2[i], a.stats + 2 * CT_H, a.bn2.g, a.bn2.be, drop2, i, i % CT_H);
    __syncthreads();
    dense256(act, a.W3, a.b3, B, cls_dim, a.logits);
    if (!a.labels) return;
    __syncthreads();
    if (tid < B) {                        // -log softmax(z)[label]; a label outside [0, cls_dim) gives NaN
        const float* z = a.logits + (size_t)tid * cls_dim;
        float m = z[0];
        for (int o = 1; o < cls_dim; ++o) m = fmaxf(m, z[o]);
        float s = 0.0f;
        for (int o = 0; o < cls_dim; ++o) s += expf(z[o] - m);
        const long long y = a.labels[tid];
        rowl[tid] = (y >= 0 && y < cls_dim) ? (m + logf(s)) - z[y] : __builtin_nanf("");
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
        for (int b = 0; b < B; ++b) s += rowl[b];
        a.loss[0] = s / (float)B;
    }
}

// For every row b < B and column k < 256: epi(b, k, sum_o G[b][o] W[o][k]), o < No (G: B x ldg, W: No x 256, both global).
// A thread owns one column k and RB rows: each weight element is loaded once for RB independent sums, the G rows are wave-uniform.
template <class Epi>
__device__ void dense_t(const float* __restrict__ G, int ldg, const float* __restrict__ W, int No, int B, Epi epi) {
    const int nrb = (B + RB - 1) / RB;
    for (int item = threadIdx.x; item < CT_H * nrb; item += HEAD_THREADS) {
        const int k = item % CT_H, r0 = (item / CT_H) * RB;
        float acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = 0.0f;
        for (int o = 0; o < No; ++o) {
            const float w = W[(size_t)o * CT_H + k];
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (r0 + r < B) acc[r] = fmaf(G[(size_t)(r0 + r) * ldg + o], w, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (r0 + r < B) epi(r0 + r, k, acc[r]);
    }
}

struct HeadBwd {
    const float *W2, *W3, *g1, *be1, *g2, *be2;
    const float* drop;
    const long long* labels;
    const float *h, *stats, *logits, *dlogits, *dloss;
    float* ws;                // (5,B,256): dz, a1', dy2 / dh2, dy1 / dh1, a2'
    float *db1, *dg1, *dbe1, *dg2, *dbe2;
};

// dy (B x 256, in place) -> the pre-BatchNorm gradient dh; dgamma, dbeta (one thread per column, rows in order).
// training: dh = gamma * rstd / B * (B dy - sum dy - xhat sum(dy xhat)); eval: dh = gamma * rstd * dy.
__device__ void bn_bwd(float* __restrict__ dy, const float* __restrict__ h, const float* stat, const float* g, int B, int training,
                       float* __restrict__ dg, float* __restrict__ dbe, float* __restrict__ dbias) {
    const int o = threadIdx.x;
    if (o >= CT_H) return;
    const float mu = stat[o], rs = stat[CT_H + o];
    float s1 = 0.0f, s2 = 0.0f;
    for (int b = 0; b < B; ++b) {
        const float d = dy[(size_t)b * CT_H + o];
        s1 += d;
        s2 = fmaf(d, (h[(size_t)b * CT_H + o] - mu) * rs, s2);
    }
    dg[o] = s2;
    dbe[o] = s1;
    const float k = g[o] * rs;
    float sb = 0.0f;
    for (int b = 0; b < B; ++b) {
        const size_t i = (size_t)b * CT_H + o;
        float dh;
        if (training) {
            const float xh = (h[i] - mu) * rs;
            dh = k / (float)B * (((float)B * dy[i] - s1) - xh * s2);
        } else {
            dh = k * dy[i];
        }
        dy[i] = dh;
        sb += dh;
    }
    if (dbias) dbias[o] = sb;
}

// ---------------------------------------------------------------------------------------------------------------- backward 1
// Logit gradient (+ the cross-entropy's), Linear 3 backward, Dropout / ReLU / BatchNorm 2 backward, the input gradient of Linear
// 2, Dropout / ReLU / BatchNorm 1 backward -> dz, a2', dh2, a1', dh1 for backward 2.  One workgroup; the B x 256 tensors in `ws`.
__global__ __launch_bounds__(HEAD_THREADS) void cls_head_bwd_kernel(int B, int cls_dim, int training, HeadBwd a) {
    __shared__ float lse[CT_MAX_B];
    const int tid = threadIdx.x;
    const size_t BH = (size_t)B * CT_H;
    float *dz = a.ws, *act = a.ws + BH, *dh2 = a.ws + 2 * BH, *dh1 = a.ws + 3 * BH, *act2 = a.ws + 4 * BH;
    const float *h1 = a.h, *h2 = a.h + BH, *st1 = a.stats, *st2 = a.stats + 2 * CT_H;
    const float* drop1 = (training && a.drop) ? a.drop : nullptr;
    const float* drop2 = (training && a.drop) ? a.drop + BH : nullptr;
    const bool ce = a.dloss && a.labels;
    if (ce && tid < B) {
        const float* z = a.logits + (size_t)tid * cls_dim;
        float m = z[0];
        for (int o = 1; o < cls_dim; ++o) m = fmaxf(m, z[o]);
        float s = 0.0f;
        for (int o = 0; o < cls_dim; ++o) s += expf(z[o] - m);
        lse[tid] = m + logf(s);
    }
    __syncthreads();
    const float gl = ce ? a.dloss[0] / (float)B : 0.0f;
    for (int i = tid; i < B * cls_dim; i += HEAD_THREADS) {
        const int b = i / cls_dim, o = i - b * cls_dim;
        float d = a.dlogits ? a.dlogits[i] : 0.0f;
        if (ce) {
            const long long y = a.labels[b];
            d += gl * (expf(a.logits[i] - lse[b]) - (y == o ? 1.0f : 0.0f));
        }
        dz[i] = d;
    }
    for (int i = tid; i < B * CT_H; i += HEAD_THREADS) act2[i] = bn_act(h2[i], st2, a.g2, a.be2, drop2, i, i % CT_H);
    __syncthreads();
    // Linear 3 input gradient da2' = dz W3 -> dy2 (through Dropout and ReLU); dW3 = dz^T a2' and db3 in backward 2
    dense_t(dz, cls_dim, a.W3, cls_dim, B, [&](int b, int k, float s) {
        const size_t i = (size_t)b * CT_H + k;
        const float y = (h2[i] - st2[k]) * st2[CT_H + k] * a.g2[k] + a.be2[k];
        dh2[i] = y > 0.0f ? (drop2 ? s * drop2[i] : s) : 0.0f;
    });
    __syncthreads();
    bn_bwd(dh2, h2, st2, a.g2, B, training, a.dg2, a.dbe2, nullptr);   // dh2 in place; db2 is its column sum (backward 2)
    __syncthreads();
    // Linear 2 input gradient da1' = dh2 W2 -> dy1; a1' for dW2 (backward 2)
    dense_t(dh2, CT_H, a.W2, CT_H, B, [&](int b, int k, float s) {
        const size_t i = (size_t)b * CT_H + k;
        const float y = (h1[i] - st1[k]) * st1[CT_H + k] * a.g1[k] + a.be1[k];
        dh1[i] = y > 0.0f ? (drop1 ? s * drop1[i] : s) : 0.0f;
        act[i] = bn_act(h1[i], st1, a.g1, a.be1, drop1, i, k);
    });
    __syncthreads();
    bn_bwd(dh1, h1, st1, a.g1, B, training, a.dg1, a.dbe1, a.db1);
}

// ---------------------------------------------------------------------------------------------------------------- backward 2
// Workgroups [0, B): cloud b -- df = dh1[b] W1, then dx[b][t][c] = dmean[c] / T + (t == argmax[b][c]) dmax[c].
// Workgroups [B, B + F): 256 entries of dW1 = dh1^T f each.  Workgroups [B + F, B + F + 256): row o of dW2 = dh2^T a1' and db2[o];
// [B + F + 256, B + F + 256 + cls_dim): row o of dW3 = dz^T a2' and db3[o].
template <class T>
__global__ __launch_bounds__(POOL_THREADS) void cls_pool_bwd_kernel(int B, int T_, int mode, int cls_dim, const float* __restrict__ W1,
                                                                    const float* __restrict__ feat, const int* __restrict__ argmax,
                                                                    const float* __restrict__ ws, T* __restrict__ dx, float* __restrict__ dW1,
                                                                    float* __restrict__ dW2, float* __restrict__ db2, float* __restrict__ dW3,
                                                                    float* __restrict__ db3) {
    __shared__ float df[2 * CT_C];
    const int F = mode ? 2 * CT_C : CT_C;
    const size_t BH = (size_t)B * CT_H;
    const float *dz = ws, *act = ws + BH, *dh2 = ws + 2 * BH, *dh1 = ws + 3 * BH, *act2 = ws + 4 * BH;
    const int tid = threadIdx.x, blk = blockIdx.x;
    if (blk < B) {
        const int b = blk;
        for (int k = tid; k < F; k += POOL_THREADS) {
            float s = 0.0f;
            for (int o = 0; o < CT_H; ++o) s = fmaf(dh1[(size_t)b * CT_H + o], W1[(size_t)o * F + k], s);
            df[k] = s;
        }
        __syncthreads();
        const float invT = 1.0f / (float)T_;
        const int* am = argmax + (size_t)b * CT_C;
        T* dxb = dx + (size_t)b * T_ * CT_C;
        for (int i = tid; i < T_ * CT_C; i += POOL_THREADS) {
            const int t = i / CT_C, c = i - t * CT_C;
            const float gm = df[c], gx = mode ? df[CT_C + c] : df[c];
            st(dxb + i, gm * invT + (am[c] == t ? gx : 0.0f));
        }
        return;
    }
    if (blk < B + F) {
        const int e = (blk - B) * POOL_THREADS + tid;      // < 256 * F
        const int o = e / F, k = e - o * F;
        float s = 0.0f;
        for (int b = 0; b < B; ++b) s = fmaf(dh1[(size_t)b * CT_H + o], feat[(size_t)b * F + k], s);
        dW1[e] = s;
        return;
    }
    if (blk < B + F + CT_H) {
        const int o = blk - B - F, k = tid;                 // o < 256, k < 256
        float s = 0.0f, sb = 0.0f;
        for (int b = 0; b < B; ++b) {
            const float d = dh2[(size_t)b * CT_H + o];
            s = fmaf(d, act[(size_t)b * CT_H + k], s);
            sb += d;
        }
        dW2[(size_t)o * CT_H + k] = s;
        if (k == 0) db2[o] = sb;
        return;
    }
    const int o = blk - B - F - CT_H, k = tid;              // o < cls_dim, k < 256
    float s = 0.0f, sb = 0.0f;
    for (int b = 0; b < B; ++b) {
        const float d = dz[(size_t)b * cls_dim + o];
        s = fmaf(d, act2[(size_t)b * CT_H + k], s);
        sb += d;
    }
    dW3[(size_t)o * CT_H + k] = s;
    if (k == 0) db3[o] = sb;
}

int check_shape(int B, int T, int C, int mode, int cls_dim, int dtype) {
    if (B < 0 || T < 1 || cls_dim < 1) return GM3D_EINVAL;
    if (C != CT_C || B > CT_MAX_B || T > CT_MAX_T || cls_dim > CT_H || (mode != 0 && mode != 1) || (dtype != GM3D_F32 && dtype != GM3D_BF16))
        return GM3D_EUNSUPPORTED;
    return GM3D_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int gm3d_cls_tail_fwd(const void* x, int B, int T, int C, int mode, const float* W1, const float* b1, const float* g1,
                                 const float* be1, const float* W2, const float* b2, const float* g2, const float* be2, const float* W3,
                                 const float* b3, int cls_dim, float* rm1, float* rv1, long long* nbt1, float* rm2, float* rv2,
                                 long long* nbt2, float eps, float momentum, int training, const float* drop, const long long* labels,
                                 float* feat, int* argmax, float* h, float* stats, float* logits, float* loss, int dtype,
                                 gm3d_stream_t stream) {
    const int rc = check_shape(B, T, C, mode, cls_dim, dtype);
    if (rc != GM3D_OK) return rc;
    if (B == 0) return GM3D_OK;
    if (!x || !W1 || !b1 || !g1 || !be1 || !W2 || !b2 || !g2 || !be2 || !W3 || !b3 || !rm1 || !rv1 || !rm2 || !rv2 || !feat || !argmax ||
        !h || !stats || !logits || (labels && !loss))
        return GM3D_EINVAL;
    if (training && (B < 2 || !nbt1 || !nbt2)) return GM3D_EINVAL;         // batch statistics need two rows
    if (!aligned16(W2) || !aligned16(W3)) return GM3D_EUNSUPPORTED;          // 16-byte weight-row loads
    const int r = by_dtype(dtype, [&](auto* t) {
        using E = std::remove_pointer_t<decltype(t)>;
        return launch_lds<cls_pool_l1_kernel<E>>(dim3(B), dim3(POOL_THREADS), 0, stream, (const E*)x, T, mode, W1, b1, feat, argmax, h);
    });
    if (r != GM3D_OK) return r;
    const HeadFwd a{W2, b2, W3, b3, BnArgs{g1, be1, rm1, rv1, nbt1}, BnArgs{g2, be2, rm2, rv2, nbt2}, drop, labels, h, stats, logits, loss};
    const size_t lds = ((size_t)B * CT_H + B) * sizeof(float);
    return launch_lds<cls_head_fwd_kernel>(dim3(1), dim3(HEAD_THREADS), lds, stream, B, cls_dim, eps, momentum, training, a);
}

extern "C" int gm3d_cls_tail_bwd(int B, int T, int C, int mode, const float* W1, const float* g1, const float* be1, const float* W2,
                                 const float* g2, const float* be2, const float* W3, int cls_dim, int training, const float* drop,
                                 const long long* labels, const float* feat, const int* argmax, const float* h, const float* stats,
                                 const float* logits, const float* dlogits, const float* dloss, float* ws, void* dx, float* dW1,
                                 float* db1, float* dg1, float* dbe1, float* dW2, float* db2, float* dg2, float* dbe2, float* dW3,
                                 float* db3, int dtype, gm3d_stream_t stream) {
    const int rc = check_shape(B, T, C, mode, cls_dim, dtype);
    if (rc != GM3D_OK) return rc;
    if (B == 0) return GM3D_OK;
    if (!W1 || !g1 || !be1 || !W2 || !g2 || !be2 || !W3 || !feat || !argmax || !h || !stats || !logits || !ws || !dx || !dW1 || !db1 ||
        !dg1 || !dbe1 || !dW2 || !db2 || !dg2 || !dbe2 || !dW3 || !db3 || (dloss && !labels))
        return GM3D_EINVAL;
    if (training && B < 2) return GM3D_EINVAL;
    const HeadBwd a{W2, W3, g1, be1, g2, be2, drop, labels, h, stats, logits, dlogits, dloss, ws, db1, dg1, dbe1, dg2, dbe2};
    int r = launch_lds<cls_head_bwd_kernel>(dim3(1), dim3(HEAD_THREADS), 0, stream, B, cls_dim, training, a);
    if (r != GM3D_OK) return r;
    const int F = mode ? 2 * CT_C : CT_C;
    const dim3 grid(B + F + CT_H + cls_dim);
    return by_dtype(dtype, [&](auto* t) {
        using E = std::remove_pointer_t<decltype(t)>;
        return launch_lds<cls_pool_bwd_kernel<E>>(grid, dim3(POOL_THREADS), 0, stream, B, T, mode, cls_dim, W1, feat, argmax,
                                                  (const float*)ws, (E*)dx, dW1, dW2, db2, dW3, db3);
    });
}
