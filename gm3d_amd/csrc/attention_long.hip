// Masked multi-head attention for 513 .. 2048 tokens per cloud: the operator of attention_masked.hip (same layouts, same mask
// semantics, same rounding points) with the head STREAMED through LDS instead of held there.  attention_masked.hip owns T <= 512
// and is not touched by this file; gm3d_attention_long_* refuse that range.
//
// Who needs it: the Point-MAE family's 8k fine-tune recipe (512 groups of 32 + the class token = 513 tokens), and the hierarchical
// encoder's level 0 at N = 4096 / 8192 (1024 / 2048 tokens at the published ratios).
//
// bf16.  A wave owns a 32-row tile exactly as in attention_masked.hip -- a query (forward, dQ) or a key (dK, dV) is a lane, the other
// side's 32 rows are accumulator registers -- and walks the other side's tiles with the same statements: the mask word of the
// (own row, tile) pair is applied before the maximum, a tile that is blocked for all 64 lanes is skipped (exact: it would add
// exp(-inf) = 0 everywhere), a lane for which a computed tile is fully blocked keeps its running maximum and sum untouched
// (alpha = 1, p = 0, never exp(-inf - -inf)).  What differs is where the other side's rows come from: the workgroup stages them in
// CHUNKS of 64 rows (two tiles) into one of two LDS buffers while it computes on the other, one __syncthreads per chunk.
//
//   forward   grid (B*H, ceil(T / 256)), 512 threads: 8 query tiles per workgroup; per buffer a K and a V image of 64 rows.
//             LDS = (2 * 2 * 64 + 256) * (2 HD + 16) bytes: 24 / 40 / 72 KiB at HD = 16 / 32 / 64 (occupancy not measured).
//   backward  ONE launch, grid (B*H, ceil(T / 128)), 512 threads (with 8 tiles and 1024 threads the 128 registers of a wave do not
//             hold the staging loads beside the accumulators: 55 .. 128 spilled): waves 0..3 own key
//             tiles (dK, dV) and walk the query chunks, waves 4..7 own the query tiles of the same rows (dQ) and walk the key
//             chunks -- so one chunk buffer holds rows [64 c, 64 c + 64) of Q, K, V and dO plus their lse and delta, and both kinds of
//             wave read the chunk that was staged once.  delta = rowsum(dO * O) is formed while staging (and by a query wave for its
//             own row, with the same statements).  LDS = 2 * (4 * 64 * (2 HD + 16) + 512) bytes: 25 / 41 / 73 KiB.
//             Every row of dQ, dK and dV has one owner, which writes it once after its walk, in the order the shapes fix: no
//             atomics, no zero-fill, two runs give the same bits.  Two launches (dK/dV, then dQ) would stage Q and dO for the one and
//             K and V for the other: the same chunks from global memory twice, and the second launch's P recomputed without the
//             first one's loads to share; a single launch with a split over key owners only would need atomics for dQ.
//
// f32 (parity mode): the same walk on the exact-fp32 MFMA (32x32x2: fp32 products, fp32 sums, one fixed order), fp32 images of
// pitch HD + 1 floats, expf / logf, `s * scale - m` never contracted into an fma.  LDS: forward 17 / 33 / 65 KiB, backward
// 35 / 67 / 131 KiB.
#include "mattn.hpp"

namespace gm3d {

constexpr int LCH = 64;                             // rows per staged chunk = two 32-row tiles

// this lane's own row fragment (8 consecutive d starting at 8 * ch) straight from global memory; rows >= T: zeros
__device__ __forceinline__ bf16x8 own_row(const bf16_t* src, size_t row_stride, int row, bool ok, int ch) {
    return ok ? *reinterpret_cast<const bf16x8*>(src + (size_t)row * row_stride + ch * 8) : zero8();
}

// ===================================================================== forward, bf16
template <int HD>
__global__ __launch_bounds__(512) void lattn_fwd_bf16_kernel(const bf16_t* __restrict__ qkv, const unsigned* __restrict__ mask,
                                                             bf16_t* __restrict__ out, float* __restrict__ lse, int T, int H, int W,
                                                             float scale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    using I = MImg<HD>;
    constexpr int NWV = 8, NTH = 64 * NWV;
    constexpr int KS = HD / 16;                     // k-steps of the q.k product
    constexpr int DT = (HD + 31) / 32;              // 32-row tiles of the transposed output
    constexpr int IMG = LCH * I::PITCH;             // one chunk image; a buffer is K | V
    const int NK = (T + 31) >> 5, NC = (T + LCH - 1) / LCH;
    unsigned char* Qi = lsm + 4 * IMG;
    int bh_, yb_;
    mattn_block(bh_, yb_);
    const int b = bh_ / H, h = bh_ % H;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const size_t rs = (size_t)3 * H * HD, os = (size_t)H * HD;
    const bf16_t* Qg = qkv + (size_t)b * T * rs + (size_t)h * HD;
    const bf16_t* Kg = Qg + os;
    const bf16_t* Vg = Qg + 2 * os;
    const int q0 = 32 * NWV * yb_;
    I::stage(Qi, Qg + (size_t)q0 * rs, rs, T - q0, 32 * NWV, tid, NTH);
    I::stage(lsm, Kg, rs, T, LCH, tid, NTH);
    I::stage(lsm + IMG, Vg, rs, T, LCH, tid, NTH);
    __syncthreads();
    const int q = q0 + 32 * w + r;                  // this lane's query
    const bool active = q0 + 32 * w < T;            // wave-uniform; a wave past the end still stages and meets the barriers
    const bool q_ok = q < T;
    const unsigned* mrow = mask ? mask + ((size_t)b * T + (q_ok ? q : 0)) * W : nullptr;
    bf16x8 fq[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) fq[s] = I::row(Qi, 32 * w + r, 2 * s + hh);
    float m = -INFINITY, l = 0.f;
    f32x16 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) o[d] = zero16();
    const int cb = 16 * ((lane >> 4) & 1);
    for (int c = 0; c < NC; ++c) {
        const unsigned char* Ki = lsm + (c & 1) * 2 * IMG;
        const unsigned char* Vi = Ki + IMG;
        if (c + 1 < NC) {                           // the next chunk into the other buffer (last read before the previous barrier)
            unsigned char* nb = lsm + ((c + 1) & 1) * 2 * IMG;
            const int k1 = LCH * (c + 1);
            I::stage(nb, Kg + (size_t)k1 * rs, rs, T - k1, LCH, tid, NTH);
            I::stage(nb + IMG, Vg + (size_t)k1 * rs, rs, T - k1, LCH, tid, NTH);
        }
        if (active) {
#pragma unroll 1
            for (int t = 0; t < LCH / 32; ++t) {
                const int kt = (LCH / 32) * c + t;
                if (kt >= NK) break;
                // as in mattn_fwd_bf16_kernel: a key tile blocked for every query of the wave's tile changes no bit when skipped
                const unsigned mw = mask_word(mrow, q_ok, kt, T);
                if (__ballot(mw != 0xffffffffu) == 0ull) continue;
                f32x16 st = zero16();
#pragma unroll
                for (int s = 0; s < KS; ++s) st = mfma_bf16(I::row(Ki, 32 * t + r, 2 * s + hh), fq[s], st);
                float tm = -INFINITY;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    st[g] = ((mw >> crow(g, hh)) & 1u) ? -INFINITY : st[g] * scale;
                    tm = fmaxf(tm, st[g]);
                }
                tm = fmaxf(tm, __shfl_xor(tm, 32));
                const float mn = fmaxf(m, tm);
                // no allowed key so far, this tile included: mn = -inf, the running state stays (alpha = 1, p = 0); the first
                // allowed key of a row after such tiles: m = -inf, mn finite, alpha = exp(-inf) = 0 on a zero state
                const float alpha = mn == -INFINITY ? 1.f : __expf(m - mn);
                float ts = 0.f;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    st[g] = mn == -INFINITY ? 0.f : __expf(st[g] - mn);
                    ts += st[g];
                }
                ts += __shfl_xor(ts, 32);
                l = l * alpha + ts;
                m = mn;
#pragma unroll
                for (int d = 0; d < DT; ++d)
#pragma unroll
                    for (int g = 0; g < 16; ++g) o[d][g] *= alpha;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 p = cvt8(st, s, 1.0f);
#pragma unroll
                    for (int d = 0; d < DT; ++d) o[d] = mfma_bf16(I::tr8(Vi, 32 * t, s, hh, 32 * d + cb, lane), p, o[d]);
                }
            }
        }
        __syncthreads();
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    if (active && q_ok) {
        bf16_t* og = out + ((size_t)b * T + q) * os + (size_t)h * HD;
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * d + 8 * g4 + 4 * hh;
                if (d0 < HD) {
                    bf16x4 pk;
#pragma unroll
                    for (int e = 0; e < 4; ++e) pk[e] = (bf16_t)(o[d][4 * g4 + e] * inv);
                    *reinterpret_cast<bf16x4*>(og + d0) = pk;
                }
            }
        if (hh == 0) lse[((size_t)b * H + h) * T + q] = l > 0.f ? m + logf(l) : 0.f;
    }
}

// ===================================================================== backward, bf16
// delta[q] = sum_d dO[q][d] * O[q][d], in the one order both of its users take
template <int HD> __device__ __forceinline__ float lattn_delta(const bf16_t* o, const bf16_t* d) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < HD / 8; ++c) {
        const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(o + c * 8);
        const bf16x8 d8 = *reinterpret_cast<const bf16x8*>(d + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (float)o8[j] * (float)d8[j];
    }
    return acc;
}

template <int HD>
__global__ __launch_bounds__(512) void lattn_bwd_bf16_kernel(const bf16_t* __restrict__ qkv, const unsigned* __restrict__ mask,
                                                                   const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                                   const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int T,
                                                                   int H, int W, float scale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    using I = MImg<HD>;
    constexpr int NTP = 4, KS = HD / 16, DT = (HD + 31) / 32, NTH = 128 * NTP;
    constexpr int IMG = LCH * I::PITCH;
    constexpr int BUF = 4 * IMG + 2 * LCH * (int)sizeof(float);       // Q | K | V | dO | lse | delta of one chunk
    const int NT = (T + 31) >> 5, NC = (T + LCH - 1) / LCH;
    int bh_, yb_;
    mattn_block(bh_, yb_);
    const int b = bh_ / H, h = bh_ % H;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const size_t rs = (size_t)3 * H * HD, os = (size_t)H * HD;
    const bf16_t* Qg = qkv + (size_t)b * T * rs + (size_t)h * HD;
    const bf16_t* Og = out + (size_t)b * T * os + (size_t)h * HD;
    const bf16_t* Dg = dout + (size_t)b * T * os + (size_t)h * HD;
    const float* Lg = lse + ((size_t)b * H + h) * T;
    auto stage_chunk = [&](unsigned char* buf, int c) {
        const int r0 = LCH * c;
        I::stage(buf, Qg + (size_t)r0 * rs, rs, T - r0, LCH, tid, NTH);
        I::stage(buf + IMG, Qg + os + (size_t)r0 * rs, rs, T - r0, LCH, tid, NTH);
        I::stage(buf + 2 * IMG, Qg + 2 * os + (size_t)r0 * rs, rs, T - r0, LCH, tid, NTH);
        I::stage(buf + 3 * IMG, Dg + (size_t)r0 * os, os, T - r0, LCH, tid, NTH);
        float* Ls = reinterpret_cast<float*>(buf + 4 * IMG);
        if (tid < LCH) {
            const int i = r0 + tid;
            Ls[tid] = i < T ? Lg[i] : 0.f;
            Ls[LCH + tid] = i < T ? lattn_delta<HD>(Og + (size_t)i * os, Dg + (size_t)i * os) : 0.f;
        }
    };
    stage_chunk(lsm, 0);
    __syncthreads();
    bf16_t* dQg = dqkv + (size_t)b * T * rs + (size_t)h * HD;
    const int cb = 16 * ((lane >> 4) & 1);
    const int tile = NTP * yb_ + (w < NTP ? w : w - NTP);
    const bool active = 32 * tile < T;              // wave-uniform; a wave past the end still stages and meets the barriers
    const int row = 32 * tile + r;                  // this lane's key (waves 0..NTP-1) or query (waves NTP..2 NTP-1)
    const bool row_ok = row < T;
    const unsigned* mrow = mask ? mask + ((size_t)b * T + (row_ok ? row : 0)) * W : nullptr;
    f32x16 x[DT], y[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) { x[d] = zero16(); y[d] = zero16(); }
    // own-row fragments: K and V of the lane's key, or Q and dO of the lane's query
    bf16x8 fa[KS], fb[KS];
    const bool keyw = w < NTP;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        fa[s] = keyw ? own_row(Qg + os, rs, row, row_ok, 2 * s + hh) : own_row(Qg, rs, row, row_ok, 2 * s + hh);
        fb[s] = keyw ? own_row(Qg + 2 * os, rs, row, row_ok, 2 * s + hh) : own_row(Dg, os, row, row_ok, 2 * s + hh);
    }
    float lq = 0.f, dq_ = 0.f;
    if (!keyw && row_ok) {
        lq = Lg[row];
        dq_ = lattn_delta<HD>(Og + (size_t)row * os, Dg + (size_t)row * os);
    }
    for (int c = 0; c < NC; ++c) {
        const unsigned char* Qi = lsm + (c & 1) * BUF;
        const unsigned char* Ki = Qi + IMG;
        const unsigned char* Vi = Ki + IMG;
        const unsigned char* Di = Vi + IMG;
        const float* Ls = reinterpret_cast<const float*>(Di + IMG);
        const float* Del = Ls + LCH;
        if (c + 1 < NC) stage_chunk(lsm + ((c + 1) & 1) * BUF, c + 1);
        if (active && keyw) {
            // phase A: X[q][key] tiles (rows = q in registers, cols = key on the lane); the mask is symmetric: row `key`, word qt
#pragma unroll 1
            for (int t = 0; t < LCH / 32; ++t) {
                const int qt = (LCH / 32) * c + t;
                if (qt >= NT) break;
                const unsigned mw = mask_word(mrow, row_ok, qt, T);
                if (__ballot(mw != 0xffffffffu) == 0ull) continue;        // every pair of this tile blocked: p = 0 throughout (exact)
                f32x16 s = zero16(), dp = zero16();
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    s = mfma_bf16(I::row(Qi, 32 * t + r, 2 * ks + hh), fa[ks], s);
                    dp = mfma_bf16(I::row(Di, 32 * t + r, 2 * ks + hh), fb[ks], dp);
                }
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int ql = 32 * t + crow(g, hh);
                    const float p = ((mw >> crow(g, hh)) & 1u) ? 0.f : __expf(s[g] * scale - Ls[ql]);
                    s[g] = p;
                    dp[g] = p * (dp[g] - Del[ql]);
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 pa = cvt8(s, ks, 1.0f), da = cvt8(dp, ks, scale);
#pragma unroll
                    for (int d = 0; d < DT; ++d) {
                        x[d] = mfma_bf16(I::tr8(Di, 32 * t, ks, hh, 32 * d + cb, lane), pa, x[d]);      // dV^T[d][key]
                        y[d] = mfma_bf16(I::tr8(Qi, 32 * t, ks, hh, 32 * d + cb, lane), da, y[d]);      // dK^T[d][key]
                    }
                }
            }
        } else if (active) {
            // phase B: X'[key][q] tiles (rows = key in registers, cols = q on the lane)
#pragma unroll 1
            for (int t = 0; t < LCH / 32; ++t) {
                const int kt = (LCH / 32) * c + t;
                if (kt >= NT) break;
                const unsigned mw = mask_word(mrow, row_ok, kt, T);
                if (__ballot(mw != 0xffffffffu) == 0ull) continue;
                f32x16 s = zero16(), dp = zero16();
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    s = mfma_bf16(I::row(Ki, 32 * t + r, 2 * ks + hh), fa[ks], s);
                    dp = mfma_bf16(I::row(Vi, 32 * t + r, 2 * ks + hh), fb[ks], dp);
                }
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float p = ((mw >> crow(g, hh)) & 1u) ? 0.f : __expf(s[g] * scale - lq);
                    dp[g] = p * (dp[g] - dq_);
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 da = cvt8(dp, ks, scale);
#pragma unroll
                    for (int d = 0; d < DT; ++d) x[d] = mfma_bf16(I::tr8(Ki, 32 * t, ks, hh, 32 * d + cb, lane), da, x[d]);   // dQ^T[d][q]
                }
            }
        }
        __syncthreads();
    }
    if (active && row_ok) {
        bf16_t* g0 = dQg + (size_t)row * rs + (keyw ? 2 * os : 0);        // dV (key waves) / dQ (query waves)
        bf16_t* g1 = dQg + (size_t)row * rs + os;                         // dK
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * d + 8 * g4 + 4 * hh;
                if (d0 < HD) {
                    bf16x4 pk, pk2;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { pk[e] = (bf16_t)x[d][4 * g4 + e]; pk2[e] = (bf16_t)y[d][4 * g4 + e]; }
                    *reinterpret_cast<bf16x4*>(g0 + d0) = pk;
                    if (keyw) *reinterpret_cast<bf16x4*>(g1 + d0) = pk2;
                }
            }
    }
}

// ===================================================================== f32 (parity mode): exact-fp32 MFMA (32x32x2), same walk
// fp32 LDS image of a (rows, HD) matrix, row pitch HD + 1 floats: a column read of 32 consecutive rows (the A operand of S = K Q^T)
// and a row read of 32 consecutive columns (the A operand of the P.V-shaped products) are both conflict-free
template <int HD> struct FImg {
    static constexpr int PITCH = HD + 1;
    static __device__ __forceinline__ void stage(float* img, const float* src, size_t row_stride, int T, int rows, int tid, int nthreads) {
        constexpr int CH = HD / 4;
        for (int c = tid; c < rows * CH; c += nthreads) {
            const int r = c / CH, ch = c - r * CH;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < T) v = *reinterpret_cast<const float4*>(src + (size_t)r * row_stride + ch * 4);
            float* d = img + r * PITCH + ch * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
};

// S-shaped product: acc[row crow(g, hh) of the staged tile][this lane's own row] += sum_d img[32 t + i][d] * own[d]; the lane holds
// own[2 s + hh] in f[s]
template <int HD> __device__ __forceinline__ f32x16 fdot(const float* img, int t, int r, int hh, const float (&f)[HD / 2], f32x16 acc) {
#pragma unroll
    for (int s = 0; s < HD / 2; ++s) acc = mfma_f32(img[(32 * t + r) * FImg<HD>::PITCH + 2 * s + hh], f[s], acc);
    return acc;
}
// PV-shaped product: acc[d = 32 dt + crow][own row] += sum over the tile's 32 rows j of img[32 t + j][d] * p[j][own row], the k index
// of step g being the tile rows crow(g, 0) and crow(g, 1) -- exactly the rows the lane halves hold in register g of p
template <int HD> __device__ __forceinline__ f32x16 facc(const float* img, int t, int r, int hh, int dt, const f32x16& p, f32x16 acc) {
    const int col = (32 * dt + r) & (HD - 1);             // HD = 16: lanes past the head dim read valid (ignored) data
#pragma unroll
    for (int g = 0; g < 16; ++g) acc = mfma_f32(img[(32 * t + crow(g, hh)) * FImg<HD>::PITCH + col], p[g], acc);
    return acc;
}
// own[2 s + hh] of the lane's own row straight from global memory; rows >= T: zeros
template <int HD> __device__ __forceinline__ void fown(float (&f)[HD / 2], const float* src, size_t row_stride, int row, bool ok, int hh) {
#pragma unroll
    for (int s = 0; s < HD / 2; ++s) f[s] = ok ? src[(size_t)row * row_stride + 2 * s + hh] : 0.f;
}
// rows d0 .. d0 + 3 of a transposed accumulator tile -> 4 consecutive floats of the lane's own row
template <int HD, int DT> __device__ __forceinline__ void fstore(float* dst, const f32x16 (&x)[DT], int hh, float mul) {
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d0 = 32 * d + 8 * g4 + 4 * hh;
            if (d0 < HD)
                *reinterpret_cast<float4*>(dst + d0) = make_float4(x[d][4 * g4] * mul, x[d][4 * g4 + 1] * mul, x[d][4 * g4 + 2] * mul,
                                                                    x[d][4 * g4 + 3] * mul);
        }
}

// grid (B*H, ceil(T / 256)), 512 threads; LDS = 2 * 2 * 64 * (HD + 1) * 4 bytes (17 / 33 / 65 KiB)
template <int HD>
__global__ __launch_bounds__(512) void lattn_fwd_f32_kernel(const float* __restrict__ qkv, const unsigned* __restrict__ mask,
                                                            float* __restrict__ out, float* __restrict__ lse, int T, int H, int W,
                                                            float scale) {
#pragma clang fp contract(off)                       // `s * scale - m` must not become one fma (see mattn_fwd_f32_kernel)
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    using I = FImg<HD>;
    constexpr int NWV = 8, NTH = 64 * NWV, DT = (HD + 31) / 32, IMG = LCH * I::PITCH;
    float* sm = reinterpret_cast<float*>(lsm);
    const int NK = (T + 31) >> 5, NC = (T + LCH - 1) / LCH;
    int bh_, yb_;
    mattn_block(bh_, yb_);
    const int b = bh_ / H, h = bh_ % H;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const size_t rs = (size_t)3 * H * HD, os = (size_t)H * HD;
    const float* Qg = qkv + (size_t)b * T * rs + (size_t)h * HD;
    const float* Kg = Qg + os;
    const float* Vg = Qg + 2 * os;
    I::stage(sm, Kg, rs, T, LCH, tid, NTH);
    I::stage(sm + IMG, Vg, rs, T, LCH, tid, NTH);
    __syncthreads();
    const int q = 32 * NWV * yb_ + 32 * w + r;      // this lane's query
    const bool active = q - r < T;                  // wave-uniform
    const bool q_ok = q < T;
    const unsigned* mrow = mask ? mask + ((size_t)b * T + (q_ok ? q : 0)) * W : nullptr;
    float fq[HD / 2];
    fown<HD>(fq, Qg, rs, q, q_ok, hh);
    float m = -INFINITY, l = 0.f;
    f32x16 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) o[d] = zero16();
    for (int c = 0; c < NC; ++c) {
        const float* Ki = sm + (c & 1) * 2 * IMG;
        const float* Vi = Ki + IMG;
        if (c + 1 < NC) {
            float* nb = sm + ((c + 1) & 1) * 2 * IMG;
            const int k1 = LCH * (c + 1);
            I::stage(nb, Kg + (size_t)k1 * rs, rs, T - k1, LCH, tid, NTH);
            I::stage(nb + IMG, Vg + (size_t)k1 * rs, rs, T - k1, LCH, tid, NTH);
        }
        if (active) {
#pragma unroll 1
            for (int t = 0; t < LCH / 32; ++t) {
                const int kt = (LCH / 32) * c + t;
                if (kt >= NK) break;
                const unsigned mw = mask_word(mrow, q_ok, kt, T);
                if (__ballot(mw != 0xffffffffu) == 0ull) continue;
                f32x16 st = fdot<HD>(Ki, t, r, hh, fq, zero16());
                float tm = -INFINITY;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    st[g] = ((mw >> crow(g, hh)) & 1u) ? -INFINITY : st[g] * scale;
                    tm = fmaxf(tm, st[g]);
                }
                tm = fmaxf(tm, __shfl_xor(tm, 32));
                const float mn = fmaxf(m, tm);
                const float alpha = mn == -INFINITY ? 1.f : expf(m - mn);
                float ts = 0.f;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    st[g] = mn == -INFINITY ? 0.f : expf(st[g] - mn);
                    ts += st[g];
                }
                ts += __shfl_xor(ts, 32);
                l = l * alpha + ts;
                m = mn;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
#pragma unroll
                    for (int g = 0; g < 16; ++g) o[d][g] *= alpha;
                    o[d] = facc<HD>(Vi, t, r, hh, d, st, o[d]);
                }
            }
        }
        __syncthreads();
    }
    if (active && q_ok) {
        fstore<HD, DT>(out + ((size_t)b * T + q) * os + (size_t)h * HD, o, hh, l > 0.f ? 1.0f / l : 0.f);
        if (hh == 0) lse[((size_t)b * H + h) * T + q] = l > 0.f ? m + logf(l) : 0.f;
    }
}

// grid (B*H, ceil(T / 128)), 512 threads: waves 0..3 own key tiles (dK, dV), waves 4..7 the query tiles of the same rows (dQ);
// LDS = 2 * (4 * 64 * (HD + 1) * 4 + 512) bytes (35 / 67 / 131 KiB)
template <int HD>
__global__ __launch_bounds__(512) void lattn_bwd_f32_kernel(const float* __restrict__ qkv, const unsigned* __restrict__ mask,
                                                            const float* __restrict__ out, const float* __restrict__ dout,
                                                            const float* __restrict__ lse, float* __restrict__ dqkv, int T, int H,
                                                            int W, float scale) {
#pragma clang fp contract(off)                       // the forward's logit s * scale, bit for bit
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    using I = FImg<HD>;
    constexpr int NTP = 4, NTH = 128 * NTP, DT = (HD + 31) / 32, IMG = LCH * I::PITCH, BUF = 4 * IMG + 2 * LCH;
    float* sm = reinterpret_cast<float*>(lsm);
    const int NT = (T + 31) >> 5, NC = (T + LCH - 1) / LCH;
    int bh_, yb_;
    mattn_block(bh_, yb_);
    const int b = bh_ / H, h = bh_ % H;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const size_t rs = (size_t)3 * H * HD, os = (size_t)H * HD;
    const float* Qg = qkv + (size_t)b * T * rs + (size_t)h * HD;
    const float* Og = out + (size_t)b * T * os + (size_t)h * HD;
    const float* Dg = dout + (size_t)b * T * os + (size_t)h * HD;
    const float* Lg = lse + ((size_t)b * H + h) * T;
    auto delta = [&](int i) {
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) acc = fmaf(Dg[(size_t)i * os + d], Og[(size_t)i * os + d], acc);
        return acc;
    };
    auto stage_chunk = [&](float* buf, int c) {
        const int r0 = LCH * c;
        I::stage(buf, Qg + (size_t)r0 * rs, rs, T - r0, LCH, tid, NTH);
        I::stage(buf + IMG, Qg + os + (size_t)r0 * rs, rs, T - r0, LCH, tid, NTH);
        I::stage(buf + 2 * IMG, Qg + 2 * os + (size_t)r0 * rs, rs, T - r0, LCH, tid, NTH);
        I::stage(buf + 3 * IMG, Dg + (size_t)r0 * os, os, T - r0, LCH, tid, NTH);
        if (tid < LCH) {
            const int i = r0 + tid;
            buf[4 * IMG + tid] = i < T ? Lg[i] : 0.f;
            buf[4 * IMG + LCH + tid] = i < T ? delta(i) : 0.f;
        }
    };
    stage_chunk(sm, 0);
    __syncthreads();
    const bool keyw = w < NTP;
    const int tile = NTP * yb_ + (keyw ? w : w - NTP);
    const bool active = 32 * tile < T;              // wave-uniform
    const int row = 32 * tile + r;                  // this lane's key (waves 0..3) or query (waves 4..7)
    const bool row_ok = row < T;
    const unsigned* mrow = mask ? mask + ((size_t)b * T + (row_ok ? row : 0)) * W : nullptr;
    f32x16 x[DT], y[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) { x[d] = zero16(); y[d] = zero16(); }
    float fa[HD / 2], fb[HD / 2];                   // K and V of the lane's key, or Q and dO of the lane's query
    fown<HD>(fa, keyw ? Qg + os : Qg, rs, row, row_ok, hh);
    fown<HD>(fb, keyw ? Qg + 2 * os : Dg, keyw ? rs : os, row, row_ok, hh);
    float lq = 0.f, dq_ = 0.f;
    if (!keyw && row_ok) { lq = Lg[row]; dq_ = delta(row); }
    for (int c = 0; c < NC; ++c) {
        const float* Qi = sm + (c & 1) * BUF;
        const float* Ki = Qi + IMG;
        const float* Vi = Ki + IMG;
        const float* Di = Vi + IMG;
        const float* Ls = Di + IMG;
        const float* Del = Ls + LCH;
        if (c + 1 < NC) stage_chunk(sm + ((c + 1) & 1) * BUF, c + 1);
        if (active) {
#pragma unroll 1
            for (int t = 0; t < LCH / 32; ++t) {
                const int ot = (LCH / 32) * c + t;      // the other side's tile: queries for a key wave, keys for a query wave
                if (ot >= NT) break;
                const unsigned mw = mask_word(mrow, row_ok, ot, T);      // symmetric mask: row `key`, word qt, for the key waves
                if (__ballot(mw != 0xffffffffu) == 0ull) continue;
                f32x16 s = fdot<HD>(keyw ? Qi : Ki, t, r, hh, fa, zero16());
                f32x16 dp = fdot<HD>(keyw ? Di : Vi, t, r, hh, fb, zero16());
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int ol = 32 * t + crow(g, hh);
                    const float p = ((mw >> crow(g, hh)) & 1u) ? 0.f : expf(s[g] * scale - (keyw ? Ls[ol] : lq));
                    s[g] = p;
                    dp[g] = p * (dp[g] - (keyw ? Del[ol] : dq_)) * scale;
                }
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    if (keyw) {
                        x[d] = facc<HD>(Di, t, r, hh, d, s, x[d]);       // dV^T[d][key]
                        y[d] = facc<HD>(Qi, t, r, hh, d, dp, y[d]);      // dK^T[d][key]
                    } else {
                        x[d] = facc<HD>(Ki, t, r, hh, d, dp, x[d]);      // dQ^T[d][q]
                    }
                }
            }
        }
        __syncthreads();
    }
    if (active && row_ok) {
        float* g = dqkv + (size_t)b * T * rs + (size_t)h * HD + (size_t)row * rs;
        fstore<HD, DT>(g + (keyw ? 2 * os : 0), x, hh, 1.0f);               // dV (key waves) / dQ (query waves)
        if (keyw) fstore<HD, DT>(g + os, y, hh, 1.0f);                      // dK
    }
}

static int lattn_check(const void* a, const void* b, int B, int T, int H, int HDv, int dtype) {
    if (!a || !b || B < 0 || T < 1 || H < 1) return GM3D_EINVAL;
    if (HDv != 16 && HDv != 32 && HDv != 64) return GM3D_EUNSUPPORTED;
    if (T <= 512 || T > 2048) return GM3D_EUNSUPPORTED;       // T <= 512: gm3d_attention_masked_* (one owner per range)
    if (dtype != GM3D_F32 && dtype != GM3D_BF16) return GM3D_EINVAL;
    if ((long long)B * H > 0x7fffffffLL / 4) return GM3D_EUNSUPPORTED;
    return GM3D_OK;
}

}  // namespace gm3d

extern "C" int gm3d_attention_long_fwd(const void* qkv, const unsigned* mask, void* out, float* lse, int B, int T, int H, int HD,
                                       float scale, int dtype, gm3d_stream_t stream) {
    using namespace gm3d;
    int rc = lattn_check(qkv, out, B, T, H, HD, dtype);
    if (rc != GM3D_OK) return rc;
    if (!lse) return GM3D_EINVAL;
    if (B == 0) return GM3D_OK;
    const int W = (T + 31) / 32;
    if (dtype == GM3D_F32) {
        const size_t lds = (size_t)4 * LCH * (HD + 1) * sizeof(float);
        const dim3 grid(B * H, (T + 255) / 256);
        return by_int<16, 32, 64>(HD, [&](auto c) {
            return launch_lds<lattn_fwd_f32_kernel<decltype(c)::value>>(grid, dim3(512), lds, stream, (const float*)qkv, mask, (float*)out,
                                                                        lse, T, H, W, scale);
        });
    }
    const size_t lds = (size_t)(4 * LCH + 256) * (HD * 2 + 16);
    const dim3 grid(B * H, (T + 255) / 256);
    return by_int<16, 32, 64>(HD, [&](auto c) {
        return launch_lds<lattn_fwd_bf16_kernel<decltype(c)::value>>(grid, dim3(512), lds, stream, (const bf16_t*)qkv, mask, (bf16_t*)out,
                                                                     lse, T, H, W, scale);
    });
}

extern "C" int gm3d_attention_long_bwd(const void* qkv, const unsigned* mask, const void* out, const void* dout, const float* lse,
                                       void* dqkv, int B, int T, int H, int HD, float scale, int dtype, gm3d_stream_t stream) {
    using namespace gm3d;
    int rc = lattn_check(qkv, out, B, T, H, HD, dtype);
    if (rc != GM3D_OK) return rc;
    if (!dout || !lse || !dqkv) return GM3D_EINVAL;
    if (B == 0) return GM3D_OK;
    const int W = (T + 31) / 32;
    if (dtype == GM3D_F32) {
        const size_t lds = (size_t)2 * (4 * LCH * (HD + 1) + 2 * LCH) * sizeof(float);
        const dim3 grid(B * H, (T + 127) / 128);
        return by_int<16, 32, 64>(HD, [&](auto c) {
            return launch_lds<lattn_bwd_f32_kernel<decltype(c)::value>>(grid, dim3(512), lds, stream, (const float*)qkv, mask,
                                                                        (const float*)out, (const float*)dout, lse, (float*)dqkv, T, H, W,
                                                                        scale);
        });
    }
    const size_t lds = (size_t)2 * (4 * LCH * (HD * 2 + 16) + 2 * LCH * sizeof(float));
    const dim3 grid(B * H, (T + 127) / 128);       // 4 key tiles (= query tiles) per workgroup
    return by_int<16, 32, 64>(HD, [&](auto c) {
        return launch_lds<lattn_bwd_bf16_kernel<decltype(c)::value>>(grid, dim3(512), lds, stream, (const bf16_t*)qkv, mask,
                                                                     (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv, T, H, W,
                                                                     scale);
    });
}
