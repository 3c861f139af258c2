// Linear probe of pretrained features (Point-MAE_SA3D/main_linprob.py:219-263): BatchNorm1d(affine=False, eps=1e-6) -> Linear,
// cross-entropy, SGD with momentum, trained on cached features with one launch per iteration.
//
// Beneath: index_select, batch_norm, addmm, log_softmax, nll_loss, their backward kernels and two optimizer passes, some two dozen
// launch-bound kernels for a 512 x 384 x 40 product, 1,710 times in a row.  Here launch K(t) of a grid of P = ceil(d / 16) column
// slices does, in workgroup p (columns 16p .. 16p + 15):
//   (a) the end of iteration t-1: every workgroup sums the P partial-logit tiles of t-1 in the order p = 0..P-1, then the bias
//       (redundantly: batch x C values), takes the max-subtracted softmax and dz, the weight gradient of its own columns from dz and
//       its own x^ slice (kept in memory by (b) of the launch before), and updates the momentum and the weights of its slice;
//       workgroup 0 also does db, the bias (read from slot (t-1) & 1, written to slot t & 1: the others still read the old one) and
//       the loss;
//   (b) the start of iteration t: it gathers its columns of the batch rows, takes the two-pass statistics of its columns, updates
//       their running statistics, normalises, and writes its partial logits x^_slice . W_slice^T with the weights just updated into
//       tile (t & 1, p) of two alternating partial buffers.
// The first launch of a range runs (b) only, the last (a) only: n iterations are n + 1 launches.  The only dependency between
// workgroups sits on a launch boundary: no workgroup waits for another, no cooperative launch, no float atomics.
//
// Orders (fixed by the shapes alone; two fits on the same inputs are equal bit for bit):
//   column sums (mean, variance)   thread (j, g) adds rows g, g + 32, ... in order; the 32 group sums are added g = 0..31
//   partial logit                  one fmaf per column onto the running sum, columns ascending, from 0
//   logit                          ((tile 0 + tile 1) + ... + tile P-1) + bias
//   softmax                        max, then the sum of expf(z - max) over the classes ascending; p = e * (1 / sum),
//                                  dz = (p - onehot) * (1 / batch)
//   dW[c][j]                       the batch in chunks of 256 rows; row group g = 0..7 of a chunk owns its rows 32g .. 32g + 31 and
//                                  adds one fmaf per row, chunks then rows ascending; the eight group sums are added g = 0..7
//   db[c]                          per chunk the same eight row groups, added g = 0..7 onto the running sum, chunks ascending
//   loss                           thread r adds the rows r, r + 256, ...; a fixed butterfly per wave; the four wave sums in order
//   evaluation logit               one fmaf per column onto the running sum, columns ascending, from 0, then + bias
//
// Training launch: 512 threads, LDS all dynamic, 94,720 bytes: W slice 64 x 16, db partials 8 x 64, column partials 32 x 16, 64 words
// of statistics and wave sums, then one region that holds in (a) the logits / dz of a chunk 64 x 257 and its x^ rows 256 x 20 (the
// eight dW partials 8 x 64 x 16 reuse the logits), in (b) the batch slice 1024 x 17.  One workgroup per CU; P <= 64 workgroups.
// Evaluation launch: 256 threads own 64 test rows, 64 columns at a time, 33,024 bytes of static LDS.
// Compiled with -ffp-contract=off: every product and sum written here is rounded once, the dot products are explicit fmaf chains.
#include "common.hpp"

using namespace gm3d;

namespace {

constexpr int LP_MAX_N = 16384, LP_MAX_D = 1024, LP_MAX_CLS = 64, LP_MAX_BATCH = 1024;
constexpr int LP_SLICE = 16, LP_THREADS = 512, LP_CHUNK = 256, LP_GROUPS = 8, LP_GROUP_ROWS = LP_CHUNK / LP_GROUPS;
constexpr int LP_ZP = LP_CHUNK + 1;                            // logits: [class][row of the chunk], odd pitch
constexpr int LP_XP = LP_SLICE + 1;                            // batch slice: [row][column], odd pitch
constexpr int LP_XCP = LP_SLICE + 4;                           // x^ rows of a chunk: 16-byte rows off the bank period
constexpr int LP_STAT_ROWS = LP_THREADS / LP_SLICE;            // 32 row groups of the column sums
constexpr int LP_GATHER = LP_MAX_BATCH * (LP_SLICE / 4) / LP_THREADS;      // float4 loads per thread of the batch slice: 8
constexpr float LP_EPS = 1e-6f, LP_BN_MOMENTUM = 0.1f;
// LDS carve, in floats; every offset is a multiple of 4 (16 bytes)
constexpr int LP_OFF_W = 0;
constexpr int LP_OFF_DBP = LP_OFF_W + LP_MAX_CLS * LP_SLICE;
constexpr int LP_OFF_RED = LP_OFF_DBP + LP_GROUPS * LP_MAX_CLS;
constexpr int LP_OFF_STAT = LP_OFF_RED + LP_STAT_ROWS * LP_SLICE;
constexpr int LP_OFF_A = LP_OFF_STAT + 64;
constexpr int LP_Z_WORDS = LP_MAX_CLS * LP_ZP;                 // 16448
constexpr int LP_A_WORDS_A = LP_Z_WORDS + LP_CHUNK * LP_XCP;   // 21568
constexpr int LP_A_WORDS_B = LP_MAX_BATCH * LP_XP;             // 17408
constexpr int LP_A_WORDS = LP_A_WORDS_A > LP_A_WORDS_B ? LP_A_WORDS_A : LP_A_WORDS_B;
constexpr size_t LP_LDS = (size_t)(LP_OFF_A + LP_A_WORDS) * sizeof(float);
static_assert(LP_LDS == 94720, "the LDS budget stated in the header comment and include/gm3d.h");
static_assert(LP_OFF_A % 4 == 0 && LP_Z_WORDS % 4 == 0 && LP_XCP % 4 == 0, "16-byte LDS carve");
static_assert(LP_GROUPS * LP_MAX_CLS * LP_SLICE <= LP_Z_WORDS, "the dW partials reuse the logits");
static_assert(LP_GROUPS * 64 == LP_THREADS && LP_MAX_CLS * LP_SLICE == 2 * LP_THREADS, "thread maps");

constexpr int LE_ROWS = 64, LE_THREADS = 256, LE_KC = 64, LE_QP = LE_KC + 1, LE_CLS_PER_THREAD = LP_MAX_CLS / (LE_THREADS / 64);

__device__ __forceinline__ int clampi(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

__global__ __launch_bounds__(LP_THREADS) void linprobe_train_kernel(
    const float* __restrict__ X, const long long* __restrict__ y, int n, int d, int C, int batch, const int* __restrict__ order,
    const float* __restrict__ lr, int t, int do_a, int do_b, float momentum, float* __restrict__ W, float* __restrict__ mom_w,
    float* __restrict__ bias2, float* __restrict__ mom_b, float* __restrict__ rmean, float* __restrict__ rvar,
    float* __restrict__ xhat, float* __restrict__ part, float* __restrict__ losses) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ws = lds + LP_OFF_W;                                // [C][16] the weights of the slice, zero beyond its width
    float* dbp = lds + LP_OFF_DBP;                             // [8][64]
    float* red = lds + LP_OFF_RED;                             // [32][16]
    float* mean = lds + LP_OFF_STAT;                           // [16]
    float* sdev = mean + LP_SLICE;                             // [16]
    float* wred = sdev + LP_SLICE;                             // [4] the loss sums of waves 0..3
    float* A = lds + LP_OFF_A;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x, P = gridDim.x, c0 = p * LP_SLICE;
    const int w = d - c0 < LP_SLICE ? d - c0 : LP_SLICE;       // 16, or 8 in the last slice of a d that is no multiple of 16
    const size_t tile = (size_t)C * batch;                     // one partial tile: [class][row]

    // the batch rows of iteration t are fetched first and held in registers: (a) does not depend on them and hides their latency
    float4 gx[LP_GATHER];
#pragma unroll
    for (int u = 0; u < LP_GATHER; ++u) gx[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    float rm_old = 0.f, rv_old = 0.f;
    if (do_b) {
        const int* rows = order + (size_t)t * batch;
#pragma unroll
        for (int u = 0; u < LP_GATHER; ++u) {
            const int e = u * LP_THREADS + tid, i = e >> 2, q = e & 3;
            if (e < batch * 4 && 4 * q < w) gx[u] = *reinterpret_cast<const float4*>(X + (size_t)clampi(rows[i], n - 1) * d + c0 + 4 * q);
        }
        if (tid < w) {
            rm_old = rmean[c0 + tid];
            rv_old = rvar[c0 + tid];
        }
    }

    if (do_a) {
        // ================= (a) finish iteration t - 1 =================
        float* zs = A;                                         // [C][257] logits, then exp, then dz of the chunk
        float* xc = A + LP_Z_WORDS;                            // [256][20] x^ rows of the chunk, own columns
        float* dwp = A;                                        // [8][64][16] after the last chunk
        const int tp = t - 1;
        const float* pt = part + (size_t)(tp & 1) * P * tile;
        const float* bias_in = bias2 + (tp & 1) * C;
        const int* rows = order + (size_t)tp * batch;
        const float inv_batch = 1.0f / (float)batch, rate = lr[tp];
        const int cb = lane >> 2, jb = lane & 3;               // the dW tile of the lane: classes 4cb .. + 3, columns 4jb .. + 3
        float acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
        float dbacc = 0.f, lacc = 0.f;

        for (int r0 = 0; r0 < batch; r0 += LP_CHUNK) {
            const int rc = batch - r0 < LP_CHUNK ? batch - r0 : LP_CHUNK;
            // -- 1: logits of the chunk (eight elements per thread at a time, so that many loads are in flight), x^ rows of the chunk
            const int lab = tid < rc ? clampi(y[clampi(rows[r0 + tid], n - 1)], C - 1) : 0;
            const int cnt = rc * C;
            for (int e0 = 0; e0 < cnt; e0 += 8 * LP_THREADS) {
                float z[8];
                int off[8], zo[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int e = e0 + k * LP_THREADS + tid, ee = e < cnt ? e : 0;     // beyond the chunk: element 0 again, not stored
                    const int c = ee / rc, il = ee - c * rc;
                    off[k] = c * batch + r0 + il;
                    zo[k] = e < cnt ? c * LP_ZP + il : -1;
                    z[k] = pt[off[k]];
                }
#pragma unroll 4
                for (int s = 1; s < P; ++s) {
                    const float* ps = pt + (size_t)s * tile;
#pragma unroll
                    for (int k = 0; k < 8; ++k) z[k] = z[k] + ps[off[k]];
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (zo[k] >= 0) zs[zo[k]] = z[k] + bias_in[zo[k] / LP_ZP];
            }
            for (int e = tid; e < rc * 4; e += LP_THREADS) {
                const int il = e >> 2, q = e & 3;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (4 * q < w) v = *reinterpret_cast<const float4*>(xhat + (size_t)(r0 + il) * d + c0 + 4 * q);
                *reinterpret_cast<float4*>(xc + il * LP_XCP + 4 * q) = v;
            }
            __syncthreads();
            // -- 2: softmax and dz, one row per thread
            if (tid < rc) {
                float* zr = zs + tid;
                float m = zr[0];
                for (int c = 1; c < C; ++c) m = fmaxf(m, zr[c * LP_ZP]);
                const float zy = zr[lab * LP_ZP];
                float s = 0.f;
                for (int c = 0; c < C; ++c) {
                    const float ex = expf(zr[c * LP_ZP] - m);
                    zr[c * LP_ZP] = ex;
                    s = s + ex;
                }
                const float rs = 1.0f / s;
                for (int c = 0; c < C; ++c) zr[c * LP_ZP] = (zr[c * LP_ZP] * rs - (c == lab ? 1.0f : 0.0f)) * inv_batch;
                lacc = lacc + ((logf(s) + m) - zy);
            }
            __syncthreads();
            // -- 3: dW of the slice (row group = wave), db partials (workgroup 0)
            {
                const int i0 = wave * LP_GROUP_ROWS, i1 = i0 + LP_GROUP_ROWS < rc ? i0 + LP_GROUP_ROWS : rc;
                if (4 * cb < C) {
                    for (int il = i0; il < i1; ++il) {
                        const float4 xv = *reinterpret_cast<const float4*>(xc + il * LP_XCP + 4 * jb);
                        const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const float g = 4 * cb + u < C ? zs[(4 * cb + u) * LP_ZP + il] : 0.f;
#pragma unroll
                            for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(g, x4[v], acc[u][v]);
                        }
                    }
                }
                if (p == 0 && lane < C) {
                    float s = 0.f;
                    for (int il = i0; il < i1; ++il) s = s + zs[lane * LP_ZP + il];
                    dbp[wave * LP_MAX_CLS + lane] = s;
                }
            }
            __syncthreads();
            // -- 4: db of the chunk onto the running sum
            if (p == 0 && tid < C) {
                for (int g = 0; g < LP_GROUPS; ++g) dbacc = dbacc + dbp[g * LP_MAX_CLS + tid];
            }
        }
        // -- the eight dW partials, the loss sums of the waves
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (4 * cb + u < C) dwp[(wave * LP_MAX_CLS + 4 * cb + u) * LP_SLICE + 4 * jb + v] = acc[u][v];
        if (p == 0 && tid < LP_CHUNK) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) lacc = lacc + __shfl_xor(lacc, off, 64);
            if (lane == 0) wred[wave] = lacc;
        }
        __syncthreads();
        // -- momentum and weights of the slice; bias and loss
        for (int o = tid; o < C * LP_SLICE; o += LP_THREADS) {
            const int c = o >> 4, j = o & 15;
            float wn = 0.f;
            if (j < w) {
                float g = dwp[c * LP_SLICE + j];
                for (int s = 1; s < LP_GROUPS; ++s) g = g + dwp[(s * LP_MAX_CLS + c) * LP_SLICE + j];
                const size_t at = (size_t)c * d + c0 + j;
                const float mu = momentum * mom_w[at] + g;
                mom_w[at] = mu;
                wn = W[at] - rate * mu;
                W[at] = wn;
            }
            ws[o] = wn;
        }
        if (p == 0 && tid < C) {
            const float mu = momentum * mom_b[tid] + dbacc;
            mom_b[tid] = mu;
            bias2[(t & 1) * C + tid] = bias_in[tid] - rate * mu;
        }
        if (p == 0 && tid == 0) losses[tp] = (((wred[0] + wred[1]) + wred[2]) + wred[3]) * inv_batch;
        __syncthreads();
    } else {
        for (int o = tid; o < C * LP_SLICE; o += LP_THREADS) {
            const int c = o >> 4, j = o & 15;
            ws[o] = j < w ? W[(size_t)c * d + c0 + j] : 0.f;
        }
    }
    if (!do_b) return;

    // ================= (b) start iteration t =================
    float* xs = A;                                             // [batch][17]
#pragma unroll
    for (int u = 0; u < LP_GATHER; ++u) {
        const int e = u * LP_THREADS + tid, i = e >> 2, q = e & 3;
        if (e < batch * 4) {
            float* dst = xs + i * LP_XP + 4 * q;
            dst[0] = gx[u].x;
            dst[1] = gx[u].y;
            dst[2] = gx[u].z;
            dst[3] = gx[u].w;
        }
    }
    __syncthreads();
    const int sj = tid & 15, sg = tid >> 4;
    {
        float s = 0.f;
        for (int i = sg; i < batch; i += LP_STAT_ROWS) s = s + xs[i * LP_XP + sj];
        red[sg * LP_SLICE + sj] = s;
    }
    __syncthreads();
    if (tid < LP_SLICE) {
        float s = 0.f;
        for (int g = 0; g < LP_STAT_ROWS; ++g) s = s + red[g * LP_SLICE + tid];
        mean[tid] = s / (float)batch;
    }
    __syncthreads();
    {
        const float mu = mean[sj];
        float s = 0.f;
        for (int i = sg; i < batch; i += LP_STAT_ROWS) {
            const float dl = xs[i * LP_XP + sj] - mu;
            s = s + dl * dl;
        }
        red[sg * LP_SLICE + sj] = s;
    }
    __syncthreads();
    if (tid < LP_SLICE) {
        float s = 0.f;
        for (int g = 0; g < LP_STAT_ROWS; ++g) s = s + red[g * LP_SLICE + tid];
        const float var = s / (float)batch;
        sdev[tid] = sqrtf(var + LP_EPS);
        if (tid < w) {
            const float unbiased = var * (float)batch / (float)(batch - 1);
            rmean[c0 + tid] = (1.0f - LP_BN_MOMENTUM) * rm_old + LP_BN_MOMENTUM * mean[tid];
            rvar[c0 + tid] = (1.0f - LP_BN_MOMENTUM) * rv_old + LP_BN_MOMENTUM * unbiased;
        }
    }
    __syncthreads();
    for (int e = tid; e < batch * LP_SLICE; e += LP_THREADS) {
        const int i = e >> 4, j = e & 15;
        const float v = (xs[i * LP_XP + j] - mean[j]) / sdev[j];
        xs[i * LP_XP + j] = v;
        if (j < w) xhat[(size_t)i * d + c0 + j] = v;
    }
    __syncthreads();
    float* po = part + ((size_t)(t & 1) * P + p) * tile;
    for (int i = tid; i < batch; i += LP_THREADS) {
        float xr[LP_SLICE];
#pragma unroll
        for (int j = 0; j < LP_SLICE; ++j) xr[j] = xs[i * LP_XP + j];
        for (int c = 0; c < C; ++c) {
            float a = 0.f;
#pragma unroll
            for (int q = 0; q < LP_SLICE / 4; ++q) {
                const float4 wv = *reinterpret_cast<const float4*>(ws + c * LP_SLICE + 4 * q);
                a = fmaf(xr[4 * q + 0], wv.x, a);
                a = fmaf(xr[4 * q + 1], wv.y, a);
                a = fmaf(xr[4 * q + 2], wv.z, a);
                a = fmaf(xr[4 * q + 3], wv.w, a);
            }
            po[(size_t)c * batch + i] = a;
        }
    }
}

// 64 test rows per workgroup; thread (row = tid & 63, cg = tid >> 6) owns the classes cg, cg + 4, ...
__global__ __launch_bounds__(LE_THREADS) void linprobe_eval_kernel(const float* __restrict__ Q, const long long* __restrict__ yq, int m,
                                                                   int d, int C, const float* __restrict__ W,
                                                                   const float* __restrict__ bias, const float* __restrict__ rmean,
                                                                   const float* __restrict__ rvar, float* __restrict__ logits,
                                                                   long long* __restrict__ pred,
                                                                   unsigned long long* __restrict__ correct) {
    __shared__ __attribute__((aligned(16))) float wsm[LP_MAX_CLS * LE_KC];     // [class][64 columns]
    __shared__ __attribute__((aligned(16))) float qs[LE_ROWS * LE_QP];         // [row][64 columns], later the logits [row][class]
    const int tid = threadIdx.x, row = tid & 63, cg = tid >> 6, r0 = blockIdx.x * LE_ROWS;
    float acc[LE_CLS_PER_THREAD];
#pragma unroll
    for (int ci = 0; ci < LE_CLS_PER_THREAD; ++ci) acc[ci] = 0.f;

    for (int k0 = 0; k0 < d; k0 += LE_KC) {
        for (int e = tid; e < C * LE_KC; e += LE_THREADS) {
            const int c = e >> 6, k = e & 63;
            wsm[e] = k0 + k < d ? W[(size_t)c * d + k0 + k] : 0.f;
        }
        {
            const int k = tid & 63;                                // the column of this thread in every pass below
            const bool in = k0 + k < d;
            const float cm = in ? rmean[k0 + k] : 0.f, cs = in ? sqrtf(rvar[k0 + k] + LP_EPS) : 1.f;
#pragma unroll
            for (int u = 0; u < LE_ROWS * LE_KC / LE_THREADS; ++u) {
                const int r = u * (LE_THREADS / LE_KC) + (tid >> 6);
                float v = 0.f;
                if (r0 + r < m && in) v = (Q[(size_t)(r0 + r) * d + k0 + k] - cm) / cs;
                qs[r * LE_QP + k] = v;
            }
        }
        __syncthreads();
        for (int k4 = 0; k4 < LE_KC / 4; ++k4) {
            const float x0 = qs[row * LE_QP + 4 * k4], x1 = qs[row * LE_QP + 4 * k4 + 1], x2 = qs[row * LE_QP + 4 * k4 + 2],
                        x3 = qs[row * LE_QP + 4 * k4 + 3];
#pragma unroll
            for (int ci = 0; ci < LE_CLS_PER_THREAD; ++ci) {
                const int c = cg + 4 * ci;
                if (c < C) {                                       // wave-uniform
                    const float4 wv = *reinterpret_cast<const float4*>(wsm + c * LE_KC + 4 * k4);
                    float a = acc[ci];
                    a = fmaf(x0, wv.x, a);
                    a = fmaf(x1, wv.y, a);
                    a = fmaf(x2, wv.z, a);
                    a = fmaf(x3, wv.w, a);
                    acc[ci] = a;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int ci = 0; ci < LE_CLS_PER_THREAD; ++ci) {
        const int c = cg + 4 * ci;
        if (c < C) qs[row * LE_QP + c] = acc[ci] + bias[c];
    }
    __syncthreads();
    if (logits) {
        for (int e = tid; e < LE_ROWS * C; e += LE_THREADS) {
            const int r = e / C, c = e - r * C;
            if (r0 + r < m) logits[(size_t)(r0 + r) * C + c] = qs[r * LE_QP + c];
        }
    }
    // classes ranked by (logit descending, class ascending): the first min(5, C)
    bool hit1 = false, hit5 = false;
    if (tid < LE_ROWS && r0 + tid < m) {
        const float* z = qs + tid * LE_QP;
        const long long tgt = yq ? yq[r0 + tid] : -1;
        const int lim = C < 5 ? C : 5;
        unsigned long long taken = 0ull;
        for (int r = 0; r < lim; ++r) {
            int best = -1;
            unsigned int bk = 0u;
            for (int c = 0; c < C; ++c) {
                if ((taken >> c) & 1ull) continue;
                const unsigned int kc = ordered_key(z[c]);
                if (best < 0 || kc > bk) {
                    best = c;
                    bk = kc;
                }
            }
            taken |= 1ull << best;
            if (r == 0 && pred) pred[r0 + tid] = best;
            if (yq && (long long)best == tgt) {
                hit1 = hit1 || r == 0;
                hit5 = true;
            }
        }
    }
    if (yq && tid < 64) {
        const unsigned long long b1 = __ballot(hit1), b5 = __ballot(hit5);
        if (tid == 0) {
            atomicAdd(correct, (unsigned long long)__popcll(b1));
            atomicAdd(correct + 1, (unsigned long long)__popcll(b5));
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int check_shape(int rows, int d, int ncls) {
    if (rows < 0 || d < 1 || ncls < 1) return GM3D_EINVAL;
    if (d > LP_MAX_D || d < 8 || d % 8 != 0 || ncls < 2 || ncls > LP_MAX_CLS) return GM3D_EUNSUPPORTED;
    return GM3D_OK;
}

}  // namespace

extern "C" int gm3d_linprobe_slices(int d) { return d < 1 ? 0 : (d + LP_SLICE - 1) / LP_SLICE; }

extern "C" int gm3d_linprobe_train(const float* X, const long long* y, int n, int d, int ncls, int batch, const int* order,
                                   const float* lr, int t_begin, int t_end, float momentum, float* W, float* mom_w, float* bias2,
                                   float* mom_b, float* running_mean, float* running_var, float* xhat, float* part, float* losses,
                                   gm3d_stream_t stream) {
    if (n < 1 || batch < 2 || batch > n || t_begin < 0 || t_end < t_begin || !(momentum >= 0.f && momentum < 1.f)) return GM3D_EINVAL;
    const int rc = check_shape(n, d, ncls);
    if (rc != GM3D_OK) return rc;
    if (n > LP_MAX_N || batch > LP_MAX_BATCH) return GM3D_EUNSUPPORTED;
    if (!X || !y || !order || !lr || !W || !mom_w || !bias2 || !mom_b || !running_mean || !running_var || !xhat || !part || !losses)
        return GM3D_EINVAL;
    if (!aligned16(X) || !aligned16(xhat)) return GM3D_EINVAL;
    if (t_end == t_begin) return GM3D_OK;
    const int P = gm3d_linprobe_slices(d);
    for (int t = t_begin; t <= t_end; ++t) {
        const int st = launch_lds<linprobe_train_kernel>(dim3(P), dim3(LP_THREADS), LP_LDS, stream, X, y, n, d, ncls, batch, order, lr, t,
                                                         t > t_begin ? 1 : 0, t < t_end ? 1 : 0, momentum, W, mom_w, bias2, mom_b,
                                                         running_mean, running_var, xhat, part, losses);
        if (st != GM3D_OK) return st;
    }
    return GM3D_OK;
}

extern "C" int gm3d_linprobe_eval(const float* Q, const long long* yq, int m, int d, int ncls, const float* W, const float* bias,
                                  const float* running_mean, const float* running_var, float* logits, long long* pred,
                                  long long* correct, gm3d_stream_t stream) {
    const int rc = check_shape(m, d, ncls);
    if (rc != GM3D_OK || m == 0) return rc;
    if (!Q || !W || !bias || !running_mean || !running_var || (yq && !correct)) return GM3D_EINVAL;
    return launch_lds<linprobe_eval_kernel>(dim3((m + LE_ROWS - 1) / LE_ROWS), dim3(LE_THREADS), 0, stream, Q, yq, m, d, ncls, W, bias,
                                            running_mean, running_var, logits, pred, reinterpret_cast<unsigned long long*>(correct));
}
