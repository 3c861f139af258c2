// Temperature-weighted k-NN probe of pretrained features (Point-MAE_SA3D/main_knn.py:153-198, knn_classifier) in one launch.
//
// Beneath: mm -> topk -> gather / scatter_ -> sort, 500 chunks with two host reads each, an (m,n) similarity matrix and an
// (m*k,C) one-hot in memory, and an unspecified order of ties.  Here one workgroup owns 32 test rows and never stores a similarity:
// it recomputes its 32 x n similarities five times on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) -- four passes of an 8-bit radix
// select over the order-preserving integer keys (a 256-bin histogram per row in LDS, integer atomics only), which leave the key of
// the k-th neighbour of every row and the number of entries at that key still to take, and one pass that keeps every key above it
// plus the first ties at it in ascending training index.  The <= 256 survivors of a row are rank-sorted in LDS by the strict total
// order (key descending, index ascending).  The order of the LDS atomics moves survivors between slots before the sort and nothing
// after it: every output is a pure function of the inputs.
//
// K order of a similarity (fixed, the same in every pass): the columns are taken 16 at a time; MFMA step j = 0..7 of a unit u adds
// column 16u + j and then column 16u + 8 + j, each as one fmaf onto the running sum.  Operands whose products and partial sums are
// exactly representable give exact results.
//
// Launch: 512 threads (8 waves, two per SIMD), one wave per 32 x 32 tile, operands straight from global memory (each lane reads
// 32 contiguous bytes of its row per unit).  LDS: 2 x 32 x 257 x 4 (survivor keys and indices) + 32 x 257 x 4 (histogram, later the
// class scores) = 98,688 bytes dynamic + 1.5 KiB static: one workgroup per CU.  See include/gm3d.h for the contracts.
// Compiled with -ffp-contract=off (the row norms, sim / T and the score sums are the operations written here, one rounding each).
#include "common.hpp"
#include "mfma.hpp"

using namespace gm3d;

namespace {

constexpr int KP_MAX_N = 16384, KP_MAX_D = 1024, KP_MAX_K = 256, KP_MAX_CLS = 64;
constexpr int KP_ROWS = 32, KP_THREADS = 512, KP_WAVES = KP_THREADS / 64;
constexpr int KP_PITCH = KP_MAX_K + 1;                        // survivor / histogram row pitch in words (odd: no bank pile-up)
constexpr int KP_SCORE_PITCH = KP_MAX_CLS + 1;
constexpr int KP_PER_THREAD = KP_ROWS * KP_MAX_K / KP_THREADS;   // survivors a thread ranks: 16
constexpr size_t KP_LDS = (size_t)3 * KP_ROWS * KP_PITCH * sizeof(unsigned int);
constexpr int NORM_THREADS = 256, NORM_ROWS = NORM_THREADS / 64;

// float -> uint32 whose unsigned order is the float order (-0 == +0, NaN above +inf), as mask.hip's ordered_key
__device__ __forceinline__ unsigned int sim_key(float v) {
    if (v == 0.f) v = 0.f;
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_sim(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// 32 x 32 similarities of the lane's test row `arow` and training row `brow` (both d floats): C column = lane & 31 (training row),
// C row = crow(reg, lane >> 5) (test row).  Lane half h reads columns 16u + 8h .. + 7 of unit u (zeros beyond d, d % 8 == 0).
__device__ __forceinline__ f32x16 sim_tile(const float* __restrict__ arow, const float* __restrict__ brow, int d, int h) {
    f32x16 acc = zero16();
    const int units = (d + 15) >> 4;
    float a[8], b[8], na[8], nb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.f;
    if (8 * h < d) {                                           // d == 8: the upper lane half has no columns
        V8<float>::load(arow + 8 * h, a);
        V8<float>::load(brow + 8 * h, b);
    }
    for (int u = 0; u < units; ++u) {
        const int kn = 16 * (u + 1) + 8 * h;                   // the next unit's operands load under this unit's MFMAs
#pragma unroll
        for (int j = 0; j < 8; ++j) na[j] = nb[j] = 0.f;
        if (kn < d) {
            V8<float>::load(arow + kn, na);
            V8<float>::load(brow + kn, nb);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a[j] = na[j];
            b[j] = nb[j];
        }
    }
    return acc;
}

__global__ __launch_bounds__(KP_THREADS) void knn_probe_kernel(const float* __restrict__ Xn, const float* __restrict__ Qn, int n, int m,
                                                               int d, int k, int* __restrict__ idx_out, float* __restrict__ sim_out,
                                                               const long long* __restrict__ train_labels, int ncls, float T,
                                                               const long long* __restrict__ test_labels, long long* __restrict__ top5,
                                                               float* __restrict__ probs, unsigned long long* __restrict__ correct) {
    extern __shared__ unsigned int lds[];
    unsigned int* skey = lds;                                  // [32][257] survivor keys, later the neighbour weights (float bits)
    int* sidx = (int*)(lds + KP_ROWS * KP_PITCH);              // [32][257] survivor training rows, later their labels
    unsigned int* hist = lds + 2 * KP_ROWS * KP_PITCH;         // [32][257] histogram, later the class scores [32][65]
    __shared__ unsigned int prefix[KP_ROWS];                   // the key bits fixed so far; after 4 passes the k-th neighbour's key
    __shared__ int need[KP_ROWS];                              // entries still to take inside the current bucket
    __shared__ int cnt[KP_ROWS], trun[KP_ROWS], tcnt[KP_WAVES][KP_ROWS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int r0 = blockIdx.x * KP_ROWS;
    const int qrow = r0 + c < m ? r0 + c : m - 1;              // rows past m repeat row m-1 and are never written
    const float* arow = Qn + (size_t)qrow * d;
    const int tiles = (n + 31) >> 5;

    if (tid < KP_ROWS) {
        prefix[tid] = 0u;
        need[tid] = k;
    }
    // ---- radix select: four 8-bit passes, most significant first -------------------------------------------------------------
    for (int p = 0; p < 4; ++p) {
        const int shift = 24 - 8 * p;
        for (int e = tid; e < KP_ROWS * KP_PITCH; e += KP_THREADS) hist[e] = 0u;
        __syncthreads();
        unsigned int pre[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) pre[g] = prefix[crow(g, h)];
        for (int ct = wave; ct < tiles; ct += KP_WAVES) {
            const int col = ct * 32 + c;
            const f32x16 acc = sim_tile(arow, Xn + (size_t)(col < n ? col : n - 1) * d, d, h);
            if (col < n) {
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const unsigned int key = sim_key(acc[g]);
                    if (((unsigned long long)(key ^ pre[g]) >> (shift + 8)) == 0ull)      // inside the bucket chosen so far
                        atomicAdd(&hist[crow(g, h) * KP_PITCH + ((key >> shift) & 255u)], 1u);
                }
            }
        }
        __syncthreads();
        if (tid < KP_ROWS) {
            const int nd = need[tid];
            int cum = 0, b = 255;
            for (; b > 0; --b) {
                const int hb = (int)hist[tid * KP_PITCH + b];
                if (cum + hb >= nd) break;
                cum += hb;
            }
            need[tid] = nd - cum;
            prefix[tid] |= (unsigned int)b << shift;
        }
        __syncthreads();
    }

    // ---- final pass: keys above the threshold in any slot, ties at it by ascending training row ---------------------------------
    if (tid < KP_ROWS) {
        cnt[tid] = 0;
        trun[tid] = 0;
    }
    unsigned int thr[16];
    int nd[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        thr[g] = prefix[crow(g, h)];
        nd[g] = need[crow(g, h)];
    }
    __syncthreads();
    const unsigned int below = (1u << c) - 1u;                 // the lanes of this half with a smaller training row
    const int iters = (tiles + KP_WAVES - 1) / KP_WAVES;
    for (int it = 0; it < iters; ++it) {
        const int ct = it * KP_WAVES + wave, col = ct * 32 + c;
        const bool valid = ct < tiles && col < n;
        unsigned int key[16];
        if (ct < tiles) {                                      // wave-uniform
            const f32x16 acc = sim_tile(arow, Xn + (size_t)(col < n ? col : n - 1) * d, d, h);
#pragma unroll
            for (int g = 0; g < 16; ++g) key[g] = sim_key(acc[g]);
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g) key[g] = 0u;
        }
        bool any_tie = false;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = crow(g, h);
            if (valid && key[g] > thr[g]) {
                const int slot = atomicAdd(&cnt[row], 1);
                if (slot < k) {
                    skey[row * KP_PITCH + slot] = key[g];
                    sidx[row * KP_PITCH + slot] = col;
                }
            }
            const unsigned long long bal = __ballot(valid && key[g] == thr[g]);
            any_tie = any_tie || bal != 0ull;
            if (c == 0) tcnt[wave][row] = __popc((unsigned int)(h ? bal >> 32 : bal));
        }
        __syncthreads();
        if (any_tie) {                                         // wave-uniform
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = crow(g, h);
                const bool tie = valid && key[g] == thr[g];
                const unsigned long long bal = __ballot(tie);
                if (tie) {
                    int rank = trun[row];
                    for (int w = 0; w < wave; ++w) rank += tcnt[w][row];
                    rank += __popc((unsigned int)(h ? bal >> 32 : bal) & below);
                    if (rank < nd[g]) {
                        const int slot = k - nd[g] + rank;
                        skey[row * KP_PITCH + slot] = key[g];
                        sidx[row * KP_PITCH + slot] = col;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < KP_ROWS) {
            int s = 0;
            for (int w = 0; w < KP_WAVES; ++w) s += tcnt[w][tid];
            trun[tid] += s;
        }
        __syncthreads();
    }

    // ---- rank sort of the k survivors of every row: (key descending, training row ascending) -----------------------------------
    const bool classify = train_labels != nullptr;
    const int total = KP_ROWS * k;
    unsigned int ky[KP_PER_THREAD];
    int ix[KP_PER_THREAD], rk[KP_PER_THREAD];
#pragma unroll
    for (int i = 0; i < KP_PER_THREAD; ++i) {
        const int e = tid + KP_THREADS * i;
        ky[i] = 0u;
        ix[i] = 0;
        rk[i] = 0;
        if (e < total) {
            const int row = e / k, j = e - row * k;
            const unsigned int kj = skey[row * KP_PITCH + j];
            const int ij = sidx[row * KP_PITCH + j];
            int rank = 0;
            for (int q = 0; q < k; ++q) {
                const unsigned int kq = skey[row * KP_PITCH + q];
                const int iq = sidx[row * KP_PITCH + q];
                rank += (kq > kj || (kq == kj && iq < ij)) ? 1 : 0;
            }
            ky[i] = kj;
            ix[i] = ij;
            rk[i] = rank;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KP_PER_THREAD; ++i) {
        const int e = tid + KP_THREADS * i;
        if (e < total) {
            const int row = e / k;
            const float s = key_sim(ky[i]);
            if (!classify) {
                if (r0 + row < m) {
                    idx_out[(size_t)(r0 + row) * k + rk[i]] = ix[i];
                    sim_out[(size_t)(r0 + row) * k + rk[i]] = s;
                }
            } else {
                const long long lab = train_labels[ix[i] < 0 ? 0 : (ix[i] < n ? ix[i] : n - 1)];     // always a row of the array
                skey[row * KP_PITCH + rk[i]] = __float_as_uint(expf(s / T));
                sidx[row * KP_PITCH + rk[i]] = (lab >= 0 && lab < ncls) ? (int)lab : -1;     // a label outside 0..ncls-1 votes for nothing
            }
        }
    }
    if (!classify) return;

    // ---- class scores in neighbour-rank order, classes ranked by (score descending, class ascending) --------------------------
    float* score = reinterpret_cast<float*>(hist);
    for (int e = tid; e < KP_ROWS * KP_SCORE_PITCH; e += KP_THREADS) score[e] = 0.f;
    __syncthreads();
    bool hit1 = false, hit5 = false;
    if (tid < KP_ROWS && r0 + tid < m) {
        float* sc = score + tid * KP_SCORE_PITCH;
        for (int j = 0; j < k; ++j) {
            const int lab = sidx[tid * KP_PITCH + j];
            if (lab >= 0) sc[lab] = sc[lab] + __uint_as_float(skey[tid * KP_PITCH + j]);
        }
        const long long tgt = test_labels ? test_labels[r0 + tid] : -1;
        const int lim = k < 5 ? (k < ncls ? k : ncls) : (ncls < 5 ? ncls : 5);
        unsigned long long taken = 0ull;
        for (int r = 0; r < 5; ++r) {
            int best = -1;
            unsigned int bk = 0u;
            for (int q = 0; q < ncls; ++q) {
                if ((taken >> q) & 1ull) continue;
                const unsigned int kq = sim_key(sc[q]);
                if (best < 0 || kq > bk) {
                    best = q;
                    bk = kq;
                }
            }
            if (best >= 0) taken |= 1ull << best;
            top5[(size_t)(r0 + tid) * 5 + r] = best;           // -1 beyond the number of classes
            if (test_labels && best >= 0 && (long long)best == tgt) {
                hit1 = hit1 || r == 0;
                hit5 = hit5 || r < lim;
            }
        }
    }
    if (test_labels && wave == 0) {
        const unsigned long long b1 = __ballot(hit1), b5 = __ballot(hit5);
        if (lane == 0) {
            atomicAdd(correct, (unsigned long long)__popcll(b1));
            atomicAdd(correct + 1, (unsigned long long)__popcll(b5));
        }
    }
    if (probs) {
        __syncthreads();
        for (int e = tid; e < KP_ROWS * ncls; e += KP_THREADS) {
            const int row = e / ncls, q = e - row * ncls;
            if (r0 + row < m) probs[(size_t)(r0 + row) * ncls + q] = score[row * KP_SCORE_PITCH + q];
        }
    }
}

// One wave per row: lane l sums x^2 over the columns l, l + 64, ... in order, then a fixed butterfly.
__global__ __launch_bounds__(NORM_THREADS) void knn_probe_normalize_kernel(const float* __restrict__ X, int n, int d,
                                                                           float* __restrict__ Y) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * NORM_ROWS + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* x = X + (size_t)row * d;
    float s = 0.f;
    for (int q = lane; q < d; q += 64) s = s + x[q] * x[q];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    const float den = fmaxf(sqrtf(s), 1e-12f);
    for (int q = lane; q < d; q += 64) Y[(size_t)row * d + q] = x[q] / den;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int check_shape(const float* Xn, const float* Qn, int n, int m, int d, int k) {
    if (n < 1 || m < 0 || d < 1 || k < 1 || k > n) return GM3D_EINVAL;
    if (n > KP_MAX_N || d > KP_MAX_D || d < 8 || d % 8 != 0 || k > KP_MAX_K) return GM3D_EUNSUPPORTED;
    if (m == 0) return GM3D_OK;
    if (!Xn || !Qn || !aligned16(Xn) || !aligned16(Qn)) return GM3D_EINVAL;
    return GM3D_OK;
}

}  // namespace

extern "C" int gm3d_knn_probe_normalize(const float* X, int n, int d, float* Y, gm3d_stream_t stream) {
    if (n < 0 || d < 1) return GM3D_EINVAL;
    if (n == 0) return GM3D_OK;
    if (!X || !Y) return GM3D_EINVAL;
    return launch_lds<knn_probe_normalize_kernel>(dim3((n + NORM_ROWS - 1) / NORM_ROWS), dim3(NORM_THREADS), 0, stream, X, n, d, Y);
}

extern "C" int gm3d_knn_probe_neighbours(const float* Xn, const float* Qn, int n, int m, int d, int k, int* idx, float* sim,
                                         gm3d_stream_t stream) {
    const int rc = check_shape(Xn, Qn, n, m, d, k);
    if (rc != GM3D_OK || m == 0) return rc;
    if (!idx || !sim) return GM3D_EINVAL;
    return launch_lds<knn_probe_kernel>(dim3((m + KP_ROWS - 1) / KP_ROWS), dim3(KP_THREADS), KP_LDS, stream, Xn, Qn, n, m, d, k, idx, sim,
                                        (const long long*)nullptr, 0, 1.0f, (const long long*)nullptr, (long long*)nullptr,
                                        (float*)nullptr, (unsigned long long*)nullptr);
}

extern "C" int gm3d_knn_probe_classify(const float* Xn, const float* Qn, int n, int m, int d, int k, const long long* train_labels,
                                       int ncls, float T, const long long* test_labels, long long* top5, float* probs,
                                       long long* correct, gm3d_stream_t stream) {
    if (ncls < 1 || !(T > 0.f)) return GM3D_EINVAL;
    if (ncls < 2 || ncls > KP_MAX_CLS) return GM3D_EUNSUPPORTED;
    const int rc = check_shape(Xn, Qn, n, m, d, k);
    if (rc != GM3D_OK || m == 0) return rc;
    if (!train_labels || !top5 || (test_labels && !correct)) return GM3D_EINVAL;
    return launch_lds<knn_probe_kernel>(dim3((m + KP_ROWS - 1) / KP_ROWS), dim3(KP_THREADS), KP_LDS, stream, Xn, Qn, n, m, d, k,
                                        (int*)nullptr, (float*)nullptr, train_labels, ncls, T, test_labels, top5, probs,
                                        reinterpret_cast<unsigned long long*>(correct));
}
