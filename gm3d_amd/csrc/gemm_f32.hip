// fp32 GEMMs of the parity mode (bf16=False) on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): the dense products the fp32 step
// otherwise hands to the BLAS library, with an accumulation order that is ours.
//
//   gm3d_gemm_tn_f32   C (M,N) = A (M,K) . W (N,K)^T (+ bias)     forward and (on the transposed weight) input gradient
//   gm3d_gemm_nt_f32   out[b] (N,K) (+)= dY[b] (R,N)^T . X[b] (R,K)  weight gradient, batched, long R cut into row slabs
//
// Accumulation-order rule.  Every output element is ONE chain of MFMA accumulations over the reduction index, in an order that
// depends on the reduction length alone: k runs in units of 16; inside a unit MFMA j (0..7) adds the products at k = 16u + j and
// k = 16u + 8 + j (TN) or at rows 2j and 2j + 1 of the unit (NT).  Neither M, N, the tile height, the grid nor the CU that ran the
// tile enters; there is no split-K in TN and no atomic anywhere.  Indices past the end are zero-filled operands (+0 products).
// NT slabs are whole launches' worth of such chains (slab s = rows [s * slab_rows, (s + 1) * slab_rows)); a second launch adds
// them in ascending slab order.
//
// Tiles: 128 (or 64) x 128 outputs per 256-thread workgroup, four waves of 64 x 64 (32 x 64), 32 reduction indices per stage,
// register prefetch of the next stage under the MFMAs of the current one.  LDS: TN rows of 32 floats at a pitch of 36 (144 bytes:
// a 16-lane group's ds_read_b128 of 16 rows lands on 16 different 16-byte slots); NT rows of 128 floats at a pitch of 160 (the two
// lane halves read rows 2j and 2j + 1, 32 banks apart).
#include "common.hpp"
#include "mfma.hpp"

using namespace gm3d;

namespace {

constexpr int F_THREADS = 256, F_BN = 128, F_BK = 32;
constexpr int TN_PITCH = F_BK + 4;              // floats
constexpr int NT_PITCH = F_BN + 32;             // floats
constexpr int NT_SLAB_ALIGN = F_BK;             // slabs start on a stage boundary

// four consecutive floats of row `row` at column `col` of a (rows, cols) row-major matrix; zeros outside.  `vec`: base 16-byte
// aligned and pitch a multiple of 4 (col is one by construction).
__device__ __forceinline__ float4 load4(const float* __restrict__ base, long long ld, long long row, long long rows, int col, int cols,
                                        bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows && col < cols) {
        const float* p = base + row * ld + col;
        if (vec && col + 4 <= cols) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            v.x = p[0];
            if (col + 1 < cols) v.y = p[1];
            if (col + 2 < cols) v.z = p[2];
            if (col + 3 < cols) v.w = p[3];
        }
    }
    return v;
}

// ---- TN ------------------------------------------------------------------------------------------------------------------------
// WM: 32-row MFMA tiles per wave in M (1: 64-row workgroup tile, 2: 128-row)
template <int WM>
__global__ __launch_bounds__(F_THREADS) void gemm_tn_f32_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                                const float* __restrict__ bias, float* __restrict__ C, int M, int N,
                                                                int K, long long lda, long long ldw, long long ldc, int tiles_n,
                                                                int total, int vec_a, int vec_w) {
    constexpr int BM = 64 * WM;
    constexpr int A_CH = BM * (F_BK / 4) / F_THREADS, W_CH = F_BN * (F_BK / 4) / F_THREADS;   // float4 chunks per thread and stage
    __shared__ __attribute__((aligned(16))) float sA[BM * TN_PITCH];
    __shared__ __attribute__((aligned(16))) float sW[F_BN * TN_PITCH];

    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tile >= total) return;
    const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
    const long long m0 = (long long)tm * BM;
    const int n0 = tn * F_BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;

    f32x16 acc[WM][2];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = zero16();

    float4 ra[A_CH], rw[W_CH];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            const int e = tid + F_THREADS * i, r = e >> 3, q = e & 7;
            ra[i] = load4(A, lda, m0 + r, M, k0 + 4 * q, K, vec_a);
        }
#pragma unroll
        for (int i = 0; i < W_CH; ++i) {
            const int e = tid + F_THREADS * i, r = e >> 3, q = e & 7;
            rw[i] = load4(W, ldw, n0 + r, N, k0 + 4 * q, K, vec_w);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            const int e = tid + F_THREADS * i, r = e >> 3, q = e & 7;
            *reinterpret_cast<float4*>(&sA[r * TN_PITCH + 4 * q]) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < W_CH; ++i) {
            const int e = tid + F_THREADS * i, r = e >> 3, q = e & 7;
            *reinterpret_cast<float4*>(&sW[r * TN_PITCH + 4 * q]) = rw[i];
        }
    };

    const int stages = (K + F_BK - 1) / F_BK;
    fetch(0);
    for (int s = 0; s < stages; ++s) {
        stash();
        __syncthreads();
        if (s + 1 < stages) fetch((s + 1) * F_BK);
        // the units of this stage that hold any k < K (a zero unit would add +0 products only; skipping it keeps the chain the same
        // for every tile because it depends on K alone)
        const int units = (K - s * F_BK > 16) ? 2 : 1;
        for (int u = 0; u < units; ++u) {
            float a[WM][8], b[2][8];
#pragma unroll
            for (int i = 0; i < WM; ++i) V8<float>::load(&sA[(wm * 32 * WM + i * 32 + c) * TN_PITCH + 16 * u + 8 * h], a[i]);
#pragma unroll
            for (int j = 0; j < 2; ++j) V8<float>::load(&sW[(wn * 64 + j * 32 + c) * TN_PITCH + 16 * u + 8 * h], b[j]);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma_f32(a[i][kk], b[j][kk], acc[i][j]);
        }
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 64 + j * 32 + c;
        if (col >= N) continue;
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const long long row = m0 + wm * 32 * WM + i * 32 + crow(g, h);
                if (row < M) C[row * ldc + col] = bias ? acc[i][j][g] + bv : acc[i][j][g];
            }
    }
}

// ---- NT ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(F_THREADS) void gemm_nt_f32_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                                float* __restrict__ out, int R, int N, int K, long long ldy,
                                                                long long ldx, long long ldo, long long stride_y, long long stride_x,
                                                                long long stride_o, long long stride_split, int splits, int slab_rows,
                                                                int tn_, int tk_, int total, int vec_y, int vec_x, int accumulate) {
    constexpr int CH = F_BK * (F_BN / 4) / F_THREADS;       // float4 chunks per thread, operand and stage
    __shared__ __attribute__((aligned(16))) float sY[F_BK * NT_PITCH];
    __shared__ __attribute__((aligned(16))) float sX[F_BK * NT_PITCH];

    int tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tile >= total) return;
    const int tk = tile % tk_;
    tile /= tk_;
    const int tn = tile % tn_;
    tile /= tn_;
    const int sp = tile % splits, b = tile / splits;
    const int n0 = tn * F_BN, k0 = tk * F_BN;
    const long long r_begin = (long long)sp * slab_rows;
    const long long r_end = r_begin + slab_rows < R ? r_begin + slab_rows : R;
    const float* Yb = dY + (size_t)b * stride_y;
    const float* Xb = X + (size_t)b * stride_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int wn = wave >> 1, wk = wave & 1;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = zero16();

    float4 ry[CH], rx[CH];
    auto fetch = [&](long long r0) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = tid + F_THREADS * i, r = e >> 5, q = e & 31;
            ry[i] = load4(Yb, ldy, r0 + r, r_end, n0 + 4 * q, N, vec_y);
            rx[i] = load4(Xb, ldx, r0 + r, r_end, k0 + 4 * q, K, vec_x);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = tid + F_THREADS * i, r = e >> 5, q = e & 31;
            *reinterpret_cast<float4*>(&sY[r * NT_PITCH + 4 * q]) = ry[i];
            *reinterpret_cast<float4*>(&sX[r * NT_PITCH + 4 * q]) = rx[i];
        }
    };

    const int stages = (int)((r_end - r_begin + F_BK - 1) / F_BK);
    fetch(r_begin);
    for (int s = 0; s < stages; ++s) {
        stash();
        __syncthreads();
        if (s + 1 < stages) fetch(r_begin + (long long)(s + 1) * F_BK);
#pragma unroll 4
        for (int j2 = 0; j2 < F_BK / 2; ++j2) {
            const int r = 2 * j2 + h;
            float a[2], bb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = sY[r * NT_PITCH + wn * 64 + i * 32 + c];
#pragma unroll
            for (int j = 0; j < 2; ++j) bb[j] = sX[r * NT_PITCH + wk * 64 + j * 32 + c];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_f32(a[i], bb[j], acc[i][j]);
        }
        __syncthreads();
    }

    float* o = out + (size_t)b * stride_o + (size_t)sp * stride_split;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = k0 + wk * 64 + j * 32 + c;
        if (col >= K) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = n0 + wn * 64 + i * 32 + crow(g, h);
                if (row < N) {
                    float* p = o + (size_t)row * ldo + col;
                    *p = accumulate ? *p + acc[i][j][g] : acc[i][j][g];
                }
            }
    }
}

// out[b] (N, ldo) (+)= part[b][0] + part[b][1] + ... in ascending slab order; part (batch, splits, N, K) dense
__global__ __launch_bounds__(256) void nt_f32_slab_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int splits, int N,
                                                              int K, long long ldo, long long stride_o, long long per_batch,
                                                              int accumulate) {
    const long long nk = (long long)N * K;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per_batch; e += (long long)gridDim.x * 256) {
        const long long b = e / nk, rem = e - b * nk;
        const long long n = rem / K, k = rem - n * K;
        const float* p = part + (size_t)b * splits * nk + rem;
        float v = p[0];
        for (int s = 1; s < splits; ++s) v += p[(size_t)s * nk];
        float* o = out + (size_t)b * stride_o + (size_t)n * ldo + k;
        *o = accumulate ? *o + v : v;
    }
}

int slab_rows_of(int R, int splits) {
    const long long per = ((long long)R + splits - 1) / splits;
    return (int)((per + NT_SLAB_ALIGN - 1) / NT_SLAB_ALIGN * NT_SLAB_ALIGN);
}

}  // namespace

extern "C" int gm3d_gemm_tn_f32(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, long long lda,
                                long long ldw, long long ldc, gm3d_stream_t stream) {
    if (!A || !W || !C || M < 1 || N < 1 || K < 1 || lda < K || ldw < K || ldc < N) return GM3D_EINVAL;
    if ((((size_t)A | (size_t)W | (size_t)C | (size_t)bias) & 3) != 0) return GM3D_EUNSUPPORTED;
    const long long tn = (N + F_BN - 1) / F_BN;
    const long long t128 = (((long long)M + 127) / 128) * tn;
    const bool small = t128 < 512;               // few tiles: 64-row tiles give the chip twice as many workgroups (same chains)
    const int bm = small ? 64 : 128;
    const long long total = (((long long)M + bm - 1) / bm) * tn;
    if (total > 0x7ffffff0LL) return GM3D_EUNSUPPORTED;
    const int grid = (int)((total + 7) / 8 * 8);
    const int vec_a = (((size_t)A & 15) == 0 && lda % 4 == 0), vec_w = (((size_t)W & 15) == 0 && ldw % 4 == 0);
    return by_int<1, 2>(bm / 64, [&](auto mi) {
        return launch_lds<gemm_tn_f32_kernel<decltype(mi)::value>>(dim3(grid), dim3(F_THREADS), 0, stream, A, W, bias, C, M, N, K, lda, ldw,
                                                                   ldc, (int)tn, (int)total, vec_a, vec_w);
    });
}

extern "C" int gm3d_gemm_nt_f32_splits(int batch, int R, int N, int K) {
    // the smallest power-of-two cut that offers the chip >= 256 workgroups while a slab keeps >= 512 rows, then the number of
    // non-empty slabs of gm3d_gemm_nt_f32_slab_rows rows: a pure function of the shape
    if (batch < 1 || R < 1 || N < 1 || K < 1) return 1;
    const long long tiles = (long long)batch * ((N + F_BN - 1) / F_BN) * ((K + F_BN - 1) / F_BN);
    int s = 1;
    while (tiles * s < 256 && s < 64 && R / (2 * s) >= 512) s *= 2;
    const int slab = slab_rows_of(R, s);
    return (int)(((long long)R + slab - 1) / slab);
}

extern "C" int gm3d_gemm_nt_f32_slab_rows(int R, int splits) {
    if (R < 1 || splits < 1) return 0;
    return slab_rows_of(R, splits);
}

extern "C" int gm3d_gemm_nt_f32(const float* dY, const float* X, float* out, float* part, int batch, int R, int N, int K, long long ldy,
                                long long ldx, long long ldo, long long stride_y, long long stride_x, long long stride_o, int splits,
                                int accumulate, gm3d_stream_t stream) {
    if (!dY || !X || !out || batch < 0 || R < 1 || N < 1 || K < 1 || splits < 1 || ldy < N || ldx < K || ldo < K) return GM3D_EINVAL;
    if (stride_y < 0 || stride_x < 0 || stride_o < 0 || (splits > 1 && !part)) return GM3D_EINVAL;
    if (batch > 1 && stride_o < (long long)(N - 1) * ldo + K) return GM3D_EINVAL;
    if (splits > 64) return GM3D_EUNSUPPORTED;
    if ((((size_t)dY | (size_t)X | (size_t)out | (size_t)part) & 3) != 0) return GM3D_EUNSUPPORTED;
    const int slab = slab_rows_of(R, splits);
    if ((long long)(splits - 1) * slab >= R) return GM3D_EINVAL;        // an empty slab: not a split gm3d_gemm_nt_f32_splits gives
    if (batch == 0) return GM3D_OK;
    const int tn_ = (N + F_BN - 1) / F_BN, tk_ = (K + F_BN - 1) / F_BN;
    const long long total = (long long)batch * splits * tn_ * tk_;
    if (total > 0x7ffffff0LL) return GM3D_EUNSUPPORTED;
    const int grid = (int)((total + 7) / 8 * 8);
    const int vec_y = (((size_t)dY & 15) == 0 && ldy % 4 == 0 && (batch == 1 || stride_y % 4 == 0));
    const int vec_x = (((size_t)X & 15) == 0 && ldx % 4 == 0 && (batch == 1 || stride_x % 4 == 0));
    if (splits == 1)
        return launch_lds<gemm_nt_f32_kernel>(dim3(grid), dim3(F_THREADS), 0, stream, dY, X, out, R, N, K, ldy, ldx, ldo, stride_y, stride_x,
                                              stride_o, 0LL, 1, slab, tn_, tk_, (int)total, vec_y, vec_x, accumulate ? 1 : 0);
    const long long nk = (long long)N * K;
    const int rc = launch_lds<gemm_nt_f32_kernel>(dim3(grid), dim3(F_THREADS), 0, stream, dY, X, part, R, N, K, ldy, ldx, (long long)K,
                                                  stride_y, stride_x, (long long)splits * nk, nk, splits, slab, tn_, tk_, (int)total, vec_y,
                                                  vec_x, 0);
    if (rc != GM3D_OK) return rc;
    const long long per_batch = (long long)batch * nk;
    const long long blocks = (per_batch + 255) / 256;
    return launch_lds<nt_f32_slab_sum_kernel>(dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, part, out, splits, N, K,
                                              ldo, stride_o, per_batch, accumulate ? 1 : 0);
}
