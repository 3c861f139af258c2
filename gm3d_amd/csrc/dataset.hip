// Batch assembly from a device-resident dataset in one launch: what the reference's __getitem__s do per sample on the host
// (Point-MAE_SA3D/datasets/ShapeNet55Dataset.py:45-67 random_sample + pc_norm, ModelNetDataset.py:138-145 and
// ScanObjectNNDataset.py:33-44 the shuffle of the train split) plus the collate and the host-to-device copy behind them.
//
// One workgroup per output cloud.  The cloud's N0 keys (one uniform draw per point, made by the caller) go to LDS as packed 64-bit
// (ordered_key, index) pairs, padded to a power of two with maximal pairs, and are sorted ascending by a bitonic network: a fixed
// sequence of compare-exchanges, no atomics, no data-dependent order.  (key, index) is a strict total order (NaN and -0 included),
// so the sorted sequence -- and with it every output -- is a pure function of the inputs: row j of the output is the point with the
// j-th smallest pair, a uniformly random ordered subset of the cloud when the keys are independent uniform draws (what
// shuffle + [:num] produces), the cloud's first num points in file order when all keys are equal.
//
// normalize = 1 is pc_norm of the selected points in fp32: the mean is a tree reduction (per thread over the rows t, t + T, ... in
// order, a fixed butterfly inside the wave, then the wave sums in wave order) divided by num; the scale is one correctly rounded
// square root of the largest squared norm ((x*x + y*y) + z*z, no FMA: the file is built with -ffp-contract=off), which equals the
// reference's largest square root because sqrt is monotone; every coordinate is then an IEEE division by it.  normalize = 0 copies
// the source bits.
#include "common.hpp"

namespace gm3d {

constexpr int DS_MAX_N = 8192, DS_THREADS_MAX = 1024;

// Sum over the workgroup, the same value in every thread: xor butterfly inside the wave, then the wave sums added in wave order.
__device__ __forceinline__ float block_sum(float v, float* red, int t, int nwaves) {
#pragma unroll
    for (int o = 1; o < GM3D_WAVE; o <<= 1) v = __fadd_rn(v, __shfl_xor(v, o));
    __syncthreads();                                         // the previous reduction's readers are done with `red`
    if ((t & (GM3D_WAVE - 1)) == 0) red[t / GM3D_WAVE] = v;
    __syncthreads();
    float s = red[0];
    for (int w = 1; w < nwaves; ++w) s = __fadd_rn(s, red[w]);
    return s;
}

__device__ __forceinline__ float block_max(float v, float* red, int t, int nwaves) {
#pragma unroll
    for (int o = 1; o < GM3D_WAVE; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((t & (GM3D_WAVE - 1)) == 0) red[t / GM3D_WAVE] = v;
    __syncthreads();
    float s = red[0];
    for (int w = 1; w < nwaves; ++w) s = fmaxf(s, red[w]);
    return s;
}

// P = N0 rounded up to a power of two; blockDim.x = T, a multiple of 64; dynamic LDS = P * 8 bytes.
__global__ __launch_bounds__(DS_THREADS_MAX) void sample_normalize_kernel(const float* __restrict__ data,
                                                                          const long long* __restrict__ cloud_idx,
                                                                          const float* __restrict__ keys, int M, int N0, int P, int num,
                                                                          int normalize, float* __restrict__ out,
                                                                          int* __restrict__ idx_out) {
    extern __shared__ unsigned long long pairs[];
    __shared__ float red[DS_THREADS_MAX / GM3D_WAVE];
    const int b = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    const float* kb = keys + (size_t)b * N0;
    for (int i = t; i < P; i += T)
        pairs[i] = i < N0 ? ((unsigned long long)ordered_key(kb[i]) << 32) | (unsigned)i : ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (P >> 1); i += T) {
                const int lo = 2 * i - (i & (j - 1)), hi = lo + j;       // the i-th pair of positions that differ in bit j
                const unsigned long long a = pairs[lo], c = pairs[hi];
                if ((a > c) == ((lo & k) == 0)) {
                    pairs[lo] = c;
                    pairs[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    long long cl = cloud_idx[b];
    cl = cl < 0 ? 0 : (cl >= M ? M - 1 : cl);                // an out-of-range cloud index must not read outside the dataset
    const float* src = data + (size_t)cl * N0 * 3;
    float* ob = out + (size_t)b * num * 3;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int j = t; j < num; j += T) {
        const int i = (int)(unsigned)pairs[j];                            // < N0: the num <= N0 smallest pairs are real ones
        const float x = src[(size_t)i * 3], y = src[(size_t)i * 3 + 1], z = src[(size_t)i * 3 + 2];
        if (idx_out) idx_out[(size_t)b * num + j] = i;
        if (!normalize) {
            ob[(size_t)j * 3] = x;
            ob[(size_t)j * 3 + 1] = y;
            ob[(size_t)j * 3 + 2] = z;
        }
        sx = __fadd_rn(sx, x);
        sy = __fadd_rn(sy, y);
        sz = __fadd_rn(sz, z);
    }
    if (!normalize) return;
    // The selected points are read again from global memory (cache hits) in each of the two passes below rather than kept in
    // registers: 1024 threads leave 128 registers each, and eight rows of three coordinates with their addresses spilled.
    const int nwaves = T / GM3D_WAVE;
    const float fn = (float)num;
    const float mx = __fdiv_rn(block_sum(sx, red, t, nwaves), fn);
    const float my = __fdiv_rn(block_sum(sy, red, t, nwaves), fn);
    const float mz = __fdiv_rn(block_sum(sz, red, t, nwaves), fn);
    float m2 = 0.f;                                          // squared norms are >= 0: 0 is the identity of their maximum
    for (int j = t; j < num; j += T) {
        const int i = (int)(unsigned)pairs[j];
        const float x = __fsub_rn(src[(size_t)i * 3], mx), y = __fsub_rn(src[(size_t)i * 3 + 1], my),
                    z = __fsub_rn(src[(size_t)i * 3 + 2], mz);
        m2 = fmaxf(m2, __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
    }
    const float m = __fsqrt_rn(block_max(m2, red, t, nwaves));
    for (int j = t; j < num; j += T) {
        const int i = (int)(unsigned)pairs[j];
        ob[(size_t)j * 3] = __fdiv_rn(__fsub_rn(src[(size_t)i * 3], mx), m);
        ob[(size_t)j * 3 + 1] = __fdiv_rn(__fsub_rn(src[(size_t)i * 3 + 1], my), m);
        ob[(size_t)j * 3 + 2] = __fdiv_rn(__fsub_rn(src[(size_t)i * 3 + 2], mz), m);
    }
}

}  // namespace gm3d

extern "C" int gm3d_sample_normalize(const float* data, const long long* cloud_idx, const float* keys, int B, int M, int N0, int num,
                                     int normalize, float* out, int* idx_out, gm3d_stream_t stream) {
    using namespace gm3d;
    if (!data || !cloud_idx || !keys || !out || B < 1 || M < 1 || N0 < 1 || num < 1 || num > N0) return GM3D_EINVAL;
    if (normalize != 0 && normalize != 1) return GM3D_EINVAL;
    if (N0 > DS_MAX_N) return GM3D_EUNSUPPORTED;
    int P = 1;
    while (P < N0) P <<= 1;
    int threads = (P / 2 + GM3D_WAVE - 1) / GM3D_WAVE * GM3D_WAVE;               // one compare-exchange per thread and step ...
    threads = threads < GM3D_WAVE ? GM3D_WAVE : (threads > DS_THREADS_MAX ? DS_THREADS_MAX : threads);   // ... up to 1024 threads
    return launch_lds<sample_normalize_kernel>(dim3(B), dim3(threads), (size_t)P * sizeof(unsigned long long), stream, data, cloud_idx,
                                               keys, M, N0, P, num, normalize, out, idx_out);
}
