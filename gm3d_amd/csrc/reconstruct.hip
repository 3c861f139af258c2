// Dense clouds from a masked autoencoder's output in one launch: the `vis` branch of the reference's Point_MAE.forward
// (Point-MAE_SA3D/models/Point_MAE.py:428-439), which gathers the visible patches and the masked centres by boolean-mask indexing
// (one host synchronisation per line), adds the centres back and concatenates.
//
// One wave per output patch (3k floats), four patches per workgroup, the rest by a grid stride.  The wave reads its patch's id and
// centre once (wave-uniform addresses), lanes 0..2 write the centre row, and lane q moves element q, q + 64, ... of the patch, so
// consecutive lanes write consecutive floats of `dense`: 16 bytes each where a patch row keeps 16-byte alignment (k % 4 == 0 and
// aligned bases: the VEC instantiation), 4 bytes each otherwise.  A visible row is neighborhood + centre, a rebuilt row
// float(pred) + centre: one fp32 add per element and nothing else, so the result is the aten chain's, bit for bit.
// No LDS, no barriers, no atomics; every element of both outputs is written exactly once.
#include "common.hpp"

namespace gm3d {

constexpr int RA_WAVES = 4, RA_MAX_BLOCKS = 2048;

template <class T> __device__ __forceinline__ void ra_load4(const T* p, float* v);
template <> __device__ __forceinline__ void ra_load4<float>(const float* p, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
template <> __device__ __forceinline__ void ra_load4<bf16_t>(const bf16_t* p, float* v) {
    typedef __bf16 v4 __attribute__((ext_vector_type(4)));
    const v4 a = *reinterpret_cast<const v4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)a[i];
}

// Elements [0, row) of one patch: out[e] = float(src[e]) + c[e % 3].
template <class S, bool VEC>
__device__ __forceinline__ void ra_patch(const S* __restrict__ src, float* __restrict__ out, int row, int lane, float cx, float cy,
                                         float cz) {
    if (VEC) {
        for (int q = lane; q < (row >> 2); q += GM3D_WAVE) {
            float v[4];
            ra_load4<S>(src + 4 * q, v);
            const int r = q % 3;                             // element 4q + t is coordinate (q + t) % 3
            const float c0 = r == 0 ? cx : (r == 1 ? cy : cz), c1 = r == 0 ? cy : (r == 1 ? cz : cx),
                        c2 = r == 0 ? cz : (r == 1 ? cx : cy);
            *reinterpret_cast<float4*>(out + 4 * q) =
                make_float4(__fadd_rn(v[0], c0), __fadd_rn(v[1], c1), __fadd_rn(v[2], c2), __fadd_rn(v[3], c0));
        }
    } else {
        for (int e = lane; e < row; e += GM3D_WAVE) {
            const int r = e % 3;
            out[e] = __fadd_rn((float)src[e], r == 0 ? cx : (r == 1 ? cy : cz));
        }
    }
}

template <class T, bool VEC>
__global__ __launch_bounds__(RA_WAVES* GM3D_WAVE) void reconstruct_assemble_kernel(
    const T* __restrict__ pred, size_t pred_bstride, const float* __restrict__ neighborhood, const float* __restrict__ center,
    const long long* __restrict__ vis_ids, size_t vis_stride, const long long* __restrict__ mask_ids, size_t mask_stride, int B, int G,
    int k, int V, int M, int layout, float* __restrict__ dense, float* __restrict__ full_center) {
    const int lane = threadIdx.x & (GM3D_WAVE - 1), wave = threadIdx.x / GM3D_WAVE;
    const int P = B * G, row = 3 * k, BV = B * V;
    for (int p = blockIdx.x * RA_WAVES + wave; p < P; p += gridDim.x * RA_WAVES) {
        int b, i;
        bool masked;
        if (layout == GM3D_RECON_PER_CLOUD) {                // cloud b: [V visible | M rebuilt]
            b = p / G;
            i = p - b * G;
            masked = i >= V;
            if (masked) i -= V;
        } else if (p < BV) {                                 // flat: all clouds' visible patches ...
            b = p / V;
            i = p - b * V;
            masked = false;
        } else {                                             // ... then all clouds' rebuilt patches
            b = (p - BV) / M;
            i = (p - BV) - b * M;
            masked = true;
        }
        long long id = masked ? mask_ids[(size_t)b * mask_stride + i] : vis_ids[(size_t)b * vis_stride + i];
        id = id < 0 ? 0 : (id >= G ? G - 1 : id);            // the ids are trusted; a wrong one still reads inside its cloud
        const float* c = center + ((size_t)b * G + (size_t)id) * 3;
        const float cx = c[0], cy = c[1], cz = c[2];
        // flat full_center is [all masked | all visible] while flat dense is [all visible | all rebuilt]: the reference's own order
        const int crow = layout == GM3D_RECON_PER_CLOUD ? p : (masked ? b * M + i : B * M + b * V + i);
        if (lane < 3) full_center[(size_t)crow * 3 + lane] = lane == 0 ? cx : (lane == 1 ? cy : cz);
        float* out = dense + (size_t)p * row;
        if (masked)
            ra_patch<T, VEC>(pred + (size_t)b * pred_bstride + (size_t)i * row, out, row, lane, cx, cy, cz);
        else
            ra_patch<float, VEC>(neighborhood + ((size_t)b * G + (size_t)id) * row, out, row, lane, cx, cy, cz);
    }
}

template <class T, bool VEC>
static void ra_launch(const void* pred, long long pred_bstride, const float* neighborhood, const float* center, const long long* vis_ids,
                      long long vis_stride, const long long* mask_ids, long long mask_stride, int B, int G, int k, int V, int M,
                      int layout, float* dense, float* full_center, hipStream_t st) {
    const int P = B * G;
    const int blocks = (P + RA_WAVES - 1) / RA_WAVES < RA_MAX_BLOCKS ? (P + RA_WAVES - 1) / RA_WAVES : RA_MAX_BLOCKS;
    hipLaunchKernelGGL((reconstruct_assemble_kernel<T, VEC>), dim3(blocks), dim3(RA_WAVES * GM3D_WAVE), 0, st, (const T*)pred,
                       (size_t)pred_bstride, neighborhood, center, vis_ids, (size_t)vis_stride, mask_ids, (size_t)mask_stride, B, G, k,
                       V, M, layout, dense, full_center);
}

}  // namespace gm3d

extern "C" int gm3d_reconstruct_assemble(const void* pred, long long pred_bstride, const float* neighborhood, const float* center,
                                         const long long* vis_ids, long long vis_stride, const long long* mask_ids,
                                         long long mask_stride, int B, int G, int k, int V, int M, int layout, float* dense,
                                         float* full_center, int dtype, gm3d_stream_t stream) {
    using namespace gm3d;
    if (!neighborhood || !center || !dense || !full_center) return GM3D_EINVAL;
    if (B < 0 || G < 1 || k < 1 || V < 0 || M < 0 || (long long)V + M != G) return GM3D_EINVAL;
    if (layout != GM3D_RECON_PER_CLOUD && layout != GM3D_RECON_FLAT) return GM3D_EINVAL;
    if (dtype != GM3D_F32 && dtype != GM3D_BF16) return GM3D_EINVAL;
    if (V > 0 && (!vis_ids || vis_stride < V)) return GM3D_EINVAL;
    if (M > 0 && (!mask_ids || mask_stride < M || !pred || pred_bstride < (long long)M * 3 * k)) return GM3D_EINVAL;
    if ((long long)B * G * k * 3 >= 0x80000000LL) return GM3D_EUNSUPPORTED;      // patch and row indices are formed in int
    if (B == 0) return GM3D_OK;
    const size_t esz = dtype == GM3D_BF16 ? 2 : 4;
    // 16-byte accesses need 16-byte patch rows everywhere: k % 4 == 0, aligned bases, and a pred batch stride of whole 4-element units
    const bool vec = k % 4 == 0 && ((uintptr_t)neighborhood | (uintptr_t)dense) % 16 == 0 &&
                     (M == 0 || ((uintptr_t)pred % (4 * esz) == 0 && pred_bstride % 4 == 0));
    hipStream_t st = (hipStream_t)stream;
#define GM3D_RA(T, VEC)                                                                                                             \
    ra_launch<T, VEC>(pred, pred_bstride, neighborhood, center, vis_ids, vis_stride, mask_ids, mask_stride, B, G, k, V, M, layout, \
                      dense, full_center, st)
    if (dtype == GM3D_BF16) {
        if (vec) GM3D_RA(bf16_t, true); else GM3D_RA(bf16_t, false);
    } else {
        if (vec) GM3D_RA(float, true); else GM3D_RA(float, false);
    }
#undef GM3D_RA
    GM3D_CHECK_LAUNCH();
    return GM3D_OK;
}
