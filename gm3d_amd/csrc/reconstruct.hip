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
//
// gm3d_reconstruct_partition is the ragged form for the hierarchical model, where the visible count differs from cloud to cloud: the
// id lists are replaced by the mask bytes, and the launch itself forms the stable partition [visible tokens | masked tokens] of every
// cloud.  ceil(G/16) workgroups per cloud; each recomputes the cloud's ranks from the G mask bytes -- one 64-bit ballot and popcount per
// 64-token chunk, an exclusive prefix over the (at most 128) chunk counts in LDS -- which is cheaper than a second launch or a
// grid-wide wait, and then moves its 16 tokens at once: 16 lanes per patch, four patches per wave -- the model's patches are 6 (k = 8)
// and 12 (k = 16) 16-byte units, so a whole wave per patch leaves most lanes idle and makes a wave walk its patches one dependent
// read chain after the other (measured: DESIGN 16).  The workgroup walks TOKENS, not slots: a token's slot is `visible tokens before
// it` or `all visible + masked tokens before it`, so no inverse map is needed and the slots, being a permutation, are still written
// exactly once.  No atomics, no dependence between workgroups.
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

// Elements [0, row) of one patch, by the LANES lanes `lane` = 0 .. LANES-1: out[e] = float(src[e]) + c[e % 3].
template <class S, bool VEC, int LANES = GM3D_WAVE>
__device__ __forceinline__ void ra_patch(const S* __restrict__ src, float* __restrict__ out, int row, int lane, float cx, float cy,
                                         float cz) {
    if (VEC) {
        for (int q = lane; q < (row >> 2); q += LANES) {
            float v[4];
            ra_load4<S>(src + 4 * q, v);
            const int r = q % 3;                             // element 4q + t is coordinate (q + t) % 3
            const float c0 = r == 0 ? cx : (r == 1 ? cy : cz), c1 = r == 0 ? cy : (r == 1 ? cz : cx),
                        c2 = r == 0 ? cz : (r == 1 ? cx : cy);
            *reinterpret_cast<float4*>(out + 4 * q) =
                make_float4(__fadd_rn(v[0], c0), __fadd_rn(v[1], c1), __fadd_rn(v[2], c2), __fadd_rn(v[3], c0));
        }
    } else {
        for (int e = lane; e < row; e += LANES) {
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

constexpr int RP_WAVES = 4, RP_LANES = 16, RP_TOKENS = RP_WAVES * GM3D_WAVE / RP_LANES, RP_MAX_G = 8192,
              RP_MAX_CHUNKS = RP_MAX_G / GM3D_WAVE;

// PRED == false: no decoder output; a masked token's rows are its true patch (T is float and `pred` is not read).
template <class T, bool VEC, bool PRED>
__global__ __launch_bounds__(RP_WAVES* GM3D_WAVE) void reconstruct_partition_kernel(
    const T* __restrict__ pred, const float* __restrict__ neighborhood, const float* __restrict__ center,
    const unsigned char* __restrict__ masked, int G, int k, int slices, float* __restrict__ dense, float* __restrict__ full_center,
    int* __restrict__ order, int* __restrict__ n_visible) {
    __shared__ unsigned long long s_vis[RP_MAX_CHUNKS];      // bit l of entry c: token 64c + l is visible
    __shared__ int s_before[RP_MAX_CHUNKS + 1];              // visible tokens in the chunks before c; the last used entry: all of them
    const int lane = threadIdx.x & (GM3D_WAVE - 1), wave = threadIdx.x / GM3D_WAVE;
    const int b = blockIdx.x / slices, slice = blockIdx.x - b * slices;
    const int chunks = (G + GM3D_WAVE - 1) / GM3D_WAVE, row = 3 * k;
    const unsigned char* m = masked + (size_t)b * G;
    for (int c = wave; c < chunks; c += RP_WAVES) {
        const int t = c * GM3D_WAVE + lane;
        const unsigned long long vis = __ballot(t < G && m[t] == 0);
        if (lane == 0) s_vis[c] = vis;
    }
    __syncthreads();
    if (wave == 0) {                                         // exclusive prefix of the chunk counts: two chunks per lane
        const int c0 = 2 * lane, c1 = c0 + 1;
        const int n0 = c0 < chunks ? __popcll(s_vis[c0]) : 0, n1 = c1 < chunks ? __popcll(s_vis[c1]) : 0;
        int incl = n0 + n1;
#pragma unroll
        for (int d = 1; d < GM3D_WAVE; d <<= 1) {
            const int up = __shfl_up(incl, d, GM3D_WAVE);
            if (lane >= d) incl += up;
        }
        const int excl = incl - (n0 + n1);
        if (c0 < chunks) s_before[c0] = excl;
        if (c1 < chunks) s_before[c1] = excl + n0;
        if (lane == GM3D_WAVE - 1) s_before[chunks] = incl;
    }
    __syncthreads();
    const int nv = s_before[chunks];
    if (slice == 0 && threadIdx.x == 0) n_visible[b] = nv;
    const int t = slice * RP_TOKENS + threadIdx.x / RP_LANES, sub = lane & (RP_LANES - 1);      // 16 lanes share a token
    if (t < G) {
        const int c = t / GM3D_WAVE, l = t & (GM3D_WAVE - 1);
        const unsigned long long vis = s_vis[c];
        const int before = s_before[c] + __popcll(vis & ((1ull << l) - 1));      // visible tokens in front of t
        const bool is_masked = !((vis >> l) & 1);
        const int slot = is_masked ? nv + (t - before) : before;
        const size_t tok = (size_t)b * G + t, dst = (size_t)b * G + slot;
        const float* cp = center + tok * 3;
        const float cx = cp[0], cy = cp[1], cz = cp[2];
        if (sub < 3) full_center[dst * 3 + sub] = sub == 0 ? cx : (sub == 1 ? cy : cz);
        if (sub == 3) order[dst] = t;
        float* out = dense + dst * row;
        if (PRED && is_masked)
            ra_patch<T, VEC, RP_LANES>(pred + tok * row, out, row, sub, cx, cy, cz);
        else
            ra_patch<float, VEC, RP_LANES>(neighborhood + tok * row, out, row, sub, cx, cy, cz);
    }
}

template <class T, bool VEC, bool PRED>
static int rp_launch(const void* pred, const float* neighborhood, const float* center, const unsigned char* masked, int B, int G, int k,
                     float* dense, float* full_center, int* order, int* n_visible, gm3d_stream_t st) {
    const int slices = (G + RP_TOKENS - 1) / RP_TOKENS;      // B * slices <= B * G < 2^31 / 3: a valid grid
    return launch_lds<reconstruct_partition_kernel<T, VEC, PRED>>(dim3((unsigned)B * slices), dim3(RP_WAVES * GM3D_WAVE), 0, st,
                                                                  (const T*)pred, neighborhood, center, masked, G, k, slices, dense,
                                                                  full_center, order, n_visible);
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
    const int P = B * G;
    const int blocks = (P + RA_WAVES - 1) / RA_WAVES < RA_MAX_BLOCKS ? (P + RA_WAVES - 1) / RA_WAVES : RA_MAX_BLOCKS;
    return by_dtype(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        auto launch = [&](auto v) {                        // v: std::true_type for the 16-byte form
            return launch_lds<reconstruct_assemble_kernel<T, decltype(v)::value>>(
                dim3(blocks), dim3(RA_WAVES * GM3D_WAVE), 0, stream, (const T*)pred, (size_t)pred_bstride, neighborhood, center, vis_ids,
                (size_t)vis_stride, mask_ids, (size_t)mask_stride, B, G, k, V, M, layout, dense, full_center);
        };
        return vec ? launch(std::true_type{}) : launch(std::false_type{});
    });
}

extern "C" int gm3d_reconstruct_partition(const void* pred, const float* neighborhood, const float* center, const unsigned char* masked,
                                          int B, int G, int k, int dtype, float* dense, float* full_center, int* order, int* n_visible,
                                          gm3d_stream_t stream) {
    using namespace gm3d;
    if (!neighborhood || !center || !masked || !dense || !full_center || !order || !n_visible) return GM3D_EINVAL;
    if (B < 0 || G < 1 || k < 1) return GM3D_EINVAL;
    if (dtype != GM3D_F32 && dtype != GM3D_BF16) return GM3D_EINVAL;
    if (G > RP_MAX_G) return GM3D_EUNSUPPORTED;                                   // the chunk prefix is one wave, two chunks per lane
    if ((long long)B * G * k * 3 >= 0x80000000LL) return GM3D_EUNSUPPORTED;      // the grid size and the row length are ints
    if (B == 0) return GM3D_OK;
    const size_t esz = dtype == GM3D_BF16 ? 2 : 4;
    // 16-byte accesses need 16-byte patch rows everywhere: k % 4 == 0 and aligned bases (pred rows are dense: 3k elements)
    const bool vec = k % 4 == 0 && ((uintptr_t)neighborhood | (uintptr_t)dense) % 16 == 0 && (!pred || (uintptr_t)pred % (4 * esz) == 0);
    // (element type, PRED) takes three of its four combinations, so this instance table stays a macro
#define GM3D_RP(T, VEC, PRED) \
    rp_launch<T, VEC, PRED>(pred, neighborhood, center, masked, B, G, k, dense, full_center, order, n_visible, stream)
    if (!pred) return vec ? GM3D_RP(float, true, false) : GM3D_RP(float, false, false);
    if (dtype == GM3D_BF16) return vec ? GM3D_RP(bf16_t, true, true) : GM3D_RP(bf16_t, false, true);
    return vec ? GM3D_RP(float, true, true) : GM3D_RP(float, false, true);
#undef GM3D_RP
}
