// Centre masking of plain Point-MAE pre-training (Point-MAE_SA3D/models/Point_MAE.py:268-317) in one launch.
//
// Beneath: MaskTransformer._mask_center_rand (a host shuffle per cloud) and _mask_center_block (norm / argsort / scatter), plus the
// boolean-mask indexing that follows them (:333-336, :411-413, :425).  Neither form can sit inside a captured step.
//
// Both modes are "mask the num_mask groups with the smallest keys": rand ranks a (B,G) noise draw (a uniformly random subset of
// exactly num_mask groups, what the shuffle produces), block ranks the squared distance to a start centre (sqrt is monotone, so the
// nearest num_mask are the same set wherever the reference's Euclidean norms are distinct).  One workgroup per cloud, one thread per
// group: the keys go to LDS as order-preserving integers, every thread counts the (key, index) pairs below its own -- at most
// 512 x 512 compares per cloud -- and is masked iff that rank is < num_mask.  (key, index) is a strict total order (NaN and -0
// included), so exactly num_mask groups are masked whatever the input holds and every id lands inside its row.  The ascending id lists
// are a prefix count over the mask bytes.  No atomics, no data-dependent order: the result is a pure function of the inputs.
#include "common.hpp"

namespace gm3d {

constexpr int MC_MAX = 512;

__global__ __launch_bounds__(MC_MAX) void mask_centers_kernel(const float* __restrict__ in, const int* __restrict__ start, int mode,
                                                              int G, int num_mask, unsigned char* __restrict__ mask_bool,
                                                              long long* __restrict__ order, int id_pitch) {
    __shared__ unsigned int key[MC_MAX];
    __shared__ unsigned char mk[MC_MAX];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < G) {
        float v;
        if (mode == 0) {
            v = in[(size_t)b * G + t];
        } else {
            const float* c = in + (size_t)b * G * 3;
            int s = start[b];
            s = s < 0 ? 0 : (s >= G ? G - 1 : s);            // an out-of-range start index must not read outside the cloud
            v = sqdist3(c[s * 3], c[s * 3 + 1], c[s * 3 + 2], c[t * 3], c[t * 3 + 1], c[t * 3 + 2]);
        }
        key[t] = ordered_key(v);
    }
    __syncthreads();
    int m = 0;
    if (t < G) {
        const unsigned int k = key[t];
        int rank = 0;
        for (int j = 0; j < G; ++j) {
            const unsigned int kj = key[j];
            rank += (kj < k || (kj == k && j < t)) ? 1 : 0;
        }
        m = rank < num_mask ? 1 : 0;
        mk[t] = (unsigned char)m;
        mask_bool[(size_t)b * G + t] = (unsigned char)m;
    }
    __syncthreads();
    if (t < G) {
        int before = 0;                                      // masked groups with a smaller id
        for (int j = 0; j < t; ++j) before += mk[j];
        const int pos = m ? (G - num_mask) + before : t - before;
        order[(size_t)b * id_pitch + pos] = (long long)t;
    }
}

}  // namespace gm3d

extern "C" int gm3d_mask_centers(const float* keys_or_center, const int* start, int mode, int B, int G, int num_mask,
                                 unsigned char* mask_bool, long long* order, int id_pitch, gm3d_stream_t stream) {
    using namespace gm3d;
    if (!keys_or_center || !mask_bool || !order || B < 0 || G < 1 || (mode != 0 && mode != 1)) return GM3D_EINVAL;
    if (mode == 1 && !start) return GM3D_EINVAL;
    if (G > MC_MAX) return GM3D_EUNSUPPORTED;
    if (num_mask < 0 || num_mask >= G || id_pitch < G) return GM3D_EINVAL;
    if (B == 0) return GM3D_OK;
    const int threads = (G + 63) / 64 * 64;
    return launch_lds<mask_centers_kernel>(dim3(B), dim3(threads), 0, stream, keys_or_center, start, mode, G, num_mask, mask_bool, order,
                                           id_pitch);
}
