// The two GeoMask3D operators that are one wavefront per cloud in embed.hip, for 65..512 tokens per cloud: one workgroup per cloud,
// one thread per token, the cloud's values in LDS.  Both are small latency-bound launches (B workgroups of at most 8 waves); a cloud
// is never split across workgroups, so neither needs atomics or a second pass and both are pure functions of their inputs.
//
// mask_select_wide_kernel -- generate_mask (P/models_mae_learn_loss.py:744-784) + the id lists of split_ids, the rule of embed.hip's
//   mask_select_kernel: the len_loss tokens with the highest loss_pred are forced masked, the others are ranked by noise and the first
//   len_keep stay visible.  Keys are compared as order-preserving integers (common.hpp ordered_key, as mask.hip does): (key, index) is
//   a strict total order for every bit pattern, so the ranks of a cloud are a permutation of 0..L-1, exactly len_keep tokens are
//   visible and every id is written once, inside its row.  A forced token's second key is the largest integer, above +inf and every
//   NaN, so a forced token is never visible (len_keep + len_loss <= L).  For finite inputs without -0 the result is the stable-argsort
//   formulation's bit for bit.
// rank_loss_wide_kernel -- the pair terms of forward_learning_loss (P/:795-805), the arithmetic of embed.hip's rank_loss_kernel with
//   the wave broadcast replaced by broadcast LDS reads; the per-cloud sums are reduced in a fixed order (wave butterfly, then an LDS
//   tree over the waves).  Outputs as rank_loss_kernel's: rank_loss_finish_kernel and rank_loss_bwd_kernel follow unchanged.
#include "guided.hpp"

namespace gm3d {

constexpr int GUIDED_WAVES = GUIDED_MAX / GM3D_WAVE;
constexpr unsigned int KEY_LAST = 0xFFFFFFFFu;          // above every ordered_key of a finite value, +inf and (almost) every NaN

// number of (key[j], j) pairs below (k, t), j < n4 (a multiple of 4, padded with KEY_LAST at indices >= L > t: never counted)
__device__ __forceinline__ int rank_below(const unsigned int* key, int n4, unsigned int k, int t) {
    int rank = 0;
    for (int j = 0; j < n4; j += 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(key + j);         // same address in every lane: one broadcast read
        rank += (q.x < k || (q.x == k && j < t)) ? 1 : 0;
        rank += (q.y < k || (q.y == k && j + 1 < t)) ? 1 : 0;
        rank += (q.z < k || (q.z == k && j + 2 < t)) ? 1 : 0;
        rank += (q.w < k || (q.w == k && j + 3 < t)) ? 1 : 0;
    }
    return rank;
}

__global__ __launch_bounds__(GUIDED_MAX) void mask_select_wide_kernel(const float* __restrict__ loss_pred, const float* __restrict__ noise,
                                                                      int L, int len_keep, int len_loss, float* __restrict__ mask,
                                                                      long long* __restrict__ vis_ids, long long* __restrict__ mask_ids,
                                                                      int vis_pitch, int mask_pitch, unsigned char* __restrict__ mask_b) {
    __shared__ __attribute__((aligned(16))) unsigned int klp[GUIDED_MAX];
    __shared__ __attribute__((aligned(16))) unsigned int knz[GUIDED_MAX];
    __shared__ int nvis[GUIDED_WAVES], nmsk[GUIDED_WAVES];
    const int b = blockIdx.x, l = threadIdx.x, w = l / GM3D_WAVE, lane = l % GM3D_WAVE;
    const bool in = l < L;                                   // blockDim.x = L rounded up to whole waves: l < GUIDED_MAX
    const int n4 = (L + 3) & ~3;                             // <= blockDim.x
    const unsigned int k1 = in ? ordered_key(loss_pred[(size_t)b * L + l]) : KEY_LAST;
    unsigned int k2 = in ? ordered_key(noise[(size_t)b * L + l]) : KEY_LAST;
    klp[l] = k1;
    __syncthreads();
    if (in && rank_below(klp, n4, k1, l) >= L - len_loss) k2 = KEY_LAST;      // one of the len_loss highest: forced masked
    knz[l] = k2;
    __syncthreads();
    const bool keep = in && rank_below(knz, n4, k2, l) < len_keep;
    const unsigned long long kb = __ballot(keep), mb = __ballot(in && !keep);
    if (lane == 0) { nvis[w] = __popcll(kb); nmsk[w] = __popcll(mb); }
    __syncthreads();
    if (in) {
        int voff = 0, moff = 0;                              // visible / masked tokens in the waves before this one
        for (int q = 0; q < w; ++q) { voff += nvis[q]; moff += nmsk[q]; }
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        mask[(size_t)b * L + l] = keep ? 0.f : 1.f;
        if (mask_b) mask_b[(size_t)b * L + l] = keep ? 0 : 1;
        if (keep) vis_ids[(size_t)b * vis_pitch + voff + __popcll(kb & below)] = l;          // < len_keep: exactly len_keep are kept
        else mask_ids[(size_t)b * mask_pitch + moff + __popcll(mb & below)] = l;             // < L - len_keep
    }
}

__global__ __launch_bounds__(GUIDED_MAX) void rank_loss_wide_kernel(const float* __restrict__ p, int ldp, const float* __restrict__ t, int M,
                                                                    float* __restrict__ out, float* __restrict__ dp) {
    __shared__ float2 pt[GUIDED_MAX];                        // (p_i, t_i)
    __shared__ float red[2][GUIDED_WAVES];
    const int b = blockIdx.x, j = threadIdx.x, w = j / GM3D_WAVE, lane = j % GM3D_WAVE;
    const bool in = j < M;
    const float pj = in ? p[(size_t)b * ldp + j] : 0.f, tj = in ? t[(size_t)b * M + j] : 0.f;
    pt[j] = make_float2(pj, tj);
    if (j < GUIDED_WAVES) { red[0][j] = 0.f; red[1][j] = 0.f; }      // waves the launch does not have add nothing
    __syncthreads();
    float ls = 0.f, cnt = 0.f, g = 0.f;
    if (in) {
        for (int i = 0; i < M; ++i) {
            const float2 v = pt[i];                          // broadcast read
            const float pi = v.x, ti = v.y;
            // pair (i, j): D = p_j - p_i
            const float sg = 1.0f / (1.0f + __expf(-(pj - pi)));
            const float ds = sg * (1.0f - sg);
            if (tj > ti) { ls -= __logf(sg + 1e-6f); cnt += 1.f; g -= ds / (sg + 1e-6f); }
            else if (tj < ti) { ls -= __logf(1.0f - sg + 1e-6f); cnt += 1.f; g += ds / (1.0f - sg + 1e-6f); }
            // pair (j, i): D' = p_i - p_j, contributes -dL/dD' to p_j
            const float s2 = 1.0f / (1.0f + __expf(-(pi - pj)));
            const float d2 = s2 * (1.0f - s2);
            if (ti > tj) g += d2 / (s2 + 1e-6f);
            else if (ti < tj) g -= d2 / (1.0f - s2 + 1e-6f);
        }
        dp[(size_t)b * M + j] = g;
    }
    for (int o = 32; o > 0; o >>= 1) { ls += __shfl_xor(ls, o); cnt += __shfl_xor(cnt, o); }
    if (lane == 0) { red[0][w] = ls; red[1][w] = cnt; }
    __syncthreads();
    for (int o = GUIDED_WAVES / 2; o > 0; o >>= 1) {         // fixed-order tree over the waves
        if (j < o) { red[0][j] += red[0][j + o]; red[1][j] += red[1][j + o]; }
        __syncthreads();
    }
    if (j == 0) { out[(size_t)b * 2] = red[0][0]; out[(size_t)b * 2 + 1] = red[1][0]; }
}

static int wide_threads(int n) { return (n + GM3D_WAVE - 1) / GM3D_WAVE * GM3D_WAVE; }

int launch_mask_select_wide(const float* loss_pred, const float* noise, int B, int L, int len_keep, int len_loss, float* mask,
                            unsigned char* mask_bool, long long* vis_ids, long long* mask_ids, int vis_pitch, int mask_pitch,
                            gm3d_stream_t stream) {
    if (L <= GUIDED_NARROW || L > GUIDED_MAX) return GM3D_EUNSUPPORTED;
    return launch_lds<mask_select_wide_kernel>(dim3(B), dim3(wide_threads(L)), 0, stream, loss_pred, noise, L, len_keep, len_loss, mask,
                                               vis_ids, mask_ids, vis_pitch, mask_pitch, mask_bool);
}

int launch_rank_loss_wide(const float* pred, int ldp, const float* target, int B, int M, float* out, float* dpred, gm3d_stream_t stream) {
    if (M <= GUIDED_NARROW || M > GUIDED_MAX) return GM3D_EUNSUPPORTED;
    return launch_lds<rank_loss_wide_kernel>(dim3(B), dim3(wide_threads(M)), 0, stream, pred, ldp, target, M, out, dpred);
}

}  // namespace gm3d
