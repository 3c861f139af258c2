// Launchers of guided.hip: the teacher-guided mask and the pairwise ranking loss for 65..512 tokens per cloud.  They sit behind
// gm3d_mask_select(_b) and gm3d_rank_loss(_tail) in embed.hip, which validate the arguments and keep the <= 64 kernels.
#pragma once
#include "common.hpp"

namespace gm3d {

constexpr int GUIDED_NARROW = 64;       // up to here: embed.hip's one-wave kernels, untouched
constexpr int GUIDED_MAX = 512;         // up to here: guided.hip, one workgroup per cloud

int launch_mask_select_wide(const float* loss_pred, const float* noise, int B, int L, int len_keep, int len_loss, float* mask,
                            unsigned char* mask_bool, long long* vis_ids, long long* mask_ids, int vis_pitch, int mask_pitch,
                            gm3d_stream_t stream);

int launch_rank_loss_wide(const float* pred, int ldp, const float* target, int B, int M, float* out, float* dpred, gm3d_stream_t stream);

}  // namespace gm3d
