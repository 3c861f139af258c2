/*
 * gm3d.h -- C ABI of libgm3d_hip.so, the MI355X (gfx950) native back end of the
 * Point-MAE + GeoMask3D pretrain hot path.
 *
 * The reference's boundary for this path is Python-level torch ops in three
 * third-party packages; each entry point below names the
 * reference interface it sits beneath.  Conventions for every call:
 *   - plain device pointers + sizes, no torch types; the caller owns every buffer;
 *   - all tensors are dense row-major ("contiguous") in the stated shape;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and the call returns without synchronising;
 *   - return value GM3D_OK or a negative GM3D_E* code, never throws, no global
 *     state, thread-compatible; argument/shape errors are detected on the host
 *     BEFORE any launch (a bad shape never reaches a kernel);
 *   - inputs are never written.
 */
#ifndef GM3D_H
#define GM3D_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *gm3d_stream_t; /* hipStream_t */

enum {
    GM3D_OK = 0,
    GM3D_EINVAL = -1,       /* null pointer / non-positive size / inconsistent shape */
    GM3D_EUNSUPPORTED = -2, /* shape outside what the kernels are built for */
    GM3D_ELAUNCH = -3       /* hipLaunchKernel reported an error */
};

enum { GM3D_F32 = 0, GM3D_BF16 = 1 };

/* ABI version (bumped on any signature change) and error text. */
int gm3d_abi_version(void);
const char *gm3d_strerror(int code);

/* Farthest point sampling.
 * Replaces pointnet2_ops.pointnet2_utils.furthest_point_sample
 *   (Point-MAE_SA3D/models_mae_learn_loss.py:931, utils/miscc.py:18,
 *    engine_finetune.py:132, tools/runner_finetune.py:141).
 * xyz (B,N,3) f32 -> idx (B,npoint) int32; centers (B,npoint,3) f32 optional (NULL
 * to skip): the gather_operation of :932 fused into the same launch.
 * Rule: idx[0]=0, running min init 1e10, points with |p|^2<=1e-3 never selected,
 * argmax ties -> lowest index, d=((dx*dx+dy*dy)+dz*dz) fp32 without FMA.
 * Limits: 1 <= npoint, N <= 16384. */
int gm3d_fps(const float *xyz, int B, int N, int npoint, int32_t *idx, float *centers,
             gm3d_stream_t stream);

/* out[b,c,j] = feat[b,c,idx[b,j]].
 * Replaces pointnet2_utils.gather_operation forward (models_mae_learn_loss.py:932,
 * utils/miscc.py:19, engine_finetune.py:134).  feat (B,C,N) f32, idx (B,M) int32. */
int gm3d_gather_points(const float *feat, const int32_t *idx, int B, int C, int N, int M,
                       float *out, gm3d_stream_t stream);

/* Backward of gather_operation: grad_feat (B,C,N) is fully written (zero where no
 * index hits); duplicates accumulate in ascending j (deterministic). */
int gm3d_gather_points_grad(const float *grad_out, const int32_t *idx, int B, int C, int N, int M,
                            float *grad_feat, gm3d_stream_t stream);

/* Brute-force k-NN, ascending, ties -> lower reference index.
 * Replaces knn_cuda.KNN(k, transpose_mode=True)(ref, query)
 *   (models_mae_learn_loss.py:924,946; models/Point_MAE.py:55,68).
 * ref (B,N,3), query (B,G,3) f32 -> idx (B,G,k) int64, dist (B,G,k) f32 Euclidean
 * (sqrt applied) or NULL.  Limits: 1 <= k <= min(N,64), N <= 12288. */
int gm3d_knn(const float *ref, const float *query, int B, int N, int G, int k,
             float *dist, int64_t *idx, gm3d_stream_t stream);

/* Fused k-NN + neighbourhood gather + centre subtract = the body of Group.forward
 * after FPS (models_mae_learn_loss.py:946-957) in one launch.
 * Outputs: idx (B,G,k) int64 (may be NULL), neighborhood (B,G,k,3) = xyz[idx]-center,
 * neighborhood_org (B,G,k,3) = xyz[idx] (may be NULL). */
int gm3d_knn_group(const float *xyz, const float *center, int B, int N, int G, int k,
                   int64_t *idx, float *neighborhood, float *neighborhood_org,
                   gm3d_stream_t stream);

/* Chamfer nearest-neighbour squared-L2 distances, both directions, first minimum wins.
 * Replaces extensions.chamfer_dist forward (ChamferDistanceL2 at
 * models_mae_learn_loss.py:188,407; models/Point_MAE.py:392-394,426).
 * xyz1 (P,n,3), xyz2 (P,m,3) f32 -> dist1 (P,n), dist2 (P,m) f32, idx1 (P,n),
 * idx2 (P,m) int32.  n==m==32 takes the wave-per-patch path. */
int gm3d_chamfer_fwd(const float *xyz1, const float *xyz2, int P, int n, int m,
                     float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                     gm3d_stream_t stream);

/* Backward of the above: gxyz1 (P,n,3), gxyz2 (P,m,3) fully written.
 * grad_dist1/2 may be NULL (treated as zeros).  n==m==32 is atomic-free and
 * deterministic; other shapes use float atomics like the upstream kernel. */
int gm3d_chamfer_bwd(const float *xyz1, const float *xyz2, const int32_t *idx1, const int32_t *idx2,
                     const float *grad_dist1, const float *grad_dist2, int P, int n, int m,
                     float *gxyz1, float *gxyz2, gm3d_stream_t stream);

/* Multi-head softmax attention core of timm-0.4.5 Attention.forward
 * (in-tree twin Point-MAE_SA3D/models/Point_MAE.py:113-125): for each (b,h)
 *   out[b,t,h,:] = softmax(scale * q k^T)[t,:] v
 * qkv is the (B,T,3,H,64) output of the qkv Linear, out is (B,T,H*64).
 * dtype GM3D_F32 (exact-f32 MFMA, parity mode) or GM3D_BF16 (bf16 MFMA, f32
 * softmax/accumulate).  lse (B,H,T) f32 = log-sum-exp of the scaled scores, saved
 * for backward (may be NULL for inference).  Limits: head_dim == 64, 1 <= T <= 128. */
int gm3d_attention_fwd(const void *qkv, void *out, float *lse, int B, int T, int H,
                       float scale, int dtype, gm3d_stream_t stream);

/* The qkv projection and the attention in one launch (bf16, T <= 64, C == 384 == H*64): replaces
 * `qkv = self.qkv(x)` + the attention above (Point-MAE_SA3D/models/Point_MAE.py:113-122) for one Block.
 * h (B*T, C) bf16 = the normalised tokens, wqkv (3*C, C) bf16 row-major (nn.Linear weight, no bias:
 * models_mae_learn_loss.py:907-911 qkv_bias=False).  out (B,T,C) bf16; lse (B,H,T) f32 or NULL;
 * qkv_out (B,T,3,H,64) bf16 or NULL (written for the backward; bit-identical to gm3d_gemm_tn_bf16_ring's
 * product, so out/lse are bit-identical to gm3d_attention_fwd on it).  GM3D_EUNSUPPORTED outside those limits. */
int gm3d_attention_qkv_fwd(const void *h, const void *wqkv, void *out, float *lse, void *qkv_out,
                           int B, int T, int H, int C, float scale, int dtype, gm3d_stream_t stream);

/* Backward: dqkv (B,T,3,H,64) fully written from dout (B,T,H*64), qkv, out, lse. */
int gm3d_attention_bwd(const void *qkv, const void *out, const void *dout, const float *lse,
                       void *dqkv, int B, int T, int H, float scale, int dtype,
                       gm3d_stream_t stream);

/* The pre-training loss on the masked patches in one pass (models_mae_learn_loss.py:384-412 forward_loss: target[mask] gather, fp32
 * cast, ChamferDistanceL2 per point (d1 + d2), mean over the 32 points -> `matrix`, mean of everything -> Chamfer_mean).
 * pred: the decoder head's output for the M masked tokens of each cloud, (B, M, 96) in `dtype` with batch stride pred_bstride
 * elements (a view of the (B, L, 96) output is fine); target (B, T, 32, 3) f32 = the neighbourhoods; ids (B, M) int64 = the masked
 * group ids (row stride ids_bstride).  Out: matrix (B, M) f32, idx1 / idx2 (B*M, 32) int32 (argmins, for the backward), mean_out (1)
 * f32.  Distances and argmins as gm3d_chamfer_fwd (bit-identical); the means are summed in a fixed order. */
int gm3d_patch_chamfer_loss_fwd(const void *pred, long long pred_bstride, const float *target, const long long *ids,
                                long long ids_bstride, int B, int T, int M, float *matrix, int32_t *idx1, int32_t *idx2,
                                float *mean_out, int dtype, gm3d_stream_t stream);
/* dpred (B, M, 96) contiguous in `dtype` = gmean[0] * d(mean_out)/d(pred). */
int gm3d_patch_chamfer_loss_bwd(const void *pred, long long pred_bstride, const float *target, const long long *ids,
                                long long ids_bstride, const int32_t *idx1, const int32_t *idx2, const float *gmean, int B, int T,
                                int M, void *dpred, int dtype, gm3d_stream_t stream);
/* ... as the gradient of the FULL prediction (B, lead + M, 96) whose last M patches entered the loss (outs['pix_pred'][:, -M:],
 * engine_pretrain.py:131): the first `lead` patches of every cloud receive zeros -- the slice's backward in the same launch. */
int gm3d_patch_chamfer_loss_bwd_full(const void *pred, long long pred_bstride, const float *target, const long long *ids,
                                     long long ids_bstride, const int32_t *idx1, const int32_t *idx2, const float *gmean, int B, int T,
                                     int M, int lead, void *dpred, int dtype, gm3d_stream_t stream);
/* The same pass for plain Point-MAE's `cdl1` loss (models/Point_MAE.py:391-392,426: ChamferDistanceL1 on the masked patches =
 * (mean(sqrt d1) + mean(sqrt d2)) / 2 over the B * M patches x 32 points).  Same arguments as gm3d_patch_chamfer_loss_fwd / _bwd;
 * matrix (B, M) = the per-patch value (sum sqrt d1 + sum sqrt d2) / 64, mean_out its mean, summed in a fixed order.  Argmins
 * bit-identical to gm3d_chamfer_fwd.  The backward multiplies by sqrt's 1 / (2 sqrt d) with no guard at d = 0, like torch.sqrt's
 * backward in the unfused form (a predicted point exactly on its neighbour gives inf * 0).  B == 0 returns GM3D_OK launching
 * nothing; B * M <= 2^26 - 1 (GM3D_EUNSUPPORTED beyond). */
int gm3d_patch_chamfer_l1_loss_fwd(const void *pred, long long pred_bstride, const float *target, const long long *ids,
                                   long long ids_bstride, int B, int T, int M, float *matrix, int32_t *idx1, int32_t *idx2,
                                   float *mean_out, int dtype, gm3d_stream_t stream);
int gm3d_patch_chamfer_l1_loss_bwd(const void *pred, long long pred_bstride, const float *target, const long long *ids,
                                   long long ids_bstride, const int32_t *idx1, const int32_t *idx2, const float *gmean, int B, int T,
                                   int M, void *dpred, int dtype, gm3d_stream_t stream);
/* The same two losses for patches of k points (the reference's config_2 / config_3 geometries: 128 x 16 and 256 x 8): pred
 * (B, M, 3k), target (B, T, k, 3) f32, idx1 / idx2 (B*M, k) int32, everything else as above.  l1 != 0 selects the `cdl1` value
 * (sum sqrt d1 + sum sqrt d2) / (2k) and its backward.  k == 32 runs the entry points above (same kernels, same bits); k == 8 / 16
 * run wave-segment kernels (k lanes per patch, 64 / k patches per wave, no LDS, no atomics, sums in a fixed order); any other k
 * is GM3D_EUNSUPPORTED.  The backward writes dpred (B, lead + M, 3k) in `dtype`, zeros for the first `lead` patches of every cloud;
 * lead != 0 with l1 is GM3D_EINVAL (the 32-point `cdl1` backward has no such form).  B == 0 returns GM3D_OK launching nothing;
 * B * (lead + M) * k <= 2^31 - 1 (GM3D_EUNSUPPORTED beyond).  Every argument is checked on the host before a launch. */
int gm3d_patch_chamfer_loss_k_fwd(const void *pred, long long pred_bstride, const float *target, const long long *ids,
                                  long long ids_bstride, int B, int T, int M, int k, int l1, float *matrix, int32_t *idx1,
                                  int32_t *idx2, float *mean_out, int dtype, gm3d_stream_t stream);
int gm3d_patch_chamfer_loss_k_bwd(const void *pred, long long pred_bstride, const float *target, const long long *ids,
                                  long long ids_bstride, const int32_t *idx1, const int32_t *idx2, const float *gmean, int B, int T,
                                  int M, int k, int lead, int l1, void *dpred, int dtype, gm3d_stream_t stream);

/* Plain LayerNorm over (R, C) rows, 4 <= C <= 512, C % 4 == 0 (nn.LayerNorm of the 96 / 192 / 384-wide Point-M2AE levels):
 * h = (x - mean) * rstd * gamma + beta in `dtype`, mean / rstd (R) f32 saved for the backward.  Backward: dx in `dtype`;
 * partial (gm3d_ln_plain_partial_rows(R), 2, C) f32: [.][0] = per-block sums of dh * xhat (dgamma), [.][1] = of dh (dbeta), to be
 * finished by gm3d_colsum_finish over 2*C columns. */
int gm3d_ln_plain_partial_rows(int R);
int gm3d_ln_plain_fwd(const void *x, const float *gamma, const float *beta, float eps, void *h, float *mean, float *rstd, int R,
                      int C, int dtype, gm3d_stream_t stream);
int gm3d_ln_plain_bwd(const void *dh, const void *x, const float *mean, const float *rstd, const float *gamma, void *dx,
                      float *partial, int R, int C, int dtype, gm3d_stream_t stream);
/* The same LayerNorm with the residual sum formed in the kernel (the pre-norm blocks of the hierarchical encoder / decoder, any
 * width 4 <= C <= 512, C % 4 == 0: Point-M2AE_SA3D/cfgs/config_Point_M2AE.yaml:57-99 dims 96 / 192 / 384):
 *   s = x + rowscale[row / rows_per_sample] * (y + ybias) + z   (y, ybias, rowscale, z optional; s_out required with y or z),
 *   h = LayerNorm(s as stored).   One pass instead of two or three elementwise launches + a LayerNorm.
 * gamma == NULL: the sum only (the tail of a block stack); gm3d_add_ln_bwd with dh == NULL is its backward (dx = gin, dy, and the
 * column sum of dy). */
int gm3d_add_ln_fwd(const void *x, const void *y, const float *ybias, const float *rowscale, int rows_per_sample, const void *z,
                    const float *gamma, const float *beta, float eps, void *s_out, void *h, float *mean, float *rstd, int R, int C,
                    int dtype, gm3d_stream_t stream);
/* Its backward: dx = gin + LayerNorm-backward(dh) (gin optional: the gradient arriving at s from the next residual sum), dy =
 * rowscale * dx (optional), partial (gm3d_ln_plain_partial_rows(R), nsum, C): [0] dgamma, [1] dbeta and, with nsum == 3, [2]
 * sum_rows dy = the gradient of ybias. */
int gm3d_add_ln_bwd(const void *dh, const void *gin, const void *x, const float *mean, const float *rstd, const float *gamma,
                    const float *rowscale, int rows_per_sample, void *dx, void *dy, float *partial, int nsum, int R, int C, int dtype,
                    gm3d_stream_t stream);
/* ... with a running sum over the sites that share an addend (the positional embedding re-added in front of every block of a
 * stack): acc (R,C) `dtype`, acc_mode 0 none / 1 acc = dx / 2 acc += dx.  dh == NULL (no LayerNorm behind the sum): x, mean, rstd,
 * gamma are not read and may be NULL. */
int gm3d_add_ln_bwd_acc(const void *dh, const void *gin, const void *x, const float *mean, const float *rstd, const float *gamma,
                        const float *rowscale, int rows_per_sample, void *dx, void *dy, float *partial, int nsum, void *acc,
                        int acc_mode, int R, int C, int dtype, gm3d_stream_t stream);

/* ---- Row-wise fused passes around the transformer-block GEMMs (gm3d_amd/csrc/rowops.hip) ------------
 * Together they restate timm-0.4.5 Block.forward (in-tree twin Point-MAE_SA3D/models/Point_MAE.py:128-146)
 * as driven by TransformerEncoder/Decoder.forward (models_mae_learn_loss.py:914-917,984-990).
 * The residual stream is fp32; `dtype` (GM3D_F32 / GM3D_BF16) is the type of the GEMM-side tensors.
 * C must be 384 (trans_dim) for the LayerNorm entry points. */

/* out_res[r,:] = res[r,:] + rowscale[r / rows_per_sample] * (y[r,:] + bias) + add[r,:]
 * h[r,:]       = LayerNorm(out_res[r,:]) * gamma + beta          (eps as given; mean/rstd saved per row)
 * res/out_res f32 (R,C); y, add, h `dtype` (R,C); bias, gamma, beta f32 (C); rowscale f32 (R/rows_per_sample)
 * = the DropPath keep/(1-p) factor per sample.  y, bias, rowscale, add, out_res, res may be NULL (at
 * least one of res/y/add must be given). */
int gm3d_residual_ln_fwd(const float *res, const void *y, const float *bias, const float *rowscale,
                         int rows_per_sample, const void *add, const float *gamma, const float *beta,
                         float eps, float *out_res, void *h, float *mean, float *rstd, int R, int C,
                         int dtype, gm3d_stream_t stream);

/* Backward of one such site.  dh (R,C) `dtype` = grad of h; gin (R,C) f32 = grad already flowing on the
 * residual stream (NULL = none); x = the saved out_res.  Writes dx (R,C) f32 = grad wrt out_res,
 * dy (R,C) `dtype` = rowscale * dx (NULL to skip), acc (R,C) f32 += dx (NULL to skip; positional grad), acc_out (R,C) `dtype` =
 * the updated acc in the GEMM-side type as well (NULL to skip; needs acc), and per-workgroup column partial sums
 * partial[gm3d_ln_partial_rows(R)][3][C] f32: [0] dgamma, [1] dbeta, [2] colsum(dy) (= gradient of `bias`). */
int gm3d_residual_ln_bwd(const void *dh, const float *gin, const float *x, const float *mean,
                         const float *rstd, const float *gamma, const float *rowscale, int rows_per_sample,
                         float *dx, void *dy, float *acc, void *acc_out, float *partial, int R, int C, int dtype,
                         gm3d_stream_t stream);
int gm3d_ln_partial_rows(int R);   /* rows of `partial` the call above writes */

/* out[c] (+)= sum_{r<nrows} partial[r*pitch + c], c < ncols (second stage of the column sums). */
int gm3d_colsum_finish(const float *partial, int nrows, int pitch, int ncols, float *out, int accumulate,
                       gm3d_stream_t stream);

/* Batched form: job j sums partial[j*job_stride + r*pitch + c] over r < nrows into out[j*out_stride + c]. */
int gm3d_colsum_finish_batched(const float *partial, int njobs, long long job_stride, int nrows, int pitch, int ncols,
                               float *out, int out_stride, gm3d_stream_t stream);

/* g = GELU(f + bias), exact erf form (nn.GELU, Mlp at models/Point_MAE.py:82-98).  C % 8 == 0. */
int gm3d_bias_gelu_fwd(const void *f, const float *bias, void *g, int R, int C, int dtype,
                       gm3d_stream_t stream);
/* df = dg * GELU'(f + bias); partial[gm3d_gelu_partial_rows(R)][C] f32 = column partial sums of df. */
int gm3d_bias_gelu_bwd(const void *dg, const void *f, const float *bias, void *df, float *partial, int R,
                       int C, int dtype, gm3d_stream_t stream);
int gm3d_gelu_partial_rows(int R);

/* ---- Mini-PointNet token embed: streaming passes between its three wide GEMMs (gm3d_amd/csrc/embed.hip) ----
 * Together with the GEMMs they restate Encoder.forward (Point-MAE_SA3D/models_mae_learn_loss.py:868-899) and its
 * backward.  Activations are (G groups, K points, C channels) row-major in `dtype`; C % 8 == 0, C <= 1024, K <= 255.
 * Kernels that reduce over rows write per-workgroup partial rows; gm3d_embed_partial_rows(kind, n, C) gives the
 * number of rows (kind 0: gm3d_moments3, n = rows; kind 1: (G,K,C) kernels, n = G; kind 2: (R,C) kernels, n = R; kind 3: gm3d_lin3_gelu_bwd, n = R;
 * kind 4: gm3d_pn_layer1_bwd_stats, n = R),
 * and gm3d_colsum_finish adds them up. */
int gm3d_embed_partial_rows(int kind, int n, int C);

/* partial[row][0..2] = sum x_j, [3..8] = sum xx,xy,xz,yy,yz,zz (fp64) of the (R,3) f32 input: BatchNorm statistics of the
 * K=3 layer are analytic in these moments (first_conv.0/.1, :873-874). */
int gm3d_moments3(const float *x, int R, double *partial, gm3d_stream_t stream);

/* a1 (R,C1) = relu(x . wf^T + bf): Conv1d(3,128) + BatchNorm (folded into wf (C1,3), bf (C1)) + ReLU (:873-875). */
int gm3d_pn_layer1_fwd(const float *x, const float *wf, const float *bf, void *a1, int R, int C1, int dtype,
                       gm3d_stream_t stream);

/* out (G,C) = max over K of in (G,K,C) (+ bias); arg (G,C) uint8 = first maximising k (torch.max(dim)[0], :895,898). */
int gm3d_group_max_fwd(const void *in, const float *bias, void *out, uint8_t *arg, int G, int K, int C, int dtype,
                       gm3d_stream_t stream);
/* din (G,K,C) = dout (G,C) at k == arg, 0 elsewhere (dense; fully written). */
int gm3d_group_max_bwd(const void *dout, const uint8_t *arg, void *din, int G, int K, int C, int dtype,
                       gm3d_stream_t stream);

/* BatchNorm over y = y0 (G,K,C) + t (G,C)[group] (second_conv.0/.1 with the concat folded, :896-897,879-880):
 * partial[row][0][c] = sum y, [1][c] = sum y^2. */
int gm3d_bn_bcast_stats(const void *y0, const void *t, int G, int K, int C, float *partial, int dtype,
                        gm3d_stream_t stream);
/* a2 = act(y * scale + shift), act(h) = h > 0 ? h : slope*h  (slope 0: ReLU of the embed; 0.2: LeakyReLU of the
 * loss-predictor head increase_dim_2, :152-158). */
int gm3d_bn_bcast_apply_relu(const void *y0, const void *t, const float *scale, const float *shift, void *a2,
                             int G, int K, int C, float slope, int dtype, gm3d_stream_t stream);
/* backward pass 1: g = da2 * [y*scale+shift > 0]; partial[row][0][c] = sum g, [1][c] = sum g * (y-mean)*rstd. */
int gm3d_bn_bcast_bwd_stats(const void *da2, const void *y0, const void *t, const float *scale, const float *shift,
                            const float *mean, const float *rstd, int G, int K, int C, float *partial, float slope,
                            int dtype, gm3d_stream_t stream);
/* backward pass 2: dy (G,K,C) = scale * (g - s1/R - yhat * s2/R), dt (G,C) f32 = sum_k dy. */
int gm3d_bn_bcast_bwd_apply(const void *da2, const void *y0, const void *t, const float *scale, const float *shift,
                            const float *mean, const float *rstd, const float *s1, const float *s2, void *dy,
                            float *dt, int G, int K, int C, float slope, int dtype, gm3d_stream_t stream);

/* Tail of the loss-predictor head increase_dim_2 (models_mae_learn_loss.py:152-158) + `.mean(-1)` (:677): Conv1d(C -> nout) followed by
 * the mean over its nout outputs is one C-vector.  gm3d_head_fold: wv[c] = mean_o W1[o][c] (f32, and a copy in `dtype`), bm = mean(b1).
 * gm3d_head_rowdot: out[r] = round_dtype(a[r,:] . wv) + bm.  Backward: gm3d_head_fold_bwd: dW1[o][c] = dwv[c]/nout,
 * db1[o] = sum_r d[r]/nout;  gm3d_head_outer: da[r][c] = d[r] * wv[c] in `dtype`. */
int gm3d_head_fold(const float *W1, const float *b1, int nout, int C, float *wv, void *wv_t, float *bm, int dtype,
                   gm3d_stream_t stream);
int gm3d_head_rowdot(const void *a, const void *wv_t, const float *bm, int R, int C, float *out, int dtype, gm3d_stream_t stream);
int gm3d_head_fold_bwd(const float *dwv, const float *d, int R, int nout, int C, float *dW1, float *db1, gm3d_stream_t stream);
int gm3d_head_outer(const float *d, const float *wv, int R, int C, void *da, int dtype, gm3d_stream_t stream);

/* Training augmentation PointcloudScaleAndTranslate.__call__ (Point-MAE_SA3D/datasets/data_transforms.py:27-35, called at
 * engine_pretrain.py:78), in place on pc (B,N,3) f32: u (2,B,3) f32 uniform draws in [0,1) -> per-cloud scale = u[0]*span+lo (span = hi-lo),
 * shift = (u[1]*2-1)*t, p = p*scale + shift. */
int gm3d_scale_translate(float *pc, const float *u, float lo, float span, float t, int B, int N, gm3d_stream_t stream);

/* The same three passes when only a SUBSET of the groups goes on to the next layer -- the student's visible tokens: x_vis =
 * tokens[~mask] (models_mae_learn_loss.py:298) discards 39 of 64 groups per cloud after the last conv + max-pool, so that conv
 * (and its backward) only needs the visible groups' rows, while the batch statistics still cover every row.
 * gm3d_group_select_maps: ids (B,V) int64 (row pitch id_pitch) -> sel (B*V) = flat source group of every selected group and
 * inv (B*G) = position in sel, or -1.  _apply_relu_sel: a2 holds the G selected groups (compact), read from groups sel[g] of
 * y0 / t.  _bwd_stats_sel: da2 holds the G selected groups (the others' gradient is zero and contributes nothing to the sums).
 * _bwd_apply_sel: all G groups are written; da2 of group g is row block inv[g] of the compact buffer, zero when inv[g] < 0.
 * sel / inv NULL = the plain forms above. */
int gm3d_group_select_maps(const long long *ids, int id_pitch, int B, int V, int G, int *sel, int *inv, gm3d_stream_t stream);
int gm3d_bn_bcast_apply_relu_sel(const void *y0, const void *t, const float *scale, const float *shift, void *a2,
                                 const int *sel, int G, int K, int C, float slope, int dtype, gm3d_stream_t stream);
int gm3d_bn_bcast_bwd_stats_sel(const void *da2, const void *y0, const void *t, const float *scale, const float *shift,
                                const float *mean, const float *rstd, const int *sel, int G, int K, int C, float *partial,
                                float slope, int dtype, gm3d_stream_t stream);
int gm3d_bn_bcast_bwd_apply_sel(const void *da2, const void *y0, const void *t, const float *scale, const float *shift,
                                const float *mean, const float *rstd, const float *s1, const float *s2, void *dy, float *dt,
                                const int *inv, int G, int K, int C, float slope, int dtype, gm3d_stream_t stream);

/* df (G,K,C) += dfg (G,C) at k == arg (in place); partial[row][c] = column sums of the result. */
int gm3d_group_scatter_add(void *df, const void *dfg, const uint8_t *arg, int G, int K, int C, float *partial,
                           int dtype, gm3d_stream_t stream);

/* Backward reductions of Conv1d(3,C1)+BatchNorm+ReLU: with g1 = da1*[a1>0], hhat = (x.w1+b1-mean)*rstd,
 * xc = x - xmean (xmean (3) f32): partial[row][q][c] in fp64 (the weight gradient is a small difference of these
 * sums), q = 0: sum g1, 1: sum g1*hhat, 2..4: sum g1*xc_j; rows = gm3d_embed_partial_rows(4, R, C1); C1 <= 256. */
int gm3d_pn_layer1_bwd_stats(const void *da1, const void *a1, const float *x, const float *w1, const float *b1,
                             const float *mean, const float *rstd, const float *xmean, int R, int C1,
                             double *partial, int dtype, gm3d_stream_t stream);
/* fp64 second stage: out[c] = sum_r partial[r*pitch + c]. */
int gm3d_colsum_finish_f64(const double *partial, int nrows, int pitch, int ncols, double *out,
                           gm3d_stream_t stream);

/* partial[row][c] = column sums of a (R,C) matrix in `dtype`; rows = gm3d_embed_partial_rows(2, R, C); C % 8 == 0, 8 <= C <= 2048. */
int gm3d_colsum_partial(const void *m, int R, int C, float *partial, int dtype, gm3d_stream_t stream);
/* The same with a per-row weight roww (R) f32 (NULL = 1): partial sums of roww[r] * m[r][c].  Replaces the library GEMV a^T d in
 * the backward of the loss-prediction head (increase_dim_2 + mean(-1), models_mae_learn_loss.py:152-158,677): fixed summation
 * order, replay-safe. */
int gm3d_colsum_partial_w(const void *m, const float *roww, int R, int C, float *partial, int dtype, gm3d_stream_t stream);

/* out (R,C) = GELU(x (R,3) . w (C,3)^T + b): first layer + activation of pos_embed (models_mae_learn_loss.py:104-108). */
int gm3d_lin3_gelu_fwd(const float *x, const float *w, const float *b, void *out, int R, int C, int dtype,
                       gm3d_stream_t stream);
/* its backward reductions: dpre = dout * GELU'(pre); partial[row][q][c] fp64, q = 0: sum dpre, 1..3: sum dpre * x_j;
 * rows = gm3d_embed_partial_rows(3, R, C); C <= 512. */
int gm3d_lin3_gelu_bwd(const void *dout, const float *x, const float *w, const float *b, int R, int C,
                       double *partial, int dtype, gm3d_stream_t stream);
/* The finish of its partial sums in the layer's own layouts: db (C) f32 = the column sums of block 0, dW (C,3) f32 column k = block 1 + k
 * (partial (nrows, 4 C) f64, the buffer gm3d_lin3_gelu_bwd filled). */
int gm3d_lin3_finish(const double *partial, int nrows, int C, float *dW, float *db, gm3d_stream_t stream);

/* Pairwise ranking loss of forward_learning_loss(relative=True) (models_mae_learn_loss.py:795-805), per sample:
 * out (B,2) f32 = [sum of pair terms, number of ordered pairs]; dpred (B,M) = d(sum of pair terms)/d pred.
 * M <= 64: one wavefront per sample; 65..512: one workgroup per sample (guided.hip); above: GM3D_EUNSUPPORTED. */
int gm3d_rank_loss(const float *pred, const float *target, int B, int M, float *out, float *dpred,
                   gm3d_stream_t stream);
/* The whole loss_learn of engine_pretrain.py:156-171 on the last M columns of a (B, ldp)-pitched prediction (pred points at the first
 * of them): gm3d_rank_loss plus tot (2) = column sums of out in a fixed order and loss (1) = tot[0] / tot[1] -- two launches, no
 * PyTorch reduction.  _bwd: dfull (B,L) = [zeros (L - M) | dpred * (g[0] / tot[1])], the gradient of the full (B,L) prediction. */
int gm3d_rank_loss_tail(const float *pred, int ldp, const float *target, int B, int M, float *out, float *dpred, float *tot, float *loss,
                        gm3d_stream_t stream);
int gm3d_rank_loss_tail_bwd(const float *dpred, const float *g, const float *tot, int B, int M, int L, float *dfull, gm3d_stream_t stream);
/* ModelEma.update on the integer buffers (BatchNorm num_batches_tracked, P/engine_pretrain.py:36-52 applies the same blend to every state_dict
 * entry): e[i] = (int64)(float(e[i]) * decay + w * float(m[i])), w = 1 - decay formed by the caller (in double, like the Python expression). */
int gm3d_ema_counters(long long *e, const long long *m, int n, float decay, float w, gm3d_stream_t stream);
/* DropPath factors out (S,B) = floor(keep[s] + u[s][b]) / keep[s] from one uniform draw u (timm DropPath, P/models/Point_MAE.py:9). */
int gm3d_drop_path_scales(const float *u, const float *keep, int S, int B, float *out, gm3d_stream_t stream);
/* dst (R,Np) = [src (R,N), row pitch lds | zeros]; N, Np, lds multiples of 8 (a narrow operand padded to a GEMM tile width). */
int gm3d_pad_cols(const void *src, long long lds, int R, int N, void *dst, int Np, int dtype, gm3d_stream_t stream);

/* ---- Optimizer step on flat buffers (gm3d_amd/csrc/optim.hip) ------------------------------------------------------
 * clip_grad_norm_(max_norm) + torch.optim.AdamW + timm ModelEma.update + bf16 shadows, replacing
 * NativeScalerWithGradNormCount.__call__ (Point-MAE_SA3D/util/misc.py:256-270), the AdamW of tools/builder.py:40-56 and
 * model_ema.update (engine_pretrain.py:212).  All buffers hold n fp32 elements (n % 4 == 0) in one common layout whose
 * first n_decay elements (n_decay % 4 == 0) take weight decay.  lr_dev, ema_w_dev (= 1 - decay) and step_dev (the step
 * count, incremented here) are single floats in device memory.  ema / shadow_p / shadow_e (bf16) may be NULL.
 * partial: gm3d_flat_partial_rows(n) floats of scratch; scal (4 floats) receives {clip coefficient, 1-beta1^t,
 * 1-beta2^t, gradient norm before clipping}.  max_norm <= 0 disables clipping. */
int gm3d_flat_partial_rows(long long n);
int gm3d_adamw_ema_flat_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, float *ema,
                             void *shadow_p, void *shadow_e, long long n, long long n_decay, const float *lr_dev,
                             float weight_decay, float beta1, float beta2, float eps, const float *ema_w_dev,
                             float max_norm, float *step_dev, float *partial, float *scal, gm3d_stream_t stream);
/* The same step with layer-wise learning-rate decay (fine-tuning: Point-MAE_SA3D/util/lr_decay.py:15-62 builds one AdamW
 * group per layer with lr = base_lr * lr_scale): lr_scale holds one multiplier per element, in the flat layout (NULL = 1). */
int gm3d_adamw_ema_flat_step_lrd(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, float *ema,
                                 void *shadow_p, void *shadow_e, long long n, long long n_decay, const float *lr_dev,
                                 const float *lr_scale, float weight_decay, float beta1, float beta2, float eps,
                                 const float *ema_w_dev, float max_norm, float *step_dev, float *partial, float *scal,
                                 gm3d_stream_t stream);

/* BatchNorm statistic finalisation in one launch (train: from sums = [sum(C), sumsq(C)] over `rows` rows, with
 * nn.BatchNorm1d's running-statistic update -- momentum, unbiased variance, num_batches_tracked += 1; eval: from the
 * running buffers): scale = gamma*rstd, shift = beta - mean*scale, plus mean / rstd for the backward. */
int gm3d_bn_finalize(const float *sums, double rows, const float *gamma, const float *beta, float eps, float momentum,
                     float *running_mean, float *running_var, long long *nbt, float *scale, float *shift,
                     float *mean_out, float *rstd_out, int C, int training, gm3d_stream_t stream);
/* Same for the K=3 first layer, whose statistics are analytic in the input moments mom9 (gm3d_moments3, summed):
 * emits the BatchNorm-folded conv wf (C,3) / bf (C), mean / rstd, and mcov = [mean(3), cov(3x3)] fp64 and
 * xmean (3) f32 for the backward. */
int gm3d_pn1_finalize(const double *mom9, double rows, const float *w, const float *b, const float *gamma,
                      const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                      long long *nbt, float *wf, float *bf, float *mean_out, float *rstd_out, double *mcov,
                      float *xmean, int C, int training, gm3d_stream_t stream);
/* Layer-1 backward tail: q (5,C) fp64 = summed gm3d_pn_layer1_bwd_stats partials, mcov from gm3d_pn1_finalize ->
 * dw (C,3), dgamma (C), dbeta (C). */
int gm3d_pn1_bwd_finalize(const double *q, const double *mcov, const float *w, const float *gamma, const float *rstd,
                          float *dw, float *dgamma, float *dbeta, int C, gm3d_stream_t stream);
/* Teacher-guided mask (models_mae_learn_loss.py:744-784 generate_mask) and the visible / masked token id lists the
 * boolean-mask indexing of :298-299,649-650 produces, in one launch.  loss_pred, noise (B,L) f32; the len_loss tokens of
 * highest loss_pred are always masked, the others are ranked by noise ((value, index) order) and the first len_keep stay
 * visible.  mask (B,L) f32: 0 keep / 1 remove; vis_ids (B,len_keep), mask_ids (B,L-len_keep) int64 ascending.
 * L <= 64: one wavefront per sample; 65..512: one workgroup per sample, keys compared as order-preserving integers (guided.hip): exactly
 * len_keep tokens are visible and every id is written once whatever the inputs hold; above: GM3D_EUNSUPPORTED.
 * id_pitch = 0: the two id arrays are dense; id_pitch >= L: their row pitch in elements (vis_ids = order, mask_ids = order + len_keep
 * of one (B,id_pitch) buffer gives the [visible | masked] permutation gm3d_token_assemble_* consume). */
int gm3d_mask_select(const float *loss_pred, const float *noise, int B, int L, int len_keep, int len_loss, float *mask,
                     long long *vis_ids, long long *mask_ids, int id_pitch, gm3d_stream_t stream);
/* ... with the mask also as bytes (mask_bool (B,L) 0 / 1 or NULL): bool_masked_pos of engine_pretrain.py:100 without a conversion pass. */
int gm3d_mask_select_b(const float *loss_pred, const float *noise, int B, int L, int len_keep, int len_loss, float *mask,
                       unsigned char *mask_bool, long long *vis_ids, long long *mask_ids, int id_pitch, gm3d_stream_t stream);
/* Centre masking of plain Point-MAE pre-training (models/Point_MAE.py:268-317 _mask_center_block / _mask_center_rand) and the id
 * lists of the boolean-mask indexing behind it, in one launch: the num_mask groups with the smallest (key, index) pairs are masked.
 * mode 0 (rand): keys_or_center = noise (B,G) f32, start ignored (may be NULL).  mode 1 (block): keys_or_center = center (B,G,3)
 * f32, start (B) int32 (required); the key of group g is the squared distance to center[b, start[b]], summed x, y, z in fp32
 * without FMA, so start[b] itself is masked whenever num_mask >= 1 (a start outside 0..G-1 is clamped into it).
 * Out: mask_bool (B,G) bytes 0 / 1; order (B,id_pitch) int64, id_pitch >= G: columns [0, G-num_mask) = the visible ids ascending,
 * [G-num_mask, G) = the masked ids ascending (the [visible | masked] permutation gm3d_mask_select writes with an id_pitch and
 * gm3d_token_assemble_* consume); columns >= G are not written.  A pure function of its inputs (no atomics).
 * Limits: 1 <= G <= 512 (GM3D_EUNSUPPORTED beyond), 0 <= num_mask < G; NULL pointers, num_mask or id_pitch out of range, or mode 1
 * without start: GM3D_EINVAL.  B == 0 returns GM3D_OK launching nothing.  All checked on the host before any launch. */
int gm3d_mask_centers(const float *keys_or_center, const int *start, int mode, int B, int G, int num_mask,
                      unsigned char *mask_bool, long long *order, int id_pitch, gm3d_stream_t stream);
/* C (M,N) bf16 = A (M,K) bf16 . W (N,K)^T bf16 (+ bias (N) f32), fp32 accumulation: nn.Linear / Conv1d(k=1) forward with W the
 * weight as stored, input gradient with W the transposed weight.  Row pitches lda / ldw / ldc in elements (multiples of 8).
 * Limits: N % 128 == 0, K % 64 == 0. */
int gm3d_gemm_tn_bf16(const void *A, const void *W, const float *bias, void *C, int M, int N, int K, int lda, int ldw,
                      int ldc, gm3d_stream_t stream);
/* fc1 + bias + exact-erf GELU in the GEMM epilogue (timm Mlp: fc1 -> GELU, Point_MAE.py:92-94):
 * F (M,N) bf16 = A . W^T (no bias; optional, NULL when no backward will follow), G (M,N) bf16 = GELU(F + bias).
 * Same operand rules and limits as gm3d_gemm_tn_bf16. */
int gm3d_gemm_tn_bf16_gelu(const void *A, const void *W, const float *bias, void *F, void *G, int M, int N, int K, int lda,
                           int ldw, int ldf, int ldg, gm3d_stream_t stream);
/* Conv1d(k=1) + max over the 32 points of each group in the GEMM epilogue (mini-PointNet, models_mae_learn_loss.py:891-897):
 * rows are (group, point) with 32 points per group (M % 32 == 0).  P (M/32,N) bf16 = max_k, arg (M/32,N) u8 = its first argmax.
 * bias_after_pool = 0: C (optional) = A.W^T + bias is written and pooled (conv2: the rows feed the next layer);
 * bias_after_pool = 1: the product is pooled and the bias added to the maximum (conv4: C may be NULL -- the (M,N) product is
 * never needed again, not even by the backward, which works from `arg`); C, when given, is the product that was pooled, WITHOUT the
 * bias, on every kernel that carries this epilogue.  Ties go to the first row, as in gm3d_group_max_fwd (the values are compared
 * as the bf16 numbers C holds; -0 == +0). */
int gm3d_gemm_tn_bf16_pool(const void *A, const void *W, const float *bias, void *C, void *P, uint8_t *arg, int M, int N, int K,
                           int lda, int ldw, int ldc, int ldp, int bias_after_pool, gm3d_stream_t stream);
/* fc2 input gradient + GELU backward in the GEMM epilogue (timm Mlp backward): dF (M,N) bf16 = (dO (M,K) . Wt (N,K)^T) *
 * GELU'(F + bias) with Wt the TRANSPOSED fc2 weight (N = hidden, K = model width), F the bf16 pre-activation saved by
 * gm3d_gemm_tn_bf16_gelu; colpart (gm3d_gemm_tile_rows(M), N) f32 receives per-row-tile column sums of dF (the fc1 bias
 * gradient after gm3d_colsum_finish). */
int gm3d_gemm_tn_bf16_gelu_bwd(const void *dO, const void *Wt, const void *F, const float *bias, void *dF, float *colpart, int M,
                               int N, int K, int lda, int ldw, int ldf, int lddf, gm3d_stream_t stream);
/* LayerNorm folded into the GEMMs around it (timm Block norm1 / norm2 + the residual adds, Point-MAE_SA3D/models/Point_MAE.py:128-146):
 *   gm3d_gemm_tn_bf16_res   proj / fc2 (N = 384) whose epilogue writes the fp32 residual stream
 *                           U = res + rowscale[row / rows_per_sample] * (bf16(A.W^T) + bias) + add   (rowscale, add may be NULL)
 *                           its bf16 copy U16, and stats (3, M, 2) f32 = per row and 128-column tile (mean, sum of squared
 *                           deviations) of the fp32 values;
 *   gm3d_gemm_tn_bf16_lna   qkv / fc1 (K = 384) that reads U16 and stats, normalises (gamma, beta, eps) while staging its A operand and
 *                           computes C = LN(U).W^T + bias (G == NULL) or F (optional) / G = GELU(..) like gm3d_gemm_tn_bf16_gelu;
 *                           H (M,384) bf16, mean / rstd (M) f32 (all optional): the normalised rows and the row statistics, for the
 *                           backward pass.
 * Together they replace GEMM -> gm3d_residual_ln_fwd -> GEMM in the bf16 (throughput) mode: the statistics are those of the fp32
 * stream; the value that is normalised is the stream rounded to bf16 (an error of at most one bf16 half-ulp of |u| / sigma per
 * element, i.e. of the size of the rounding of the normalised row itself).  The fp32 parity mode keeps the three-kernel form. */
int gm3d_gemm_tn_bf16_res(const void *A, const void *W, const float *bias, const float *res, const float *rowscale, int rows_per_sample,
                          const void *add, float *U, void *U16, float *stats, int M, int N, int K, int lda, int ldw, int bm,
                          gm3d_stream_t stream);
int gm3d_gemm_tn_bf16_lna(const void *U16, const float *stats, const float *gamma, const float *beta, float eps, const void *W,
                          const float *bias, void *C, void *G, void *H, float *mean, float *rstd, int M, int N, int K, int ldu, int ldw,
                          int ldc, int ldg, gm3d_stream_t stream);
int gm3d_gemm_tile_rows(int M);
/* The same product as gm3d_gemm_tn_bf16 (bit-identical results) through a four-stage LDS-DMA ring: for long K over few output
 * tiles (fc2, the fc1 / qkv input gradients: N = 384, K = 1152 .. 1536), where one workgroup per CU has to keep more loads in
 * flight than the register-prefetch kernel does.  bm = 64 or 128: tile height.  N need only be a multiple of 8 here (a ragged
 * last column tile: the 96-wide reconstruction head increase_dim_just_network_without_feature, models_mae_learn_loss.py:169-176). */
int gm3d_gemm_tn_bf16_ring(const void *A, const void *W, const float *bias, void *C, int M, int N, int K, int lda, int ldw, int ldc,
                           int bm, gm3d_stream_t stream);
/* The TALL products of the mini-PointNet (Encoder.first_conv.3 / second_conv.0 / second_conv.3 over the B*G*k = 262,144 point rows,
 * models_mae_learn_loss.py:876-882, and their input gradients; K <= 512) with the weights STATIONARY IN REGISTERS (csrc/gemm_ws.hip):
 * persistent workgroups, 32 output columns of W per wave for the whole K, A streamed once per column block through an LDS ring
 * filled by loader waves.  HBM-bound by design (A in + C out).  Instantiated for (K -> N) = 256 -> 512, 512 -> 256, 384 -> 512,
 * 256 -> 128, 128 -> 256, 512 -> 384 (gm3d_gemm_ws_supported); results bit-identical to gm3d_gemm_tn_bf16. */
int gm3d_gemm_tn_bf16_ws(const void *A, const void *W, const float *bias, void *C, int M, int N, int K, int lda, int ldw, int ldc,
                         gm3d_stream_t stream);
/* ... with the max-pool epilogue of gm3d_gemm_tn_bf16_pool (one 32-row tile = one group of 32 points): 128 -> 256 and 512 -> 384. */
int gm3d_gemm_tn_bf16_ws_pool(const void *A, const void *W, const float *bias, void *C, void *P, unsigned char *arg, int M, int N, int K,
                              int lda, int ldw, int ldc, int ldp, int bias_after_pool, gm3d_stream_t stream);
/* ... for groups of group_rows = 16 or 32 rows (Point-M2AE's level-0 groups hold 16 points, Point-M2AE_SA3D/cfgs/config_Point_M2AE.yaml:60:
 * a 32-row tile is then two groups): P / arg (M / group_rows, N), arg counts within its group.  Also 512 -> 96 (that level's token width).
 * The weight-stationary kernel also takes ragged K (multiples of 8: 96, 192, 288 against N = 96 / 192 / 288 / 384 / 512) for the
 * hierarchical model's tall products; gm3d_gemm_ws_supported lists every (N, K). */
int gm3d_gemm_tn_bf16_ws_poolg(const void *A, const void *W, const float *bias, void *C, void *P, unsigned char *arg, int M, int N, int K,
                               int lda, int ldw, int ldc, int ldp, int bias_after_pool, int group_rows, gm3d_stream_t stream);
int gm3d_gemm_ws_supported(int N, int K, int pool);
/* second_conv.0 (256 -> 512 on the local half of the split concat, models_mae_learn_loss.py:880) together with the BatchNorm1d(512)
 * + ReLU behind it (:881), T (M / 32, N) bf16 being the per-group term (global feature @ W_g^T + bias), M % 32 == 0:
 *   _bn_apply  eval-mode BatchNorm (the EMA teacher): C = act((bf16(A.W^T) + T[row / 32]) * scale + shift), act(h) = h > 0 ? h : slope h
 *              -- bit-identical to gm3d_gemm_tn_bf16_ws followed by gm3d_bn_bcast_apply_relu, the product never reaches HBM;
 *   _bn_stats  train mode: C = bf16(A.W^T) plus per-workgroup column sums of y = C + T[row / 32] and y^2 into partial
 *              (gm3d_gemm_ws_stats_rows(M, N, K) rows x 2 N f32, every row written): what gm3d_bn_bcast_stats would read C again for.
 *              Sum the rows in order (gm3d_colsum_finish) -> the input of gm3d_bn_finalize.  Deterministic. */
int gm3d_gemm_tn_bf16_ws_bn_apply(const void *A, const void *W, const void *T, const float *scale, const float *shift, float slope, void *C,
                                  int M, int N, int K, int lda, int ldw, int ldt, int ldc, gm3d_stream_t stream);
int gm3d_gemm_tn_bf16_ws_bn_stats(const void *A, const void *W, const void *T, void *C, float *partial, int M, int N, int K, int lda,
                                  int ldw, int ldt, int ldc, gm3d_stream_t stream);
/* ... for groups of group_rows = 16 or 32 rows (T (M / group_rows, N)): the hierarchical model's level-0 groups hold 16 points */
int gm3d_gemm_tn_bf16_ws_bn_apply_g(const void *A, const void *W, const void *T, const float *scale, const float *shift, float slope, void *C,
                                    int M, int N, int K, int lda, int ldw, int ldt, int ldc, int group_rows, gm3d_stream_t stream);
int gm3d_gemm_tn_bf16_ws_bn_stats_g(const void *A, const void *W, const void *T, void *C, float *partial, int M, int N, int K, int lda,
                                    int ldw, int ldt, int ldc, int group_rows, gm3d_stream_t stream);
int gm3d_gemm_ws_stats_rows(int M, int N, int K);
/* The ring kernel with 96-column tiles (N % 96 == 0): N = 384 -- attn.proj, mlp.fc2 and the input gradients of fc1 / qkv / proj of
 * the timm Block (Point-MAE_SA3D/models/Point_MAE.py:82-125) -- as four column tiles per row block instead of three: 200 / 256
 * workgroups instead of 150 / 192 for 256 CUs, each pulling fewer operand bytes from L2.  Bit-identical results.  bm = 64 or 128. */
int gm3d_gemm_tn_bf16_ring96(const void *A, const void *W, const float *bias, void *C, int M, int N, int K, int lda, int ldw, int ldc,
                             int bm, gm3d_stream_t stream);
/* The same products for SHORT K over many tiles (csrc/gemm_dma.hip: 64- or 128-row x 192-column tiles, LDS-DMA double buffer, two
 * workgroups per CU): qkv, fc1, proj, the proj / fc2 input gradients (K = 384).  N % 192 == 0, K % 64 == 0, 16-byte aligned
 * operands; results bit-identical to gm3d_gemm_tn_bf16 / gm3d_gemm_tn_bf16_ring.  bm = 64 or 128. */
int gm3d_gemm_tn_bf16_dma(const void *A, const void *W, const float *bias, void *C, int M, int N, int K, int lda, int ldw, int ldc,
                          int bm, gm3d_stream_t stream);
/* The same kernel with the tile width chosen by the caller: bn = 128, 192 or 256 columns (N % bn == 0).  The 256-column form is
 * for the mini-PointNet convolutions over the B*G*k = 262,144 point rows and their input gradients (Encoder.second_conv,
 * models_mae_learn_loss.py:878-883: 256 -> 512, 512 -> 384 and back), which stream A once from HBM; the 128-column form for
 * first_conv.3's input gradient (256 -> 128, :876) and pos_embed.2's (384 -> 128, :104-108).  Bit-identical to the other forms. */
int gm3d_gemm_tn_bf16_dmaw(const void *A, const void *W, const float *bias, void *C, int M, int N, int K, int lda, int ldw, int ldc,
                           int bm, int bn, gm3d_stream_t stream);
/* ... with the max-pool epilogue of gm3d_gemm_tn_bf16_pool (mini-PointNet Conv1d(k=1) + max over each group's 32 points,
 * models_mae_learn_loss.py:893,897): same roundings and decisions, bm x bn tiles with bn = 128 or 192. */
int gm3d_gemm_tn_bf16_dma_pool(const void *A, const void *W, const float *bias, void *C, void *P, unsigned char *arg, int M, int N,
                               int K, int lda, int ldw, int ldc, int ldp, int bias_after_pool, int bm, int bn, gm3d_stream_t stream);
/* ... with the fc1 epilogue of gm3d_gemm_tn_bf16_gelu: F (optional) = bf16(A.W^T), G = GELU(F + bias). */
int gm3d_gemm_tn_bf16_dma_gelu(const void *A, const void *W, const float *bias, void *F, void *G, int M, int N, int K, int lda,
                               int ldw, int ldf, int ldg, int bm, gm3d_stream_t stream);
/* ... with the fc2 input-gradient epilogue of gm3d_gemm_tn_bf16_gelu_bwd: dF = bf16(dO.Wt^T) * GELU'(F + bias) (bit-identical);
 * colpart (ceil(M / bm), N) f32 = per-row-tile column sums of the fp32 products. */
int gm3d_gemm_tn_bf16_dma_gelu_bwd(const void *dO, const void *Wt, const void *F, const float *bias, void *dF, float *colpart, int M,
                                   int N, int K, int lda, int ldw, int ldf, int lddf, int bm, gm3d_stream_t stream);
/* dst (batch, cols, rows) = transposes of `batch` row-major (rows, cols) bf16 matrices that start src_batch_stride elements apart
 * (the per-block weights of one kind inside the optimizer's flat bf16 shadow).  rows, cols multiples of 8 (64 x 64 tiles, ragged edges
 * guarded per 8-element chunk: the hierarchical model's 96 / 288-wide weights). */
int gm3d_transpose_bf16_batched(const void *src, void *dst, int batch, int rows, int cols, long long src_batch_stride,
                                gm3d_stream_t stream);
/* `count` (<= 8) of those in ONE launch (the four transposed weight shadows a block stack's backward reads). */
int gm3d_transpose_bf16_multi(int count, const void *const *src, void *const *dst, const int *batch, const int *rows, const int *cols,
                              const long long *src_batch_stride, gm3d_stream_t stream);
/* Token / positional-embedding assembly around the mask (models_mae_learn_loss.py:298-300,649-658) in one pass each way.
 * order (B,L) int64 = [visible ids | masked ids], a permutation of 0..L-1 per sample (gm3d_mask_select writes exactly this when its
 * two id outputs are the halves of one (B,L) buffer).  fwd: x_vis, pos_vis (B,V,C) and pos_full (B,L,C) gathered from tokens / pos
 * (B,L,C).  bwd: dtokens, dpos (B,L,C) from dx_vis, dpos_vis (B,V,C) and dpos_full (B,L,C) (any may be NULL = zero).
 * tokens and x_vis both NULL (fwd) / dtokens NULL (bwd): positions only -- the tokens were embedded for the visible groups alone. */
int gm3d_token_assemble_fwd(const void *tokens, const void *pos, const long long *order, int B, int L, int V, int C, void *x_vis,
                            void *pos_vis, void *pos_full, int dtype, gm3d_stream_t stream);
int gm3d_token_assemble_bwd(const void *dx_vis, const void *dpos_vis, const void *dpos_full, const long long *order, int B, int L,
                            int V, int C, void *dtokens, void *dpos, int dtype, gm3d_stream_t stream);
/* out (njobs, ncols) f32 = sum over the nrows (<= 64) rows of each job of partial (njobs, nrows, ncols): the S-way row-split
 * weight-gradient partial products.  ncols % 4 == 0. */
int gm3d_sum_few_rows(const float *partial, int njobs, int nrows, long long ncols, float *out, gm3d_stream_t stream);
/* Weight-gradient GEMM, batched: out[b] (N,K) f32 = dY[b]^T . X[b] with dY[b] (R,N) and X[b] (R,K) bf16, both row-major with row
 * pitches ldy / ldx (multiples of 8) and batch strides in elements; out row pitch ldo.  This is the .grad of every Linear /
 * Conv1d(k=1) weight of the path (P/models/Point_MAE.py:82-125, P/models_mae_learn_loss.py:873-882) -- the reference leaves it
 * to autograd (one cuBLAS NT GEMM per weight).  N, K multiples of 128, R a multiple of 32 * splits, 16-byte aligned operands.
 * splits > 1: the rows are cut into `splits` ranges and split s writes its partial product at out + b*stride_o + s*stride_split
 * (gm3d_sum_few_rows adds them in order); gm3d_gemm_nt_splits suggests a value for a shape. */
int gm3d_gemm_nt_bf16(const void *dY, const void *X, float *out, int batch, int R, int N, int K, int ldy, int ldx, int ldo,
                      long long stride_y, long long stride_x, long long stride_o, int splits, long long stride_split,
                      gm3d_stream_t stream);
int gm3d_gemm_nt_splits(int batch, int R, int N, int K);
/* gm3d_gemm_nt_bf16 on 128 x 384 output tiles (512-thread workgroups, 1.5 x the flops per byte staged from L2, fragment reads
 * software-pipelined against the MFMAs; measured SLOWER on MI355X, kept as a tested variant that no product calls).  Same arguments;
 * N % 128 == 0 and K % 384 == 0 -- every weight of the transformer blocks -- else GM3D_EUNSUPPORTED.  Results are equal to
 * gm3d_gemm_nt_bf16's for equal row splits.  gm3d_gemm_nt_splits speaks for the 128 x 128 kernel only. */
int gm3d_gemm_nt_bf16_big(const void *dY, const void *X, float *out, int batch, int R, int N, int K, int ldy, int ldx, int ldo,
                          long long stride_y, long long stride_x, long long stride_o, int splits, long long stride_split,
                          gm3d_stream_t stream);
/* gm3d_gemm_nt_bf16 with the sum over the row splits INSIDE the launch (no gm3d_sum_few_rows pass): the workgroup that finishes a
 * tile's last slab adds that tile's slabs in slab order (bit-identical to the two-launch form, whatever the arrival order) and writes
 * out (batch, N, ldo; batch stride stride_o; ldo % 4 == 0).  part: (batch, splits, N, K) f32 scratch; counters: batch *
 * gm3d_gemm_nt_tiles(N, K) ints, zero on entry, zero again on exit, not shared with a launch that may run concurrently.  splits >= 2. */
int gm3d_gemm_nt_bf16_sum(const void *dY, const void *X, float *part, float *out, int *counters, int batch, int R, int N, int K, int ldy,
                          int ldx, int ldo, long long stride_y, long long stride_x, long long stride_o, int splits, gm3d_stream_t stream);
int gm3d_gemm_nt_tiles(int N, int K);
/* `count` (<= 16) problems of gm3d_gemm_nt_bf16 (128 x 128 tiles) as ONE launch + ONE slab-sum launch: the twelve batched weight
 * gradients of a step's three block stacks (timm Block qkv / proj / fc1 / fc2, P/models/Point_MAE.py:82-125) without twelve ramps and
 * partly filled last waves.  Per problem j: dY[j] (batch, R, N) bf16 rows of pitch ldy[j], X[j] (batch, R, K), out[j] (batch, N, K) f32
 * with batch stride stride_o[j], part[j] (batch, splits, N, K) f32 scratch when splits[j] > 1 (else ignored).  Bit-identical to the
 * separate launches.  The descriptors are passed by value (a captured launch keeps them). */
int gm3d_gemm_nt_bf16_multi(int count, const void *const *dY, const void *const *X, float *const *out, float *const *part, const int *batch,
                            const int *R, const int *N, const int *K, const int *ldy, const int *ldx, const long long *stride_y,
                            const long long *stride_x, const long long *stride_o, const int *splits, gm3d_stream_t stream);
/* fp32 GEMMs of the parity mode on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, fp32 accumulate): csrc/gemm_f32.hip.
 * ACCUMULATION-ORDER RULE (both kernels): every output element is one chain of MFMA accumulations over the reduction index whose
 * order depends on the reduction length alone -- units of 16 indices in ascending order; inside unit u, step j = 0..7 adds the
 * products at 16u + j and 16u + 8 + j (TN: k; NT: rows 16u + 2j and 16u + 2j + 1).  Neither the other two sizes, the tile height,
 * the grid nor the CU that ran a tile enters; no split-K in TN, no atomics anywhere: equal inputs give equal bits, and a row of a
 * TN product has the bits it would have in a product with more or fewer rows.
 *
 * gm3d_gemm_tn_f32: C (M,N) = A (M,K) . W (N,K)^T (+ bias (N), NULL = none); all fp32, row-major with row pitches lda / ldw / ldc
 * in elements.  M, N, K >= 1, ragged in all three (K = 3 works); rows need 4-byte alignment only (16-byte loads are taken when a
 * pointer and its pitch allow).  Elements of C outside the (M,N) window are not touched.  M, N or K < 1, a NULL operand, or a
 * pitch smaller than the width (negative ones included): GM3D_EINVAL; a misaligned pointer or more than 2^31 tiles:
 * GM3D_EUNSUPPORTED -- checked on the host before any launch. */
int gm3d_gemm_tn_f32(const float *A, const float *W, const float *bias, float *C, int M, int N, int K, long long lda,
                     long long ldw, long long ldc, gm3d_stream_t stream);
/* gm3d_gemm_nt_f32: out[b] (N,K) = sum over r of dY[b] (R,N)^T . X[b] (R,K), b < batch (the weight gradient); row pitches ldy /
 * ldx / ldo and batch strides in elements; accumulate != 0 adds the product to what out holds.  splits > 1 cuts the rows into
 * slabs of gm3d_gemm_nt_f32_slab_rows(R, splits) rows (a multiple of 32; the last one shorter, none empty, splits <= 64): each slab
 * is a chain of its own, as if computed by a splits = 1 call on its rows, written to part (batch, splits, N, K) f32, and a second
 * launch inside the call adds the slabs in ascending slab order (then adds out when accumulate).  gm3d_gemm_nt_f32_splits is the
 * split the package uses: a pure function of (batch, R, N, K).  Errors as for gm3d_gemm_tn_f32; an empty slab or splits > 1 without
 * part: GM3D_EINVAL. */
int gm3d_gemm_nt_f32(const float *dY, const float *X, float *out, float *part, int batch, int R, int N, int K, long long ldy,
                     long long ldx, long long ldo, long long stride_y, long long stride_x, long long stride_o, int splits,
                     int accumulate, gm3d_stream_t stream);
int gm3d_gemm_nt_f32_splits(int batch, int R, int N, int K);
int gm3d_gemm_nt_f32_slab_rows(int R, int splits);
/* Masked multi-head attention of the hierarchical (Point-M2AE) encoder blocks -- SURVEY.md 8f.4; the reference ships only the
 * hyper-parameters (Point-M2AE_SA3D/cfgs/config_Point_M2AE.yaml:57-99: dims 96/192/384, 6 heads, local_radius 0.32/0.64/1.28).
 * qkv (B,T,3,H,HD) as the qkv Linear emits it, HD in {16,32,64}, T <= 512; mask (B,T,ceil(T/32)) uint32 bitset, bit (j&31) of
 * word j>>5 of row i set = query i must not attend to key j (NULL: no mask); the mask must be symmetric.  out (B,T,H*HD), lse
 * (B,H,T) f32 (0 for a query with no allowed key, whose output and gradients are zero).  dtype GM3D_BF16: flash-style MFMA
 * kernels; GM3D_F32: exact fp32 kernels (parity mode).  bf16 keeps the head in LDS: the forward needs (2*32*ceil(T/32) + 128) *
 * (2 HD + 16) bytes, the backward 4*32*ceil(T/32) * (2 HD + 16) + 8*32*ceil(T/32), at most 160 KiB -- i.e. T <= 512 for HD = 16,
 * T <= 512 forward / T <= 480 backward for HD = 32 and T <= 480 forward / T <= 256 backward for HD = 64 (GM3D_EUNSUPPORTED
 * beyond).  With mask = NULL and HD = 64 these are also
 * the attention of the Point-MAE models for more than 128 tokens (cfgs/config_3.yaml: 256 groups). */
/* Deterministic backward of a row gather with repeated indices (the hierarchical model's member / 3-NN token gathers: PyTorch's
 * gather backward scatter-adds with colliding float atomics).  gm3d_gather_inverse: idx (B,J) int64 with values in [0,S) -> the
 * inverse lists in CSR form, off (B,S+1) int32 and list (B,J) int32, every list in ascending j (S <= 4096, J <= 16384);
 * gm3d_gather_rows_bwd: dx (B,S,C) = sum over each source's list of dy (B,J,C) rows, in list order (fp32 accumulation, C % 8 == 0). */
int gm3d_gather_inverse(const long long *idx, int B, int J, int S, int *off, int *list, gm3d_stream_t stream);
int gm3d_gather_rows_bwd(const void *dy, const int *off, const int *list, void *dx, int B, int J, int S, int C, int dtype,
                         gm3d_stream_t stream);
/* The bitset mask of one level of the hierarchical encoder: bits (B,G,ceil(G/32)), bit j of row i set iff token i or token j is
 * not visible (vis (B,G) bytes, NULL = all visible) or their centres (B,G,3) are >= radius apart (radius <= 0: no radius test).
 * G <= 8192, B <= 65535 (GM3D_EUNSUPPORTED beyond). */
int gm3d_radius_mask_bits(const float *center, const unsigned char *vis, float radius, int B, int G, unsigned *bits,
                          gm3d_stream_t stream);
/* ... with the flags' sense selectable: flags_are_masked != 0 -> a non-zero byte means NOT visible (the multi-scale masks as they are) */
int gm3d_radius_mask_bits_m(const float *center, const unsigned char *flags, int flags_are_masked, float radius, int B, int G,
                            unsigned *bits, gm3d_stream_t stream);
/* Visible-first token order of one masked level (the student's pass: multi-scale masking at ratio 0.8,
 * Point-M2AE_SA3D/cfgs/config_Point_M2AE.yaml:57-99; gm3d_amd/point_m2ae.py).  masked (B,T) bytes (non-zero = masked), T <= 1024,
 * 1 <= Tc <= T (a static bound on the visible count, or T):  perm_c (B,Tc) int32 = token at compact slot j (visible tokens in
 * ascending order, then masked ones as filler); perm_v (B,Tc) = the same with -1 in filler slots; inv_v (B,T) = slot of token t
 * if visible and below Tc, else -1; inv_m (B,T) = t if token t is masked, else -1; vis_c (B,Tc) bytes = 1 in slots holding a
 * visible token; *overflow set to 1 if a cloud has
 * more than Tc visible tokens (the caller's bound was wrong; never cleared here). */
int gm3d_partition_visible(const unsigned char *masked, int B, int T, int Tc, int *perm_c, int *perm_v, int *inv_v, int *inv_m,
                           unsigned char *vis_c, int *overflow, gm3d_stream_t stream);
/* Multi-scale masking one level down (gm3d_amd/point_m2ae.py back_project): masked_f (B,Gf) bytes = 1 unless some VISIBLE group of the
 * coarser level (masked_c (B,Gc) bytes, 0 = visible) lists the finer group among its k members (member (B,Gc,k) int64).  Gf <= 8192. */
int gm3d_back_project(const unsigned char *masked_c, const long long *member, int B, int Gc, int k, int Gf, unsigned char *masked_f,
                      gm3d_stream_t stream);
/* Token propagation of the hierarchical decoder (3-NN inverse-squared-distance interpolation, PointNet++ style; configuration
 * Point-M2AE_SA3D/cfgs/config_Point_M2AE.yaml:88-99): out (B,N,C1+C2) = [fine (B,N,C1) | sum_j w[b][n][j] * coarse[b][idx[b][n][j]]],
 * coarse (B,S,C2), idx (B,N,3) int64, w (B,N,3) f32; C1, C2 % 8 == 0 (C1 = 0: no fine part).  Backward of the interpolated half:
 * gm3d_gather_inverse over idx viewed as (B,3N), then gm3d_gather_rows_bwd_w: dx (B,S,C) = sum over each source's list, in list order,
 * of w[b][j] * dy[b][j / refs_per_row][col0 : col0 + C] (dy rows of pitch ldy). */
int gm3d_interp3_fwd(const void *coarse, const long long *idx, const float *w, const void *fine, void *out, int B, int N, int S, int C1,
                     int C2, int dtype, gm3d_stream_t stream);
int gm3d_gather_rows_bwd_w(const void *dy, int ldy, int col0, int refs_per_row, const float *w, const int *off, const int *list, void *dx,
                           int B, int J, int S, int C, int dtype, gm3d_stream_t stream);
/* out[row] = flag[row] (xor invert) ? alt[row] : a[row] over `rows` rows of C elements (elem_bytes 2 / 4); a NULL / alt NULL: zeros;
 * alt_bcast: alt is one row (C) for every row (the decoder's mask token).  gm3d_amd/point_m2ae.py's per-token choices and their backward. */
int gm3d_where_rows(const unsigned char *flag, int invert, const void *a, const void *alt, int alt_bcast, void *out, long long rows, int C,
                    int elem_bytes, gm3d_stream_t stream);
/* out (B,J,C) = a[b][idx[b][j]] for int64 idx (B,J) with repeats (the forward of the member gathers; backward: gm3d_gather_rows_bwd). */
int gm3d_take_rows(const void *a, const long long *idx, void *out, int B, int S, int J, int C, int elem_bytes, gm3d_stream_t stream);
/* out (B,T,C) row by row: idx[b][t] >= 0 -> a[b][idx[b][t]] (a is (B,Ta,C)), else alt[b][t] (alt (B,T,C)) or zeros (alt NULL).
 * elem_bytes 2 or 4.  Gather into / scatter out of the compact order above, forward and backward (indices without repeats). */
int gm3d_select_rows(const void *a, const int *idx, const void *alt, void *out, int B, int Ta, int T, int C, int elem_bytes,
                     gm3d_stream_t stream);
int gm3d_attention_masked_fwd(const void *qkv, const unsigned *mask, void *out, float *lse, int B, int T, int H, int HD, float scale,
                              int dtype, gm3d_stream_t stream);
int gm3d_attention_masked_bwd(const void *qkv, const unsigned *mask, const void *out, const void *dout, const float *lse, void *dqkv,
                              int B, int T, int H, int HD, float scale, int dtype, gm3d_stream_t stream);
/* The same operator for 513 <= T <= 2048 (gm3d_amd/csrc/attention_long.hip): arguments, layouts, mask semantics and rounding points
 * of gm3d_attention_masked_fwd/bwd -- qkv (B,T,3,H,HD), HD in {16,32,64}; mask (B,T,ceil(T/32)) symmetric bitset or NULL; out
 * (B,T,H*HD); lse (B,H,T) f32, 0 for a query with no allowed key, whose output row and gradient rows are zero; dqkv shaped like
 * qkv; B * H <= (2^31 - 1) / 4.  T <= 512 and T > 2048 are GM3D_EUNSUPPORTED (T <= 512 belongs to gm3d_attention_masked_*: one
 * owner per range), as is any other HD; a dtype other than GM3D_F32 / GM3D_BF16 or a NULL tensor is GM3D_EINVAL; all of it is
 * decided on the host before any launch, and B = 0 returns GM3D_OK after these checks.  GM3D_BF16: flash-style MFMA kernels that
 * stream the head through LDS in chunks of 64 rows, two buffers (forward: K, V and 256 query rows, at most 72 KiB; backward: one
 * launch, Q, K, V, dO, lse and delta = rowsum(dO * O) of a chunk, at most 73 KiB); every row of dQ, dK and dV is written once by
 * its one owner -- no atomics, no zero-fill, equal bits on every run.  GM3D_F32: the same kernels on the exact-fp32 MFMA (parity
 * mode; fp32 images, forward at most 65 KiB, backward at most 131 KiB). */
int gm3d_attention_long_fwd(const void *qkv, const unsigned *mask, void *out, float *lse, int B, int T, int H, int HD, float scale,
                            int dtype, gm3d_stream_t stream);
int gm3d_attention_long_bwd(const void *qkv, const unsigned *mask, const void *out, const void *dout, const float *lse, void *dqkv,
                            int B, int T, int H, int HD, float scale, int dtype, gm3d_stream_t stream);

/* ---- Voting evaluation of the fine-tuned classifier (gm3d_amd/csrc/vote.hip) --------------------------------------------
 * Replaces the per-vote loop of validate_vote / test_vote (Point-MAE_SA3D/tools/runner_finetune.py:293-309 and :421-437):
 * V times fps_idx_raw[:, np.random.choice(point_all, npoints, False)], gather_operation, test_transforms
 * (PointcloudScaleAndTranslate, datasets/data_transforms.py:27-35) and base_model(points), then the vote mean and argmax.
 *
 * gm3d_vote_sample: points (B,N0,3) f32, fps_idx (B,point_all) int32, subsets (V,npoints) int64, scale / shift (V,B,3) f32 ->
 * out (V*B,npoints,3) f32, vote-major (row v*B+b) = points[b][fps_idx[b][subsets[v][j]]] * scale[v][b] + shift[v][b], product and
 * sum rounded separately (bit-equal to the torch op chain).  An index out of range yields a NaN point.
 * Limits: npoints <= point_all <= N0.
 *
 * gm3d_cls_tail_vote: the eval-mode cls_head_finetune (P/models/Point_MAE.py:489-499, :575-577) on the stack output after norm_p,
 * x (V*B,T,C) in `dtype` (16-byte aligned), for all V votes of every cloud, plus the vote mean and its argmax:
 * feature = [x[:,0] ; max over tokens 1..T-1], Linear W1 (256,2C) b1, BatchNorm (g1, be1, running rm1 / rv1, eps), ReLU,
 * Linear W2 (256,256) b2, BatchNorm (g2, be2, rm2, rv2, eps), ReLU, Linear W3 (cls_dim,256) b3 (Dropout = identity); all f32,
 * the running statistics are read on every call.  mean (B,cls_dim) f32 = sum of the votes in order v = 0..V-1, then / V;
 * pred (B) int64 = argmax (ties -> lowest index); *correct += number of b with pred[b] == labels[b] (int64, no float atomics);
 * votes (V,B,cls_dim) f32 per-vote logits, or NULL.
 * Limits: C == 384, T >= 2, 1 <= cls_dim <= 256, 1 <= V <= 16. */
int gm3d_vote_sample(const float *points, const int32_t *fps_idx, const long long *subsets, const float *scale, const float *shift,
                     int B, int N0, int point_all, int npoints, int V, float *out, gm3d_stream_t stream);
int gm3d_cls_tail_vote(const void *x, int V, int B, int T, int C, const float *W1, const float *b1, const float *g1, const float *be1,
                       const float *rm1, const float *rv1, const float *W2, const float *b2, const float *g2, const float *be2,
                       const float *rm2, const float *rv2, const float *W3, const float *b3, int cls_dim, float eps,
                       const long long *labels, float *mean, long long *pred, long long *correct, float *votes, int dtype,
                       gm3d_stream_t stream);

/* ---- Classification tail of the Point-M2AE classifiers (gm3d_amd/csrc/cls_tail.hip, gm3d_amd/point_m2ae_cls.py) ---------------------
 * gm3d_cls_tail_fwd: x (B,T,C) in `dtype` -> pooled feature feat (B,F) f32: mode 0 = mean over the tokens + max over the tokens (F = C),
 * mode 1 = [mean ; max] (F = 2C); argmax (B,C) int32 = the token of each channel's maximum (ties -> lowest index, a NaN wins);
 * Linear W1 (256,F) b1 -> h[0] (B,256); BatchNorm g1 / be1 -> ReLU -> times drop[0] (B,256); Linear W2 (256,256) b2 -> h[1];
 * BatchNorm g2 / be2 -> ReLU -> times drop[1]; Linear W3 (cls_dim,256) b3 -> logits (B,cls_dim) f32.  training != 0: BatchNorm with
 * the batch mean and biased variance, running statistics rm <- (1 - momentum) rm + momentum mean, rv <- (1 - momentum) rv +
 * momentum var B / (B - 1), *nbt += 1; training == 0: the running statistics, no dropout, nothing written to rm / rv / nbt.
 * drop (2,B,256) f32 dropout factors (0 or 1 / (1 - p)) or NULL (factor 1).  stats (4,256) f32 receives the mean and 1 / sqrt(var + eps)
 * of both BatchNorms; feat, argmax, h and stats are what gm3d_cls_tail_bwd reads.  labels (B) int64 or NULL: loss (1) f32 = mean
 * cross-entropy of the logits (a label outside [0, cls_dim) gives NaN).  Two launches.
 *
 * gm3d_cls_tail_bwd: the gradients of the same computation from dlogits (B,cls_dim) f32 and / or dloss (1) f32 (the cross-entropy's;
 * needs labels), either may be NULL.  dx (B,T,C) in `dtype`: dmean / T on every token + dmax on the argmax token.  dW1 (256,F), db1,
 * dg1, dbe1, dW2 (256,256), db2, dg2, dbe2, dW3 (cls_dim,256), db3 in f32, every sum in a fixed order without float atomics (a graph
 * replay equals an eager call bit for bit).  ws: 5 * B * 256 f32 of scratch.  `training` and `drop` as in the forward.  Two launches.
 *
 * Limits: C == 384, 1 <= T <= 512, B <= 128 (B >= 2 in training), 1 <= cls_dim <= 256, mode 0 or 1; W2 and W3 16-byte aligned.
 * B == 0 returns GM3D_OK after the shape checks, launching nothing. */
int gm3d_cls_tail_fwd(const void *x, int B, int T, int C, int mode, const float *W1, const float *b1, const float *g1, const float *be1,
                      const float *W2, const float *b2, const float *g2, const float *be2, const float *W3, const float *b3, int cls_dim,
                      float *rm1, float *rv1, long long *nbt1, float *rm2, float *rv2, long long *nbt2, float eps, float momentum,
                      int training, const float *drop, const long long *labels, float *feat, int *argmax, float *h, float *stats,
                      float *logits, float *loss, int dtype, gm3d_stream_t stream);
int gm3d_cls_tail_bwd(int B, int T, int C, int mode, const float *W1, const float *g1, const float *be1, const float *W2, const float *g2,
                      const float *be2, const float *W3, int cls_dim, int training, const float *drop, const long long *labels,
                      const float *feat, const int *argmax, const float *h, const float *stats, const float *logits,
                      const float *dlogits, const float *dloss, float *ws, void *dx, float *dW1, float *db1, float *dg1, float *dbe1,
                      float *dW2, float *db2, float *dg2, float *dbe2, float *dW3, float *db3, int dtype, gm3d_stream_t stream);

/* ---- Voting evaluation of the Point-M2AE classifiers (gm3d_amd/csrc/vote.hip) ------------------------------------------------------
 * gm3d_cls_tail_vote_pool: gm3d_cls_tail_vote with the Point-M2AE classifiers' pooling.  x (V*B,T,C) in `dtype` (16-byte aligned),
 * the final-norm tokens of all V votes, vote-major (row v*B+b); feature = the pooling of gm3d_cls_tail_fwd, bit for bit: mode 0 =
 * mean over the tokens + max over the tokens (F = C), mode 1 = [mean ; max] (F = 2C), the mean a sum over t = 0..T-1 in order
 * then / T, the max the first maximum (a NaN wins).  The eval-mode head Linear W1 (256,F) b1, BatchNorm (g1, be1, running rm1 / rv1,
 * eps), ReLU, Linear W2 (256,256) b2, BatchNorm (g2, be2, rm2, rv2, eps), ReLU, Linear W3 (cls_dim,256) b3 (Dropout = identity);
 * all f32, the running statistics read on every call.  mean (B,cls_dim) f32 = sum of the votes in order v = 0..V-1, then / V;
 * pred (B) int64 = argmax (ties -> lowest index, a NaN wins); *correct += number of b with pred[b] == labels[b] (int64, no float
 * atomics); votes (V,B,cls_dim) f32 per-vote logits, or NULL; feat (V*B,F) f32 the pooled features, or NULL.  One launch.
 * Limits: C == 384, 1 <= T <= 512, 1 <= V <= 16, 1 <= cls_dim <= 256, mode 0 or 1; LDS (V*F + V*256) * 4 bytes, 64 KiB at V = 16,
 * F = 768.  B == 0 returns GM3D_OK after the shape checks, launching nothing. */
int gm3d_cls_tail_vote_pool(const void *x, int V, int B, int T, int C, int mode, const float *W1, const float *b1, const float *g1,
                            const float *be1, const float *rm1, const float *rv1, const float *W2, const float *b2, const float *g2,
                            const float *be2, const float *rm2, const float *rv2, const float *W3, const float *b3, int cls_dim,
                            float eps, const long long *labels, float *mean, long long *pred, long long *correct, float *votes,
                            float *feat, int dtype, gm3d_stream_t stream);

/* ---- Linear-SVM validation (gm3d_amd/csrc/svm.hip) -------------------------------------------------------------------------------
 * The solver of sklearn's SVC(C, kernel="linear") (libsvm C-SVC, one-vs-one) behind the pretraining validation,
 * without libsvm's shrinking (it does not move the fixed point).  Training rows are grouped by class: class_start is a HOST array of
 * ncls+1 ints, class_start[0] = 0 < class_start[1] < ... < class_start[ncls] = n (every class non-empty); class c holds the rows
 * [class_start[c], class_start[c+1]).  Pairs p = 0..P-1, P = ncls(ncls-1)/2, run in the order (0,1), (0,2), ..., (1,2), ...; pair
 * (s,t) sees the rows of s with y = +1, then the rows of t with y = -1, in row order, and its alpha sits in the concatenated alpha
 * array at the sum of n_s + n_t over the pairs before it ((ncls-1)*n doubles in all).
 * Limits: n <= 16384, d <= 1024, 2 <= ncls <= 64, n_s + n_t <= 4096 for every pair (GM3D_EUNSUPPORTED beyond, checked on the host).
 *
 * gm3d_svm_gram: X (n,d) f32 -> K (n,n) f64 = X X^T: f32 products are exact in f64, the sums run on v_mfma_f64_16x16x4_f64 in a
 *   fixed order; only the lower triangle is computed and it is mirrored, so K is exactly symmetric.
 * gm3d_svm_smo: one workgroup per pair, alpha / gradient / diag(K) in LDS as f64.  alpha = 0, G = -1; i = argmax over I_up of -yG
 *   (Gmax); j = argmin over k in I_low with b = Gmax + y_k G_k > 0 of -b^2/a, a = K_ii + K_kk - 2 K_ik (1e-12 when a <= 0); stop when
 *   Gmax + max over I_low of yG < tol; libsvm's clipped two-variable update; G_k += Q_ki dalpha_i + Q_kj dalpha_j, Q = yy^T K.  Ties
 *   go to the lowest row.  I_up = {y=+1, alpha<C} u {y=-1, alpha>0}, I_low = {y=+1, alpha>0} u {y=-1, alpha<C}.  rho (P) f64 by
 *   libsvm's rule (mean of yG over the free alpha, else the midpoint of its bounds), iters (P) int32 the updates made.  max_iter <= 0
 *   means libsvm's cap max(10^7, 100 (n_s + n_t)); every pair that reaches the cap adds 1 to *capped (device int, not zeroed here).
 *   LDS 24 bytes per row of the largest pair.  Bitwise reproducible.
 * gm3d_svm_weights: w (P,d) f64, w[p] = sum over the pair's rows in order of y alpha X[row] (X the same grouped f32 rows).
 * gm3d_svm_predict: X (m,d) f32 test rows -> pred (m) int64 = the first class with the most one-vs-one votes (pair (s,t) votes for s
 *   when w_p . x - rho_p > 0, else for t); labels (m) int64 class indices, or NULL: *correct += the rows with pred == label (int64,
 *   no float atomics).  One launch; m == 0 returns GM3D_OK launching nothing. */
int gm3d_svm_gram(const float *X, int n, int d, double *K, gm3d_stream_t stream);
int gm3d_svm_smo(const double *K, int n, int ncls, const int *class_start, double C, double tol, long long max_iter, double *alpha,
                 double *rho, int *iters, int *capped, gm3d_stream_t stream);
int gm3d_svm_weights(const float *X, int n, int d, int ncls, const int *class_start, const double *alpha, double *w,
                     gm3d_stream_t stream);
int gm3d_svm_predict(const float *X, int m, int d, int ncls, const double *w, const double *rho, const long long *labels,
                     long long *pred, long long *correct, gm3d_stream_t stream);

/* ---- Weighted k-NN probe of pretrained features (gm3d_amd/csrc/knn_probe.hip) ------------------------------------------------------
 * The temperature-weighted k-NN classifier of Point-MAE_SA3D/main_knn.py:153-198 (knn_classifier) on L2-normalised features, the
 * solver-free second quality signal beside the linear SVM.  Xn (n,d) f32 training rows, Qn (m,d) f32 test rows, both 16-byte
 * aligned; the similarity of a pair is their dot product on v_mfma_f32_32x32x2_f32 (exact fp32: one fmaf per column onto the
 * running sum) in a fixed column order: 16 columns at a time, column 16u + j then column 16u + 8 + j for j = 0..7.  Operands whose
 * products and partial sums are exactly representable give exact similarities.  The (m,n) similarity matrix is never stored: a
 * workgroup of 512 threads owns 32 test rows and recomputes their similarities in four 8-bit radix-select passes over the
 * order-preserving integer keys of the similarities (-0 == +0, NaN above +inf) and one collecting pass.  Selection is exact.
 * Neighbours are ordered by the strict total order (similarity descending, training row ascending).  Stream-ordered, no host
 * synchronisation, no global state, no float atomics; every output is bitwise reproducible.
 * LDS: 98,688 bytes dynamic (survivor keys and rows 2 x 32 x 257 x 4, histogram / class scores 32 x 257 x 4) + 1.5 KiB static;
 * __launch_bounds__(512); one workgroup per CU.  Measured at 9,843 / 2,468 x 384, 40 classes: 4.3 ms (k = 20), 4.6 ms (k = 200) per
 * launch; MFMA utilisation and the cost of the LDS atomics: not measured.
 * Limits (GM3D_EINVAL for n < 1, m < 0, d < 1, k < 1, k > n, ncls < 1, T <= 0 or NaN, a NULL or misaligned required pointer;
 * GM3D_EUNSUPPORTED beyond the kernel's range; all checked on the host before any launch):
 *   1 <= n <= 16384, 8 <= d <= 1024, d % 8 == 0, 1 <= k <= min(n, 256), 2 <= ncls <= 64, T > 0, m >= 0.
 * m == 0 returns GM3D_OK after the shape checks, launching nothing.
 *
 * gm3d_knn_probe_normalize: Y[i] = X[i] / max(||X[i]||_2, 1e-12) (F.normalize(p=2, dim=1)), fp32; the row sum of squares is taken by
 *   one wave, lane l over the columns l, l + 64, ... in order, then a fixed butterfly.  Any n >= 0, d >= 1; Y may be X.
 * gm3d_knn_probe_neighbours: idx (m,k) int32, sim (m,k) f32 = the k training rows of largest similarity per test row, in the order
 *   above (sim holds +0 for a similarity of -0).
 * gm3d_knn_probe_classify: the same selection, then in the same launch: the weight of a neighbour is expf(sim / T) (an fp32
 *   division, then expf, the reference's div_(T).exp_()); the score of class c is the sum of the weights of the neighbours with
 *   train_labels[row] == c, added in neighbour-rank order in fp32 (a label outside 0..ncls-1 adds to no class); classes are ranked
 *   by (score descending, class ascending), so classes without a neighbour rank by id after the voted ones.  top5 (m,5) int64 = the
 *   first five classes (-1 beyond ncls); probs (m,ncls) f32 = the scores, or NULL; test_labels (m) int64 or NULL: correct[0] += the
 *   rows whose first class is the label, correct[1] += the rows with the label among the first min(5, k, ncls) classes (int64
 *   atomics; with test_labels NULL correct is not touched and may be NULL). */
int gm3d_knn_probe_normalize(const float *X, int n, int d, float *Y, gm3d_stream_t stream);
int gm3d_knn_probe_neighbours(const float *Xn, const float *Qn, int n, int m, int d, int k, int *idx, float *sim,
                              gm3d_stream_t stream);
int gm3d_knn_probe_classify(const float *Xn, const float *Qn, int n, int m, int d, int k, const long long *train_labels, int ncls,
                            float T, const long long *test_labels, long long *top5, float *probs, long long *correct,
                            gm3d_stream_t stream);

/* ---- Batch assembly from a device-resident dataset (gm3d_amd/csrc/dataset.hip) -------------------------------------------------------
 * gm3d_sample_normalize: what the reference's datasets do per sample on the host, for a whole batch in one launch:
 *   Point-MAE_SA3D/datasets/ShapeNet55Dataset.py:45-67 (random_sample: shuffle + [:num]; pc_norm), ModelNetDataset.py:138-145 and
 *   ScanObjectNNDataset.py:33-44 (the train split's shuffle of all points), with the collate and the host-to-device copy behind them.
 * data (M,N0,3) f32 the resident dataset; cloud_idx (B) int64 the batch's clouds, any order, repeats allowed (an index outside
 * 0..M-1 is clamped into it); keys (B,N0) f32 one draw per point, made by the caller (the kernel draws nothing); out (B,num,3) f32;
 * idx_out (B,num) int32 the selected point indices, or NULL.
 * Order: row j of cloud b is the point i with the j-th smallest (ordered_key(keys[b,i]), i), ordered_key the order-preserving integer
 * of gm3d_mask_centers (-0 == +0, NaN above +inf).  The order is strict and total: idx_out[b] always holds num distinct indices in
 * 0..N0-1, all keys equal give data[cloud_idx[b], :num], and every output is a pure function of the inputs (an in-LDS bitonic sort of
 * packed 64-bit pairs, N0 padded to a power of two with maximal pairs; no atomics).  Independent uniform keys give a uniformly random
 * ordered subset, with num == N0 a uniformly random permutation.
 * normalize = 0: rows are bit copies of the source points.  normalize = 1: pc_norm of the selected points in fp32 -- minus their mean
 * (a workgroup tree sum / num), divided (IEEE) by the square root of the largest squared norm (x*x + y*y) + z*z, no FMA; selected
 * points that all coincide give 0 / 0 like the reference.
 * One workgroup of min(1024, max(64, P/2)) threads per cloud, P = N0 rounded up to a power of two; LDS 8 P bytes dynamic (64 KiB at
 * N0 = 8192) + 64 bytes static.
 * Limits, checked on the host before any launch: GM3D_EINVAL for a NULL data / cloud_idx / keys / out, B < 1, M < 1, N0 < 1, num < 1,
 * num > N0, normalize not 0 or 1; GM3D_EUNSUPPORTED for N0 > 8192. */
int gm3d_sample_normalize(const float *data, const long long *cloud_idx, const float *keys, int B, int M, int N0, int num,
                          int normalize, float *out, int *idx_out, gm3d_stream_t stream);

/* ---- Point-cloud augmentations as one launch (gm3d_amd/csrc/augment.hip) -------------------------------------------------------------
 * gm3d_augment: an ordered program of 1..GM3D_AUG_MAX_OPS transforms of Point-MAE_SA3D/datasets/data_transforms.py applied IN PLACE to
 * pc (B,N,3) f32 (the one entry point that writes its input: the reference's transforms do).  One workgroup per cloud, one launch.
 * The program is read from host memory at call time (ops (nops) int, params (nops,3) f32) and handed to the kernel by value: no
 * device allocation, no copy, no synchronisation; a captured graph bakes the program in and replays it on whatever the draw tensors
 * hold.  The kernel draws nothing.
 *
 *   op (ops[j] & 0xff)         draws/cloud  params[j]        what it does to every point (x, y, z) of cloud b
 *   GM3D_AUG_ROTATE          :6-18     1    -                angle = 2 pi u; c, s = cos, sin in double, rounded to f32;
 *                                                            x' = x c - z s, y' = y, z' = x s + z c
 *   GM3D_AUG_SCALE           :51-63    3    lo, span         p * (u * span + lo)
 *   GM3D_AUG_TRANSLATE       :65-76    3    t                p + (u * 2 - 1) * t
 *   GM3D_AUG_SCALE_TRANSLATE :20-35    3+3  lo, span, t      p * (u * span + lo) + (u' * 2 - 1) * t: bit-identical to gm3d_scale_translate
 *   GM3D_AUG_JITTER          :37-49    0    std, clip        p + clamp(point_z[b,i] * std, -clip, clip)
 *   GM3D_AUG_DROPOUT         :79-94    1    max_ratio        point i becomes point 0 (as it stands when the op starts) iff
 *                                                            (double)point_u[b,i] <= (double)u * (double)max_ratio
 *   GM3D_AUG_FLIP            :96-118   3    upright axis     draws [gate, lower axis, higher axis] (the two axes that are not upright, in
 *                            (0, 1 or 2)                     ascending order): if (double)gate < 0.95, each of them whose (double)draw < 0.5
 *                                                            becomes max over the cloud's points - coordinate
 * Every product and sum is rounded separately in f32 (no FMA), the flip's maximum is exact (NaN coordinates are skipped by it).
 * ops[j] | GM3D_AUG_FINAL (parity tests): the op's draws hold the final quantity instead of the uniform -- SCALE: the scales;
 * TRANSLATE: the shifts; SCALE_TRANSLATE: scales, then shifts; DROPOUT: the ratio point_u is compared with; JITTER: point_z is the noise
 * before the clamp (std is not applied).  ROTATE and FLIP take their uniforms either way.  Same kernel code: the flag skips one map.
 *
 * cloud_u holds B * D f32, D the sum of the draws/cloud over the program (what one torch.rand(B, D) makes), as one block per draw
 * group in program order: a group of cnt = 1 or 3 draws that starts at column c (the sum of the counts in front of it) is the
 * (B,cnt) row-major block at cloud_u + B * c; SCALE_TRANSLATE is two groups, scales then shifts -- alone it is gm3d_scale_translate's
 * (2,B,3).  point_u (B,N) f32 uniforms: needed by DROPOUT; point_z (B,N,3) f32 normals: needed by JITTER; either may be NULL
 * otherwise, and cloud_u when D = 0.
 * Limits, checked on the host before any launch: GM3D_EINVAL for a NULL pc / ops / params, N < 1, B < 0, nops outside
 * 1..GM3D_AUG_MAX_OPS, an unknown op code or flag bit, an upright axis other than 0, 1, 2, more than one DROPOUT or more than one
 * JITTER in a program (there is one point_u and one point_z), or a missing draw tensor the program needs.  B = 0 returns GM3D_OK
 * without a launch.  No limit on N: min(1024, N rounded up to 64) threads per cloud, 408 bytes of LDS. */
enum {
    GM3D_AUG_NONE = 0,
    GM3D_AUG_ROTATE = 1,
    GM3D_AUG_SCALE = 2,
    GM3D_AUG_TRANSLATE = 3,
    GM3D_AUG_SCALE_TRANSLATE = 4,
    GM3D_AUG_JITTER = 5,
    GM3D_AUG_DROPOUT = 6,
    GM3D_AUG_FLIP = 7,
    GM3D_AUG_FINAL = 0x100,
    GM3D_AUG_MAX_OPS = 8
};
int gm3d_augment(float *pc, int B, int N, int nops, const int *ops, const float *params, const float *cloud_u,
                 const float *point_u, const float *point_z, gm3d_stream_t stream);

/* ---- Linear probe of pretrained features (gm3d_amd/csrc/linprobe.hip) ----------------------------------------------------------------
 * The linear probe of Point-MAE_SA3D/main_linprob.py:219-263 on cached features: BatchNorm1d(affine=False, eps=1e-6) -> Linear,
 * cross-entropy, SGD(momentum, weight decay 0), all in fp32 (the reference's fp16 autocast is not reproduced).
 * X (n,d) f32 training features, y (n) int64 class indices (a label outside 0..ncls-1 is clamped into it: the caller checks the
 * range), order (T*batch) int32 the training rows of iteration t at order[t*batch .. (t+1)*batch) (clamped into 0..n-1), lr (T) f32
 * the rate of every iteration, W (ncls,d), mom_w (ncls,d), mom_b (ncls), running_mean (d), running_var (d), losses (T), and bias2
 * (2,ncls): slot t & 1 holds the bias BEFORE iteration t, so after T iterations the bias is bias2[T & 1].
 * One training iteration on the batch rows B (|B| = batch), per column j and class c:
 *   mean_j = sum_i x_ij / batch, var_j = sum_i (x_ij - mean_j)^2 / batch (two passes), x^_ij = (x_ij - mean_j) / sqrt(var_j + 1e-6),
 *   running_mean_j = 0.9 running_mean_j + 0.1 mean_j, running_var_j = 0.9 running_var_j + 0.1 var_j batch / (batch - 1),
 *   z = x^ W^T + b, losses[t] = mean_i (log sum_c exp(z_ic - max_i) + max_i - z_i[y_i]),
 *   dz = (softmax(z) - onehot(y)) / batch, dW = dz^T x^, db = sum_i dz_i (nothing flows into the BatchNorm),
 *   mu = momentum mu + g, p = p - lr[t] mu for W and b alike (torch.optim.SGD; mu starts at 0, so mu = g on the first step).
 * gm3d_linprobe_train runs the iterations t_begin .. t_end - 1 in t_end - t_begin + 1 launches of ceil(d / 16) workgroups, one per
 *   16 columns: launch K(t) finishes iteration t-1 (sums the partial logits of all column slices in slice order plus the bias,
 *   softmax, dz, dW / momentum / weights of its slice; workgroup 0: db, bias, loss) and starts iteration t (gather, statistics,
 *   running statistics, partial logits of its slice with the weights just updated); the first launch only starts, the last only
 *   finishes.  A workgroup never waits for another inside a launch; no cooperative launch, no float atomics; stream-ordered, no host
 *   synchronisation.  Every reduction runs in an order fixed by the shapes (linprobe.hip lists them): equal inputs give equal bits.
 *   Scratch: xhat (batch,d) f32 16-byte aligned, part (2 * gm3d_linprobe_slices(d) * ncls * batch) f32; both are written before they
 *   are read and must stay untouched between two calls that continue one fit.  t_end == t_begin launches nothing.
 *   LDS: 94,720 bytes dynamic, none static; __launch_bounds__(512); one workgroup per CU.
 * gm3d_linprobe_eval: z = ((Q - running_mean) / sqrt(running_var + 1e-6)) W^T + bias for all m rows of Q (m,d) f32, one fmaf per
 *   column onto the running sum, columns ascending, then + bias; the classes are ranked by (logit descending, class ascending, -0 ==
 *   +0, NaN above +inf).  logits (m,ncls) f32 or NULL; pred (m) int64 = the first class, or NULL; yq (m) int64 or NULL: correct[0] +=
 *   the rows whose first class is the label, correct[1] += the rows with the label among the first min(5, ncls) classes (int64
 *   atomics; with yq NULL correct is not touched and may be NULL).  One launch of ceil(m / 64) workgroups of 256 threads.
 * gm3d_linprobe_slices: ceil(d / 16), the number of column slices (0 for d < 1).
 * Limits (GM3D_EINVAL for n < 1, m < 0, d < 1, ncls < 1, batch < 2, batch > n, t_begin < 0, t_end < t_begin, momentum outside [0, 1)
 * or NaN, a NULL required pointer, a misaligned X or xhat; GM3D_EUNSUPPORTED beyond the kernels' range; all checked on the host
 * before any launch):
 *   1 <= n <= 16384, m >= 0, 8 <= d <= 1024, d % 8 == 0, 2 <= ncls <= 64, 2 <= batch <= min(n, 1024).
 * m == 0 returns GM3D_OK after the shape checks, launching nothing. */
int gm3d_linprobe_slices(int d);
int gm3d_linprobe_train(const float *X, const long long *y, int n, int d, int ncls, int batch, const int *order, const float *lr,
                        int t_begin, int t_end, float momentum, float *W, float *mom_w, float *bias2, float *mom_b,
                        float *running_mean, float *running_var, float *xhat, float *part, float *losses, gm3d_stream_t stream);
int gm3d_linprobe_eval(const float *Q, const long long *yq, int m, int d, int ncls, const float *W, const float *bias,
                       const float *running_mean, const float *running_var, float *logits, long long *pred, long long *correct,
                       gm3d_stream_t stream);

/* ---- Reconstructed clouds (gm3d_amd/csrc/reconstruct.hip) -----------------------------------------------------------------------------
 * The `vis` branch of Point-MAE_SA3D/models/Point_MAE.py:428-439 in one launch: the visible patches moved back to their centres, the
 * decoder's patches placed at the masked centres, and the centres in matching order.
 * pred (B,M,3k) f32 or bf16 (dtype), batch stride pred_bstride in elements (the last-M view of a (B,L,3k) tensor is taken as it is;
 * rows are dense); neighborhood (B,G,k,3) f32, centre-relative; center (B,G,3) f32; vis_ids (B,V) and mask_ids (B,M) int64 with row
 * strides vis_stride / mask_stride in elements.  The ids are trusted, like gm3d_token_assemble_fwd's (one outside 0..G-1 is clamped
 * into that range, so no read leaves its cloud).  dense (B*G*k,3) f32 and full_center (B*G,3) f32: every element is written.
 *   visible row  = neighborhood[b, id, j] + center[b, id]                      (one fp32 add)
 *   rebuilt row  = float(pred[b, m, 3j .. 3j+2]) + center[b, mask_ids[b, m]]   (one fp32 add)
 * layout GM3D_RECON_PER_CLOUD: patch block b*G + i of dense is cloud b's [visible patches in vis_ids order | rebuilt patches in
 *   mask_ids order]; full_center has the same order, so centre i belongs to rows i*k .. i*k + k - 1.
 * layout GM3D_RECON_FLAT (the reference's, for any B): all clouds' visible patches (block b*V + i), then all clouds' rebuilt patches
 *   (B*V + b*M + i); full_center is all MASKED centres (row b*M + i), then all visible ones (B*M + b*V + i) -- the reference's own
 *   disagreement between its two outputs, kept.
 * Limits, checked on the host before any launch: GM3D_EINVAL for a NULL neighborhood / center / dense / full_center, B < 0, G < 1,
 * k < 1, V < 0, M < 0, V + M != G, an unknown layout or dtype, a NULL vis_ids or vis_stride < V when V > 0, a NULL mask_ids / pred,
 * mask_stride < M or pred_bstride < M*3k when M > 0 (with V == 0 or M == 0 the matching pointers may be NULL);
 * GM3D_EUNSUPPORTED for B*G*k*3 >= 2^31.  B == 0 returns GM3D_OK without a launch.
 * One wave per patch, 16-byte accesses when k % 4 == 0 and the bases are aligned, 4-byte ones otherwise; no LDS. */
enum { GM3D_RECON_PER_CLOUD = 0, GM3D_RECON_FLAT = 1 };
int gm3d_reconstruct_assemble(const void *pred, long long pred_bstride, const float *neighborhood, const float *center,
                              const long long *vis_ids, long long vis_stride, const long long *mask_ids, long long mask_stride,
                              int B, int G, int k, int V, int M, int layout, float *dense, float *full_center, int dtype,
                              gm3d_stream_t stream);
/* The ragged form, for the hierarchical model (gm3d_amd/point_m2ae.py), whose visible count at the finer levels differs from cloud
 * to cloud: a stable per-cloud partition of the G tokens by `masked` (B,G) bytes (non-zero = masked, gm3d_partition_visible's sense)
 * with the patches moved back to their centres in that order, in one launch.  Slot order of cloud b: its visible tokens in ascending
 * token index, then its masked tokens in ascending token index; order (B,G) int32 = the token at each slot, n_visible (B) int32 = the
 * number of visible tokens.  neighborhood (B,G,k,3) f32, centre-relative; center (B,G,3) f32; pred (B,G,3k) f32 or bf16 (dtype),
 * contiguous, a row for EVERY token -- rows of visible tokens are never read --, or NULL: a masked token's rows are then its true patch
 * (dense = [visible patches | hidden ground truth]).  dense (B*G*k,3) f32, full_center (B*G,3) f32, order and n_visible: every
 * element is written exactly once.
 *   visible token t at slot s:  dense[b, s, j] = neighborhood[b, t, j] + center[b, t]                    (one fp32 add)
 *   masked token t at slot s:   dense[b, s, j] = float(pred[b, t, 3j .. 3j+2]) + center[b, t]            (one fp32 add)
 *   full_center[b, s] = center[b, t]
 * Limits, checked on the host before any launch: GM3D_EINVAL for a NULL neighborhood / center / masked / dense / full_center / order /
 * n_visible, B < 0, G < 1, k < 1 or an unknown dtype (also with pred NULL); GM3D_EUNSUPPORTED for G > 8192 or B*G*k*3 >= 2^31.
 * B == 0 returns GM3D_OK without a launch.
 * ceil(G/16) workgroups per cloud; each recomputes its cloud's ranks from the G mask bytes (64-bit ballots, popcounts, a prefix over
 * the 64-token chunks in LDS) and moves 16 tokens at once, 16 lanes per patch, with 16-byte accesses when k % 4 == 0 and the bases are
 * aligned and 4-byte ones otherwise.  No atomics, no dependence between workgroups. */
int gm3d_reconstruct_partition(const void *pred, const float *neighborhood, const float *center, const unsigned char *masked, int B,
                               int G, int k, int dtype, float *dense, float *full_center, int *order, int *n_visible,
                               gm3d_stream_t stream);

/* ---- Soft-target cross-entropy and point mixup (gm3d_amd/csrc/soft_ce.hip, gm3d_amd/losses.py) -----------------------------------------
 * gm3d_soft_ce_fwd: logits (B,C) f32 or bf16 (dtype), all arithmetic f32.  The target row t_i is given in exactly one of two forms:
 *   compact: ya (B) int64, yb (B) int64 or NULL, coef (3) f32 ON THE DEVICE = (wa, wb, u): t_ic = u + wa [c = ya_i] + wb [c = yb_i]
 *            (with yb NULL the wb term is absent and coef[1] is not used);
 *   dense:   dense (B,C) f32 (ya, yb and coef NULL).
 * Per row: m = max_c z_c, lse_i = m + log sum_c exp(z_c - m), row_loss_i = sum_c t_ic (lse_i - z_c) formed as written -- products of a
 * weight and the non-negative lse - z_c; compact: (wa (lse - z[ya]) + wb (lse - z[yb])) + u sum_c (lse - z_c), the last term left out
 * when u == 0.  loss (1) = the mean of row_loss over B.  A label outside [0, C) makes that row's loss (and the mean) NaN, as in
 * gm3d_cls_tail_fwd; its lse is still written.  row_loss (B), lse (B) and loss (1) f32 are all written.  One launch of one workgroup
 * (one wave per row, min(16, B) waves); the sums run in the fixed order soft_ce.hip states, without atomics.
 *
 * gm3d_soft_ce_bwd: dlogits_ic = dloss[0] / B * (S_i exp(z_c - lse_i) - t_ic) in the logits' dtype, S_i = sum_c t_ic (compact:
 * (C u + wa) + wb; dense: summed, nothing assumed), from the same target arguments, the forward's lse (B) and dloss (1) f32.
 * exp(z_c - lse_i) is divided by its own row sum, which is 1 up to the rounding of the stored lse_i (half an ulp of lse: 1.5e-5 at
 * |lse| = 300) and takes that rounding out again.  A row whose label is outside [0, C) is NaN.  One launch, one wave per row, every
 * element written once by its one owner.
 *
 * Limits, checked on the host before any launch: GM3D_EINVAL for a NULL logits or output, B < 0, C < 1, an unknown dtype, both target
 * forms or neither, a compact form without ya or coef; GM3D_EUNSUPPORTED for B > 4096 or C > 1024.  B == 0 returns GM3D_OK after the
 * checks without a launch.
 *
 * gm3d_mixup_points (Point-MAE_SA3D/engine_finetune.py:43-76): out[b] = fl(fl(l x[b]) + fl(m x[perm[b]])) for x (B,N,3) f32 -- two
 * products rounded separately and one add, no FMA -- with coef2 (2) f32 ON THE DEVICE = (l, m) = (f32(lam), f32(1 - lam)), perm (B)
 * int64 on the device; the same launch writes yb[b] = ya[perm[b]] (ya, yb (B) int64: both or neither).  Out of place (a cloud is read by
 * two outputs): out == x is refused.  perm cannot be checked on the host; values in [0, B) are the caller's contract, and one outside
 * reads nothing: that cloud becomes NaN and its yb -1.  One workgroup per cloud, one launch.
 * Limits as gm3d_augment's: GM3D_EINVAL for a NULL x / perm / coef2 / out, out == x, N < 1, B < 0, ya without yb or yb without ya; no
 * limit on N.  B == 0 returns GM3D_OK without a launch. */
int gm3d_soft_ce_fwd(const void *logits, int B, int C, const long long *ya, const long long *yb, const float *coef, const float *dense,
                     float *row_loss, float *lse, float *loss, int dtype, gm3d_stream_t stream);
int gm3d_soft_ce_bwd(const void *logits, int B, int C, const long long *ya, const long long *yb, const float *coef, const float *dense,
                     const float *lse, const float *dloss, void *dlogits, int dtype, gm3d_stream_t stream);
int gm3d_mixup_points(const float *x, int B, int N, const long long *perm, const float *coef2, const long long *ya, float *out,
                      long long *yb, gm3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GM3D_H */
