/*
 * m3slam.h - C ABI of libm3slam_hip.so: the MI355X (gfx950) hot path of MASt3R-SLAM.
 *
 * Drop-in boundary.  Every entry point replaces one array-in /
 * array-out operator of the reference's kernel-dispatch layer
 * (/root/reference/src/mlx_mast3r_slam/backends/mpsgraph/kernels.py) or one
 * fused span of its MLX host code; the replaced interface is cited per function.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (hipMalloc / torch ROCm storage) unless
 *     the parameter is documented as "host"; arrays are C-contiguous;
 *   - the caller owns and allocates every buffer, including workspaces; the
 *     library allocates nothing and keeps no mutable state between calls except
 *     per-kernel, per-device "large-LDS opt-in done" bits (atomic; a process may
 *     drive several devices from several threads) and the thread-local text of
 *     the last HIP error;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work
 *     is stream-ordered and asynchronous, nothing synchronises the host;
 *   - return value: M3_OK (0) or a negative m3_status; no silent fallback exists;
 *   - float = IEEE binary32, poses are 8 floats [tx,ty,tz,qx,qy,qz,qw,s].
 */
#ifndef M3SLAM_H
#define M3SLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    M3_OK = 0,
    M3_ERR_INVALID_ARG = -1,   /* null pointer, non-positive size, unsupported value */
    M3_ERR_LAUNCH = -2,        /* hipGetLastError() != hipSuccess after a launch */
    M3_ERR_UNSUPPORTED = -3    /* size outside what the kernel was built for */
} m3_status;

/* ABI version (major*1000 + minor) and human-readable status text. */
int m3_abi_version(void);
const char *m3_status_string(int status);
/* Text of the last HIP error seen by this library on the calling thread ("" if none). */
const char *m3_last_hip_error(void);
/* Compute units of the current device (cached per device): the "fills the chip" grid thresholds of the convolution
 * dispatch (ops.conv3x3_direct_ok, the sliced single-pass convolution) derive from it instead of a constant 256. */
int m3_device_cu_count(void);

/* ------------------------------------------------------------------ matching */

/* prep_for_iter_proj (matching.py:134-175 + normalize_rays :121 + img_gradient
 * image.py:9-34).  X11,X21 [B,H,W,3]; idx_init int64 [B,H*W] or NULL (identity).
 * Out: rays_with_grad [B,H,W,9] = (ray, d ray/dx, d ray/dy), pts3d_norm [B,H*W,3],
 * p_init [B,H*W,2] = (idx % W, idx / W) as float. */
int m3_prep_iter_proj(const float *X11, const float *X21, const int64_t *idx_init,
                      float *rays_with_grad, float *pts3d_norm, float *p_init,
                      int B, int H, int W, void *stream);

/* kernels.iter_proj (kernels.py:107-148, numpy twin :151-254; Metal iter_proj.metal:82).
 * rays_with_grad [B,H,W,9], pts3d_norm [B,N,3], p_init [B,N,2] -> p_out [B,N,2],
 * valid_out uint8 [B,N].  ws: uint32 [m3_iter_proj_ws_words(B, N, max_iter)] workspace (per-wave step
 * maxima, plain stores - no atomics - plus the per-item iteration limit).
 * stop_scope: 0 = reference behaviour, all points stop at the first LM iteration whose
 * max step norm over the WHOLE call is < convergence_thresh; 1 = per batch item. */
int64_t m3_iter_proj_ws_words(int B, int N, int max_iter);
int m3_iter_proj(const float *rays_with_grad, const float *pts3d_norm, const float *p_init,
                 float *p_out, uint8_t *valid_out, uint32_t *ws,
                 int B, int H, int W, int N, int max_iter, float lambda_init,
                 float convergence_thresh, int stop_scope, void *stream);

/* kernels.refine_matches (kernels.py:463-493, numpy twin :496-537; Metal
 * refine_matches.metal:160).  D11 [B,H,W,D], D21 [B,N,D], p_in int32 [B,N,2] ->
 * p_out int32 [B,N,2].  chained = 0: numpy-twin semantics (every dilation pass
 * re-centres on p_in, i.e. the dilation-1 pass decides); 1: Metal semantics (passes
 * chain).  p_out must not alias p_in. */
int m3_refine_matches(const float *D11, const float *D21, const int32_t *p_in, int32_t *p_out,
                      int B, int H, int W, int D, int N, int radius, int dilation_max,
                      int chained, void *stream);
/* Same with both descriptor arrays stored as IEEE half ("fp16 features", BASELINE configs[4]; halves the
 * kernel's HBM bytes).  Values are widened to fp32 exactly and scored with the same fp32 sequence,
 * so p_out equals m3_refine_matches on the half-rounded descriptors bit for bit. */
int m3_refine_matches_f16(const void *D11, const void *D21, const int32_t *p_in, int32_t *p_out,
                          int B, int H, int W, int D, int N, int radius, int dilation_max,
                          int chained, void *stream);

/* Tail of match_iterative_proj (matching.py:436-461): gather X11 at clip(p), 3-D distance
 * test, AND with valid_proj, idx = u + W*v.  p_f32 (iter_proj output, truncated like
 * .astype(int32), matching.py:410) is used when p_i32 is NULL. */
int m3_match_epilogue(const float *X11, const float *X21, const int32_t *p_i32, const float *p_f32,
                      const uint8_t *valid_proj, int64_t *idx_out, uint8_t *valid_out,
                      int B, int H, int W, float dist_thresh, void *stream);

/* match_simple (matching.py:41-90): idx = idx_init or arange; valid = |X11[idx]-X21| < thresh.
 * idx_out may alias idx_init. */
int m3_match_simple(const float *X11, const float *X21, const int64_t *idx_init,
                    int64_t *idx_out, uint8_t *valid_out, int B, int H, int W,
                    float dist_thresh, void *stream);

/* float [.,2] -> int32 [.,2] truncation (p.astype(int32), matching.py:410). */
int m3_trunc_i32(const float *p, int32_t *out, int64_t count, void *stream);

/* Nearest neighbour in descriptor space, the search primitive of "fast reciprocal NN" matching (named by
 * BASELINE.json; absent from the reference tree - SURVEY 8a row K8 - so the semantics are this library's):
 * idx_out[b][s] = argmax_n <Q[b][s], DB[b][n]> in fp32 (two fused-multiply-add chains over the even and the
 * odd dimensions, added at the end), ties to the lowest n; score_out (may be NULL) = the maximum.  Q [B,S,D], DB [B,N,D] f32, D in {16, 24, 32},
 * 16-byte aligned; keys_ws: uint64 [B*S] scratch. */
int m3_nn_search(const float *Q, const float *DB, int32_t *idx_out, float *score_out, uint64_t *keys_ws,
                 int B, int S, int N, int D, void *stream);

/* The same search on the matrix cores (v_mfma_f32_16x16x32_f16, one k-step covers D <= 32): operands are packed to
 * K-padded fp16 first - fp16 descriptors (in_f16 = 1, BASELINE configs[4] "fp16 features") take 1 MFMA per 16 x 16
 * scores with exact products; fp32 descriptors (in_f16 = 0) are split hi + lo and take 3 (score error <= 2^-24 for
 * unit vectors).  Ties to the lowest n as above.  pack_ws: m3_nn_pack_bytes(...) bytes, 16-byte aligned. */
int64_t m3_nn_pack_bytes(int B, int S, int N, int in_f16);
int m3_nn_search_mfma(const void *Q, const void *DB, int32_t *idx_out, float *score_out, uint64_t *keys_ws,
                      void *pack_ws, int B, int S, int N, int D, int in_f16, void *stream);

/* Fast reciprocal nearest-neighbour matching, P pairs at once, loop on the device (MASt3R sec. 3.3; BASELINE.json names
 * it, the reference tree has no code for it: semantics in mast3r_slam/matching.py, oracle/matching.py).  Each
 * descriptor map [P,N,D] (fp32, or IEEE fp16 with in_f16 = 1; D in {16, 24, 32}) is packed ONCE
 * (m3_frnn_pack -> m3_frnn_pack_bytes(P, N, in_f16) bytes, 16-byte aligned) and serves as the database of one search
 * direction and as the query source of the other.  m3_frnn_round runs view 1 -> view 2 -> view 1 for every seed:
 * cur int32 [P,S] = the view-1 pixel a seed sits on (in / out), active uint8 [P,S] (in / out), got1 / got2 int32
 * [P,S] = this round's reciprocal pairs (-1 where none), xy2_ws int32 [P,S], keys_ws uint64 [P,S] scratch that
 * must be zero on entry and is left zero. */
int64_t m3_frnn_pack_bytes(int P, int N, int in_f16);
int m3_frnn_pack(const void *Dmap, void *packed, int P, int N, int D, int in_f16, void *stream);
int m3_frnn_round(const void *packed1, const void *packed2, int32_t *cur, uint8_t *active, int32_t *got1,
                  int32_t *got2, int32_t *xy2_ws, uint64_t *keys_ws, int P, int S, int N1, int N2, int in_f16,
                  void *stream);
/* The same round restricted to the seeds that are still active (rounds >= 2): act_ws int32 [P * (S + 1)] scratch receives
 * the ascending list of active seed slots per pair and their count; search workgroups past a pair's count exit at once.
 * Same results as m3_frnn_round. */
int m3_frnn_round_active(const void *packed1, const void *packed2, int32_t *cur, uint8_t *active, int32_t *got1,
                         int32_t *got2, int32_t *xy2_ws, uint64_t *keys_ws, int32_t *act_ws, int P, int S, int N1,
                         int N2, int in_f16, void *stream);
/* The same rounds with an EXACT pruned search (round 4).  The maps are H x W pixels in raster order (N = H * W).  Per
 * packed map, once per call, m3_frnn_blockstats writes for every 8 x 8 pixel tile a reference point (its centroid, fp16),
 * its radius and a norm bound (stats: m3_frnn_stats_bytes(P, H, W) bytes, 16-byte aligned).  A search then scores the
 * queries against the tile centroids on the matrix core (1/64 of the full search), drops every (16-query tile, block)
 * whose Cauchy-Schwarz bound <q, c> + |q| r lies below a lower bound of the query's final maximum, and scores the
 * surviving blocks with the MFMA sequence of the brute-force kernel - index and score equal m3_frnn_round's bit for bit
 * (a block holding the maximum or a tie always survives; ties go to the lowest pixel index).  When more than a quarter
 * of the pairs survive (descriptor maps without spatial coherence) the brute-force kernel runs instead; both test one
 * device counter, no host decision.  act_ws as in m3_frnn_round_active, or NULL for a round on every seed; seed_order
 * int32 [S] or NULL: the order in which the active slots are listed (with act_ws) - the searches work on groups of
 * consecutive entries, so an order that walks the seed grid in small patches prunes more; no result depends on it.
 * prune_ws: m3_frnn_prune_ws_bytes(...) bytes, 16-byte aligned.  Finite descriptors are assumed. */
int64_t m3_frnn_stats_bytes(int P, int H, int W);
int m3_frnn_blockstats(const void *packed, void *stats, int P, int H, int W, int in_f16, void *stream);
int64_t m3_frnn_prune_ws_bytes(int P, int S, int H1, int W1, int H2, int W2);
int m3_frnn_round_pruned(const void *packed1, const void *packed2, const void *stats1, const void *stats2, int32_t *cur,
                         uint8_t *active, int32_t *got1, int32_t *got2, int32_t *xy2_ws, uint64_t *keys_ws,
                         int32_t *act_ws, const int32_t *seed_order, void *prune_ws, int P, int S, int H1, int W1, int H2,
                         int W2, int in_f16, void *stream);
/* The reciprocal pairs of `rounds` rounds (got1 / got2 int32 [rounds,P,S]) as fixed-shape device outputs - no sort, no
 * host synchronisation (the matcher can be captured into a hipGraph): map1 int32 [P,N1] = view-1 pixel -> its partner
 * in view 2 (-1 = none); optionally the tracker's maps idx2 int64 [P,N2] / valid2 uint8 [P,N2] (view-2 pixel -> view-1
 * pixel; both or neither); pairs int32 [P,S,2] = the distinct (p1, p2) of every image pair sorted by p1, count int32 [P]
 * (rows >= count[pair] are -1; a seed converges at most once, so S bounds the number of pairs); chunk_ws int32
 * [P * m3_frnn_chunks(N1)] scratch. */
int m3_frnn_chunks(int N1);
int m3_frnn_collect(const int32_t *got1, const int32_t *got2, int rounds, int P, int S, int N1, int N2, int32_t *map1,
                    int64_t *idx2, uint8_t *valid2, int32_t *pairs, int32_t *count, int32_t *chunk_ws, void *stream);

/* ------------------------------------------------------------------ tracking */

/* FrameTracker.track glue (tracker.py:88-113, _get_points_poses :177-214): for each
 * keyframe pixel n:  Xf_g = Xf_canon[idx[n]], Cf = Cf_avg[idx[n]],
 * Qk = sqrt(Qff[idx[n]] * Qkf[n]), valid_opt = valid_match & Cf>C_conf & Ck>C_conf & Qk>Q_conf,
 * valid_kf = valid_match & Qk>Q_conf.  counts int32[2] = (sum valid_opt, sum valid_kf)
 * (zeroed by the call). */
int m3_track_gather(const float *Xf_canon, const float *Cf_avg, const float *Ck_avg,
                    const float *Qff, const float *Qkf, const int64_t *idx,
                    const uint8_t *valid_match, float *Xf_g, float *Qk,
                    uint8_t *valid_opt, uint8_t *valid_kf, int32_t *counts,
                    int N, float C_conf, float Q_conf, void *stream);

/* Batched forms: P independent problems laid out back to back ([P,N,...] arrays, [P,8] poses,
 * counts int32 [P,2], info double [P,4], ws double [P * m3_track_ws_doubles()]); one launch
 * sequence serves all P (the per-GPU shard of a keyframe-pair batch). */
int m3_track_gather_batch(const float *Xf_canon, const float *Cf_avg, const float *Ck_avg,
                          const float *Qff, const float *Qkf, const int64_t *idx,
                          const uint8_t *valid_match, float *Xf_g, float *Qk, uint8_t *valid_opt,
                          uint8_t *valid_kf, int32_t *counts, int P, int N, float C_conf,
                          float Q_conf, void *stream);
int m3_track_gn_ray_dist_batch(const float *Xf, const float *Xk, const float *Qk,
                               const uint8_t *valid, const float *T_WCf, const float *T_WCk,
                               float *T_WCf_out, float *T_CkCf_out, double *info, double *ws,
                               int P, int N, int max_iters, float huber_k, float sigma_ray,
                               float sigma_dist, float rel_error, float delta_norm,
                               int fixed_iters, void *stream);

/* Number of doubles the tracking workspace needs (per problem). */
int64_t m3_track_ws_doubles(void);

/* FrameTracker._opt_pose_ray_dist_sim3 (tracker.py:258-324) with _solve (:216-256),
 * act_Sim3 / point_to_ray_dist (geometry.py:46-137), Sim3 inv/mul/exp/retr
 * (liegroups/sim3.py:107-262), check_convergence (optimizer.py:11-46) - the whole
 * <= max_iters Gauss-Newton loop runs on the device with no host round trip.
 * Xf [N,3] (already gathered), Xk [N,3], Qk [N], valid uint8 [N], T_WCf/T_WCk [8].
 * Out: T_WCf_out [8], T_CkCf_out [8], info double[4] = (iterations run, last cost,
 * last |tau|, status: 0 = iteration budget used up, 1 = converged, 2 = solve failed - singular
 * normal matrix or divergent step, the pose is the last good one; the reference raises there and
 * FrameTracker.track returns try_reloc, tracker.py:121-141).  ws: double[m3_track_ws_doubles()].
 * fixed_iters != 0 disables the convergence test (exactly max_iters iterations). */
int m3_track_gn_ray_dist(const float *Xf, const float *Xk, const float *Qk, const uint8_t *valid,
                         const float *T_WCf, const float *T_WCk,
                         float *T_WCf_out, float *T_CkCf_out, double *info, double *ws,
                         int N, int max_iters, float huber_k, float sigma_ray, float sigma_dist,
                         float rel_error, float delta_norm, int fixed_iters, void *stream);

/* FrameTracker._opt_pose_calib_sim3 (tracker.py:326-406) with project_calib (geometry.py:156-227):
 * residual (u, v, log z) of keyframe pixel n = (n % W, n / W) minus the projection of T . Xf[n], gated by
 * valid & Xk.z > depth_eps & projection inside the image.  Xf/Xk must already be ray-constrained
 * (m3_constrain_points_to_ray).  K4 = HOST array (fx, fy, cx, cy).  Batched over P problems like
 * m3_track_gn_ray_dist_batch; same outputs and workspace. */
int m3_track_gn_calib_batch(const float *Xf, const float *Xk, const float *Qk, const uint8_t *valid,
                            const float *T_WCf, const float *T_WCk, float *T_WCf_out,
                            float *T_CkCf_out, double *info, double *ws, int P, int N, int H, int W,
                            const float *K4, int max_iters, float huber_k, float sigma_pixel,
                            float sigma_depth, float pixel_border, float depth_eps, float rel_error,
                            float delta_norm, int fixed_iters, void *stream);

/* constrain_points_to_ray (geometry.py:273-302): out[n] = ((u-cx)/fx z, (v-cy)/fy z, z) with z = X[n].z
 * and (u, v) the pixel of n; X, out [P,H*W,3]; K4 = HOST (fx, fy, cx, cy). */
int m3_constrain_points_to_ray(const float *X, float *out, int P, int H, int W, const float *K4,
                               void *stream);

/* One Gauss-Newton normal-equation build at a given relative pose (the JTJ/JTr
 * reduction of tracker.py:239-244): out double[36] = H upper triangle (28, row-major),
 * g (7), cost (1).  ws as above. */
int m3_track_normal_eq(const float *Xf, const float *Xk, const float *Qk, const uint8_t *valid,
                       const float *T_CkCf, double *out, double *ws, int N, float huber_k,
                       float sigma_ray, float sigma_dist, void *stream);

/* The same build for the calibrated residual of m3_track_gn_calib_batch (one problem, N == H * W): the sums of
 * one linearisation at T_CkCf, gated by valid & Xk.z > depth_eps & projection inside the image less pixel_border.
 * K4 = HOST array (fx, fy, cx, cy).  out and ws as for m3_track_normal_eq. */
int m3_track_normal_eq_calib(const float *Xf, const float *Xk, const float *Qk, const uint8_t *valid,
                             const float *T_CkCf, double *out, double *ws, int N, int H, int W,
                             const float *K4, float huber_k, float sigma_pixel, float sigma_depth,
                             float pixel_border, float depth_eps, void *stream);

/* Sim3.act over a point map (tracker.py:146 Xkk = T_CkCf.act(Xkf)): out = s R X + t. */
int m3_sim3_act(const float *T, const float *X, float *out, int N, void *stream);

/* ------------------------------------------------------------------ frame / keyframe state */

/* Frame.update_pointmap (frame.py:75-133), in place on the frame's X_canon [N,3] / C [N] (the summed
 * confidence; get_average_conf = C / N_frames stays on the host side).  If T (device, [8]) is not NULL
 * the new points are first moved by Sim3.act(T, .) - the keyframe update of tracker.py:146-147
 * (Xkk = T_CkCf.act(Xkf); keyframe.update_pointmap(Xkk, Ckf)) in one pass.  Modes:
 *   REPLACE             X, C <- new                      ("first" on its first update, "recent", a winning "best_score")
 *   INDEP_CONF          per point: take new where C_new > C           (frame.py:108-114)
 *   WEIGHTED_POINTMAP   X <- (C X + C_new X_new) / (C + C_new), C <- C + C_new   (:115-120, the default)
 *   WEIGHTED_SPHERICAL  the same average on (r, phi, theta)           (:121-129, geometry.py:318-351) */
enum { M3_FUSE_REPLACE = 0, M3_FUSE_INDEP_CONF = 1, M3_FUSE_WEIGHTED_POINTMAP = 2, M3_FUSE_WEIGHTED_SPHERICAL = 3 };
int m3_fuse_pointmap(float *X_canon, float *C, const float *X_new, const float *C_new, const float *T,
                     int N, int mode, void *stream);

/* "best_score" filtering (frame.py:59-73, :103-107) without the host: m3_median_f32 = the median of v[0..N) as
 * np.median / mx.median define it (mean of the two middle order statistics, float32) by an exact radix select on the
 * float bits - out float [1] on the device, ws uint32 [m3_median_ws_words()] scratch; any finite values, -0 < +0.
 * m3_fuse_pointmap_if_better: best_state float [2] on the device = (best score so far, flag); if *score_new >
 * best_state[0] the frame's pointmap is REPLACED (as M3_FUSE_REPLACE, T as above), best_state[0] <- *score_new and
 * best_state[1] <- 1, else nothing changes and best_state[1] <- 0.  Initialise best_state[0] with the first pointmap's
 * score (the first update always replaces, frame.py:88-92). */
int64_t m3_median_ws_words(void);
int m3_median_f32(const float *v, int N, uint32_t *ws, float *out, void *stream);
int m3_fuse_pointmap_if_better(float *X_canon, float *C, const float *X_new, const float *C_new, const float *T, int N,
                               const float *score_new, float *best_state, void *stream);

/* Number of distinct values among idx[n] with valid[n] != 0 (tracker.py:153-155, mx.unique(idx[valid])),
 * values in [0, range): bitmap (atomicOr) + popcount, an exact integer.  bitmap_ws: uint32
 * [m3_count_unique_ws_words(range)] scratch; count_out: int32 [1] on the device. */
int64_t m3_count_unique_ws_words(int range);
int m3_count_unique(const int64_t *idx, const uint8_t *valid, int N, int range, uint32_t *bitmap_ws,
                    int32_t *count_out, void *stream);

/* ------------------------------------------------------------------ backend GN ("rays") */

/* Per-edge normal-equation blocks of kernels.gauss_newton_rays (kernels.py:262-322; numpy
 * twin gauss_newton.py:100-251; Metal gn_jacobian_kernel gauss_newton.metal:66-252 + host
 * reduction gn_metal_runner.py:221-292).  Twc [K,8], Xs [K,P,3], Cs [K,P], ii,jj int32 [E],
 * idx int32 [E,P], valid uint8 [E,P], Q [E,P] -> blocks double [E,36] = (Hjj upper triangle
 * 28, gj 7, valid count 1).  With the reference's Ji = -Jj: Hii = Hjj, Hij = -Hjj, gi = -gj.
 * ws: double [E * m3_gn_rays_chunks(P) * 36].
 * point_mode = 1 selects kernels.gauss_newton_points (kernels.py:396-460, numpy twin
 * gauss_newton_points.py:17-207; Metal gn_points_jacobian_kernel gauss_newton_points.metal:65):
 * the same residual with the extra scale-invariant weight 1/(|Xi| + 1e-6) and sigma = sigma_point.
 * point_mode = 2 selects kernels.gauss_newton_calib (kernels.py:325-393, numpy twin
 * gauss_newton_calib.py:17-274; Metal gn_calib_jacobian_kernel gauss_newton_calib.metal:74): residual
 * ((du, dv)/sigma_pixel, dlog z/sigma_depth) with depth and image-border gates; `calib` is a HOST
 * array of 10 floats (fx, fy, cx, cy, width, height, border, z_eps, sigma_pixel, sigma_depth),
 * NULL otherwise; sigma_ray is ignored in that mode (pass any positive value). */
int m3_gn_rays_chunks(int P);
int m3_gn_rays_blocks(const float *Twc, const float *Xs, const float *Cs, const int32_t *ii,
                      const int32_t *jj, const int32_t *idx, const uint8_t *valid, const float *Q,
                      double *blocks, double *ws, int K, int P, int E, float sigma_ray,
                      float C_thresh, float Q_thresh, int point_mode, const float *calib,
                      void *stream);

/* Dense normal equations from the per-edge blocks (gauss_newton.py:220-251): H double
 * [dim,dim], g double [dim], dim = 7*num_free (both zeroed by the call; the 1e-6 I
 * regulariser of gauss_newton.py:254 is NOT added here). */
int m3_gn_rays_assemble(const double *blocks, const int32_t *ii, const int32_t *jj,
                        const int32_t *local, double *H, double *g, int K, int E, int num_free,
                        void *stream);

/* T[kf] <- exp(dx[7*local[kf] ..]) * T[kf] for every free keyframe (retract_sim3,
 * sim3_ops.py:229-251; Metal pose_update_kernel gauss_newton.metal:255). */
int m3_gn_rays_retract(float *Twc, const double *dx, const int32_t *local, int K, void *stream);

/* Whole gauss_newton_rays loop on the device (gauss_newton.py:95-280): per iteration
 * blocks -> dense H (7F x 7F, + 1e-6 I) and g -> Cholesky solve -> |dx| < delta_thresh stop
 * -> T <- exp(dx) T (retract_sim3, sim3_ops.py:229) for the free keyframes.
 * local int32 [K]: keyframe -> free-block index, < 0 = pinned or unused (host builds it
 * from unique(ii,jj) and pin, gauss_newton.py:73-81).  Twc is updated IN PLACE.
 * Hbuf double [m3_gn_rays_hbuf_doubles(dim)], dim = 7*num_free: ANY size - systems up to
 * m3_gn_rays_max_dim() (63) are factored in place by one workgroup, larger ones (BASELINE configs[4]: 256
 * keyframes -> 1785 unknowns) by the blocked Cholesky of gn_chol.hip; either way the loop never
 * leaves the stream (the reference solves on the host, gauss_newton.py:253-260).
 * info double[4] = (iterations applied, last |dx|, converged/stopped flag, solver failure flag). */
int m3_gn_rays_max_dim(void);
int64_t m3_gn_rays_hbuf_doubles(int dim);
int m3_gn_rays_solve(float *Twc, const float *Xs, const float *Cs, const int32_t *ii,
                     const int32_t *jj, const int32_t *idx, const uint8_t *valid, const float *Q,
                     const int32_t *local, double *blocks, double *ws, double *Hbuf, double *info,
                     int K, int P, int E, int num_free, float sigma_ray, float C_thresh,
                     float Q_thresh, int max_iter, float delta_thresh, int point_mode,
                     const float *calib, void *stream);

/* One Gauss-Newton step from per-edge blocks the caller already has (the edge-sharded solve: every rank
 * evaluated its own edges, the 36-double blocks were all-gathered): assemble -> factor -> solve -> stop test
 * -> retract, stream-ordered, stop / failure flags on the device in info (m3_gn_rays_info_init once first). */
int m3_gn_rays_info_init(double *info, void *stream);
int m3_gn_rays_step(float *Twc, const double *blocks, const int32_t *ii, const int32_t *jj,
                    const int32_t *local, double *Hbuf, double *info, int K, int E, int num_free,
                    float delta_thresh, void *stream);

/* linalg.cholesky_solve (linalg.py:17-50) for a system of any size: (H + shift I) x = b in float64 by blocked
 * Cholesky (block 64), stream-ordered.  H [dim,dim] row-major (lower triangle read; destroyed), b [dim]
 * (destroyed), x [dim], ws double[m3_chol_ws_doubles(dim)]: ws[0] = 0 ok / 1 not positive definite (the rest is
 * scratch: the substitution vector and the 64 x 64 diagonal factors, which are kept OUT of H so that no
 * workgroup of a panel launch ever reads a diagonal block another one has already overwritten).
 * The backward substitution is ONE launch whose workgroups hand x_k to each other through device flags; a consumer
 * always has a higher workgroup index than its producer, i.e. the chain assumes workgroups are dispatched in index
 * order (true on gfx950, not promised by HIP).  The wait is bounded: if a producer has not published after ~0.3 s
 * of polling the launch gives up and ws[0] = 1 (status "failed"), it never hangs the stream. */
int64_t m3_chol_ws_doubles(int dim);
int m3_chol_solve(double *H, double *b, double *x, double *ws, int dim, double shift, void *stream);

/* ----------------------------------------------------------------- retrieval */

/* Keyframe retrieval database, "simple retrieval" of RetrievalDatabase (mast3r_utils.py:696-715 compute_signature,
 * :717-795 update / query).  Host side: mast3r_slam/retrieval.py.
 *
 * Signature: sig[b] = m / sqrt(sum(m^2) + 1e-8) with m = mean over t of feat[b, t, :], fp32 throughout.  feat [B,T,C]
 * contiguous, 16-byte aligned, dtype M3_RETRIEVAL_BF16 / _F16 (the M3_DT_BF16 / M3_DT_F16 codes of m3slam_model.h) or
 * _F32; T >= 1, C a multiple of 8.  Row b is written at sig + b * sig_stride (floats): a database row is the output.
 * The token sum is split into 32-row slices whose column sums (ws: m3_retrieval_signature_ws_bytes bytes) are added in
 * slice order by a second launch; no atomics, so a row's bits depend on its own tokens only (not on B or its position).
 *
 * Top-k: score(q, n) = <qsig[q], db[n]> in fp32 with an order fixed by C alone.  Query q sees database rows [0, N), or
 * [0, N + q) with causal = 1 (a batch of queries whose signatures are rows N, N+1, ... of the same buffer: each sees
 * only the rows inserted before it).  Per query: idx [Q,k] int32 and score [Q,k] fp32 in descending score, equal
 * scores to the LARGER row index first (a reversed stable ascending argsort), count [Q] int32 = number kept
 * (<= min(k, rows seen)); with use_thresh = 1 only scores > min_thresh are kept.  Unused slots: idx -1, score 0.
 * qsig [Q,ldq], db [>= N (+Q-1), ldd] fp32, 16-byte aligned, ldq / ldd multiples of 4; 1 <= k <= 64; C <= 8192
 * (else M3_ERR_UNSUPPORTED).  ws: m3_retrieval_ws_bytes(N, Q, k, causal) bytes, 16-byte aligned.  Two launches:
 * per-row-block scores and partial top-k, then a per-query merge. */
enum { M3_RETRIEVAL_BF16 = 0, M3_RETRIEVAL_F16 = 1, M3_RETRIEVAL_F32 = 3 };
int64_t m3_retrieval_signature_ws_bytes(int B, int T, int C);
int m3_retrieval_signature(const void *feat, float *sig, int64_t sig_stride, float *ws, int64_t ws_bytes, int B, int T,
                           int C, int dtype, void *stream);
int64_t m3_retrieval_ws_bytes(int N, int Q, int k, int causal);
int m3_retrieval_topk(const float *qsig, int64_t ldq, const float *db, int64_t ldd, int N, int Q, int C, int k,
                      int use_thresh, float min_thresh, int causal, int32_t *count, int32_t *idx, float *score, void *ws,
                      int64_t ws_bytes, void *stream);

/* ----------------------------------------------------------------- map export */

/* Dense map export (slam.py:320-415 _get_results / save_pointcloud).  Host side: mast3r_slam/export.py.
 *
 * K keyframes share a point count N and arrive as DEVICE tables with one entry per keyframe: X[k] -> float [N,3]
 * canonical points, C[k] -> float [N] summed confidence, img[k] -> the colour image, poses [K,8] (t, q xyzw, s),
 * Nk [K] int32 fusion counts.  Source point (k, n) is kept when C[k][n] / (float)Nk[k] > thresh (IEEE fp32 divide,
 * strict, NaN fails; use_thresh = 0 skips this test) and all three components of the world point s R X + t are finite.
 * Kept points are written in ascending source index k * N + n:
 *   points float [M,3], colors uint8 [M,3], and when the pointers are not NULL index int64 [M] (the source index) and
 *   conf float [M] (the average confidence, the input of the voxel stage).
 * layout M3_MAP_IMG_F32_CHW: img[k] is float [3,N] planes, colour = (uint8)floorf(min(max(v, 0), 1) * 255.0f), NaN -> 0;
 * M3_MAP_IMG_U8_HWC: img[k] is uint8 [N,3], passed through.  16-byte loads are used per keyframe when N % 4 == 0 and
 * its arrays are 16-byte aligned; any other input takes scalar loads, with the same result.
 *
 * m3_map_export_count: two launches (kept points per 1024-point workgroup tile, then an exclusive scan in one
 * workgroup).  Afterwards the first int32 of ws is M - the one value the host has to read - and the rest holds the
 * tile offsets.  m3_map_export_scatter: one launch with the SAME inputs, threshold and ws, M as read back (>= 1; the
 * host launches nothing when M = 0) and outputs of exactly M rows.  No launch count depends on K.  Output positions
 * come from the scan, never from an atomic counter: two calls give identical bytes.
 * ws: m3_map_export_ws_bytes(K, N) bytes (0 = unsupported shape: K * N must stay below 2^31), 16-byte aligned.
 *
 * Voxel thinning of an exported cloud (points / conf / colors / index as written above, M rows): the voxel of a point
 * is floorf(p / voxel_size) per axis (correctly rounded fp32 divide); per occupied voxel the point with the largest
 * confidence survives, equal confidences (-0 = +0) go to the smaller row, a NaN confidence ranks below every number;
 * survivors keep their order.  A point with |voxel coordinate| >= 2^20 on any axis does not fit the 3 x 21-bit key: it
 * is dropped and counted.  m3_map_voxel_count: clears an open-addressing table of m3_map_voxel_table_slots(M) 64-bit
 * keys (claimed with atomicCAS) and values (confidence key << 32 | ~row, raised with atomicMax), inserts, counts the
 * winners per tile and scans.  Afterwards ws int32 [0] = M2 (survivors) and [1] = dropped points.  Integer atomics
 * commute, so the result is reproducible bit for bit.  m3_map_voxel_scatter: one launch, M2 as read back (>= 1),
 * outputs of exactly M2 rows; index may be NULL (index_out then receives the row number in the input cloud), index_out
 * may be NULL.  ws: m3_map_voxel_ws_bytes(M) bytes, 16-byte aligned; 1 <= M < 2^31. */
enum { M3_MAP_IMG_F32_CHW = 0, M3_MAP_IMG_U8_HWC = 1 };
int64_t m3_map_export_ws_bytes(int K, int N);
int m3_map_export_count(const float *const *X, const float *const *C, const float *poses, const int32_t *Nk, int K, int N,
                        int use_thresh, float thresh, void *ws, int64_t ws_bytes, void *stream);
int m3_map_export_scatter(const float *const *X, const float *const *C, const void *const *img, const float *poses,
                          const int32_t *Nk, int K, int N, int use_thresh, float thresh, int layout, const void *ws,
                          int64_t ws_bytes, int64_t M, float *points, uint8_t *colors, int64_t *index, float *conf,
                          void *stream);
int64_t m3_map_voxel_table_slots(int64_t M);
int64_t m3_map_voxel_ws_bytes(int64_t M);
int m3_map_voxel_count(const float *points, const float *conf, int64_t M, float voxel_size, void *ws, int64_t ws_bytes,
                       void *stream);
int m3_map_voxel_scatter(const float *points, const uint8_t *colors, const int64_t *index, int64_t M, const void *ws,
                         int64_t ws_bytes, int64_t M2, float *points_out, uint8_t *colors_out, int64_t *index_out,
                         void *stream);

/* ------------------------------------------------------------------ map mesh */

/* Triangle mesh of the keyframe map.  Host side: mast3r_slam/export.py collect_mesh.
 *
 * The map arrives as for m3_map_export_*: device tables X[k] -> float [N,3] (points in the keyframe's own camera frame),
 * C[k] -> float [N], img[k]; poses [K,8], Nk [K], layout M3_MAP_IMG_*; N = H * W in row-major order.  stride s >= 1,
 * edge_ratio > 0 (fp32), the export's use_thresh / thresh.
 *
 *   grid        vertices at pixels (gy * s, gx * s), gy < Hg = ceil(H / s), gx < Wg = ceil(W / s); source index
 *               k * N + (gy * s) * W + gx * s.  Cells (gy, gx), gy < Hg - 1, gx < Wg - 1, corners a = (gy, gx),
 *               b = (gy, gx + 1), c = (gy + 1, gx), d = (gy + 1, gx + 1)
 *   triangles   t = 0 is (a, c, b), t = 1 is (b, c, d), in this order: counter-clockwise seen from the keyframe's
 *               camera (x right, y down, z forward); the diagonal is always b - c
 *   valid       the export rule: C[k][n] / (float)Nk[k] > thresh (strict, NaN fails; use_thresh = 0 skips it) and the
 *               world point s R X + t finite, as the exporter computes it
 *   edge (p,q)  on the camera-frame points, fp32, every operation separately rounded: dx = p.x - q.x, ...,
 *               l2 = (dx*dx + dy*dy) + dz*dz, r2 = (x*x + y*y) + z*z per vertex, t2 = edge_ratio * edge_ratio; passes
 *               iff l2 <= t2 * fminf(r2_p, r2_q) (a NaN on either side fails; no square root)
 *   kept        a triangle: its three vertices valid and its three edges pass; a vertex: referenced by a kept triangle
 *   outputs     vertices float [V,3] (world points, the exporter's bytes), colors uint8 [V,3] (the export's colour
 *               rule), index int64 [V] (source index; may be NULL) in ascending source index; faces int32 [F,3], rows of
 *               the vertex arrays, in ascending (k, gy, gx, t)
 *
 * m3_mesh_count: three launches (two bits per cell from LDS-staged vertex rows and kept triangles per row segment of
 * 256 cells; used vertices per 1024-point tile; an exclusive scan of both).  Afterwards ws int32 [0] = V and [1] = F: the
 * host reads both in one copy.  m3_mesh_scatter: two launches (vertices, which also write the vertex -> row remap into
 * ws; faces, which read it) with the SAME inputs and ws, V and F as read back (both >= 1: the host launches nothing
 * when F = 0) and outputs of exactly V and F rows.  m3_mesh_launches() = 5 whatever K, H, W and the content are.  No
 * allocation, no host synchronisation and no atomics: positions are tile / segment offset + rank inside it, so two
 * calls give identical bytes, and a keyframe's faces depend on the other keyframes only through the row offset.
 * 16-byte loads are used per keyframe when stride = 1, N % 4 == 0 and its arrays are 16-byte aligned; any other input
 * takes scalar loads, with the same result.
 * ws: m3_mesh_ws_bytes(K, H, W, stride) bytes (0 = unsupported: K * H * W and 2 * K * (Hg-1) * (Wg-1) must stay below
 * 2^31), 16-byte aligned, contents ignored on entry: int32 [4] header, the vertex tile and face segment offsets, int32 remap
 * per grid vertex, one byte per cell.  K = 0, Hg < 2 or Wg < 2: m3_mesh_count only writes V = F = 0 (the tables may then
 * be NULL).  M3_ERR_INVALID_ARG for NULL pointers, stride < 1, edge_ratio not > 0 (NaN included) or a short ws. */
int64_t m3_mesh_ws_bytes(int K, int H, int W, int stride);
int m3_mesh_launches(void);
int m3_mesh_count(const float *const *X, const float *const *C, const float *poses, const int32_t *Nk, int K, int H, int W,
                  int stride, int use_thresh, float thresh, float edge_ratio, void *ws, int64_t ws_bytes, void *stream);
int m3_mesh_scatter(const float *const *X, const float *const *C, const void *const *img, const float *poses,
                    const int32_t *Nk, int K, int H, int W, int stride, int use_thresh, float thresh, float edge_ratio,
                    int layout, void *ws, int64_t ws_bytes, int64_t V, int64_t F, float *vertices, uint8_t *colors,
                    int32_t *faces, int64_t *index, void *stream);

/* ------------------------------------------------------------- map rendering */

/* Headless renderer of the keyframe map.  Host side: mast3r_slam/render.py.
 *
 * The map arrives as for m3_map_export_*: device tables X / C / img with one entry per keyframe, poses [K,8], Nk [K],
 * layout M3_MAP_IMG_*; K = 0 draws the background (the tables may then be NULL).  The camera is view_pose, 8 floats
 * (t, q xyzw, s) of T_WC in DEVICE memory, read by the kernel, and a pinhole (fx, fy, cx, cy) of an Hv x Wv image.
 *
 *   candidate(k, n)  <=>  the export rule: C[k][n] / (float)Nk[k] > thresh (use_thresh = 0 skips it) and the world
 *                         point p = s R X + t finite (fp32, as the exporter computes it)
 *   camera point     c = (R_v^T (p - t_v)) * (1 / s_v): the nine entries of R_v^T (quaternion formula, no
 *                         normalisation) and 1 / s_v are formed in float64 per workgroup and rounded to fp32; then
 *                         d = p - t_v, c.x = ((r00 d.x + r01 d.y) + r02 d.z) * inv_s, ... separately rounded
 *   kept             <=>  near < c.z < far (strict, NaN fails)
 *   pixel            px = floorf((fx * (c.x / c.z) + cx) + 0.5f), py likewise: integer coordinates are pixel centres
 *   footprint        the point_size x point_size square centred on (px, py), every pixel of it inside the image
 *   winner per pixel the smallest key (bits of c.z as uint32) << 32 | (k * N + n): nearest, ties to the smaller index
 *   outputs          rgb uint8 [Hv,Wv,3] (the winner's colour by the export's colour rule, else bg), depth float
 *                    [Hv,Wv] (c.z of the winner, else +inf), index int64 [Hv,Wv] (k * N + n, else -1; may be NULL)
 *
 * m3_render_launches(K) launches are queued (3: clear, splat, resolve; 2 for K = 0), whatever K is; there is no host
 * synchronisation and no allocation, so the call can be captured into a graph.  The only atomics are 64-bit unsigned
 * minima on the key buffer: the bytes of every output are the same on every call.
 * ws: m3_render_ws_bytes(Hv, Wv) = Hv * Wv * 8 bytes (0 = unsupported: 1 <= Hv, Wv <= 16384), 16-byte aligned, contents
 * ignored on entry.  K * N < 2^31 as for the export; point_size 1, 3, 5 or 7; fx, fy > 0; 0 <= near < far (far may be
 * +inf); bg_* in 0 ... 255. */
int64_t m3_render_ws_bytes(int Hv, int Wv);
int m3_render_launches(int K);
int m3_render_map(const float *const *X, const float *const *C, const void *const *img, const float *poses,
                  const int32_t *Nk, int K, int N, int use_thresh, float thresh, int layout, const float *view_pose,
                  float fx, float fy, float cx, float cy, int Hv, int Wv, float near, float far, int point_size, int bg_r,
                  int bg_g, int bg_b, void *ws, int64_t ws_bytes, uint8_t *rgb, float *depth, int64_t *index,
                  void *stream);

/* ------------------------------------------------------------ mesh rendering */

/* Triangle rasteriser for the meshes.  Host side: mast3r_slam/render.py render_mesh.
 *
 * The mesh arrives as m3_mesh_scatter and the surface extraction write it: vertices float [V,3] (world), colors uint8
 * [V,3], faces int32 [F,3] (rows of the vertex arrays).  The camera is as for m3_render_map: view_pose, 8 floats of T_WC
 * in DEVICE memory, and a pinhole (fx, fy, cx, cy) of an Hv x Wv image.  S = 256 sub-pixel steps, guard band G = 16384.
 *
 *   vertex           c as m3_render_map's camera point; ok <=> near < c.z < far (strict, NaN fails);
 *                    u = fx * (c.x / c.z) + cx, v likewise; in_guard <=> |u| <= G and |v| <= G;
 *                    sx = (int)floorf(u * 256 + 0.5f), sy likewise.  Every operation is a separately rounded fp32 one
 *   drawn face       its three indices lie in [0, V) (any other face is skipped and never dereferenced), its vertices are
 *                    ok and in_guard, and A = (bx-ax)(cy-ay) - (by-ay)(cx-ax) != 0 (int64 on sx, sy).  cull = 1 also drops
 *                    A > 0: with y down that is clockwise on the screen, so the counter-clockwise faces of m3_mesh_*
 *                    seen from their keyframe (A < 0) stay.  There is NO clipping: a face with a vertex behind near,
 *                    beyond far or outside the guard band is dropped whole
 *   coverage         b and c are swapped when A < 0.  E_i = (qx-px)(Y-py) - (qy-py)(X-px) for the edge p -> q from vertex
 *                    i+1 to vertex i+2 at the pixel centre (X, Y) = (256 x, 256 y), in int64.  Covered <=> for every i:
 *                    E_i > 0, or E_i == 0 and the edge is top-left (dy < 0, or dy == 0 and dx > 0)
 *   depth            l_i = (float)E_i / (float)A, iz_i = 1.0f / z_i, w = (l_0 iz_0 + l_1 iz_1) + l_2 iz_2, z = 1.0f / w
 *   winner per pixel the smallest key (bits of z as uint32) << 32 | face index: nearest, ties to the smaller face index
 *   colour           m_i = l_i * iz_i * z on the E_i of the winner, recomputed exactly; per channel
 *                    floorf(((m_0 c_0 + m_1 c_1) + m_2 c_2) + 0.5f) clamped to 0 ... 255: smooth shading only
 *   outputs          rgb uint8 [Hv,Wv,3] (else bg), depth float [Hv,Wv] (else +inf), index int64 [Hv,Wv] (the face index,
 *                    else -1; may be NULL)
 *
 * m3_raster_launches(F) launches are queued (4: clear, project, raster, resolve; 2 for F = 0), whatever V and F are; there
 * is no host synchronisation and no allocation, so the call can be captured into a graph.  The only atomics are 64-bit
 * unsigned minima on the key buffer: the bytes of every output are the same on every call.  A face whose screen-clipped
 * bounding box holds more than 64 pixels is walked by a whole wave in 8 x 8 blocks, any other by one lane; a mesh of fewer
 * than 262 k faces shares the rows of blocks of its large faces among up to 64 slices of workgroups of the same launch.
 * ws: m3_raster_ws_bytes(V, Hv, Wv) = V * 16 + Hv * Wv * 8 rounded up to 16 bytes (0 = unsupported: the view limits of
 * m3_render_ws_bytes, 0 <= V <= 2^31 - 1), 16-byte aligned, contents ignored on entry: a 16-byte record per vertex and the
 * dense key buffer.  0 <= F <= 2^31 - 1; V = 0 or F = 0 draws the background (vertices / colors, or faces / view_pose,
 * may then be NULL); cull 0 or 1; fx, fy > 0; 0 <= near < far (far may be +inf); bg_* in 0 ... 255. */
int64_t m3_raster_ws_bytes(int64_t V, int Hv, int Wv);
int m3_raster_launches(int64_t F);
int m3_raster_mesh(const float *vertices, const uint8_t *colors, const int32_t *faces, int64_t V, int64_t F,
                   const float *view_pose, float fx, float fy, float cx, float cy, int Hv, int Wv, float near, float far,
                   int cull, int bg_r, int bg_g, int bg_b, void *ws, int64_t ws_bytes, uint8_t *rgb, float *depth,
                   int64_t *index, void *stream);

/* ------------------------------------------------------- multi-view consistency */

/* Geometric consistency of the keyframe map across keyframes.  Host side:
 * mast3r_slam/consistency.py.
 *
 * The map arrives as for m3_map_export_*: device tables X[k] -> float [N,3] (points in the keyframe's own camera frame)
 * and C[k] -> float [N], poses [K,8] and Nk [K] in DEVICE memory, N = H * W pixels in row-major order.  (fx, fy, cx, cy)
 * is the pinhole of that grid, integer coordinates are pixel centres.  nbr int32 [K,V] names the keyframes each
 * keyframe is checked against, -1 = none; 0 <= V <= 255 (V = 0: nbr may be NULL).
 *
 *   observation plane  D[j][m] = X[j][m].z when point (j, m) passes the export's confidence test (C[j][m] / (float)Nk[j]
 *                      > thresh, fp32 divide, strict, NaN fails; use_thresh = 0 skips it), that z is finite and
 *                      z > z_min; otherwise NaN.  X is in j's camera frame: this is j's observed depth at pixel m
 *   candidate(k, n)    the export rule: the confidence test and a finite world point p = s R X + t (fp32, as the
 *                      exporter computes it).  A non-candidate has support = conflict = 0 and is not kept
 *   per slot v         j = nbr[k][v]; skipped when j < 0, j >= K or j == k.  c = (R_j^T (p - t_j)) * (1 / s_j) by the
 *                      renderer's formula (the nine entries of R_j^T and 1 / s_j formed in float64 from poses[j] and
 *                      rounded to fp32; then separately rounded fp32 operations).  Skipped unless c.z > z_min (strict,
 *                      NaN fails).  px = floorf((fx * (c.x / c.z) + cx) + 0.5f), py likewise; skipped unless
 *                      0 <= px < W and 0 <= py < H (compared as floats).  d = D[j][py * W + px]; NaN: skipped.
 *                      fabsf(c.z - d) <= depth_rtol * d: support += 1; else c.z < d: conflict += 1 (j saw through the
 *                      point); else nothing (the point is occluded in j)
 *   kept               candidate and support >= min_views and (max_conflicts < 0 or conflict <= max_conflicts)
 *   outputs            support uint8 [K,N], conflict uint8 [K,N], conf float [K,N] = C[k][n] when kept, else -inf
 *
 * m3_consistency_launches() = 3 launches are queued on `stream` (inverse poses, observation planes, count) whatever K,
 * N and V are; K = 0 queues nothing.  No allocation, no host synchronisation, no atomics and no floating-point
 * reduction: the call can be captured into a graph and the bytes of every output are the same on every call; a
 * keyframe's rows depend on itself and the keyframes its row of nbr names, nothing else.  16-byte loads are used per
 * keyframe when N % 4 == 0 and its arrays are 16-byte aligned; any other input takes scalar loads, with the same result.
 * ws: m3_consistency_ws_bytes(K, N) bytes (64 per keyframe for the inverse poses, then the planes; 0 = unsupported: K * N
 * must stay below 2^31), 16-byte aligned, contents ignored on entry.  support and conflict 4-byte aligned, conf 16-byte
 * aligned.  M3_ERR_INVALID_ARG for NULL pointers, V outside 0 ... 255, depth_rtol outside (0, 1), a negative or NaN
 * z_min, min_views < 0, max_conflicts < -1, a side beyond 2^24, fx / fy not positive and finite or a short ws. */
int64_t m3_consistency_ws_bytes(int K, int N);
int m3_consistency_launches(void);
int m3_consistency(const float *const *X, const float *const *C, const float *poses, const int32_t *Nk, int K, int H, int W,
                   int use_thresh, float thresh, float fx, float fy, float cx, float cy, const int32_t *nbr, int V,
                   float z_min, float depth_rtol, int min_views, int max_conflicts, void *ws, int64_t ws_bytes,
                   uint8_t *support, uint8_t *conflict, float *conf, void *stream);

/* ----------------------------------------------------------- volumetric fusion */

/* TSDF fusion of the keyframe map and one surface mesh from it.  Host side:
 * mast3r_slam/fusion.py.  The map arrives as for m3_consistency (device tables X, C, img, poses [K,8] and Nk [K] in
 * DEVICE memory, layout M3_MAP_IMG_*, N = H * W in row-major order, the pinhole of that grid).
 *
 * Integration rule.
 * Inputs: the keyframe tables (X float32 [K,N,3] in each keyframe's own camera frame, C float32 [K,N], img, poses
 * float32 [K,8], N_k), the common grid H x W (N = H * W), a pinhole (fx, fy, cx, cy) of that grid, thr (or none), z_min,
 * and a volume: origin fp32 [3], voxel size vs > 0, trunc > 0 and dims Dx, Dy, Dz, each in 2 ... 1024 with
 * Dx * Dy * Dz <= 2^30.
 *   observation plane   D[j][m] = X_j[m].z when point (j, m) passes the exporter's confidence test (C / N_j > thr: fp32
 *                       divide, strict, NaN fails; thr none: no test), that z is finite and z > z_min; otherwise NaN.
 *                       This is exactly step 1 of the consistency rule.
 *   voxel (iz, iy, ix)  centre p.x = origin.x + ((float)ix + 0.5f) * vs, likewise y and z.  It holds sum = 0.f, n = 0
 *                       and the colour sums r = g = b = 0, cn = 0 as uint32.
 *   for j = 0 .. K-1    in ascending order, every keyframe:
 *                       c = view_point(view_inverse(T_j), p) as in view_dev.h.  Skip unless c.z > z_min (strict, NaN
 *                       fails).
 *                       px = floorf((fx * (c.x / c.z) + cx) + 0.5f), py likewise.  Skip unless 0 <= px < W and
 *                       0 <= py < H, compared as floats before converting to int.
 *                       d = D[j][py * W + px].  Skip if d is NaN.
 *                       sdf = (d - c.z) * s_j, s_j the pose's scale in fp32 (camera units to world units).  Skip unless
 *                       sdf >= -trunc: the voxel is occluded in j.
 *                       t = fminf(sdf / trunc, 1.f); sum += t; n += 1.  A voxel far in front of the surface counts as
 *                       free space with t = 1: this carves away floating outliers.
 *                       If sdf <= trunc: add the colour of pixel (py, px) of keyframe j (the export's colour rule:
 *                       uint8 passed through, float (uint8)floorf(min(max(v, 0), 1) * 255.0f)) to r, g, b; cn += 1.
 *   outputs             tsdf float32 [Dz,Dy,Dx] = sum / (float)n, or 1.f when n == 0; weight int32 [Dz,Dy,Dx] = n;
 *                       color uint8 [Dz,Dy,Dx,3] = (2 * r + cn) / (2 * cn) in integer division per channel, or 0 when
 *                       cn == 0; colored uint8 [Dz,Dy,Dx] = (cn > 0), the bit the extraction's colour rule needs.
 * Every fp32 operation is separately rounded, and the divides are IEEE.
 * The sdf is projective (along z) with nearest-pixel depth; the pointmap is treated as a depth image of the pinhole (the
 * consistency filter's approximation, exact when the points lie on the rays of the pinhole); weights are counts, not
 * confidences.
 *
 * Extraction rule (naive surface nets).
 * Inputs: tsdf, weight, color, colored, origin, vs and min_weight >= 1.
 *   valid voxel         weight >= min_weight.       inside voxel: tsdf < 0 (strict: a value of 0 is outside).
 *   cell (z, y, x)      for z < Dz-1, y < Dy-1, x < Dx-1, with the 8 corner voxels (z+dz, y+dy, x+dx).  Active iff all 8
 *                       corners are valid and are neither all inside nor all outside.
 *   vertex              one per active cell, in ascending (z, y, x).  Walk the 12 cell edges - the 4 x-edges by
 *                       (dz,dy) = (0,0),(0,1),(1,0),(1,1); then the 4 y-edges by (dz,dx); then the 4 z-edges by (dy,dx)
 *                       - and add the crossing point of every edge whose ends differ in "inside" to acc = 0 (per
 *                       component, in that order).  An edge from corner a to b = a + e_d has tt = Fa / (Fa - Fb); its
 *                       crossing point is a's 0/1 offsets as floats, with tt along d.  local = acc / (float)count;
 *                       world.x = origin.x + (((float)x + 0.5f) + local.x) * vs, likewise y and z.  Colour per channel:
 *                       the rounded integer mean over the corners with colored set, (2 * sum + m) / (2 * m), or 0 when
 *                       there is none.
 *   faces               visit every grid edge from voxel (z, y, x) along d, d in the order x, y, z.  It yields faces when
 *                       its ends differ in "inside" and its four surrounding cells all exist and are active: cells
 *                       (z-1..z, y-1..y, x) for d = x, (z-1..z, y, x-1..x) for d = y, (z, y-1..y, x-1..x) for d = z.
 *                       With (u, v, d) right-handed - d=x: (y,z), d=y: (z,x), d=z: (x,y) - the cells at (du,dv) =
 *                       (-1,-1),(0,-1),(0,0),(-1,0) are q0..q3.  First end inside: (q0,q1,q2),(q0,q2,q3); otherwise
 *                       (q3,q2,q1),(q3,q1,q0).  Face normals then point to the free-space side.  Faces come in
 *                       ascending (z, y, x, d, triangle).
 *   outputs             vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3] (rows of the vertex arrays).
 *
 * m3_tsdf_integrate: m3_tsdf_integrate_launches() = 3 launches are queued on `stream` (inverse poses, observation planes,
 * one thread per voxel) whatever K >= 1 and the dims are; K = 0 queues the voxel kernel alone, which writes the
 * unobserved volume (tsdf 1, weight 0, colour 0; the tables and ws may then be NULL).  No allocation, no host
 * synchronisation, no atomics and no floating-point reduction across threads: the call can be captured into a graph and
 * the bytes of every output are the same on every call.  colored may be NULL (not written).
 * ws: m3_tsdf_integrate_ws_bytes(K, N) bytes (64 per keyframe for the inverse poses, then K * N floats of planes;
 * 0 = K == 0 or unsupported: K * N must stay below 2^31), 16-byte aligned, contents ignored on entry.
 *
 * m3_tsdf_extract_count: three launches (the flag byte of every voxel - valid, inside, active cell - and the active
 * cells per workgroup of 256 consecutive voxels; face-yielding edges per workgroup; an exclusive scan of both).
 * Afterwards ws int32 [0] = V and [1] = F / 2 (the face-yielding edges): the host reads both in one copy.
 * m3_tsdf_extract_scatter: two launches (vertices, which also write the cell -> row remap into ws; faces, which read it)
 * with the SAME volume, min_weight and ws, V and F as read back (V >= 1, F >= 2: the host launches nothing when
 * F = 0).  m3_tsdf_extract_launches() = 5 whatever the dims and the content are.  colored NULL: every voxel counts as
 * coloured.  Positions are workgroup offset + rank inside it, never an atomic counter: two calls give identical bytes.
 * ws: m3_tsdf_extract_ws_bytes(Dx, Dy, Dz) bytes, 16-byte aligned, contents ignored on entry: int32 [4] header, two int32
 * offset tables of ceil(Dx*Dy*Dz / 256) entries (each padded to 16 bytes), int32 remap per voxel, one flag byte per voxel
 * (padded to 16).  0 = unsupported: edges are counted in int32, so 3 * Dx * Dy * Dz must stay below 2^31.
 *
 * M3_ERR_INVALID_ARG, before any HIP call, for NULL pointers, a dim outside 2 ... 1024 or more than 2^30 voxels, a
 * non-finite origin, voxel_size or trunc (or one that is not > 0), a negative or NaN z_min, fx / fy not positive and
 * finite, min_weight < 1, an odd F, a misaligned or short ws, or tsdf / weight / vertices / faces not 4-byte aligned. */
int64_t m3_tsdf_integrate_ws_bytes(int K, int N);
int m3_tsdf_integrate_launches(void);
int m3_tsdf_integrate(const float *const *X, const float *const *C, const void *const *img, const float *poses,
                      const int32_t *Nk, int K, int H, int W, int use_thresh, float thresh, int layout, float fx, float fy,
                      float cx, float cy, float z_min, float ox, float oy, float oz, float voxel_size, float trunc, int Dx,
                      int Dy, int Dz, void *ws, int64_t ws_bytes, float *tsdf, int32_t *weight, uint8_t *color,
                      uint8_t *colored, void *stream);
int64_t m3_tsdf_extract_ws_bytes(int Dx, int Dy, int Dz);
int m3_tsdf_extract_launches(void);
int m3_tsdf_extract_count(const float *tsdf, const int32_t *weight, int Dx, int Dy, int Dz, int min_weight, void *ws,
                          int64_t ws_bytes, void *stream);
int m3_tsdf_extract_scatter(const float *tsdf, const int32_t *weight, const uint8_t *color, const uint8_t *colored, float ox,
                            float oy, float oz, float voxel_size, int Dx, int Dy, int Dz, int min_weight, void *ws,
                            int64_t ws_bytes, int64_t V, int64_t F, float *vertices, uint8_t *colors, int32_t *faces,
                            void *stream);

/* ------------------------------------------------------------ mesh components */

/* Connected components of a triangle mesh, and the clean-up that keeps the large ones.  Host side:
 * mast3r_slam/components.py.  The reference has no counterpart: this rule is the contract, and tests/components_twin.py
 * restates it in numpy.
 *
 * The input is a mesh as collect_mesh / extract_surface return it:
 *   - vertices float32 [V,3],
 *   - colors uint8 [V,3],
 *   - faces int32 [F,3], each entry a row of the vertex arrays.
 *
 * Connectivity.  Connectivity is by row, never by position.  Two vertices are connected when a valid face names both.
 * Two vertices at the same coordinates but in different rows are not connected.
 *
 * Valid faces.  A face is valid when its three rows lie in [0, V).
 *   - An invalid face connects nothing and is never kept.
 *   - Invalid faces are counted.  The host raises ValueError when the count it reads back is non-zero.
 *   - A face that names one row twice is valid.  It connects its rows and counts as a face.
 *
 * Labels.  label[v] (int32) is the smallest row in the component of v.  A vertex named by no valid face is its own
 * component with 0 faces.
 *
 * Face counts.
 *   - faces_of[c] is the number of valid faces whose first row lies in component c.
 *   - largest is the maximum of faces_of.
 *   - The winner is the component that attains largest.  On a tie the smaller label wins.
 *
 * Kept components.  A component is kept when all of these hold:
 *   - faces_of >= max(1, min_faces).
 *   - min_fraction == 0, or (double)faces_of >= (double)min_fraction * (double)largest.  Here min_fraction is an fp32
 *     argument in [0, 1].  The test is one IEEE double multiply and one compare, exactly what the twin does in numpy
 *     float64.
 *   - largest_only == 0, or the component is the winner.
 *
 * Outputs.
 *   - The kept vertices are the vertices of kept components.  They come out in ascending input row, with their colours
 *     as passed.
 *   - The kept faces are the valid faces of kept components.  They come out in ascending input face row, rewritten to
 *     the new vertex rows.
 *   - Optional: the input vertex row (int64 [V2]) and the input face row (int64 [F2]).
 *
 * Two calls give identical bytes.
 *
 * Left out.  Component area and any float criterion are out.  A float sum over atomics is not reproducible, and face
 * counts are enough for both mesh sources.
 *
 * m3_mesh_components_label: six launches (parent[v] = v; one thread per face hooks the roots of its two edges, the larger
 * under the smaller, with a compare-and-swap on parent - lock-free, nobody waits for another thread's store, and a
 * stale load only makes the compare-and-swap fail; label[v] = root(v); valid faces per component with int32 atomicAdd;
 * the winner with one 64-bit atomicMax of count << 32 | ~label; the header and faces_of_out).  F = 0 skips the two
 * launches that have one thread per face.  labels_out int32 [V] and faces_of_out int32 [V] (the count of each vertex's
 * component) may be NULL.  Afterwards ws int32 [4] = the components with at least one face, [5] = largest, [6] = the
 * winner's label (-1 when there is no valid face), [7] = the invalid faces.
 * m3_mesh_components_count, with the ws of a label call and the SAME V, F and faces: three launches (kept vertices and
 * kept faces per tile of 256 rows, one exclusive scan of both).  Afterwards ws int32 [0] = V2 and [1] = F2: the host
 * reads words 0 ... 7 in one copy.  largest and the winner are read from ws on the device.  V = 0 or F = 0: V2 = F2 = 0
 * are written and nothing is launched.
 * m3_mesh_components_scatter, with the same ws, mesh and V2, F2 as read back (both >= 1: the host launches nothing when
 * F2 = 0): two launches (vertices, which also write the old row -> new row remap into ws; faces, which read it).  The
 * filter is the one the count left in ws.  vertex_rows_out int64 [V2] and face_rows_out int64 [F2] may be NULL.
 * m3_mesh_components_launches() = 11 = 6 + 3 + 2, whatever V, F and the content are.  No allocation and no host
 * synchronisation: label and count can be captured into a graph.  The atomics are integer and commute, and output rows
 * are tile offset + rank, never an atomic counter.
 * ws: m3_mesh_components_ws_bytes(V, F) = 64 + pad(4 * ceil(V / 256)) + pad(4 * ceil(F / 256)) + 4 * pad(4 * V) bytes,
 * pad rounding up to 16 (0 = unsupported: 0 <= V, F <= 2^31 - 1), 16-byte aligned, contents ignored on entry of label:
 * int32 [16] header, the two offset tables, then parent, label, count and remap, int32 [V] each.
 * M3_ERR_INVALID_ARG, before any HIP call, for NULL pointers (faces may be NULL when F = 0), negative sizes, min_fraction
 * outside [0, 1] or NaN, largest_only other than 0 or 1, V2 outside 1 ... V, F2 outside 1 ... F, a misaligned ws or (label)
 * a short one. */
int64_t m3_mesh_components_ws_bytes(int64_t V, int64_t F);
int m3_mesh_components_launches(void);
int m3_mesh_components_label(const int32_t *faces, int64_t V, int64_t F, void *ws, int64_t ws_bytes, int32_t *labels_out,
                             int32_t *faces_of_out, void *stream);
int m3_mesh_components_count(void *ws, int64_t V, int64_t F, const int32_t *faces, int min_faces, float min_fraction,
                             int largest_only, void *stream);
int m3_mesh_components_scatter(const float *vertices, const uint8_t *colors, const int32_t *faces, int64_t V, int64_t F,
                               void *ws, int64_t V2, int64_t F2, float *vertices_out, uint8_t *colors_out, int32_t *faces_out,
                               int64_t *vertex_rows_out, int64_t *face_rows_out, void *stream);

/* --------------------------------------------------------------- mesh normals */

/* Per-vertex normals of a triangle mesh, and vertex colours lit with them.  Host side:
 * mast3r_slam/normals.py.  The reference has no counterpart: this rule is the contract, and tests/normals_twin.py
 * restates it in numpy.  The rule is Open3D's - unit face normals, equal weights - with the sum made reproducible by
 * doing it in integers.  Every fp32 and float64 operation below is rounded on its own (no fused multiply-add).
 *
 * Face f = (i0, i1, i2) with vertices a, b, c (rows i0, i1, i2 of vertices float32 [V,3]):
 *   e1 = b - a, e2 = c - a                                            (fp32)
 *   n  = (e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x)
 *   len2 = (n.x * n.x + n.y * n.y) + n.z * n.z
 * A face contributes nothing when
 *   - an index lies outside [0, V) (nothing is dereferenced for such a face), or
 *   - len2 is not finite or len2 < 2^-80: a repeated index, zero area, a NaN or infinite vertex.  With this threshold
 *     no result depends on how subnormal numbers are treated.
 * Every other face contributes u = n / sqrtf(len2) as q_k = (int64) rintf(u_k * 16777216.0f) (round to nearest even;
 * the scaling by 2^24 is exact).  q is added to three int64 sums of each of the face's three vertices.  Integer adds
 * commute, so the sums depend neither on the order of the faces nor on the order of the threads.
 *
 * Vertex v with sums (x, y, z):
 *   - all three 0 (no face names it, only degenerate faces do, or the contributions cancel exactly): normal (0, 0, 0);
 *   - otherwise x, y, z are converted to float64, L = sqrt((x * x + y * y) + z * z), normal_k = (float)(s_k / L).
 * The conversions to float64 are exact while fewer than 2^29 faces share one vertex (|sum| < 2^29 * 2^24 = 2^53).
 *
 * m3_mesh_normals: three queued operations whatever V and F are (clear the sums; one thread per face, 64-bit integer
 * atomic adds in global memory; one thread per vertex).  normals float32 [V,3].  V = 0 or F = 0 is valid; with F = 0 all
 * normals are 0.  No allocation, nothing read back: the call can be captured into a graph, and two calls give identical
 * bytes.  m3_mesh_normals_launches() = 3.
 * ws: m3_mesh_normals_ws_bytes(V) = max(16, 24 * V rounded up to 16) bytes (0 = unsupported: 0 <= V <= 2^31 - 1),
 * 16-byte aligned, contents ignored on entry: int64 [3][V], a plane per component.
 *
 * m3_mesh_shade: one launch, one thread per vertex, fp32.  out uint8 [V,3] from vertices float32 [V,3], normals float32
 * [V,3] and colors uint8 [V,3] (NULL: the constant albedo_r, albedo_g, albedo_b, each 0 ... 255).  c_k is the colour
 * channel as a float, n the normal, p the vertex.
 *   mode 0 (lambert):
 *     l = eye - p with eye = view_pose[0 ... 2] read on the device (light 0, the headlight; view_pose is a Sim(3) pose
 *         t, q xyzw, s as the rasteriser takes it), or the constant (lx, ly, lz) (light 1: the world direction from the
 *         surface towards the light)
 *     d = ((n.x * l.x + n.y * l.y) + n.z * l.z) / sqrtf((l.x * l.x + l.y * l.y) + l.z * l.z)
 *     d = fabsf(d) when two_sided
 *     d = d > 0 ? fminf(d, 1) : 0                                      (a NaN gives 0)
 *     I = ambient + (1 - ambient) * d                                  (1 - ambient is rounded first)
 *     out_k = clamp(floorf(c_k * I + 0.5f), 0, 255)
 *     A zero normal gets the ambient term alone.
 *   mode 1 (normals): out_k = clamp(floorf((n_k * 0.5f + 0.5f) * 255.f + 0.5f), 0, 255), a NaN giving 0: world-space
 *     normals as colours, (0, 0, 0) -> 128.  vertices, colors, view_pose and the light are not read.
 * clamp(x, 0, 255) = fminf(fmaxf(x, 0), 255).
 *
 * M3_ERR_INVALID_ARG, before any HIP call: NULL vertices / faces / normals / out where V (for faces: F) > 0, a NULL,
 * misaligned or short ws, pointers not aligned to 4 bytes, V or F outside 0 ... 2^31 - 1, ambient outside [0, 1] or
 * NaN, mode other than 0 or 1, light other than 0 or 1, two_sided other than 0 or 1, an albedo outside 0 ... 255; in mode 0
 * a NULL view_pose with light 0, and a zero or non-finite (lx, ly, lz) with light 1. */
int64_t m3_mesh_normals_ws_bytes(int64_t V);
int m3_mesh_normals_launches(void);
int m3_mesh_normals(const float *vertices, const int32_t *faces, int64_t V, int64_t F, void *ws, int64_t ws_bytes,
                    float *normals, void *stream);
int m3_mesh_shade(const float *vertices, const float *normals, const uint8_t *colors, int64_t V, const float *view_pose,
                  int light, float lx, float ly, float lz, float ambient, int two_sided, int mode, int albedo_r,
                  int albedo_g, int albedo_b, uint8_t *out, void *stream);

/* ------------------------------------------------------------- mesh simplify */

/* Mesh simplification by vertex clustering.  Host side: mast3r_slam/simplify.py.  The rule is
 * Open3D's simplify_vertex_clustering with the average made exact: one output vertex per occupied voxel, faces
 * rewritten, collapsed and repeated faces removed.  This text is the contract, and tests/simplify_twin.py restates it
 * in numpy; device and twin agree byte for byte.  Every float64 operation below is rounded on its own (no fused
 * multiply-add).
 *
 * Inputs: vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3] (each entry a row of the vertex arrays), and
 * voxel, the fp32 argument voxel_size (finite, > 0) converted to float64.  0 <= V, F <= 2^31 - 1.
 *
 * Cell of a vertex.  Per axis, for the coordinate x:
 *   t    = (double)x / voxel                                          (one float64 divide)
 *   cell = floor(t)
 *   q    = llrint((t - cell) * 2^24)                                  (round to nearest even; 0 ... 2^24)
 * A vertex is out of range when on any axis x is not finite or |cell| >= 2^20 (the limit of the point-cloud voxel
 * table).  An out-of-range vertex joins no cluster.  Such vertices are counted; they are not an error.
 *
 * Clusters.  The in-range vertices with the same cell triple form a cluster.
 *   - Its leader is the smallest input row in it.
 *   - Clusters are output in ascending leader row: in the order of first appearance in the input.
 *   - Every cluster is output, whether or not a kept face names it.
 *
 * Position and colour of a cluster of n vertices.
 *   - n = 1: the vertex's own bits and colour.  So a voxel finer than the mesh returns the vertex and colour arrays
 *     byte for byte.
 *   - n > 1, per axis: S = the integer sum of the members' q (below 2^55).
 *       mean = (double)S / ((double)n * 2^24)
 *       out  = (float)(((double)cell + mean) * voxel)
 *   - n > 1, per channel: C = the integer sum of the members' values; out = (2 C + n) / (2 n) in integer arithmetic,
 *     the rounded mean.
 *
 * Faces.
 *   - A face that names a row outside [0, V) is invalid.  Invalid faces are counted and never kept; the host raises
 *     ValueError when the count it reads back is non-zero.
 *   - Every other face is mapped to the three clusters of its rows.  It is dropped when one of its rows is out of
 *     range, and when two of its three clusters are the same.
 *   - The key of a remaining face is its triple of cluster output rows, rotated so that the smallest comes first.  A
 *     rotation keeps the orientation: two faces over the same three clusters with opposite winding have different
 *     keys.
 *   - Of the faces with the same key only the one with the smallest input row is kept.
 *   - Kept faces come out in ascending input row, written as their key.
 *
 * Outputs: vertices float32 [V2,3], colors uint8 [V2,3], faces int32 [F2,3]; optionally cluster_of int64 [V] (the
 * output row of every input vertex, -1 when it is out of range) and face_rows int64 [F2] (the input row of every kept
 * face).  Two calls give identical bytes, and so do two orders of the threads.
 *
 * Left out: quadric placement and any error-driven decimation, a target face count, normal-aware clustering, and
 * carrying vertex normals through (m3_mesh_normals recomputes them).
 *
 * m3_mesh_simplify_count: six launches (clear the tables and the header with a kernel; one thread per vertex claims
 * the slot of its cell in an open-addressing table with a 64-bit compare-and-swap, lowers the slot's leader row with
 * atomicMin and adds q, the colour and 1 to the slot's integer sums; one thread per vertex reads its leader, leaders
 * per tile of 256 rows; one thread per face claims the slot of its key in a second table that holds a face row per
 * slot - an occupied slot is compared by rebuilding the occupant's key, and an equal key lowers the row with
 * atomicMin; winning faces per tile; one exclusive scan of both counts).  Afterwards ws int32 [0] = V2, [1] = F2,
 * [2] = the out-of-range vertices, [3] = the invalid faces: the host reads them in one copy.  vertices and colors may
 * be NULL when V = 0, faces when F = 0.
 * m3_mesh_simplify_scatter, with the same ws, mesh and V2, F2 as read back: two launches (leaders write their cluster
 * and leave their output row in ws; winning faces are written as their key, and cluster_of for every input vertex).
 * voxel_size is the one the count left in ws.  vertices_out and colors_out may be NULL when V2 = 0, faces_out when
 * F2 = 0; cluster_of_out and face_rows_out may be NULL.
 * m3_mesh_simplify_launches() = 8 = 6 + 2, whatever V, F and the content are.  No allocation and no host
 * synchronisation: count and scatter can each be captured into a graph.  The atomics are integer and commute, and
 * output rows are tile offset + rank, never an atomic counter.
 * ws: m3_mesh_simplify_ws_bytes(V, F) = 64 + pad(4 * max(1, ceil(V / 256))) + pad(4 * max(1, ceil(F / 256)))
 * + 3 * pad(4 * V) + pad(4 * F) + 64 * SV + 4 * SF bytes, pad rounding up to 16, SV and SF the smallest powers of two
 * that are >= 1024 and >= 2 V, 2 F (0 = unsupported: 0 <= V, F <= 2^31 - 1), 16-byte aligned, contents ignored on entry
 * of count.
 * M3_ERR_INVALID_ARG, before any HIP call, for NULL pointers where a size is non-zero, negative sizes, a voxel_size that
 * is not finite and > 0, V2 outside 0 ... V, F2 outside 0 ... F, pointers not aligned to their element, a misaligned
 * or short ws. */
int64_t m3_mesh_simplify_ws_bytes(int64_t V, int64_t F);
int m3_mesh_simplify_launches(void);
int m3_mesh_simplify_count(const float *vertices, const uint8_t *colors, const int32_t *faces, int64_t V, int64_t F,
                           float voxel_size, void *ws, int64_t ws_bytes, void *stream);
int m3_mesh_simplify_scatter(const float *vertices, const uint8_t *colors, const int32_t *faces, int64_t V, int64_t F,
                             void *ws, int64_t ws_bytes, int64_t V2, int64_t F2, float *vertices_out, uint8_t *colors_out,
                             int32_t *faces_out, int64_t *cluster_of_out, int64_t *face_rows_out, void *stream);

/* --------------------------------------------------------------- mesh smooth */

/* Edge topology of a triangle mesh, and Laplacian / Taubin smoothing on it.  Host side:
 * mast3r_slam/smooth.py.  The filters are Open3D's filter_smooth_laplacian and filter_smooth_taubin (uniform weights)
 * with the order of every sum fixed.  This text is the contract, and tests/smooth_twin.py restates it in numpy; device
 * and twin agree byte for byte.  Every float64 operation below is rounded on its own (no fused multiply-add).
 *
 * Inputs: vertices float32 [V,3], faces int32 [F,3] (each entry a row of the vertex array).
 * 0 <= V <= 2^31 - 1 and 0 <= F <= (2^31 - 1) / 6: the adjacency holds at most 6 F entries, indexed in int32.
 *
 * Edges.
 *   - Face f with rows (a, b, c) contributes the undirected pairs {a,b}, {b,c}, {c,a}.
 *   - A pair with two equal rows is no edge.
 *   - A face that names a row outside [0, V) is invalid: it contributes nothing and is counted.
 *   - An edge is the pair (lo, hi), lo < hi, by row and never by position.
 *   - faces_of(edge) is the number of face corners that contribute it.  A repeated face counts every time, and
 *     either winding counts.
 *   - Boundary edge: faces_of == 1.  Non-manifold edge: faces_of > 2.
 *   - A boundary vertex lies on at least one boundary edge.
 *
 * Adjacency.
 *   - row(v) is the other ends of the unique edges at v, in ascending order; degree[v] is its length.
 *   - This is a CSR: off int32 [V + 1], nbr int32 [2 E], E the number of edges.
 *   - It is canonical: it depends on the set of edges, not on the order of the faces or of the threads.
 *
 * One pass with weight w.  w is an fp32 argument converted to float64.  Every vertex is computed from the positions
 * before the pass; p_v is the position of v before the pass.
 *   - If v is pinned, or a coordinate of p_v is not finite, the output is p_v bit for bit.
 *   - Otherwise walk row(v) in ascending order.  For every neighbour j whose three coordinates are finite (tested on
 *     the positions before this pass): s += (double)p_j per axis, n += 1.  s starts at 0.0.
 *   - If n == 0, the output is p_v bit for bit.
 *   - Otherwise, per axis: m = s / (double)n, out = (float)((double)p_v + w * (m - (double)p_v)).
 *
 * Methods.
 *   - laplacian (method 0): `iterations` passes with lam.
 *   - taubin (method 1): `iterations` times (a pass with lam, then a pass with mu).
 *   - 0 < lam <= 1; mu is any finite value (Open3D's defaults are lam = 0.5, mu = -0.53).  iterations >= 0;
 *     iterations = 0 returns the input's bytes.
 *   - Pinned: the boundary vertices when fix_boundary, united with the rows where the caller's mask is non-zero.  The
 *     pinned set is the same for every pass.
 *
 * Left out: cotangent and other geometric weights, smoothing of colours or normals (m3_mesh_normals recomputes
 * them), feature-preserving or bilateral filters, hole filling.
 *
 * m3_mesh_topology_build: seven launches (clear the table, the degrees and the header with a kernel; one thread per
 * face claims, for each of its three pairs, the slot of the key lo << 31 | hi in an open-addressing table with a
 * 64-bit compare-and-swap and a probe loop bounded by the table size, adds 1 to the slot's face count, and - only the
 * thread whose compare-and-swap claimed the slot - adds 1 to degree[lo] and degree[hi]; the exclusive scan of the
 * degrees in three: sums per tile of 256 rows, one scan of the tiles, tile offset + rank; one thread per face again -
 * the corner that claimed a slot writes each end into the other's row at a cursor taken with an integer add, marked
 * when the slot's count is 1, and adds to the header's counts; every row is sorted ascending - a thread per row up to 32 entries, the lanes of a wave together
 * for a longer one - and the boundary flag of its vertex is the or of its marks).  Afterwards ws int32 [0] = 2 E,
 * [1] = the boundary edges, [2] = the non-manifold edges, [3] = the invalid faces: the host reads them in one 16-byte
 * copy.  faces may be NULL when F = 0.
 * m3_mesh_smooth_launches() = 7: the launches of m3_mesh_topology_build, whatever V, F and the content are.
 * m3_mesh_topology_read: one launch; degree_out int32 [V], boundary_out uint8 [V] (0 or 1) from a built ws.
 * m3_mesh_topology_edges, with E as read back: three launches (neighbours above v per tile of 256 rows; one scan;
 * scatter at tile offset + rank).  edges_out int32 [E,2] in lexicographic (lo, hi) order, edge_faces_out int32 [E] =
 * faces_of, looked up in the table.
 * m3_mesh_smooth_passes, on a ws built from the same V and faces: one launch per pass (iterations, or 2 * iterations
 * for taubin), one thread per vertex; iterations = 0 is one copy launch.  Between passes the positions live in ws as
 * 16 bytes per vertex (x, y, z and a word that holds the finite and the pinned flag); the first pass reads vertices,
 * the last writes out, and vertices is never written.  pinned: uint8 [V] or NULL.  out must not be vertices.
 * No entry point allocates or synchronises with the host: each can be captured into a graph.  The atomics are integer
 * and commute (compare-and-swap to claim, add); no thread waits for another.  Which slot an edge lands in and
 * where in its row a neighbour first lands depend on the arrival order; nothing after the sort does.
 * ws: m3_mesh_smooth_ws_bytes(V, F) = 64 + pad(4 * ceil((V + 1) / 256)) + pad(4 * (V + 2)) + 12 * S + pad(V)
 * + pad(12 * F) + 2 * pad(24 * F) + 32 * V bytes, pad rounding up to 16, S the smallest power of two that is >= 1024 and >= 6 F (the
 * table stays at most half full) (0 = unsupported V or F), 16-byte aligned, contents ignored on entry of build.
 * M3_ERR_INVALID_ARG, before any HIP call, for NULL pointers where a size is non-zero, sizes out of range, a
 * misaligned or (build, passes) short ws, pointers not aligned to 4 bytes, E outside 0 ... 3 F, fix_boundary other
 * than 0 or 1, method other than 0 or 1, iterations < 0, lam outside (0, 1] or NaN, a mu that is not finite, and
 * out == vertices. */
int64_t m3_mesh_smooth_ws_bytes(int64_t V, int64_t F);
int m3_mesh_smooth_launches(void);
int m3_mesh_topology_build(const int32_t *faces, int64_t V, int64_t F, void *ws, int64_t ws_bytes, void *stream);
int m3_mesh_topology_read(const void *ws, int64_t V, int64_t F, int32_t *degree_out, uint8_t *boundary_out, void *stream);
int m3_mesh_topology_edges(void *ws, int64_t V, int64_t F, int64_t E, int32_t *edges_out, int32_t *edge_faces_out,
                           void *stream);
int m3_mesh_smooth_passes(const float *vertices, int64_t V, int64_t F, void *ws, int64_t ws_bytes, const uint8_t *pinned,
                          int fix_boundary, int method, int iterations, float lam, float mu, float *out, void *stream);

/* ---------------------------------------------------------------- point cloud */

/* Fixed-radius neighbourhoods of a point cloud, and the two passes on top of them: normals and the radius outlier
 * filter.  Host side: mast3r_slam/cloud.py.  This text is the contract, and tests/cloud_twin.py
 * restates it in numpy; counts and moments of device and twin agree byte for byte.  Every float64 operation below is
 * rounded on its own (no fused multiply-add).
 *
 * Inputs: points float32 [M,3], 0 <= M <= 2^30; radius, a float32 value r > 0; scale = 2^20 / (double)r, a double the
 * host computes (the device does not divide for it; an entry point refuses a scale with scale * r > 2^21).
 *
 * Finite points.  A point is finite when its three coordinates are.  A point that is not finite has no neighbours and
 * is nobody's neighbour.
 *
 * Range.  The cell of a finite point is floor((double)p / h) per axis, h = (double)r * (1 + 2^-10) (exact in float64),
 * the quotient an IEEE float64 division.  A point with a cell coordinate c, |c| >= 2^20, on some axis is out of range:
 * it is counted in the header of ws, and is treated as a point that is not finite.  The caller is expected to refuse
 * the cloud then (the Python layer raises ValueError).
 *
 * Neighbour set N(i) of a finite point i: every finite j, i itself included, with
 *     d = (double)p_j - (double)p_i per axis,  d2 = (dx dx + dy dy) + dz dz,  d2 <= (double)r * (double)r.
 * The boundary is inclusive, and duplicate points are neighbours of each other.
 *
 * Outputs per point.
 *   - count[i] = |N(i)|, int32; 0 for a point that is not finite.
 *   - moments[i], int64 [9], over N(i), from q = rint(d * scale) per axis (round half to even) as integers:
 *     sum qx, sum qy, sum qz, sum qx qx, sum qx qy, sum qx qz, sum qy qy, sum qy qz, sum qz qz; zeros where count = 0.
 * Every sum is an integer sum, so the result depends neither on the order of the threads nor on the order of the input
 * rows.  |q| <= 2^20 + 1, so no sum overflows below about 2^22 neighbours of one point; that bound is not enforced.
 *
 * Normals from count and moments, one point at a time, in float64.  n = count, S1 the first three moments, S2 the
 * symmetric matrix of the last six.
 *   - C = S2 / n - (S1 / n)(S1 / n)^T; the device forms n S2 - S1 S1^T exactly in 128-bit integers and rounds that.
 *   - The normal is a unit eigenvector of the smallest eigenvalue of C (cyclic Jacobi, a fixed number of sweeps, only
 *     + - * / sqrt), rounded to float32; eigenvalues l0 <= l1 <= l2.
 *   - count < min_points (min_points >= 1), trace(C) == 0 or a point that is not finite: normal (0,0,0), variation 0.
 *   - toward given: the normal is negated when sum_a n_a * ((double)c_a - (double)p_a) < 0, c the viewpoint of the
 *     point (toward + i * toward_stride); a zero or NaN sum leaves it.  toward NULL: the component of largest
 *     magnitude is made positive, a tie going to the lower axis.
 *   - variation = l0 / (l0 + l1 + l2) as float32 (0 on a plane, 1/3 for an isotropic blob).
 *
 * Radius filter: keep(i) <=> count[i] - 1 >= min_neighbors, min_neighbors >= 0 - the other points within r; a point
 * that is not finite has count 0 and is never kept.  Kept rows come in input order.
 *
 * k-nearest-neighbour queries and the statistical outlier filter: the m3_knn_* entry points below.  Left out: normal
 * propagation for clouds without viewpoints, per-point radii.
 *
 * m3_cloud_neighbors: m3_cloud_launches() = 7 launches whatever M and the content are (clear header, table and cell
 * counts with a kernel; one thread per point claims the slot of its cell's key - 3 x 21 bits, as the voxel pass of
 * m3_map_voxel_count packs them - with a 64-bit compare-and-swap and takes its rank in the cell with an integer add,
 * or writes its zero outputs when it has no cell; the exclusive scan of the cell counts in three - sums per tile of
 * 256 slots, one scan of the tiles, tile offset + rank; one thread per point writes (x, y, z, i) as 16 bytes at its
 * cell's start + its rank; one thread per entry of that cell-sorted list walks the 27 cells around its own with ten
 * accumulators in registers).  moments may be NULL: counts only.  Afterwards ws int32 [0] = the points out of range,
 * [1] = the points that have a cell.  The 27-cell walk is complete: see the header comment of csrc/cloud.hip.
 * m3_cloud_normals: one launch, one thread per point, no workspace.  toward float32 [3] (toward_stride 0) or [M,3]
 * (toward_stride 3) or NULL; variation float32 [M] or NULL.
 * m3_cloud_radius_count: two launches (kept rows per tile of 1024, one scan); ws int32 [2] = the kept rows M2, and
 * words [0], [1] stay as m3_cloud_neighbors left them, so that the host reads all in one 16-byte copy.
 * m3_cloud_radius_scatter with M2 as read back: one launch; points_out float32 [M2,3]; colors / colors_out uint8
 * [M,3] / [M2,3] or both NULL; index int64 [M] or NULL, index_out int64 [M2] or NULL (= index[i], or i without index);
 * rows_out int64 [M2] or NULL (= i).
 * No entry point allocates or synchronises with the host: each can be captured into a graph.  The atomics are integer
 * and commute (compare-and-swap to claim, add); no thread waits for another.  Which slot a cell lands in and the order
 * inside a cell depend on the arrival order; nothing that is output does.
 * ws: m3_cloud_ws_bytes(M) = 64 + pad(4 * ceil((S + 1) / 256)) + pad(4 * (S + 1)) + 8 * S + 3 * pad(4 * M) + 16 * M
 * bytes, pad rounding up to 16, S the smallest power of two that is >= 1024 and >= 2 M (the table stays at most half
 * full) (0 = M outside 0 ... 2^30), 16-byte aligned, contents ignored on entry of m3_cloud_neighbors.
 * M3_ERR_INVALID_ARG, before any HIP call, for NULL pointers where M is non-zero, M out of range, a misaligned or
 * short ws, pointers not aligned to their element, a radius that is not finite and > 0, a scale that is not finite
 * and > 0 or has scale * r > 2^21, toward_stride other than 0 or 3, min_points < 1, min_neighbors < 0, M2 outside
 * 0 ... M, colors without colors_out or the reverse, and index without index_out. */
int64_t m3_cloud_ws_bytes(int64_t M);
int m3_cloud_launches(void);
int m3_cloud_neighbors(const float *points, int64_t M, float radius, double scale, int32_t *count, int64_t *moments,
                       void *ws, int64_t ws_bytes, void *stream);
int m3_cloud_normals(const float *points, int64_t M, const int32_t *count, const int64_t *moments, const float *toward,
                     int toward_stride, int min_points, float *normals, float *variation, void *stream);
int m3_cloud_radius_count(const int32_t *count, int64_t M, int min_neighbors, void *ws, int64_t ws_bytes, void *stream);
int m3_cloud_radius_scatter(const float *points, const uint8_t *colors, const int64_t *index, const int32_t *count,
                            int64_t M, int min_neighbors, const void *ws, int64_t ws_bytes, int64_t M2, float *points_out,
                            uint8_t *colors_out, int64_t *index_out, int64_t *rows_out, void *stream);

/* k nearest neighbours within a radius on the same index, and the two passes on top of them: the statistical outlier
 * filter and normals over the k nearest.  Host side: mast3r_slam/cloud.py.  This text is the
 * contract, and tests/knn_twin.py restates it in numpy - brute force over all pairs, no cells; index, dist2, found, q and
 * the kept rows of device and twin agree byte for byte.  Every float64 operation is rounded on its own.
 *
 * The search is hybrid: the k nearest among the points within r.  The grid is the one above (cells of edge h =
 * r (1 + 2^-10)), so the 27 cells around a query hold every candidate; an unbounded k-NN would need ring expansion with
 * no bound on the work for an isolated point and is left out.
 *
 * Queries.  Self mode (queries NULL, Q = M): the queries are the points; row i is not its own neighbour, other rows at
 * the same position are, at distance 0.  Cross mode: queries float32 [Q,3], nothing is excluded.
 *
 * Candidates of a query q: every point j that is finite and in range (it has a cell, as above) with
 *     d = (double)p_j - (double)q per axis,  d2 = (dx dx + dy dy) + dz dz,  d2 <= (double)r * (double)r
 * - the membership test of m3_cloud_neighbors, so that in self mode the candidates of i are N(i) without i.  A query
 * that is not finite, or whose own cell coordinate floor((double)q / h) reaches +-2^20 on some axis (out of range), has
 * no candidates; the queries that are finite but out of range are counted in header word [3] (cross mode only: in self
 * mode they are the points of word [0]).
 *
 * Order.  Candidates are ordered by one unsigned 64-bit key, ascending:
 *     key = (bits(d2) & ~(2^30 - 1)) | j
 * bits(d2) the IEEE pattern of the non-negative float64 d2, its low 30 bits replaced by the row j (M <= 2^30).  That is:
 * by squared distance to its 22 leading explicit mantissa bits, ties to the lower row.  TWO CANDIDATES WHOSE d2 DIFFER
 * ONLY IN THE 30 DROPPED BITS (a relative difference below 2^-22) ARE ORDERED BY ROW, NOT BY DISTANCE.  No float32
 * conversion and no denormal takes part in the ordering; one compare decides each pair.
 *
 * Outputs per query, 1 <= k <= 64:
 *   - found int32 = min(k, number of candidates);
 *   - index int32 [Q,k]: the rows of the `found` smallest keys in ascending key order, then -1;
 *   - dist2 float32 [Q,k]: (float)d2 of those rows (d2 as above, rounded once to float32), then +inf.
 * All of it is a function of the point set and the query alone: two calls give identical bytes, and permuting the
 * point rows permutes the rows named in index and changes nothing else unless two keys tie in their distance bits.
 *
 * Moments over the k nearest (m3_knn_moments): the neighbourhood of i is i and its `found` nearest others; count =
 * found + 1 and the nine sums of q = rint(d * scale) as for m3_cloud_neighbors; count 0 and zeros for a point that is
 * not finite or out of range.  m3_cloud_normals consumes them unchanged.  Where no point has more than k others within
 * r, count and moments are those of m3_cloud_neighbors byte for byte.
 *
 * Statistical filter, in integers.  A row is complete when found == k.  For a complete row i
 *     D_e = rint(d2_e * factor), factor = 2^32 / ((double)r * (double)r) computed once by the host in float64 (d2 the
 *     float64 value recomputed as above, not dist2), s_e = floor(sqrt(D_e)) exactly (an integer check corrects the
 *     floating square root), q_i = sum of s_e over the k neighbours <= 64 * 2^16 = 2^22: the mean distance to the k
 *     nearest in units of r / (k 2^16).
 * Rows that are not complete - points that are not finite among them - have q = -1.  The device adds up n = the
 * complete rows, S1 = sum q and S2 = sum q^2 over them, S2 as two words, S2 = S2lo + 2^32 S2hi with S2lo the sum of
 * q^2 mod 2^32 and S2hi the sum of floor(q^2 / 2^32).  The host forms, in float64 from exact integers,
 *     mu = S1 / n,  var = (n S2 - S1^2) / (n (n - 1)) (0 for n < 2),  T = mu + std_ratio * sqrt(var),
 * and a row is kept <=> it is complete and q_i <= floor(T) (the device gets min(floor(T), 2^31 - 1) as `threshold`).
 * Kept rows come in input order.  Against Open3D's remove_statistical_outlier: a point with fewer than k others within
 * r is dropped and takes no part in mu and var, and distances are these integers; where every point is complete the
 * selection is Open3D's up to arithmetic.
 *
 * m3_knn_query: m3_knn_launches() = 7 launches whatever the cloud holds - the six that build the index, exactly those of
 * m3_cloud_neighbors, then one query kernel: one query per thread (self mode in the order of the cell-sorted list),
 * the k best keys in LDS, [k][threads] 64-bit words, 256 threads per workgroup for k <= 16, 128 for k <= 32, 64 above.
 * Afterwards ws int32 [0], [1] are as after m3_cloud_neighbors and [3] = the queries out of range.
 * m3_knn_moments: one launch, no workspace.  m3_knn_mean_distance: one launch; q int32 [M]; it ADDS to the header of a
 * ws that m3_knn_query has just filled (the index build cleared it): int32 [4] = n, uint64 at bytes 24, 32, 40 = S1,
 * S2lo, S2hi.  The host reads the 64-byte header once.  m3_knn_stat_count / m3_knn_stat_scatter: as
 * m3_cloud_radius_count / m3_cloud_radius_scatter with the predicate 0 <= q <= threshold; ws int32 [2] = M2.
 * No entry point allocates or synchronises with the host: each can be captured into a graph.  Every range and row read
 * from ws or index is bounds-checked: a stale ws gives wrong numbers, not a fault.
 * M3_ERR_INVALID_ARG, before any HIP call, as for the entry points above, and for k outside 1 ... 64, Q outside
 * 0 ... 2^30, queries NULL with Q != M, a factor that is not finite and > 0, threshold < 0.
 *
 * Left out: unbounded k-NN, normal propagation over a minimum spanning tree, per-point radii, cross queries sorted
 * through an index of their own. */
int m3_knn_launches(void);
int m3_knn_query(const float *points, int64_t M, float radius, const float *queries, int64_t Q, int k, int32_t *index,
                 float *dist2, int32_t *found, void *ws, int64_t ws_bytes, void *stream);
int m3_knn_moments(const float *points, int64_t M, float radius, double scale, const int32_t *index, const int32_t *found,
                   int k, int32_t *count, int64_t *moments, void *stream);
int m3_knn_mean_distance(const float *points, int64_t M, double factor, const int32_t *index, const int32_t *found, int k,
                         int32_t *q, void *ws, int64_t ws_bytes, void *stream);
int m3_knn_stat_count(const int32_t *q, int64_t M, int threshold, void *ws, int64_t ws_bytes, void *stream);
int m3_knn_stat_scatter(const float *points, const uint8_t *colors, const int64_t *index, const int32_t *q, int64_t M,
                        int threshold, const void *ws, int64_t ws_bytes, int64_t M2, float *points_out, uint8_t *colors_out,
                        int64_t *index_out, int64_t *rows_out, void *stream);

/* Registration of a source cloud onto a target cloud over Sim(3): point-to-point and point-to-plane ICP on the same index
 * (DESIGN.md section 7q).  Host side: mast3r_slam/register.py.  This text is the contract; tests/icp_twin.py restates it
 * in numpy and state, history, sums and correspondences of device and twin agree byte for byte.
 *
 * Arithmetic.  Only float64 + - * /, each rounded on its own; a unary minus is exact.  No sqrt and no transcendental
 * function takes part in an iteration.  Brackets below give the order of the operations.
 *
 * Pose.  x' = s R x + t: R double [9] row-major, t double [3], s double.  `pose` in the calls below is HOST memory,
 * double [13] = R | t | s, read before the call returns.
 *
 * Per source row i (source float32 [Ns,3]; x, y, z converted to float64):
 *     p_a = s * ((R_a0 x + R_a1 y) + R_a2 z) + t_a                          a = 0, 1, 2
 *     q32 = (float)p per axis: the search query.  The row is FINITE when the three components of q32 are.
 *   Correspondence: the k = 1 cross-mode result of m3_knn_query on the target with the query q32 - the same cells
 *   (h = r (1 + 2^-10)), the same candidates (target rows that are finite and in range with d2 <= (double)r (double)r,
 *   d = (double)target_j - (double)q32), the smallest key (bits(d2) & ~(2^30 - 1)) | j.  A row that is not finite, a
 *   finite row whose own cell coordinate reaches +-2^20 (OUT OF RANGE) and a row without candidate have no
 *   correspondence: j = -1.
 *   Residual, from the float64 p, not from q32:  e_a = p_a - (double)target_j,a.
 *
 * Terms of a contributing row: 36 values v, the upper triangle of H = J^T J row by row (H00 .. H06, H11 .. H16, ...,
 * H66: v[0 .. 27]), g = J^T residual (v[28 .. 34]) and the cost (v[35]); unknowns (tau [3], omega [3], sigma).
 *   Point to point (mode 0): every row with a correspondence contributes.  With (x, y, z) = p:
 *     H row 0:  1, 0, 0, 0, z, -y, x        row 1:  1, 0, -z, 0, x, y        row 2:  1, y, -x, 0, z
 *     H33 = y y + z z, H34 = -(x y), H35 = -(x z), H36 = 0;  H44 = x x + z z, H45 = -(y z), H46 = 0;
 *     H55 = x x + y y, H56 = 0;  H66 = (x x + y y) + z z
 *     g = e0, e1, e2, y e2 - z e1, z e0 - x e2, x e1 - y e0, (x e0 + y e1) + z e2;  cost = (e0 e0 + e1 e1) + e2 e2
 *   (J = [I | -[p]x | p] with the products by 0 and 1 carried out and z y - y z = 0.)
 *   Point to plane (mode 1): n = (double)target_normals_j.  The row contributes when the three components of the
 *   float32 normal are finite and not all zero (m3_cloud_normals writes (0,0,0) for sparse points).
 *     J = n0, n1, n2, y n2 - z n1, z n0 - x n2, x n1 - y n0, (n0 x + n1 y) + n2 z;   rho = (n0 e0 + n1 e1) + n2 e2
 *     H_uv = J_u J_v,  g_u = J_u rho,  cost = rho rho
 *   A row that does not contribute has 36 times +0.0.
 *
 * Reduction.  A tile is 256 consecutive source rows (the last one padded with rows that do not contribute).  Within a
 * tile each of the 36 sums is the pairwise tree over the slots: x = x[0::2] + x[1::2], eight times.  Per tile also three
 * integers: contributing rows (PAIRS), finite rows, rows out of range.  Second stage, 256 slots: slot j starts at +0.0
 * and adds the partials of tiles j, j + 256, j + 512, ... in ascending order; then the same tree over the 256 slots.
 * The integers are added exactly.  No float atomics: the bytes do not depend on scheduling.
 *
 * Step (mode-independent), from the 36 sums S and the pair count:
 *   n = 7 with scale, else 6 (the leading 6 x 6 block of H, sigma = 0).
 *   pairs < min_pairs:  status = 1 (too few pairs).
 *   else LDL^T without pivoting, for j = 0 .. n-1:
 *       w_k = L_jk d_k and d_j = (..((H_jj - L_j0 w_0) - L_j1 w_1) ..) - L_j,j-1 w_j-1                   k < j
 *       d_j <= 1e-12 H_jj, or d_j not finite:  status = 2 (singular), stop
 *       L_ij = ((..(H_ij - L_i0 w_0) ..) - L_i,j-1 w_j-1) / d_j                                           i > j
 *     y_i = (..((-g_i) - L_i0 y_0) ..) - L_i,i-1 y_i-1;      delta_i = (..((y_i / d_i) - L_i+1,i delta_i+1) ..) -
 *     L_n-1,i delta_n-1 for i = n-1 .. 0;  (tau, omega, sigma) = delta.
 *   status != 0: the pose stays and the iteration is finished.  Otherwise, with a = omega * 0.5,
 *     c = 2 / (1 + ((a0 a0 + a1 a1) + a2 a2)), k = 1 + sigma,
 *     D00 = 1 + c (-(a1 a1 + a2 a2)), D11 = 1 + c (-(a0 a0 + a2 a2)), D22 = 1 + c (-(a0 a0 + a1 a1)),
 *     D01 = c (a0 a1 - a2), D02 = c (a0 a2 + a1), D10 = c (a0 a1 + a2), D12 = c (a1 a2 - a0), D20 = c (a0 a2 - a1),
 *     D21 = c (a1 a2 + a0)                 (Cayley's map I + 2 / (1 + a.a) ([a]x + [a]x [a]x): orthogonal, I + [omega]x
 *                                           to first order)
 *     R_ab <- (D_a0 R_0b + D_a1 R_1b) + D_a2 R_2b;   t_a <- k ((D_a0 t_0 + D_a1 t_1) + D_a2 t_2) + tau_a;   s <- k s
 *     tt = (tau0 tau0 + tau1 tau1) + tau2 tau2, ww likewise of omega, rr = tol * (double)r;
 *     done = 1 when tt <= rr rr and ww <= tol tol and sigma sigma <= tol tol.
 *   Every iteration that ran adds 1 to `iterations run` and writes its history row: pairs, cost, tt, ww, sigma (tt = ww
 *   = sigma = 0 when status != 0).  Once done or status is set, the kernels of the remaining iterations return at once.
 *
 * Evaluation.  After the last iteration one more accumulate in mode 0 at the final pose and one reduction:
 * eval pairs and eval cost (the squared error sum).  fitness = eval pairs / finite rows and inlier_rmse =
 * sqrt(eval cost / eval pairs) are the host's.  pairs int32 [Ns], when given: the final correspondence, -1 where none.
 *
 * ws, 16-byte aligned, contents ignored on entry: the target's index (m3_cloud_ws_bytes(Nt) rounded up to 16) | state
 * double [24] | history double [iterations][5], rounded up to 16 bytes | tile partials 8 bytes [ntile][40] (36 sums,
 * int64 pairs, finite, out of range, 0), ntile = max(1, ceil(Ns / 256)).  State words: [0..8] R, [9..11] t, [12] s,
 * [13] iterations run, [14] done, [15] status, [16] pairs and [17] cost of the last iteration, [18] finite source rows and
 * [19] rows out of range of the last accumulate, [20] eval pairs, [21] eval cost, [22..23] 0.  The index header keeps
 * its meaning: int32 [0] = target points out of range.
 * m3_icp_ws_bytes(Ns, Nt, iterations): 0 for Ns or Nt outside 0 ... 2^30 or iterations outside 0 ... 1000.
 * m3_icp_launches(iterations) = 6 + 2 iterations + 2 whatever the clouds hold (0: iterations out of range): the six index
 * launches of the target, two per iteration, two for the evaluation.  Nothing allocates or synchronises: the call can be
 * captured into a graph.  Every range and row read from ws is bounds-checked: a stale ws gives wrong numbers, not a fault.
 * m3_icp_sums: the index, one accumulate at `pose` and the reduction (8 launches; ws of m3_icp_ws_bytes(Ns, Nt, 0)):
 * count int64 [3] = pairs, finite rows, rows out of range; sums double [36]; pairs int32 [Ns] or NULL - all device memory.
 * M3_ERR_INVALID_ARG, before any HIP call: a NULL pose, count or sums; source NULL with Ns > 0, target NULL with Nt > 0;
 * a misaligned pointer; a radius that is not finite and > 0; a mode other than 0, 1; mode 1 without normals (Nt > 0);
 * iterations outside 0 ... 1000; min_pairs < 1; tol not finite or < 0; with_scale other than 0, 1; a ws that is NULL,
 * short or not 16-byte aligned.
 *
 * Left out: robust kernels and trimming, a normal-compatibility gate, source rows sorted through the target's cells,
 * multi-scale radii, colour terms, global registration (FPFH, RANSAC). */
int64_t m3_icp_ws_bytes(int64_t Ns, int64_t Nt, int iterations);
int m3_icp_launches(int iterations);
int m3_icp_sums(const float *source, int64_t Ns, const float *target, const float *target_normals, int64_t Nt, float radius,
                int mode, const double *pose, int64_t *count, double *sums, int32_t *pairs, void *ws, int64_t ws_bytes,
                void *stream);
int m3_icp_register(const float *source, int64_t Ns, const float *target, const float *target_normals, int64_t Nt,
                    float radius, int mode, const double *pose, int with_scale, int iterations, double tol, int64_t min_pairs,
                    int32_t *pairs, void *ws, int64_t ws_bytes, void *stream);

/* ---------------------------------------------------------- camera intrinsics */

/* Focal length of every keyframe from its own pointmap.  Host side: mast3r_slam/intrinsics.py.
 *
 * The map arrives as for m3_map_export_*: device tables X[k] -> float [N,3] (points in the keyframe's own camera frame)
 * and C[k] -> float [N], Nk [K] int32, N = H * W pixels in row-major order.  The pinhole's principal point is (cx, cy)
 * in pixel-centre coordinates; fx = fy = f is estimated per keyframe.
 *
 *   valid(k, n)   <=>  the export rule C[k][n] / (float)Nk[k] > thresh (IEEE fp32 divide, strict, NaN fails;
 *                      use_thresh = 0 skips it), x, y, z of X[k][n] all finite, and z > z_min (strict).  No other
 *                      pixel contributes to any sum.
 *   per pixel          float64 from the fp32 inputs, every operation separately rounded:
 *                      u = (n % W) - cx, v = (n / W) - cy, a = x / z, b = y / z, pq = a u + b v, qq = a a + b b
 *   pass 0             f_0 = sum pq / sum qq                                   (the least-squares focal)
 *   pass i = 1..iters  d = sqrt((u - f a)^2 + (v - f b)^2) at f = f_{i-1}, w = 1 / (d > 1e-8 ? d : 1e-8),
 *                      f_i = sum w pq / sum w qq                               (Weiszfeld step of sum d -> min)
 *   last pass          the mean of d at f = f_iters
 *   out[k]             double [4]: f_iters, f_0, the number of valid pixels, the mean d in pixels.  No valid pixel:
 *                      (NaN, NaN, 0, NaN); a zero denominator gives what IEEE division gives; nothing is clamped.
 *
 * m3_focal_launches(iters) = iters + 3 launches are queued (iters + 2 passes over the pixels and one that finishes the
 * mean), whatever K and N are (0: iters out of range); there is no host synchronisation, no allocation and no copy, so
 * the call can be captured into a graph.  There are no floating-point atomics: a workgroup reduces a fixed tile of one
 * keyframe (4096 pixels; larger only where a keyframe would otherwise have more than 256 tiles) in a fixed order -
 * per thread in pixel order, a shuffle tree per wave, the waves in order through LDS - and stores its sums to ws; the
 * workgroups of the next pass each add their keyframe's tile sums in ascending tile order to get f.  The bytes of out
 * are therefore the same on every call, and a keyframe's row does not depend on which keyframes share the call.
 * 16-byte loads are used per keyframe when N % 4 == 0 and its arrays are 16-byte aligned; any other input takes
 * scalar loads, with the same result.
 * ws: m3_focal_ws_bytes(K, N) bytes (0 = unsupported shape: K * N must stay below 2^31 and K * tiles within 2^22),
 * 16-byte aligned, contents ignored on entry.  M3_ERR_INVALID_ARG for H * W != N, iters outside 0 ... 64, a negative
 * or NaN z_min, a non-finite cx / cy or a short ws.  K = 0 queues nothing and returns M3_OK. */
int64_t m3_focal_ws_bytes(int K, int N);
int m3_focal_launches(int iters);
int m3_focal_estimate(const float *const *X, const float *const *C, const int32_t *Nk, int K, int N, int H, int W,
                      int use_thresh, float thresh, double cx, double cy, float z_min, int iters, void *ws,
                      int64_t ws_bytes, double *out, void *stream);

/* -------------------------------------------------------------- preprocessing */

/* Frame preprocessing in front of m3_patchify16_dt (mast3r_utils.py:132-207 resize_img).  Host side:
 * mast3r_slam/preprocess.py, which builds the tables.
 *
 * src uint8 [B,Hs,Ws,3] interleaved RGB is resampled to [Hr,Wr] with the 8-bit arithmetic of Pillow's Image.resize and
 * the box [crop_y0, crop_y0 + Hc) x [crop_x0, crop_x0 + Wc) of the result is written: dst uint8 [B,Hc,Wc,3] and, when
 * img is not NULL, img float [B,Hc,Wc,3] = (v / 255.0f - 0.5f) / 0.5f (three separately rounded fp32 operations).
 * Per axis and output index o the host gives bounds[o] = (first source index, tap count n <= ksize) and n int32
 * coefficients in 2^22 fixed point; a pass is out = clamp((2^21 + sum_t src[first + t] * k[t]) >> 22, 0, 255) in int32
 * (the host guarantees 255 * sum|k| + 2^21 < 2^31 and |k| < 2^23: products are formed by the 24-bit multiplier).  The horizontal pass runs first and its result is rounded to uint8
 * before the vertical pass.  Wr == Ws / Hr == Hs: no pass on that axis, its tables are ignored (may be NULL).
 *   bounds_h int32 [Wr,2], coef_h int32 [ksize_h,Wr] (TAP-major: 64 neighbouring columns read 256 contiguous bytes
 *   per tap); bounds_v int32 [Hr,2], coef_v int32 [Hr,ksize_v] (a wave owns one output row: uniform reads).
 * One launch, no workspace, no atomics; nothing depends on the image content.  A workgroup stages the source rows of a
 * 64-column x TH-row output tile through LDS; TH (16 ... 1) and the staging depth follow from the sizes alone, and a
 * problem whose single-row tile does not fit 64 KiB of LDS is M3_ERR_UNSUPPORTED (a source edge of 8192 fits for every
 * target the host produces).  Table entries are clamped before they address anything.  src, dst and img 16-byte
 * aligned; B <= 65535; sizes <= 65536. */
int m3_resize_crop_u8(const uint8_t *src, const int32_t *bounds_h, const int32_t *coef_h, int ksize_h,
                      const int32_t *bounds_v, const int32_t *coef_v, int ksize_v, uint8_t *dst, float *img, int B, int Hs,
                      int Ws, int Hr, int Wr, int crop_x0, int crop_y0, int Hc, int Wc, void *stream);

/* Lens undistortion in front of m3_resize_crop_u8: a bilinear remap of src uint8 [B,Hs,Ws,3] through a fixed-point
 * coordinate table int32 [Ho,Wo,2] shared by the batch, dst uint8 [B,Ho,Wo,3].  Host side: mast3r_slam/camera.py,
 * which builds the table from a camera model in float64 (source coordinate times 256, rounded to nearest; integer
 * coordinates are pixel centres).  Integer arithmetic only; for the entry (qx, qy) of an output pixel
 *   ix = qx >> 8, iy = qy >> 8 (arithmetic shift = floor), a = qx & 255, b = qy & 255
 *   out = (p00 (256-a)(256-b) + p01 a (256-b) + p10 (256-a) b + p11 a b + 2^15) >> 16      per channel, in int32
 *   p00 = src[iy][ix], p01 = src[iy][ix+1], p10 = src[iy+1][ix], p11 = src[iy+1][ix+1]
 * A tap outside [0,Ws) x [0,Hs) reads `border` (0 ... 255, the same for the three channels).  The sentinel entry
 * (INT32_MIN, INT32_MIN) of a coordinate the host could not represent has every tap outside, so it writes `border`.
 * One launch, no workspace, no atomics, no host synchronisation (capturable); the bytes depend on the inputs alone.
 * A thread owns four neighbouring output pixels (two 16-byte table loads, three 4-byte stores; a row tail or a row
 * that is not suitably aligned takes a per-pixel path with the same result) and reads its taps from global memory.
 * Every tap index is clamped into the source before it addresses anything: a table that does not belong to the sizes
 * cannot move a load or a store out of its buffers.  src, table and dst 16-byte aligned; B <= 65535; sizes <= 2^20. */
int m3_remap_bilinear_u8(const uint8_t *src, const int32_t *table, uint8_t *dst, int B, int Hs, int Ws, int Ho, int Wo,
                         int border, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* M3SLAM_H */
