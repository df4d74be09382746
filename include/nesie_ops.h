/*
 * nesie_ops.h -- C ABI of libnesie_hip.so (MI355X / gfx950).
 *
 * These are the entry points the reference's pybind11 extension modules expose
 * for the VoteNet/Nesie hot path.  Each one replaces a
 * `*_wrapper` / `forward` / `backward` function of the reference; the cited
 * file:line is the reference interface it stands in for.  Conventions follow
 * the reference's: all buffers are device pointers to contiguous memory owned
 * by the caller, outputs are pre-allocated by the caller and written in place,
 * dimensions are passed redundantly as ints, and the launch is asynchronous on
 * the HIP stream given as the last argument (`hipStream_t` passed as void*;
 * NULL = the null stream).  Differences from the reference, all deliberate:
 *   - no torch types anywhere in the signatures;
 *   - every function returns 0 on success or a non-zero nesie_status, and
 *     nesie_last_error() gives a message, instead of fprintf+exit(-1)
 *     (e.g. reference group_points_cuda.cu:48-53);
 *   - every launch goes to the caller's stream (the reference launches
 *     sort_vertices and points_in_boxes on the legacy default stream).
 */
#ifndef NESIE_OPS_H_
#define NESIE_OPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  NESIE_OK = 0,
  NESIE_ERR_INVALID_ARG = 1, /* null pointer / negative or inconsistent size  */
  NESIE_ERR_UNSUPPORTED = 2, /* size outside what the kernels are built for   */
  NESIE_ERR_LAUNCH = 3       /* HIP reported a launch error (see last_error)  */
} nesie_status;

/* Library identity and diagnostics. */
int nesie_abi_version(void);
const char *nesie_last_error(void); /* thread-local, never NULL */

/* Form of the squared distance in furthest_point_sampling / ball_query / three_nn / grid_taps
 * (process-wide; default 0).  The reference writes
 *   (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1)
 * (furthest_point_sample_cuda.cu:65-66, ball_query_cuda.cu:41-42, three_nn_cuda.cu:41) and nvcc's
 * default -fmad=true may contract it; no output of that build exists to decide.
 *   0  ((dx*dx) + (dy*dy)) + (dz*dz), no contraction (the tuned kernels)
 *   1  fma(dz, dz, fma(dx, dx, dy*dy))      2  fma(dz, dz, fma(dy, dy, dx*dx))
 * Forms 1 / 2 run on the plain kernels (no bucket pruning, no spatial index; nesie_fps_leaves_index
 * then returns 0): a one-flag check against a CUDA-produced fixture, not a fast path.  The CPU
 * oracle has the same switch (oracle_set_distance_form). */
int nesie_set_distance_form(int form);
int nesie_get_distance_form(void);
/* CUs the persistent grids of the layer / weight-gradient kernels are sized for (default 256 = the
 * chip).  A caller that runs other long-lived work beside them -- the next batch's furthest point
 * sampling holds one CU per scene and XCD for milliseconds (furthest_point_sample_cuda.cu's one block
 * per batch element) -- sizes them for the CUs that are left, so that no workgroup of a one-round
 * grid waits for a CU that will not come free.  n % 8 == 0 (one XCD-balanced grid). */
int nesie_set_cu_count(int n);
int nesie_get_cu_count(void);

/* mmdet3d/ops/furthest_point_sample/src/furthest_point_sample.cpp:32-58
 * furthest_point_sampling_wrapper(b, n, m, points[B,N,3], temp[B,N], idx[B,M]).
 * temp must hold 1e10 on entry (furthest_point_sample.py:30) and holds the
 * final running-min squared distances on return.  idx[:,0] = 0. */
int nesie_furthest_point_sampling_wrapper(int b, int n, int m, const float *xyz,
                                          float *temp, int *idx, void *stream);

/* Same operator with caller-provided scratch (no reference counterpart: the
 * reference kernel needs none).  For 4096 < n <= 65536 the kernel spatially sorts
 * the scene into `workspace` and prunes whole 64-point buckets each round (results
 * bit-identical); nesie_fps_workspace_bytes() says how much it needs (0 = this
 * size runs without scratch).  workspace must be 16-byte aligned.  With a NULL or
 * short workspace this behaves exactly like nesie_furthest_point_sampling_wrapper. */
size_t nesie_fps_workspace_bytes(int b, int n);
int nesie_furthest_point_sampling_ws(int b, int n, int m, const float *xyz, float *temp,
                                     int *idx, void *workspace, size_t workspace_bytes,
                                     void *stream);

/* furthest_point_sample.cpp:59-65  furthest_point_sampling_with_dist_wrapper
 * (b, n, m, dist[B,N,N], temp[B,N], idx[B,M]). */
int nesie_furthest_point_sampling_with_dist_wrapper(int b, int n, int m,
                                                    const float *dist,
                                                    float *temp, int *idx,
                                                    void *stream);

/* mmdet3d/ops/ball_query/src/ball_query.cpp:30-47  ball_query_wrapper
 * (b, n, m, min_radius, max_radius, nsample, new_xyz[B,M,3], xyz[B,N,3],
 *  idx[B,M,nsample]).  idx must be zero on entry (ball_query.py:35). */
int nesie_ball_query_wrapper(int b, int n, int m, float min_radius,
                             float max_radius, int nsample,
                             const float *new_xyz, const float *xyz, int *idx,
                             void *stream);

/* ball_query_wrapper over the spatial index nesie_furthest_point_sampling_ws leaves in its
 * workspace (no reference counterpart; same results as nesie_ball_query_wrapper).  For sizes
 * where nesie_fps_leaves_index(b, n) != 0 the workspace holds, after the call returns, the scene
 * sorted into 64-point buckets with one bounding box each; a ball query of the SAME xyz then
 * visits only the buckets within max_radius.  nsample <= 64; NESIE_ERR_UNSUPPORTED otherwise. */
int nesie_fps_leaves_index(int b, int n);
int nesie_ball_query_indexed(int b, int n, int m, float min_radius, float max_radius,
                             int nsample, const float *new_xyz, const void *fps_workspace,
                             size_t workspace_bytes, int *idx, void *stream);

/* mmdet3d/ops/knn/src/knn.cpp  knn_wrapper
 * (b, n, m, nsample, xyz[B,N,3], new_xyz[B,M,3], idx[B,M,nsample], dist2[B,M,nsample]).
 * For every centre: the nsample points of the same scene with the smallest squared distance, the
 * distance taken in the process-wide form above (fp32, left to right, no contraction by default),
 * written in ascending order of the pair (distance, point index); dist2 receives the fp32
 * distances.  With n < nsample the remaining slots hold index 0 and distance 1e10f, the state the
 * reference's heap starts from (knn_cuda.cu:74-77); n == 0 fills both rows with that padding.
 * The reference selects with a binary heap and heap-sorts: where a centre's distances are distinct
 * that is the sorted k smallest, exactly this rule; where distances tie, its index order inside a
 * group of equal distances follows the heap's history, here it is the point index.  The dist2 rows
 * are equal in both cases.  (The reference's heap also never admits a point at d2 >= 1e10; here
 * such a point is a point like any other.)
 * nsample 1 .. 128 (the reference's arrays hold 100): nsample <= 0 or a negative size is
 * NESIE_ERR_INVALID_ARG, nsample > 128 NESIE_ERR_UNSUPPORTED; b, m or n == 0 succeeds without a
 * kernel launch. */
int nesie_knn_wrapper(int b, int n, int m, int nsample, const float *xyz,
                      const float *new_xyz, int *idx, float *dist2, void *stream);

/* mmdet3d/ops/group_points/src/group_points.cpp:31-45  forward
 * (b, c, n, npoints, nsample, points[B,C,N], idx[B,M,ns], out[B,C,M,ns]). */
int nesie_group_points_forward(int b, int c, int n, int npoints, int nsample,
                               const float *points, const int *idx, float *out,
                               void *stream);

/* group_points.cpp:47-62  backward
 * (b, c, n, npoints, nsample, grad_out[B,C,M,ns], idx, grad_points[B,C,N]).
 * grad_points must be zero on entry (group_points.py:218). */
int nesie_group_points_backward(int b, int c, int n, int npoints, int nsample,
                                const float *grad_out, const int *idx,
                                float *grad_points, void *stream);

/* QueryAndGroup's data movement in one pass (mmdet3d/ops/group_points/group_points.py:100-128
 * transposes the points, groups xyz and features separately, subtracts the centre, divides by
 * the radius and concatenates): out[B, 3+C, M, ns] = cat[(xyz[idx] - centre) / radius,
 * features[idx]]; xyz (B,N,3), centres (B,M,3), features (B,C,N) (c = 0: xyz only),
 * radius <= 0: no division.  backward: grad_features (B,C,N, zeroed) += channels 3.. of
 * grad_out (B, 3+C, M, ns), read in place (no slice copy). */
int nesie_query_and_group_forward(int b, int c, int n, int npoints, int nsample,
                                  const float *xyz, const float *centres,
                                  const float *features, const int *idx, float radius,
                                  float *out, void *stream);
int nesie_query_and_group_backward(int b, int c, int n, int npoints, int nsample,
                                   const float *grad_out, const int *idx, float *grad_features,
                                   void *stream);
/* Same result through an inverted index of idx: order[B, M*ns] = the grouped columns sorted
 * by their source point, sources[B, M*ns] = that point for each (nesie_inverted_index builds
 * both; any n: n <= 2048 by a stable counting sort in one workgroup per scene, larger n in windows
 * of 8192 source points per workgroup).  Lanes own sorted entries, a segmented scan inside each wave sums the runs;
 * every run is summed by exactly ONE wave (the one that holds its first entry follows it through
 * the next chunks) and written by one lane: no float atomics; grad_features is WRITTEN in full
 * (round 5: a point without entries gets its zero here, the caller need not clear it).  Inside a run the columns are in ascending order (scratch[B, M*ns] holds the
 * arrival-order placement that the second pass ranks), so the sums are bitwise reproducible.
 * An entry of idx outside [0, n) is clamped to the nearest point (0 or n - 1): it sorts, and appears
 * in sources, as that point.  e_total = 0 is a no-op that writes nothing. */
int nesie_inverted_index(int b, int n, long long e_total, const int *idx, int *order,
                         int *sources, int *scratch, void *stream);
/* nesie_group_points_backward / nesie_gather_points_grad_wrapper (nsample = 1) through the same
 * index: grad_points (B,C,N) = scatter of grad_out (B,C,npoints,nsample) (WRITTEN in full: the caller
 * need not clear it), every point's run summed by
 * one wave in ascending column order (replaces the atomicAdd of group_points_cuda.cu:10-31 and
 * gather_points_cuda.cu:51-70 with a defined order). */
int nesie_group_points_backward_csr(int b, int c, int n, int npoints, int nsample,
                                    const float *grad_out, const int *order, const int *sources,
                                    float *grad_points, void *stream);
int nesie_query_and_group_backward_csr(int b, int c, int n, int npoints, int nsample,
                                       const float *grad_out, const int *order,
                                       const int *sources, float *grad_features, void *stream);

/* The tail of VoteModule.forward behind its last convolution (model_utils/vote_module.py:106-147
 * with vote_per_seed = 1, with_res_feat, no vote_xyz_range): raw (B, 3+c, N) = [offset, residual]
 * -> vote_points (B, N, 3) = seed_points + offset^T, vote_feats (B, c, N) = (seed_feats + residual)
 * divided by its channel-wise L2 norm (normalise != 0), inv_norm (B, N) kept for the backward.
 * Backward: g_feats (B, c, N) / g_points (B, N, 3), either may be NULL -> d_raw (B, 3+c, N) (rows
 * 0..2 = g_points^T, rows 3.. = the gradient of seed_feats + residual). */
int nesie_vote_finish_forward(int b, int c, int n, int normalise, const float *raw,
                              const float *seed_points, const float *seed_feats, float *vote_points,
                              float *vote_feats, float *inv_norm, void *stream);
int nesie_vote_finish_backward(int b, int c, int n, int normalise, const float *g_feats,
                               const float *g_points, const float *vote_feats, const float *inv_norm,
                               float *d_raw, void *stream);

/* QueryAndGroup over NETWORK-COMPUTED coordinates (vote aggregation groups the predicted votes
 * around centres sampled from them, nesie_head.py:243 -> point_sa_module.py:122-131,
 * group_points.py:98-110): the sampled centres straight from the (B, N, 3) array, and the
 * coordinate gradient -- what autograd assembles from the backward of transpose / gather_points /
 * group_points (two atomicAdd scatters) / sub / div / cat:
 *   d_xyz[p] = (1/r) sum_{idx[e] = p} g[0:3, e] - (1/r) sum_{sample[m] = p} sum_s g[0:3, m, s]
 *              + sum_{sample[m] = p} d_centres[m]          (r = radius, 0: no division)
 * with grad_out (B, 3+c, npoints, nsample), (order, sources) = nesie_inverted_index(idx),
 * sample (B, npoints) the centres' indices, d_centres (B, npoints, 3) or NULL; d_xyz (B, N, 3) is
 * written (not accumulated), every point by one thread in a fixed order. */
int nesie_gather_rows3(int b, int n, int m, const float *xyz, const int *sample, float *centres,
                       void *stream);
int nesie_query_and_group_backward_xyz(int b, int c, int n, int npoints, int nsample, float radius,
                                       const float *grad_out, const int *order,
                                       const int *sources, const int *sample,
                                       const float *d_centres, float *d_xyz, void *stream);

/* three_interpolate_grad_wrapper through an inverted index of idx[B, n, 3] over the m known
 * points (nesie_inverted_index with e_total = 3n): grad_points[B, C, m] = scatter of
 * weight * grad_out, WRITTEN in full, no float atomics, fixed order; grad_out (B, C, n) with a free
 * batch stride (a channel slice of a wider gradient: no copy). */
int nesie_three_interpolate_grad_csr(int b, int c, int n, int m, const float *grad_out,
                                     long long grad_out_bstride, const float *weight, const int *order,
                                     const int *sources, float *grad_points, void *stream);

/* mmdet3d/ops/gather_points/src/gather_points.cpp:28-42  gather_points_wrapper
 * (b, c, n, npoints, points[B,C,N], idx[B,M], out[B,C,M]). */
int nesie_gather_points_wrapper(int b, int c, int n, int npoints,
                                const float *points, const int *idx, float *out,
                                void *stream);

/* gather_points.cpp:44-59  gather_points_grad_wrapper
 * (b, c, n, npoints, grad_out[B,C,M], idx, grad_points[B,C,N] zeroed). */
int nesie_gather_points_grad_wrapper(int b, int c, int n, int npoints,
                                     const float *grad_out, const int *idx,
                                     float *grad_points, void *stream);

/* mmdet3d/ops/interpolate/src/interpolate.cpp:46-58  three_nn_wrapper
 * (b, n, m, unknown[B,n,3], known[B,m,3], dist2[B,n,3], idx[B,n,3]).
 * Also stands in for mmcv.ops.three_nn (side_pooling_module.py:204). */
int nesie_three_nn_wrapper(int b, int n, int m, const float *unknown,
                           const float *known, float *dist2, int *idx,
                           void *stream);

/* interpolate.cpp:60-75  three_interpolate_wrapper
 * (b, c, m, n, points[B,C,M], idx[B,N,3], weight[B,N,3], out[B,C,N]). */
int nesie_three_interpolate_wrapper(int b, int c, int m, int n,
                                    const float *points, const int *idx,
                                    const float *weight, float *out,
                                    void *stream);

/* Grid points of the side-aware quality head and their 3-NN taps among the seeds, one launch
 * per grid set (dense_heads/side_pooling_module.py:87-157 builds the box-frame grid, selects
 * the faces, rotates and translates it; :204-225 finds the 3 nearest seeds and the
 * inverse-distance weights).  centre/size (B,K,3), heading (B,K), mult/plane (gp,3) = box-frame
 * multipliers of the gp grid points of a proposal and the +-10 % plane factors of the SAQE
 * variant (quelity_estimation_module.py:142-167; zeros otherwise), known (B,m,3) ->
 * idx (B,K*gp,3) i32 (three_nn_wrapper's order), weight (B,K*gp,3), rel (B,K*gp,3) = grid point
 * relative to the proposal centre. */
int nesie_grid_taps(int b, int kprop, int gp, int m, const float *centre, const float *size,
                    const float *heading, const float *mult, const float *plane,
                    const float *known, int *idx, float *weight, float *rel, void *stream);

/* The quality head's grid features in their consumer's layout, optionally folded with the
 * first 1x1 conv of the MiniPointNet that consumes them.
 * Reference: dense_heads/side_pooling_module.py:226-243 builds cat([rel_xyz, interpolated]),
 * :304-313 splits it per face and makes each face contiguous, :346-349 feeds it to
 * Conv2d(3+C, H, 1, bias=False).  The n = K*segs*seg_len queries are ordered (proposal k,
 * face s, grid point g); out is (B, segs, c_total, K*seg_len) and query (k,s,g), channel ch
 * lands at out[b, s, c_offset+ch, k*seg_len+g]:
 *     out = w0*T[j0] + w1*T[j1] + w2*T[j2]  (+ wx[s][ch] . rel[q])
 * with T = table[b, j, s*seg_off + ch], a POINT-major table of row pitch `pitch` floats.
 *   - table = seed features (B, M, C), seg_off = 0, rel = wx = NULL, c_offset = 3:
 *     three_interpolate_wrapper's values (bit-identical) in the per-face layout;
 *   - table = F . W_f^T (seed features times the feature columns of each face's first conv,
 *     (B, M, segs*H), seg_off = H) and wx = the conv's xyz columns (segs, H, 3): the first
 *     conv's OUTPUT, W . cat[rel, blend(F)] = W_xyz . rel + blend(W_f . F) by linearity.
 * backward (second form): dy (B, segs, c, K*seg_len) = the gradient of out; ADDS into
 * d_table (B, M, pitch) columns [s*seg_off, +c) (zeroed by the caller) and WRITES
 * d_wx (B, R, segs, c, 3), R = nesie_blend_conv_runs(n, segs), one partial sum of dy x rel per
 * workgroup for the caller to add up (NULL = skip); c in
 * {64, 128, 192, 256} and K*seg_len % 64 == 0.  Sum order is not fixed (float atomics), like
 * the reference's scatter.  Channels outside [c_offset, c_offset+c) of out are left
 * untouched by the forward. */
int nesie_blend_conv_forward(int b, int c, int m, int n, const float *table, int pitch,
                             int seg_off, const int *idx, const float *weight,
                             const float *rel, const float *wx, float *out, int segs,
                             int seg_len, int c_total, int c_offset,
                             float *stat_partial /* NULL, or [segs*c][B*K*seg_len/64][2]: (sum,
                             sum of squares) per 64-query tile for nesie_bn_relu_forward's
                             pre_partial */, void *stream);
int nesie_blend_conv_runs(int n, int segs);
int nesie_blend_conv_backward(int b, int c, int m, int n, const float *dy, int pitch, int seg_off, const int *idx, const float *weight,
                              const float *rel, float *d_table, float *d_wx, int segs,
                              int seg_len, void *stream);
/* The same backward when the blend's output Z (B, segs, c, n/segs) is followed by a training
 * BatchNorm + ReLU (MiniPointNet.first_conv[1:3], side_pooling_module.py:346-348): da is the
 * gradient of relu(bn(Z)) and the norm backward's apply pass runs on the tile load with
 * bnb [segs*c][8] from nesie_pw_bnb_coef (the partial sums come from the launch that produced da,
 * nesie_pw_dgrad_bn_reduce) -- the pass that read (da, Z) and wrote dZ disappears. */
int nesie_blend_conv_backward_bn(int b, int c, int m, int n, const float *da, const float *z,
                                 const float *bnb, int pitch, int seg_off, const int *idx,
                                 const float *weight, const float *rel, float *d_table,
                                 float *d_wx, int segs, int seg_len, void *stream);

/* The two backward entry points above WITHOUT float atomics (round 4; the default of the python
 * layer since round 5): every 16-query group stores the row it has summed per seed into staging
 * slots of its own (48 per group), a counting sort per chunk of 128 groups lists each seed's slots
 * in ascending order (chunk-major, with the run starts), and one wave per (scene, face, seed) walks
 * the chunks, adds its rows in that order and WRITES the d_table row -- bitwise reproducible,
 * d_table needs no zero fill.  Needs m <= 2047 seeds, pitch and seg_off multiples of 4, d_table
 * 16-byte aligned.  z / bnb both NULL: plain
 * backward; both given: the norm backward on the tile load (as nesie_blend_conv_backward_bn).
 * d_wx as above.  workspace: nesie_blend_conv_backward_workspace_bytes(b, c, n, segs) bytes. */
size_t nesie_blend_conv_backward_workspace_bytes(int b, int c, int n, int segs);
int nesie_blend_conv_backward_staged(int b, int c, int m, int n, const float *dy, const float *z,
                                     const float *bnb, int pitch, int seg_off, const int *idx,
                                     const float *weight, const float *rel, float *d_table,
                                     float *d_wx, int segs, int seg_len, void *workspace,
                                     size_t workspace_bytes, void *stream);
/* The same backward for ANY shape, without float atomics: any c >= 1 (no 64-channel blocks, no
 * upper bound), any number of queries per face, any m >= 1, any pitch >= (segs - 1) * seg_off + c
 * (no multiple of 4, no alignment beyond a float's), segs >= 1; b = 0 is a no-op, n = 0 writes
 * zeros.  dy (B, segs, c, n/segs), idx / weight / rel (B, n, 3) in (proposal, face, grid point)
 * order; idx values outside [0, m) are clamped as the forward clamps them.  z / bnb both NULL:
 * plain backward; both given: the norm backward on the load (as nesie_blend_conv_backward_bn).
 * A transposing pass stores dZ^T (B, segs, n/segs, c) query-major, nesie_inverted_index sorts the
 * scene's 3n taps by seed, and one wave per (scene, face, seed, 256 channels) WRITES
 *     d_table[b, j, s * seg_off + ch] = sum over the taps (p, t) of face s with idx[b, p, t] = j,
 *                                       in ASCENDING tap position 3p + t, of weight[b,p,t] * dZ[p, ch]
 * starting from 0 (the product rounded, then added): every element of the columns
 * [s * seg_off, + c), s < segs, of every row is written exactly once (zero for a seed without
 * taps), so with seg_off == c or segs == 1 the caller need not clear d_table.
 * d_wx (segs, c, 3) (NULL = skip) is WRITTEN with the final sum of dy x rel: per (scene, run of
 * 1024 queries of a face) the queries in four interleaved groups of 16 per 64-tile, ascending, the
 * groups added as (0 + 1) + (2 + 3), then the partials in ascending (scene, run) order.
 * Both orders depend on the shape and idx alone: two launches give the same bits.
 * workspace: nesie_blend_conv_backward_any_workspace_bytes(b, c, m, n, segs) bytes, 4-byte aligned;
 * no host synchronisation, so the launch sequence captures into a graph. */
size_t nesie_blend_conv_backward_any_workspace_bytes(int b, int c, int m, int n, int segs);
int nesie_blend_conv_backward_any(int b, int c, int m, int n, const float *dy, const float *z,
                                  const float *bnb, int pitch, int seg_off, const int *idx,
                                  const float *weight, const float *rel, float *d_table,
                                  float *d_wx, int segs, int seg_len, void *workspace,
                                  size_t workspace_bytes, void *stream);
/* out[g * c + ch] = sum over the batch entries n = g (mod ng) and the p positions of x[n][ch][pos];
 * x (nb, c, p) with batch stride x_bstride >= c * p (a channel slice of a wider tensor is fine).
 * The bias gradient of a convolution without a norm behind it (autograd's grad.sum((0, 2)) for the
 * nn.Conv1d outputs of reliable_conv_bbox_module.py:144-177, vote_module.py:75-79,
 * side_pooling_module.py:55-78; ng = the S stacked nets of the quality head); one workgroup per
 * (group, channel), fixed summation order. */
int nesie_channel_sum(int nb, int ng, int c, long long p, const float *x, long long x_bstride,
                      float *out, void *stream);

/* bnb[ch] = (scale, shift, a, mean, d1, e0, -, -) of a BatchNorm + ReLU backward from the partial
 * sums part [(channels) * nslots * 2] = (sum g, sum g zhat), the folded forward coefficients
 * z_coef [channels][4] and gamma; count = elements per channel; dgamma / dbeta written. */
int nesie_pw_bnb_coef(int channels, int nslots, double count, const float *part,
                      const float *z_coef, const float *gamma, float *bnb, float *dgamma,
                      float *dbeta, void *stream);

/* interpolate.cpp:77-93  three_interpolate_grad_wrapper
 * (b, c, n, m, grad_out[B,C,N], idx, weight, grad_points[B,C,M] zeroed). */
int nesie_three_interpolate_grad_wrapper(int b, int c, int n, int m,
                                         const float *grad_out, const int *idx,
                                         const float *weight,
                                         float *grad_points, void *stream);

/* mmdet3d/ops/rotated_iou/cuda_op/sort_vert.cpp:6-30  sort_vertices_forward
 * (vertices[B,N,M,2] f32, mask[B,N,M] bool(1 byte), num_valid[B,N] i32)
 * -> idx[B,N,9] i32.  The reference allocates idx; here the caller does. */
int nesie_sort_vertices_forward(int b, int n, int m, const float *vertices,
                                const uint8_t *mask, const int *num_valid,
                                int *idx, void *stream);

/* mmdet3d/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:46-48 /
 * points_in_boxes_cuda.cu:153-181  points_in_boxes_batch
 * (boxes[B,T,7] LiDAR frame bottom-centre, pts[B,M,3], out[B,M,T] i32 zeroed). */
int nesie_points_in_boxes_batch(int b, int boxes_num, int pts_num,
                                const float *boxes, const float *pts, int *out,
                                void *stream);

/* points_in_boxes_cuda.cu:51-77, :116-151  points_in_boxes_gpu
 * (boxes[B,T,7], pts[B,M,3], out[B,M] i32): the index of the FIRST box of the scene that holds the
 * point under the same test, else -1.  WRITTEN in full (the reference pre-fills -1), also with
 * boxes_num == 0.  A negative size is NESIE_ERR_INVALID_ARG; b or pts_num == 0 succeeds without a
 * launch. */
int nesie_points_in_boxes_gpu(int b, int boxes_num, int pts_num, const float *boxes,
                              const float *pts, int *out, void *stream);

/* mmdet3d/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu  roiaware_pool3d forward / backward
 * (the size arguments in the order of its launchers, :228-275 / :343-364, plus pts_num and the
 * membership table).
 *   rois[N,7] LiDAR frame (x, y, z_bottom, w, l, h, rz), pts[P,3], pts_feature[P,C] fp32,
 *   (out_x, out_y, out_z) each 1 .. 256, m = max_pts_each_voxel >= 1, pool_method 0 = max, 1 = avg.
 * In-box test and local coordinates (:14-44): the test of nesie_points_in_boxes_batch, exactly --
 *   cos / sin of (float)(rz + pi/2) evaluated in double and rounded to float, products and sums
 *   fp32 without contraction, the z window |z - (z_bottom + h/2)| <= h/2 and the half extents
 *   compared in double; x / y strict, z inclusive (csrc/pib_test.h is the one device copy).
 * Voxel of an inside point (:65-78), all fp32 with IEEE division: x_res = l / out_x,
 *   y_res = w / out_y, z_res = h / out_z; x_idx = trunc((local_x + l/2) / x_res),
 *   y_idx = trunc((local_y + w/2) / y_res), z_idx = trunc((pts.z - rois.z) / z_res), each clamped
 *   into [0, out - 1].
 * Collection (:93-127): per voxel the inside points in ascending point index, only the first
 *   m - 1 kept.  pts_idx_of_voxels[N,ox,oy,oz,m] i32: slot 0 = the kept count, slots 1 .. count =
 *   the indices, the rest 0.  pts_voxel[N,P] i32 (no reference output; its pts_mask, :45-91, after
 *   the capacity rule): the flat voxel (x_idx * oy + y_idx) * oz + z_idx in which the box KEEPS the
 *   point, else -1.  The backward gathers through it; it may be null when no backward follows.
 * Max pool (:129-187): per voxel and channel over the kept points in slot order with strict >
 *   starting from -inf (the lowest index wins a tie); argmax[N,ox,oy,oz,C] = that point, -1 for a
 *   voxel without a kept point (or none above -inf); pooled = the maximum, 0 where argmax == -1.
 * Avg pool (:189-226): an fp32 running sum in slot order divided by the count; 0 for an empty
 *   voxel; argmax is written 0 (the reference leaves its zero fill).
 * pooled[N,ox,oy,oz,C], argmax, pts_idx_of_voxels and pts_voxel are WRITTEN in full.
 * Backward (:277-341): max: grad_in[argmax, c] += grad_out; avg: grad_in[p, c] += grad_out *
 *   (1 / max(count, 1)) for every kept point, the product rounded to fp32 before the add.  The
 *   reference adds with float atomics; here every grad_in[p, c] is the sum of its contributions in
 *   ascending (box, voxel) order, without contraction, by one thread: no float atomics in either
 *   setting of the deterministic switch.  grad_in[P,C] is WRITTEN in full.
 * No entry allocates, every launch goes on the given stream.  nesie_roiaware_pool3d_sizes:
 *   out[0] = elements of pts_idx_of_voxels, out[1] = of pooled / argmax, out[2] = of pts_voxel.
 * A negative size, m < 1 or another pool_method is NESIE_ERR_INVALID_ARG; an out_* outside
 * 1 .. 256 NESIE_ERR_UNSUPPORTED.  N, P or C == 0 succeeds without a kernel launch and clears
 * whatever output is not empty (zeros; pts_voxel -1). */
int nesie_roiaware_pool3d_sizes(int boxes_num, int pts_num, int channels, int out_x, int out_y,
                                int out_z, int max_pts_each_voxel, long long *out);
int nesie_roiaware_pool3d_forward(int boxes_num, int pts_num, int channels,
                                  int max_pts_each_voxel, int out_x, int out_y, int out_z,
                                  const float *rois, const float *pts, const float *pts_feature,
                                  int *argmax, int *pts_idx_of_voxels, float *pooled_features,
                                  int *pts_voxel, int pool_method, void *stream);
int nesie_roiaware_pool3d_backward(int boxes_num, int pts_num, int out_x, int out_y, int out_z,
                                   int channels, int max_pts_each_voxel,
                                   const int *pts_idx_of_voxels, const int *argmax,
                                   const int *pts_voxel, const float *grad_out, float *grad_in,
                                   int pool_method, void *stream);

/* Max over the neighbourhood axis of a grouped tensor: x[rows, nsample] -> out[rows],
 * argmax[rows] (one byte, smallest index on ties).  No extension entry in the reference:
 * it calls ATen's F.max_pool2d(kernel=[1, nsample]) (point_sa_module.py:149-150) and
 * torch.max(dim=-1) (side_pooling_module.py:361,368); same values, same tie rule.
 * nsample must be a power of two in 4..64; x / grad_x 16-byte aligned. */
int nesie_group_max_pool_forward(long long rows, int nsample, const float *x, float *out,
                                 uint8_t *argmax, void *stream);
int nesie_group_max_pool_backward(long long rows, int nsample, const float *grad_out,
                                  const uint8_t *argmax, float *grad_x, void *stream);
/* grad_x[row, argmax[row]] += grad_out[row] into an existing dense gradient (a tensor that
 * feeds both the max and another consumer: MiniPointNet's f, side_pooling_module.py:359-365). */
int nesie_group_max_pool_backward_add(long long rows, int nsample, const float *grad_out,
                                      const uint8_t *argmax, float *grad_x, void *stream);

/* Same-class LHS-NMS of the teacher's pseudo boxes, on the device: boxes[B,K,8] f32 =
 * axis-aligned (x1,y1,z1,x2,y2,z2,score,class), K <= 64; keep[B,K] u8 = 1 for every box
 * the reference's lhs_3d_faster_samecls returns in `pick`
 * (models/detectors/votenet_nesie.py:733-779; the reference runs it in numpy on the host). */
int nesie_lhs_nms_samecls(int b, int k, const float *boxes, float thr, uint8_t *keep,
                          void *stream);

/* Rotated 3-D IoU of n box pairs (x, y, z, dx, dy, dz, yaw; rotation about z only) with the
 * Jacobian w.r.t. the 7 parameters of box1 (jac may be NULL: value only).  One kernel for
 * the reference's torch chain cal_iou_3d -> cal_iou -> oriented_box_intersection_2d ->
 * sort_v (rotated_iou/oriented_iou_loss.py:86-109, box_intersection_2d.py:13-184), same
 * formulas, masks and vertex order; box2 is treated as a constant. */
int nesie_iou3d_forward(int n, const float *box1, const float *box2, float *iou, float *jac,
                        void *stream);

/* oriented_iou_loss.py:112-152  cal_giou_3d / cal_diou_3d, one launch.
 * kind 0: GIoU loss = 1 - iou3d + (v_c - u3d) / v_c,            v_c = z_range * w * h
 * kind 1: DIoU loss = 1 - iou3d + d2 / c2,  c2 = w*w + h*h + z_range*z_range, d2 = |centre1 - centre2|^2
 * enclosing 0: "smallest" (min_enclosing_box.py:142-172), 1: "aligned" (oriented_iou_loss.py:166-194)
 * loss[n], iou[n] (may be NULL), jac[n,7] = d loss / d box1 (may be NULL: values only); box2 constant.
 * iou3d, u3d and z_range = max(zmax) - min(zmin), clamped at 0, are those of cal_iou_3d(verbose=True):
 * the same per-pair chain as nesie_iou3d_forward, and iou[] holds its bits.  (w, h) of "smallest" is
 * the reference's brute force over its 24 candidate hull edges in fp32 and in its order of
 * operations (slope (y2-y1)/(x2-x1+1e-8), projection range over all 8 corners, distance range over
 * the other 6 with sqrt(dy^2+dx^2+1e-14), area + 1e8 where it is exactly 0, first minimum); max,
 * min and arg-min are piecewise constant in the Jacobian, as autograd treats them.
 * A negative n, an unknown kind or enclosing, or a null box1 / box2 / loss with n > 0 is
 * NESIE_ERR_INVALID_ARG; n == 0 succeeds without a launch. */
int nesie_giou3d_forward(int n, const float *box1, const float *box2, int kind, int enclosing,
                         float *loss, float *iou, float *jac, void *stream);

/* mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py:201-320  axis_aligned_bbox_overlaps_3d
 * (AxisAlignedBboxOverlaps3D :170-198; the loss of models/losses/axis_aligned_iou_loss.py:9-25 and
 * of iou3d_loss.py:21-35 is 1 - the paired form).  Boxes are corners (x1, y1, z1, x2, y2, z2), f32,
 * rows 8-byte aligned.  mode 0: IoU = overlap / max(area1 + area2 - overlap, eps), overlap the
 * product of clamp(min(hi) - max(lo), 0); mode 1: GIoU = IoU - (enclose - union) / enclose with
 * enclose = max(prod(clamp(max(hi) - min(lo), 0)), eps).  Same operations in the same order as the
 * reference, products and sums rounded separately.  Derivatives are those torch autograd takes of
 * that function: clamp(x, 0) passes the gradient where x >= 0 (x == 0 included), a max / min of two
 * equal arguments gives each side one half, max(., eps) likewise.
 *   paired  (is_aligned=True) : out[n]; jac1[n,6] = d out / d box1, jac2[n,6] = d out / d box2,
 *           either may be NULL.
 *   matrix  (is_aligned=False): box1 (b,m,6), box2 (b,n,6), out (b,m,n); the reference's leading
 *           batch dimensions flattened to b.
 *   matrix backward: grad1 (b,m,6) = sum over n, grad2 (b,n,6) = sum over m of grad_out (b,m,n)
 *           times the recomputed Jacobian, either may be NULL; every sum runs in a fixed order
 *           (lane-strided partials, then a fixed tree), without atomics: the same bits every run.
 * A negative size, a mode outside {0, 1}, or a null box1 / box2 / out / grad_out (or a row pointer
 * that is not 8-byte aligned) with a positive count is NESIE_ERR_INVALID_ARG; n == 0 (matrix:
 * b * m * n == 0) succeeds without a launch and touches nothing. */
int nesie_aa_iou3d_paired_forward(int n, const float *box1, const float *box2, int mode, float eps,
                                  float *out, float *jac1, float *jac2, void *stream);
int nesie_aa_iou3d_matrix_forward(int b, int m, int n, const float *box1, const float *box2,
                                  int mode, float eps, float *out, void *stream);
int nesie_aa_iou3d_matrix_backward(int b, int m, int n, const float *box1, const float *box2,
                                   int mode, float eps, const float *grad_out, float *grad1,
                                   float *grad2, void *stream);

/* Training-mode BatchNorm with an optional fused ReLU over x[B, C, P] (statistics per
 * channel over B*P; biased variance for normalisation, unbiased for running_var, as
 * torch.nn.BatchNorm{1,2}d).  No extension entry in the reference: it builds
 * conv -> BN -> ReLU from mmcv ConvModule / nn.BatchNorm + nn.ReLU
 * (point_sa_module.py:277-289, side_pooling_module.py:55-78,346-358).
 * forward : y = relu?(gamma * (x - mean) * invstd + beta); writes save_mean/save_invstd
 *           [C] and updates running_mean/var [C] in place (NULL = skip) with `momentum`.
 * backward: dx, dgamma [C], dbeta [C] from dy, x, y (y only read when relu != 0) and the
 *           forward's fwd_coef [C,4] = (scale, bias, mean, invstd).
 * row_bias (NULL = none): the normalised input is x[b,c,i] + row_bias[b,c,i/group] with
 *           row_bias[B, C, P/group] -- the per-proposal half of side_pooling_module.py:359-368's
 *           second_conv input (the max-pooled global feature repeated over the `group` grid
 *           points of a proposal), added on the fly instead of materialising the repeat+concat;
 *           group must be a power of two in 4..256.  backward writes d_row_bias (same shape)
 *           = sum of dx over each group.
 *           group == 0: row_bias[C] is ONE value per channel -- the bias of the convolution in
 *           front (mmcv ConvModule with bias=True and a norm: vote_module.py / base_conv_bbox_head),
 *           added in registers with the rounding of the separate add.  Its gradient is identically
 *           zero (the mean subtraction removes it): d_row_bias must be NULL.
 * workspace: nesie_bn_workspace_bytes(b, c, p) bytes, 16-byte aligned tensors. */
size_t nesie_bn_workspace_bytes(int b, int c, long long p);
int nesie_bn_relu_forward(int b, int c, long long p, const float *x, const float *gamma,
                          const float *beta, float *running_mean, float *running_var,
                          float momentum, float eps, int relu, float *y, float *save_mean,
                          float *save_invstd, float *fwd_coef /* [C,4] out */,
                          const float *row_bias, int group,
                          const float *pre_partial /* NULL, or unshifted (sum, sum^2) partials
                          [C][pre_nslice][2] left by the producer of x: the statistics pass over
                          x is skipped */, int pre_nslice, void *workspace,
                          size_t workspace_bytes, void *stream);
/* y == NULL with relu != 0: the normalised tensor was never stored (nesie_pw_layer_forward applied
 * it on its operand load); the mask is fma(x, scale, bias) > 0 from fwd_coef.  d_row_bias without
 * row_bias: the per-group sums of dx (the producer had added the row term to x itself). */
int nesie_bn_relu_backward(int b, int c, long long p, const float *dy, const float *x,
                           const float *y, const float *gamma, const float *beta,
                           const float *save_mean, const float *save_invstd,
                           const float *fwd_coef /* from the forward */, int relu, float *dx,
                           float *dgamma, float *dbeta, const float *row_bias, int group,
                           float *d_row_bias, void *workspace, size_t workspace_bytes,
                           void *stream);

/* The apply pass of nesie_bn_relu_backward alone (relu, y == NULL form), for a producer that has
 * already left the reduction's partials: partial[(ch * nslice + i) * 2 + {0, 1}] = sum(g),
 * sum(g * xhat) over slice i (nesie_pw_dgrad_bn_reduce).  dgamma / dbeta are written.
 * save_invstd == NULL: column 3 of fwd_coef (also accepted by nesie_bn_relu_maxpool_backward). */
int nesie_bn_relu_backward_apply(int b, int c, long long p, const float *dy, const float *x,
                                 const float *gamma, const float *save_invstd,
                                 const float *fwd_coef, const float *partial, int nslice,
                                 float *dx, float *dgamma, float *dbeta, int group,
                                 float *d_row_bias, void *stream);

/* Synchronised training BatchNorm (+ ReLU): the norm above cut open between each local reduction
 * and its finalise step, so that the caller can put a SUM all-reduce in the cut (reference:
 * NaiveSyncBatchNorm1d/2d, mmdet3d/ops/norm.py:27-133).  x, y, dy, dx [B, C, P] fp32 of ONE rank.
 *   local_moments : moments [C][3] float64 = (n_local, sum x, sum x^2): raw moments, the one form
 *                   that adds across ranks (the fp32 partials are taken about a per-rank shift and
 *                   un-shifted in double).  The caller all-reduces `moments`.
 *   forward_apply : from the reduced moments, in double: mean = sum x / n, var = max(sum x^2 / n -
 *                   mean^2, 0), invstd = 1 / sqrt(var + eps); writes fwd_coef [C,4] = (scale, bias,
 *                   mean, invstd), y = relu?(x * scale + bias), and updates running_mean /
 *                   running_var (both NULL = skip) with the BIASED variance, as the reference does.
 *                   The statistics are those of the concatenated batch whatever the ranks' sizes
 *                   (n travels in the moments).
 *   backward_local: sums [C][2] float64 = (sum g, sum g * xhat) over this rank's positions, g = dy
 *                   masked by x * scale + bias > 0 when relu (the forward's two fp32 operations,
 *                   scale / bias from fwd_coef); dgamma, dbeta [C] fp32 (NULL = skip) are these
 *                   LOCAL sums.  The caller all-reduces `sums`.
 *   backward_apply: dx = gamma * invstd * (g - sum g / n - xhat * sum g xhat / n) from the reduced
 *                   sums and the reduced moments; the same mask expression.
 *                   Both backward passes take mean and invstd in double from the reduced moments
 *                   and `eps` (the forward's) and evaluate xhat and the closed form in double,
 *                   rounding dx once: with few positions per channel the form cancels completely.
 * Fixed summation order, no atomics, no host read of a device value.  b, c, p >= 1.  workspace:
 * nesie_syncbn_workspace_bytes(b, c, p) for the two local passes; tensors 16-byte aligned when
 * p % 4 == 0. */
size_t nesie_syncbn_workspace_bytes(int b, int c, long long p);
int nesie_syncbn_local_moments(int b, int c, long long p, const float *x, double *moments,
                               void *workspace, size_t workspace_bytes, void *stream);
int nesie_syncbn_forward_apply(int b, int c, long long p, const float *x, const double *moments,
                               const float *gamma, const float *beta, float *running_mean,
                               float *running_var, float momentum, float eps, int relu, float *y,
                               float *fwd_coef, void *stream);
int nesie_syncbn_backward_local(int b, int c, long long p, const float *dy, const float *x,
                                const float *fwd_coef, const double *moments, float eps, int relu,
                                double *sums, float *dgamma, float *dbeta, void *workspace,
                                size_t workspace_bytes, void *stream);
int nesie_syncbn_backward_apply(int b, int c, long long p, const float *dy, const float *x,
                                const float *fwd_coef, const float *gamma, const double *sums,
                                const double *moments, float eps, int relu, float *dx,
                                void *stream);

/* Training BatchNorm + ReLU + max over the neighbourhood axis for the LAST layer of a
 * set-abstraction MLP: x[B, C, M, ns] -> pooled[B, C, M] (+ argmax[B, C, M], one byte, smallest
 * index on ties) without writing the normalised tensor.  Reference: ConvModule's BN2d + ReLU
 * followed by F.max_pool2d(kernel=[1, ns]) (point_sa_module.py:277-289, 136-158); same
 * values as nesie_bn_relu_forward followed by nesie_group_max_pool_forward.
 * backward: dx[B, C, M, ns], dgamma, dbeta from grad_pooled[B, C, M], argmax, x, pooled and the
 * forward's fwd_coef.  ns a power of two in 4..64; workspace =
 * nesie_bn_workspace_bytes(b, c, m * ns). */
int nesie_bn_relu_maxpool_forward(int b, int c, int m, int ns, const float *x,
                                  const float *gamma, const float *beta, float *running_mean,
                                  float *running_var, float momentum, float eps, float *pooled,
                                  uint8_t *argmax, float *save_mean, float *save_invstd,
                                  float *fwd_coef, void *workspace, size_t workspace_bytes,
                                  void *stream);
int nesie_bn_relu_maxpool_backward(int b, int c, int m, int ns, const float *grad_pooled,
                                   const uint8_t *argmax, const float *x, const float *pooled,
                                   const float *gamma, const float *save_invstd,
                                   const float *fwd_coef, float *dx, float *dgamma,
                                   float *dbeta, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* NesieHead.side2box + Integral + the bbox_probs softmax (dense_heads/nesie_head.py:19-52,
 * 150-209, 255-257), one thread per proposal.  reg (B, 6*bins+2, K) channel-major = the
 * regression branch's output (6 sides x bins logits, then the (sin, cos)-like heading pair);
 * agg (B, K, 3) aggregated points; scale / sign [6].
 *   forward : probs (B, 6, bins, K) = per-side softmax; surface (B, K, 6) = agg +- E[bin] * scale;
 *             bbox (B, K, 7) = ((lo+hi)/2, hi-lo, atan2(h0/|h|, h1/|h|)).
 *   backward: d_reg (B, 6*bins+2, K), d_agg (B, K, 3) from d_surface, d_bbox (either may be NULL).
 * bins <= 33. */
int nesie_side_decode_forward(int b, int k, int bins, const float *reg, const float *agg,
                              const float *scale, const float *sign, float *probs,
                              float *surface, float *bbox, void *stream);
int nesie_side_decode_backward(int b, int k, int bins, const float *reg, const float *probs,
                               const float *scale, const float *sign, const float *d_surface,
                               const float *d_bbox, float *d_reg, float *d_agg, void *stream);

/* Evaluation-mode BatchNorm (+ ReLU) (+ max over the neighbourhood axis): the running statistics
 * are folded by the caller into coef [C,4] = (scale, bias, -, -), scale = gamma / sqrt(var + eps),
 * bias = beta - mean * scale (what torch.nn.BatchNorm{1,2}d.eval() + nn.ReLU compute for the
 * ConvModules of point_sa_module.py:277-289 / side_pooling_module.py:346-358 at test time).
 * row_bias / group as in nesie_bn_relu_forward. */
/* coef [C,4] of an evaluation-mode BatchNorm from its parameters and running statistics (gamma /
 * beta may be NULL); one launch, recomputed per call (torch.nn.BatchNorm.eval() folds the same
 * numbers inside its kernel on every call). */
int nesie_bn_eval_coef(int c, const float *gamma, const float *beta, const float *running_mean,
                       const float *running_var, float eps, float *coef, void *stream);
int nesie_affine_relu_forward(int b, int c, long long p, const float *x, const float *coef,
                              int relu, const float *row_bias, int group, float *y,
                              void *stream);
int nesie_affine_relu_maxpool_forward(int b, int c, int m, int ns, const float *x,
                                      const float *coef, float *pooled, uint8_t *argmax,
                                      void *stream);

/* ---- inference post-processing and evaluation geometry -------------- */

/* aligned_3d_nms (core/post_processing/box3d_nms.py:129-176) for B scenes at once.
 * boxes (B,K,6) f32 axis-aligned (x1,y1,z1,x2,y2,z2), scores (B,K) f32, classes (B,K) i32,
 * valid (B,K) u8 or NULL: only boxes with valid != 0 take part (the reference indexes them
 * out with a boolean mask first, nesie_head.py:752-755).  picks (B,K) i32 = input positions
 * of the kept boxes in pick order (descending score), padded with -1; count (B) i32.
 * fp32 arithmetic in the reference's order; equal scores order by index (the later one is
 * picked first, as a stable ascending argsort read from its end).  K <= 512. */
int nesie_aligned_3d_nms(int b, int k, const float *boxes, const float *scores,
                         const int *classes, const uint8_t *valid, float thr, int *picks,
                         int *count, void *stream);

/* counts[b, t] = number of points of scene b inside box t: the column sums of
 * points_in_boxes_batch (same test, same LiDAR-frame operands) that
 * NesieHead.multiclass_nms_single takes for its non-empty mask
 * (`box_indices.T.sum(1) > 5`, nesie_head.py:744-750), without the (M, T) table. */
int nesie_points_in_boxes_count(int b, int boxes_num, int pts_num, const float *boxes,
                                const float *pts, int *counts, void *stream);

/* iou3d_cuda.boxes_overlap_bev_gpu (ops/iou3d/src/iou3d.cpp:66-90, iou3d_kernel.cu:127-264):
 * overlap AREA of every pair of rotated BEV rectangles (x1, y1, x2, y2, angle);
 * boxes_a (N,5), boxes_b (M,5) -> ans_overlap (N,M).  BaseInstance3DBoxes.overlaps
 * (base_box3d.py:387-438) multiplies it by the height overlap for the 3-D IoU of indoor_eval. */
int nesie_boxes_overlap_bev(int num_a, const float *boxes_a, int num_b, const float *boxes_b,
                            float *ans_overlap, void *stream);

/* iou3d_cuda.nms_gpu / nms_normal_gpu (ops/iou3d/src/iou3d.cpp:95-200, iou3d_kernel.cu:244-345)
 * over s independent segments in one fixed sequence of launches, without a host round trip.
 *   boxes (n,5) f32 (x1, y1, x2, y2, ry), scores (n) f32, valid (n) u8 or NULL (rows with
 *   valid == 0 take no part), offsets (s+1) i32 on the device: segment t is rows
 *   [offsets[t], offsets[t+1]); max_seg: a bound on every segment's length, <= 8192
 *   (NESIE_ERR_INVALID_ARG above; a segment longer than max_seg reports count -1).
 *   rotated 1: iou_bev (rotated overlap / fmaxf(sa + sb - ov, 1e-8)); 0: iou_normal (ry
 *   ignored).  A box is suppressed when iou > thr.
 *   keep (n) i32: the kept input rows of segment t at keep[offsets[t] .. + count[t]), in
 *   descending score order (equal scores by ascending row, NaN after every number);
 *   count (s) i32.
 *   workspace: n * (8 * ceil(max_seg / 64) + 24) bytes, device memory. */
int nesie_bev_nms(int n, int s, int max_seg, const float *boxes, const float *scores,
                  const uint8_t *valid, const int *offsets, float thr, int rotated, int *keep,
                  int *count, void *workspace, size_t workspace_bytes, void *stream);

/* ---- input side ---------------------------------------------------------- */

/* One training batch from HBM-resident scenes: the reference's per-sample CPU pipeline
 * IndoorPointSample -> RandomFlip3D -> GlobalRotScaleTrans after GlobalAlignment
 * (datasets/pipelines/transforms_3d.py:821-891, 59-162, 497-648, 410-488) in one gather pass.
 *   pool    (pool_rows, 3) f32  raw xyz of all resident scenes, back to back
 *   height  (pool_rows)    f32  shifted height z - percentile(z, 0.99) (loading.py:424-430)
 *   choices (B, n)         i32  sampled rows of the pool (np.random.choice + scene offset)
 *   xform   (B, 20)        f32  per scene: axis-align R[9] row-major, t[3]; flip_x, flip_y
 *                               (-1 = flipped, +1 = not); cos, sin of the rotation noise;
 *                               scale; trans[3]
 *   out     (B, n, 4)      f32  (x, y, z, height) as DefaultFormatBundle3D hands them on
 * out = ((flip(p R^T + t)) [[c, s, 0], [-s, c, 0], [0, 0, 1]]) * scale + trans; height * scale. */
int nesie_scene_assemble(int b, int n, long long pool_rows, const float *pool,
                         const float *height, const int *choices, const float *xform,
                         float *out, void *stream);

/* One pointwise (1x1) convolution layer of a grouped MLP on the fp32 matrix cores, with the
 * previous layer's BatchNorm + ReLU folded into the operand load and this layer's statistics /
 * pooling tail folded into the epilogue.  No extension entry in the reference: it evaluates mmcv
 * ConvModule(Conv2d 1x1 -> BN2d -> ReLU) and the pooling op by op (point_sa_module.py:277-289,
 * 136-158; side_pooling_module.py:343-370).
 *   y[n] = W[n % ng] . act(x[n]) (+ row_bias) (+ bias)       n < nb, nb % ng == 0
 *   x[n] (k, p) at x + n*x_bstride; y[n] (cout, p) at y + n*y_bstride (y NULL: not stored)
 *   W[g][m][kk] = w[g*w_gstride + m*w_rstride + kk*w_cstride]  (strides: W or its transpose)
 *   act(v) = in_coef ? max(fma(v, in_coef[g*k+kk][0], in_coef[g*k+kk][1]), in_relu ? 0 : -inf) : v
 *   row_bias (nb, cout, p / rb_group) or NULL; bias [ng*cout] or NULL
 *   stat_part (NULL = skip): [ng][nesie_pw_stat_slots(...)][cout][4] = (count, shift,
 *            sum(y - shift), sum((y - shift)^2)) per wave, merged by nesie_pw_stats_finalize
 *   pool_group 0 / 16 / 32: max (and, pool_min != 0, min) over each pool_group consecutive
 *            positions -> pool_*_out (nb, cout, p / pool_group), arg_*_out the position inside it.
 * Built for k <= 260, cout <= 256, p a multiple of the tile (nesie_pw_supported). */
int nesie_pw_supported(int k, int cout, long long p);
int nesie_pw_stat_slots(int nb, int ng, int k, int cout, long long p);
int nesie_pw_layer_forward(int nb, int ng, int k, int cout, long long p, const float *x,
                           long long x_bstride, const float *w, long long w_gstride,
                           int w_rstride, int w_cstride, const float *in_coef, int in_relu,
                           const float *row_bias, int rb_group, const float *bias, float *y,
                           long long y_bstride, float *stat_part, int pool_group, int pool_min,
                           float *pool_max_out, float *pool_min_out, uint8_t *arg_max_out,
                           uint8_t *arg_min_out, void *stream);
/* Input gradient of a layer whose input was relu(bn(Z)): y[n] = W[n % ng] . x[n] (W = the
 * transposed weight view, x = the gradient of the layer's raw output) as nesie_pw_layer_forward
 * computes it, and in the same launch the reduction pass of that BatchNorm's backward
 * (torch.nn.BatchNorm2d backward behind mmcv ConvModule, point_sa_module.py:277-289):
 *   bn_part[(g*cout + m) * nslots + slot][2] = sum(gg), sum(gg * zhat) over the slot's positions,
 *   gg = y [fma(Z, bn_coef[.][0], bn_coef[.][1]) > 0], zhat = (Z - bn_coef[.][2]) * bn_coef[.][3]
 * Z[n] (cout, p) at bn_z + n*bnz_bstride; nslots = nesie_pw_stat_slots(nb, ng, k, cout, p), every
 * slot is written; nesie_bn_relu_backward_apply consumes bn_part with nslice = nslots. */
int nesie_pw_dgrad_bn_reduce(int nb, int ng, int k, int cout, long long p, const float *x,
                             long long x_bstride, const float *w, long long w_gstride,
                             int w_rstride, int w_cstride, float *y, long long y_bstride,
                             const float *bn_z, long long bnz_bstride, const float *bn_coef,
                             float *bn_part, void *stream);
/* stat_part -> coef[ch][4] = (scale, bias, mean, invstd), scale = gamma * invstd, bias = beta -
 * mean * scale (fp64, Chan's merge of the shifted partials), running statistics updated like
 * torch.nn.BatchNorm2d in training mode.  channels = ng * cout (stacked layers).
 * chan_bias [channels] or NULL: the bias of a convolution in FRONT of the norm (mmcv ConvModule
 * with bias=True and a norm, vote_module.py:65-74).  The layer kernel leaves it out -- the mean
 * subtraction cancels it in every normalised value and its gradient is identically zero -- and
 * only the running mean, which tracks the biased output, gets it added here. */
int nesie_pw_stats_finalize(int channels, int cout, int nslots, const float *stat_part,
                            const float *gamma, const float *beta, float *running_mean,
                            float *running_var, float momentum, float eps, float *coef,
                            const float *chan_bias, void *stream);
/* Pooling tail: combine the group / pool_group partial extrema of every group of `group`
 * positions; with coef (this layer's BatchNorm) the value is relu?(scale * ext + bias) of the
 * extremum the sign of the scale selects (= max over the group of the normalised activation).
 * pooled (nb, channels, p / group), argmax the position inside the group (first on ties);
 * zstar (NULL = skip), like pooled: the raw extremum each pooled value came from. */
int nesie_pw_pool_finish(int nb, int ng, int channels, long long p, int group, int pool_group,
                         const float *pmax, const float *pmin, const uint8_t *amax,
                         const uint8_t *amin, const float *coef, int relu, float *pooled,
                         uint8_t *argmax, float *zstar, void *stream);

/* Backward of a POOLED TAIL -- last 1x1 conv (k -> c, bias-free) + training-mode BatchNorm + ReLU +
 * max over the ns samples of every group (PointSAModule's shared MLP and _pool_features,
 * point_sa_module.py:136-158, 277-289; autograd's max_pool2d / relu / batch_norm / conv2d backward
 * chain in the reference) -- without the dense pre-pool tensor: the forward keeps only pooled,
 * argmax and zstar, and with dZ = ghat + alpha + beta Z (per channel; ghat the pooled gradient at
 * the arg-max, one non-zero per channel and group)
 *   dA = W^T ghat + W^T alpha + (W^T diag(beta) W) A,   dW = sum ghat A^T + alpha s^T + diag(beta) W M,
 *   s = sum A, M = sum A A^T,  A = relu(coef_prev . z_prev) the layer's operand (k, p) per batch element.
 * nesie_pool_tail_supported: 1 when (k, c, p, ns) is built (k = 64, c = 128, ns in {16, 32, 64}).
 * nesie_pool_tail_sizes: out[0] = reduction slots of the input-gradient launch (bn_part [k][out[0]][2]),
 *   out[1] = partials of the weight-gradient pass.
 * nesie_pool_tail_prepare: dgamma, dbeta [c] (written); ab [c][4] = (alpha, beta, gamma invstd, -);
 *   ent [nb][m][c][2] = (masked pooled gradient, arg-max position as int bits);
 *   wcat [k][c + k] = [W^T diag(gamma invstd) | W^T diag(beta) W]; c0 [k] = W^T alpha.
 *   grad_pooled / pooled / zstar / argmax (nb, c, m); coef [c][4] = (scale, bias, mean, invstd) of
 *   this layer's norm; w (c, k) row-major.
 * nesie_pool_tail_dgrad: da (nb, k, p) = gradient of A, and in bn_part the two sums of the
 *   PREVIOUS layer's norm backward (as nesie_pw_dgrad_bn_reduce leaves them).
 * nesie_pool_tail_wgrad: dw (c, k) written; part_m [out[1]][k][k], part_s [out[1]][k],
 *   part_w [out[1]][c][k], ms [k k + k] doubles are scratch. */
int nesie_pool_tail_supported(int k, int c, long long p, int ns);
int nesie_pool_tail_sizes(int nb, int k, int c, long long p, int *out);
int nesie_pool_tail_prepare(int nb, int c, int m, int ns, int k, const float *grad_pooled,
                            const float *pooled, const float *zstar, const uint8_t *argmax,
                            const float *coef, const float *gamma, const float *w, float *dgamma,
                            float *dbeta, float *ab, float *ent, float *wcat, float *c0,
                            void *stream);
int nesie_pool_tail_dgrad(int nb, int k, int c, long long p, int ns, const float *z_prev,
                          long long z_bstride, const float *coef_prev, const float *wcat,
                          const float *c0, const float *ent, float *da, long long da_bstride,
                          float *bn_part, void *stream);
int nesie_pool_tail_wgrad(int nb, int k, int c, long long p, int ns, const float *z_prev,
                          long long z_bstride, const float *coef_prev, const float *ent,
                          const float *ab, const float *w, float *part_m, float *part_s,
                          float *part_w, double *ms, float *dw, void *stream);

/* A convolution (k -> c = 128, bias-free) that is max-pooled DIRECTLY over groups of ns positions (the
 * MiniPointNet's conv4 + max, side_pooling_module.py:343-370; autograd's max_pool2d / conv2d backward
 * in the reference): the gradient of its output is one non-zero per channel and group, and its
 * backward runs from the ENTRIES instead of the dense (nb, c, p) tensor.
 * nesie_pool_tail_pack: ent [nb][m][c][2] = (grad_pooled masked by pooled > 0 -- pooled NULL: no mask
 *   --, arg-max position as int bits); grad_pooled / pooled / argmax (nb, c, m); c % 32 == 0.
 * nesie_pw_dgrad_bn_reduce_sparse: nesie_pw_dgrad_bn_reduce with x given as ent (c = 128, ns in
 *   {16, 32, 64}, p % 64 == 0): the same launch parameters, y and bn_part bit for bit the dense
 *   launch's; nslots = nesie_pw_stat_slots(nb, ng, 128, cout, p).
 * nesie_pw_wgrad_sparse: nesie_pw_wgrad (below) with dy given as ent
 *   (co = 128, ci = 256, ns in {16, 64}; x_coef required, act = relu): a sparse product on the vector
 *   ALUs, one pass over x, that walks the dense launch's tiles and leaves the dense launch's partials --
 *   dw is bit for bit what nesie_pw_wgrad computes from the expanded tensor; same workspace size
 *   (nesie_pw_wgrad_workspace_bytes), same reduction, same `defer`. */
int nesie_pool_tail_pack(int nb, int c, int m, const float *grad_pooled, const float *pooled,
                         const uint8_t *argmax, float *ent, void *stream);
int nesie_pw_dgrad_bn_reduce_sparse(int nb, int ng, int c, int cout, long long p, int ns,
                                    const float *ent, const float *w, long long w_gstride,
                                    int w_rstride, int w_cstride, float *y, long long y_bstride,
                                    const float *bn_z, long long bnz_bstride, const float *bn_coef,
                                    float *bn_part, void *stream);
int nesie_pw_wgrad_sparse_supported(int co, int ci, long long p, int ns);
int nesie_pw_wgrad_sparse(int nb, int ng, int co, int ci, long long p, int ns, const float *ent,
                          const float *x, long long x_bstride, const float *x_coef, float *dw,
                          void *workspace, size_t workspace_bytes, int defer, void *stream);

/* Weight gradient of the same layers: dw[g][co][ci] = sum over the batches n of group g (n % ng
 * == g) and all positions of dy[n][co][pos] * act(x[n][ci][pos]), act as in
 * nesie_pw_layer_forward (x_coef [ng*ci][4], NULL = identity): the Conv2d weight gradient that
 * autograd computes for ConvModule (point_sa_module.py:277-289) with the normalised activation
 * recomputed on load.  dy[n] (co, p) at dy + n*dy_bstride, x[n] (ci, p) at x + n*x_bstride;
 * dw (ng, co, ci); partials are added in a fixed order (bitwise reproducible).
 * Supported: co <= 256, 9 <= ci <= 1024, p % 32 == 0; a layer wider than one workgroup's
 * accumulators (co <= 128: ci > 320; co > 128: ci > 128) runs as column blocks of dw, one
 * launch each -- or, when the position count is small (nesie_pw_wgrad_tiled: the 1-D chains,
 * 256 x 512 over 8 x 1024 positions), as ONE launch over 64 x 64 blocks of the product, every
 * block with its own runs of positions (split-K with a fixed-order reduction).
 * workspace = nesie_pw_wgrad_workspace_bytes(nb, ng, co, ci, p); defer: see "Deferred reductions". */
int nesie_pw_wgrad_supported(int co, int ci, long long p);
int nesie_pw_wgrad_tiled(int nb, int ng, int co, int ci, long long p);
size_t nesie_pw_wgrad_workspace_bytes(int nb, int ng, int co, int ci, long long p);
int nesie_pw_wgrad(int nb, int ng, int co, int ci, long long p, const float *dy,
                   long long dy_bstride, const float *x, long long x_bstride,
                   const float *x_coef, int x_relu, float *dw, void *workspace,
                   size_t workspace_bytes, int defer, void *stream);

/* Deferred reductions: nothing in a backward pass reads a weight gradient (its consumers are the
 * optimiser and the gradient all-reduce), so every weight-gradient entry point (nesie_pw_wgrad,
 * nesie_pw_wgrad_sparse, nesie_pw_wgrad_bn_backward and its _k4 / _k4_fused forms) takes `defer`:
 * 0 reduces at once; anything else runs the product only and leaves the fixed-order addition of the
 * per-workgroup partials PENDING (whatever else the launch writes -- dz, dgamma, dbeta, the input
 * gradient's reductions -- is complete on return).  nesie_pw_wgrad_flush_deferred(stream)
 * then finishes every pending gradient in ONE launch (descriptor table in the kernel arguments;
 * each element is summed exactly as by an immediate launch: bit-identical).  Until the flush the
 * workspace of a deferred launch must stay untouched and dw holds no valid data.  A launch that
 * runs as several column blocks reduces immediately.  nesie_pw_wgrad_pending(): how many wait;
 * nesie_pw_wgrad_drop_deferred(): forget them (error paths).  Host-side queue, one per process. */
int nesie_pw_wgrad_flush_deferred(void *stream);
int nesie_pw_wgrad_pending(void);
int nesie_pw_wgrad_drop_deferred(void);

/* The same weight gradient fused with the BatchNorm + ReLU backward that PRODUCES its dY operand
 * (replaces nesie_bn_relu_backward_apply + nesie_pw_wgrad for a conv -> BatchNorm -> ReLU layer of
 * ConvModule, point_sa_module.py:277-289): da (nb, co, p) is the gradient of relu(bn(z)), z the raw
 * conv output (both at n*z_bstride), z_coef [ng*co][4] the layer's folded forward coefficients
 * (scale, shift, mean, invstd), part [(ng*co) * nslots * 2] the (sum g, sum g zhat) partials the
 * input-gradient launch that produced da left (nesie_pw_dgrad_bn_reduce).  Tiles of (da, z) are
 * turned into dz = gamma invstd (g - mean(g) - zhat mean(g zhat)), g = da [fma(z, scale, shift) > 0],
 * on their way into LDS: dz is the MFMA operand and is written once (dz may be da) for the
 * input-gradient launch that follows; dgamma, dbeta [ng*co] are written.  coef_ws: ng*co*8 floats.
 * d_row_bias (optional): the gradient of a per-group row bias that the forward added to z
 * (nesie_pw_layer_forward's row_bias, groups of rb_group = 16 or 64 positions):
 * d_row_bias[n][r][pos / rb_group] = sum of dz over the group; with rb_group 64 the buffer must
 * arrive ZERO-FILLED (two partial sums per group are added atomically); requires z_bstride = co*p.
 * Supported where one launch owns every column of dw (nesie_pw_wgrad_bn_supported). */
int nesie_pw_wgrad_bn_supported(int co, int ci, long long p);
int nesie_pw_wgrad_bn_backward(int nb, int ng, int co, int ci, long long p, const float *da,
                               const float *z, long long z_bstride, const float *z_coef,
                               const float *gamma, const float *part, int nslots, const float *x,
                               long long x_bstride, const float *x_coef, int x_relu, float *dz,
                               float *dw, float *dgamma, float *dbeta, float *coef_ws,
                               float *d_row_bias, int rb_group, void *workspace,
                               size_t workspace_bytes, int defer, void *stream);

/* The layer kernel for skinny HBM-bound first layers (cin <= 64, cout <= 128): W stays in
 * LDS / registers and every wave streams its own 32-position columns straight from global
 * memory into the MFMA operand registers (no LDS tile, no barrier in the main loop).
 *   y[b] = W . act(x[b]),  x[b] (cin, p) at x + b*x_bstride, W (cout, cin), y (B, cout, p);
 *   act(v) = in_coef ? relu?(in_coef[k][0] * v + in_coef[k][1]) : v;
 *   stat_partial (NULL = skip): nesie_mlp_stream_partials(b, p) x cout x 2 floats, the
 *   per-workgroup (sum, sum of squares) of y. */
long long nesie_mlp_stream_partials(int b, long long p);
/* (sum, sum of squares) partials -> coef[c][4] = (scale, bias, mean, invstd) (fp64), running
 * statistics updated like torch.nn.BatchNorm2d in training mode.  stat_partial is [nparts][c][2]
 * (the streaming kernel) or, channel_major != 0, [c][nparts][2] (nesie_blend_conv_forward). */
int nesie_mlp_stat_finalize(int c, long long nparts, double count, const float *stat_partial,
                            const float *gamma, const float *beta, float *running_mean,
                            float *running_var, float momentum, float eps, float *coef,
                            int channel_major, void *stream);
int nesie_mlp_layer_forward_stream(int b, int cin, int cout, long long p, const float *x,
                                   long long x_bstride, const float *w, const float *in_coef,
                                   int in_relu, float *y, float *stat_partial, void *stream);

/* ---- round 5: the first shared-MLP layer of PointSAModule over a 4-channel input WITHOUT its
 * output tensor.  Reference: the first ConvModule (Conv2d(4, 64, 1) + BatchNorm2d + ReLU) of SA1's
 * `self.mlps[0]` (point_sa_module.py:277-289, pointnet2_sa_ssg.py:62-79), its output's three
 * consumers in the forward / backward of the SECOND ConvModule, and autograd's conv2d / batch_norm
 * backward for the first.  Z0 = W0 . X4 (X4 = the grouped coordinates + height, (nb, 4, p), 17 MB at
 * 8 x 131 072 positions; Z0 would be 268 MB) is rebuilt from X4 with one fixed fma chain wherever
 * it is an operand, and the first layer's weight gradient follows from reductions:
 *  - nesie_k4_moments: the first and second moments of X4 (20 sums, per-workgroup partials in
 *    double, nesie_k4_moments_bytes() bytes); nesie_k4_stat_finalize: the first layer's BatchNorm
 *    statistics from them -- mean(Z0[c]) = W0[c] . mean(X4), var(Z0[c]) = W0[c]^T Cov(X4) W0[c] --
 *    as coef [64][4] = (scale, bias, mean, invstd) + the running statistics (no pass over Z0;
 *    nesie_mlp_layer_forward_stream with y == NULL is the direct form of the same statistics);
 *  - nesie_pw_layer_forward_k4: the second layer, y = W . relu(in_coef . Z0) (cout = 64; w0 (64, 4)
 *    row-major; in_coef [64][4] the first layer's folded norm), with statistics like
 *    nesie_pw_layer_forward;
 *  - nesie_pw_wgrad_bn_backward_k4: nesie_pw_wgrad_bn_backward of the second layer (64 x 64) with
 *    its X operand rebuilt (x_coef = in_coef above);
 *  - nesie_pw_dgrad_bn_reduce_k4: nesie_pw_dgrad_bn_reduce of the second layer whose OUTPUT (the
 *    gradient of the first activation) is not stored: bn_part as there, and
 *    g_part[(m * nslots + slot)][4] = sum over the slot's positions of gg[m] X4[j], j = 0 .. 3
 *    (nslots = nesie_pw_stat_slots(nb, 1, k, 64, p));
 *  - nesie_k4_first_layer_wgrad: dW0[m][j] = a G[m][j] + e0 Sx[j] + d1 (mu Sx[j] - sum_k W0[m][k] M[k][j])
 *    with (.., a, mu, d1, e0, ..) = bnb[m][2..5] of nesie_pw_bnb_coef over that bn_part, G the slot
 *    sums of g_part, Sx / M the first and second moments of X4 (mom_part of nesie_k4_moments).
 * All of it requires no gradient for X4 (the backbone's grouped input coordinates). */
int nesie_pw_layer_forward_k4(int nb, int cout, long long p, const float *x4, long long x4_bstride,
                              const float *w0, const float *w, int w_rstride, int w_cstride,
                              const float *in_coef, float *y, long long y_bstride, float *stat_part,
                              void *stream);
int nesie_pw_dgrad_bn_reduce_k4(int nb, int k, long long p, const float *x, long long x_bstride,
                                const float *w, int w_rstride, int w_cstride, const float *x4,
                                long long x4_bstride, const float *w0, const float *bn_coef,
                                float *bn_part, float *g_part, void *stream);
int nesie_pw_wgrad_bn_backward_k4(int nb, long long p, const float *da, const float *z,
                                  long long z_bstride, const float *z_coef, const float *gamma,
                                  const float *part, int nslots, const float *x4,
                                  long long x4_bstride, const float *w0, const float *x_coef,
                                  float *dz, float *dw, float *dgamma, float *dbeta, float *coef_ws,
                                  void *workspace, size_t workspace_bytes, int defer, void *stream);
/* nesie_pw_wgrad_bn_backward_k4 and nesie_pw_dgrad_bn_reduce_k4 as ONE launch: the dZ tile that the
 * weight gradient forms in LDS is also multiplied by w^T (w (64, 64) row-major, the layer's weight) and
 * only the reductions of that product leave the kernel -- in_part [64][slots][2], in_gpart
 * [64][slots][4], slots = nesie_pw_wgrad_bn_backward_k4_slots(nb, p); dZ itself is written nowhere
 * (da is left untouched). */
int nesie_pw_wgrad_bn_backward_k4_slots(int nb, long long p);
int nesie_pw_wgrad_bn_backward_k4_fused(int nb, long long p, const float *da, const float *z,
                                        long long z_bstride, const float *z_coef, const float *gamma,
                                        const float *part, int nslots, const float *x4,
                                        long long x4_bstride, const float *w0, const float *x_coef,
                                        const float *w, float *dw, float *dgamma, float *dbeta,
                                        float *coef_ws, float *in_part, float *in_gpart,
                                        void *workspace, size_t workspace_bytes, int defer, void *stream);
size_t nesie_k4_moments_bytes(void);
int nesie_k4_moments(int nb, long long p, const float *x4, long long x4_bstride, void *mom_part,
                     void *stream);
int nesie_k4_stat_finalize(double count, const void *mom_part, const float *w0, const float *gamma,
                           const float *beta, float *running_mean, float *running_var, float momentum,
                           float eps, float *coef, void *stream);
int nesie_k4_first_layer_wgrad(const void *mom_part, const float *w0, const float *bnb,
                               const float *g_part, int nslots, float *dw, void *stream);

/* Weight gradient of a 1x1 conv on the matrix cores: dw[cout][cin] = sum over scenes and
 * positions of dy[b][m][p] * act(x[b][k][p]); dy (B, cout, p), x[b] (cin, p) at x + b*x_bstride,
 * act as in nesie_mlp_layer_forward_stream (x_coef NULL = identity).  Reference: the conv2d backward
 * that autograd runs for ConvModule's Conv2d (point_sa_module.py:277-289).  Partials are added in
 * a fixed order (bitwise reproducible).  dy[b] (cout, p) at dy + b*dy_bstride.  cout <= 128 with
 * cin <= 288, or cout <= 256 with cin <= 128;
 * workspace = nesie_conv_wgrad_workspace_bytes(b, cout, cin, p). */
size_t nesie_conv_wgrad_workspace_bytes(int b, int cout, int cin, long long p);
int nesie_conv_wgrad(int b, int cout, int cin, long long p, const float *dy,
                     long long dy_bstride, const float *x, long long x_bstride,
                     const float *x_coef, int x_relu, float *dw, void *workspace,
                     size_t workspace_bytes, void *stream);
/* The same with the BatchNorm + ReLU backward that produces dy applied on the load: da = gradient of
 * relu(bn(z)), bnb [cout][8] from nesie_pw_bnb_coef; dz is never written (for a layer whose input
 * needs no gradient, e.g. the first layer of SA1: nothing else reads it). */
int nesie_conv_wgrad_bn(int b, int cout, int cin, long long p, const float *da, const float *z,
                        long long z_bstride, const float *bnb, const float *x, long long x_bstride,
                        const float *x_coef, int x_relu, float *dw, void *workspace,
                        size_t workspace_bytes, void *stream);

/* mmdet3d/ops/voxel: dynamic / hard voxelization (src/voxelization_cpu.cpp, voxelization_cuda.cu)
 * and dynamic_scatter (src/scatter_points_cuda.cu).  fp32 features, int32 coordinates, 3 spatial
 * dimensions.  The default training step launches none of it.
 * Grid (voxelization_cuda.cu:209-211): grid[j] = roundf((hi[j] - lo[j]) / vs[j]) for j = x, y, z,
 *   computed on the host in fp32, halves rounded away from zero.  voxel_size (3 floats, x y z) and
 *   coors_range (6 floats, lo xyz then hi xyz) are HOST pointers.  Every grid[j] >= 1 and
 *   cells = grid_x * grid_y * grid_z < 2^31, else NESIE_ERR_UNSUPPORTED before any launch;
 *   nesie_voxel_grid_size is the size query: grid[3] (x, y, z) and *cells, or that status.
 * Cell of a point (voxelization_cpu.cpp:20-37, voxelization_cuda.cu:33-60), all fp32:
 *   c_j = floor((p_j - lo_j) / vs_j), one subtraction, one IEEE division, then floor.  The point is
 *   out of range if any c_j < 0, any c_j >= grid_j, or a quotient is NaN or infinite (a quotient of
 *   2^31 or more is out of range too).  Coordinates are written reversed, (c_z, c_y, c_x).  An
 *   out-of-range point gets (-1, -1, -1).  DEPARTURE 1: that is the row of the reference's CPU
 *   program; its CUDA kernel returns at the first failing axis and leaves (-1, 0, 0) or
 *   (-1, -1, 0).  points[N, C], C >= 3; columns beyond the first three are payload.
 * nesie_dynamic_voxelize: coors[N,3] i32, WRITTEN in full.
 * nesie_hard_voxelize (voxelization_cpu.cpp:65-96, the same result as voxelization_cuda.cu:106-180):
 *   walk the points in ascending index; a cell becomes a voxel the first time one of its points is
 *   met, provided fewer than max_voxels voxels exist, otherwise that point and every later point of
 *   the cell are dropped; a point of an existing voxel is stored at slot num if num < max_points,
 *   else dropped.  So voxels appear in order of first appearance, a voxel's points are in ascending
 *   index, num_points_per_voxel = min(count, max_points), *voxel_num = min(distinct in-range
 *   cells, max_voxels).  voxels[max_voxels, max_points, C] f32, coors[max_voxels, 3] i32,
 *   num_points_per_voxel[max_voxels] i32, voxel_num one i32 ON THE DEVICE (the entry never
 *   synchronises).  The rows below *voxel_num are WRITTEN in full, unused slots 0; the rows at and
 *   above it are NOT TOUCHED and keep whatever the caller's buffers held.  max_points, max_voxels
 *   >= 1 (the reference's -1 means dynamic voxelization: call that entry).
 * nesie_dynamic_scatter_forward (scatter_points_cuda.cu:183-234): coors[N,3] i32; dims[3] (HOST
 *   pointer) are exclusive upper bounds of the three columns, each >= 1, product < 2^31, else
 *   NESIE_ERR_UNSUPPORTED.  A row is invalid if any entry is negative or >= its dims entry (the
 *   reference knows negative entries only; it has no bound to test against).  The voxels are the
 *   distinct valid rows in ascending lexicographic order (the order of at::unique_dim).
 *   coors_map[N] = each point's voxel row, -1 for an invalid row; voxel_coors[M,3];
 *   reduce_count[M] = points per voxel; voxel_feats[M,C]: reduce_type 2 (max) per voxel and channel
 *   over its points in ascending point index starting from -inf, a value replacing the running one
 *   only if it compares greater -- fmaxf's value: a NaN never wins (of +0 and -0 the first met
 *   stays); 0 (sum) an fp32 running sum in ASCENDING POINT INDEX without contraction; 1 (mean)
 *   that sum divided by (float)count, IEEE division.  No float atomics: bitwise reproducible.
 *   DEPARTURE 2: the reference always discards the first row of unique_dim's output on the
 *   assumption that it is (-1, -1, -1), and so loses the smallest real voxel when no row is
 *   invalid; here a voxel is dropped only if it is the invalid one.
 *   M is data dependent: the caller allocates voxel_feats, voxel_coors, reduce_count with N rows;
 *   *num_voxels = M is one i32 on the device and only the first M rows are written.  Two arrays
 *   are saved for the backward: order[N], the point indices sorted by (voxel, index), invalid
 *   rows last, and voxel_start[N], of which the first M entries hold the position in `order` where
 *   each voxel's points begin.  voxel_start is the one argument added to the proposed list: the
 *   max backward walks a voxel's points in index order and has to know where they begin.
 * nesie_dynamic_scatter_backward (:236-303): grad_feats[N,C] WRITTEN in full, zeros for invalid
 *   rows.  sum: grad_voxel[map]; mean: grad_voxel[map] / (float)count, IEEE division; max: per
 *   voxel and channel the LOWEST-INDEX point whose feature equals voxel_feats takes the gradient
 *   (:136-160, the atomicMin of the index), every other point gets 0.  A cell whose maximum no
 *   feature equals (every feature NaN) passes no gradient; the reference writes out of bounds
 *   there (its reduce_from keeps the fill value num_input).  feats, voxel_feats, order,
 *   voxel_start and num_voxels are read by the max backward only and may be null otherwise.
 * Scratch: `workspace` holds nesie_voxel_workspace_bytes(n, cells) bytes (cells = the grid's, or
 *   the product of dims) and may be reused by the next call on the same stream.  No entry
 *   allocates or synchronises; every launch (and the 4-byte memset of an empty call) goes on the
 *   given stream, so forward and backward capture into a graph.
 * A negative size, reduce_type outside 0 .. 2, max_points / max_voxels < 1, C < 3 for the
 *   voxelizers, or a null pointer for a non-empty problem is NESIE_ERR_INVALID_ARG; more than
 *   2^31 - 1025 points NESIE_ERR_UNSUPPORTED.  N == 0 or C == 0 succeeds without a kernel launch
 *   and sets *voxel_num / *num_voxels to 0 (:192-196). */
int nesie_voxel_grid_size(const float *voxel_size, const float *coors_range, int *grid,
                          long long *cells);
int nesie_voxel_workspace_bytes(long long n, long long cells, long long *out);
int nesie_dynamic_voxelize(long long n, int c, const float *points, const float *voxel_size,
                           const float *coors_range, int *coors, void *stream);
int nesie_hard_voxelize(long long n, int c, const float *points, const float *voxel_size,
                        const float *coors_range, int max_points, int max_voxels, float *voxels,
                        int *coors, int *num_points_per_voxel, int *voxel_num, void *workspace,
                        void *stream);
int nesie_dynamic_scatter_forward(long long n, int c, const float *feats, const int *coors,
                                  const int *dims, int reduce_type, float *voxel_feats,
                                  int *voxel_coors, int *coors_map, int *reduce_count,
                                  int *num_voxels, int *order, int *voxel_start, void *workspace,
                                  void *stream);
int nesie_dynamic_scatter_backward(long long n, int c, const float *grad_voxel, const float *feats,
                                   const float *voxel_feats, const int *coors_map,
                                   const int *reduce_count, const int *order,
                                   const int *voxel_start, const int *num_voxels, int reduce_type,
                                   float *grad_feats, void *stream);

/* mmdet3d/ops/spconv: sparse 3-D convolution (semantics of ops/spconv/include/spconv/geometry.h
 * :25-85 and spconv_ops.h:60-140; none of its structure).  fp32 features, int32 sites, 3 spatial
 * dimensions, dilation 1, groups 1.  The default training step launches none of it.
 * Sites and keys: a row of indices[N,4] is (b, z, y, x); the grid is spatial_shape = (D, H, W) with
 *   batch_size samples; the key of a site is ((b * D + z) * H + y) * W + x.  batch_size * D * H * W
 *   must be below 2^31 for the input AND the output grid, else NESIE_ERR_UNSUPPORTED (a
 *   41 x 1600 x 1408 grid fits up to batch 23).  spatial_shape, ksize, stride, padding are HOST
 *   pointers to 3 ints (z, y, x); at most 512 taps; N * K at most 2^31 - 1025 (the sort's limit).
 * Geometry: cross-correlation.  Tap k enumerates (kz, ky, kx) row-major, weight is
 *   [kz, ky, kx, Cin, Cout].  Output site o reads input site o * stride - padding + k per axis;
 *   output size per axis (in + 2 * pad - (k - 1) - 1) / stride + 1 (nesie_spconv_out_shape is the
 *   size query, an addition to the proposed list: the host needs the output grid before it sizes
 *   out_indices).  Submanifold (subm != 0): stride 1 and padding k / 2 WHATEVER was passed
 *   (spconv_ops.h:76-79), the output sites are the input sites.
 * Rulebook = two gather tables and a count, functions of the indices alone (bit-identical from
 *   build to build): nbr[M,K] = the input row that output row o reads at tap k, or -1;
 *   nbr_t[N,K] = the output row that input row i feeds at tap k, or -1 (unique: (i, k) fixes the
 *   output site); pair_num[K] = the valid entries of column k.  The output rows of a regular conv
 *   are the distinct reachable output sites in ascending key order (= lexicographic (b, z, y, x));
 *   of a submanifold conv the input rows themselves, same order (out_indices is then neither read
 *   nor written by phase 1 and may be null; phase 2 takes the input indices as out_indices).
 * Input validity: rows must lie inside the grid (b in 0 .. batch_size - 1) and be pairwise
 *   distinct.  Offending rows -- a row outside the grid (tested per axis BEFORE a key is formed), and
 *   every row of a run of equal keys except the one of lowest index -- are counted on the device and
 *   take part in no pair.
 * nesie_spconv_out_sites (phase 1): sorted_keys[N] / sorted_rows[N] = the input keys in ascending
 *   order (an outside row carries the key batch_size * D * H * W and sorts last) and the rows that
 *   own them; nbr_t[N,K] WRITTEN in full; out_indices[cap,4] with cap = min(N * K, output cells),
 *   rows below M written; counts[2] on the device = {M, offending rows} (the entry never
 *   synchronises; the caller reads both in one copy).
 * nesie_spconv_gather_table (phase 2, M known): nbr[M,K] WRITTEN in full, pair_num[K].
 * nesie_spconv_gather_gemm: dst[r] = sum_k src[table[r,k]] . W[k] for r < rows, taps ascending,
 *   source channels ascending inside a tap, -1 (or an entry >= src_rows) a zero row.  W[k] is
 *   [c_src, c_dst], or with weight_transposed != 0 it is stored [c_dst, c_src] and read transposed.
 *   One accumulator chain (v_mfma_f32_32x32x2_f32, an fp32 fma chain) per output element: no float
 *   atomics, no split over workgroups, no dependence on nesie_set_cu_count; dst WRITTEN in full.
 *   Non-finite weights are outside the contract (a zero row times inf).  The four feature products
 *   are this one entry: forward (nbr, W); input gradient dIn[i] = sum_k dOut[nbr_t[i,k]] . W[k]^T
 *   (nbr_t, transposed); inverse-conv forward out'[i] = sum_k in'[nbr_t[i,k]] . W'[k] (nbr_t, W');
 *   inverse-conv input gradient (nbr, transposed).  Any c_src, c_dst >= 1.
 * nesie_spconv_wgrad: dW[k] = sum_r src[table[r,k]]^T . dout[r], r < rows.  The rows are cut into
 *   min(16, ceil(rows / 512)) chunks (a function of `rows` only); every (tap, chunk) writes a
 *   partial product into `workspace` (nesie_spconv_wgrad_workspace_bytes), a second launch adds the
 *   partials in ascending chunk order.  dw[K, c_in, c_out] WRITTEN in full; bit-identical from run
 *   to run.
 * Scratch of phase 1: nesie_spconv_rules_workspace_bytes(n, kvol, subm).  No entry allocates or
 *   synchronises; every launch and memset goes on the given stream.
 * n == 0 (phase 1), m == 0 (phase 2), rows == 0 (and, for wgrad, src_rows == 0) succeed without
 *   touching the device.  A negative size, a size triple with an entry < 1 (padding < 0), or a null
 *   pointer for a non-empty problem is NESIE_ERR_INVALID_ARG. */
int nesie_spconv_rules_workspace_bytes(long long n, int kvol, int subm, long long *out);
int nesie_spconv_out_shape(const int *spatial_shape, const int *ksize, const int *stride,
                           const int *padding, int subm, int batch_size, int *out_shape,
                           long long *out_cells);
int nesie_spconv_out_sites(long long n, const int *indices, int batch_size,
                           const int *spatial_shape, const int *ksize, const int *stride,
                           const int *padding, int subm, int *sorted_keys, int *sorted_rows,
                           int *nbr_t, int *out_indices, int *counts, void *workspace,
                           void *stream);
int nesie_spconv_gather_table(long long m, const int *out_indices, long long n,
                              const int *sorted_keys, const int *sorted_rows, int batch_size,
                              const int *spatial_shape, const int *ksize, const int *stride,
                              const int *padding, int subm, int *nbr, int *pair_num, void *stream);
int nesie_spconv_gather_gemm(long long rows, long long src_rows, int kvol, int c_src, int c_dst,
                             const float *src, const float *weight, int weight_transposed,
                             const int *table, float *dst, void *stream);
int nesie_spconv_wgrad_workspace_bytes(long long rows, int kvol, int c_in, int c_out,
                                       long long *out);
int nesie_spconv_wgrad(long long rows, long long src_rows, int kvol, int c_in, int c_out,
                       const float *src, const float *dout, const int *table, float *dw,
                       void *workspace, void *stream);

/* mmdet3d/ops/paconv/src/assign_score_withk_cuda.cu:38-141  assign_score_withk forward / backward
 * (PAConv's aggregation of a position-adaptive weight bank over a neighbourhood).
 * Sizes: b, n0 source points, n1 centres, k neighbours, m bank kernels, o output channels.
 *   points[B,N0,M,O]  centers[B,N0,M,O]  scores[B,N1,K,M]  knn_idx[B,N1,K] (int64, as the reference)
 * With kn = knn_idx[b,n,k] and cn = knn_idx[b,n,0], the pair (n,k) is VALID iff 0 <= kn < N0.
 * forward:  output[b,o,n,k] = sum_m scores[b,n,k,m] * (points[b,kn,m,o] - centers[b,cn,m,o]) for a
 *   valid pair, exactly 0.0f for an invalid one; layout (B,O,N1,K); per element one chain
 *   acc = fma(score, point - centre, acc) with m ascending; WRITTEN in full.
 * backward (any of the three gradient pointers may be NULL = not wanted):
 *   grad_scores[b,n,k,m]  = sum_o (points[b,kn,m,o] - centers[b,cn,m,o]) * grad_out[b,o,n,k], one
 *     fma chain with o ascending; exactly 0 for an invalid pair;
 *   grad_points[b,j,m,o]  = sum over the valid (n,k) with kn == j of scores[b,n,k,m] *
 *     grad_out[b,o,n,k], one fma chain in ascending n*K + k;
 *   grad_centers[b,j,m,o] = - (sum over the n with cn == j, over their valid k, of the same
 *     product), one fma chain in ascending n*K + k, negated at the end;
 *   all three WRITTEN in full: a point that nobody references gets zeros.
 * The reference's `aggregate` argument does not reach its kernels and has no counterpart here.
 * Departures from the reference:
 *   - it asserts cn < N0 and otherwise reads out of bounds; here the centre term of an out-of-range
 *     cn is dropped (a zero row) in forward and backward (k = 0 then has kn = cn invalid and is zero
 *     anyway);
 *   - it adds points * score - centers * score per m; here the difference is taken first;
 *   - its output and gradients are atomicAdd sums in arrival order; here the order of every sum is
 *     fixed, two runs give the same bits, there is no atomic variant and NESIE_DETERMINISTIC=0
 *     changes nothing.
 * The scatter goes through nesie_inverted_index over N0 + 1 sources (invalid entries sit in the
 * sentinel bucket N0, which is skipped).  Scratch comes from the caller (16-byte aligned, at least
 * nesie_assign_score_withk_backward_workspace_bytes); nothing allocates or synchronises, so both
 * calls capture into a graph.
 * A negative size or k, m or o <= 0 is NESIE_ERR_INVALID_ARG; an element count of any tensor at or
 * above 2^31 is NESIE_ERR_UNSUPPORTED (workspace_bytes then answers 0); both before any launch.
 * b, n1 or n0 == 0 succeeds without a launch. */
int nesie_assign_score_withk_forward(int b, int n0, int n1, int k, int m, int o,
                                     const float *points, const float *centers,
                                     const float *scores, const long long *knn_idx, float *output,
                                     void *stream);
size_t nesie_assign_score_withk_backward_workspace_bytes(int b, int n0, int n1, int k, int m, int o);
int nesie_assign_score_withk_backward(int b, int n0, int n1, int k, int m, int o,
                                      const float *grad_out, const float *points,
                                      const float *centers, const float *scores,
                                      const long long *knn_idx, float *grad_points,
                                      float *grad_centers, float *grad_scores, void *workspace,
                                      size_t workspace_bytes, void *stream);

/* Sigmoid focal loss (mmcv ops sigmoid_focal_loss; mmdet FocalLoss builds on it).  The mmcv source is
 * not in the reference tree: the formulas below are the specification.
 *   x[N,C] logits, target[N] int64 labels.  Element (n, c) is POSITIVE iff target[n] == c; a label
 *   outside [0, C) (mmdet's background label C, -1, anything) makes the whole row negative and is
 *   never used as an index.  With z = x, a = alpha for a positive element and z = -x,
 *   a = 1 - alpha for a negative one, and softplus(v) = max(v, 0) + log1p(exp(-|v|)):
 *     term      = a * exp(-gamma * softplus(z)) * softplus(-z)        (= -a (1 - p_t)^gamma log p_t)
 *     d term/dz = -a * exp(-gamma * softplus(z)) * (gamma * sigmoid(z) * softplus(-z) + sigmoid(-z))
 *   and d term/dx carries the sign of dz/dx.  Nothing is subtracted or clamped, so every finite
 *   logit gives a finite term and gradient for every gamma >= 0 (gamma = 0: alpha-weighted BCE).
 * Weights: class_weight (C,) or NULL scales row n by class_weight[target[n]], by 1.0 for a label
 *   outside [0, C) (mmcv reads out of bounds there); sample_weight is NULL (sample_weight_mode 0),
 *   (N,) per row (mode 1) or (N, C) per element (mode 2).
 * Departure in value from mmcv: it clamps log() at FLT_MIN, so its loss stops growing at
 *   |x| ~ 87.3 and its gradient drops to 0 beyond; here the loss keeps growing linearly in -z and
 *   d term/dz keeps its limit -a, for every gamma.
 *   forward      loss[N,C] = term * weights * scale, every element written.
 *   forward_sum  out[0] = (sum of term * weights over all N * C elements) * scale * (*scale_dev),
 *                scale_dev a one-element device tensor or NULL (= 1); the (N, C) loss is never
 *                stored.  The sum runs in a fixed order that depends on N * C only (chunks of 4096
 *                elements, a fixed tree inside a chunk, then the chunks' partials in a fixed order):
 *                no atomics, the same bits whatever the CU budget or the stream.  workspace: at
 *                least nesie_sigmoid_focal_loss_workspace_bytes(n, c) bytes, 4-byte aligned; may be
 *                NULL when that is 0 (a single chunk: one launch instead of two).
 *   backward     grad_x[N,C] = d term/dx * weights * upstream, every element written in one launch;
 *                upstream = grad_out[n,c] * scale * (*scale_dev) with grad_out (N, C), or
 *                (*grad_scalar) * scale * (*scale_dev) with a one-element device tensor: exactly one
 *                of grad_out / grad_scalar is non-NULL, both are read on the device.
 * Nothing allocates or synchronises: all three capture into a graph.  n == 0 or c == 0 succeeds
 * without a launch and touches nothing.  A negative size, gamma < 0 or NaN, a mode outside 0..2 or
 * one that disagrees with sample_weight, or a null x / target / output of a non-empty problem is
 * NESIE_ERR_INVALID_ARG; n * c >= 2^31 is NESIE_ERR_UNSUPPORTED (workspace_bytes then answers 0). */
int nesie_sigmoid_focal_loss_forward(int n, int c, const float *x, const long long *target,
                                     const float *class_weight, const float *sample_weight,
                                     int sample_weight_mode, float gamma, float alpha, float scale,
                                     float *loss, void *stream);
size_t nesie_sigmoid_focal_loss_workspace_bytes(int n, int c);
int nesie_sigmoid_focal_loss_forward_sum(int n, int c, const float *x, const long long *target,
                                         const float *class_weight, const float *sample_weight,
                                         int sample_weight_mode, float gamma, float alpha,
                                         float scale, const float *scale_dev, float *out,
                                         void *workspace, size_t workspace_bytes, void *stream);
int nesie_sigmoid_focal_loss_backward(int n, int c, const float *x, const long long *target,
                                      const float *class_weight, const float *sample_weight,
                                      int sample_weight_mode, float gamma, float alpha,
                                      const float *grad_out, const float *grad_scalar, float scale,
                                      const float *scale_dev, float *grad_x, void *stream);

/* Lovasz-Softmax loss (reference mmdet3d/models/losses/lovasz_loss.py:38-126), loss and gradient in
 * one call.
 *   probas: float32 class probabilities of B images, C classes and S points, element (b, c, s) at
 *   probas[b * stride_b + c * stride_c + s * stride_s] (element strides): the channel-first
 *   (B, C, S) tensor and the flat (P, C) one (B = 1, stride_c = 1, stride_s = C) are read in place.
 *   labels[B, S] int64.  has_ignore / ignore: the void label.
 * A SEGMENT is one class over all B * S points (per_image = 0) or one (image, class) pair over its
 *   S points (per_image = 1).  In segment c, fg_i = (label_i == c) and e_i = |fg_i - p_ic| in fp32.
 *   A label outside [0, C) that is not `ignore` is background for every class and is never an
 *   index.  The entries are ordered by e descending, EQUAL ERRORS BY ASCENDING POINT INDEX
 *   (torch.sort leaves ties open; the loss does not depend on them, the gradient does).  +inf and
 *   NaN errors sort first, as torch.sort(descending=True) puts them, and reach the loss as inf or
 *   NaN.  A void point (label == ignore) sorts after every valid point of its segment with fg = 0:
 *   only prefixes enter the Lovasz gradient, so this equals the reference's compaction; its
 *   gradient is 0.
 *   With G the segment's foreground count and cf_i / cb_i the inclusive foreground / background
 *   counts of the first i sorted entries, U_i = G + cb_i, I_i = G - cf_i:
 *     g_i = 1 / U_i (fg_i)     g_i = I_i / (U_i (U_i - 1)) (otherwise)     g_0 = 1 when G = 0
 *   which is jaccard_i - jaccard_{i-1} of the reference without the difference of two numbers near
 *   1; evaluated in double from the integer counts.  loss_c = sum_i e_i g_i in double, in a fixed
 *   order; d loss_c / d p_ic = -g_i (fg_i) or +g_i.
 * class_mode 0: every class is averaged; 1: the classes present in the segment's labels (G > 0,
 *   decided on the device); 2: class c counts class_mask[c] times (C ints; a class list, a negative
 *   entry is 0).  loss[0] = mean of loss_c over the averaged classes (per_image: the mean over the
 *   B images of each image's class mean; an image without an averaged class contributes 0 and is
 *   still counted).  No averaged class at all: loss 0 and a zero gradient.
 *   grad: d loss / d probas, WRITTEN in full with the strides of probas (the divisor applied).
 * workspace: nesie_lovasz_softmax_workspace_bytes(images, classes, points) bytes, 8-byte aligned.
 * Nothing allocates, synchronises, reads back or uses an atomic: the call captures into a graph and
 *   gives the same bits in every run.  images, classes or points == 0 succeeds without a launch and
 *   touches nothing.  A negative size, a class_mode outside 0 .. 2, mode 2 without a mask or a null
 *   pointer of a non-empty problem is NESIE_ERR_INVALID_ARG; images * classes * points above
 *   2^31 - 1025 is NESIE_ERR_UNSUPPORTED (workspace_bytes then answers 0); all before any launch. */
size_t nesie_lovasz_softmax_workspace_bytes(int images, int classes, long long points);
int nesie_lovasz_softmax(int images, int classes, long long points, const float *probas,
                         long long stride_b, long long stride_c, long long stride_s,
                         const long long *labels, int has_ignore, long long ignore, int per_image,
                         int class_mode, const int *class_mask, float *loss, float *grad,
                         void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NESIE_OPS_H_ */
