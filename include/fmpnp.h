/*
 * fmpnp.h -- C ABI of libfmpnp.so, the MI355X (gfx950) feature-metric PnP refiner.
 *
 * Drop-in boundary for the reference's hot path (aunagar/FeatureMetric-PnP):
 *
 *   fmpnp_refine_batch / fmpnp_refine_batch_async
 *       replace sparseFeaturePnP.forward          featurePnP/model.py:245-494
 *       (and, with FMPNP_MODE_COMPUTE_COST,
 *        sparseFeaturePnP.compute_cost            featurePnP/model.py:216-243)
 *       -- the LM loop, the losses of          featurePnP/helpers/utils.py:15-78,
 *          optimizer_step                       featurePnP/model.py:37-72,
 *          indexing_ / points_within_image      featurePnP/model.py:74-117,
 *          ratio_threshold_feature_errors       featurePnP/model.py:120-129,
 *          so3exp_map                           featurePnP/helpers/utils.py:209-221.
 *   fmpnp_pack_features / fmpnp_pack_features_batch / fmpnp_pack_features_f
 *       replaces sobel_filter + the fp64 cast   featurePnP/helpers/utils.py:81-104,
 *                                               optimize_feature_pnp.py:57,61
 *       (fused Sobel + channels-last [H][W][3][C] packing).
 *   fmpnp_gather_reference
 *   fmpnp_gather_reference_async / fmpnp_gather_reference_batch
 *       replaces the per-point fref gather       optimize_feature_pnp.py:51-56.
 *   fmpnp_point_costs
 *       replaces find_inliers' per-point costs   featurePnP/model.py:132-146
 *       (projection, support mask, indexing_, 0.5||e||^2; the loss and ratio mask,
 *        model.py:147-152, stay in the façade).
 *   fmpnp_exhaustive_match / fmpnp_exhaustive_match_async / fmpnp_exhaustive_match_cpu
 *       replace exhaustive_search               s2dhm/pose_prediction/exhaustive_search.py:8-55
 *       (the dense correlation, the argmax and the modified ratio test).
 *   fmpnp_exhaustive_match_ex / _ex_async / _ex_cpu, fmpnp_correlation_ex_async, fmpnp_localize_ex
 *       the same with a precision: FMPNP_MATCH_F32 (the exact default) or the opt-in FMPNP_MATCH_F16.
 *   fmpnp_gather_sparse_descriptors
 *       replaces fast_sparse_keypoint_descriptor s2dhm/pose_prediction/keypoint_association.py:40-86.
 *   fmpnp_pnp_ransac / fmpnp_pnp_ransac_async / fmpnp_pnp_ransac_cpu
 *       replace solve_pnp's cv2 calls            s2dhm/pose_prediction/solve_pnp.py:44-69
 *       (P3P RANSAC, then a reprojection polish on the inliers; parity with OpenCV unpinned).
 *   fmpnp_hypercolumn_assemble / fmpnp_hypercolumn_assemble_async / fmpnp_hypercolumn_assemble_cpu
 *       replace the assembly half of compute_hypercolumn   s2dhm/network/network.py:149-173
 *       (bilinear resize of every layer, channel concatenation, per-texel L2 normalisation).
 *   fmpnp_hypercolumn_pack / fmpnp_hypercolumn_pack_async / fmpnp_hypercolumn_pack_cpu
 *       fuse that assembly with fmpnp_pack_features: the layers go straight into the packed map
 *       (fmpnp_feature_pnp_query_layers: the one-call refiner on them).
 *   fmpnp_localize / fmpnp_localize_async / fmpnp_localize_build_cpu / fmpnp_localize_pick_cpu
 *       replace the loop that joins the stages   s2dhm/pose_prediction/sparse_to_dense_predictor.py:140-191,233
 *       (matches -> PnP problems, the fallback, the best pick), device-resident between the stages.
 *   fmpnp_localize_refined / fmpnp_localize_refine_async / fmpnp_localize_refine_prep_cpu
 *       the same with the winners' refinement queued behind the pick (opt-in): every query's refiner problem
 *       assembled on the device, one gather and one launch per level over all the queries, one host wait.
 *   fmpnp_conv3x3 / fmpnp_relu_async / fmpnp_maxpool2x2 (with their _async and _cpu forms)
 *       the operators of the encoder             s2dhm/network/network.py:47-51,134-147
 *       (VGG-16's features[:-2]: 3x3 convolutions as exact-fp32 fmaf chains, ReLU, 2x2 max-pool; opt-in).
 *   fmpnp_conv1x1 (with its _async and _cpu forms)
 *       the 1x1 convolution of SuperPoint's heads third_party/SuperPointPretrainedNetwork/demo_superpoint.py:93-98
 *       (convPb and convDb, the same exact-fp32 chains; with the operators above the whole network; opt-in).
 *   fmpnp_conv3x3_dilated / fmpnp_avgpool2x2s1 / fmpnp_dense_pyramid_step (with their _async and _cpu forms)
 *       the d2-net dense features                s2dhm/d2net_utils/dense_pyramid.py:5-42
 *       (a VGG-16 trunk with conv4 dilated by 2 and an average pool of stride 1, and the scale pyramid's
 *       resize-add-normalise step; opt-in).
 *       the image front end                      s2dhm/network/images_from_list.py:57-103
 *       (Pillow-exact Lanczos resize of decoded uint8 pixels and the networks' value transforms; opt-in).
 *
 * Conventions: plain pointers and sizes, no torch types.  Feature / point
 * buffers are caller-owned DEVICE memory; results and traces of the
 * synchronous entry points are host memory.  Every entry point returns 0 on
 * success, a negative FMPNP_E* code for invalid arguments, or a positive
 * hipError_t; nothing throws.
 *
 * Threads: the asynchronous entry points touch only caller-owned memory.  The synchronous ones
 * (fmpnp_refine_batch, fmpnp_feature_pnp, fmpnp_exhaustive_match, fmpnp_pnp_ransac, fmpnp_localize,
 * fmpnp_localize_refined) keep their scratch
 * per (entry point, device, stream), each behind its own mutex, and drain their stream before returning
 * an error once work is queued: calls on distinct streams or devices run concurrently, calls on one
 * stream from several threads serialise.  (One exception among the asynchronous ones: the image front end's
 * fmpnp_image_*_async keep their coefficient tables and the intermediate image in such a scratch too, used in
 * stream order without waiting; see "image front end".)  Multi-GPU = one host thread (or process) per device.
 */
#ifndef FMPNP_H
#define FMPNP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMPNP_ABI_VERSION 4  /* 3: fmpnp_problem.window (windowed f-only packs); 4: fmpnp_feature_pnp */

/* robust losses, featurePnP/helpers/utils.py:15-78 */
typedef enum {
    FMPNP_SQUARED = 0,        /* squared_loss          :16-17 */
    FMPNP_HUBER = 1,          /* huber_loss            :20-29 */
    FMPNP_CAUCHY = 2,         /* cauchy_loss = barron(alpha=0)   :32-34 */
    FMPNP_GEMAN_MCCLURE = 3,  /* geman_mcclure = barron(alpha=-2) :37-38 */
    FMPNP_BARRON = 4          /* barron_loss(x, alpha) :40-78 */
} fmpnp_loss;

typedef enum {
    FMPNP_NEAREST = 0,   /* the reference: round(K P / z) - 1, floor rescale (model.py:88-89,306-308) */
    FMPNP_BILINEAR = 1   /* extension: 2x2 bilinear taps of f, gx, gy; the map must have
                            Hf < 32768 and Wf < 65535 (FMPNP_ETOOBIG otherwise) */
} fmpnp_sampling;

/* Storage type of the packed map (f, gx, gy) and of fref.
 *
 * FMPNP_F16 (opt-in; nothing selects it by default): IEEE binary16 storage.
 *   Pack.  Every stored value is the value the FMPNP_F32 pack stores, rounded once more to binary16: round to
 *       nearest even, subnormal results kept, magnitudes above 65504 become +-Inf, NaN stays NaN.  f: one
 *       rounding of the fp32 input; gx, gy: the pack's fp64 Sobel -> fp32 -> binary16 (two conversions).  So
 *       pack(dtype_out = F16) is pack(dtype_out = F32) narrowed elementwise, bit for bit; a reference-gather
 *       row is the fp32 row narrowed the same way.
 *   Strides.  cstride is C rounded up to a multiple of 8 (a plane's run stays 16-byte aligned), channels
 *       [C, cstride) zero; a cstride or ld_ref that is no multiple of 8 is FMPNP_EALIGN (LM launch, plan,
 *       workspace size -- which then reports 0 --, point costs, compute_cost, the CPU twin).
 *   LM kernel, fmpnp_point_costs, fmpnp_compute_cost_async.  Texels and descriptors are widened exactly to
 *       fp64 and everything after that is the code the other storage types run, so results do not depend on
 *       the launch shape, helpers, speculation or windows.  They are NOT bit-identical to the fp32 kernel on
 *       the widened values: a lane owns 8 channels, not 4, so the fp64 channel sums associate differently.
 *   Supported: FMPNP_LAYOUT_FGRAD, nearest sampling, every loss, the ratio test, both modes, teams, the
 *       first-evaluation helpers, speculation (channel slices of at most 512), packed windows, channel
 *       ranges and levels, fmpnp_feature_pnp.
 *   FMPNP_EINVAL: FMPNP_BILINEAR, FMPNP_LAYOUT_F, dtype_in = FMPNP_F16 (maps arrive as fp32 or fp64),
 *       fmpnp_feature_pnp_layers / _query_layers, the hypercolumn kernels' dtype_out, the localisation
 *       chain's refinement stage.  The planner never picks the compile-time 512-point carve for it. */
typedef enum { FMPNP_F32 = 0, FMPNP_F64 = 1, FMPNP_F16 = 2 } fmpnp_dtype;

typedef enum {
    FMPNP_LAYOUT_FGRAD = 0, /* feat = [Hf][Wf][3][cstride]: f, gx, gy (fmpnp_pack_features) */
    FMPNP_LAYOUT_F = 1      /* feat = [Hf][Wf][cstride]: f only (fmpnp_pack_features_f); the LM kernel
                               forms a texel's Sobel gradients from its 3x3 neighbourhood, in fp64,
                               when it gathers the texel.  fp32 storage, nearest sampling. */
} fmpnp_layout;

typedef enum {
    FMPNP_MODE_FORWARD = 0,       /* sparseFeaturePnP.forward */
    FMPNP_MODE_COMPUTE_COST = 1   /* sparseFeaturePnP.compute_cost at (R0, t0) */
} fmpnp_mode;

/* per-problem status bits (fmpnp_result.status) */
#define FMPNP_STATUS_OK 0
#define FMPNP_STATUS_NO_SUPPORT 1        /* no point inside the image at (R0,t0): model.py:316-320 */
#define FMPNP_STATUS_NAN 2               /* NaN step: model.py:411-413 (reference: NameError) */
#define FMPNP_STATUS_NO_SUPPORT_TRIAL 4  /* no point inside at a trial pose: model.py:441-445 */
#define FMPNP_STATUS_SYNC_TIMEOUT 8      /* internal: a cross-workgroup exchange timed out */
#define FMPNP_STATUS_HELPER_WAIT 16      /* informational: a first-evaluation helper workgroup did not
                                            publish in time and the main workgroup gathered that block
                                            itself (results unaffected: same gather code) */
#define FMPNP_STATUS_WINDOW 32           /* a point reached a texel whose 3x3 neighbourhood lies outside
                                            the problem's packed window (fmpnp_problem.window): the
                                            problem stopped early and its result is invalid -- pack its
                                            map in full and refine it again (fmpnp.pipeline does) */

/* argument errors (negative return codes) */
#define FMPNP_EINVAL -1
#define FMPNP_EALIGN -2
#define FMPNP_ENOMEM -3
#define FMPNP_ETOOBIG -4
#define FMPNP_ENODEV -5
#define FMPNP_ERANGE -6  /* fmpnp_feature_pnp: a reference inlier maps outside the reference map
                            (the reference raises IndexError, optimize_feature_pnp.py:56) */

typedef struct {
    int mode;               /* fmpnp_mode */
    int n_iters;            /* sparseFeaturePnP(n_iters) */
    double lambda0;         /* sparseFeaturePnP(lambda_), default 0.01 */
    int use_ratio;          /* ratio_threshold is not None */
    double ratio_threshold; /* keep |rho| < max|rho| * thr */
    int loss;               /* fmpnp_loss */
    double barron_alpha;    /* FMPNP_BARRON only */
    int sampling;           /* fmpnp_sampling */
    int dtype;              /* fmpnp_dtype of the packed features and fref */
    int wgs_per_problem;    /* workgroups cooperating on one problem; 0 = auto */
    int max_teams;          /* cap on concurrently resident problem teams; 0 = auto */
    int no_memo;            /* 1: re-gather every point's texel at every evaluation (the
                               reference's data movement); 0 (default): re-gather only points
                               whose texel changed and, where the planner enables it, also gather
                               the texels points are predicted to move to next beside the LM tail
                               (speculation: on by default; -DFMPNP_SPEC=0 compiles it out);
                               2: memoised without speculation -- all bit-identical results.
                               FMPNP_BILINEAR: 0/2 keep each point's cell memo (the six sums as
                               quadratics over its 2x2 cell, rebuilt when the cell changes; same
                               sums up to fp64 rounding), 1 samples every point every evaluation */
    int layout;             /* fmpnp_layout of every problem's feat */
    int sobel_flags;        /* FMPNP_LAYOUT_F: bit 0 normalized (/8), bit 1 replicate padding
                               (the flags fmpnp_pack_features would have been given) */
    int helpers;            /* first-evaluation helper workgroups per problem (small batches with
                               idle CUs): 0 = the planner's choice, < 0 = none (e.g. when other
                               kernels share the device and could keep helpers from being
                               resident: the main workgroups would wait up to 0.2 s for them),
                               > 0 = at most this many.  Results do not depend on it. */
} fmpnp_options;

typedef struct {
    const void *feat;       /* device, [Hf][Wf][3][cstride] of dtype: planes f, gx, gy
                               (FMPNP_LAYOUT_F: [Hf][Wf][cstride], f only) */
    const void *fref;       /* device, [N][ld_ref] of dtype; columns [c_begin, c_end) used */
    const double *pts3d;    /* device, [N][3] fp64 */
    int Hf, Wf, cstride, c_begin, c_end, ld_ref, N;
    int im_width, im_height;        /* image size in pixels (forward's im_width/im_height) */
    double K[9], R0[9], t0[3];      /* row-major */
    const unsigned char *window;    /* NULL: feat holds every texel.  Else (FMPNP_LAYOUT_F, one workgroup
                                       per problem) device [2][Hf][Wf] bytes written by
                                       fmpnp_pack_features_f_window_batch: plane 0 = texel packed, plane 1 =
                                       texel whose whole 3x3 neighbourhood is packed.  The LM kernel checks
                                       plane 1 at every gather and stops the problem with
                                       FMPNP_STATUS_WINDOW on a miss, so a result without that bit equals the
                                       fully packed map's bit for bit.  FMPNP_LAYOUT_FGRAD (nearest
                                       sampling; fmpnp_feature_pnp's windowed packs): plane 0 is checked,
                                       and a miss only sets FMPNP_STATUS_WINDOW (the problem finishes). */
} fmpnp_problem;

typedef struct {
    double R[9], t[3];      /* returned pose (R_best/t_best, or the current pose on early exit) */
    double initial_cost;    /* mean rho at (R0,t0) (forward i==0 / compute_cost); NaN if none */
    double best_cost;       /* best_cost_ (NaN when never set) */
    double final_lambda, final_lr;
    int best_num_inliers;   /* best_num_inliers_ (-1 when never set) */
    int n_evals;            /* tracked evaluations: 1 + trials */
    int n_steps;            /* optimizer steps taken */
    int n_accepted;
    int status;             /* FMPNP_STATUS_* bits */
    int has_best;           /* best_cost_ was set */
    long long texel_gathers; /* point-texel gathers actually read from memory by the problem's
                                first workgroup (a texel is re-read only when a point's pixel
                                changes: the channel sums of an unchanged texel are reused) */
} fmpnp_result;

typedef struct {            /* one tracked evaluation (model.track_, model.py:170-176) */
    double R[9], t[3];
    double cost;            /* mean rho at this pose */
    double lambda_after, lr_after;
    int n_supported, n_kept, accepted;
} fmpnp_trace_entry;

/* library identity / device check */
int fmpnp_abi_version(void);
const char *fmpnp_build_info(void);
int fmpnp_device_check(int device); /* 0 if `device` is a gfx950 the library can run on */

/* Fused Sobel (3x3, unnormalised unless sobel_normalized -> /8; zero or replicate
 * padding) + channels-last pack: chw [C][H][W] (dtype_in) -> out [H][W][3][cstride]
 * (dtype_out).  When gx_chw/gy_chw are non-NULL they are packed as given instead of
 * computing the Sobel (forward() receives its gradients from the caller). */
int fmpnp_pack_features(const void *chw, const void *gx_chw, const void *gy_chw, int dtype_in, int C, int H,
                        int W, void *out, int dtype_out, int cstride, int sobel_normalized,
                        int sobel_replicate_pad, void *hip_stream);

/* Channels-last copy of f only, [H][W][cstride] fp32 (dtype_out = FMPNP_F32, cstride a
 * multiple of 4, out 16-byte aligned; channels [C, cstride) zero-filled): the
 * FMPNP_LAYOUT_F input of the LM kernel, a third of fmpnp_pack_features' output bytes. */
int fmpnp_pack_features_f(const void *chw, int dtype_in, int C, int H, int W, void *out, int dtype_out,
                          int cstride, void *hip_stream);

/* fref gather of optimize_feature_pnp.py:51-56: for each of the N reference
 * inliers (x, y) (device [N][2] fp64), row = trunc(y * W_ref / img1),
 * col = trunc(x * H_ref / img0) of ref_chw [C][H_ref][W_ref] -> out [N][ld_out]. */
int fmpnp_gather_reference(const void *ref_chw, int dtype_in, int C, int H_ref, int W_ref,
                           const double *ref_inliers, int N, int img0, int img1, void *out, int dtype_out,
                           int ld_out, void *hip_stream);

/* Asynchronous form of fmpnp_gather_reference: nothing is synchronised; an inlier
 * outside the reference map ORs 1 into *err_flag (a device int the caller zeroes
 * beforehand and reads after the stream reached this point) and zeroes its row.
 * The batch pipeline (fmpnp.pipeline) uses it so preparing one batch never waits
 * for the device. */
int fmpnp_gather_reference_async(const void *ref_chw, int dtype_in, int C, int H_ref, int W_ref,
                                 const double *ref_inliers, int N, int img0, int img1, void *out, int dtype_out,
                                 int ld_out, int *err_flag, void *hip_stream);

/* Batched forms for a caller preparing many queries at once (fmpnp.pipeline): one host
 * call, one launch per item on hip_stream, nothing synchronised.  Host arrays of n entries;
 * shape[4*i..] = (C, H, W, cstride) of map i, ref_shape[3*i..] = (C, H_ref, W_ref) of
 * reference map i; err_flags is a DEVICE int[n] the caller zeroes (set as in
 * fmpnp_gather_reference_async).  Every item is validated before anything is launched. */
int fmpnp_pack_features_batch(int n, const void *const *chw, void *const *out, const int *shape, int dtype_in,
                              int dtype_out, int sobel_normalized, int sobel_replicate_pad, int layout,
                              void *hip_stream);
/* Windowed f-only pack (FMPNP_LAYOUT_F) of n problems: only the texels within `radius` texels
 * (Chebyshev distance, radius >= 2) of a point's texel at the problem's initial pose (R0, t0) are
 * written to feat ([Hf][Wf][cstride] fp32, channels [c_end, cstride) zero), and window ([2][Hf][Wf]
 * bytes, see fmpnp_problem.window) records which: plane 1 marks the texels within radius - 1.
 * The reference's refinement reads only the 3x3 neighbourhoods of the texels its points visit
 * (optimize_feature_pnp.py:57-61 packs all of them), so a radius a little above the points' motion
 * in texels leaves most of the map unwritten and mostly unread.  probs_dev / probs_host: the same
 * descriptors in device / host memory (feat and window set, c_begin = 0, C = c_end channels);
 * chw[i]: map i, [c_end][Hf][Wf] of dtype_in.  Asynchronous on hip_stream. */
int fmpnp_pack_features_f_window_batch(const fmpnp_problem *probs_dev, const fmpnp_problem *probs_host, int n,
                                       const void *const *chw, int dtype_in, int radius, void *hip_stream);
int fmpnp_gather_reference_batch(int n, const void *const *ref_chw, const int *ref_shape,
                                 const double *const *ref_inliers, const int *n_inliers, int img0, int img1,
                                 void *const *out, const int *ld_out, int dtype_in, int dtype_out, int *err_flags,
                                 void *hip_stream);

/* Per-point residual costs at the descriptor's pose (R0, t0): the projection,
 * points_within_image and indexing_ of find_inliers (featurePnP/model.py:132-146).
 * supported[i] = 1 when point i's rounded pixel lies in the image, and then
 * cost[i] = 0.5 * sum over [c_begin, c_end) of (f(p_i) - fref_i)^2 (fp64), else 0.
 * cost ([N] fp64) and supported ([N] int32) are DEVICE arrays; the descriptor is host
 * memory; asynchronous on hip_stream.  layout / dtype as in fmpnp_options (FMPNP_LAYOUT_F
 * is fp32 only).  The façade's find_inliers applies the loss and the ratio mask. */
int fmpnp_point_costs(const fmpnp_problem *prob, int layout, int dtype, double *cost, int *supported,
                      void *hip_stream);

/* compute_cost (featurePnP/model.py:216-243) at the descriptor's pose (R0, t0): the mean over the
 * supported points -- after the ratio test when use_ratio (model.py:230-236) -- of
 * 0.5 ||f(p_i) - fref_i||^2 over [c_begin, c_end).  fmpnp_point_costs (one wave per point) into
 * cost / supported (DEVICE [N] fp64 / int32 scratch), then one fixed-order reduction into *result
 * (DEVICE): initial_cost (NaN when the ratio test keeps nothing), status FMPNP_STATUS_NO_SUPPORT when
 * no point is supported (the reference returns None), R / t = (R0, t0).  The descriptor is host
 * memory; asynchronous on hip_stream.  One evaluation: it is not an LM launch. */
int fmpnp_compute_cost_async(const fmpnp_problem *prob, int layout, int dtype, int use_ratio, double ratio_threshold,
                             double *cost, int *supported, fmpnp_result *result, void *hip_stream);

/* Device workspace needed by fmpnp_refine_batch_async for n problems (team exchange slots and,
 * for small batches, the first-evaluation helpers' records; no initialisation needed, reusable
 * by later launches on the same stream). */
size_t fmpnp_workspace_size(const fmpnp_problem *probs_host, int n, const fmpnp_options *opt);

/* Asynchronous batched refinement: descriptors, results and trace in DEVICE
 * memory; nothing is synchronised.  probs_host: the same descriptors in host memory
 * (required: the launch plan reads every problem's sizes and channel slice); max_N is
 * unused (kept for ABI stability). */
int fmpnp_refine_batch_async(const fmpnp_problem *probs_dev, const fmpnp_problem *probs_host, int n, int max_N,
                             const fmpnp_options *opt, fmpnp_result *results_dev, fmpnp_trace_entry *trace_dev,
                             int trace_stride, void *workspace, size_t workspace_bytes, void *hip_stream);

/* Synchronous convenience: host descriptors in, host results (and optional
 * trace, [n][trace_stride] entries) out.  Uploads descriptors, launches on
 * hip_stream and waits for that stream.  Its device workspace and pinned staging are this
 * (device, stream)'s own (see Threads above). */
int fmpnp_refine_batch(const fmpnp_problem *probs_host, int n, const fmpnp_options *opt, fmpnp_result *results,
                       fmpnp_trace_entry *trace, int trace_stride, void *hip_stream);

/* CPU twin of fmpnp_refine_batch: the same descriptors, options, results and trace
 * with HOST pointers -- feat (the packed [Hf][Wf][3][cstride] of fmpnp_pack_features, or the f-only
 * [Hf][Wf][cstride] of FMPNP_LAYOUT_F), fref and pts3d in host memory.  The LM loop of
 * sparseFeaturePnP.forward (featurePnP/model.py:245-494; compute_cost :216-243 with
 * FMPNP_MODE_COMPUTE_COST) on n_threads host threads (0: every core), one problem per thread at a
 * time.  Nearest sampling only (FMPNP_BILINEAR: FMPNP_EINVAL); no windows.  An explicit CPU entry
 * point -- the timed CPU baseline and a parity bridge -- never a fallback of the HIP entry points.
 * FMPNP_F16 storage: binary16 maps and fref in host memory, widened exactly (strides in multiples of 8 channels:
 * FMPNP_EALIGN otherwise).  Returns 0, FMPNP_EINVAL or FMPNP_EALIGN. */
int fmpnp_refine_batch_cpu(const fmpnp_problem *probs_host, int n, const fmpnp_options *opt, fmpnp_result *results,
                           fmpnp_trace_entry *trace, int trace_stride, int n_threads);

/* ---- dense exhaustive matching: the producer of the 2D-3D matches --------------------------------
 * (s2dhm/pose_prediction/exhaustive_search.py, keypoint_association.py; per reference image in
 *  sparse_to_dense_predictor.py:140-191).  All values fp32.
 *
 *   scores[i][j] = sum_k sparse[i][k] * dense[k][j]          torch.mm, exhaustive_search.py:45-46
 *       one fp32 fmaf chain per score over k = 0 .. C-1 in ascending order from +0 (the exact-fp32
 *       MFMA of gfx950 computes that chain): no split-K, no atomics, independent of the launch.
 *   per row i (retrieve_argmax, exhaustive_search.py:8-21):
 *       argmax[i]  the flat index of the maximum; the lowest index among equal maxima; NaN counts as
 *                  greater than everything (torch.topk) and the lowest NaN wins; -0 counts as +0
 *       top[i]     d1, the maximum                            dist_nn[0]
 *       kth[i]     d_k, the top_k-th largest value, an exact selection (an element of the row)
 *                                                             dist_nn[-1] of topk(top_k), :16
 *       mask[i]    (float)(ratio * ratio) * d1 >= d_k, one fp32 product           :17
 *   top_k = int(factor * W * H) (:13) is the caller's; top_k < 1 or > WH is FMPNP_EINVAL (the
 *   reference raises there).  ratio: retrieve_argmax's default 0.9 (:8). */

/* Device bytes fmpnp_exhaustive_match_async needs as workspace when it is not given a scores map: the
 * score rows of one round (the rows are processed in rounds of at most 256 MB of scores). */
size_t fmpnp_match_workspace_size(int N, int WH);

/* Asynchronous: every pointer is DEVICE memory, nothing is synchronised.  sparse [N][ld_sparse]
 * (ld_sparse >= C), dense [C][ld_dense] (ld_dense >= WH); argmax / top / kth / mask: [N].  scores: NULL,
 * or [N][WH] that receives the whole correlation map (workspace may then be NULL). */
int fmpnp_exhaustive_match_async(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH,
                                 int ld_dense, int top_k, double ratio, int *argmax, float *top, float *kth,
                                 unsigned char *mask, float *scores, void *workspace, size_t workspace_bytes,
                                 void *hip_stream);

/* The correlation alone (torch.mm, exhaustive_search.py:45-46): scores [N][WH] = sparse x dense under the
 * numeric contract above; DEVICE pointers, asynchronous on hip_stream (tools/match_bench.py times it). */
int fmpnp_correlation_async(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                            float *scores, void *hip_stream);

/* Synchronous: DEVICE sparse / dense (and scores_dev, NULL or [N][WH]), HOST argmax / top / kth / mask;
 * launches on hip_stream and waits for it.  Its device scratch is this (device, stream)'s own (see
 * Threads above). */
int fmpnp_exhaustive_match(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                           int top_k, double ratio, int *argmax, float *top, float *kth, unsigned char *mask,
                           float *scores_dev, void *hip_stream);

/* CPU twin of fmpnp_exhaustive_match: HOST pointers, the same contract (fmaf in ascending k), so its
 * scores (NULL or [N][WH]), argmax, top, kth and mask are the GPU's bit for bit.  n_threads host
 * threads (0: every core), rows in parallel.  An explicit CPU entry point, never a fallback.  Returns
 * 0, FMPNP_EINVAL or FMPNP_ENOMEM. */
int fmpnp_exhaustive_match_cpu(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH,
                               int ld_dense, int top_k, double ratio, int *argmax, float *top, float *kth,
                               unsigned char *mask, float *scores, int n_threads);

/* ---- fp16 precision of the match stage (opt-in) -------------------------------------------------------
 * The exact-fp32 contract above is the default of every entry point and of every caller that does not ask
 * otherwise.  FMPNP_MATCH_F16 trades it for the fp16 matrix rate (16 x the fp32 MFMA's); the hypercolumns it
 * is meant for are L2-normalised, elements around 1 / sqrt(C), well inside fp16's normal range.
 *
 *   Operands.  Each fp32 operand x is used as fl16(x): IEEE binary16, round-to-nearest-even.  NaN and +-Inf
 *       are kept; |x| >= 65520 becomes +-Inf (fl16 of anything above 65504 + half an ulp).  Whether an operand
 *       with |fl16(x)| < 2^-14 (an fp16 subnormal) is kept or taken as zero by the matrix instruction is
 *       UNSPECIFIED; the conversion itself keeps it, and so does the CPU reference.
 *   Score.  score[i][j] = sum_k fl16(a[i][k]) * fl16(b[k][j]).  The products are exact (22 significand bits fit
 *       fp32); they are accumulated in fp32 by v_mfma_f32_32x32x16_f16, the 16-deep k-blocks in ascending order
 *       into one accumulator per score that starts at +0.  No split-K, no atomics; zero-padded k tails are the
 *       only padding (they add exact zeros).
 *   Launch independence.  The bits of a score depend only on its row vector, its column vector and C: not on
 *       N, W*H, the tile or grid it landed in, the round, the stream or the workspace.  So one call over
 *       concatenated rows equals the separate calls bit for bit, as under the exact contract.
 *   Inner summation order.  The order (and any intermediate rounding) of the 16 products inside one MFMA is not
 *       documented.  The f16 precision therefore has NO bit-identical CPU twin: fmpnp_exhaustive_match_ex_cpu
 *       is its REFERENCE (below), and the GPU's scores lie within C * 2^-23 * sum_k |fl16(a)| |fl16(b)| +
 *       2^-24 |s| of it (twice the any-order fp32 summation bound).  On operands that are exact in fp16 and whose
 *       partial sums are exact in fp32 (small integers) every order gives the same bits, the exact twin's.
 *   Row reduction.  argmax, top, kth and mask come from the same select on these scores, with the same NaN /
 *       +-0 / tie rules and the same one-product mask.
 * Against the exact fp64 product of the fp32 operands a reference score is within
 * (2^-10 + 2^-22) * sum_k |a| |b| + 2^-24 |s| (each operand's relative error 2^-11, their cross term, the final
 * rounding), absent overflow and subnormal operands. */
typedef enum { FMPNP_MATCH_F32 = 0, FMPNP_MATCH_F16 = 1 } fmpnp_match_precision;

/* Device bytes the _ex entry points need as workspace.  FMPNP_MATCH_F32: fmpnp_match_workspace_size(N, WH).
 * FMPNP_MATCH_F16: the fp16 operand images (dense, k-blocked [ceil64(C) / 8][WH][8]; sparse, rows [N][ceil64(C)])
 * plus the score rows of one round.  0 for an unknown precision or an empty shape. */
size_t fmpnp_match_workspace_size_ex(int N, int C, int WH, int precision);

/* fmpnp_exhaustive_match_async / fmpnp_correlation_async / fmpnp_exhaustive_match with a precision.
 * FMPNP_MATCH_F32: the existing entry point, its bits (fmpnp_correlation_ex_async's workspace may be NULL).
 * FMPNP_MATCH_F16: both operands are converted once per call into the workspace (16-byte aligned), which is
 * required even when a scores map is given (then fmpnp_match_workspace_size_ex less the score rows of one round
 * suffices, as it does for fmpnp_correlation_ex_async).  Any other precision: FMPNP_EINVAL. */
int fmpnp_exhaustive_match_ex_async(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH,
                                    int ld_dense, int top_k, double ratio, int *argmax, float *top, float *kth,
                                    unsigned char *mask, float *scores, void *workspace, size_t workspace_bytes,
                                    int precision, void *hip_stream);
int fmpnp_correlation_ex_async(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                               float *scores, void *workspace, size_t workspace_bytes, int precision, void *hip_stream);
int fmpnp_exhaustive_match_ex(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                              int top_k, double ratio, int *argmax, float *top, float *kth, unsigned char *mask,
                              float *scores_dev, int precision, void *hip_stream);

/* FMPNP_MATCH_F32: fmpnp_exhaustive_match_cpu, the exact twin.  FMPNP_MATCH_F16: the REFERENCE of the f16
 * precision, not a twin: operands rounded to binary16 (nearest-even, subnormals kept), the exact products
 * accumulated in fp64 in ascending k, the sum rounded once to fp32; then the twin's key, select and mask. */
int fmpnp_exhaustive_match_ex_cpu(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH,
                                  int ld_dense, int top_k, double ratio, int *argmax, float *top, float *kth,
                                  unsigned char *mask, float *scores, int n_threads, int precision);

/* ---- layered matching (opt-in) ---------------------------------------------------------------------------
 * fmpnp_exhaustive_match_layers: the same scores from the query's encoder layers, correlated per layer at the
 * layer's own resolution, without the dense operand.  Its contract and entry points stand below, after the
 * hypercolumn sections, because they take fmpnp_hc_layer. */

/* fast_sparse_keypoint_descriptor over generate_dense_keypoints' grid (keypoint_association.py:7-86):
 * out[p][0..C) = the descriptor of the cell centre nearest to point p, without the [M x N] distance
 * matrix.  dense_chw [C][D1][D2] fp32, points2d [N][2] fp64, out [N][ld_out] fp32: DEVICE memory;
 * asynchronous on hip_stream.  The grid's centres are i * cell + cell / 2 per axis (:26-27): cell0 =
 * image_resolution[0] / D1 is the cell size along the map's first dimension, cell1 =
 * image_resolution[1] / D2 along its last -- the cell sizes generate_dense_keypoints returns (:38;
 * they, not the resolution, fix the centres).  Point coordinate 0 pairs with the last dimension
 * (i0 = clip(ceil(p0 / cell1 - 1), 0, D2 - 1)), coordinate 1 with the first (i1 likewise with cell0, D1);
 * the cell is i1 * D2 + i0 (:30-33,53-54).  A point exactly between two centres takes the lower cell,
 * as fast_closest_points' argmin does (:84-85). */
int fmpnp_gather_sparse_descriptors(const float *dense_chw, int C, int D1, int D2, const double *points2d, int N,
                                    double cell0, double cell1, float *out, int ld_out, void *hip_stream);

/* ---- P3P RANSAC and reprojection polish: the initial pose ------------------------------------------
 * (s2dhm/pose_prediction/solve_pnp.py:44-69: cv2.solvePnPRansac(iterationsCount=5000, SOLVEPNP_P3P), then
 *  cv2.solvePnP(useExtrinsicGuess, SOLVEPNP_ITERATIVE) on the inliers; once per reference image in
 *  sparse_to_dense_predictor.py:140-191).  It produces the pose, 3D points and inliers fmpnp_feature_pnp reads.
 *  Parity with OpenCV is UNPINNED: cv2 is not importable where this library is built and tested, so no
 *  golden vector was recorded from the reference; the tests pin the contract below instead.
 *
 * All arithmetic is fp64; every + - * / sqrt is one correctly rounded IEEE operation without contraction
 * (csrc/fmpnp_pnp_impl.h is the one definition, compiled into the kernels and the CPU twin), so a result
 * depends on neither the launch geometry nor the side that computed it.
 *
 *   Camera.  K row-major 3x3; fx = K[0], fy = K[4], cx = K[2], cy = K[5] are used (no skew, as OpenCV).
 *       dist = OpenCV's (k1, k2, p1, p2); n_dist must be 4 (FMPNP_EINVAL otherwise).  Forward model on
 *       normalised (x, y): r2 = x^2 + y^2, rad = 1 + k1 r2 + k2 r2^2,
 *       xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2), yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y, u = fx xd + cx,
 *       v = fy yd + cy.  Scoring and the polish use it.  The P3P bearings are (x, y, 1) of the observation
 *       undistorted once by 10 fixed-point iterations x <- (x0 - dx(x)) / rad(x) from x0 = (u - cx) / fx
 *       (OpenCV's undistortPoints scheme, a fixed count).  All-zero coefficients: the identity, exactly.
 *   Sampling.  mix64(seed, n): z = seed + 0x9E3779B97F4A7C15 n; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
 *       z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31 (splitmix64, 64-bit wrap-around).  Hypothesis h
 *       in [0, iters) makes draws j = 0..3: r_j = ((mix64(seed, 4 h + j + 1) >> 32) (M - j)) >> 32, and the
 *       sample's j-th point is the r_j-th index of [0, M), in ascending order, that draws 0..j-1 did not
 *       take.  Four draws whatever M >= 4 is (M = 4: a permutation of the four points); a function of
 *       (seed, h) alone.
 *   Minimal solver.  Lambda Twist (Persson & Nordberg, ECCV 2018) on the sample's first three points:
 *       the cubic's root by 7 to 50 Newton steps (it stops once |f| <= 1e-13), eigenvectors by sqrt, at most
 *       5 Gauss-Newton steps on the depths; only + - * / sqrt.  Solutions in the order (+v, tau1),
 *       (+v, tau2), (-v, tau1), (-v, tau2); kept: finite, three depths > 0 and |R R^T - I| <= 1e-6
 *       entrywise (a degenerate triple's output is not a rotation).  Of those, the one with the smallest
 *       squared reprojection error at the fourth point among those that put it at depth > 0; the lowest
 *       index on a tie; none: the hypothesis has no model and scores 0.
 *   Score.  Point i is an inlier iff its camera-frame depth is > 0 and its squared reprojection error is
 *       <= threshold^2 (a NaN anywhere makes it an outlier: the comparisons are false).  The score is the
 *       inlier count; the best hypothesis has the maximum count, the lowest h among equals (an integer
 *       maximum over the key count << 32 | ~h).  All iters hypotheses are always evaluated.
 *       Differences from OpenCV, by design: it stops early at confidence 0.99 and does not test depth.
 *   Polish.  min sum |pi(R X + t) - x|^2 over the best hypothesis's inliers (never re-derived), from that
 *       hypothesis: Levenberg-Marquardt with R <- exp([w]x) R, t <- t + dt, (H + lambda diag H) d = -g by
 *       Cholesky, lambda = 1e-3 at first, / 10 (not below 1e-15) after an accepted step (a strictly smaller
 *       finite cost), x 10 after a rejected or unsolvable one.  It stops when |d|^2 <= 1e-24 before the
 *       step is tried, when lambda > 1e12, or after 100 trial poses.  H (21 upper-triangle entries), g (6)
 *       and the cost are reduced in this order: lane l of 256 adds the inliers among points l, l + 256,
 *       l + 512, ... in ascending order from +0; then lane l += lane l + s for s = 128, 64, .., 1.
 *   fmpnp_pnp_result: R, t the polished pose (x_cam = R X + t); R_hyp, t_hyp the best hypothesis; cost
 *       the polish's sum at (R, t); polish_iters the trial poses evaluated. */

/* per-problem status bits of this stage (fmpnp_pnp_result.status); none is an error return */
#define FMPNP_PNP_OK 0
#define FMPNP_PNP_TOO_FEW 1        /* M < 4: nothing else of the result, and no mask byte, is written */
#define FMPNP_PNP_NO_MODEL 2       /* the best count is 0: num_inliers 0, best_h -1, poses and cost 0, mask 0 */
#define FMPNP_PNP_POLISH_FAILED 4  /* singular or non-finite polish: R, t = R_hyp, t_hyp, cost at that pose */

typedef struct {
    const double *points3d;  /* [M][3] world points */
    const double *points2d;  /* [M][2] observations, pixels */
    double K[9];             /* row-major */
    double dist[4];          /* k1, k2, p1, p2 */
    double threshold;        /* pixels, >= 0 */
    unsigned long long seed;
    long long mask_offset;   /* this problem's M bytes start here in the shared mask buffer */
    int M;
    int iters;               /* >= 1 */
    int n_dist;              /* the number of coefficients in dist: must be 4 */
    int reserved;
} fmpnp_pnp_problem;

typedef struct {
    double R[9], t[3];          /* polished */
    double R_hyp[9], t_hyp[3];  /* best hypothesis */
    double cost;
    int num_inliers, best_h, status, polish_iters;
} fmpnp_pnp_result;

/* Device bytes fmpnp_pnp_ransac_async needs as workspace for n problems (one 64-bit key each). */
size_t fmpnp_pnp_workspace_size(int n);

/* Asynchronous: probs_dev (with DEVICE points3d / points2d), results_dev, mask_dev ([mask_bytes]) and
 * workspace are DEVICE memory; probs_host: the same descriptors in host memory (sizes and validation;
 * its point pointers are not read).  Nothing is synchronised.  Every problem's [mask_offset,
 * mask_offset + M) must lie inside mask_bytes.  n <= 65535. */
int fmpnp_pnp_ransac_async(const fmpnp_pnp_problem *probs_dev, const fmpnp_pnp_problem *probs_host, int n,
                           fmpnp_pnp_result *results_dev, unsigned char *mask_dev, size_t mask_bytes,
                           void *workspace, size_t workspace_bytes, void *hip_stream);

/* Synchronous: HOST descriptors, results and mask; points_on_device != 0: points3d / points2d are DEVICE
 * pointers, else HOST pointers the call uploads.  Results and mask are zeroed first (so a FMPNP_PNP_TOO_FEW
 * problem reads as zeros).  Launches on hip_stream and waits for it; its device scratch is this (device,
 * stream)'s own (see Threads above). */
int fmpnp_pnp_ransac(const fmpnp_pnp_problem *probs_host, int n, int points_on_device, fmpnp_pnp_result *results,
                     unsigned char *mask, size_t mask_bytes, void *hip_stream);

/* CPU twin of fmpnp_pnp_ransac with HOST pointers: the same contract from the same code, so every result
 * field and mask byte equals the GPU's.  n_threads host threads (0: every core) over the hypotheses.
 * An explicit CPU entry point, never a fallback.  Returns 0, FMPNP_EINVAL or FMPNP_ENOMEM. */
int fmpnp_pnp_ransac_cpu(const fmpnp_pnp_problem *probs_host, int n, fmpnp_pnp_result *results, unsigned char *mask,
                         size_t mask_bytes, int n_threads);

/* The minimal solver alone: bearings [3][3] (any positive length) and world points [3][3] in, the kept
 * solutions (see above) out as R_out [4][9], t_out [4][3].  Returns their number, 0..4, or FMPNP_EINVAL. */
int fmpnp_p3p_cpu(const double *bearings, const double *points, double *R_out, double *t_out);

/* ---- localisation chain: the glue between the match, the initial pose and the refiner ----------------
 * (s2dhm/pose_prediction/sparse_to_dense_predictor.py:140-191 per reference image, :233-244 and
 *  predictor.py:48-73 per query).  Two kernels keep the chain on the device: the first turns the match
 *  stage's argmax / mask into the PnP stage's problems, the second picks the query's best prediction
 *  from the PnP stage's results and assembles the refiner's inputs.  No count ever reaches the host
 *  before the one download at the end.  csrc/fmpnp_localize_impl.h is the one definition of the
 *  arithmetic and of the decisions, compiled into the kernels and the CPU twins.
 *
 * A pair is (query q, reference j); the pairs of one query are contiguous and in rank order.  Pair p
 * owns the rows [row_offset, row_offset + n_rows) of the match output and of every per-row buffer below
 * (n_rows: the reference's count of visible 3D points, the pair's capacity; the pairs' ranges must not
 * overlap and must lie inside total_rows).
 *
 *   Build (per pair).  For each row i of the pair with mask[i] != 0, in ascending i, match m = 0, 1, ..:
 *       query2d_f32[m] the query point of exhaustive_search.py:18-19,51-54, formed in fp32 with every
 *                      operation rounded separately: a_x = argmax % dim[1], a_y = argmax / dim[1];
 *                      cell_k = (float)image_shape[k] / (float)dim[k];
 *                      x = (float)a_x * cell_0 + cell_0 / 2, y = (float)a_y * cell_1 + cell_1 / 2
 *       query2d[m]     the same two values widened to fp64 (the PnP stage's observations)
 *       points3d[m]    the pair's points3d[i];  ref2d[m] the pair's points2d[i];  src_row[m] = i
 *     counts[p] = the number of matches, and the pair's fmpnp_pnp_problem: pointers to its compacted
 *     query2d / points3d, K, dist, threshold, seed, iters, n_dist 4, mask_offset = row_offset, and
 *     M = count when count > minimum_matches (solve_pnp.py:44), else 0.  Rows m >= count are not written.
 *   Pick (per query).  Pair j is solved when its result's status is FMPNP_PNP_OK and num_inliers >=
 *     minimum_inliers (score num_inliers, pose the polished R, t); else a fallback when has_fallback
 *     (sparse_to_dense_predictor.py:179-189: score 0, pose fallback_R / fallback_t, all the pair's
 *     matches); else absent.  Of a result whose status is not FMPNP_PNP_OK nothing but the status is read.
 *     The best pair has the maximum score, the lowest j among equals (np.argmax, predictor.py:51).
 *     fmpnp_loc_record: best = j relative to the query's first pair (-1: no eligible pair), kind,
 *     num_matches = the best pair's count, num_inliers (0 for a fallback), N, R0, t0 (zeros when none).
 *     At the query's out_offset, compacted in ascending order, N rows each of pts3d, ref2d, query2d
 *     (fp32): the PnP inliers when solved and return_masked, else all the pair's matches
 *     (solve_pnp.py:99-111); and idx: the num_inliers positions of the PnP inliers in the pair's match list
 *     (the reference's inlier_mask; nothing for a fallback).  Rows past those counts, and everything of
 *     a query without an eligible pair but its record, are not written.  out_cap must be at least the
 *     largest n_rows among the query's pairs, and the queries' [out_offset, out_offset + out_cap) must
 *     lie inside total_rows without overlap.
 * No output depends on what a buffer held before the call. */
#define FMPNP_LOC_NONE 0
#define FMPNP_LOC_SOLVED 1
#define FMPNP_LOC_FALLBACK 2

typedef struct {
    const double *points3d;  /* [n_rows][3] the reference's 3D points */
    const double *points2d;  /* [n_rows][2] their observations in the reference image */
    double K[9], dist[4];    /* the reference's camera (fmpnp_pnp_problem) */
    double fallback_R[9], fallback_t[3];
    long long row_offset;
    float image_shape[2];    /* exhaustive_search's image_shape, as fp32 */
    int dim[2];              /* the query map's (width, height) */
    int n_rows;
    int has_fallback;
} fmpnp_loc_pair;

typedef struct {
    long long out_offset;
    int pair_begin, pair_count;
    int out_cap, reserved;
} fmpnp_loc_query;

typedef struct {
    double threshold;        /* solve_pnp's reprojection_threshold, pixels */
    unsigned long long seed;
    int iters, minimum_matches, minimum_inliers, return_masked;
} fmpnp_loc_params;

typedef struct {             /* the build step's outputs: [total_rows] rows each, counts [n_pairs] */
    float *query2d_f32;
    double *query2d, *points3d, *ref2d;
    int *src_row, *counts;
} fmpnp_loc_matches;

typedef struct {
    double R0[9], t0[3];
    int best, kind, num_matches, num_inliers, N, reserved;
} fmpnp_loc_record;

typedef struct {             /* the pick step's outputs: [total_rows] rows each, records [n_queries] */
    double *pts3d, *ref2d;
    float *query2d;
    int *idx;
    fmpnp_loc_record *records;
} fmpnp_loc_best;

/* Device bytes fmpnp_localize_async needs as workspace: the pairs' fmpnp_pnp_problems, then the PnP stage's. */
size_t fmpnp_localize_workspace_size(int n_pairs);

/* Asynchronous: build, fmpnp_pnp_ransac_async over all the pairs, pick, on hip_stream; nothing is
 * synchronised.  pairs_dev / queries_dev (and the pairs' point pointers), argmax / mask (the match
 * stage's outputs, [total_rows]), every pointer in matches and best, results_dev [n_pairs], pnp_mask_dev
 * [total_rows] and workspace (8-byte aligned) are DEVICE memory; pairs_host / queries_host: the same
 * descriptors in host memory (validation and grid sizes only).  n_pairs <= 65535 (FMPNP_ETOOBIG).
 * n_pairs == 0: only the records (all FMPNP_LOC_NONE) are written. */
int fmpnp_localize_async(const fmpnp_loc_pair *pairs_dev, const fmpnp_loc_pair *pairs_host, int n_pairs,
                         const fmpnp_loc_query *queries_dev, const fmpnp_loc_query *queries_host, int n_queries,
                         const fmpnp_loc_params *params, const int *argmax, const unsigned char *mask,
                         long long total_rows, const fmpnp_loc_matches *matches, const fmpnp_loc_best *best,
                         fmpnp_pnp_result *results_dev, unsigned char *pnp_mask_dev, void *workspace,
                         size_t workspace_bytes, void *hip_stream);

/* Where a pair's sparse descriptors come from: the reference's dense map (the rows are gathered by
 * fmpnp_gather_sparse_descriptors at the pair's points2d, straight into the concatenated row buffer), or,
 * when dense_chw is NULL, precomputed rows. */
typedef struct {
    const float *dense_chw;  /* DEVICE [C][D1][D2], or NULL */
    const float *sparse;     /* DEVICE [n_rows][ld_sparse], read when dense_chw is NULL */
    double cell0, cell1;     /* fmpnp_gather_sparse_descriptors' cell sizes */
    int D1, D2, ld_sparse, reserved;
} fmpnp_loc_source;

/* Synchronous: the whole chain up to the best prediction on hip_stream, with one upload, one pinned download
 * and one wait: the sparse-descriptor gathers, one fmpnp_exhaustive_match_async per query (its pairs' rows must
 * be contiguous and share dim; query_dense[q]: DEVICE [C][dim[0] * dim[1]], top_k[q], ratio as there), then
 * fmpnp_localize_async.  pairs (with HOST point pointers), sources, queries, top_k and every output are HOST
 * memory: best (rows up to the largest out_offset + out_cap), and, each NULL or given, all (every pair's
 * compacted matches, [total_rows] rows; only the rows the contract names are written), results [n_pairs]
 * and pnp_mask [total_rows] (both zeroed on the device first, so a FMPNP_PNP_TOO_FEW problem reads as zeros).
 * Its device scratch and pinned staging are this (device, stream)'s own (see Threads above). */
int fmpnp_localize(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                   const fmpnp_loc_query *queries, const float *const *query_dense, const int *top_k, int n_queries, int C,
                   double ratio, const fmpnp_loc_params *params, long long total_rows, const fmpnp_loc_best *best,
                   const fmpnp_loc_matches *all, fmpnp_pnp_result *results, unsigned char *pnp_mask, void *hip_stream);

/* fmpnp_localize with the match stage's precision (fmpnp_match_precision; FMPNP_MATCH_F32 is fmpnp_localize).
 * With FMPNP_MATCH_F16 each query's map is converted once and shared by all its pairs' rows; the results equal
 * the staged composition through fmpnp_exhaustive_match_ex_async bit for bit.  The match stage's scratch is the
 * stream's own, so fmpnp_localize_workspace_size does not change.  An unknown precision: FMPNP_EINVAL. */
int fmpnp_localize_ex(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                      const fmpnp_loc_query *queries, const float *const *query_dense, const int *top_k, int n_queries,
                      int C, double ratio, const fmpnp_loc_params *params, long long total_rows,
                      const fmpnp_loc_best *best, const fmpnp_loc_matches *all, fmpnp_pnp_result *results,
                      unsigned char *pnp_mask, int match_precision, void *hip_stream);

/* CPU twins of the two steps, HOST pointers, the same contract from the same code: every byte the contract
 * names equals the GPU's.  Compose them with fmpnp_exhaustive_match_cpu and fmpnp_pnp_ransac_cpu (probs:
 * [n_pairs], the problems to hand to it with mask_bytes = total_rows).  Explicit CPU entry points, never a
 * fallback.  Return 0, FMPNP_EINVAL or FMPNP_ETOOBIG. */
int fmpnp_localize_build_cpu(const fmpnp_loc_pair *pairs, int n_pairs, const fmpnp_loc_params *params,
                             const int *argmax, const unsigned char *mask, long long total_rows,
                             const fmpnp_loc_matches *matches, fmpnp_pnp_problem *probs);
int fmpnp_localize_pick_cpu(const fmpnp_loc_pair *pairs, int n_pairs, const fmpnp_loc_query *queries, int n_queries,
                            const fmpnp_loc_params *params, const fmpnp_pnp_result *results,
                            const unsigned char *pnp_mask, long long total_rows, const fmpnp_loc_matches *matches,
                            const fmpnp_loc_best *best);

/* One channel level of multilevel_optimization's pyramid (featurePnP/model.py:193-210): the
 * channel range [c_begin, c_end) of the query map (input_configs/default_robotcar.gin:75). */
typedef struct {
    int c_begin, c_end;
} fmpnp_level;

/* ---- batched refinement of the chain's winners (opt-in: the per-query fmpnp_feature_pnp stays the default) ----
 * After the pick nothing of a query needs the host: its record, the compacted pts3d / ref2d at its out_offset
 * and the reference the device chose are all in device memory.  This stage assembles every query's refiner
 * problem there, gathers its reference descriptors, and runs compute_cost and every channel level as launches
 * over all n_queries queries, queued behind fmpnp_localize_async on the same stream.
 *
 *   Contract.  For a query q whose record has kind SOLVED or FALLBACK the results are those of
 *     fmpnp_feature_pnp on that query, bit for bit, called with window_radius = 0, the best pair's reference map
 *     (fmpnp_loc_refine_source), the record's N rows of best.ref2d / best.pts3d, the record's R0, t0, the K of
 *     the query's LAST pair (FMPNP_LOC_K_LAST: sparse_to_dense_predictor.py:143,167,244) or of the best pair
 *     (FMPNP_LOC_K_BEST), and the same fmpnp_options, levels, img0, img1.  results is fmpnp_result
 *     [n_queries][n_res]: n_res = 1 without levels, 1 + n_levels with levels (slot 0: compute_cost), as
 *     fmpnp_feature_pnp's.  flags [n_queries]: non-zero when one of the query's inliers maps outside its
 *     reference map (or is NaN); that row of fref is zeroed -- the per-query call's FMPNP_ERANGE.
 *     A query of kind NONE, or whose best pair has a NULL source, gets N = 0: nothing of it is read through a
 *     pointer, its results are unspecified (written, never out of bounds).
 *   Launches.  loc_refine_prep_kernel (one workgroup per query: the n_res fmpnp_problem descriptors, N from
 *     the record, pts3d = best.pts3d + 3 out_offset, fref = the row slab + out_offset cstride, feat = the query's
 *     packed map, window NULL, c_begin / c_end per level, and the flag cleared); loc_refine_gather_kernel (the
 *     rows of every query in one grid sized from out_cap, blocks beyond the device's N exit; fmpnp_gather_reference's
 *     convention: col = trunc(x H_ref / img0), row = trunc(y W_ref / img1), a row in [-H_ref, 0) / col in
 *     [-W_ref, 0) wraps, conversion to the storage dtype, channels [C, cstride) zero); with levels the batched
 *     point costs (grid (ceil(cap / 4), n_queries)) and cost mean (one workgroup per query: fmpnp_compute_cost_async's
 *     arithmetic and reduction order); then one fmpnp_refine_batch_async per level over the n_queries descriptors,
 *     whose HOST descriptors carry N = out_cap (the plan's capacity; the kernels read N from the device), and
 *     between levels one small kernel that stores every query's result and copies its pose into the next
 *     level's R0 / t0.  Every kernel is bounded by its grid and counts: no waits between workgroups, no atomics
 *     but the flag's atomicOr.
 *   Untouched bytes.  fref rows, costs and anything else past a query's N are not written; no output depends on
 *     what a buffer held before the call. */
#define FMPNP_LOC_K_LAST 0
#define FMPNP_LOC_K_BEST 1
#define FMPNP_LOC_REFINE_MAX_LEVELS 32

typedef struct {              /* per PAIR: the reference map the refinement reads when the pair is the best */
    const void *ref_chw;      /* DEVICE [C][H_ref][W_ref] of dtype, or NULL (the query then gets N = 0) */
    int dtype, H_ref, W_ref, reserved;
} fmpnp_loc_refine_source;

typedef struct {              /* per QUERY: its packed map (fmpnp_pack_features, FMPNP_LAYOUT_FGRAD) */
    const void *feat;         /* DEVICE [Hf][Wf][3][cstride] of the storage dtype */
    int Hf, Wf;
} fmpnp_loc_refine_map;

typedef struct {
    int C, cstride;           /* the maps' channels; the row stride of the packed maps and of fref (>= C) */
    int img0, img1;           /* fmpnp_feature_pnp's */
    int intrinsics;           /* FMPNP_LOC_K_LAST / FMPNP_LOC_K_BEST */
    int n_levels;             /* 0 .. FMPNP_LOC_REFINE_MAX_LEVELS */
    const fmpnp_level *levels; /* HOST [n_levels] */
} fmpnp_loc_refine_params;

typedef struct {              /* DEVICE buffers of the stage; R = the largest out_offset + out_cap */
    fmpnp_problem *probs;     /* [n_res][n_queries]: level r's descriptors are contiguous (one launch each) */
    void *fref;               /* [R][cstride] of the storage dtype */
    double *cost;             /* [R] compute_cost's per-point costs (levels only; else may be NULL) */
    int *supported;           /* [R] (levels only; else may be NULL) */
    fmpnp_result *results;    /* [n_queries][n_res] */
    int *flags;               /* [n_queries] */
} fmpnp_loc_refine_buffers;

/* Device bytes fmpnp_localize_refine_async needs as workspace: the LM launches' (the largest level's plan at
 * N = out_cap) and, with levels, one level's results.  0 for invalid arguments or a capacity the LM plan
 * cannot take (fmpnp_localize_refine_async then reports which). */
size_t fmpnp_localize_refine_workspace_size(const fmpnp_loc_query *queries_host, int n_queries,
                                            const fmpnp_loc_refine_map *maps_host,
                                            const fmpnp_loc_refine_params *params, const fmpnp_options *opt);

/* Asynchronous: queued on hip_stream behind fmpnp_localize_async, which wrote best (records included) there;
 * nothing is synchronised.  pairs_dev / queries_dev / sources_dev [n_pairs] / maps_dev [n_queries], every
 * pointer in best and buffers, and workspace (256-byte aligned) are DEVICE memory; queries_host / maps_host:
 * the same descriptors in host memory (capacities and sizes only).  opt: FMPNP_MODE_FORWARD,
 * FMPNP_LAYOUT_FGRAD; opt->dtype is the storage of the packed maps and of fref.  A capacity whose LM plan does
 * not fit returns FMPNP_ETOOBIG before anything is queued. */
int fmpnp_localize_refine_async(const fmpnp_loc_pair *pairs_dev, int n_pairs, const fmpnp_loc_query *queries_dev,
                                const fmpnp_loc_query *queries_host, int n_queries,
                                const fmpnp_loc_refine_source *sources_dev, const fmpnp_loc_refine_map *maps_dev,
                                const fmpnp_loc_refine_map *maps_host, const fmpnp_loc_refine_params *params,
                                const fmpnp_options *opt, const fmpnp_loc_best *best,
                                const fmpnp_loc_refine_buffers *buffers, void *workspace, size_t workspace_bytes,
                                void *hip_stream);

/* Synchronous: fmpnp_localize_ex followed by the refinement stage, with ONE upload (it also carries the pairs'
 * refine sources), ONE pinned download (the records, the best arrays, the results and the flags) and ONE host
 * wait.  The queries' maps (query_dense[q]: DEVICE fp32 [C][Hf * Wf], query_hw[2 q ..] = Hf, Wf with
 * Hf * Wf = the pairs' dim[0] * dim[1]) are packed (fmpnp_pack_features_batch's launches, opt->sobel_flags,
 * cstride = C rounded up to 4) into the stream's scratch ahead of the match.  refine_sources: HOST [n_pairs]
 * with DEVICE maps of C channels; refine_results: HOST [n_queries][n_res]; refine_flags: HOST [n_queries].
 * Every other argument is fmpnp_localize_ex's.  Its device scratch and pinned staging are this (device,
 * stream)'s own (see Threads above). */
int fmpnp_localize_refined(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                           const fmpnp_loc_query *queries, const float *const *query_dense, const int *top_k,
                           int n_queries, int C, double ratio, const fmpnp_loc_params *params, long long total_rows,
                           const fmpnp_loc_best *best, const fmpnp_loc_matches *all, fmpnp_pnp_result *results,
                           unsigned char *pnp_mask, int match_precision,
                           const fmpnp_loc_refine_source *refine_sources, const int *query_hw,
                           const fmpnp_loc_refine_params *refine_params, const fmpnp_options *opt,
                           fmpnp_result *refine_results, int *refine_flags, void *hip_stream);

/* CPU twin of the prep and gather kernels, HOST pointers throughout (the sources' maps and best too): the
 * descriptors ([n_res][n_queries]; their pointer fields point into the host arrays), the fref rows and the
 * flags, from the same code (csrc/fmpnp_localize_impl.h), bit for bit.  dtype: the storage of fref.  An explicit
 * CPU entry point, never a fallback.  Returns 0 or FMPNP_EINVAL. */
int fmpnp_localize_refine_prep_cpu(const fmpnp_loc_pair *pairs, int n_pairs, const fmpnp_loc_query *queries,
                                   int n_queries, const fmpnp_loc_refine_source *sources,
                                   const fmpnp_loc_refine_map *maps, const fmpnp_loc_refine_params *params, int dtype,
                                   const fmpnp_loc_best *best, fmpnp_problem *probs, void *fref, int *flags);

/* Hypercolumn assembly: the second half of ImageRetrievalModel.compute_hypercolumn (s2dhm/network/network.py:
 * 149-173) in one kernel -- every layer resized to the output size (bilinear, align_corners=True), the layers
 * concatenated along the channels, each texel's channel vector divided by its L2 norm.  No weights: the
 * convolutions that produce the layers stay with the caller.
 *
 * Numeric contract (fmpnp_hypercolumn_assemble and its CPU twin implement it with the same code,
 * csrc/fmpnp_hypercolumn_impl.h; results are the same bits for every launch shape and thread count):
 *   Inputs.  L layers, 1 <= L <= 8; layer l is fp32 [B][C_l][H_l][W_l], element (b, c, y, x) at
 *       data[b * stride_b + c * stride_c + y * stride_y + x] (strides in elements, >= 0, stride_y >= W_l).  The
 *       output is fp32 [B][C][H][W], C = sum C_l, element (b, c, y, x) at out[b * out_stride_b + c * out_stride_c
 *       + y * out_stride_y + x]: it may be a view into a larger buffer, of any 4-byte alignment; no other byte of
 *       that buffer is written.  The channels of layer l follow those of layer l - 1.  Every size is <= 2^24.
 *   Interpolation.  Per output texel (y, x) and layer, per axis (n_in the layer's size, n_out the output's, d
 *       the output coordinate): scale = (float)(n_in - 1) / (float)(n_out - 1), one fp32 division (0 when
 *       n_out == 1); src = scale * (float)d, one fp32 product; i0 = min((int)src, n_in - 1);
 *       i1 = i0 + (i0 < n_in - 1); w1 = src - (float)i0; w0 = 1.0f - w1.  With a, b the layer's values at
 *       (y0, x0), (y0, x1) and c, d those at (y1, x0), (y1, x1):
 *           top = w0x * a + w1x * b;  bot = w0x * c + w1x * d;  v = w0y * top + w1y * bot,
 *       every operation a separate fp32 rounding (no contraction): the operation order of PyTorch's GPU
 *       kernel for align_corners=True.  Equal sizes make it an exact copy of finite values; a larger layer is
 *       sampled without antialiasing, as interpolate does.
 *   Normalisation (FMPNP_HC_NORMALIZE).  Per output texel the sum of squares over the concatenated channel
 *       index c, in fp64: the channels fall in blocks [64 k, 64 k + 64) (the last one ragged; blocks may
 *       straddle layers; 64 is part of the contract); a block's partial is the chain
 *       acc = fma((double)v, (double)v, acc) from +0 in ascending c; the partials are added in ascending k
 *       from +0; n = (float)sqrt(sum); out = v / n, one correctly rounded fp32 division.  Without the flag
 *       out = v.
 *   Edge cases.  A texel whose channels are all zero gives 0 / 0 = NaN in every channel, as the reference
 *       does; NaN and Inf inputs propagate by the same arithmetic (a tap of weight 0 on an Inf is a NaN). */
typedef struct {
    const float *data;
    int C, H, W, reserved;
    long long stride_b, stride_c, stride_y;
} fmpnp_hc_layer;

#define FMPNP_HC_NORMALIZE 1      /* divide by the L2 norm over the channels */
/* launch knobs (the results do not depend on them); neither: the library's choice */
#define FMPNP_HC_DWORD_STORES 2  /* 4-byte stores, 64 texels of a row per workgroup */
#define FMPNP_HC_VECTOR_STORES 4  /* 16-byte stores, 256 texels per workgroup, where the output's alignment allows */

/* Asynchronous: layers is HOST memory (L descriptors, copied into the kernel's arguments) whose data pointers,
 * like out, are DEVICE memory.  One kernel on hip_stream; nothing is synchronised, nothing allocated.
 * FMPNP_EINVAL: L outside 1..8, B, H, W or a layer's C, H, W < 1, a null pointer, a negative stride, a row
 * stride below its width, unknown flags.  FMPNP_ETOOBIG: a size above 2^24, or more than 2^31 - 8 tiles. */
int fmpnp_hypercolumn_assemble_async(const fmpnp_hc_layer *layers, int L, int B, float *out, int H, int W,
                                     long long out_stride_b, long long out_stride_c, long long out_stride_y,
                                     int flags, void *hip_stream);

/* Synchronous: the same, then waits for hip_stream. */
int fmpnp_hypercolumn_assemble(const fmpnp_hc_layer *layers, int L, int B, float *out, int H, int W,
                               long long out_stride_b, long long out_stride_c, long long out_stride_y, int flags,
                               void *hip_stream);

/* CPU twin with HOST pointers: the same contract from the same code, so every output element equals the
 * GPU's bit for bit.  n_threads host threads (0: every core) over the output rows.  An explicit CPU entry
 * point, never a fallback.  Returns 0, FMPNP_EINVAL, FMPNP_ETOOBIG or FMPNP_ENOMEM. */
int fmpnp_hypercolumn_assemble_cpu(const fmpnp_hc_layer *layers, int L, int B, float *out, int H, int W,
                                   long long out_stride_b, long long out_stride_c, long long out_stride_y,
                                   int flags, int n_threads);

/* Sparse hypercolumns: the hypercolumn's descriptors at N points, formed straight from the layers -- the dense
 * [B][C][H][W] map is never written.  A texel of the assembly depends only on each layer's 2 x 2 taps at that
 * texel, so the rows equal "assemble, then gather" bit for bit:
 *
 *   Output value.  out[p * ld_out + c], for c < C = sum C_l, is exactly the value fmpnp_hypercolumn_assemble*
 *       writes at (item[p], c, row_p, col_p) of a [B][C][H][W] output with the same flags & FMPNP_HC_NORMALIZE:
 *       the same scale division, taps, weights and bilerp order, the same fp64 chains over the blocks
 *       [64 k, 64 k + 64) of the concatenated channel index added in ascending k from +0, n = (float)sqrt(sum)
 *       and the same single fp32 division, all from the functions of csrc/fmpnp_hypercolumn_impl.h built
 *       without contraction.  dtype_out is FMPNP_F32, or FMPNP_F64: the fp32 value widened (exact).
 *   Index of a point (`at`; the rules are csrc/fmpnp_hypercolumn_impl.h's locate()):
 *       FMPNP_HC_AT_TEXEL      points is int32 [N][2] = (row, col); out of [0, H) x [0, W) is an error.
 *       FMPNP_HC_AT_REFERENCE  points is fp64 [N][2] = (x, y), p0, p1 = img0, img1: fmpnp_gather_reference's index,
 *                              col = (int)((double)H / img0 * x), row = (int)((double)W / img1 * y) (the swap is
 *                              the reference's); a row in [-H, 0) / a col in [-W, 0) wraps; anything else outside
 *                              the map, or a NaN coordinate, is an error.
 *       FMPNP_HC_AT_CELL       points is fp64 [N][2], p0, p1 = cell0, cell1: fmpnp_gather_sparse_descriptors'
 *                              index with D1 = H, D2 = W, col = clip(ceil(x / cell1 - 1), 0, W - 1), row likewise
 *                              from y, cell0 and H; NaN gives 0.  This mode never errors.
 *       item: NULL (item 0 for every point) or int32 [N]; an item outside [0, B) is an error.
 *   Errors.  An error row is written as zeros in [0, C) and ORs 1 into *err_flag (never reset here; it may be
 *       NULL in the async form).  No address is ever formed from a bad point.
 *   Untouched bytes.  Only elements [0, C) of rows [0, N) are written.  N == 0 returns 0 and launches nothing.
 *   Independence.  A row's bits depend only on its own point: not on N, the order of the points, duplicates,
 *       the launch shape or (when C exceeds what the kernel keeps on chip) the path a launch takes.
 *   Arguments.  The layers and sizes as fmpnp_hypercolumn_assemble (FMPNP_EINVAL / FMPNP_ETOOBIG); ld_out < C,
 *       N < 0, an unknown `at`, dtype or flag (only FMPNP_HC_NORMALIZE is known here), p0 or p1 not > 0 for the
 *       two fp64 modes, a null points or out with N > 0: FMPNP_EINVAL. */
#define FMPNP_HC_AT_TEXEL 0     /* points: int32 [N][2] = (row, col) of the H x W hypercolumn */
#define FMPNP_HC_AT_REFERENCE 1 /* points: fp64 [N][2] = (x, y); fmpnp_gather_reference's index */
#define FMPNP_HC_AT_CELL 2      /* points: fp64 [N][2]; fmpnp_gather_sparse_descriptors' index */

/* Asynchronous: layers is HOST memory; the layers' data, points, item, out and err_flag are DEVICE memory.  One
 * kernel on hip_stream (one workgroup per point); nothing is synchronised, nothing allocated. */
int fmpnp_hypercolumn_sparse_async(const fmpnp_hc_layer *layers, int L, int B, int H, int W, const void *points,
                                   const int *item, int N, int at, double p0, double p1, void *out, int dtype_out,
                                   long long ld_out, int flags, int *err_flag, void *hip_stream);

/* Synchronous: the same, then waits for hip_stream.  err_flag: a DEVICE int the caller has zeroed, or NULL (the
 * library then uses one of its own).  Returns FMPNP_ERANGE when the flag was set (the other rows are valid). */
int fmpnp_hypercolumn_sparse(const fmpnp_hc_layer *layers, int L, int B, int H, int W, const void *points,
                             const int *item, int N, int at, double p0, double p1, void *out, int dtype_out,
                             long long ld_out, int flags, int *err_flag, void *hip_stream);

/* CPU twin with HOST pointers (err_flag too; NULL allowed): the same contract from the same code, bit for bit.
 * n_threads host threads (0: every core) over the points.  Returns FMPNP_ERANGE when a row was an error row (the
 * other rows are valid).  An explicit CPU entry point, never a fallback. */
int fmpnp_hypercolumn_sparse_cpu(const fmpnp_hc_layer *layers, int L, int B, int H, int W, const void *points,
                                 const int *item, int N, int at, double p0, double p1, void *out, int dtype_out,
                                 long long ld_out, int flags, int *err_flag, int n_threads);

/* ---- Packed hypercolumns: the encoder's layers straight into the refiner's layout ------------------------
 * fmpnp_hypercolumn_pack* write batch item `item` of the hypercolumn of the layers (as fmpnp_hypercolumn_assemble
 * takes them), at output size H x W, as the packed map the LM kernel gathers from -- [H][W][3][cstride] =
 * (f, gx, gy) of dtype_out (FMPNP_LAYOUT_FGRAD) or [H][W][cstride] fp32 (FMPNP_LAYOUT_F, cstride a multiple of
 * 4) -- without the dense [C][H][W] map in between.
 *
 *   Defining property.  Every element written is, bit for bit (NaNs by position), the one that
 *       fmpnp_hypercolumn_assemble (same layers, size, flags & FMPNP_HC_NORMALIZE) followed by
 *       fmpnp_pack_features (same Sobel flags, dtype_out) / fmpnp_pack_features_f writes there.
 *   Values.  A texel's f is the assembly's contract above: taps, weights, each fp32 rounding, the fp64 chains over
 *       the blocks [64 k, 64 k + 64) of the FULL concatenated channel index (whatever the channel range),
 *       n = (float)sqrt(sum) and one correctly rounded fp32 division; zero texels and non-finite inputs behave as
 *       there.  The Sobel reads that (normalised) map with zero padding, or replicate padding
 *       (sobel_replicate_pad); with a, d, g the widened values of a column of the 3 x 3 window from top to bottom,
 *       sx = (a + 2 d) + g and sy = g - a per column in fp64, gx = sx(x+1) - sx(x-1),
 *       gy = (sy(x-1) + 2 sy(x)) + sy(x+1), times 0.125 with sobel_normalized, each rounded once to dtype_out
 *       (csrc/fmpnp_hypercolumn_pack_impl.h; the Sobel pack's association for fp32 maps).
 *   What is written.  Only channels [c_begin, c_end) of the concatenated channels, of the texels whose byte in
 *       marks ([H][W], the plane-0 format of fmpnp_problem.window; NULL: every texel) is non-zero, in all three
 *       planes (FMPNP_LAYOUT_FGRAD).  Padding channels, unmarked texels and every other byte of the buffer stay
 *       as they are: a caller who wants zero padding channels zeroes them once.
 *   Workspace.  With FMPNP_HC_NORMALIZE the norms are formed first, one fp32 per texel, in `workspace`
 *       (fmpnp_hypercolumn_pack_workspace_size(H, W) bytes of DEVICE memory, 4-byte aligned); they do not depend
 *       on the channel range.  Without the flag workspace may be NULL.
 *   Arguments.  The layers and sizes as fmpnp_hypercolumn_assemble (FMPNP_EINVAL / FMPNP_ETOOBIG; H * W >= 2^31
 *       is FMPNP_ETOOBIG); item outside [0, B), an empty or out-of-range channel range, cstride < C, an unknown
 *       flag (only FMPNP_HC_NORMALIZE is known), layout or dtype, FMPNP_LAYOUT_F with fp64 storage or a cstride
 *       that is no multiple of 4, a null out, a missing or short workspace: FMPNP_EINVAL; out or workspace not
 *       aligned to its element: FMPNP_EALIGN.  Nothing is written then. */
size_t fmpnp_hypercolumn_pack_workspace_size(int H, int W); /* 0: invalid size */

/* Asynchronous: layers is HOST memory; the layers' data, marks, out and workspace are DEVICE memory.  Two kernels
 * on hip_stream (one without FMPNP_HC_NORMALIZE); nothing is synchronised, nothing allocated. */
int fmpnp_hypercolumn_pack_async(const fmpnp_hc_layer *layers, int L, int B, int item, int H, int W, int flags,
                                 int c_begin, int c_end, int layout, int dtype_out, int cstride, int sobel_normalized,
                                 int sobel_replicate_pad, const unsigned char *marks, void *out, void *workspace,
                                 size_t workspace_bytes, void *hip_stream);

/* Synchronous: the same, then waits for hip_stream.  workspace NULL: the library uses one of its own. */
int fmpnp_hypercolumn_pack(const fmpnp_hc_layer *layers, int L, int B, int item, int H, int W, int flags, int c_begin,
                           int c_end, int layout, int dtype_out, int cstride, int sobel_normalized,
                           int sobel_replicate_pad, const unsigned char *marks, void *out, void *workspace,
                           size_t workspace_bytes, void *hip_stream);

/* CPU twin with HOST pointers (no workspace: it keeps the norms itself): the same contract from the same code,
 * bit for bit.  n_threads host threads (0: every core) over the output rows.  An explicit CPU entry point, never a
 * fallback.  Returns 0, FMPNP_EINVAL, FMPNP_EALIGN, FMPNP_ETOOBIG or FMPNP_ENOMEM. */
int fmpnp_hypercolumn_pack_cpu(const fmpnp_hc_layer *layers, int L, int B, int item, int H, int W, int flags,
                               int c_begin, int c_end, int layout, int dtype_out, int cstride, int sobel_normalized,
                               int sobel_replicate_pad, const unsigned char *marks, void *out, int n_threads);

/* ---- layered matching (opt-in): the match stage's scores straight from the query's layers -----------------
 * (the block after "fp16 precision of the match stage"; it stands here because it takes fmpnp_hc_layer.)
 * The align_corners=True bilinear resize is linear in the layer's values and its weights depend on the texel only,
 * so the unnormalised score of descriptor d at texel p is
 *     sum_l sum_c d[off_l + c] * resize(layer_l[c])(p)  =  sum_l resize( sum_c d[off_l + c] * layer_l[c] )(p):
 * the correlation runs on each layer at the layer's own resolution, and the small score maps are resized and
 * summed.  The dense [C][H * W] operand of fmpnp_exhaustive_match is never formed.  Numeric contract
 * (fmpnp_exhaustive_match_layers and its CPU twin implement it with the same code,
 * csrc/fmpnp_match_layers_impl.h over csrc/fmpnp_hypercolumn_impl.h, built without contraction):
 *   Inputs.  L layers (1 <= L <= 8) as fmpnp_hypercolumn_assemble takes them, a batch item `item` (0 <= item < B),
 *       the output size H x W, sparse [N][ld_sparse] with ld_sparse >= C = sum C_l; off_l = sum of C_m, m < l.
 *       Every layer plane must be contiguous, stride_y == W_l and stride_c >= H_l * W_l (the correlation reads
 *       layer l as [C_l][H_l * W_l] with ld = stride_c); otherwise FMPNP_EINVAL.
 *   Coarse scores.  S_l[i][q] = sum_c sparse[i][off_l + c] * layer_l[item][c][q]: the contract of dense exhaustive
 *       matching above -- one fp32 fmaf chain from +0 over c = 0 .. C_l - 1 ascending, no split-K, no atomics.
 *   Resize.  r_l = the bilerp of the assembly contract on S_l[i] at output texel (y, x): the same scale division,
 *       taps, weights and operation order, for every layer, equal-size ones included.
 *   Sum.  t = r_0, then t = t + r_l for l = 1 .. L - 1, each add its own fp32 rounding.
 *   Norm (FMPNP_HC_NORMALIZE).  n(y, x) is exactly the n of the assembly contract (fp64 chains over the 64-channel
 *       blocks of the concatenated index, partials in ascending order, (float)sqrt); score = t / n, one correctly
 *       rounded fp32 division.  Without the flag score = t.
 *   Layout.  score[i][y * W + x]: the column index of the assembled [C][H][W] map viewed as [C][H * W], so argmax
 *       means what it means for fmpnp_exhaustive_match on that map.
 *   Non-finite values.  The arithmetic above is applied literally: a texel that is zero in every channel scores
 *       0 / 0 = NaN in every row, as the dense path does; NaN and Inf propagate by the same operations in the
 *       kernel and the twin.
 *   Row reduction.  argmax, top, kth and mask: the select of dense exhaustive matching on these scores.
 *   Independence.  A row's bits depend on its descriptor, the layers, item and (H, W) only: not on N, the round,
 *       the workspace, the stream or the launch shape.
 *   Relation to the dense path.  The result is NOT fmpnp_exhaustive_match's bits on the assembled map: the rounding
 *       order differs.  Without normalisation the two agree bit for bit on operands whose every intermediate is
 *       exact (small integers with equal-size layers, or resizes with dyadic weights such as 3 -> 5).  In general
 *       both lie within `bound` of the exact value (real arithmetic, resize weights without rounding).  With
 *       u = 2^-24, g(k) = k u / (1 - k u), w_l = 4 u (H_l + W_l - 2), R = the exact resize, a = layer_l[item][c]:
 *           M(i, p) = sum_l sum_c |d[off_l + c]| * R(|a|)(p)
 *           G(i)    = sum_l w_l sum_c |d[off_l + c]| * max_q |a[q]|
 *           E_t     = g(C + L + 5) * (M + G) + G                                   (the bound without the flag)
 *           dn(p)   = sqrt( sum_l sum_c ( g(5) * R(|a|)(p) + w_l * max_q |a[q]| )^2 ) + u * n(p),  rho = dn / n
 *           E       = (E_t + M * rho) / (n * (1 - rho)),      bound = E + u * (M / n + E)
 *       (n: the exact norm.)  g(C + L + 5): any order of an fp32 sum of at most C products (the per-layer chains,
 *       or the dense path's one chain) with the five roundings of a bilerp and its w0 = 1 - w1, the L - 1 adds
 *       and, on the dense path, the element's own division; G: the resize weights' rounding, at most 2 u (n_in - 1)
 *       in a source coordinate per axis, against a slope of at most twice the layer's largest magnitude; rho: the
 *       norm's relative error from the same two causes, and the cast of the square root.  DESIGN.md 4.8.2 derives
 *       it; it is not fitted to observed errors.
 * FMPNP_EINVAL: L, sizes, strides, item, ld_sparse < C, top_k outside 1 .. H * W, a NaN ratio, unknown flags, null
 * pointers, a workspace too small for one row.  FMPNP_ETOOBIG: as fmpnp_hypercolumn_assemble, or a map of more
 * than 2^31 - 2^16 - 1 texels. */

/* Device bytes the layered entry points need as workspace when they are not given a scores map: the norm plane
 * (H * W floats, 256-byte aligned), then the coarse maps and the score rows of one round.  The rows go in rounds
 * of at most 256 MB of coarse maps and score rows (one row at least).  0 for an invalid shape. */
size_t fmpnp_match_layers_workspace_size(const fmpnp_hc_layer *layers, int L, int N, int H, int W);

/* Asynchronous: layers is HOST memory (L descriptors) whose data pointers are DEVICE memory, as every other
 * pointer; nothing is synchronised.  argmax / top / kth / mask: [N].  scores: NULL, or [N][H * W] that receives
 * the whole score map; it takes the score rows' place in the workspace.  workspace: 16-byte aligned; a workspace
 * that holds fewer rows than fmpnp_match_layers_workspace_size asks for makes the rounds shorter (at least one row;
 * no result depends on it).  Launches per round: one correlation per layer, the combine, the select; the norm
 * plane is formed once per call. */
int fmpnp_exhaustive_match_layers_async(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L,
                                        int B, int item, int H, int W, int flags, int top_k, double ratio, int *argmax,
                                        float *top, float *kth, unsigned char *mask, float *scores, void *workspace,
                                        size_t workspace_bytes, void *hip_stream);

/* The score map alone: scores [N][H * W] (required) under the contract above; the workspace then holds the norm
 * plane and one round's coarse maps (tools/match_bench.py times it). */
int fmpnp_correlation_layers_async(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L, int B,
                                   int item, int H, int W, int flags, float *scores, void *workspace,
                                   size_t workspace_bytes, void *hip_stream);

/* Synchronous: DEVICE sparse / layer data (and scores_dev, NULL or [N][H * W]), HOST argmax / top / kth / mask;
 * launches on hip_stream and waits for it.  Its device scratch is this (device, stream)'s own (see Threads above). */
int fmpnp_exhaustive_match_layers(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L, int B,
                                  int item, int H, int W, int flags, int top_k, double ratio, int *argmax, float *top,
                                  float *kth, unsigned char *mask, float *scores_dev, void *hip_stream);

/* CPU twin with HOST pointers: the same contract from the same code, so its scores (NULL or [N][H * W]), argmax,
 * top, kth and mask are the GPU's bit for bit.  n_threads host threads (0: every core), rows in parallel.  An
 * explicit CPU entry point, never a fallback.  Returns 0, FMPNP_EINVAL, FMPNP_ETOOBIG or FMPNP_ENOMEM. */
int fmpnp_exhaustive_match_layers_cpu(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L,
                                      int B, int item, int H, int W, int flags, int top_k, double ratio, int *argmax,
                                      float *top, float *kth, unsigned char *mask, float *scores, int n_threads);

/* One query of fmpnp_localize_layers: its layers (HOST descriptors, DEVICE data), item and output size; flags:
 * FMPNP_HC_NORMALIZE or 0. */
typedef struct {
    const fmpnp_hc_layer *layers;
    int L, B, item, H, W, flags;
} fmpnp_loc_query_layers;

/* fmpnp_localize with query_dense[q] replaced by each query's layers: the match of query q is one
 * fmpnp_exhaustive_match_layers_async over all its pairs' rows (so its norm plane is formed once), fp32 only;
 * H * W must equal the pairs' dim[0] * dim[1] and sum C_l must equal C.  Everything else is fmpnp_localize's; the
 * results equal the staged composition through fmpnp_exhaustive_match_layers_async bit for bit. */
int fmpnp_localize_layers(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                          const fmpnp_loc_query *queries, const fmpnp_loc_query_layers *query_layers, const int *top_k,
                          int n_queries, int C, double ratio, const fmpnp_loc_params *params, long long total_rows,
                          const fmpnp_loc_best *best, const fmpnp_loc_matches *all, fmpnp_pnp_result *results,
                          unsigned char *pnp_mask, void *hip_stream);

/* ---- retrieval: NetVLAD pooling and the top-n reference ranking --------------------------------------
 * NetVLAD.forward (s2dhm/network/netvlad.py:45-70) over a batch of encoder outputs, and compute_ranks'
 * scores and argsort (s2dhm/image_retrieval/rank_images.py:81-84) cut to the first n ranks.  The PCA between
 * them (image_retrieval/pca.py) is torch plumbing in fmpnp/retrieval.py.
 *
 * Numeric contract of the pooling (fmpnp_netvlad_pool* and the CPU twin implement it with the same code,
 * csrc/fmpnp_retrieval_impl.h; every product is an fp32 fmaf chain, which is what v_mfma_f32_32x32x2_f32
 * computes; nothing is contracted, nothing is atomic), in the order of netvlad.py:45-70:
 *   Inputs.  x is fp32 [B][C][P], element (b, c, p) at x[b * x_stride_b + c * x_stride_c + p] (strides in
 *       elements, x_stride_c >= P, x_stride_b >= 0): an NCHW encoder output with P = h * w, or batch slices
 *       of one.  weight is [K][ld_w >= C] (conv.weight), centroids [K][ld_c >= C], out [B][ld_out >= K * C]
 *       with element (b, k, c) at out[b * ld_out + k * C + c].  Any K, C, P >= 1 up to 2^24 (P up to
 *       2^24 - 256) with K * C < 2^31 - 1024.
 *   x^ (normalize_input = 1).  Per position the sum of squares over c in four interleaved chains: chain q
 *       takes c = q, q + 4, ... ascending, s_q = fmaf(x, x, s_q) from +0; ss = (s_0 + s_1) + (s_2 + s_3);
 *       d = max(sqrtf(ss), 1e-12f) (F.normalize's floor: an all-zero position gives x^ = 0, not NaN);
 *       x^ = x / d, one correctly rounded division.  With normalize_input = 0, x^ = x.
 *   Logits.  s[k][p] = the chain acc = fmaf(weight[k][c], x^[c][p], acc) over c ascending from +0: the chain
 *       fmpnp_correlation_async defines.
 *   Softmax over k.  m = the maximum of s[.][p] (NaN ignored unless all are NaN); e[k] = exp(s[k][p] - m) by
 *       the library's own routine (csrc/fmpnp_retrieval_impl.h exp_neg: fmaf and integer exponent assembly,
 *       the same bits on both sides; no libm or device-library exp; at most FMPNP_NETVLAD_EXP_MAX_ULP ulp
 *       from the exact exponential over [-104, 0], +0 below -104.5); sum = the chain sum + e[k] over k
 *       ascending from +0; a[k][p] = e[k] / sum.  The logits reach +-alpha (hundreds): subtracting m keeps
 *       every argument <= 0.
 *   Aggregation, the only step where a launch could change a result and does not.  The positions are cut
 *       into segments [FMPNP_NETVLAD_SEGMENT * j, FMPNP_NETVLAD_SEGMENT * (j + 1)) (the last one ragged; the
 *       length is part of the contract).  A segment's partial is V_j[k][c] = the chain
 *       acc = fmaf(a[k][p], x^[c][p], acc) over the segment's p ascending from +0, and its assignment sum
 *       S_j[k] = the chain acc = acc + a[k][p] in the same order.  V[k][c] and S[k] add the partials in
 *       ascending j from +0.
 *   Centroid term.  v[k][c] = fmaf(-S[k], centroids[k][c], V[k][c]).
 *   Intra-normalisation.  Per k the sum of squares over c in 64 interleaved chains (chain i takes c = i,
 *       i + 64, ... ascending, fmaf(v, v, s_i) from +0) combined by t[i] = t[i] + t[i + o] for o = 32, 16,
 *       ..., 1; n = max(sqrtf(t[0]), 1e-12f); u[k][c] = v[k][c] / n.
 *   Final normalisation.  T[k] = the same 64-chain sum of squares of u[k][.]; total = the chain
 *       total + T[k] over k ascending from +0; out = u / max(sqrtf(total), 1e-12f).
 *   The output bits depend on the inputs of that image only: not on B, on the image's place in the batch,
 *   on the grid, the stream, the workspace's content or the twin's thread count.  NaN and Inf inputs propagate
 *   by the same arithmetic. */
#define FMPNP_NETVLAD_SEGMENT 256       /* positions per aggregation segment */
/* measured over every float of [-104, 0] by `build/test_retrieval_cpu exp 1`: 1.0103 ulp, at x = -5.87788439 */
#define FMPNP_NETVLAD_EXP_MAX_ULP 1.011f

/* Bytes of device workspace fmpnp_netvlad_pool_async needs (assignments, denominators, segment partials of a
 * round of images; bounded however large B is).  0 for arguments the pooling would refuse. */
size_t fmpnp_netvlad_workspace_size(int B, int K, int C, int P);

/* Asynchronous: every pointer is DEVICE memory; four kernels per round of images on hip_stream; nothing is
 * synchronised, nothing allocated.  workspace: 4-byte aligned (FMPNP_EALIGN otherwise), at least
 * fmpnp_netvlad_workspace_size(B, K, C, P) bytes; its content before the call does not matter.
 * FMPNP_EINVAL: B < 0, K, C or P < 1, a stride or leading dimension below its row, normalize_input not 0 or 1,
 * a null pointer (B > 0), a short workspace.  FMPNP_ETOOBIG: a size beyond the limits above.  B = 0 is a no-op. */
int fmpnp_netvlad_pool_async(const float *x, int B, int C, int P, long long x_stride_b, long long x_stride_c,
                             const float *weight, int K, int ld_w, const float *centroids, int ld_c,
                             int normalize_input, float *out, long long ld_out, void *workspace,
                             size_t workspace_bytes, void *hip_stream);

/* Synchronous: the same with the library's own workspace (kept per device and stream, like the other synchronous
 * entry points' scratch), then waits for hip_stream.  Also FMPNP_ENOMEM, FMPNP_ENODEV. */
int fmpnp_netvlad_pool(const float *x, int B, int C, int P, long long x_stride_b, long long x_stride_c,
                       const float *weight, int K, int ld_w, const float *centroids, int ld_c, int normalize_input,
                       float *out, long long ld_out, void *hip_stream);

/* CPU twin with HOST pointers: the same contract from the same code, so every output element equals the GPU's
 * bit for bit.  n_threads host threads (0: every core) over the images; the result does not depend on it.  An
 * explicit CPU entry point, never a fallback.  Returns 0, FMPNP_EINVAL, FMPNP_ETOOBIG or FMPNP_ENOMEM. */
int fmpnp_netvlad_pool_cpu(const float *x, int B, int C, int P, long long x_stride_b, long long x_stride_c,
                           const float *weight, int K, int ld_w, const float *centroids, int ld_c,
                           int normalize_input, float *out, long long ld_out, int n_threads);

/* Top-n ranking: scores[q][r] = sum_d qry[q][d] * ref_t[d][r], the fmaf chain of fmpnp_correlation_async (its
 * kernel: qry is the `sparse` operand [Q][ld_q >= D], ref_t the `dense` one, the references transposed,
 * [D][ld_r >= R]); idx[q][i], i < n, is the reference of rank i of query q and top[q][i] its score, in
 * descending score order.  rank_images.py's ranks[:n, q] is idx[q][:n].
 *   Order.  Equal scores rank the lower reference index first; -0 counts as +0; NaN ranks LAST, where
 *       np.argsort(-scores) puts it -- the opposite of fmpnp_exhaustive_match's select, whose key (torch.topk's
 *       convention) puts NaN first.  The order is total, so idx is a function of the scores alone.
 *   Limits.  1 <= n <= R (FMPNP_EINVAL otherwise) and n <= FMPNP_RANK_TOPN_CAP (FMPNP_ETOOBIG beyond it: the
 *       n best are sorted in LDS); Q, D, R <= 2^24 (FMPNP_ETOOBIG).  Q = 0 is a no-op.
 *   scores: NULL, or [Q][R] DEVICE memory that receives the whole map.  With NULL the map goes through
 *       `workspace`, at least fmpnp_match_workspace_size(Q, R) bytes (rounds of rows, as the match's). */
#define FMPNP_RANK_TOPN_CAP 1024

/* Asynchronous: DEVICE pointers, the correlation and one selection kernel per round on hip_stream. */
int fmpnp_rank_topn_async(const float *qry, int Q, int ld_q, const float *ref_t, int D, int R, int ld_r, int n,
                          int *idx, float *top, float *scores, void *workspace, size_t workspace_bytes,
                          void *hip_stream);

/* Synchronous: DEVICE pointers, the library's own workspace (per device and stream), then waits for hip_stream. */
int fmpnp_rank_topn(const float *qry, int Q, int ld_q, const float *ref_t, int D, int R, int ld_r, int n, int *idx,
                    float *top, float *scores, void *hip_stream);

/* CPU twin with HOST pointers: the GPU's scores, idx and top bit for bit; n_threads host threads (0: every core)
 * over the queries.  scores: NULL or [Q][R].  Returns 0, FMPNP_EINVAL, FMPNP_ETOOBIG or FMPNP_ENOMEM. */
int fmpnp_rank_topn_cpu(const float *qry, int Q, int ld_q, const float *ref_t, int D, int R, int ld_r, int n,
                        int *idx, float *top, float *scores, int n_threads);

/* ---- SuperPoint baseline: detector head, NMS, descriptor sampling, 2-NN matching, assembly ------------
 * The part of the reference's SuperPointPredictor (s2dhm/pose_prediction/superpoint_predictor.py) between the
 * network's two output tensors and the 2D-3D matches fmpnp_pnp_ransac takes: SuperPointFrontend.run and
 * nms_fast (third_party/SuperPointPretrainedNetwork/demo_superpoint.py:151-284), fast_keypoint_matching and
 * fast_closest_points (keypoint_association.py:77-108) and _assemble_matches (superpoint_predictor.py:45-65).
 * The convolutions stay the caller's here; "the 1x1 convolution" below, with the encoder's operators, is what
 * fmpnp/superpoint.py's HipSuperPointNet runs the network itself through (opt-in).  Five stages; each has an asynchronous form (every pointer DEVICE
 * memory, on hip_stream), a synchronous form (the same DEVICE inputs, HOST outputs, the library's own scratch
 * per device and stream, waits for hip_stream) and a CPU twin (HOST pointers) built from the same code
 * (csrc/fmpnp_superpoint_impl.h, no contraction on either side), so the three agree bit for bit.  The twins
 * are explicit entry points, never a fallback.
 *
 * 1. Detector head.  semi [65][Hc][Wc] fp32 -> heat [8 Hc][8 Wc] fp32.  Per cell: e_c = exp(semi_c) by the
 *    library's own routine (the retrieval stage's exp_neg up to 0, the same reduction and polynomial above 0,
 *    +Inf from 89 up); s = ((e_0 + e_1) + ...) + e_64; heat[8 yc + c / 8][8 xc + c % 8] = e_c / (s + 1e-5f),
 *    c < 64.  No maximum is subtracted (the reference subtracts none).  So a logit of 89 or more makes s +Inf:
 *    that channel's heat is NaN (Inf / Inf) and every other heat of the cell +0; a NaN logit makes the cell's 64
 *    values NaN.  Where a stage's result is a NaN, the three forms agree that it is one, not on its sign bit.
 * 2. NMS.  The candidates are the pixels with heat >= (float)conf_thresh (a NaN is none).  The greedy walk of
 *    nms_fast: candidates in descending heat (-0 as +0), equal heats by ascending row-major pixel index; a
 *    candidate is kept iff no earlier kept one lies within Chebyshev distance nms_dist.  Then the kept points
 *    with x < border, x >= W - border, y < border or y >= H - border are dropped (they have suppressed their
 *    neighbours).  pts [3][ld_pts] fp64: rows x, y, heat, the first n columns in that descending order;
 *    ld_pts >= fmpnp_sp_nms_capacity(H, W, nms_dist), the most points the walk can keep.  Columns from n on are
 *    not written.  The GPU reaches the greedy result in rounds of two launches (a live candidate with a kept
 *    point in its window is suppressed; then a live candidate whose order beats every live or newly kept
 *    candidate of its window is kept) and reads the live count back after every `group` rounds: the result
 *    does not depend on group.  nms_dist <= FMPNP_SP_MAX_NMS_DIST, H, W <= 16384 (FMPNP_ETOOBIG).
 * 3. Descriptors.  coarse [D][Hc][Wc] fp32; per point g_x = (float)(x / (W / 2.) - 1.) (fp64 inside), g_y
 *    likewise with H; grid_sample's un-normalisation in fp32 (align_corners 0: ((g + 1) size - 1) / 2; 1:
 *    ((g + 1) / 2)(size - 1)), bilinear weights as torch forms them, the in-bounds taps' products added in
 *    the order nw, ne, sw, se from +0 (zero padding).  The sum of squares over the channels in 64 interleaved
 *    chains (chain i: c = i, i + 64, ... by fmaf from +0) combined by t[i] = t[i] + t[i ^ o], o = 32 .. 1;
 *    desc[c][p] = v / sqrtf(t[0]).  desc [D][ld_desc >= N], k-major: fmpnp_correlation_async's `dense` operand.
 * 4. Two nearest neighbours.  s[i][j] = the fmaf chain of fmpnp_correlation_async over desc1 [N1][ld1 >= D]
 *    and desc2_t [D][ld2 >= N2]; dist = 2 (1 - s), two fp32 roundings.  Per row nn_idx[i][0..1] / nn_dist the
 *    two smallest distances: equal distances take the lower index, -0 counts as +0, NaN sorts after every
 *    number; ok[i] = nn_dist[i][0] <= (float)(ratio^2) * nn_dist[i][1].  matches [n][2] int64 = (i, nn_idx[i][0])
 *    of the ok rows in ascending i, *count = n.  N2 < 2 is FMPNP_EINVAL (topk(2) raises); N1 = 0 gives n = 0.
 *    The score map passes through a bounded workspace in rounds of rows; no bit depends on the rounds.
 * 5. Association and assembly.  argmin[i], i < N2 = the landmark m < M with the smallest
 *    (px - rx)(px - rx) + (py - ry)(py - ry) in fp64, no contraction, the lowest m among equal minima (a NaN
 *    distance never wins; if every distance is NaN, 0).  For every reference keypoint i that occurs in
 *    matches[:][1], in ascending i, with q = the lowest matches[:][0] naming it: x2d [n][2] = query keypoint
 *    q's (x, y), x2d_ref [n][2] = keypoint i's, x3d [n][3] = points3d[argmin[i]]; *count = n.  Keypoints are
 *    [>= 2][ld] fp64 arrays as stage 2 writes them; a match outside [0, N1) x [0, N2) is ignored.
 * Outputs past each count keep what they held. */
#define FMPNP_SP_CELL 8
#define FMPNP_SP_BORDER 4           /* SuperPointFrontend.border_remove */
#define FMPNP_SP_MAX_NMS_DIST 16
#define FMPNP_SP_MAX_KEYPOINTS 65536 /* kept interior points beyond this: FMPNP_ETOOBIG (the rank sort is quadratic) */

int fmpnp_sp_heatmap_async(const float *semi, int Hc, int Wc, float *heat, void *hip_stream);
int fmpnp_sp_heatmap(const float *semi, int Hc, int Wc, float *heat_host, void *hip_stream);
int fmpnp_sp_heatmap_cpu(const float *semi, int Hc, int Wc, float *heat);

long long fmpnp_sp_nms_capacity(int H, int W, int nms_dist);
size_t fmpnp_sp_nms_workspace_size(int H, int W, int nms_dist);
/* n_host / rounds_host: HOST ints that receive the count and the rounds the walk took (rounds_host may be
 * NULL): every round up to the first that leaves no live candidate, which may be one that only suppresses (a row
 * of 200 equal pixels at nms_dist 1 keeps 100 points in 101 rounds); 0 without a candidate.
 * count_dev: NULL or a DEVICE int that receives the count too.  group >= 1: rounds per host read.
 * workspace: 8-byte aligned, fmpnp_sp_nms_workspace_size bytes.  Waits for hip_stream between groups. */
int fmpnp_sp_nms_async(const float *heat, int H, int W, double conf_thresh, int nms_dist, int border, double *pts,
                       long long ld_pts, int *count_dev, int group, int *n_host, int *rounds_host, void *workspace,
                       size_t workspace_bytes, void *hip_stream);
int fmpnp_sp_nms(const float *heat, int H, int W, double conf_thresh, int nms_dist, int border, double *pts_host,
                 long long ld_pts, int group, int *n_host, int *rounds_host, void *hip_stream);
int fmpnp_sp_nms_cpu(const float *heat, int H, int W, double conf_thresh, int nms_dist, int border, double *pts,
                     long long ld_pts, int *n);

int fmpnp_sp_describe_async(const float *coarse, int D, int Hc, int Wc, const double *pts, long long ld_pts, int N,
                            int H, int W, int align_corners, float *desc, long long ld_desc, void *hip_stream);
int fmpnp_sp_describe(const float *coarse, int D, int Hc, int Wc, const double *pts, long long ld_pts, int N, int H,
                      int W, int align_corners, float *desc_host, long long ld_desc, void *hip_stream);
int fmpnp_sp_describe_cpu(const float *coarse, int D, int Hc, int Wc, const double *pts, long long ld_pts, int N,
                          int H, int W, int align_corners, float *desc, long long ld_desc);

/* nn_idx int [N1][2], nn_dist float [N1][2], ok bytes [N1], matches int64 [N1][2], count one int.  workspace: at
 * least fmpnp_match_workspace_size(N1, N2) bytes (the score rows of one round). */
int fmpnp_sp_match_async(const float *desc1, int N1, int ld1, const float *desc2_t, int D, int N2, int ld2,
                         double ratio, int *nn_idx, float *nn_dist, unsigned char *ok, long long *matches, int *count,
                         void *workspace, size_t workspace_bytes, void *hip_stream);
int fmpnp_sp_match(const float *desc1, int N1, int ld1, const float *desc2_t, int D, int N2, int ld2, double ratio,
                   int *nn_idx_host, float *nn_dist_host, unsigned char *ok_host, long long *matches_host,
                   int *count_host, void *hip_stream);
int fmpnp_sp_match_cpu(const float *desc1, int N1, int ld1, const float *desc2_t, int D, int N2, int ld2, double ratio,
                       int *nn_idx, float *nn_dist, unsigned char *ok, long long *matches, int *count);

/* points2d [M][2], points3d [M][3] fp64; matches [n_matches][2] int64; argmin int [N2]; x2d, x2d_ref [N2][2],
 * x3d [N2][3] fp64; count one int.  workspace: 4-byte aligned, 4 * N2 bytes. */
int fmpnp_sp_assemble_async(const double *query_pts, int N1, long long ld_q, const double *ref_pts, int N2,
                            long long ld_r, const double *points2d, const double *points3d, int M,
                            const long long *matches, int n_matches, int *argmin, double *x2d, double *x2d_ref,
                            double *x3d, int *count, void *workspace, size_t workspace_bytes, void *hip_stream);
int fmpnp_sp_assemble(const double *query_pts, int N1, long long ld_q, const double *ref_pts, int N2, long long ld_r,
                      const double *points2d, const double *points3d, int M, const long long *matches, int n_matches,
                      int *argmin_host, double *x2d_host, double *x2d_ref_host, double *x3d_host, int *count_host,
                      void *hip_stream);
int fmpnp_sp_assemble_cpu(const double *query_pts, int N1, long long ld_q, const double *ref_pts, int N2,
                          long long ld_r, const double *points2d, const double *points3d, int M,
                          const long long *matches, int n_matches, int *argmin, double *x2d, double *x2d_ref,
                          double *x3d, int *count);

/* (fmpnp_level, one channel level of the pyramid, is defined with the localisation chain above.)
 *
 * One query of feature_pnp (s2dhm/pose_prediction/optimize_feature_pnp.py:50-71) in one call,
 * with one host wait: pack the query map (opt->layout; opt->sobel_flags are the Sobel's flags),
 * gather the reference descriptors of the N reference inliers (x, y) with the adapter's
 * truncation, then
 *   n_levels == 0: forward over channels [0, C)                     (model.py:245-494)
 *                  -> results[0];
 *   n_levels >  0: multilevel_optimization over the channel levels  (model.py:178-213):
 *                  compute_cost at (R0, t0) over [0, C) -> results[0] (status NO_SUPPORT: the
 *                  reference returns (R0, t0) without refining -- the caller applies that), then
 *                  forward per level, each from the previous level's result pose -> results[1 + l].
 * query_chw [C][H][W] and ref_chw [C_ref][H_ref][W_ref] (C_ref == C) are DEVICE maps; ref_inliers
 * [N][2], pts3d [N][3], K, R0, t0 (row-major) and results / trace ([max(n_levels, 1)][trace_stride]
 * entries, or NULL) are HOST memory.  opt->mode must be FMPNP_MODE_FORWARD; opt->dtype is the
 * packed storage.  Returns 0, FMPNP_ERANGE when an inlier maps outside the reference map (results
 * are still written), another FMPNP_E* code or a hipError_t.  The library keeps, per (device,
 * hip_stream), the device buffers, a pinned staging buffer and a second stream with two events
 * between calls (see Threads above): with levels, the first level's channels are packed first and the
 * other channels' pack and compute_cost run on that second stream under the first level's launch. */
int fmpnp_feature_pnp(const void *query_chw, int dtype_query, int C, int H, int W, const void *ref_chw,
                      int dtype_ref, int C_ref, int H_ref, int W_ref, const double *ref_inliers,
                      const double *pts3d, int N, const double K[9], const double R0[9], const double t0[3],
                      int img0, int img1, const fmpnp_level *levels, int n_levels, const fmpnp_options *opt,
                      int window_radius, fmpnp_result *results, fmpnp_trace_entry *trace, int trace_stride,
                      void *hip_stream);
/* window_radius > 0 (FMPNP_LAYOUT_FGRAD, nearest sampling): pack only the texels within that many texels
 * (Chebyshev) of a point's texel at (R0, t0) -- the refinement reads the texels its points visit, a
 * few from where they start.  An LM gather outside the window marks the attempt invalid and the call
 * runs again fully packed, so the results are the full pack's bit for bit either way.  0: full pack.
 * fmpnp_feature_pnp_reruns(): how many calls of this process ran again after a window miss. */
long long fmpnp_feature_pnp_reruns(void);

/* fmpnp_feature_pnp with the reference given as the encoder's layers instead of its dense hypercolumn: the
 * reference descriptors are formed by the sparse hypercolumn kernel (FMPNP_HC_AT_REFERENCE with img0, img1, the
 * storage dtype, straight into the call's reference rows, the same error flag), so the H_ref x W_ref map is
 * never assembled.  ref_layers: HOST descriptors (n_ref_layers of them, batch item 0) of DEVICE fp32 layers whose
 * channels add up to C (FMPNP_EINVAL otherwise); ref_flags: FMPNP_HC_NORMALIZE or 0.  Everything else, the one
 * upload, one download and one wait and the window re-run included, is fmpnp_feature_pnp's: the results are
 * those of fmpnp_feature_pnp on fmpnp_hypercolumn_assemble's map of the same layers, bit for bit. */
int fmpnp_feature_pnp_layers(const void *query_chw, int dtype_query, int C, int H, int W,
                             const fmpnp_hc_layer *ref_layers, int n_ref_layers, int H_ref, int W_ref, int ref_flags,
                             const double *ref_inliers, const double *pts3d, int N, const double K[9],
                             const double R0[9], const double t0[3], int img0, int img1, const fmpnp_level *levels,
                             int n_levels, const fmpnp_options *opt, int window_radius, fmpnp_result *results,
                             fmpnp_trace_entry *trace, int trace_stride, void *hip_stream);

/* fmpnp_feature_pnp with the QUERY given as the encoder's layers: the packed map is formed by the fused
 * hypercolumn pack (fmpnp_hypercolumn_pack above: the norm plane once per attempt, before the first pack, then
 * the channel ranges, with the window's marks when window_radius > 0), so the dense [C][H][W] query map is never
 * assembled.  query_layers: HOST descriptors (n_query_layers of them, batch item 0) of DEVICE fp32 layers; C is
 * the sum of their channels, H x W the hypercolumn's size, query_flags FMPNP_HC_NORMALIZE or 0.  The reference is
 * given either as a dense map (ref_chw, dtype_ref; ref_layers NULL) or as layers (ref_chw NULL; ref_layers,
 * n_ref_layers, ref_flags as fmpnp_feature_pnp_layers); exactly one of the two, FMPNP_EINVAL otherwise.
 * Everything else -- the one upload, one download and one wait, the first level's channels packed first and the
 * rest on the second stream, the windowed attempt and its fully packed re-run -- is fmpnp_feature_pnp's: the
 * results are those of fmpnp_feature_pnp on fmpnp_hypercolumn_assemble's map of the same layers, bit for bit. */
int fmpnp_feature_pnp_query_layers(const fmpnp_hc_layer *query_layers, int n_query_layers, int H, int W,
                                   int query_flags, const void *ref_chw, int dtype_ref,
                                   const fmpnp_hc_layer *ref_layers, int n_ref_layers, int H_ref, int W_ref,
                                   int ref_flags, const double *ref_inliers, const double *pts3d, int N,
                                   const double K[9], const double R0[9], const double t0[3], int img0, int img1,
                                   const fmpnp_level *levels, int n_levels, const fmpnp_options *opt,
                                   int window_radius, fmpnp_result *results, fmpnp_trace_entry *trace,
                                   int trace_stride, void *hip_stream);

/* Debug: when device_buf != NULL, later LM launches write per-workgroup phase cycle
 * totals (s_memtime) to device_buf[grid][8 waves][12] (8 phases, then the first evaluation's
 * projection, gather, loss and contribution phases separately; phases 3-7 are wave 0's LM tail);
 * NULL switches it off. */
int fmpnp_debug_stamps(unsigned long long *device_buf);

/* Last launch geometry of this thread (for benches / tests). */
int fmpnp_last_launch(int *teams, int *wgs_per_problem, int *grid, int *lds_bytes);

/* LM kernel builds (fmpnp_launch_info.build) */
#define FMPNP_BUILD_WIDE 1        /* 256-thread workgroups, one wave per SIMD (bilinear cell memo) */
#define FMPNP_BUILD_LATENCY 2     /* 512-thread workgroups, one per CU */
#define FMPNP_BUILD_THROUGHPUT 4  /* 256-thread workgroups, two per CU (batches >= 2 per CU) */

/* LM kernel variants (fmpnp_launch_info.variant): which code paths are compiled into the
 * kernel that ran -- the loss / sampling / layout specialisation, the speculative next-texel
 * gathers (_SPEC) and the first-evaluation helpers' hand-off (_H) */
#define FMPNP_VAR_NEAREST 0        /* any loss, nearest sampling, packed f/gx/gy (and compute_cost) */
#define FMPNP_VAR_GM 1             /* Geman-McClure forward, nearest, packed */
#define FMPNP_VAR_BILINEAR 2       /* bilinear cell memo */
#define FMPNP_VAR_F_NEAREST 3      /* FMPNP_LAYOUT_F, any loss */
#define FMPNP_VAR_F_GM 4           /* FMPNP_LAYOUT_F, Geman-McClure */
#define FMPNP_VAR_BIL_DIRECT 5     /* bilinear, every point sampled every evaluation */
#define FMPNP_VAR_GM_SPEC 6
#define FMPNP_VAR_NEAREST_SPEC 7
#define FMPNP_VAR_GM_SPEC_H 8
#define FMPNP_VAR_NEAREST_SPEC_H 9
#define FMPNP_VAR_GM_H 10
#define FMPNP_VAR_NEAREST_H 11
#define FMPNP_VAR_GM_SPEC_512 12    /* GM_SPEC / GM_SPEC_H compiled for a 512-point workgroup (the LDS carve at */
#define FMPNP_VAR_GM_SPEC_H_512 13  /* compile-time offsets: configs[1]/[2]'s N = 512, fp32); otherwise as those */
#define FMPNP_VAR_GM_W 14          /* GM / NEAREST / GM_H / NEAREST_H with the packed-window check compiled */
#define FMPNP_VAR_NEAREST_W 15     /* in (fmpnp_problem.window on the packed f/gx/gy planes: fmpnp_feature_pnp's */
#define FMPNP_VAR_GM_H_W 16        /* windowed packs); the other packed variants carry no check */
#define FMPNP_VAR_NEAREST_H_W 17

typedef struct {
    int teams, wgs_per_problem, grid, lds_bytes;
    int build;              /* FMPNP_BUILD_* */
    int variant;            /* FMPNP_VAR_* */
    int team;               /* 1: wgs_per_problem > 1 (cross-workgroup exchange compiled in) */
    int ratio;              /* 1: the ratio-test specialisation */
    int dtype;              /* fmpnp_dtype of the texels */
    int helpers;            /* first-evaluation helper workgroups per problem */
    int speculate;          /* speculative next-texel gathers enabled */
} fmpnp_launch_info;

/* The LM launch plan for these problems and options, without launching anything (needs
 * the current device: CU count and occupancy).  Returns 0 or the launch's error code. */
int fmpnp_plan(const fmpnp_problem *probs_host, int n, const fmpnp_options *opt, fmpnp_launch_info *out);

/* Plan of the last LM launch of this thread. */
int fmpnp_last_launch_info(fmpnp_launch_info *out);

/* ---- the encoder's operators (opt-in): 3x3 convolution, ReLU, 2x2 max-pool ------------------------------
 * VGG-16's features[:-2] (s2dhm/network/network.py:47-51) is made of these three and nothing else.  All values
 * fp32, every tensor contiguous [B][C][H][W].
 *
 *   Convolution.  in [B][Cin][H][W], weight [Cout][Cin][3][3], bias [Cout], out [B][Cout][H][W]; stride 1, zero
 *       padding 1; a cross-correlation, as torch.nn.Conv2d computes:
 *           out[b][co][y][x] = sum_k a_k * w[co][k],   k = ci * 9 + ky * 3 + kx  (the weight's own flat order),
 *           a_k = in[b][ci][y + ky - 1][x + kx - 1], or 0 for a tap outside the image.
 *       Each output is ONE fp32 accumulator's fmaf chain from +0 over k ascending, acc = fmaf(a_k, w_k, acc): what
 *       v_mfma_f32_32x32x2_f32 computes, as for fmpnp_correlation_async.  A tap outside the image, and the zero
 *       tail that pads k to the kernel's k tile, contribute fmaf(0, w, acc): for finite w no value changes (an
 *       accumulator of -0 would become +0).  Then one fp32 add of bias[co] (FMPNP_CONV_BIAS), then the ReLU below
 *       (FMPNP_CONV_RELU).  No split-K, no atomics: the bits of an output depend on its 9 * Cin operands, its
 *       weights and its bias only -- not on B, the tile, the grid or the stream.
 *       Weights and biases must be finite (a 0 operand times an infinite weight would be NaN where torch pads; the
 *       caller checks once, fmpnp/encoder.py does when a plan is built).  UNSPECIFIED: non-finite activations, and
 *       products or sums in the subnormal range (whether the matrix instruction keeps or flushes them).
 *   ReLU.  x > 0 ? x : (x != x ? x : +0): a NaN stays, -0 and everything negative become +0.
 *   Max-pool.  2 x 2 windows, stride 2, floor mode: out [B][C][H / 2][W / 2], an odd last row or column is dropped;
 *       H < 2 or W < 2 (an empty output) is FMPNP_EINVAL.  m = the window's (0,0) value, then (0,1), (1,0), (1,1)
 *       in that order with m = (v > m || v != v) ? v : m: a NaN wins, of +0 and -0 the first met stays.
 *   Limits.  B, Cin, Cout, C, H, W >= 1 (FMPNP_EINVAL); every tensor below 2^31 elements (FMPNP_ETOOBIG); sizes
 *       are formed in size_t.  NULL tensors, unknown flag bits, and FMPNP_CONV_BIAS with a NULL bias: FMPNP_EINVAL.
 * The *_async forms take DEVICE pointers and queue on hip_stream, nothing is synchronised or allocated; the plain
 * forms queue the same launch and wait for the stream.  The *_cpu forms are the CPU twins: HOST pointers, the same
 * chains through the same fmaf, so their outputs are the GPU's bit for bit; n_threads host threads (0: every
 * core); explicit entry points, never a fallback (0, FMPNP_EINVAL, FMPNP_ETOOBIG or FMPNP_ENOMEM).  out may equal
 * in for the ReLU only. */
#define FMPNP_CONV_BIAS 1
#define FMPNP_CONV_RELU 2
int fmpnp_conv3x3_async(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                        int flags, float *out, void *hip_stream);
int fmpnp_conv3x3(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                  int flags, float *out, void *hip_stream);
int fmpnp_conv3x3_cpu(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                      int flags, float *out, int n_threads);
/* n elements, n >= 0 (n = 0: nothing is read) */
int fmpnp_relu_async(const float *in, float *out, long long n, void *hip_stream);
int fmpnp_relu_cpu(const float *in, float *out, long long n, int n_threads);
int fmpnp_maxpool2x2_async(const float *in, int B, int C, int H, int W, float *out, void *hip_stream);
int fmpnp_maxpool2x2(const float *in, int B, int C, int H, int W, float *out, void *hip_stream);
int fmpnp_maxpool2x2_cpu(const float *in, int B, int C, int H, int W, float *out, int n_threads);

/* ---- the 1x1 convolution (opt-in): SuperPoint's head convolutions ----------------------------------------
 * convPb (256 -> 65) and convDb (256 -> 256) of the SuperPoint network are 1x1, stride 1, padding 0; with the 3x3
 * convolution, the ReLU and the max-pool above, and fmpnp_hypercolumn_assemble of one layer for the descriptor head's
 * normalisation, that is the whole network.  The conventions are the encoder's operators': all values fp32, every
 * tensor contiguous.
 *
 *   Tensors.  in [B][Cin][H][W], weight [Cout][Cin] (a Conv2d's [Cout][Cin][1][1] as it lies), bias [Cout],
 *       out [B][Cout][H][W].  flags: FMPNP_CONV_BIAS | FMPNP_CONV_RELU, with the 3x3 convolution's meaning.
 *   Values.  With p the flat pixel index y * W + x of a channel plane,
 *           out[b][co][p] = sum_ci in[b][ci][p] * weight[co][ci],
 *       ONE fp32 accumulator's fmaf chain from +0 over ci ascending, acc = fmaf(in[b][ci][p], weight[co][ci], acc):
 *       the chain fmpnp_correlation_async defines, with sparse = weight and dense = in[b], and what
 *       v_mfma_f32_32x32x2_f32 computes.  The zero tail that pads ci to the kernel's k tile contributes
 *       fmaf(0, w, acc).  Then one fp32 add of bias[co] (FMPNP_CONV_BIAS), then the ReLU of the encoder's operators
 *       (FMPNP_CONV_RELU): the 3x3 convolution's epilogue, shared as code.  No split-K, no atomics: the bits of an
 *       output depend on its Cin operands, its weights and its bias only -- not on B, H, W, Cout, the tile, the
 *       grid, the width of the kernel's loads or the stream.  Pixels have no row geometry: only H * W matters.
 *       Weights and biases must be finite.  UNSPECIFIED, as for the 3x3 convolution: non-finite activations, and
 *       products or sums in the subnormal range.
 *   Limits.  B, Cin, Cout, H, W >= 1 (FMPNP_EINVAL); every tensor below 2^31 elements (FMPNP_ETOOBIG); NULL
 *       tensors, unknown flag bits, and FMPNP_CONV_BIAS with a NULL bias: FMPNP_EINVAL.  The host validates before
 *       anything touches the device.  out must not overlap in.
 * fmpnp_conv1x1_async takes DEVICE pointers and queues one launch for any B on hip_stream, nothing is synchronised
 * or allocated; fmpnp_conv1x1 queues the same launch and waits for the stream.  fmpnp_conv1x1_cpu is the CPU twin:
 * HOST pointers, the same chains through the same fmaf, the GPU's output bit for bit; n_threads host threads (0:
 * every core), the result does not depend on it; an explicit entry point, never a fallback (0, FMPNP_EINVAL,
 * FMPNP_ETOOBIG or FMPNP_ENOMEM). */
int fmpnp_conv1x1_async(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                        int flags, float *out, void *hip_stream);
int fmpnp_conv1x1(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                  int flags, float *out, void *hip_stream);
int fmpnp_conv1x1_cpu(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                      int flags, float *out, int n_threads);

/* ---- the encoder's fp16 precision (opt-in): the 3x3 convolution on the fp16 matrix cores ------------------
 * The exact-fp32 contract above stays the default of every entry point and of every caller that does not ask
 * otherwise.  The *_f16 forms trade it for the fp16 matrix rate (16 x the fp32 MFMA's), after the pattern of the
 * match stage's fp16 precision above.  Tensors, flags, padding and the limits are fmpnp_conv3x3's; activations stay
 * fp32 in memory, and the ReLU, the pool and everything downstream are unchanged.
 *
 *   Operands.  Every input value and every weight is used as fl16(x): IEEE binary16, round-to-nearest-even (the
 *       fl16 of the match stage; a round-toward-zero pack conversion is NOT this contract).  The input is rounded
 *       while it is staged, bit for bit what a separate conversion would give; the weights are rounded once, into
 *       the packed image below.  |x| >= 65520 becomes +-Inf by the conversion and the results are then
 *       UNSPECIFIED, as the exact contract leaves non-finite activations; so are operands with |fl16(x)| < 2^-14
 *       (fp16 subnormals: whether the matrix instruction keeps them or takes them as zero).  Nothing checks the
 *       activations; weights must be finite and below 65520 in magnitude (the caller checks once, fmpnp/encoder.py
 *       does when a plan is built).
 *   Sum.  With CB = ceil(Cin / 16):
 *           s[b][co][y][x] = sum over steps st = cb * 9 + (ky * 3 + kx), ascending, cb = 0 .. CB - 1, of the 16
 *           products fl16(a) * fl16(w) of the input channels 16 cb .. 16 cb + 15 at the tap (ky, kx),
 *       a = in[b][ci][y + ky - 1][x + kx - 1], or 0 for a tap outside the image or a channel >= Cin.  The products are
 *       exact (11 + 11 significand bits fit fp32).  A step is one v_mfma_f32_32x32x16_f16: the steps go in this
 *       order into ONE fp32 accumulator per output that starts at +0.  No split-K, no atomics.
 *   After the sum.  One fp32 add of bias[co] (FMPNP_CONV_BIAS), then the ReLU of the exact contract
 *       (FMPNP_CONV_RELU): the exact entry points' epilogue.
 *   Launch independence.  The bits of an output depend only on its operands, Cin and the flags: not on B, Cout,
 *       the tile, the grid or the stream.
 *   No bit-identical CPU twin.  The order (and any intermediate rounding) of the 16 products inside one MFMA is
 *       not documented, so fmpnp_conv3x3_f16_cpu is a REFERENCE: the same fl16 operands, the products accumulated
 *       in fp64 in the order above (the channels of a step ascending), ONE rounding to fp32, then the fp32 bias add
 *       and the ReLU.  With K_p = 16 * 9 * CB the GPU's output lies within
 *           K_p * 2^-23 * sum |fl16(a)| |fl16(w)|  +  2^-24 |s|  +  2^-24 |s + b|
 *       of it (per step twice the any-order fp32 summation bound, as for the match stage; the reference's rounding
 *       of s; the two bias adds' roundings; the ReLU is 1-Lipschitz and changes nothing).  On operands that are
 *       exact in fp16 and whose partial sums are exact in fp32 (small integers) every order gives the same bits:
 *       the exact kernel's.
 *   Packed weights.  The GPU forms take the weights as an fp16 image [Cout_p][CB][9][16], Cout_p = Cout rounded up
 *       to a multiple of 32:  image[co][cb][t][c] = fl16(weight[co][16 cb + c][t / 3][t % 3]), zero for
 *       16 cb + c >= Cin and for co >= Cout.  fmpnp_conv3x3_f16_weights_size(Cin, Cout) is its size in bytes (0 for
 *       an invalid or too large shape); it must be 16-byte aligned.  fmpnp_conv3x3_pack_weights_f16_async builds it
 *       on the device from the fp32 weights, fmpnp_conv3x3_pack_weights_f16_cpu on the host: the two are
 *       bit-identical (they only convert and move; finite weights).  An image serves every B, H and W.
 *   Limits and errors.  fmpnp_conv3x3's (FMPNP_EINVAL, FMPNP_ETOOBIG from 2^31 elements; the packed image too stays
 *       below 2^31 elements); a packed image that is NULL or not 16-byte aligned: FMPNP_EINVAL. */
size_t fmpnp_conv3x3_f16_weights_size(int Cin, int Cout);
int fmpnp_conv3x3_pack_weights_f16_async(const float *weight, int Cin, int Cout, void *packed, void *hip_stream);
int fmpnp_conv3x3_pack_weights_f16_cpu(const float *weight, int Cin, int Cout, void *packed);
int fmpnp_conv3x3_f16_async(const float *in, int B, int Cin, int H, int W, const void *packed, const float *bias, int Cout,
                            int flags, float *out, void *hip_stream);
int fmpnp_conv3x3_f16(const float *in, int B, int Cin, int H, int W, const void *packed, const float *bias, int Cout,
                      int flags, float *out, void *hip_stream);
/* the reference: HOST pointers, the fp32 weights [Cout][Cin][3][3] (it rounds them itself) */
int fmpnp_conv3x3_f16_cpu(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                          int flags, float *out, int n_threads);

/* ---- dense features (opt-in): dilated 3x3 convolution, 2x2 / stride 1 average pool, the scale pyramid's step ----
 * What a D2-Net style trunk needs beside the encoder's operators -- VGG-16 to conv4_3 with pool3 an
 * AvgPool2d(2, stride 1) and the conv4 layers dilated by 2 with padding 2 -- and the pyramid over image scales of
 * s2dhm/d2net_utils/dense_pyramid.py:5-42.  The conventions are the encoder's operators': all values fp32, every
 * tensor contiguous [B][C][H][W], the *_async forms take DEVICE pointers and queue one launch on hip_stream (nothing
 * is synchronised or allocated), the plain forms queue the same launch and wait for the stream, the *_cpu forms are
 * the CPU twins (HOST pointers, the GPU's output bit for bit for any n_threads; 0: every core; explicit entry points,
 * never a fallback).  The host validates before anything touches the device.
 *
 *   Dilated convolution.  fmpnp_conv3x3's tensors, flags and limits; stride 1, zero padding = dilation, so the output
 *       has the input's size.  dilation 1 and 2 are built; any other value is FMPNP_EINVAL and launches nothing.
 *       The contract is fmpnp_conv3x3's: every output is ONE fp32 accumulator's fmaf chain from +0 over
 *       k = ci * 9 + ky * 3 + kx ascending, acc = fmaf(a_k, w_k, acc), with
 *           a_k = in[b][ci][y + (ky - 1) * dilation][x + (kx - 1) * dilation], or 0 for a tap outside the image;
 *       then one fp32 add of bias[co] (FMPNP_CONV_BIAS), then the ReLU (FMPNP_CONV_RELU): fmpnp_conv3x3's epilogue,
 *       shared as code.  No split-K, no atomics: the bits do not depend on B, the stream, the tile form or the grid.
 *       With dilation 1 the result is fmpnp_conv3x3's bit for bit (the GPU form is that entry point's own launch).
 *       The off-map rule.  A tap outside the image, and the zero tail that pads k to the kernel's k tile,
 *       contribute fmaf(0, w, acc) -- they are NOT skipped.  For finite w nothing changes (an accumulator of -0
 *       would become +0); a NaN or infinite weight at such a tap makes the output NaN (0 * NaN, 0 * Inf) on the
 *       kernel and the twin alike, where torch's padding would also multiply it by a zero.  Inside the image a
 *       +-Inf or NaN input follows fmaf's IEEE rules in chain order on both: Inf * w accumulates +-Inf, Inf * 0 and
 *       Inf - Inf give NaN.  Callers keep weights and biases finite (fmpnp/encoder.py checks when a plan is built);
 *       as for fmpnp_conv3x3, which NaN a non-finite activation yields (sign, payload) and products or sums in the
 *       subnormal range are UNSPECIFIED.  There is no fp16 precision of the dilated form.
 *   Average pool.  in [B][C][H][W] -> out [B][C][H - 1][W - 1]: 2 x 2 windows, stride 1, no padding (ceil or floor
 *       mode and count_include_pad make no difference).  H < 2 or W < 2 (an empty output) is FMPNP_EINVAL.
 *           out[y][x] = (((in[y][x] + in[y][x + 1]) + in[y + 1][x]) + in[y + 1][x + 1]) * 0.25f,
 *       three fp32 adds in this order and one multiplication (exact short of underflow), stated once in
 *       csrc/fmpnp_encoder_impl.h for the kernel and the twin.  NaN and +-Inf pass through as IEEE addition has it.
 *       out must not overlap in.
 *   Pyramid step.  cur [B][C][h][w], prev [B][C][hp][wp] or NULL (hp, wp are then ignored), out [B][C][h][w];
 *       flags: FMPNP_PYR_NORMALIZE or 0.  For every texel and channel
 *           v = cur + r,   r = prev resized to h x w, bilinear, align_corners=True,
 *       the resize being fmpnp_hypercolumn_assemble's (axis_scale, axis_tap and bilerp of
 *       csrc/fmpnp_hypercolumn_impl.h: the same taps, weights and roundings), the add ONE fp32 add, skipped when prev
 *       is NULL (v = cur, the bits of cur).  Without the flag out = v.  With it
 *           out = v / max(n, 1e-12f),
 *       n the assembly's norm of the v over the channels of the texel: fp64 chains acc = fma(v, v, acc) over blocks
 *       of 64 channels, the block sums added in block order, n = (float)sqrt(sum).  The clamp is
 *       torch.nn.functional.normalize's, which the assembly does not have: an all-zero column gives 0, not NaN.  A
 *       NaN norm is not clamped: a NaN (or a pair of infinities that make one) in any channel makes its texel's
 *       whole column NaN and touches no other texel.  out MAY BE cur itself (the reference's in-place +=): every
 *       element of cur is read before the same element of out is written.  out must not overlap cur in any other
 *       way and must not overlap prev.
 *   Limits.  B, C, H, W, h, w (and hp, wp with a prev) >= 1, every size at most 2^24 and every tensor below 2^31
 *       elements (FMPNP_EINVAL, FMPNP_ETOOBIG); NULL cur or out, unknown flag bits: FMPNP_EINVAL. */
#define FMPNP_PYR_NORMALIZE 1
int fmpnp_conv3x3_dilated_async(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias,
                                int Cout, int flags, float *out, int dilation, void *hip_stream);
int fmpnp_conv3x3_dilated(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                          int flags, float *out, int dilation, void *hip_stream);
int fmpnp_conv3x3_dilated_cpu(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias,
                              int Cout, int flags, float *out, int dilation, int n_threads);
int fmpnp_avgpool2x2s1_async(const float *in, int B, int C, int H, int W, float *out, void *hip_stream);
int fmpnp_avgpool2x2s1(const float *in, int B, int C, int H, int W, float *out, void *hip_stream);
int fmpnp_avgpool2x2s1_cpu(const float *in, int B, int C, int H, int W, float *out, int n_threads);
int fmpnp_dense_pyramid_step_async(const float *cur, const float *prev, int B, int C, int h, int w, int hp, int wp,
                                   float *out, int flags, void *hip_stream);
int fmpnp_dense_pyramid_step(const float *cur, const float *prev, int B, int C, int h, int w, int hp, int wp, float *out,
                             int flags, void *hip_stream);
int fmpnp_dense_pyramid_step_cpu(const float *cur, const float *prev, int B, int C, int h, int w, int hp, int wp,
                                 float *out, int flags, int n_threads);

/* ---- image front end (opt-in): Pillow-exact 8-bit Lanczos resize and the networks' value transforms ----
 * Decoded uint8 pixels in, the bytes or the float32 tensor the networks take out: the stage the reference runs on the
 * host in s2dhm/network/images_from_list.py:57-103 (PIL thumbnail / resize with Image.ANTIALIAS, then ToTensor +
 * Normalize), s2dhm/d2net_utils/extract_dense_features.py:27-45 (the same resize, then the d2-net "caffe" / "torch"
 * preprocessing) and s2dhm/superpoint/detect_and_compute_superpoint.py:6-10 (gray / 255).  Decoding a file stays on the
 * host.  Pillow's 8-bit resampling is fixed-point integer arithmetic, so the result is Pillow's BIT FOR BIT
 * (Image.resize(size, Image.LANCZOS) of Pillow 12.2.0, recorded in tests/golden/image_lanczos.npz), not within a
 * tolerance.
 *
 *   Tensors.  src: uint8 [B][H][W][3], pixel (b, y, x) at src + b * image_stride + y * row_stride + 3 x (strides in
 *       bytes; a crop view of a larger image works; image_stride is ignored for B = 1; the images of a batch share one
 *       size).  dst: uint8 [B][h][w][3] (fmpnp_image_resize_u8) or float32 [B][C][h][w] (fmpnp_image_to_tensor; C = 3, or
 *       1 for FMPNP_IMAGE_GRAY), contiguous.
 *   Coefficient tables.  Built on the host in double, once per (input size, output size) pair of an axis; the kernels
 *       and the twins consume the same table.  For `in` source and `out` output samples:
 *           scale = in / out, fs = max(scale, 1.0), support = 3.0 * fs, ksize = (int)ceil(support) * 2 + 1;
 *           for output xx: center = (xx + 0.5) * scale,
 *                          xmin = max((int)(center - support + 0.5), 0),
 *                          xmax = min((int)(center + support + 0.5), in) - xmin,
 *                          w[x] = L((x + xmin - center + 0.5) * (1.0 / fs)) for x < xmax,
 *           L(t) = sinc(t) * sinc(t / 3) on -3 <= t < 3, otherwise 0; sinc(t) = sin(pi t) / (pi t), sinc(0) = 1;
 *           each w[x] divided by the left-to-right sum ww of the w[x], if ww != 0;
 *           k[x] = (int)(w < 0 ? -0.5 + w * 2^22 : 0.5 + w * 2^22).
 *       (The argument of L is multiplied by the reciprocal 1.0 / fs, as Pillow's precompute_coeffs does, not divided
 *       by fs.)  sin is the C library's, as in Pillow: equality with the recorded Pillow results assumes the same sin
 *       values.  glibc's sin is correctly rounded in all but exceedingly rare cases and has been stable across the 2.2x
 *       and 2.3x releases; a C library whose sin differs in the last place could move a coefficient by one unit of
 *       2^-22, and the twin and the kernel would still agree with each other.
 *   One pass.  acc = 2^21 + sum over x < xmax of src[xmin + x] * k[x] in int32 (a coefficient fits 24 signed bits, a
 *       pixel 8; 255 * sum |k| < 2^31 for Lanczos, so acc cannot overflow); the result is clamp(acc >> 22, 0, 255) with
 *       an arithmetic shift.
 *   Order.  The horizontal pass runs first and only if w != W; it rounds to uint8.  The vertical pass runs on that
 *       uint8 image and only if h != H.  With the size unchanged the bytes pass through.  The intermediate rounding is
 *       part of Pillow's result.
 *   Value transforms (fmpnp_image_to_tensor's mode), the epilogue of the last pass, p the resized byte of output
 *       channel c:
 *           FMPNP_IMAGE_TORCH  ((float)p / 255.0f - mean[c]) / std[c]: two true fp32 divisions and one fp32
 *                              subtraction, no reciprocal, no contraction (torchvision's ToTensor + Normalize bit for
 *                              bit; multiplying by 1/255 is not).  mean / std NULL: (0.485, 0.456, 0.406) and
 *                              (0.229, 0.224, 0.225).
 *           FMPNP_IMAGE_CAFFE  channels reversed to BGR, (float)p - mean[c]; mean NULL: (103.939, 116.779, 123.68)
 *                              (mean[c] belongs to OUTPUT channel c); std must be NULL.
 *           FMPNP_IMAGE_RAW    (float)p; mean and std must be NULL.
 *           FMPNP_IMAGE_GRAY   one channel, (float)y / 255.0f with y = (9798 a + 19235 g + 3735 b + 16384) >> 15,
 *                              g the source's channel 1; with the flag FMPNP_IMAGE_SWAP_RB a is the source's channel
 *                              2 and b its channel 0 (the reference hands cv2.imread's BGR pixels to COLOR_RGB2GRAY, so
 *                              for an RGB source its weighting is the swapped one); without it a is channel 0, the
 *                              conventional weighting.  Parity of these weights and this rounding with OpenCV 4.2's
 *                              cvtColor is UNPINNED: cv2 is not available to the tests.  mean and std must be NULL.
 *       The flag is FMPNP_EINVAL with any other mode.
 *   Launch independence.  Every output byte or float depends only on its own image, the sizes and the mode: not on B,
 *       the position in the batch, the stream, the tile, the strides or the alignment of the source.
 *   Forms.  *_async: DEVICE pointers; at most two launches on hip_stream (one without a resize, which then touches the
 *       caller's memory only).  With a resize the intermediate image and the tables live in the library's scratch of
 *       (device, stream): its growth (stream-ordered allocation), a table's upload from pinned staging and the launches
 *       are all ordered on hip_stream and nothing is waited for, except that replacing one of the four cached axis
 *       tables first waits until the replaced table's own upload has been read.  The plain forms queue the same and
 *       wait for the stream.  *_cpu: the CPU twins, HOST pointers, the same bits for any n_threads (0: every core);
 *       explicit entry points, never a fallback.
 *   Errors.  NULL src or dst, a size below 1, row_stride < 3 W, image_stride (B > 1) smaller than an image, a
 *       destination that overlaps the source, an unknown mode or flag, mean / std where the mode takes none,
 *       n_threads < 0: FMPNP_EINVAL.  A size or B above 16384, a destination of 2^33 bytes or more: FMPNP_ETOOBIG.
 *       An allocation that fails: FMPNP_ENOMEM.  mean and std are HOST memory [3] in every form.
 *   Out of scope.  Decoding; Pillow's reducing_gap (thumbnail's integer box reduction from a 4x shrink on, JPEG draft:
 *       this is the fair resampling, Image.resize(..., reducing_gap=None)); other filters; alpha; 16-bit images. */
#define FMPNP_IMAGE_TORCH 0
#define FMPNP_IMAGE_CAFFE 1
#define FMPNP_IMAGE_RAW 2
#define FMPNP_IMAGE_GRAY 3
#define FMPNP_IMAGE_SWAP_RB 1
int fmpnp_image_resize_u8_async(const unsigned char *src, long long image_stride, long long row_stride, int B, int H,
                                int W, int h, int w, unsigned char *dst, void *hip_stream);
int fmpnp_image_resize_u8(const unsigned char *src, long long image_stride, long long row_stride, int B, int H, int W,
                          int h, int w, unsigned char *dst, void *hip_stream);
int fmpnp_image_resize_u8_cpu(const unsigned char *src, long long image_stride, long long row_stride, int B, int H,
                              int W, int h, int w, unsigned char *dst, int n_threads);
int fmpnp_image_to_tensor_async(const unsigned char *src, long long image_stride, long long row_stride, int B, int H,
                                int W, int h, int w, int mode, int flags, const float *mean, const float *std,
                                float *dst, void *hip_stream);
int fmpnp_image_to_tensor(const unsigned char *src, long long image_stride, long long row_stride, int B, int H, int W,
                          int h, int w, int mode, int flags, const float *mean, const float *std, float *dst,
                          void *hip_stream);
int fmpnp_image_to_tensor_cpu(const unsigned char *src, long long image_stride, long long row_stride, int B, int H,
                              int W, int h, int w, int mode, int flags, const float *mean, const float *std,
                              float *dst, int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* FMPNP_H */
