/*
 * splat_hip.h -- C ABI of libsplat_hip.so, the MI355X (gfx950) drop-in for the native half of the
 * Splat-SLAM mapping hot path.  Torch-free: plain device pointers, sizes and a stream handle.
 *
 * Which reference interface each entry point replaces (paths relative to /root/reference):
 *
 *   sgr_forward            -> diff_gaussian_rasterization._C.rasterize_gaussians, reached through
 *                             GaussianRasterizer.forward at
 *                             thirdparty/gaussian_splatting/gaussian_renderer/__init__.py:130-141
 *                             (settings built at :58-72).  The native source is the un-vendored submodule
 *                             thirdparty/diff-gaussian-rasterization-w-pose (.gitmodules:4-6, README.md:88-92).
 *   sgr_backward           -> diff_gaussian_rasterization._C.rasterize_gaussians_backward, triggered by
 *                             loss.backward() at src/mapper.py:329,490,699.
 *   sgr_saved_bytes,
 *   sgr_scratch_bytes      -> the resizeFunctional geom/binning/image buffer callbacks of the same module.
 *   sgr_mapping_loss       -> get_loss_mapping / get_loss_mapping_rgbd, thirdparty/monogs/utils/slam_utils.py:71-105
 *   sgr_ssim_scratch_bytes,
 *   sgr_ssim,
 *   sgr_ssim_backward      -> ssim of thirdparty/gaussian_splatting/utils/loss_utils.py:61-101 (the ssim_loss: True mapping loss,
 *                             thirdparty/monogs/utils/slam_utils.py:89-98, imported at src/mapper.py:35) and its autograd backward
 *   sgr_render_metrics     -> the PSNR / SSIM / depth-L1 part of eval_rendering, src/utils/eval_utils.py:90-128, called from
 *                             src/slam.py:153,193
 *   sgr_lpips_*            -> the LPIPS part of the same function (eval_utils.py:66-68, 125, 192: torchmetrics'
 *                             LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True))
 *   sgr_tsdf_*, sgr_mesh_* -> the mesh branch of the same function (eval_utils.py:70-74, 142-179: Open3D's ScalableTSDFVolume
 *                             integrate / extract_triangle_mesh) and clean_mesh (:331-379, trimesh connected components)
 *   sgr_surface_sample*, sgr_nn_*, sgr_icp_accumulate, sgr_cloud_metrics, sgr_eval_reduce_bytes
 *                          -> the eval_mesh branch of the same function (eval_utils.py:174-187: run_evaluation of
 *                             evaluate_3d_reconstruction_lib, distance_thresh 0.05, icp_align=True): surface sampling, exact nearest
 *                             neighbours, point-to-point ICP sums and the accuracy / completion reductions
 *   sgr_traj_*             -> src/utils/eval_traj.py: the camera centres and the skip rule of align_kf_traj (:20-55) and align_full_traj
 *                             (:57-80), the sums behind evo's PoseTrajectory3D.align(correct_scale=True) (umeyama_alignment), and the
 *                             errors and statistics of traj_eval_and_plot (:83-110: APE of the translation part, get_all_statistics);
 *                             sgr_traj_associate and sgr_traj_pose_errors: evo's time association and its APE / RPE of every pose relation
 *   sgr_plot_*             -> the per-keyframe figure of the same function (eval_utils.py:131-135, plot_rgbd_silhouette): the six cells,
 *                             their titles and the heading as one RGB panel
 *   sgr_frame_prepare      -> BaseDataset.__getitem__ / get_color of src/utils/datasets.py:133-216: cv2.undistort, cv2.resize, / 255, the
 *                             nearest resize of the depth and the crop of the edge (the project's own integer arithmetic, not OpenCV's bits)
 *   sgr_adam_step          -> torch.optim.Adam(eps=1e-15) over the GaussianModel groups,
 *                             thirdparty/gaussian_splatting/scene/gaussian_model.py:264-313, stepped at
 *                             src/mapper.py:352,557,703
 *   sgr_activate,
 *   sgr_gaussian_adam_step,
 *   sgr_gaussian_adam_shard -> the activation getters (exp / normalize / sigmoid, gaussian_model.py:76-101) and the Adam step of
 *                             the five per-Gaussian groups incl. the isotropy regulariser of src/mapper.py:487-489
 *   sgr_masked_adam        -> the keyframe (exposure) optimiser of src/mapper.py:1096-1111, stepped at :561
 *   sgr_map_views          -> the per-view body of Mapper.map (src/mapper.py:426-490): render, loss, backward for <= 16 views
 *   sgr_map_step           -> one iteration of Mapper.map / initialize_map / final_refine (src/mapper.py:303-353, 414-568, 656-708)
 *   sgr_map_run            -> a run of such iterations between two densify / reset points (the `for` loops at :304, :414, :656)
 *   sgr_ssim_term_bytes,
 *   sgr_mapping_loss_ssim,
 *   sgr_map_step_ssim,
 *   sgr_map_run_ssim       -> the same with the ssim_loss: True mapping loss, thirdparty/monogs/utils/slam_utils.py:89-105
 *   sgr_deform_points      -> Mapper.update_mapping_points, src/mapper.py:154-255
 *   sgr_keep_list,
 *   sgr_gather_rows        -> prune_points / _prune_optimizer and the row selects of densify_and_clone,
 *                             thirdparty/gaussian_splatting/scene/gaussian_model.py:519-557, 690-719
 *   sgr_query*, sgr_profile_*,
 *   sgr_set_option         -> (no reference counterpart) capacity protocol, work counters, per-kernel HIP-event timing, options
 *   sknn_dist2             -> simple_knn._C.distCUDA2, thirdparty/gaussian_splatting/scene/gaussian_model.py:18,194-200
 *   sgr_dba_*              -> droid_backends.{ba, frame_distance, projmap, iproj, depth_filter} (thirdparty/glorie_slam/lib/droid.cpp),
 *                             thirdparty/glorie_slam/depth_video.py:195-204 (frame_distance), :231 (ba), :363 (depth_filter)
 *   sgr_video_*            -> DepthVideo.upsample (:154-158) and update_valid_depth_mask (:340-375) of the same file
 *   sgr_dspo_*             -> stage 2 ("depth_scale") of DepthVideo.dspo, thirdparty/glorie_slam/depth_video.py:236-299:
 *                             BA_with_scale_shift (thirdparty/glorie_slam/geom/ba.py) and align_scale_and_shift
 *                             (src/utils/common.py:68-104)
 *   sgr_corr_*             -> droid_backends.{corr_index_forward, corr_index_backward, altcorr_forward, altcorr_backward}
 *                             (thirdparty/glorie_slam/lib/droid.cpp), called from CorrSampler and CorrLayer of
 *                             thirdparty/glorie_slam/modules/droid_net/corr.py:27,34,98,106
 *   sgr_graph_*            -> FactorGraph.update's reprojection and motion features and the edge selection of
 *                             add_proximity_factors / add_backend_proximity_factors, thirdparty/glorie_slam/factor_graph.py
 *   se3_*                  -> lietorch SE3 ops used on the mapping path, thirdparty/glorie_slam/depth_video.py:327-330
 *                             (SE3(pose).inv().matrix()), and the tau convention of
 *                             thirdparty/monogs/utils/pose_utils.py:66-98.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 / int32 unless it says "host";
 *   - [N,C] arrays are row-major; images are CHW; 4x4 matrices are 16 floats in the layout the reference
 *     passes them (transposed / row-vector convention: camera_utils.py:94-104, mapper.py:841-850);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued on it;
 *   - functions return 0 on success, a negative SgrStatus otherwise; sgr_last_error() gives the text;
 *   - the library never allocates device memory: the caller owns inputs, outputs and both workspaces.
 */
#ifndef SPLAT_HIP_H_
#define SPLAT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGR_ABI_VERSION 10

/* In front of a pointer to a scalar: it addresses HOST memory (every unmarked pointer to a scalar or to void is a device pointer
 * unless its comment says otherwise).  Expands to nothing; the Python binding reads it to give the pointer its element type. */
#define SGR_HOST

typedef enum SgrStatus {
  SGR_OK = 0,
  SGR_ERR_INVALID = -1,     /* bad argument (null pointer, inconsistent option set, ...)            */
  SGR_ERR_WORKSPACE = -2,   /* saved / scratch workspace smaller than sgr_*_bytes() demands          */
  SGR_ERR_CAPACITY = -3,    /* more (tile, Gaussian) pairs than `capacity`; *num_rendered_host = need */
  SGR_ERR_HIP = -4          /* a HIP runtime call failed                                              */
} SgrStatus;

/* The 13 fields of GaussianRasterizationSettings (gaussian_renderer/__init__.py:58-72) + array extents. */
typedef struct SgrSettings {
  int32_t num_gaussians;       /* N */
  int32_t image_height;
  int32_t image_width;
  int32_t sh_degree;           /* active degree (0..3) */
  int32_t sh_coeffs;           /* M: `shs` is [N, M, 3]; ignored when colors_precomp is given */
  float tanfovx;
  float tanfovy;
  float scale_modifier;
  int32_t prefiltered;
  int32_t debug;
  const float* bg;             /* [3]  */
  const float* viewmatrix;     /* [16] world_view_transform  (W2C transposed) */
  const float* projmatrix;     /* [16] full_proj_transform   */
  const float* projmatrix_raw; /* [16] projection_matrix     */
  const float* campos;         /* [3]  */
} SgrSettings;

/* Arguments of GaussianRasterizer.forward (gaussian_renderer/__init__.py:130-141). NULL = "None". */
typedef struct SgrInputs {
  const float* means3D;        /* [N,3] */
  const float* opacities;      /* [N]   */
  const float* shs;            /* [N,M,3] or NULL */
  const float* colors_precomp; /* [N,3]   or NULL */
  const float* scales;         /* [N,3]   or NULL */
  const float* rotations;      /* [N,4]   or NULL (w,x,y,z; used as given, not re-normalised) */
  const float* cov3D_precomp;  /* [N,6]   or NULL */
} SgrInputs;

/* The 5-tuple returned at gaussian_renderer/__init__.py:130. */
typedef struct SgrOutputs {
  float* color;                /* [3,H,W] */
  float* depth;                /* [1,H,W] */
  float* opacity;              /* [1,H,W] */
  int32_t* radii;              /* [N] */
  int32_t* n_touched;          /* [N] */
} SgrOutputs;

typedef struct SgrWorkspace {
  void* saved;                 /* lives from forward until the matching backward (one per forward call) */
  size_t saved_bytes;
  void* scratch;               /* transient inside one call; may be shared by calls on the same stream   */
  size_t scratch_bytes;
  int64_t capacity;            /* max (tile, Gaussian) pairs the workspaces were sized for               */
  int32_t counters_clean;      /* != 0: the per-tile pair counters inside `saved` are zero -- every completed forward
                                  (same N, H, W, capacity) leaves them so; 0 for a fresh / foreign block: the library
                                  then spends one extra launch zeroing them */
  int32_t max_list_hint;       /* > 0: the LONGEST per-8x8-tile list the caller has measured for these cameras (header word 10 of a
                                  recent forward, sgr_query_header): picks the sort build of the compositing kernels -- a
                                  deterministic function of a measurement.  0: guessed from `capacity` / tiles */
} SgrWorkspace;

typedef struct SgrGradOutputs {
  const float* dL_dcolor;      /* [3,H,W] */
  const float* dL_ddepth;      /* [1,H,W] or NULL (= zeros) */
} SgrGradOutputs;

/* Every pointer may be NULL when the caller does not need that gradient. Written, not accumulated. */
typedef struct SgrGradInputs {
  float* dL_dmeans3D;          /* [N,3] */
  float* dL_dmeans2D;          /* [N,3]  (x,y in NDC-scaled pixel units, z = 0) */
  float* dL_dopacities;        /* [N]   */
  float* dL_dshs;              /* [N,M,3] */
  float* dL_dcolors_precomp;   /* [N,3] */
  float* dL_dscales;           /* [N,3] */
  float* dL_drotations;        /* [N,4] */
  float* dL_dcov3D_precomp;    /* [N,6] */
  float* dL_dtau;              /* [6] = (rho[3], theta[3]) summed over Gaussians */
  /* --- fused mapping-loop extensions (all optional; zero / NULL = plain backward) ------------------------------
   * accumulate != 0: the per-Gaussian gradients above are ADDED to the buffers (only Gaussians with radii > 0 are
   * touched), so the <= 12 views of one mapping iteration (src/mapper.py:426-490) sum without autograd.
   * stat_*: densification statistics of add_densification_stats + the max_radii2D update
   * (gaussian_model.py:738-742, src/mapper.py:522-529), fused into the same pass:
   *   stat_grad_accum[i] += |dL_dmeans2D[i, :2]|, stat_denom[i] += 1, stat_max_radii[i] = max(., radii[i])
   *   for every Gaussian with radii > 0. */
  int32_t accumulate;
  float* stat_grad_accum;      /* [N] */
  float* stat_denom;           /* [N] */
  float* stat_max_radii;       /* [N] */
} SgrGradInputs;

int sgr_abi_version(void);
const char* sgr_last_error(void);

size_t sgr_saved_bytes(int32_t num_gaussians, int32_t image_height, int32_t image_width, int64_t capacity);
size_t sgr_scratch_bytes(int32_t num_gaussians, int32_t image_height, int32_t image_width, int64_t capacity);

/* num_rendered_host: host pointer or NULL.
 *   non-NULL: the call synchronises once on `stream` to learn the pair count R, sorts exactly R pairs, stores R
 *             there, and fails with SGR_ERR_CAPACITY (outputs untouched) when R > ws->capacity;
 *   NULL    : fully asynchronous; pairs beyond ws->capacity are dropped and the overflow word of the saved
 *             block is raised -- poll it with sgr_query().
 * Overflow word: 0 = fine; 1 = R > capacity (grow the workspace and redo); 2 = more than 65280 splats fell on ONE 8x8 tile
 * (the per-tile pair counters are 16-bit fields of a word shared by a 2x2 block of tiles; only a degenerate map gets there)
 * -- the synchronous form fails with SGR_ERR_INVALID.  A view whose overflow word is non-zero contributes zeros to
 * sgr_backward / sgr_map_* gradients instead of sums over truncated lists. */
int sgr_forward(const SgrSettings* settings, const SgrInputs* in, const SgrOutputs* out,
                const SgrWorkspace* ws, SGR_HOST int64_t* num_rendered_host, void* stream);

int sgr_backward(const SgrSettings* settings, const SgrInputs* in, const int32_t* radii,
                 const SgrGradOutputs* grad_out, const SgrGradInputs* grad_in,
                 const SgrWorkspace* ws, void* stream);

/* The backward of SEVERAL forwards that share the Gaussian inputs, in one host call and -- when the views share N, H, W, the
 * view-independent settings and the capacity, and have private scratch blocks -- one launch per stage: what a mapping
 * iteration's loss.backward() asks of the rasterizer (src/mapper.py:426-490: up to 12 forwards, then ONE backward).  The
 * per-Gaussian gradients in `grad_in` are the SUMS over the views (written in full when grad_in->accumulate == 0, added
 * otherwise); every view additionally receives its own dL_dmeans2D ([N,3]; only rows of Gaussians with radii > 0 are written:
 * pass a zeroed buffer) and dL_dtau ([6]).  grad_in->dL_dmeans2D / dL_dtau are ignored.  The drop-in package's autograd
 * collector calls this once per backward pass. */
typedef struct SgrBackwardView {
  SgrSettings settings;
  const int32_t* radii;        /* [N] as written by the view's sgr_forward */
  SgrWorkspace ws;             /* the view's saved block + a scratch block of its own */
  const float* dL_dcolor;      /* [3,H,W] */
  const float* dL_ddepth;      /* [1,H,W] or NULL */
  float* dL_dmeans2D;          /* [N,3] zero-initialised by the caller, or NULL */
  float* dL_dtau;              /* [6] or NULL */
} SgrBackwardView;
int sgr_backward_views(int32_t num_views, const SgrBackwardView* views, const SgrInputs* in, const SgrGradInputs* grad_in,
                       void* stream);

/* add_densification_stats + the max_radii2D update of one view (gaussian_model.py:738-742, src/mapper.py:522-529) in one pass:
 * for every Gaussian with radii > 0: grad_accum += |dL_dmeans2D[i, :2]|, denom += 1, max_radii = max(max_radii, radii). */
int sgr_densify_stats(int64_t n, const float* dL_dmeans2D, const int32_t* radii, float* stat_grad_accum, float* stat_denom,
                      float* stat_max_radii, void* stream);

/* Synchronous read-back of (pair count, overflow flag) from a saved block produced by sgr_forward. */
int sgr_query(const void* saved, SGR_HOST int64_t* num_rendered_host, SGR_HOST int32_t* overflow_host, void* stream);

/* The whole 64-byte header of a saved block, synchronously: uint32 words [0] pair count R the workspace must hold (the larger of
 * pairs binned and partial slots reserved), [1] overflow flag, [2] pairs sorted, [3] visible Gaussians, [4] tiles with more
 * than 64 pairs, [5..8] internal, [9] pairs actually binned, [10] longest per-tile list, [11] internal, [12] STICKY: number of
 * forwards of this workspace whose overflow flag came out non-zero since the block's counters were last zeroed (counters_clean = 0),
 * [13] STICKY: the largest [0] of any of those forwards -- [1] only describes the LAST forward, and a span of sgr_map_run puts dozens
 * of forwards through one workspace between two host checks -- [14] internal (a flag between two blocks of the binning kernel: zero
 * whenever no forward is running), [15] zero. */
int sgr_query_header(const void* saved, SGR_HOST uint32_t words_host[16], void* stream);

/* Asynchronous variant: enqueues a 64-byte copy of the same header into PINNED host memory on `stream`.
 * The caller pre-sets word 15 to a non-zero sentinel and knows the copy has landed when it reads 0 there: a later call can
 * then learn R without ever waiting (the drop-in package sizes its capacity this way). */
int sgr_header_to_host(const void* saved, void* pinned_host64, void* stream);

/* Work counters of one forward, read back synchronously (bench / roofline accounting only):
 *   stats[0] = V  Gaussians with radii > 0          stats[1] = R  (tile, Gaussian) pairs binned
 *   stats[2] = R_eff = sum over tiles of min(list length, last contributor): pairs the blend kernels walk
 *   stats[3] = number of non-empty 8x8 tiles */
int sgr_query_stats(const SgrWorkspace* ws, int32_t num_gaussians, int32_t image_height, int32_t image_width,
                    const int32_t* radii, SGR_HOST int64_t stats_host[4], void* stream);
/* The fp32 view-space depth of every Gaussian with radii > 0 as the forward computed it (0 elsewhere) -- the bit pattern
 * that orders the splats of a tile.  Parity tooling: lets a comparison break depth near-ties (equal to the last ulp) the way
 * this forward did.  depth_out: device [N]. */
int sgr_query_depth_keys(const SgrWorkspace* ws, int32_t num_gaussians, int32_t image_height, int32_t image_width,
                         const int32_t* radii, float* depth_out, void* stream);
/* Histogram of the per-tile list lengths the blend kernels walk (same synchronous, accounting-only use):
 * bins 0, 1-4, 5-8, 9-16, 17-32, 33-64, 65-256, >256 splats. */
int sgr_query_list_histogram(const SgrWorkspace* ws, int32_t num_gaussians, int32_t image_height, int32_t image_width,
                             SGR_HOST int64_t hist_host[8], void* stream);

/* Run-time options of the library (process-wide; no reference counterpart).
 *   SGR_OPT_FUSED_BLEND (default 1): sgr_map_views / sgr_map_step / sgr_map_run composite a tile, evaluate the mapping loss
 *     and run the tile's backward in ONE kernel (the same wave, pixel state in registers).  0: the two halves run as the
 *     separate kernels sgr_forward / sgr_backward use (bitwise identical results) -- for timing the halves on their own.
 *   SGR_OPT_UPSTREAM_POSE_JACOBIAN (default 0): how the projected-mean path enters the camera-pose gradient dL/dtau.
 *     0: the exact derivative of the projection (x_ndc = (P00 X + P02 Z) / Z ...), what autograd through the reference's
 *        own SE3_exp / update_pose convention gives (thirdparty/monogs/utils/pose_utils.py:66-98);
 *     1: the form the pinned CUDA rasterizer is believed to use: five scalars of projmatrix_raw
 *        (P00, P11, P22, P23, P32), d x_ndc / d p_cam = (P00 / w, 0, -x_hom / w^2) -- i.e. WITHOUT the principal-point terms
 *        P02 / w, P12 / w.  Identical when cx = W/2 and cy = H/2; differs by O(|P02|) otherwise (8e-4 on Replica).  Only
 *        dL/dtau changes; every other gradient is the same.  The oracle has the same switch (UPSTREAM_POSE_JACOBIAN).
 *   SGR_OPT_SEGMENT_TEST (default 0): the forward tests every 256-Gaussian segment's bounding box against each view before
 *     testing its Gaussians one by one (a map that grows keyframe by keyframe is spatially coherent: whole segments miss
 *     whole views).  Conservative: results are identical either way.  Off by default because it does not pay on MI355X:
 *     preprocess_fwd is bound by its counting atomics and output writes, not by the per-Gaussian visibility arithmetic
 *     (measured on a keyframe-ordered 300 k map: 65.6 us with, 64.7 us without).
 *   SGR_OPT_ADAM_IN_K1 (default 1; SGR_ADAM_IN_K1=0 in the environment, read once, also turns it off): inside sgr_map_run the
 *     optimiser step of every iteration but the last is not a launch of its own: the blocks of the next iteration's forward
 *     preprocess run it for their own 256 Gaussians before they start (bitwise identical results) -- where that launch has one
 *     block per segment, i.e. on maps large enough to fill the chip that way (sgr_common.h: k1_parts_for).  0: every step is
 *     launched on its own, the sequence sgr_map_step gives.  2: on every map; the forward preprocess of such an iteration then
 *     runs with one block per segment whatever the map's size (tests and experiments on small maps). */
#define SGR_OPT_FUSED_BLEND 0
#define SGR_OPT_UPSTREAM_POSE_JACOBIAN 1
#define SGR_OPT_SEGMENT_TEST 2
#define SGR_OPT_ADAM_IN_K1 3
#define SGR_OPT_COUNT 4
int sgr_set_option(int32_t option, int32_t value);
int sgr_get_option(int32_t option);

/* Per-kernel HIP-event timing.  kind: 0 preprocess_fwd (+ binning; + the previous iteration's optimiser step where the launch
 * carries it, SGR_OPT_ADAM_IN_K1), 1 tile_scan, 2 scatter, 3 fused tile kernel (blend
 * forward + loss + blend backward), 4 blend_fwd (+ in-wave tile sort), 5 blend_bwd, 6 preprocess_bwd (+ gather, pose reduce)
 * and the optimiser pass where it is a launch of its own (a record of its own).  sgr_profile_enable(mask) arms event pairs around the kinds whose
 * bit is set (0 disarms); sgr_profile_read() synchronises, returns accumulated milliseconds and launch counts per
 * kind since the last read, and resets them. Events are recorded on the stream the kernel is launched on. */
#define SGR_PROFILE_KINDS 7
int sgr_profile_enable(uint32_t kind_mask);
int sgr_profile_read(SGR_HOST float ms_host[SGR_PROFILE_KINDS], SGR_HOST int64_t launches_host[SGR_PROFILE_KINDS]);

/* Fused mapping loss (slam_utils.py:71-105): loss = alpha*mean|m*(e^a*I+b) - m*gt| + (1-alpha)*mean|md*D - md*gtD|
 * with m = (sum_c gt > rgb_boundary_threshold), md = (gtD > 0.01).  Writes loss[1] and the four gradients
 * scaled by `upstream` (dLoss/dloss).  exposure may be NULL (initialization=True branch, :72-73). */
int sgr_mapping_loss(int32_t H, int32_t W, const float* image, const float* depth,
                     const float* gt_image, const float* gt_depth,
                     const float* exposure_a, const float* exposure_b,
                     float alpha, float rgb_boundary_threshold, float upstream,
                     float* loss, float* dL_dimage, float* dL_ddepth, float* dL_dexp_a, float* dL_dexp_b,
                     void* scratch, size_t scratch_bytes, void* stream);

/* SSIM (loss_utils.py:36-101): 11-tap Gaussian window of sigma 1.5 (the 2-D window its outer product), every channel filtered on
 * its own with zero padding 5, C1 = 0.01^2, C2 = 0.03^2.  img1, img2: [B,C,H,W].  sgr_ssim writes the mean of the SSIM map of each
 * image to ssim_out[B] (the reference's size_average=True result is their mean).  With `maps` != NULL ([3,B,C,H,W]) it also writes
 * the three per-pixel derivatives of an image's mean, divided by C*H*W, that sgr_ssim_backward needs:
 *   dm = d/dmu1 (through the sigmas), d11 = d/dE[x^2], d12 = d/dE[xy]   (x = img1, y = img2, E = the window average).
 * sgr_ssim_backward: dL/dimg1 = u_b * (G*dm + 2 x (G*d11) + y (G*d12)) with u_b = upstream[b * upstream_stride] * upstream_scale
 * (device scalar: no host sync; stride 0 broadcasts one value).  Only img1 is differentiated (ssim(image, gt_image)).
 * `scratch` (sgr_ssim_scratch_bytes) holds the per-workgroup partials: fixed-order sums, bitwise reproducible. */
size_t sgr_ssim_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int sgr_ssim(int32_t B, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, float* ssim_out, float* maps,
             void* scratch, size_t scratch_bytes, void* stream);
int sgr_ssim_backward(int32_t B, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* maps,
                      const float* upstream, int32_t upstream_stride, float upstream_scale, float* dL_dimg1, void* stream);

/* Rendering metrics of eval_rendering (eval_utils.py:90-128) for n frames of [C,H,W] in one call (launches of up to 16 frames
 * each plus one final pass), host array `frames`:
 *   image    = clamp(exp(a) * render + b, 0, 1)  (:96-100; exposure NULL = identity, the first frame),
 *   psnr     = 20 log10(1 / sqrt(mean over gt > 0 of (image - gt)^2))   (:109,123, image_utils.py:19-21),
 *   ssim     = ssim(image, gt_image)                                      (:124),
 *   depth_l1 = mean over depth > 0 and gt_depth > 0 of |global_scale * depth - gt_depth|   (:116-120; depth [H,W] may be NULL).
 * out[3 * f + 0..2] = (psnr, ssim, depth_l1) of frame f on the device.  An empty mask gives NaN (the reference's 0/0), a perfect
 * frame PSNR inf.  scratch: sgr_ssim_scratch_bytes(n, C, H, W). */
typedef struct SgrMetricFrame {
  const float* render;         /* [C,H,W] */
  const float* gt_image;       /* [C,H,W] */
  const float* depth;          /* [H,W] rendered depth, or NULL */
  const float* gt_depth;       /* [H,W], or NULL */
  const float* exposure_a;     /* device scalar, or NULL */
  const float* exposure_b;     /* device scalar, or NULL */
} SgrMetricFrame;
int sgr_render_metrics(int32_t n, const SgrMetricFrame* frames, int32_t C, int32_t H, int32_t W, float global_scale, float* out,
                       void* scratch, size_t scratch_bytes, void* stream);

/* TSDF fusion and mesh extraction of eval_rendering's `mesh` branch (eval_utils.py:70-74, 142-179; clean_mesh :331-379), after
 * Open3D's ScalableTSDFVolume (RGB8) and trimesh; the conventions are listed in DESIGN.md section 3.
 * The volume is a hash from unit key (16^3 voxels, unit length 16 * voxel_length) to a pool of units.  Unit u of the pool holds
 * SGR_TSDF_UNIT_FLOATS floats: five planes of 4096 voxels (tsdf, weight, r, g, b on 0..255), voxel v = x + 16 y + 256 z.
 * Keys pack floor(p / unit_length) per axis as three 21-bit offset-binary fields (x high), so keys sort as (x, y, z).
 * `state` (sgr_tsdf_bytes(hash_capacity)) holds the hash, the per-slot frame marks, the touched list and int32 counters:
 *   counters[0] units allocated (pool indices handed out), [1] != 0: the hash was full, [2] touched-list length,
 *   [3] != 0: integration met a unit beyond pool_capacity (a caller error).
 * Per chunk of <= SGR_TSDF_MAX_FRAMES frames: sgr_tsdf_touch (idempotent: it may be re-run after sgr_tsdf_rehash into a larger
 * hash), then the caller reads the counters once, grows the pool if counters[0] > pool_capacity (pool indices never change:
 * copy the old pool to the front of a zeroed larger one), and calls sgr_tsdf_integrate with counters[2].  Integration may not
 * be repeated: weights accumulate. */
#define SGR_TSDF_UNIT_FLOATS (5 * 4096)
#define SGR_TSDF_MAX_FRAMES 16
typedef struct SgrTsdfVolume {
  float voxel_length;          /* 5/512 in the reference */
  float sdf_trunc;             /* 0.04 */
  float depth_trunc;           /* 30: depth above it is dropped (create_from_color_and_depth) */
  int32_t hash_capacity;       /* power of two, >= 64 */
  int32_t pool_capacity;       /* units */
  void* state;                 /* sgr_tsdf_bytes(hash_capacity) */
  float* pool;                 /* [pool_capacity, SGR_TSDF_UNIT_FLOATS] */
} SgrTsdfVolume;
typedef struct SgrTsdfFrame {
  const float* render;         /* [3,H,W] rendered colour */
  const float* depth;          /* [H,W] rendered depth */
  const float* gt_depth;       /* [H,W]: depth is dropped where it is 0; or NULL */
  const float* exposure_a;     /* device scalar, or NULL (colour = clamp(exp(a) render + b, 0, 1), truncated to 0..255) */
  const float* exposure_b;     /* device scalar, or NULL */
  float fx, fy, cx, cy;
  float w2c[16];               /* host, row-major world -> camera */
  float global_scale;          /* depth = global_scale * rendered depth */
} SgrTsdfFrame;
size_t sgr_tsdf_bytes(int32_t hash_capacity);
int sgr_tsdf_reset(const SgrTsdfVolume* vol, void* stream);                       /* empty hash, zero counters and pool */
int sgr_tsdf_rehash(const SgrTsdfVolume* src, const SgrTsdfVolume* dst, void* stream);   /* dst: reset, larger; marks dropped */
int sgr_tsdf_touch(const SgrTsdfVolume* vol, int32_t n, const SgrTsdfFrame* frames, int32_t H, int32_t W, void* stream);
int sgr_tsdf_integrate(const SgrTsdfVolume* vol, int32_t n, const SgrTsdfFrame* frames, int32_t H, int32_t W, int32_t n_touched,
                       void* stream);
/* Marching cubes over the n_units allocated units (counters[0]) in ascending key order: sgr_tsdf_extract_count writes
 * totals[0..1] = (vertices, triangles) on the device; sgr_tsdf_extract then writes vertices [V,3], colours [V,3] (0..1) and
 * triangles [F,3] with the same scratch.  Vertices are ordered by (unit key, voxel, edge x/y/z), triangles by (unit key, cube,
 * table order). */
size_t sgr_tsdf_extract_bytes(int32_t hash_capacity, int32_t pool_capacity);
int sgr_tsdf_extract_count(const SgrTsdfVolume* vol, int32_t n_units, void* scratch, size_t scratch_bytes, int32_t* totals,
                           void* stream);
int sgr_tsdf_extract(const SgrTsdfVolume* vol, int32_t n_units, void* scratch, size_t scratch_bytes, float* vertices,
                     float* colors, int32_t* triangles, void* stream);
/* clean_mesh: connected components over triangle edges (label = smallest vertex id of the component), components of at least
 * min_len vertices kept; then faces with a repeated index or zero area and repeated faces (same vertex set; the first is kept)
 * dropped.  sgr_mesh_components writes totals[0..1] = kept (vertices, triangles); sgr_mesh_compact writes them in their original
 * order, reindexed, and vertex_map[V] (new index or -1) when not NULL. */
size_t sgr_mesh_bytes(int32_t V, int32_t F);
int sgr_mesh_components(int32_t V, int32_t F, const float* vertices, const int32_t* triangles, int32_t min_len, void* scratch,
                        size_t scratch_bytes, int32_t* totals, void* stream);
int sgr_mesh_compact(int32_t V, int32_t F, const float* vertices, const float* colors, const int32_t* triangles, void* scratch,
                     size_t scratch_bytes, float* out_vertices, float* out_colors, int32_t* out_triangles, int32_t* vertex_map,
                     void* stream);

/* Mesh evaluation of eval_rendering's eval_mesh branch (eval_utils.py:174-187: run_evaluation(pred_ply, ..., distance_thresh=0.05,
 * icp_align=True) of evaluate_3d_reconstruction_lib, whose conventions are assumed as listed in DESIGN.md section 3).
 * sgr_surface_sample: n points drawn uniformly by area from the mesh (fp64 areas and CDF; the uniforms are a hash of (seed, sample
 * index), so the output does not depend on the launch shape), points [n,3] and the face of each [n]; *total_area (device, may be
 * NULL) receives the mesh's area.  Faces of zero area are never picked.  n = 0 only computes the area. */
size_t sgr_surface_sample_bytes(int32_t F);
int sgr_surface_sample(int32_t V, int32_t F, const float* vertices, const int32_t* triangles, int32_t n, uint64_t seed, void* scratch,
                       size_t scratch_bytes, float* points, int32_t* tri_idx, double* total_area, void* stream);
/* Exact nearest neighbours: sgr_nn_grid_build sorts the n target points (transformed by the host 3x4 row-major matrix `transform`
 * when not NULL) into a uniform grid held in `grid` (sgr_nn_grid_bytes(n) bytes, caller-owned, built once, queried many times).
 * sgr_nn_query: for each of the nq query points (transformed on the fly by `transform` when not NULL) dist = Euclidean distance to
 * the nearest target point and idx = its index (ties: the smallest index); where that distance exceeds max_dist (INFINITY: no
 * limit) dist = INFINITY and idx = -1. */
size_t sgr_nn_grid_bytes(int32_t n);
int sgr_nn_grid_build(int32_t n, const float* points, SGR_HOST const float* transform, void* grid, size_t grid_bytes, void* stream);
int sgr_nn_query(int32_t n, const void* grid, size_t grid_bytes, int32_t nq, const float* query, SGR_HOST const float* transform,
                 float max_dist, float* dist, int32_t* idx, void* stream);
/* Fixed-order fp64 reductions (per-workgroup partials in `scratch` of sgr_eval_reduce_bytes() bytes, then one ordered pass; no
 * float atomics).  sgr_icp_accumulate: over the sources with idx >= 0, p = transform * source (as sgr_nn_query forms it) and
 * q = target[idx]: sums[17] = count, sum |p - q|^2, sum p (3), sum q (3), sum p q^T (9, row-major).  sgr_cloud_metrics:
 * out[4] = sum dist_a, #(dist_a < thresh), sum dist_b, #(dist_b < thresh). */
size_t sgr_eval_reduce_bytes(void);
int sgr_icp_accumulate(int32_t n, const float* source, SGR_HOST const float* transform, const int32_t* idx, int32_t n_target,
                       const float* target, double* sums, void* scratch, size_t scratch_bytes, void* stream);
int sgr_cloud_metrics(int32_t na, const float* dist_a, int32_t nb, const float* dist_b, float thresh, double* out, void* scratch,
                      size_t scratch_bytes, void* stream);

/* Culling a mesh to what a set of cameras saw, before it is scored ("Mesh culling"): a frustum test, an
 * occlusion test against depth rendered from the mesh itself, faces of unseen vertices dropped.  Frames come in chunks of at most
 * SGR_CULL_MAX_FRAMES.  Pixel centres sit at integer (u, v); coordinates are snapped to 2^-SGR_CULL_SUBPIXEL_BITS pixel.
 * sgr_cull_project: per (vertex, frame) in fp64, p = w2c (x, y, z, 1), u = fx p.x / p.z + cx, v = fy p.y / p.z + cy;
 *   xy[n,V,2] = llrint(256 u), llrint(256 v) and z[n,V] = (float)p.z.  A vertex with p.z < near, anything non-finite, |u| or |v|
 *   beyond SGR_CULL_GUARD_PIXELS or a p.z that fp32 holds as 0 or inf is invalid: z = 0, xy = 0.
 * sgr_cull_raster: the z-buffer depth[n,H,W] of the triangles from xy and z: +inf where nothing is hit, else the minimum over the
 *   covering triangles of the perspective-correct depth A / (E0/z0 + E1/z1 + E2/z2) (fp32).  Coverage is exact on the snapped
 *   coordinates: pixel (i, j) is covered when the three edge functions at (256 j, 256 i) are >= 0 after orienting the triangle to
 *   doubled area A > 0 (inclusive, both windings; A = 0 is skipped).  The result does not depend on the order of the triangles.  A
 *   triangle with an invalid vertex is not drawn (there is no near-plane clipping) and counted in skipped[n] when not NULL.
 *   H, W <= SGR_CULL_GUARD_PIXELS.  scratch: sgr_cull_raster_bytes(F, n).
 * sgr_cull_visibility: seen[v] += the number of the n frames that see vertex v: z > 0, z <= far, pixel j = (x + 128) >> 8,
 *   i = (y + 128) >> 8 with edge <= j < W - edge and edge <= i < H - edge and, with a depth map (depth[n,H,W], or NULL: frustum
 *   only) d at that pixel, !(d > 0) || z - d <= eps (one fp32 subtraction): zero, negative and NaN depth constrain nothing.
 * sgr_cull_select: a face is kept when all three (SGR_CULL_RULE_ALL) or any (SGR_CULL_RULE_ANY) of its vertices have
 *   seen >= min_views; vertices that no kept face references are dropped; totals[0..1] = kept (vertices, triangles) on the device.
 *   sgr_cull_compact, with the same scratch (sgr_cull_select_bytes(V, F)), writes them in their original order, reindexed, and
 *   vertex_map[V] (new index or -1) when not NULL. */
#define SGR_CULL_MAX_FRAMES 16
#define SGR_CULL_SUBPIXEL_BITS 8
#define SGR_CULL_GUARD_PIXELS 16384
#define SGR_CULL_RULE_ALL 0
#define SGR_CULL_RULE_ANY 1
typedef struct SgrCullFrame {
  double w2c[12];              /* host, row-major 3x4 world -> camera */
  double fx, fy, cx, cy;
} SgrCullFrame;
int sgr_cull_project(int32_t V, const float* vertices, int32_t n, const SgrCullFrame* frames, double near, int32_t* xy, float* z,
                     void* stream);
size_t sgr_cull_raster_bytes(int32_t F, int32_t n);
int sgr_cull_raster(int32_t V, int32_t F, const int32_t* triangles, int32_t n, const int32_t* xy, const float* z, int32_t H, int32_t W,
                    float* depth, int32_t* skipped, void* scratch, size_t scratch_bytes, void* stream);
int sgr_cull_visibility(int32_t V, int32_t n, const int32_t* xy, const float* z, const float* depth, int32_t H, int32_t W, int32_t edge,
                        float far, float eps, int32_t* seen, void* stream);
size_t sgr_cull_select_bytes(int32_t V, int32_t F);
int sgr_cull_select(int32_t V, int32_t F, const int32_t* triangles, const int32_t* seen, int32_t min_views, int32_t rule, void* scratch,
                    size_t scratch_bytes, int32_t* totals, void* stream);
int sgr_cull_compact(int32_t V, int32_t F, const float* vertices, const float* colors, const int32_t* triangles, void* scratch,
                     size_t scratch_bytes, float* out_vertices, float* out_colors, int32_t* out_triangles, int32_t* vertex_map,
                     void* stream);

/* One torch.optim.Adam step (no weight decay, no amsgrad) on a flat parameter slab. step = the value AFTER
 * increment (1 on the first call).  lr may differ per call (update_learning_rate, gaussian_model.py:315-329). */
int sgr_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  float lr, float beta1, float beta2, float eps, int64_t step, void* stream);

/* The same step for MANY SMALL tensors that share lr / betas / eps, in one launch per 48 tensors (block = tensor): the keyframe
 * optimiser of src/mapper.py:1096-1111 holds two one-element exposure parameters (and two 3-vectors of pose deltas) per window
 * keyframe.  Each tensor carries its own step count (AFTER increment). */
typedef struct SgrAdamTensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;                   /* elements (<= 2^20) */
  int64_t step;
} SgrAdamTensor;
int sgr_adam_step_multi(int32_t count, const SgrAdamTensor* tensors, float lr, float beta1, float beta2, float eps, void* stream);

/* Activations of the GaussianModel getters (gaussian_model.py:76-101) in one pass:
 * scales_out = exp(scaling), rot_out = rotation / max(|rotation|, 1e-12), opac_out = sigmoid(opacity). */
int sgr_activate(int64_t n, const float* scaling, const float* rotation, const float* opacity,
                 float* scales_out, float* rot_out, float* opac_out, void* stream);

/* One fused optimiser step of the mapping loop for all Gaussian parameter groups (src/mapper.py:487-489,557):
 * takes the gradients wrt the ACTIVATED rasterizer inputs (as accumulated by sgr_backward), applies the chain rule
 * through exp / sigmoid / normalize, adds the gradient of the isotropy regulariser
 * iso_weight * mean|s - mean(s)| (0 disables it: initialize_map / final_refine), then runs torch.optim.Adam's update
 * (eps as given, no weight decay) in place on the raw parameters and their exp_avg / exp_avg_sq, and zeroes the
 * gradient accumulators for the next iteration.  lr order: xyz, f_dc, opacity, scaling, rotation.
 * f_dc is [N,3] (sh_degree 0 layout [N,1,3]). */
typedef struct SgrAdamGroup {
  float* param;
  float* grad;                 /* accumulator wrt the activated input; zeroed on return */
  float* exp_avg;
  float* exp_avg_sq;
  float lr;
  int32_t skip;                /* != 0: leave param/moments untouched, only zero the accumulator (a group whose
                                  tensor was just replaced has grad None in the reference: Adam skips it) */
  int64_t step;                /* this group's Adam step count AFTER increment (>= 1 unless skip) */
} SgrAdamGroup;
int sgr_gaussian_adam_step(int64_t n, const SgrAdamGroup groups[5], float beta1, float beta2, float eps,
                           float iso_weight, void* stream);

/* The same step for a SLICE of the optimiser (multi-GPU ZeRO-1, SURVEY.md 8e: gradients reduce-scattered over the ranks,
 * every rank steps the rows it owns, parameters all-gathered afterwards): group k is stepped for the Gaussians
 * row0[k] <= i < row1[k] only; its four pointers still address ROW 0 of the (virtual) full arrays and are only
 * dereferenced inside that range, so `grad` may point into a rank-local shard buffer.  The isotropy term is normalised by
 * n_total (the whole map).  No activations are written: the caller re-activates after its all-gather. */
int sgr_gaussian_adam_shard(int64_t n_total, const SgrAdamGroup groups[5], SGR_HOST const int64_t row0[5],
                            SGR_HOST const int64_t row1[5], float beta1, float beta2, float eps, float iso_weight, void* stream);

/* One mapping-loop view: render, mapping loss and its gradient, backward (src/mapper.py:426-456 for one viewpoint).
 * sgr_map_views runs the sequence  sgr_forward(async) -> sgr_mapping_loss -> sgr_backward  for `num_views` views
 * that share the Gaussian inputs `in` and the gradient sinks `grads` (use accumulate = 1) with ONE host call, so the
 * host cost of a mapping iteration is the kernel launches only. */
typedef struct SgrMapView {
  SgrSettings settings;
  SgrOutputs out;              /* color / depth / opacity may ALL be NULL when only loss + gradients are wanted;
                                  n_touched may be NULL (not counted) */
  SgrWorkspace ws;
  const float* gt_image;       /* [3,H,W] */
  const float* gt_depth;       /* [H,W]   */
  const float* exposure_a;     /* [1] or NULL */
  const float* exposure_b;     /* [1] or NULL */
  float* loss;                 /* [1] */
  float* dL_dimage;            /* [3,H,W] scratch for this view.  Uniform batches (the normal case) pass the pixel
                                  gradients of the L1 loss from the compositing epilogue to the backward as ONE code
                                  byte per pixel in its first H*W bytes (2 bits per value: 0, +, -); only the
                                  one-view-at-a-time path of heterogeneous batches leaves float gradients here */
  float* dL_ddepth;            /* [1,H,W] scratch (same remark) */
  float* dL_dexposure;         /* [2] = (d/da, d/db) or NULL */
  float* dL_dtau;              /* [6] or NULL */
  void* loss_scratch;
  size_t loss_scratch_bytes;
} SgrMapView;
int sgr_map_views(int32_t num_views, const SgrMapView* views, const SgrInputs* in, const SgrGradInputs* grads,
                  float alpha, float rgb_boundary_threshold, int32_t forward_only, void* stream);

/* One whole mapping iteration (src/mapper.py:414-568 without densification) in ONE host call:
 *   sgr_activate -> sgr_map_views -> sgr_gaussian_adam_step -> sgr_masked_adam (exposures).
 * Any stage is skipped when its pointer block is NULL / its count is 0.
 * An optimiser-only step (num_views == 0 with adam_groups: the second half of a multi-GPU iteration, after the gradient
 * all-reduce) does not activate first: its Adam pass writes scales_out / rot_out / opac_out of the UPDATED parameters
 * (for the non-NULL ones of scaling / rotation / opacity), so the next views step can skip sgr_activate. */
typedef struct SgrMapStep {
  int64_t num_gaussians;
  const float* scaling;        /* raw parameters for sgr_activate (NULL = skip activation) */
  const float* rotation;
  const float* opacity;
  float* scales_out;
  float* rot_out;
  float* opac_out;
  int32_t num_views;
  int32_t forward_only;
  const SgrMapView* views;
  const SgrInputs* in;
  const SgrGradInputs* grads;
  float alpha;
  float rgb_boundary_threshold;
  const SgrAdamGroup* adam_groups;   /* [5] or NULL (no optimiser step this iteration) */
  float beta1, beta2, eps, iso_weight;
  int32_t exp_rows;            /* rows of the exposure slab to consider (0 = skip) */
  int32_t exp_row_width;
  float* exp_param;
  const float* exp_grad;
  float* exp_avg;
  float* exp_avg_sq;
  int32_t* exp_step;
  const int32_t* exp_active;
  float exp_lr, exp_beta1, exp_beta2, exp_eps;
  int32_t grads_clean;         /* > 0: the gradient sinks are known to be all-zero on entry (as every Adam step leaves
                                  them); the fused gather+Adam pass then never touches them.  0: unknown.
                                  -1: keep gather and Adam as separate passes (verification)
                                  -2 (with adam_groups == NULL): no optimiser step, but the gather pass of the fused form
                                  ADDS the views' gradient sums to the sinks and carries the loss sums and the exposure
                                  step -- the first half of a multi-GPU iteration (an all-reduce of the sinks and an
                                  optimiser-only step follow)
                                  -3: like -2, but the pass STORES the sums (zeros for Gaussians no view of the batch sees)
                                  into the sinks of all num_gaussians rows instead of adding: the sinks need not be zeroed
                                  between two iterations (one 56 B x N memset per exchange less).  A batch that cannot take the
                                  fused gather pass (a view asks for dL_dtau, heterogeneous views, > 16 views) has its sinks
                                  zeroed by the library first and is then accumulated: the sinks hold this call's sums on
                                  every path */
} SgrMapStep;
int sgr_map_step(const SgrMapStep* step, void* stream);

/* A run of `num_iters` REGULAR mapping iterations (no densification / opacity reset between them) enqueued by one host
 * call: what `for _ in range(iters)` of Mapper.map (src/mapper.py:414-568) or Mapper.final_refine (:656-708) does
 * between two map-surgery points.  Iteration k renders window[0..num_window) plus pool[picks[k*picks_per_iter + j]]
 * (the reference's random keyframes, drawn by the caller so that its RNG stream is unchanged), steps Adam with
 * adam_groups[0].lr = lr0[k] (the xyz schedule, src/mapper.py:564) and bumps every non-skipped group's step counter;
 * `adam_groups` is updated in place so that the caller can read the counters back.
 * pool_exp_row (optional): exposure-slab row of each pool entry (-1 = none); when given, iteration k steps only the
 * row of its first pick (final_refine: torch's Adam skips parameters without a gradient) -- step.exp_* then point at
 * row 0 of the slab and step.exp_active at an all-ones array. */
typedef struct SgrMapRun {
  SgrMapStep step;              /* template of one iteration; its views / num_views / adam_groups are ignored */
  int32_t num_iters;
  int32_t num_window;
  const SgrMapView* window;
  int32_t pool_size;
  int32_t picks_per_iter;
  const SgrMapView* pool;
  SGR_HOST const int32_t* picks;         /* host, [num_iters * picks_per_iter] */
  SGR_HOST const float* lr0;             /* host, [num_iters] or NULL (keep adam_groups[0].lr) */
  SgrAdamGroup* adam_groups;    /* host, [5] or NULL */
  SGR_HOST const int32_t* pool_exp_row;  /* host, [pool_size] or NULL */
  int32_t n_touched_last_only;  /* != 0: n_touched is only produced by the last iteration (nobody can observe the others) */
  const SgrWorkspace* pick_ws;  /* host, [picks_per_iter] or NULL.  Non-NULL: pick j of every iteration renders in pick_ws[j]
                                   instead of its pool entry's own workspace -- a map holds hundreds of keyframes, an iteration
                                   touches picks_per_iter of them (src/mapper.py:458-485), and a workspace is ~300 MB.  The
                                   pool entries' `ws` are then ignored. */
} SgrMapRun;
int sgr_map_run(const SgrMapRun* run, void* stream);

/* The mapping loss with the SSIM term (`ssim_loss: True`, thirdparty/monogs/utils/slam_utils.py:89-105; lambda = opt_params.lambda_dssim):
 *   L = alpha mean_{c,p}[(1 - lambda) |m (x - gt)| + lambda (1 - ssim(x, gt))] + (1 - alpha) mean_p |md (depth - gt_depth)|
 * with x = exp(a) image + b (image itself with NULL exposures), SSIM on the raw x (no clamp, no mask).  Per batch of views: one
 * launch pair (moments and derivative maps; blurred maps -> float dL/dimage, dL/ddepth and the partial sums), then the usual
 * fixed-order final sum.  No float atomics: bitwise reproducible.
 * SgrSsimTerm.arena (sgr_ssim_term_bytes(max_views, H, W), device) holds the derivative maps of up to max_views views at a time
 * and the partial sums of one view; its contents need not survive between calls.
 * sgr_mapping_loss_ssim: the standalone loss of one [3,H,W] view, gradients times `upstream` (like sgr_mapping_loss).
 * sgr_map_step_ssim / sgr_map_run_ssim: sgr_map_step / sgr_map_run with this loss.  Every view must render its image, depth and
 * opacity (SgrOutputs without NULLs), its loss_scratch must hold 3 * ceil(H/16) * ceil(W/32) records of 16 B, and dL_dimage
 * receives the FLOAT gradient [3,H,W].  term == NULL is exactly sgr_map_step / sgr_map_run. */
typedef struct SgrSsimTerm {
  float lambda_dssim;
  int32_t max_views;            /* views whose maps the arena holds at once (a batch runs in groups of this many) */
  void* arena;
  size_t arena_bytes;
} SgrSsimTerm;
size_t sgr_ssim_term_bytes(int32_t max_views, int32_t H, int32_t W);
int sgr_mapping_loss_ssim(int32_t H, int32_t W, const float* image, const float* depth, const float* gt_image,
                          const float* gt_depth, const float* exposure_a, const float* exposure_b, float alpha,
                          float rgb_boundary_threshold, float upstream, const SgrSsimTerm* term, float* loss,
                          float* dL_dimage, float* dL_ddepth, float* dL_dexp_a, float* dL_dexp_b, void* stream);
int sgr_map_step_ssim(const SgrMapStep* step, const SgrSsimTerm* term, void* stream);
int sgr_map_run_ssim(const SgrMapRun* run, const SgrSsimTerm* term, void* stream);

/* Adam on a small slab with a per-row switch: row r (width `row_width`) is updated iff active[r] != 0, using its own
 * step counter step[r] (incremented in place).  The exposure parameters of the keyframe optimiser
 * (src/mapper.py:1096-1111: lr 0.01, default eps 1e-8) live in such a slab. */
int sgr_masked_adam(int32_t rows, int32_t row_width, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    int32_t* step, const int32_t* active, float lr, float beta1, float beta2, float eps, void* stream);

/* Mapper.update_mapping_points (src/mapper.py:154-255) as ONE pass: the Gaussians anchored to keyframe `frame_idx`
 * (unique_kfIDs == frame_idx) are depth-rescaled along the old camera's ray (unless rigid), moved by `transform`
 * (= inv(inv(w2c_old) @ w2c_new), host, row-major) and rotated by its quaternion; every rotation leaves normalised (the
 * reference writes the activated rotations back).  In place on the raw parameter tensors; resetting the Adam moments of
 * the three tensors (replace_tensor_to_optimizer, gaussian_model.py:488-501) stays with the caller. */
typedef struct SgrDeformFrame {
  int32_t frame_idx;
  int32_t rigid;               /* != 0: pose change only (no depth rescale, depth maps unused) */
  float w2c_old[16];           /* host, row-major 4x4 */
  float c2w_old[16];           /* inverse of w2c_old */
  float transform[16];
  float quat_wxyz[4];          /* rotation part of `transform` */
  float intrinsics[9];         /* row-major K */
  int32_t height, width;
  const float* depth_new;      /* device [H,W] */
  const float* depth_old;      /* device [H,W] */
} SgrDeformFrame;
int sgr_deform_points(int64_t n, const int32_t* unique_kfIDs, const SgrDeformFrame* frame, float* xyz, float* rotation,
                      float* scaling, void* stream);

/* Densify / prune compaction (gaussian_model.py:519-557 prune_points, _prune_optimizer; :690-719 the row selects of
 * densify_and_clone / densify_and_split): sgr_keep_list turns a byte mask into the ascending list of kept row indices
 * (count written to a device int64, no host sync); sgr_gather_rows copies rows src_rows[k] -> k for up to any number of
 * tensors (parameters, Adam moments, statistics, keyframe ids ...) in one launch per 32 tensors. */
typedef struct SgrRowTensor {
  const void* in;              /* [n_in, row_bytes] */
  void* out;                   /* [m, row_bytes], must not alias `in` */
  int32_t row_bytes;           /* multiple of 4 */
} SgrRowTensor;
size_t sgr_compact_scratch_bytes(int64_t n);
int sgr_keep_list(int64_t n, const uint8_t* keep, int32_t* src_rows, int64_t* count_device, void* scratch, size_t scratch_bytes,
                  void* stream);
int sgr_gather_rows(int64_t m, const int32_t* src_rows, int32_t num_tensors, const SgrRowTensor* tensors, void* stream);

/* simple_knn distCUDA2: mean squared distance to the 3 nearest neighbours (self excluded). */
size_t sknn_scratch_bytes(int32_t n);
int sknn_dist2(const float* xyz, int32_t n, float* mean_dist2, void* scratch, size_t scratch_bytes, void* stream);

/* Dense bundle adjustment and frame geometry of the tracker (droid_backends).  Poses are [N,7] (t, q xyzw) world -> camera,
 * disparity maps [N,ht,wd], intrinsics [4] (fx, fy, cx, cy), edge lists int64.  Edges whose frames lie outside both poses and
 * disps take part in nothing (ba) or give NaN (frame_distance, projmap).
 * sgr_dba_ba runs `iterations` Gauss-Newton steps in place on poses[t0, t1) and on the disparities of the K frames
 * kx = sorted unique(ii U [t0, t1)), with no host synchronisation.  dx is [t1-t0, 6] and dz [K, ht*wd] of the last step.  The
 * window is limited to 512 frames (SGR_ERR_CAPACITY beyond).  A reduced system that is not positive definite gives dx = 0 and the
 * step goes on.  When K differs from the number of distinct depth frames found on the device, nothing is updated and dx, dz
 * are NaN.  motion_only solves the pose blocks alone (dz untouched, may be NULL); depth_only leaves the poses as they are. */
#define SGR_DBA_MAX_WINDOW 512              /* sgr_dba_ba: frames t1 - t0 of the window */
typedef struct SgrDbaProblem {
  float* poses;                /* [num_poses, 7], updated */
  int32_t num_poses;
  float* disps;                /* [num_frames, ht, wd], updated */
  int32_t num_frames, ht, wd;
  const float* intrinsics;     /* [4] */
  const float* disps_sens;     /* [num_frames, ht, wd]: sensor disparity, > 0 where measured */
  const float* targets;        /* [num_edges, 2, ht, wd] */
  const float* weights;        /* [num_edges, 2, ht, wd] */
  const float* eta;            /* [num_depth, ht, wd] */
  const int64_t* ii;           /* [num_edges] */
  const int64_t* jj;           /* [num_edges] */
  int32_t num_edges, num_depth;
  int32_t t0, t1, iterations;
  float lm, ep;
  int32_t motion_only, depth_only;
  float* dx;                   /* [t1-t0, 6] out */
  float* dz;                   /* [num_depth, ht*wd] out */
} SgrDbaProblem;
size_t sgr_dba_scratch_bytes(int32_t num_frames, int32_t num_edges, int32_t num_depth, int32_t window, int32_t ht, int32_t wd);
int sgr_dba_ba(const SgrDbaProblem* problem, void* scratch, size_t scratch_bytes, void* stream);
/* dist [num_edges]; beta weighs the full flow against the translation-only flow */
int sgr_dba_frame_distance(const float* poses, int32_t num_poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd,
                           const float* intrinsics, const int64_t* ii, const int64_t* jj, int32_t num_edges, float beta, float* dist,
                           void* stream);
/* coords [num_edges, ht, wd, 3] (third channel 0), valid [num_edges, ht, wd, 1] */
int sgr_dba_projmap(const float* poses, int32_t num_poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd,
                    const float* intrinsics, const int64_t* ii, const int64_t* jj, int32_t num_edges, float* coords, float* valid,
                    void* stream);
/* points [num_frames, ht, wd, 3]; poses has at least num_frames rows */
int sgr_dba_iproj(const float* poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const float* intrinsics,
                  float* points, void* stream);
/* counter [num, ht, wd]: neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 of each ix = inds[b] that agree within thresh[b] */
int sgr_dba_depth_filter(const float* poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const float* intrinsics,
                         const int64_t* inds, int32_t num, const float* thresh, float* counter, void* stream);

/* DSPO stage 2 of the tracker ("depth_scale"): disparities, and one scale and shift per frame for the mono-depth prior, with the
 * poses fixed.  Conventions are those of sgr_dba_*; the algorithm is stated in DESIGN.md section 3, "DSPO stage 2".
 * sgr_dspo_align: for each of `num` frames of `pixels` pixels, the scale s and shift q that minimise sum w (s prediction + q - target)^2
 * and the mean error sum w |s prediction + q - target| / sum w, as out [num, 3] = (s, q, error).  Sums, the 2 x 2 solve and the error
 * are fp64, rounded once; a zero determinant gives what IEEE arithmetic gives (inf / NaN).  weights: NULL with SGR_DSPO_WEIGHTS_NONE
 * (all ones), float with _F32, bytes (non-zero = 1) with _U8.
 * sgr_dspo_ba runs `iterations` Gauss-Newton steps in place on the disparities of the M depth frames kx = sorted unique(ii) and on
 * their scales and shifts, with no host synchronisation.  edge_keep (may be NULL = all) masks edges out; a depth frame none of whose
 * edges is kept is left untouched and its dwq and dz rows are zero.  dwq is [M, 2] and dz [M, ht*wd] of the last step.  A frame
 * whose reduced 2 x 2 system is not positive definite gets dwq = 0 (that frame alone).  When M differs from the number of distinct
 * ii found on the device, nothing is updated and dwq, dz are NaN. */
#define SGR_DSPO_WEIGHTS_NONE 0
#define SGR_DSPO_WEIGHTS_F32 1
#define SGR_DSPO_WEIGHTS_U8 2
typedef struct SgrDspoProblem {
  const float* poses;              /* [num_poses, 7], not changed */
  int32_t num_poses;
  float* disps;                    /* [num_frames, ht, wd], updated */
  int32_t num_frames, ht, wd;
  const float* intrinsics;         /* [4] */
  const float* mono_disps;         /* [num_frames, ht, wd]: mono-depth prior as disparity, < 1e-6 where there is none */
  const uint8_t* valid_depth_mask; /* [num_frames, ht, wd]: non-zero where the disparity passed the two-view consistency check */
  float* scales;                   /* [num_frames], updated */
  float* shifts;                   /* [num_frames], updated */
  const float* targets;            /* [num_edges, ht, wd, 2]: (x, y) per pixel */
  const float* weights;            /* [num_edges, ht, wd, 2] */
  const float* eta;                /* [num_depth, ht, wd] */
  const int64_t* ii;               /* [num_edges] */
  const int64_t* jj;               /* [num_edges] */
  const uint8_t* edge_keep;        /* [num_edges] or NULL */
  int32_t num_edges, num_depth;
  int32_t ignore_frames, iterations;
  float lm, ep, alpha;
  float* dwq;                      /* [num_depth, 2] out */
  float* dz;                       /* [num_depth, ht*wd] out */
} SgrDspoProblem;
int sgr_dspo_align(const float* prediction, const float* target, const void* weights, int32_t weights_kind, int32_t num, int32_t pixels,
                   float* out, void* stream);
size_t sgr_dspo_scratch_bytes(int32_t num_frames, int32_t num_edges, int32_t num_depth, int32_t ht, int32_t wd);
int sgr_dspo_ba(const SgrDspoProblem* problem, void* scratch, size_t scratch_bytes, void* stream);

/* The keyframe store of the tracker (DepthVideo, thirdparty/glorie_slam/depth_video.py): convex upsampling of the disparity maps
 * (:154-158) and the two-view consistency mask (update_valid_depth_mask, :340-375).  Stated in DESIGN.md section 3, "Depth video".
 * inds [num] int64 are distinct frame indices; an index outside [0, num_frames) makes its slot a no-op (its thresh is NaN).
 * num <= 65535.  Everything is stream-ordered, allocates nothing and is bitwise reproducible.
 * sgr_video_cvx_upsample: disps [num_frames, ht, wd], mask [num, 576, ht, wd] of logits (fp32 or fp16), channel k*64 + dy*8 + dx with
 * k = 3*(ny+1) + (nx+1); disps_up [num_frames, 8*ht, 8*wd] (16-byte aligned), of which only the frames named in inds are written:
 * out[8y+dy, 8x+dx] = sum_k softmax_k(mask[k*64+dy*8+dx, y, x]) * d[y+ny, x+nx], d = 0 outside the map, the softmax in fp32.
 * sgr_video_depth_thresh: thresh[b] = rel * mean(1.0f / disp) over frame inds[b]; the sum is fp64, rounded once.
 * sgr_video_mask_from_counts: counts [num, ht, wd] as sgr_dba_depth_filter writes them; candidates are the pixels with
 * counts >= visible_num whose depth 1.0f / disp is not NaN; mask_out [num_frames, ht, wd] bytes (only the frames of inds) =
 * candidate && depth < 3.0f * (lower median of the candidates' depths), all zero when there is no candidate.
 * sgr_video_valid_mask: the chain thresholds -> sgr_dba_depth_filter -> mask; poses cover num_frames.
 * scratch: sgr_video_scratch_bytes(num, ht, wd) bytes, 16-byte aligned (0 = unsupported sizes). */
#define SGR_VIDEO_MASK_F32 0
#define SGR_VIDEO_MASK_F16 1
#define SGR_VIDEO_MAX_FRAMES 65535          /* sgr_video_*: `num` of one call */
int sgr_video_cvx_upsample(const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const int64_t* inds, int32_t num,
                           const void* mask, int32_t mask_kind, float* disps_up, void* stream);
int sgr_video_depth_thresh(const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const int64_t* inds, int32_t num, float rel,
                           float* thresh, void* stream);
size_t sgr_video_scratch_bytes(int32_t num, int32_t ht, int32_t wd);
int sgr_video_mask_from_counts(const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const int64_t* inds, int32_t num,
                               const float* counts, int32_t visible_num, uint8_t* mask_out, void* scratch, size_t scratch_bytes,
                               void* stream);
int sgr_video_valid_mask(const float* poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const float* intrinsics,
                         const int64_t* inds, int32_t num, float rel, int32_t visible_num, uint8_t* mask_out, void* scratch,
                         size_t scratch_bytes, void* stream);

/* Keyframe depth fusion: the depth map the mapper seeds and supervises with (Mapper.get_w2c_and_depth, src/mapper.py:258-301).  Stated
 * in DESIGN.md section 3, "Keyframe depth fusion".  Everything is stream-ordered, allocates nothing, synchronises nothing and is
 * bitwise reproducible (fixed-order sums, no floating-point atomics).  ht, wd >= 1, ht * wd < 2^28, num <= 65535.
 * sgr_fuse_prepare: for each of `num` mono-depth maps [num, ht, wd] (what depends on the mono map alone; once per keyframe):
 *   mean = sum / (ht wd), the sum in fp64 in the order of sgr_video_depth_thresh, rounded once; pixels > 4 mean become 0;
 *   eroded [num, ht, wd] bytes = 1 iff every pixel within chessboard distance 5 inside the image is > 0 (outside counts as > 0);
 *   mono_filled [num, ht, wd] = the map where eroded == 1; the others are filled in passes k = 1, 2, ...: with K the set known
 *   before pass k (K = eroded at first), every pixel outside K with an 8-neighbour in K gets sum w v / sum w over the pixels of K in
 *   its 7 x 7 window, w = 1 / (dx^2 + dy^2), fp32, row-major; the pixels filled in a pass join K after it.  A map without a known
 *   pixel stays zero.
 * sgr_fuse_depth: for each of `num` frames f = inds[b] (int64, any order, repeats allowed), read in place from disps_up,
 *   valid_depth_mask (bytes, non-zero = valid), mono_filled and eroded, all [num_frames, ht, wd]:
 *   count = sum valid; invalid[b] = count < min_valid; (s, q) = the scale and shift of sgr_dspo_align with prediction mono_filled,
 *   target 1.0f / disp and weight eroded & valid (sums and the 2 x 2 solve in fp64, rounded once; pixels of weight zero contribute
 *   nothing; a zero determinant gives IEEE inf / NaN); depth [num, ht, wd] = valid ? 1.0f / disp : s * mono_filled + q, a rounded
 *   multiply followed by a rounded add; scale[b] = s, shift[b] = q.  An invalid frame gets depth = valid ? 1.0f / disp : 0 and its
 *   scale and shift are left unwritten.  A slot whose index lies outside [0, num_frames) gets invalid = 1 and a depth of zeros.  A frame
 *   gives the same bits alone and in any batch.
 * scratch: sgr_fuse_scratch_bytes(num, ht, wd) bytes, 16-byte aligned, serves either call (0 = unsupported sizes). */
#define SGR_FUSE_MAX_FRAMES 65535           /* sgr_fuse_*: `num` of one call */
size_t sgr_fuse_scratch_bytes(int32_t num, int32_t ht, int32_t wd);
int sgr_fuse_prepare(const float* mono, int32_t num, int32_t ht, int32_t wd, float* mono_filled, uint8_t* eroded, void* scratch,
                     size_t scratch_bytes, void* stream);
int sgr_fuse_depth(const float* disps_up, const uint8_t* valid_depth_mask, const float* mono_filled, const uint8_t* eroded,
                   int32_t num_frames, int32_t ht, int32_t wd, const int64_t* inds, int32_t num, int32_t min_valid, float* depth,
                   float* scale, float* shift, uint8_t* invalid, void* scratch, size_t scratch_bytes, void* stream);

/* Correlation lookups of the tracker's update operator (droid_backends).  rd = 2*radius + 1; outputs run over the x offset first,
 * then the y offset.  A sample is bilinear with zero padding; a pixel whose floor(x0) or floor(y0) is not finite or lies outside
 * [-(radius+2), w2+radius+1] resp. [-(radius+2), h2+radius+1] reads nothing and gives zeros (no coordinate value reaches memory).
 * Sums are kept in fp32 and rounded once; every output element is written exactly once (no zero-fill by the caller), except
 * fmap2_grad, which must be ZERO on entry and is accumulated with fp32 atomic adds (the only output that is not bitwise
 * reproducible).  batch*h1*w1 (times num for the alt pair) and h2*w2 must each fit int32 (SGR_ERR_CAPACITY); radius <= 1023.
 * corr_index: volume, volume_grad [batch,h1,w1,h2,w2] and corr, corr_grad [batch,rd,rd,h1,w1] in `dtype`; coords [batch,2,h1,w1]
 * fp32 (x, y planes).  corr_alt: fmap1 [batch,h1,w1,channels], fmap2 [batch,h2,w2,channels], coords [batch,num,h1,w1,2] (x, y),
 * corr, corr_grad [batch,num,rd*rd,h1,w1], all fp32; channels is a positive multiple of 4. */
#define SGR_CORR_F32 0
#define SGR_CORR_F16 1
#define SGR_CORR_MAX_RADIUS 1023            /* sgr_corr_index_*, sgr_corr_alt_forward / _backward */
#define SGR_CORR_PYRAMID_MAX_RADIUS 4       /* the pyramid lookups: sgr_corr_alt_pyramid_forward, sgr_corr_index_pyramid_forward */
#define SGR_CORR_PYRAMID_MAX_LEVELS 4       /* num_levels of the pyramid calls (the level0 .. level3 arguments) */
#define SGR_CORR_VOLUME_CHANNEL_STEP 32     /* sgr_corr_volume_pyramid: channels is a positive multiple of this ... */
#define SGR_CORR_VOLUME_MAX_CHANNELS 1024   /* ... up to this */
#define SGR_CORR_VOLUME_MAX_EDGES 65535     /* sgr_corr_volume_pyramid: edges of one call */
int sgr_corr_index_forward(const void* volume, const float* coords, void* corr, int32_t dtype, int32_t batch, int32_t h1, int32_t w1,
                           int32_t h2, int32_t w2, int32_t radius, void* stream);
int sgr_corr_index_backward(const float* coords, const void* corr_grad, void* volume_grad, int32_t dtype, int32_t batch, int32_t h1,
                            int32_t w1, int32_t h2, int32_t w2, int32_t radius, void* stream);
int sgr_corr_alt_forward(const float* fmap1, const float* fmap2, const float* coords, float* corr, int32_t batch, int32_t num, int32_t h1,
                         int32_t w1, int32_t h2, int32_t w2, int32_t channels, int32_t radius, void* stream);
int sgr_corr_alt_backward(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad, float* fmap1_grad,
                          float* fmap2_grad, int32_t batch, int32_t num, int32_t h1, int32_t w1, int32_t h2, int32_t w2, int32_t channels,
                          int32_t radius, void* stream);
/* corr_alt_forward at every level of a feature pyramid in one launch, the two frames of an edge read through their indices.
 * level_l [frames, h >> l, w >> l, channels], channels last, fp16 or fp32 by `dtype`, l < num_levels <= 4 (the others are ignored; a
 * level without pixels may be NULL); src, dst [edges] int64; coords [edges,h,w,2] fp32 (x, y) at the scale of level 0;
 * corr [edges, num_levels*rd*rd, h, w] fp32: level l fills the channels [l*rd*rd, (l+1)*rd*rd), x offset first, and is
 * corr_alt_forward(level_0[src], level_l[dst], coords * 2^-l).  The window rule above applies per level; a level without pixels
 * and an edge whose src or dst lies outside [0, frames) give zeros and read nothing.  Products and sums are fp32 (fp16 is widened
 * exactly), one fixed chain per dot product: an edge gives the same bits alone and inside any batch.  edges*h*w must fit int32,
 * channels is a positive multiple of 4, radius <= 4 (SGR_ERR_CAPACITY beyond). */
int sgr_corr_alt_pyramid_forward(const void* level0, const void* level1, const void* level2, const void* level3, const int64_t* src,
                                 const int64_t* dst, const float* coords, float* corr, int32_t dtype, int32_t frames, int32_t edges,
                                 int32_t h, int32_t w, int32_t channels, int32_t radius, int32_t num_levels, void* stream);
/* The all-pairs correlation volumes of a batch of edges, written into the slots of a store, and the lookup that reads them there.
 * Stated in DESIGN.md section 3, "Fused correlation volume".  Both calls are stream-ordered, allocate nothing, synchronise nothing,
 * use no atomics and are bitwise reproducible; indices into the levels are 64-bit.
 * level_l [capacity, h, w, h >> l, w >> l] fp16, l < num_levels <= 4 (the others are ignored; a level without pixels may be NULL).
 * sgr_corr_volume_pyramid: maps [planes, channels, h, w] fp16, channels first; src, dst [edges] int64 plane indices; slots [edges]
 *   int64.  Level 0 of slot slots[e] is V0[p1, p2] = (1/16) sum_c maps[src[e], c, p1] maps[dst[e], c, p2], the products exact in
 *   fp32, the sum in fp32 by mfma_f32_16x16x32_f16 in an order the tile fixes.  Level l is the mean of the fp32 V0 over the aligned
 *   2^l x 2^l block of p2, formed by successive 2 x 2 sums ((a + b) + (c + d), rows first) each scaled by 0.25, for block rows
 *   < h >> l and block columns < w >> l (an odd last row or column is dropped).  Each level is rounded to fp16 once, on its store
 *   (overflow gives inf).  An edge whose src or dst lies outside [0, planes) (compared in 64 bits) gets zeros in every element of its
 *   slot at every level and reads nothing; an edge whose slot lies outside [0, capacity) writes nothing; two edges of one call with
 *   the same slot are undefined.  An edge gives the same bits alone, in any batch and in any slot.  h, w >= 1; h*w must fit int32
 *   and edges <= 65535; channels must be a positive multiple of 32 up to 1024 (SGR_ERR_CAPACITY otherwise).  edges = 0 is a no-op.
 * sgr_corr_index_pyramid_forward: coords [edges, h, w, 2] fp32 (x, y) at the scale of level 0; corr [edges, num_levels*rd*rd, h, w]
 *   fp16: the channels [l*rd*rd, (l+1)*rd*rd) are bit for bit sgr_corr_index_forward(level_l[slots], coords * 2^-l, radius) (the same
 *   window rule, walk and single rounding).  A level without pixels and an edge whose slot lies outside [0, capacity) give zeros;
 *   every output element is written.  edges >= 1, edges*h*w must fit int32, radius <= 4 (SGR_ERR_CAPACITY beyond). */
int sgr_corr_volume_pyramid(const void* maps, const int64_t* src, const int64_t* dst, const int64_t* slots, void* level0, void* level1,
                            void* level2, void* level3, int32_t planes, int32_t edges, int32_t capacity, int32_t channels, int32_t h,
                            int32_t w, int32_t num_levels, void* stream);
int sgr_corr_index_pyramid_forward(const void* level0, const void* level1, const void* level2, const void* level3, const int64_t* slots,
                                   const float* coords, void* corr, int32_t capacity, int32_t edges, int32_t h, int32_t w, int32_t radius,
                                   int32_t num_levels, void* stream);

/* The factor graph of the tracker (FactorGraph, thirdparty/glorie_slam/factor_graph.py).  Stated in DESIGN.md section 3, "Factor
 * graph".  Everything is stream-ordered, allocates nothing, synchronises nothing and is bitwise reproducible.
 * sgr_graph_reproject: projective_transform (geom/projective_ops.py:110-139) with PER-FRAME intrinsics [num_frames,4] (fx, fy, cx, cy)
 * and, when target [E,ht,wd,2] is given, the motion features of FactorGraph.update.  For edge e = (i, j) and pixel (x, y) with
 * disparity d of frame i: X0 = ((x-cx_i)/fx_i, (y-cy_i)/fy_i, 1, d), G = G_j G_i^-1 (i == j: t = (-0.1, 0, 0), q = identity),
 * X1 = R X0.xyz + t d, Z = X1.z < 0.1 ? 1 : X1.z, coords [E,ht,wd,2] = (fx_j X1.x/Z + cx_j, fy_j X1.y/Z + cy_j), valid [E,ht,wd,1] =
 * X1.z > 0.2, motn [E,4,ht,wd] = clamp((coords - (x, y), target - coords), -64, 64).  target and motn are both given or both NULL.
 * An edge with an index outside [0, min(num_poses, num_frames)) gets zeros in every output and reads nothing.  E <= 65535.
 * sgr_graph_select_proximity / _backend: the greedy edge selection of add_proximity_factors (:337-397) and
 * add_backend_proximity_factors (:400-477) over the distance matrix d (read only), rows i - t0 (t_start_loop), columns j - t1
 * (t_start), both ending at frame t (t_end); at most 512 x 512.  Entries are visited in ascending distance, equal distances in
 * ascending flat index.  es [cap,2] int64 receives the pairs in the order of the sequential rule, counts[0] their number and
 * counts[1] the number of loop pairs among them (loop != 0); nothing is written past cap.  ii_old, jj_old [num_old]: the existing
 * edges, of any value.  thresh is finite, 0 <= nms <= 512, 0 <= rad.
 * scratch: sgr_graph_select_scratch_bytes(rows, cols) bytes, 16-byte aligned (0 = unsupported sizes). */
#define SGR_GRAPH_MAX_EDGES 65535           /* sgr_graph_reproject: edges of one call */
#define SGR_GRAPH_MAX_SIDE 512              /* sgr_graph_select_*: rows and columns of the distance window, and nms */
int sgr_graph_reproject(const float* poses, int32_t num_poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd,
                        const float* intrinsics, const int64_t* ii, const int64_t* jj, int32_t num_edges, const float* target,
                        float* coords, float* valid, float* motn, void* stream);
size_t sgr_graph_select_scratch_bytes(int32_t rows, int32_t cols);
int sgr_graph_select_proximity(const float* d, int32_t t0, int32_t t1, int32_t t, const int64_t* ii_old, const int64_t* jj_old,
                               int32_t num_old, int32_t rad, int32_t nms, float thresh, int32_t max_factors, int64_t* es, int32_t cap,
                               int32_t* counts, void* scratch, size_t scratch_bytes, void* stream);
int sgr_graph_select_backend(const float* d, int32_t t_start, int32_t t_end, int32_t t_start_loop, int32_t loop, int32_t nms,
                             int32_t radius, float thresh, int32_t max_factors, int64_t* es, int32_t cap, int32_t* counts,
                             void* scratch, size_t scratch_bytes, void* stream);

/* The update operator of the tracker (UpdateModule, thirdparty/glorie_slam/modules/droid_net/droid_net.py:83-153), inference only.
 * Stated in DESIGN.md section 3, "Update operator".  Everything is stream-ordered, allocates nothing, synchronises nothing and is
 * bitwise reproducible.  Activations are channels-last fp16: [pixel m = (edge, y, x)][channel], a row stride counted in halfs that is
 * a multiple of 8, a 16-byte aligned base.  E*h*w must fit int32.
 * sgr_update_pack: src [E,C,h,w] with element strides (a NULL data pointer stands for zeros) -> dst[m * dst_stride + c], c < c_pad,
 * the channels C <= c < c_pad zero; c_pad is a multiple of 8.
 * sgr_update_conv: out[m][n] = act(bias[n] + eadd[edge][n] + sum_{tap,c} W[n][tap][c] x[m + tap][c]), zero padding, stride 1, square
 * kernels of size 1, 3 or 7.  Input channel c < split comes from src0[c], the others from src1[c - split] (src1 NULL: all from src0); cin
 * is the padded channel count, a multiple of 8.  weight is fp16 [round_up(cout, 64)][round_up(ksize^2 * cin, 32)], k = tap * cin + c,
 * padding zero; bias fp32 [round_up(cout, 64)].  fp16 products, fp32 sums (mfma_f32_16x16x32_f16).  Epilogues on the fp32 sum v:
 * NONE, RELU, SIGMOID, TANH; ETA = 0.01 softplus(v); GATE = sigmoid(v) * aux0[m][n]; ZR (cout = 256): n < 128 writes sigmoid(v) to
 * out[m][n], n >= 128 writes sigmoid(v) * aux0[m][n-128] to out2[m][n-128]; BLEND: (1 - z) * aux0 + z * tanh(v) with z = aux1[m][n],
 * written to out and, as NCHW fp16, to out2.  aux0, aux1 and out2 of ZR are channels-last fp16.
 * sgr_update_forward: the whole operator.  layer[] order: corr_encoder.0, .2, flow_encoder.0, .2, gru.w, gru.convz|convr (rows
 * stacked), gru.convq, delta.0|weight.0 (rows stacked), delta.2, weight.2, agg.conv1, agg.conv2, agg.eta.0, agg.upmask.0; input channels
 * of corr_encoder.0 padded to 200, of flow_encoder.0 to 8.  glo_weight fp32 [384][128], glo_bias [384]: convz_glo, convr_glo,
 * convq_glo stacked.  K = 0 (ix, eta, upmask unused) skips GraphAgg; otherwise ix[e] in [0, K) is the group of edge e.  Only the
 * launches first_launch <= i <= last_launch of the 17 are enqueued (0 and 16 for all of them): a single one can be timed on the buffers
 * that a whole call has left in scratch.
 * scratch: sgr_update_scratch_bytes(E, K, h, w) bytes, 16-byte aligned (0 = unsupported sizes). */
#define SGR_UPDATE_F32 0
#define SGR_UPDATE_F16 1
#define SGR_UPDATE_ACT_NONE 0
#define SGR_UPDATE_ACT_RELU 1
#define SGR_UPDATE_ACT_SIGMOID 2
#define SGR_UPDATE_ACT_TANH 3
#define SGR_UPDATE_ACT_ETA 4
#define SGR_UPDATE_ACT_GATE 5
#define SGR_UPDATE_ACT_ZR 6
#define SGR_UPDATE_ACT_BLEND 7
#define SGR_UPDATE_OUT_CL_F16 0
#define SGR_UPDATE_OUT_CL_F32 1
#define SGR_UPDATE_OUT_NCHW_F16 2
#define SGR_UPDATE_OUT_NCHW_F32 3
#define SGR_UPDATE_LAYERS 14
#define SGR_UPDATE_LAUNCHES 17
typedef struct SgrUpdateTensor {
  const void* data;
  int64_t stride[4];               /* elements: edge, channel, y, x */
  int32_t dtype;                   /* SGR_UPDATE_F32 / _F16 */
} SgrUpdateTensor;
typedef struct SgrUpdateConv {
  const void* src0;
  const void* src1;
  int32_t stride0, stride1, split, cin, ksize;
  int32_t E, h, w;
  const void* weight;
  int64_t weight_elems;
  const float* bias;
  int32_t cout, act;
  const float* eadd;               /* [E][eadd_stride] or NULL */
  int32_t eadd_stride;
  const void* aux0;
  const void* aux1;
  int32_t aux0_stride, aux1_stride;
  void* out;
  void* out2;
  int32_t out_kind, out_stride, out2_stride;
} SgrUpdateConv;
typedef struct SgrUpdateLayer {
  const void* weight;
  int64_t weight_elems;
  const float* bias;
} SgrUpdateLayer;
typedef struct SgrUpdateWeights {
  SgrUpdateLayer layer[SGR_UPDATE_LAYERS];
  const float* glo_weight;
  const float* glo_bias;
} SgrUpdateWeights;
typedef struct SgrUpdateCall {
  SgrUpdateTensor net, inp, corr, flow;   /* [E,128,h,w], [E,128,h,w], [E,196,h,w], [E,4,h,w] (flow.data NULL: zeros) */
  int32_t E, h, w, K;
  const int64_t* ix;               /* [E] */
  void* net_out;                   /* [E,128,h,w] fp16 */
  void* delta;                     /* [E,h,w,2] fp16 */
  void* weight;                    /* [E,h,w,2] fp16 */
  float* eta;                      /* [K,h,w] */
  void* upmask;                    /* [K,576,h,w] fp16 */
  int32_t first_launch, last_launch;
} SgrUpdateCall;
size_t sgr_update_scratch_bytes(int32_t E, int32_t K, int32_t h, int32_t w);
int sgr_update_pack(const SgrUpdateTensor* src, int32_t E, int32_t C, int32_t h, int32_t w, void* dst, int32_t dst_stride, int32_t c_pad,
                    void* stream);
int sgr_update_conv(const SgrUpdateConv* conv, void* stream);
int sgr_update_forward(const SgrUpdateWeights* weights, const SgrUpdateCall* call, void* scratch, size_t scratch_bytes, void* stream);

/* The feature and context encoders of the tracker (BasicEncoder, thirdparty/glorie_slam/modules/droid_net/extractor.py: fnet with
 * InstanceNorm2d, cnet without a norm), inference only.  Stated in DESIGN.md section 3, "Encoders".  Everything is stream-ordered,
 * allocates nothing, synchronises nothing and is bitwise reproducible; image i of a batch gives the bits of that image alone.
 * Activations are channels-last fp16 [image][y][x][channel] as in the update operator.  The output map of a stride-s convolution is
 * ((h - 1) / s + 1) x ((w - 1) / s + 1); h * w of one image must fit int32, n <= 65535.
 * sgr_encoder_pack: src [n,3,H,W] with element strides -> dst [n*H*W][8] fp16, channels 3..7 zero; with mean and std (3 host floats
 * each, or both NULL) the value stored is (x - mean[c]) / std[c], evaluated in fp32.
 * sgr_encoder_conv: zero padding (ksize - 1) / 2, ksize 1, 3 or 7, stride 1 or 2, cin a multiple of 8, cout 32, 64, 128 or 256.  weight
 * is fp16 [cout][round_up(ksize^2 * cin, 32)], k = tap * cin + c, padding zero; bias fp32 [cout], 16-byte aligned.  Without a norm:
 * v = act(sum + bias), act NONE or RELU, then with a residual map (channels-last fp16) v = relu(residual + v); out_kind is one of
 * SGR_UPDATE_OUT_*.  act SPLIT (cout = 256): channel c < 128 writes tanh(v) to out[image][c][pixel], the others relu(v) to
 * out2[image][c - 128][pixel], both NCHW fp16.  With norm = INSTANCE (cout <= 128, channels-last out, act NONE or RELU): the first launch
 * writes the bias-free fp32 sums to raw [n*ho*wo][cout] and per-tile statistics to stats [n][ceil(ho*wo / 128)][cout][4]; the second
 * merges the statistics in fp64 in a fixed order and writes relu?(residual + act((v - mean) * rstd)), InstanceNorm2d's biased variance
 * and eps = 1e-5.  The bias is not read: it cancels.
 * sgr_encoder_forward: a whole encoder.  layer[] order: conv1, layer1.0.conv1, layer1.0.conv2, layer1.1.conv1, layer1.1.conv2,
 * layer2.0.conv1, layer2.0.conv2, layer2.0.downsample.0, layer2.1.conv1, layer2.1.conv2, layer3.0.conv1, layer3.0.conv2,
 * layer3.0.downsample.0, layer3.1.conv1, layer3.1.conv2, conv2; conv1's input channels padded to 8.  With norm = INSTANCE every layer
 * but conv2 is normalised.  out is [n,out_dim,h,w] fp16, or with split (out_dim = 256) out = tanh of channels 0..127 and out2 = relu
 * of channels 128..255, each [n,128,h,w] fp16.  Only the launches first_launch <= i <= last_launch are enqueued (32 with a norm, 17
 * without).  scratch: sgr_encoder_scratch_bytes(n, H, W, out_dim, norm) bytes, 16-byte aligned (0 = unsupported sizes, among them a
 * normalised map of a single element). */
#define SGR_ENCODER_NORM_NONE 0
#define SGR_ENCODER_NORM_INSTANCE 1
#define SGR_ENCODER_ACT_NONE 0
#define SGR_ENCODER_ACT_RELU 1
#define SGR_ENCODER_ACT_SPLIT 2
#define SGR_ENCODER_LAYERS 16
#define SGR_ENCODER_LAUNCHES_NONE 17        /* launches of sgr_encoder_forward with norm = SGR_ENCODER_NORM_NONE ... */
#define SGR_ENCODER_LAUNCHES_INSTANCE 32    /* ... and with SGR_ENCODER_NORM_INSTANCE */
typedef struct SgrEncoderConv {
  const void* src;
  int32_t src_stride, cin, ksize, stride;
  int32_t n, h, w;                 /* the input maps */
  const void* weight;
  int64_t weight_elems;
  const float* bias;
  int32_t cout, norm, act;
  const void* residual;            /* [n*ho*wo][residual_stride] fp16 or NULL */
  int32_t residual_stride;
  void* out;
  void* out2;
  int32_t out_kind, out_stride;
  float* raw;                      /* norm only */
  int64_t raw_elems;
  float* stats;                    /* norm only */
  int64_t stats_elems;
} SgrEncoderConv;
typedef struct SgrEncoderWeights {
  SgrUpdateLayer layer[SGR_ENCODER_LAYERS];
  int32_t out_dim, norm;
} SgrEncoderWeights;
typedef struct SgrEncoderCall {
  SgrUpdateTensor images;          /* [n,3,H,W] */
  int32_t n, H, W, normalize;
  float mean[3], std_[3];          /* read when normalize != 0 */
  void* out;
  void* out2;
  int32_t split, first_launch, last_launch;
} SgrEncoderCall;
size_t sgr_encoder_scratch_bytes(int32_t n, int32_t H, int32_t W, int32_t out_dim, int32_t norm);
int sgr_encoder_pack(const SgrUpdateTensor* src, int32_t n, int32_t H, int32_t W, SGR_HOST const float* mean,
                     SGR_HOST const float* std_, void* dst, void* stream);
int sgr_encoder_conv(const SgrEncoderConv* conv, void* stream);
int sgr_encoder_forward(const SgrEncoderWeights* weights, const SgrEncoderCall* call, void* scratch, size_t scratch_bytes, void* stream);

/* The vision transformer of the mono-depth prior (timm's ViT blocks as the DPT of thirdparty/mono_priors/omnidata/modules/midas reads
 * them), inference only.  Stated in DESIGN.md section 3, "Vision transformer".  Everything is stream-ordered, allocates nothing,
 * synchronises nothing and is bitwise reproducible (no atomics; the order of every sum follows from the shape alone), and an image
 * gives the same bits alone and inside any batch.  dim D = 64 * heads, heads 1..16, head dimension 64, hidden width 4 D, tokens
 * T = 1 + gh * gw >= 2 per image, B * T must fit int32.  The residual stream is fp32 [B*T][D]; every GEMM operand is fp16, every sum
 * fp32 (mfma_f32_16x16x32_f16).  fp16 buffers need 16-byte aligned bases and row strides that are multiples of 8 elements.
 * sgr_vit_layernorm: out[m][:] = fp16((x[m][:] - mean) * rsqrt(var + 1e-6) * gamma + beta), biased variance, mean and variance in
 * fp32 of the row shifted by its first element (a constant row gives beta exactly); x fp32 [M][D], D a multiple of 64 up to 1024.
 * sgr_vit_gemm: v[m][n] = sum_k a[m * lda + k] w[n * ldw + k] + bias[n] (bias NULL: 0), M >= 1, N and K multiples of 64, then by epi:
 *   STORE_F16  out fp16 [m * ldo + n] = v;   STORE_F32  out fp32 [m * ldo + n] = v;   GELU_F16  out fp16 [m * ldo + n] = gelu(v), the
 *   exact erf form;   RESIDUAL  out fp32 [m * ldo + n] += v and, with tap, tap fp16 [m * ldo + n] = the updated value;
 *   READOUT  row m = (image b, token t) of T tokens: t = 0 writes nothing, t > 0 writes out fp16 [(b * N + n) * (T - 1) + t - 1] =
 *   gelu(v + aux[b * N + n]);   EMBED  row m = (image b, patch p) of T - 1 patches: out fp32 [(b * T + 1 + p) * ldo + n] =
 *   v + aux[(1 + p) * N + n].
 * sgr_vit_attention: qkv fp16 [B][T][3][heads][64] -> out fp16 [B][T][heads * 64] = softmax(q k^T / 8) v per (image, head), flash
 * style: scores, running maximum and sum in fp32, the probabilities rounded to fp16 for the second product, one division at the end.
 * sgr_vit_forward: patches fp16 [B][gh*gw][cin] (cin a multiple of 64) -> two tap maps fp16 [B][D][gh][gw].  pos is fp32 [T][D], row 0
 * the class token plus its position row, row 1 + p the position row of patch p.  Launch 0 writes the stream (class rows, then the
 * patch embedding with epilogue EMBED); block i is launches 1 + 7 i .. 7 + 7 i: norm1, qkv, attention, proj (RESIDUAL), norm2, fc1
 * (GELU), fc2 (RESIDUAL, with the tap copy when i is tap[0] or tap[1]: the block's output before any final norm); then per tap j the
 * class-token half of the readout, readout_w[j][:, D:] x_cls + readout_b[j] as fp32 [B][D], and the token half with epilogue READOUT:
 * 5 + 7 depth launches, of which first_launch <= i <= last_launch are enqueued.  readout_w[j] is fp16 [D][2 D].
 * scratch: sgr_vit_scratch_bytes(B, T, heads, depth) bytes, 16-byte aligned (0 = unsupported sizes). */
#define SGR_VIT_EPI_STORE_F16 1
#define SGR_VIT_EPI_GELU_F16 2
#define SGR_VIT_EPI_RESIDUAL 3
#define SGR_VIT_EPI_READOUT 4
#define SGR_VIT_EPI_EMBED 5
#define SGR_VIT_EPI_STORE_F32 6
typedef struct SgrVitGemm {
  const void* a;                   /* fp16 [M][lda] */
  const void* w;                   /* fp16 [N][ldw] */
  const float* bias;               /* [N] or NULL */
  int64_t lda, ldw, ldo;
  int32_t M, N, K, epi;
  void* out;
  void* tap;                       /* RESIDUAL: fp16 [M][ldo] or NULL */
  const float* aux;                /* READOUT: [B][N]; EMBED: [T][N] */
  int32_t T;                       /* READOUT, EMBED: tokens per image */
} SgrVitGemm;
typedef struct SgrVitBlock {
  const float* ln1_g;
  const float* ln1_b;
  const void* qkv_w;               /* fp16 [3 D][D] */
  const float* qkv_b;
  const void* proj_w;              /* fp16 [D][D] */
  const float* proj_b;
  const float* ln2_g;
  const float* ln2_b;
  const void* fc1_w;               /* fp16 [4 D][D] */
  const float* fc1_b;
  const void* fc2_w;               /* fp16 [D][4 D] */
  const float* fc2_b;
} SgrVitBlock;
typedef struct SgrVitWeights {
  int32_t dim, heads, depth, cin;
  int32_t tap[2];                  /* two distinct blocks in [0, depth) */
  const void* embed_w;             /* fp16 [D][cin] */
  const float* embed_b;
  const SgrVitBlock* blocks;       /* host array [depth] */
  const void* readout_w[2];
  const float* readout_b[2];
} SgrVitWeights;
typedef struct SgrVitCall {
  const void* patches;
  int32_t B, gh, gw;
  const float* pos;
  void* out[2];
  int32_t first_launch, last_launch;
} SgrVitCall;
size_t sgr_vit_scratch_bytes(int32_t B, int32_t T, int32_t heads, int32_t depth);
int sgr_vit_layernorm(const float* x, const float* gamma, const float* beta, int64_t M, int32_t D, void* out, void* stream);
int sgr_vit_gemm(const SgrVitGemm* gemm, void* stream);
int sgr_vit_attention(const void* qkv, int32_t B, int32_t T, int32_t heads, void* out, void* stream);
int sgr_vit_forward(const SgrVitWeights* weights, const SgrVitCall* call, void* scratch, size_t scratch_bytes, void* stream);

/* The ResNet-V2 backbone of the mono-depth prior (weight-standardised convolutions without bias, group norms, bottleneck blocks),
 * inference only.  Stated in DESIGN.md section 3, "ResNet-V2 backbone".  Everything is stream-ordered, allocates nothing, synchronises
 * nothing and is bitwise reproducible (no atomics; the order of every sum follows from the shapes alone), and an image gives the same
 * bits alone and inside any batch.  Activations are channels-last fp16 [image][y][x][channel]; h * w of one image must fit int32,
 * n <= 65535.
 * sgr_resnet_conv: ksize 1, 3 or 7, stride 1 or 2, cin a multiple of 8 up to 1024, cout a multiple of 16 in 16..1024.  Output pixel
 * (oy, ox) of the ho x wo map sums the taps (oy * stride - pad_top + dy, ox * stride - pad_left + dx); taps outside the h x w map read
 * zero, so the padding after the map is implied.  0 <= pad < ksize, and ho (wo alike) must be (h + pad_top + after - ksize) / stride + 1
 * for some 0 <= after < ksize.  weight is fp16 [cout][round_up(ksize^2 * cin, 32)], k = tap * cin + c, padding zero.  Without a norm:
 * v = act(sum + bias), bias fp32 [cout] or NULL, act NONE or RELU, out_kind one of SGR_UPDATE_OUT_*.  With norm = GROUP (groups divides
 * cout into a power of two of at most 64 channels, at most 256 groups, at least 2 elements per group and image): writes the fp32 sums
 * to raw [n*ho*wo][cout] and, per tile of 128 pixels and group, (count, s, sum (v - s), sum (v - s)^2) to stats
 * [n][ceil(ho*wo / 128)][groups][4], s being the group's first sum at the tile's first pixel; bias, act and out are not read.
 * sgr_resnet_stats: the same statistics of a given fp32 map raw [n*hw][cout].
 * sgr_resnet_groupnorm: merges the statistics of each (image, group) in fp64 in a fixed order and writes channels-last fp16
 * relu?(residual + ((v - mean) * rstd * gamma[c] + beta[c])), biased variance, eps = 1e-5, gamma and beta fp32 [cout]; a constant
 * group gives beta[c] exactly.  residual is channels-last fp16 or NULL.
 * sgr_resnet_maxpool: 3x3, stride 2, TF "same" padding filled with -inf: [n][h][w][channels] -> [n][ceil(h/2)][ceil(w/2)][channels],
 * channels a multiple of 8.
 * sgr_resnet_forward: images [n,3,H,W], H and W multiples of 32 -> the three stage maps l1 [n][H/4*W/4][stage_chs[0]],
 * l2 [n][H/8*W/8][stage_chs[1]], l3 [n][H/16*W/16][stage_chs[2]] (l3 is the patches layout of sgr_vit_forward).  stem_chs is a
 * multiple of 16, stage_chs multiples of 64, the bottleneck width stage_chs / 4.  layers[] order: stem, then per block conv1, conv2,
 * conv3 and, in the first block of a stage, downsample; every convolution has TF "same" padding and is followed by its group norm.
 * Launches: pack (sgr_encoder_pack, with mean and std when normalize), stem conv, stem norm (ReLU), pool, then per block conv1, norm1
 * (ReLU), in the first block of a stage downsample conv and norm, conv2 (stride 2 in the first block of stages 1 and 2), norm2 (ReLU),
 * conv3, norm3 (+ shortcut, ReLU): 4 + sum over stages (6 blocks + 2), of which first_launch <= i <= last_launch are enqueued.
 * scratch: sgr_resnet_scratch_bytes(n, H, W, stem_chs, stage_chs[0..2]) bytes, 16-byte aligned (0 = unsupported sizes). */
#define SGR_RESNET_NORM_NONE 0
#define SGR_RESNET_NORM_GROUP 1
#define SGR_RESNET_ACT_NONE 0
#define SGR_RESNET_ACT_RELU 1
typedef struct SgrResnetConv {
  const void* src;
  int32_t src_stride, cin, ksize, stride;
  int32_t n, h, w;                 /* the input maps */
  int32_t pad_top, pad_left, ho, wo;
  const void* weight;
  int64_t weight_elems;
  const float* bias;               /* [cout] or NULL; not read with a norm */
  int32_t cout, norm, act, groups;
  void* out;
  int32_t out_kind, out_stride;
  float* raw;                      /* norm only */
  int64_t raw_elems;
  float* stats;                    /* norm only */
  int64_t stats_elems;
} SgrResnetConv;
typedef struct SgrResnetNorm {
  const float* raw;                /* [n*hw][cout] */
  const float* stats;              /* [n][ceil(hw / 128)][groups][4] */
  int32_t n, hw, cout, groups, relu;
  const float* gamma;
  const float* beta;
  const void* residual;            /* [n*hw][residual_stride] fp16 or NULL */
  int32_t residual_stride;
  void* out;                       /* [n*hw][out_stride] fp16 */
  int32_t out_stride;
} SgrResnetNorm;
typedef struct SgrResnetLayer {
  const void* weight;              /* packed, standardised fp16 */
  int64_t weight_elems;
  const float* gamma;
  const float* beta;
} SgrResnetLayer;
typedef struct SgrResnetWeights {
  int32_t stem_chs, stage_chs[3], stage_blocks[3], groups, num_layers;
  const SgrResnetLayer* layers;    /* host array [num_layers] */
} SgrResnetWeights;
typedef struct SgrResnetCall {
  SgrUpdateTensor images;          /* [n,3,H,W] */
  int32_t n, H, W, normalize;
  float mean[3], std_[3];          /* read when normalize != 0 */
  void* l1;
  void* l2;
  void* l3;
  int32_t first_launch, last_launch;
} SgrResnetCall;
size_t sgr_resnet_scratch_bytes(int32_t n, int32_t H, int32_t W, int32_t stem_chs, int32_t chs0, int32_t chs1, int32_t chs2);
int sgr_resnet_conv(const SgrResnetConv* conv, void* stream);
int sgr_resnet_stats(const float* raw, int32_t n, int32_t hw, int32_t cout, int32_t groups, float* stats, void* stream);
int sgr_resnet_groupnorm(const SgrResnetNorm* norm, void* stream);
int sgr_resnet_maxpool(const void* src, int32_t n, int32_t h, int32_t w, int32_t channels, void* dst, void* stream);
int sgr_resnet_forward(const SgrResnetWeights* weights, const SgrResnetCall* call, void* scratch, size_t scratch_bytes, void* stream);

/* The decoder of the mono-depth prior (reassemble, layerN_rn, four fusion blocks, head) and the two resizes of predict, inference
 * only.  Stated in DESIGN.md section 3, "DPT decoder".  Everything is stream-ordered, allocates nothing, synchronises nothing, uses no
 * atomics and is bitwise reproducible; an image gives the same bits alone and inside any batch.  Maps are channels-last fp16
 * [image][y][x][channel] with a row stride in halfs that is a multiple of 8 and a 16-byte aligned base; n * h * w must fit int32.
 * sgr_dpt_conv: stride 1, ksize 1 or 3, zero padding (ksize - 1) / 2, cin a multiple of 8 up to 1024, cout 1..1024.  weight is fp16
 * [round_up(cout, 64)][round_up(ksize^2 * cin, 32)], k = tap * cin + c, padding zero; bias fp32 [round_up(cout, 64)] or NULL.  With
 * relu_in every input value x is read as max(x, 0).  In fp32: v = sum + bias, with relu v = max(v, 0), then v += res0[m][n] and
 * v += res1[m][n] (each channels-last fp16 or NULL), one rounding.  out_kind SGR_UPDATE_OUT_CL_F16 (out_stride a multiple of 8) or
 * SGR_UPDATE_OUT_CL_F32 (any out_stride >= cout; cout = 1, out_stride = 1 is the plane [n][h][w]).  A tile of 128 pixels may span images.
 * sgr_dpt_up2: bilinear, align_corners = True, [n][h][w][channels] -> [n][2h][2w][channels], channels a multiple of 8; output row o
 * reads the source position o (h - 1) / (2h - 1), split into integer and fraction in integers; the four weights and the sum are fp32.
 * sgr_dpt_resize_in: src fp32 [planes][H][W] -> dst fp16 [planes][h][w] = ((antialiased bilinear resize, align_corners = False) - 0.5)
 * / 0.5: with S = max(in, out) per axis, output o sums the taps x with integer weight max(0, 2S - |(2x + 1) out - (2o + 1) in|),
 * divided by their sum.
 * sgr_dpt_resize_out: src fp32 [planes][h][w] -> dst fp32 [planes][H][W] = clamp(bicubic(clamp(src, 0, 1)), 0, 1): cubic convolution with
 * A = -0.75, align_corners = False, source position ((2o + 1) in - out) / (2 out) from integers, border indices clamped.
 * sgr_dpt_forward: taps [n,dim,H/16,W/16] (NCHW, any strides), l1 [n][H/4*W/4][chs0] and l2 [n][H/8*W/8][chs1] (the stage maps of
 * sgr_resnet_forward) -> depth fp32 [n][H][W].  layer[] order: act_postprocess3.3, act_postprocess4.3, act_postprocess4.4 (packed as
 * for sgr_resnet_conv: [dim] rows, bias fp32 [dim]), layer1_rn .. layer4_rn, refinenet4.{resConfUnit2.conv1, .conv2, out_conv}, for
 * i = 3, 2, 1 refinenet{i}.{resConfUnit1.conv1, .conv2, resConfUnit2.conv1, .conv2, out_conv}, output_conv.0, .2, .4.  The 35
 * launches: pack3, act_postprocess3.3, pack4, act_postprocess4.3, act_postprocess4.4 (sgr_resnet_conv, stride 2), the four layerN_rn,
 * per fusion block its convolutions (the adds in the epilogues), up2 and out_conv, then output_conv.0, up2, output_conv.2 (ReLU),
 * output_conv.4 (ReLU, fp32); first_launch <= i <= last_launch are enqueued.  dim and features are multiples of 16 up to 1024, H and W
 * multiples of 32.  scratch: sgr_dpt_scratch_bytes(n, H, W, dim, features) bytes, 16-byte aligned (0 = unsupported sizes). */
#define SGR_DPT_LAYERS 28
#define SGR_DPT_LAUNCHES 35
typedef struct SgrDptConv {
  const void* src;
  int32_t src_stride, cin, ksize;
  int32_t n, h, w;
  const void* weight;
  int64_t weight_elems;
  const float* bias;
  int32_t cout, relu_in, relu;
  const void* res0;
  const void* res1;
  int32_t res0_stride, res1_stride;
  void* out;
  int32_t out_kind, out_stride;
} SgrDptConv;
typedef struct SgrDptWeights {
  int32_t dim, features, chs0, chs1;
  SgrUpdateLayer layer[SGR_DPT_LAYERS];
} SgrDptWeights;
typedef struct SgrDptCall {
  SgrUpdateTensor tap3, tap4;      /* [n,dim,H/16,W/16] */
  const void* l1;
  const void* l2;
  int32_t n, H, W;
  float* depth;                    /* [n][H][W] */
  int32_t first_launch, last_launch;
} SgrDptCall;
size_t sgr_dpt_scratch_bytes(int32_t n, int32_t H, int32_t W, int32_t dim, int32_t features);
int sgr_dpt_conv(const SgrDptConv* conv, void* stream);
int sgr_dpt_up2(const void* src, int32_t n, int32_t h, int32_t w, int32_t channels, int32_t src_stride, void* dst, int32_t dst_stride,
                void* stream);
int sgr_dpt_resize_in(const float* src, int32_t planes, int32_t H, int32_t W, void* dst, int32_t h, int32_t w, void* stream);
int sgr_dpt_resize_out(const float* src, int32_t planes, int32_t h, int32_t w, float* dst, int32_t H, int32_t W, void* stream);
int sgr_dpt_forward(const SgrDptWeights* weights, const SgrDptCall* call, void* scratch, size_t scratch_bytes, void* stream);

/* LPIPS v0.1 on the AlexNet trunk, the third image figure of eval_rendering (eval_utils.py:66-68, 125, 192), inference only.  Stated in
 * DESIGN.md section 3, "LPIPS".  Everything is stream-ordered, allocates nothing, synchronises nothing, uses no atomics and is bitwise
 * reproducible; a pair gives the same bits alone and inside any batch.  Maps are channels-last fp16 [image][y][x][channel], 16-byte
 * aligned.  A call on n pairs works on 2n images: image i is the first and image n + i the second member of pair i.
 * sgr_lpips_pack: frames (host table, n <= SGR_LPIPS_MAX_PAIRS; depth fields unused) -> dst [2n][H][W][8]: channels 0..2 =
 * (2 img - 1 - shift[c]) / scale[c], channels 3..7 = 0; img = clamp(exp(a) render + b, 0, 1) for image i (NULL exposure = identity),
 * the ground truth for image n + i.  sgr_lpips_pack_pairs: the same from img0, img1 fp32 [n][3][H][W], taken as they are; with
 * normalize 0 the value is (img - shift[c]) / scale[c].  shift and scale are host arrays of 3.
 * sgr_lpips_conv: relu(conv(src) + bias), ksize 11, 5 or 3, stride 1 or 4, symmetric zero padding pad < ksize, cin a multiple of 8,
 * cout a multiple of 64, both up to 1024: [n][h][w][cin] -> [n][ho][wo][cout], ho = (h + 2 pad - ksize) / stride + 1.  weight is fp16
 * [cout][round_up(ksize^2 * cin, 32)], k = tap * cin + c, padding zero; bias fp32 [cout].
 * sgr_lpips_maxpool: 3x3, stride 2, no padding: [n][h][w][channels] -> [n][(h - 3) / 2 + 1][(w - 3) / 2 + 1][channels], channels a
 * multiple of 8, h and w >= 3.
 * sgr_lpips_distance: maps [2n][P][C] (C one of 64, 192, 256, 384), weight fp32 [C] -> partials [n][ceil(P / SGR_LPIPS_DIST_PIXELS)],
 * the sums over a workgroup's pixels p of d_p = sum_c w_c (u_c - v_c)^2, u = f0 / sqrt(1e-8 + sum f0^2), v likewise; per_pixel (or
 * NULL) [n][P] receives every d_p.  u and v are rounded to fp32 before they are subtracted, so equal maps give exactly 0 and
 * swapped maps the same bits.
 * sgr_lpips_forward: the SGR_LPIPS_LAUNCHES launches pack, conv1, distance1, pool1, conv2, distance2, pool2, conv3, distance3, conv4,
 * distance4, conv5, distance5, final; first_launch <= i <= last_launch are enqueued.  The input is the frame table when frames is
 * set, otherwise img0 / img1.  out [n] = the sum of the five tap means (each merged in fp64 in a fixed order); levels (or NULL)
 * [n][5] the tap means.  1 <= n <= SGR_LPIPS_MAX_PAIRS, H and W >= 31.  scratch: sgr_lpips_scratch_bytes(n, H, W) bytes, 16-byte
 * aligned (0 = unsupported sizes). */
#define SGR_LPIPS_MAX_PAIRS 16
#define SGR_LPIPS_DIST_PIXELS 128
#define SGR_LPIPS_LAUNCHES 14
typedef struct SgrLpipsConv {
  const void* src;
  int32_t n, h, w, cin;
  int32_t ksize, stride, pad;
  const void* weight;
  int64_t weight_elems;
  const float* bias;
  int32_t cout;
  void* out;
} SgrLpipsConv;
typedef struct SgrLpipsWeights {
  SgrUpdateLayer conv[5];          /* packed as for sgr_lpips_conv: 3(8)->64 11x11, 64->192 5x5, 192->384, 384->256, 256->256 3x3 */
  const float* lin[5];             /* fp32 [64], [192], [384], [256], [256] */
  float shift[3], scale[3];
} SgrLpipsWeights;
typedef struct SgrLpipsCall {
  const SgrMetricFrame* frames;    /* host array [n], or NULL */
  const float* img0;               /* [n][3][H][W], read when frames is NULL */
  const float* img1;
  int32_t normalize;               /* of img0 / img1: 2 x - 1 first */
  int32_t n, H, W;
  float* out;                      /* [n] */
  float* levels;                   /* [n][5], or NULL */
  int32_t first_launch, last_launch;
} SgrLpipsCall;
size_t sgr_lpips_scratch_bytes(int32_t n, int32_t H, int32_t W);
int sgr_lpips_pack(int32_t n, const SgrMetricFrame* frames, int32_t H, int32_t W, SGR_HOST const float* shift,
                   SGR_HOST const float* scale, void* dst, void* stream);
int sgr_lpips_pack_pairs(const float* img0, const float* img1, int32_t n, int32_t H, int32_t W, int32_t normalize,
                         SGR_HOST const float* shift, SGR_HOST const float* scale, void* dst, void* stream);
int sgr_lpips_conv(const SgrLpipsConv* conv, void* stream);
int sgr_lpips_maxpool(const void* src, int32_t n, int32_t h, int32_t w, int32_t channels, void* dst, void* stream);
int sgr_lpips_distance(const void* maps, int32_t n, int32_t P, int32_t C, const float* weight, float* partials, float* per_pixel,
                       void* stream);
int sgr_lpips_forward(const SgrLpipsWeights* weights, const SgrLpipsCall* call, void* scratch, size_t scratch_bytes, void* stream);

/* Trajectory scoring (src/utils/eval_traj.py; DESIGN.md section 3, "Trajectory scoring").  Stream-ordered, no allocation, fixed-order
 * fp64 reductions (per-workgroup partials in `scratch`, merged in workgroup order; no float atomics): bitwise reproducible.
 * 1 <= n <= SGR_TRAJ_MAX_POSES pairs; scratch: sgr_traj_scratch_bytes(n) bytes (0 = unsupported n), for both calls.
 * sgr_traj_accumulate (SGR_TRAJ_ACCUMULATE_LAUNCHES launches): pair i is (row i of est, row i of ref).
 *   est, kind SGR_TRAJ_POSE7_W2C: [est_rows, 7] (tx,ty,tz,qx,qy,qz,qw) world -> camera, the video's layout, read in place; the centre is
 *     the translation of SE3(p).inv() in the fp32 arithmetic of se3_inv, widened to fp64.  Kind SGR_TRAJ_MAT4_C2W: [est_rows, 16]
 *     row-major camera -> world, 16-byte aligned; the centre is (m[3], m[7], m[11]).
 *   inds: NULL (rows 0 .. n-1 of est) or a HOST list [n] of est rows; an entry outside [0, est_rows) is SGR_ERR_INVALID before anything
 *     is launched.  The list is copied into scratch on the stream: it stays valid until the stream has passed the call.
 *   ref: [n, 16] row-major camera -> world, 16-byte aligned; a pair is skipped iff any of the 16 entries is not finite (eval_traj.py:30-33,
 *     63-66: the sum of the matrix is nan or inf exactly then).
 *   pos [n,2,3]: the centre x of the estimate and y of the reference of every pair (skipped ones too); valid [n]: 1 = used.
 *   sums[17] over the used pairs: count, sum x (3), sum y (3), then about the means xm = sum x / count, ym = sum y / count:
 *     sum |x - xm|^2, sum (y - ym)(x - xm)^T (9, row-major, the index of y first).
 * sgr_traj_errors (SGR_TRAJ_ERRORS_LAUNCHES launches): sim3 = (s, R row-major (9), t (3)) on the host, read before the call returns.
 *   err[n]: |s R x + t - y| of the used pairs, NaN for skipped ones.  stats[8] over the used pairs: count, sum e, sum e^2, min, max, the
 *   order statistics of rank (count - 1) / 2 and count / 2 (each exactly an element of err; equal for an odd count), and
 *   sum (e - sum e / count)^2.  With no used pair the sums are 0 and the other five NaN. */
#define SGR_TRAJ_POSE7_W2C 0
#define SGR_TRAJ_MAT4_C2W 1
#define SGR_TRAJ_MAX_POSES 65535
#define SGR_TRAJ_ACCUMULATE_LAUNCHES 2
#define SGR_TRAJ_ERRORS_LAUNCHES 2
size_t sgr_traj_scratch_bytes(int32_t n);
int sgr_traj_accumulate(int32_t kind, const float* est, int32_t est_rows, SGR_HOST const int64_t* inds, int32_t n, const float* ref,
                        double* pos, uint8_t* valid, double* sums, void* scratch, size_t scratch_bytes, void* stream);
int sgr_traj_errors(int32_t n, const double* pos, const uint8_t* valid, SGR_HOST const double* sim3, double* err, double* stats,
                    void* scratch, size_t scratch_bytes, void* stream);

/* Time association and pose-to-pose errors ("Trajectory scoring": evo's matching_time_indices, APE and RPE of
 * every pose relation).  The same house rules: stream-ordered, no allocation, fp64, fixed-order reductions, bitwise reproducible.
 * sgr_traj_associate (SGR_TRAJ_ASSOCIATE_LAUNCHES launches): for every stamps_a[i], i < na, the nearest of stamps_b[j] + offset_b,
 *   j < nb (stamps_b non-decreasing): j = argmin_j |(stamps_b[j] + offset_b) - stamps_a[i]| in fp64 as written, the lowest j among
 *   equal distances; match[i] = j where that distance <= max_diff, else -1 (a NaN distance is no match).  Several i may share a j.
 *   1 <= na <= SGR_TRAJ_MAX_POSES, 1 <= nb <= SGR_TRAJ_MAX_STAMPS; scratch: sgr_traj_associate_scratch_bytes(na, nb) (0 = unsupported).
 *   a_inds[na], b_inds[na]: the matched (i, match[i]) compacted in the order of i, -1 behind them.
 *   header[SGR_TRAJ_HEADER_WORDS]: [0] the number of matches, [1] 1 iff some stamps_b[j + 1] >= stamps_b[j] does not hold (EVERY j is
 *   looked at, a NaN stamp counts as out of order; match is then within bounds but meaningless), the rest 0.
 * sgr_traj_pose_errors (SGR_TRAJ_POSE_ERRORS_LAUNCHES launches): pair i < n is (row est_inds[i] of est, row ref_inds[i] of ref), row i
 *   of either where its DEVICE list is NULL.  est as in sgr_traj_accumulate, but a pose7 row is normalised and inverted in fp64;
 *   ref [ref_rows, 16]; both 4 x 4 layouts 16-byte aligned, of each matrix the upper 3 x 4 [R | t] is used as a rigid pose.
 *   A pair is unused iff an index is outside [0, rows), or any entry of its ref row or of its est row is not finite (nor its
 *   normalised pose: a zero quaternion).  P = [r_a R | s r_a t + t_a] of the estimate under sim3 (as sgr_traj_errors), Q the reference.
 *   The c used pairs are ranked in the order of i.  mode SGR_TRAJ_ABSOLUTE: one item per used pair, E = Q^-1 P.  SGR_TRAJ_RELATIVE,
 *   delta >= 1: items over the ranks (k delta, (k + 1) delta), k < floor((c - 1) / delta), or with all_pairs (r, r + delta), r < c - delta;
 *   E = (Q_i^-1 Q_j)^-1 (P_i^-1 P_j).  Inverses are rigid: [R | t]^-1 = [R^T | -R^T t].  The error of an item by `relation`:
 *   |E_t|, atan2(|a|, tr E_R - 1) with a = (E32 - E23, E13 - E31, E21 - E12) in radians or degrees, |E_R - I|_F, |E - I|_F.
 *   err[n]: the m items' errors, NaN behind them; pair_rows[n,2]: the pairs i (and j, else -1) of each item, -1 behind them;
 *   stats[8] over the items, the layout and the device code of sgr_traj_errors; header: [0] m, [1] c, [2] n - c, [3] 0.
 *   scratch: sgr_traj_pose_errors_scratch_bytes(n) (0 = unsupported n). */
#define SGR_TRAJ_MAX_STAMPS 16777216
#define SGR_TRAJ_HEADER_WORDS 4
#define SGR_TRAJ_ASSOCIATE_LAUNCHES 2
#define SGR_TRAJ_POSE_ERRORS_LAUNCHES 4
#define SGR_TRAJ_ABSOLUTE 0
#define SGR_TRAJ_RELATIVE 1
#define SGR_TRAJ_TRANSLATION_PART 0
#define SGR_TRAJ_ROTATION_ANGLE_RAD 1
#define SGR_TRAJ_ROTATION_ANGLE_DEG 2
#define SGR_TRAJ_ROTATION_PART 3
#define SGR_TRAJ_FULL_TRANSFORMATION 4
size_t sgr_traj_associate_scratch_bytes(int32_t na, int32_t nb);
int sgr_traj_associate(const double* stamps_a, int32_t na, const double* stamps_b, int32_t nb, double offset_b, double max_diff,
                       int32_t* match, int32_t* a_inds, int32_t* b_inds, int32_t* header, void* scratch, size_t scratch_bytes,
                       void* stream);
size_t sgr_traj_pose_errors_scratch_bytes(int32_t n);
int sgr_traj_pose_errors(int32_t kind, const float* est, int32_t est_rows, const float* ref, int32_t ref_rows, const int32_t* est_inds,
                         const int32_t* ref_inds, int32_t n, SGR_HOST const double* sim3, int32_t mode, int32_t delta, int32_t all_pairs,
                         int32_t relation, double* err, int32_t* pair_rows, double* stats, int32_t* header, void* scratch,
                         size_t scratch_bytes, void* stream);

/* Frame preparation of the dataset streams (src/utils/datasets.py:170-216; DESIGN.md section 3, "Datasets and frame preparation"):
 * undistortion, bilinear resize to (H_oe, W_oe), crop of the edge and / 255 of the colour, nearest resize, crop and / depth_scale of the
 * depth, for n >= 1 frames of one camera in SGR_FRAME_PREPARE_LAUNCHES launch.  Stream-ordered, no scratch, every output element written.
 *   color_u8 [n,H,W,ps]: ps = 3 or 4 bytes a pixel, R G B first (with ps = 4 the fourth byte is ignored and color_u8 is 4-byte aligned).
 *   depth_u16 [n,H,W] and out_depth [n,H_out,W_out] are given together or both NULL.  H_out = H_oe - 2 H_edge, W_out = W_oe - 2 W_edge.
 *   map_q [H,W,2] int32, 8-byte aligned, or NULL (no undistortion): (qx, qy) of every full-size pixel, the source position in 1/32 pixel.
 *   Colour, in integers: U(v,u,c) = (sum w p + 512) >> 10 over the taps (iy,ix), (iy,ix+1), (iy+1,ix), (iy+1,ix+1) with ix = qx >> 5,
 *   ax = qx & 31 (iy, ay likewise), weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax ay, a tap outside the image counting as 0; without
 *   a map U is the source level.  Per axis of input size S and output size D, output index j has n = (2j+1) S - D, d = 2D, s = floor(n/d),
 *   b = floor((4096 (n - s d) + d) / (2d)); s < 0 gives s = 0, b = 0; s >= S-1 gives s = S-1, b = 0 and the second tap at S-1.
 *   R = (sum_y sum_x wy wx U + 2^21) >> 22 with w in {2048 - b, b}; out_color[c][y][x] = (float)R(y + H_edge, x + W_edge, c) / 255.0f.
 *   Depth: sy = min((int)floorf((y + H_edge) * ((float)H / (float)H_oe)), H - 1), sx likewise, out = (float)d / depth_scale: the bits of
 *   torch's F.interpolate(mode="nearest") on the CPU, then the crop.  Both fp32 divisions are correctly rounded.
 *   SGR_ERR_INVALID (nothing launched): n outside [1, 65535], a side outside [1, 16384], edges that leave no pixel, ps not 3 or 4, depth
 *   given on one side only or with a depth_scale that is not positive and finite, a misaligned pointer. */
#define SGR_FRAME_PREPARE_LAUNCHES 1
int sgr_frame_prepare(int32_t n, const uint8_t* color_u8, int32_t ps, const uint16_t* depth_u16, int32_t H, int32_t W, const int32_t* map_q,
                      int32_t H_oe, int32_t W_oe, int32_t H_edge, int32_t W_edge, float depth_scale, float* out_color, float* out_depth,
                      void* stream);

/* The per-keyframe figure of eval_rendering (src/utils/eval_utils.py:131-135, plot_rgbd_silhouette; DESIGN.md section 3, "Plots"): for
 * each of n frames one RGB panel of 2 x 3 cells, ground truth above the render: colour, depth, difference.  Each cell shows its image
 * reduced by the integer factor s: a source pixel is first turned into the byte triple a full-size plot would show, a cell pixel is the
 * integer mean (sum + cnt / 2) / cnt per channel over its s x s block, cnt the pixels of the block that exist.  Source pixels:
 *   (0,0) (int)(255 clamp(gt, 0, 1));  (1,0) the same of clamp(exp(a) render + b, 0, 1), the image of sgr_render_metrics;
 *   (0,1) jet(gt_depth / depth_max);   (1,1) jet((global_scale * depth) / depth_max);
 *   (0,2) jet index min(255, 256 e / max e), e = the sum over the channels of |level of (0,0) - level of (1,0)|, in integers;
 *   (1,2) jet(e / max e), e = |global_scale * depth - gt_depth| where depth > 0 and gt_depth > 0, else 0.
 * jet(t) is entry clamp((int)floor(256 t), 0, 255) of the 256-entry jet table; every product, difference and quotient above is one
 * correctly rounded fp32 operation.  A maximum is taken over the frame's finite values and 0 gives t = 0; a value that is not finite
 * is drawn white.  Layout: white background; the heading at (SGR_PLOT_MARGIN, SGR_PLOT_MARGIN), clipped at PW - SGR_PLOT_MARGIN; cell
 * (r, c) of size ch x cw = ceil(H / s) x ceil(W / s) has its left edge at SGR_PLOT_MARGIN + c (cw + SGR_PLOT_MARGIN), its title's top at
 * 2 SGR_PLOT_MARGIN + SGR_PLOT_CHAR_H + r (SGR_PLOT_CHAR_H + SGR_PLOT_TITLE_GAP + ch + SGR_PLOT_MARGIN) and its image
 * SGR_PLOT_CHAR_H + SGR_PLOT_TITLE_GAP below that; a title is clipped at its cell's right edge.  Text is black, one 5 x 7 glyph at
 * twice its size in the top left of each SGR_PLOT_CHAR_W x SGR_PLOT_CHAR_H character cell; a text ends at its first NUL or after
 * SGR_PLOT_TEXT - 1 bytes, and a byte outside 32 .. 126 is drawn as '?'.
 * sgr_plot_panel_size: host arithmetic only; PH = PW = 0 for H, W outside [1, 16384] or s < 1.
 * sgr_plot_panels: `frames` is a host array, copied into scratch on the stream: it stays valid until the stream has passed the call.
 * SGR_PLOT_LAUNCHES launches per SGR_PLOT_MAX_FRAMES frames (the maxima by integer atomicMax, order-independent; the composition, every
 * output byte written once); a frame's panel is the same alone and in any batch.  depth and gt_depth are required; exposure_a / _b as
 * in SgrMetricFrame.  SGR_ERR_INVALID / SGR_ERR_WORKSPACE before anything is launched. */
#define SGR_PLOT_MAX_FRAMES 16
#define SGR_PLOT_LAUNCHES 2
#define SGR_PLOT_TEXT 64
#define SGR_PLOT_MARGIN 8
#define SGR_PLOT_CHAR_W 12
#define SGR_PLOT_CHAR_H 16
#define SGR_PLOT_TITLE_GAP 4
typedef struct SgrPlotFrame {
  const float* render;         /* [3,H,W] */
  const float* gt_image;       /* [3,H,W] */
  const float* depth;          /* [H,W] rendered depth */
  const float* gt_depth;       /* [H,W] */
  const float* exposure_a;     /* device scalar, or NULL */
  const float* exposure_b;     /* device scalar, or NULL */
  char heading[SGR_PLOT_TEXT];
  char titles[6 * SGR_PLOT_TEXT];    /* cell (r, c) at 64 (3 r + c) */
} SgrPlotFrame;
void sgr_plot_panel_size(int32_t H, int32_t W, int32_t s, SGR_HOST int32_t* PH, SGR_HOST int32_t* PW);
size_t sgr_plot_scratch_bytes(int32_t n);
int sgr_plot_panels(int32_t n, const SgrPlotFrame* frames, int32_t H, int32_t W, int32_t s, float global_scale, float depth_max,
                    uint8_t* panels, void* scratch, size_t scratch_bytes, void* stream);

/* Exposure fit of the novel-view evaluation ("Novel-view evaluation"; the reference scores mapped keyframes only
 * and has no counterpart).  For each of 1 <= n <= SGR_EXPOSURE_FIT_MAX_FRAMES rows of the host table `frames`, of which render and
 * gt_image [C,H,W] are read and the other fields ignored, the gain g and bias b that minimise
 *   sum over the elements with gt_image > 0 of (g render + b - gt_image)^2        (the mask of sgr_render_metrics' PSNR)
 * from the six fp64 sums m (the mask count), S_r, S_t, S_rr, S_rt, S_tt (r = render, t = gt_image; every term formed in fp64):
 *   det = m S_rr - S_r^2,   g = (m S_rt - S_r S_t) / det,   b = (S_t - g S_r) / m;   ab[2 f] = log g, ab[2 f + 1] = b.
 * flags[f] = 1 and ab[2 f] = ab[2 f + 1] = 0 (the identity) where m < 2, or det <= 0 or det is not above m^2 2^-40 max(S_rr / m, 1)
 * (a render that is constant on the mask), or g is <= 0 or not finite, or a value would not be finite as fp32; else flags[f] = 0.
 * Nothing that is not finite is written.  A caller points exposure_a / exposure_b of row f at ab + 2 f and ab + 2 f + 1 and hands the
 * same table to sgr_render_metrics, sgr_lpips_pack and sgr_plot_panels behind this call on the same stream.
 * SGR_EXPOSURE_FIT_LAUNCHES launches, stream-ordered, no allocation, no float atomics; the order of every addition is fixed (per lane,
 * across the wave, the waves left to right, then the workgroups in order), so a frame's result has the same bits alone and in any
 * batch.  scratch: sgr_exposure_fit_bytes(n, C, H, W) (0 = unsupported: n outside its range, a side < 1 or C H W > 2^30).
 * SGR_ERR_INVALID / SGR_ERR_WORKSPACE before anything is launched. */
#define SGR_EXPOSURE_FIT_MAX_FRAMES 16
#define SGR_EXPOSURE_FIT_LAUNCHES 2
size_t sgr_exposure_fit_bytes(int32_t n, int32_t C, int32_t H, int32_t W);
int sgr_exposure_fit(int32_t n, const SgrMetricFrame* frames, int32_t C, int32_t H, int32_t W, float* ab, int32_t* flags, void* scratch,
                     size_t scratch_bytes, void* stream);

/* SE3 ops, batched over n. Pose =(tx,ty,tz,qx,qy,qz,qw) as in lietorch / depth_video.py:69; tau = (rho, theta). */
int se3_exp(const float* tau, int64_t n, float* pose_out, void* stream);
int se3_log(const float* pose, int64_t n, float* tau_out, void* stream);
int se3_inv(const float* pose, int64_t n, float* pose_out, void* stream);
int se3_mul(const float* pose_a, const float* pose_b, int64_t n, float* pose_out, void* stream);
int se3_act(const float* pose, const float* pts, int64_t n, float* pts_out, void* stream);
int se3_adjT(const float* pose, const float* a, int64_t n, float* out, void* stream);
int se3_matrix(const float* pose, int64_t n, float* mat_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLAT_HIP_H_ */
