"""ctypes binding of libsplat_hip.so (C ABI declared in include/splat_hip.h).

There is deliberately no fallback: if the HIP library is missing or cannot be loaded the import of the
product path fails with a clear error (a silent CPU path would void every parity claim).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SPLAT_HIP_LIB: another BUILD of the same library, for A/B measurements of kernel changes -- scripts/micro/ab_hash.py)
LIB_PATH = os.environ.get("SPLAT_HIP_LIB") or os.path.join(_HERE, "lib", "libsplat_hip.so")

SGR_OPT_FUSED_BLEND = 0
SGR_OPT_UPSTREAM_POSE_JACOBIAN = 1
SGR_OPT_SEGMENT_TEST = 2
SGR_OK, SGR_ERR_INVALID, SGR_ERR_WORKSPACE, SGR_ERR_CAPACITY, SGR_ERR_HIP = 0, -1, -2, -3, -4

_fp = C.c_void_p


class SgrSettings(C.Structure):
    _fields_ = [("num_gaussians", C.c_int32), ("image_height", C.c_int32), ("image_width", C.c_int32),
                ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("scale_modifier", C.c_float), ("prefiltered", C.c_int32), ("debug", C.c_int32),
                ("bg", _fp), ("viewmatrix", _fp), ("projmatrix", _fp), ("projmatrix_raw", _fp), ("campos", _fp)]


class SgrInputs(C.Structure):
    _fields_ = [("means3D", _fp), ("opacities", _fp), ("shs", _fp), ("colors_precomp", _fp), ("scales", _fp),
                ("rotations", _fp), ("cov3D_precomp", _fp)]


class SgrOutputs(C.Structure):
    _fields_ = [("color", _fp), ("depth", _fp), ("opacity", _fp), ("radii", _fp), ("n_touched", _fp)]


class SgrWorkspace(C.Structure):
    _fields_ = [("saved", _fp), ("saved_bytes", C.c_size_t), ("scratch", _fp), ("scratch_bytes", C.c_size_t),
                ("capacity", C.c_int64), ("counters_clean", C.c_int32), ("max_list_hint", C.c_int32)]


class SgrGradOutputs(C.Structure):
    _fields_ = [("dL_dcolor", _fp), ("dL_ddepth", _fp)]


class SgrGradInputs(C.Structure):
    _fields_ = [("dL_dmeans3D", _fp), ("dL_dmeans2D", _fp), ("dL_dopacities", _fp), ("dL_dshs", _fp),
                ("dL_dcolors_precomp", _fp), ("dL_dscales", _fp), ("dL_drotations", _fp), ("dL_dcov3D_precomp", _fp),
                ("dL_dtau", _fp), ("accumulate", C.c_int32), ("stat_grad_accum", _fp), ("stat_denom", _fp),
                ("stat_max_radii", _fp)]


class SgrMapView(C.Structure):
    _fields_ = [("settings", SgrSettings), ("out", SgrOutputs), ("ws", SgrWorkspace), ("gt_image", _fp), ("gt_depth", _fp),
                ("exposure_a", _fp), ("exposure_b", _fp), ("loss", _fp), ("dL_dimage", _fp), ("dL_ddepth", _fp),
                ("dL_dexposure", _fp), ("dL_dtau", _fp), ("loss_scratch", _fp), ("loss_scratch_bytes", C.c_size_t)]


class SgrBackwardView(C.Structure):
    _fields_ = [("settings", SgrSettings), ("radii", _fp), ("ws", SgrWorkspace), ("dL_dcolor", _fp), ("dL_ddepth", _fp),
                ("dL_dmeans2D", _fp), ("dL_dtau", _fp)]


class SgrAdamGroup(C.Structure):
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp), ("lr", C.c_float), ("skip", C.c_int32),
                ("step", C.c_int64)]


class SgrAdamTensor(C.Structure):
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp), ("n", C.c_int64), ("step", C.c_int64)]


class SgrMapStep(C.Structure):
    _fields_ = [("num_gaussians", C.c_int64), ("scaling", _fp), ("rotation", _fp), ("opacity", _fp), ("scales_out", _fp),
                ("rot_out", _fp), ("opac_out", _fp), ("num_views", C.c_int32), ("forward_only", C.c_int32),
                ("views", C.POINTER(SgrMapView)), ("in_", C.POINTER(SgrInputs)), ("grads", C.POINTER(SgrGradInputs)),
                ("alpha", C.c_float), ("rgb_boundary_threshold", C.c_float), ("adam_groups", C.POINTER(SgrAdamGroup)),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("iso_weight", C.c_float),
                ("exp_rows", C.c_int32), ("exp_row_width", C.c_int32), ("exp_param", _fp), ("exp_grad", _fp),
                ("exp_avg", _fp), ("exp_avg_sq", _fp), ("exp_step", _fp), ("exp_active", _fp), ("exp_lr", C.c_float),
                ("exp_beta1", C.c_float), ("exp_beta2", C.c_float), ("exp_eps", C.c_float), ("grads_clean", C.c_int32)]


class SgrMapRun(C.Structure):
    _fields_ = [("step", SgrMapStep), ("num_iters", C.c_int32), ("num_window", C.c_int32), ("window", C.POINTER(SgrMapView)),
                ("pool_size", C.c_int32), ("picks_per_iter", C.c_int32), ("pool", C.POINTER(SgrMapView)),
                ("picks", C.POINTER(C.c_int32)), ("lr0", C.POINTER(C.c_float)), ("adam_groups", C.POINTER(SgrAdamGroup)),
                ("pool_exp_row", C.POINTER(C.c_int32)), ("n_touched_last_only", C.c_int32), ("pick_ws", C.POINTER(SgrWorkspace))]


class SgrDeformFrame(C.Structure):
    _fields_ = [("frame_idx", C.c_int32), ("rigid", C.c_int32), ("w2c_old", C.c_float * 16), ("c2w_old", C.c_float * 16),
                ("transform", C.c_float * 16), ("quat_wxyz", C.c_float * 4), ("intrinsics", C.c_float * 9),
                ("height", C.c_int32), ("width", C.c_int32), ("depth_new", _fp), ("depth_old", _fp)]


class SgrMetricFrame(C.Structure):
    _fields_ = [("render", _fp), ("gt_image", _fp), ("depth", _fp), ("gt_depth", _fp), ("exposure_a", _fp), ("exposure_b", _fp)]


class SgrSsimTerm(C.Structure):
    _fields_ = [("lambda_dssim", C.c_float), ("max_views", C.c_int32), ("arena", _fp), ("arena_bytes", C.c_size_t)]


class SgrTsdfVolume(C.Structure):
    _fields_ = [("voxel_length", C.c_float), ("sdf_trunc", C.c_float), ("depth_trunc", C.c_float), ("hash_capacity", C.c_int32),
                ("pool_capacity", C.c_int32), ("state", _fp), ("pool", _fp)]


class SgrTsdfFrame(C.Structure):
    _fields_ = [("render", _fp), ("depth", _fp), ("gt_depth", _fp), ("exposure_a", _fp), ("exposure_b", _fp), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("w2c", C.c_float * 16), ("global_scale", C.c_float)]


SGR_TSDF_UNIT_FLOATS = 5 * 4096
SGR_TSDF_MAX_FRAMES = 16


class SgrRowTensor(C.Structure):
    _fields_ = [("in_", _fp), ("out", _fp), ("row_bytes", C.c_int32)]


class SgrDbaProblem(C.Structure):
    _fields_ = [("poses", _fp), ("num_poses", C.c_int32), ("disps", _fp), ("num_frames", C.c_int32), ("ht", C.c_int32),
                ("wd", C.c_int32), ("intrinsics", _fp), ("disps_sens", _fp), ("targets", _fp), ("weights", _fp), ("eta", _fp),
                ("ii", _fp), ("jj", _fp), ("num_edges", C.c_int32), ("num_depth", C.c_int32), ("t0", C.c_int32), ("t1", C.c_int32),
                ("iterations", C.c_int32), ("lm", C.c_float), ("ep", C.c_float), ("motion_only", C.c_int32),
                ("depth_only", C.c_int32), ("dx", _fp), ("dz", _fp)]


class SgrDspoProblem(C.Structure):
    _fields_ = [("poses", _fp), ("num_poses", C.c_int32), ("disps", _fp), ("num_frames", C.c_int32), ("ht", C.c_int32),
                ("wd", C.c_int32), ("intrinsics", _fp), ("mono_disps", _fp), ("valid_depth_mask", _fp), ("scales", _fp),
                ("shifts", _fp), ("targets", _fp), ("weights", _fp), ("eta", _fp), ("ii", _fp), ("jj", _fp), ("edge_keep", _fp),
                ("num_edges", C.c_int32), ("num_depth", C.c_int32), ("ignore_frames", C.c_int32), ("iterations", C.c_int32),
                ("lm", C.c_float), ("ep", C.c_float), ("alpha", C.c_float), ("dwq", _fp), ("dz", _fp)]


class SgrUpdateTensor(C.Structure):
    _fields_ = [("data", _fp), ("stride", C.c_int64 * 4), ("dtype", C.c_int32)]


class SgrUpdateConv(C.Structure):
    _fields_ = [("src0", _fp), ("src1", _fp), ("stride0", C.c_int32), ("stride1", C.c_int32), ("split", C.c_int32), ("cin", C.c_int32),
                ("ksize", C.c_int32), ("E", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("weight", _fp), ("weight_elems", C.c_int64),
                ("bias", _fp), ("cout", C.c_int32), ("act", C.c_int32), ("eadd", _fp), ("eadd_stride", C.c_int32), ("aux0", _fp),
                ("aux1", _fp), ("aux0_stride", C.c_int32), ("aux1_stride", C.c_int32), ("out", _fp), ("out2", _fp),
                ("out_kind", C.c_int32), ("out_stride", C.c_int32), ("out2_stride", C.c_int32)]


class SgrUpdateLayer(C.Structure):
    _fields_ = [("weight", _fp), ("weight_elems", C.c_int64), ("bias", _fp)]


SGR_UPDATE_LAYERS, SGR_UPDATE_LAUNCHES = 14, 17


class SgrUpdateWeights(C.Structure):
    _fields_ = [("layer", SgrUpdateLayer * SGR_UPDATE_LAYERS), ("glo_weight", _fp), ("glo_bias", _fp)]


class SgrUpdateCall(C.Structure):
    _fields_ = [("net", SgrUpdateTensor), ("inp", SgrUpdateTensor), ("corr", SgrUpdateTensor), ("flow", SgrUpdateTensor),
                ("E", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("K", C.c_int32), ("ix", _fp), ("net_out", _fp), ("delta", _fp),
                ("weight", _fp), ("eta", _fp), ("upmask", _fp), ("first_launch", C.c_int32), ("last_launch", C.c_int32)]


class SgrEncoderConv(C.Structure):
    _fields_ = [("src", _fp), ("src_stride", C.c_int32), ("cin", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32), ("n", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("weight", _fp), ("weight_elems", C.c_int64), ("bias", _fp), ("cout", C.c_int32),
                ("norm", C.c_int32), ("act", C.c_int32), ("residual", _fp), ("residual_stride", C.c_int32), ("out", _fp), ("out2", _fp),
                ("out_kind", C.c_int32), ("out_stride", C.c_int32), ("raw", _fp), ("raw_elems", C.c_int64), ("stats", _fp),
                ("stats_elems", C.c_int64)]


SGR_ENCODER_LAYERS = 16
SGR_ENCODER_LAUNCHES = {0: 17, 1: 32}       # by norm


class SgrEncoderWeights(C.Structure):
    _fields_ = [("layer", SgrUpdateLayer * SGR_ENCODER_LAYERS), ("out_dim", C.c_int32), ("norm", C.c_int32)]


class SgrEncoderCall(C.Structure):
    _fields_ = [("images", SgrUpdateTensor), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("normalize", C.c_int32),
                ("mean", C.c_float * 3), ("std_", C.c_float * 3), ("out", _fp), ("out2", _fp), ("split", C.c_int32),
                ("first_launch", C.c_int32), ("last_launch", C.c_int32)]


class SgrVitGemm(C.Structure):
    _fields_ = [("a", _fp), ("w", _fp), ("bias", _fp), ("lda", C.c_int64), ("ldw", C.c_int64), ("ldo", C.c_int64), ("M", C.c_int32),
                ("N", C.c_int32), ("K", C.c_int32), ("epi", C.c_int32), ("out", _fp), ("tap", _fp), ("aux", _fp), ("T", C.c_int32)]


class SgrVitBlock(C.Structure):
    _fields_ = [(n, _fp) for n in ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w",
                                   "fc2_b")]


class SgrVitWeights(C.Structure):
    _fields_ = [("dim", C.c_int32), ("heads", C.c_int32), ("depth", C.c_int32), ("cin", C.c_int32), ("tap", C.c_int32 * 2),
                ("embed_w", _fp), ("embed_b", _fp), ("blocks", C.POINTER(SgrVitBlock)), ("readout_w", _fp * 2), ("readout_b", _fp * 2)]


class SgrVitCall(C.Structure):
    _fields_ = [("patches", _fp), ("B", C.c_int32), ("gh", C.c_int32), ("gw", C.c_int32), ("pos", _fp), ("out", _fp * 2),
                ("first_launch", C.c_int32), ("last_launch", C.c_int32)]


class SgrResnetConv(C.Structure):
    _fields_ = [("src", _fp), ("src_stride", C.c_int32), ("cin", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32), ("n", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("pad_top", C.c_int32), ("pad_left", C.c_int32), ("ho", C.c_int32), ("wo", C.c_int32),
                ("weight", _fp), ("weight_elems", C.c_int64), ("bias", _fp), ("cout", C.c_int32), ("norm", C.c_int32), ("act", C.c_int32),
                ("groups", C.c_int32), ("out", _fp), ("out_kind", C.c_int32), ("out_stride", C.c_int32), ("raw", _fp),
                ("raw_elems", C.c_int64), ("stats", _fp), ("stats_elems", C.c_int64)]


class SgrResnetNorm(C.Structure):
    _fields_ = [("raw", _fp), ("stats", _fp), ("n", C.c_int32), ("hw", C.c_int32), ("cout", C.c_int32), ("groups", C.c_int32),
                ("relu", C.c_int32), ("gamma", _fp), ("beta", _fp), ("residual", _fp), ("residual_stride", C.c_int32), ("out", _fp),
                ("out_stride", C.c_int32)]


class SgrResnetLayer(C.Structure):
    _fields_ = [("weight", _fp), ("weight_elems", C.c_int64), ("gamma", _fp), ("beta", _fp)]


class SgrResnetWeights(C.Structure):
    _fields_ = [("stem_chs", C.c_int32), ("stage_chs", C.c_int32 * 3), ("stage_blocks", C.c_int32 * 3), ("groups", C.c_int32),
                ("num_layers", C.c_int32), ("layers", C.POINTER(SgrResnetLayer))]


class SgrResnetCall(C.Structure):
    _fields_ = [("images", SgrUpdateTensor), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("normalize", C.c_int32),
                ("mean", C.c_float * 3), ("std_", C.c_float * 3), ("l1", _fp), ("l2", _fp), ("l3", _fp), ("first_launch", C.c_int32),
                ("last_launch", C.c_int32)]


SGR_DPT_LAYERS, SGR_DPT_LAUNCHES = 28, 35


class SgrDptConv(C.Structure):
    _fields_ = [("src", _fp), ("src_stride", C.c_int32), ("cin", C.c_int32), ("ksize", C.c_int32), ("n", C.c_int32), ("h", C.c_int32),
                ("w", C.c_int32), ("weight", _fp), ("weight_elems", C.c_int64), ("bias", _fp), ("cout", C.c_int32), ("relu_in", C.c_int32),
                ("relu", C.c_int32), ("res0", _fp), ("res1", _fp), ("res0_stride", C.c_int32), ("res1_stride", C.c_int32), ("out", _fp),
                ("out_kind", C.c_int32), ("out_stride", C.c_int32)]


class SgrDptWeights(C.Structure):
    _fields_ = [("dim", C.c_int32), ("features", C.c_int32), ("chs0", C.c_int32), ("chs1", C.c_int32),
                ("layer", SgrUpdateLayer * SGR_DPT_LAYERS)]


class SgrDptCall(C.Structure):
    _fields_ = [("tap3", SgrUpdateTensor), ("tap4", SgrUpdateTensor), ("l1", _fp), ("l2", _fp), ("n", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("depth", _fp), ("first_launch", C.c_int32), ("last_launch", C.c_int32)]


SGR_LPIPS_MAX_PAIRS, SGR_LPIPS_DIST_PIXELS, SGR_LPIPS_LAUNCHES = 16, 128, 14


class SgrLpipsConv(C.Structure):
    _fields_ = [("src", _fp), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("cin", C.c_int32), ("ksize", C.c_int32),
                ("stride", C.c_int32), ("pad", C.c_int32), ("weight", _fp), ("weight_elems", C.c_int64), ("bias", _fp), ("cout", C.c_int32),
                ("out", _fp)]


class SgrLpipsWeights(C.Structure):
    _fields_ = [("conv", SgrUpdateLayer * 5), ("lin", _fp * 5), ("shift", C.c_float * 3), ("scale", C.c_float * 3)]


class SgrLpipsCall(C.Structure):
    _fields_ = [("frames", C.POINTER(SgrMetricFrame)), ("img0", _fp), ("img1", _fp), ("normalize", C.c_int32), ("n", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("out", _fp), ("levels", _fp), ("first_launch", C.c_int32), ("last_launch", C.c_int32)]


SGR_RESNET_NORM_NONE, SGR_RESNET_NORM_GROUP = 0, 1
SGR_RESNET_ACTS = {"none": 0, "relu": 1}
SGR_VIT_EPI = {"store_f16": 1, "gelu_f16": 2, "residual": 3, "readout": 4, "embed": 5, "store_f32": 6}
SGR_ENCODER_NORM_NONE, SGR_ENCODER_NORM_INSTANCE = 0, 1
SGR_ENCODER_ACTS = {"none": 0, "relu": 1, "split": 2}
SGR_UPDATE_OUT_CL_F16, SGR_UPDATE_OUT_CL_F32 = 0, 1
SGR_UPDATE_F32, SGR_UPDATE_F16 = 0, 1
SGR_UPDATE_ACTS = {"none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}
SGR_UPDATE_OUT_NCHW_F16, SGR_UPDATE_OUT_NCHW_F32 = 2, 3
SGR_DBA_MAX_WINDOW = 512
SGR_DSPO_WEIGHTS_NONE, SGR_DSPO_WEIGHTS_F32, SGR_DSPO_WEIGHTS_U8 = 0, 1, 2
SGR_CORR_F32, SGR_CORR_F16 = 0, 1
SGR_VIDEO_MASK_F32, SGR_VIDEO_MASK_F16 = 0, 1
SGR_VIDEO_MAX_FRAMES = 65535
SGR_FUSE_MAX_FRAMES = 65535
SGR_CORR_MAX_RADIUS = 1023
SGR_CORR_PYRAMID_MAX_RADIUS, SGR_CORR_PYRAMID_MAX_LEVELS = 4, 4
SGR_CORR_VOLUME_CHANNEL_STEP, SGR_CORR_VOLUME_MAX_CHANNELS, SGR_CORR_VOLUME_MAX_EDGES = 32, 1024, 65535
SGR_GRAPH_MAX_EDGES = 65535
SGR_GRAPH_MAX_SIDE = 512


# name -> (restype, argtypes); must list every symbol include/splat_hip.h declares (tests/test_abi.py checks)
SIGNATURES = {
    "sgr_abi_version": (C.c_int, []),
    "sgr_last_error": (C.c_char_p, []),
    "sgr_saved_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "sgr_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "sgr_forward": (C.c_int, [C.POINTER(SgrSettings), C.POINTER(SgrInputs), C.POINTER(SgrOutputs),
                              C.POINTER(SgrWorkspace), C.POINTER(C.c_int64), _fp]),
    "sgr_backward": (C.c_int, [C.POINTER(SgrSettings), C.POINTER(SgrInputs), _fp, C.POINTER(SgrGradOutputs),
                               C.POINTER(SgrGradInputs), C.POINTER(SgrWorkspace), _fp]),
    "sgr_backward_views": (C.c_int, [C.c_int32, C.POINTER(SgrBackwardView), C.POINTER(SgrInputs), C.POINTER(SgrGradInputs), _fp]),
    "sgr_densify_stats": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp]),
    "sgr_query": (C.c_int, [_fp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _fp]),
    "sgr_query_header": (C.c_int, [_fp, C.POINTER(C.c_uint32), _fp]),
    "sgr_header_to_host": (C.c_int, [_fp, _fp, _fp]),
    "sgr_query_stats": (C.c_int, [C.POINTER(SgrWorkspace), C.c_int32, C.c_int32, C.c_int32, _fp, C.POINTER(C.c_int64), _fp]),
    "sgr_query_depth_keys": (C.c_int, [C.POINTER(SgrWorkspace), C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp]),
    "sgr_query_list_histogram": (C.c_int, [C.POINTER(SgrWorkspace), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), _fp]),
    "sgr_set_option": (C.c_int, [C.c_int32, C.c_int32]),
    "sgr_get_option": (C.c_int, [C.c_int32]),
    "sgr_profile_enable": (C.c_int, [C.c_uint32]),
    "sgr_profile_read": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "sgr_mapping_loss": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, C.c_float, C.c_float,
                                   C.c_float, _fp, _fp, _fp, _fp, _fp, _fp, C.c_size_t, _fp]),
    "sgr_ssim_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "sgr_ssim": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, C.c_size_t, _fp]),
    "sgr_ssim_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, C.c_int32, C.c_float, _fp, _fp]),
    "sgr_render_metrics": (C.c_int, [C.c_int32, C.POINTER(SgrMetricFrame), C.c_int32, C.c_int32, C.c_int32, C.c_float, _fp, _fp,
                                     C.c_size_t, _fp]),
    "sgr_tsdf_bytes": (C.c_size_t, [C.c_int32]),
    "sgr_tsdf_reset": (C.c_int, [C.POINTER(SgrTsdfVolume), _fp]),
    "sgr_tsdf_rehash": (C.c_int, [C.POINTER(SgrTsdfVolume), C.POINTER(SgrTsdfVolume), _fp]),
    "sgr_tsdf_touch": (C.c_int, [C.POINTER(SgrTsdfVolume), C.c_int32, C.POINTER(SgrTsdfFrame), C.c_int32, C.c_int32, _fp]),
    "sgr_tsdf_integrate": (C.c_int, [C.POINTER(SgrTsdfVolume), C.c_int32, C.POINTER(SgrTsdfFrame), C.c_int32, C.c_int32,
                                     C.c_int32, _fp]),
    "sgr_tsdf_extract_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "sgr_tsdf_extract_count": (C.c_int, [C.POINTER(SgrTsdfVolume), C.c_int32, _fp, C.c_size_t, _fp, _fp]),
    "sgr_tsdf_extract": (C.c_int, [C.POINTER(SgrTsdfVolume), C.c_int32, _fp, C.c_size_t, _fp, _fp, _fp, _fp]),
    "sgr_mesh_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "sgr_mesh_components": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp, C.c_size_t, _fp, _fp]),
    "sgr_mesh_compact": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, C.c_size_t, _fp, _fp, _fp, _fp, _fp]),
    "sgr_surface_sample_bytes": (C.c_size_t, [C.c_int32]),
    "sgr_surface_sample": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, C.c_int32, C.c_uint64, _fp, C.c_size_t, _fp, _fp, _fp, _fp]),
    "sgr_nn_grid_bytes": (C.c_size_t, [C.c_int32]),
    "sgr_nn_grid_build": (C.c_int, [C.c_int32, _fp, C.POINTER(C.c_float), _fp, C.c_size_t, _fp]),
    "sgr_nn_query": (C.c_int, [C.c_int32, _fp, C.c_size_t, C.c_int32, _fp, C.POINTER(C.c_float), C.c_float, _fp, _fp, _fp]),
    "sgr_eval_reduce_bytes": (C.c_size_t, []),
    "sgr_icp_accumulate": (C.c_int, [C.c_int32, _fp, C.POINTER(C.c_float), _fp, C.c_int32, _fp, _fp, _fp, C.c_size_t, _fp]),
    "sgr_cloud_metrics": (C.c_int, [C.c_int32, _fp, C.c_int32, _fp, C.c_float, _fp, _fp, C.c_size_t, _fp]),
    "sgr_adam_step": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float, C.c_float,
                                C.c_int64, _fp]),
    "sgr_adam_step_multi": (C.c_int, [C.c_int32, C.POINTER(SgrAdamTensor), C.c_float, C.c_float, C.c_float, C.c_float, _fp]),
    "sgr_activate": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "sgr_gaussian_adam_step": (C.c_int, [C.c_int64, C.POINTER(SgrAdamGroup), C.c_float, C.c_float, C.c_float, C.c_float, _fp]),
    "sgr_gaussian_adam_shard": (C.c_int, [C.c_int64, C.POINTER(SgrAdamGroup), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.c_float, C.c_float, C.c_float, C.c_float, _fp]),
    "sgr_map_views": (C.c_int, [C.c_int32, C.POINTER(SgrMapView), C.POINTER(SgrInputs), C.POINTER(SgrGradInputs),
                                C.c_float, C.c_float, C.c_int32, _fp]),
    "sgr_map_step": (C.c_int, [C.POINTER(SgrMapStep), _fp]),
    "sgr_map_run": (C.c_int, [C.POINTER(SgrMapRun), _fp]),
    "sgr_ssim_term_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "sgr_mapping_loss_ssim": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float,
                                        C.POINTER(SgrSsimTerm), _fp, _fp, _fp, _fp, _fp, _fp]),
    "sgr_map_step_ssim": (C.c_int, [C.POINTER(SgrMapStep), C.POINTER(SgrSsimTerm), _fp]),
    "sgr_map_run_ssim": (C.c_int, [C.POINTER(SgrMapRun), C.POINTER(SgrSsimTerm), _fp]),
    "sgr_masked_adam": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float,
                                  C.c_float, _fp]),
    "sgr_deform_points": (C.c_int, [C.c_int64, _fp, C.POINTER(SgrDeformFrame), _fp, _fp, _fp, _fp]),
    "sgr_compact_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "sgr_keep_list": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, C.c_size_t, _fp]),
    "sgr_gather_rows": (C.c_int, [C.c_int64, _fp, C.c_int32, C.POINTER(SgrRowTensor), _fp]),
    "sknn_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "sknn_dist2": (C.c_int, [_fp, C.c_int32, _fp, _fp, C.c_size_t, _fp]),
    "sgr_dba_scratch_bytes": (C.c_size_t, [C.c_int32] * 6),
    "sgr_dba_ba": (C.c_int, [C.POINTER(SgrDbaProblem), _fp, C.c_size_t, _fp]),
    "sgr_dba_frame_distance": (C.c_int, [_fp, C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_int32, C.c_float,
                                         _fp, _fp]),
    "sgr_dba_projmap": (C.c_int, [_fp, C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_int32, _fp, _fp, _fp]),
    "sgr_dba_iproj": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp]),
    "sgr_dba_depth_filter": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp, _fp]),
    "sgr_dspo_align": (C.c_int, [_fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "sgr_dspo_scratch_bytes": (C.c_size_t, [C.c_int32] * 5),
    "sgr_dspo_ba": (C.c_int, [C.POINTER(SgrDspoProblem), _fp, C.c_size_t, _fp]),
    "sgr_video_cvx_upsample": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, _fp, C.c_int32, _fp, _fp]),
    "sgr_video_depth_thresh": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, C.c_float, _fp, _fp]),
    "sgr_video_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "sgr_video_mask_from_counts": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, _fp, C.c_int32, _fp, _fp, C.c_size_t,
                                             _fp]),
    "sgr_video_valid_mask": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, C.c_float, C.c_int32, _fp, _fp,
                                       C.c_size_t, _fp]),
    "sgr_fuse_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "sgr_fuse_prepare": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_size_t, _fp]),
    "sgr_fuse_depth": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp,
                                 C.c_size_t, _fp]),
    "sgr_corr_index_forward": (C.c_int, [_fp, _fp, _fp] + [C.c_int32] * 7 + [_fp]),
    "sgr_corr_index_backward": (C.c_int, [_fp, _fp, _fp] + [C.c_int32] * 7 + [_fp]),
    "sgr_corr_alt_forward": (C.c_int, [_fp, _fp, _fp, _fp] + [C.c_int32] * 8 + [_fp]),
    "sgr_corr_alt_backward": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp] + [C.c_int32] * 8 + [_fp]),
    "sgr_corr_alt_pyramid_forward": (C.c_int, [_fp] * 8 + [C.c_int32] * 8 + [_fp]),
    "sgr_corr_volume_pyramid": (C.c_int, [_fp] * 8 + [C.c_int32] * 7 + [_fp]),
    "sgr_corr_index_pyramid_forward": (C.c_int, [_fp] * 7 + [C.c_int32] * 6 + [_fp]),
    "sgr_graph_reproject": (C.c_int, [_fp, C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_int32, _fp, _fp, _fp, _fp,
                                      _fp]),
    "sgr_graph_select_scratch_bytes": (C.c_size_t, [C.c_int32] * 2),
    "sgr_graph_select_proximity": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                             C.c_int32, _fp, C.c_int32, _fp, _fp, C.c_size_t, _fp]),
    "sgr_graph_select_backend": (C.c_int, [_fp] + [C.c_int32] * 6 + [C.c_float, C.c_int32, _fp, C.c_int32, _fp, _fp, C.c_size_t, _fp]),
    "sgr_update_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "sgr_update_pack": (C.c_int, [C.POINTER(SgrUpdateTensor)] + [C.c_int32] * 4 + [_fp, C.c_int32, C.c_int32, _fp]),
    "sgr_update_conv": (C.c_int, [C.POINTER(SgrUpdateConv), _fp]),
    "sgr_update_forward": (C.c_int, [C.POINTER(SgrUpdateWeights), C.POINTER(SgrUpdateCall), _fp, C.c_size_t, _fp]),
    "sgr_encoder_scratch_bytes": (C.c_size_t, [C.c_int32] * 5),
    "sgr_encoder_pack": (C.c_int, [C.POINTER(SgrUpdateTensor)] + [C.c_int32] * 3 + [C.POINTER(C.c_float), C.POINTER(C.c_float), _fp, _fp]),
    "sgr_encoder_conv": (C.c_int, [C.POINTER(SgrEncoderConv), _fp]),
    "sgr_encoder_forward": (C.c_int, [C.POINTER(SgrEncoderWeights), C.POINTER(SgrEncoderCall), _fp, C.c_size_t, _fp]),
    "sgr_vit_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "sgr_vit_layernorm": (C.c_int, [_fp, _fp, _fp, C.c_int64, C.c_int32, _fp, _fp]),
    "sgr_vit_gemm": (C.c_int, [C.POINTER(SgrVitGemm), _fp]),
    "sgr_vit_attention": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "sgr_vit_forward": (C.c_int, [C.POINTER(SgrVitWeights), C.POINTER(SgrVitCall), _fp, C.c_size_t, _fp]),
    "sgr_resnet_scratch_bytes": (C.c_size_t, [C.c_int32] * 7),
    "sgr_resnet_conv": (C.c_int, [C.POINTER(SgrResnetConv), _fp]),
    "sgr_resnet_stats": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "sgr_resnet_groupnorm": (C.c_int, [C.POINTER(SgrResnetNorm), _fp]),
    "sgr_resnet_maxpool": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "sgr_resnet_forward": (C.c_int, [C.POINTER(SgrResnetWeights), C.POINTER(SgrResnetCall), _fp, C.c_size_t, _fp]),
    "sgr_dpt_scratch_bytes": (C.c_size_t, [C.c_int32] * 5),
    "sgr_dpt_conv": (C.c_int, [C.POINTER(SgrDptConv), _fp]),
    "sgr_dpt_up2": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, _fp]),
    "sgr_dpt_resize_in": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, C.c_int32, _fp]),
    "sgr_dpt_resize_out": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, C.c_int32, _fp]),
    "sgr_dpt_forward": (C.c_int, [C.POINTER(SgrDptWeights), C.POINTER(SgrDptCall), _fp, C.c_size_t, _fp]),
    "sgr_lpips_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "sgr_lpips_pack": (C.c_int, [C.c_int32, C.POINTER(SgrMetricFrame), C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                 _fp, _fp]),
    "sgr_lpips_pack_pairs": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       _fp, _fp]),
    "sgr_lpips_conv": (C.c_int, [C.POINTER(SgrLpipsConv), _fp]),
    "sgr_lpips_maxpool": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "sgr_lpips_distance": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp]),
    "sgr_lpips_forward": (C.c_int, [C.POINTER(SgrLpipsWeights), C.POINTER(SgrLpipsCall), _fp, C.c_size_t, _fp]),
    "se3_exp": (C.c_int, [_fp, C.c_int64, _fp, _fp]),
    "se3_log": (C.c_int, [_fp, C.c_int64, _fp, _fp]),
    "se3_inv": (C.c_int, [_fp, C.c_int64, _fp, _fp]),
    "se3_mul": (C.c_int, [_fp, _fp, C.c_int64, _fp, _fp]),
    "se3_act": (C.c_int, [_fp, _fp, C.c_int64, _fp, _fp]),
    "se3_adjT": (C.c_int, [_fp, _fp, C.c_int64, _fp, _fp]),
    "se3_matrix": (C.c_int, [_fp, C.c_int64, _fp, _fp]),
}

_lib = None


def lib():
    """Loads (once) and returns the ctypes handle.  Raises, never falls back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). splat_slam_amd has no CPU fallback by design.")
        # The caller's device memory and streams are torch's: load torch FIRST so that this process ends up with ONE HIP
        # runtime (torch's bundled libamdhip64). Loading /opt/rocm's copy first gives a second runtime that cannot see
        # the device ("no ROCm-capable device is detected").
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if h.sgr_abi_version() != 10:
            raise ImportError("libsplat_hip.so ABI version mismatch")
        _lib = h
    return _lib


def last_error():
    return lib().sgr_last_error().decode()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
