"""ctypes binding of libmoss_raster.so (the C ABI declared in include/moss_raster.h).

There is NO fallback: if the HIP library is missing the import of any op fails loudly.  PyTorch is used for
device memory and streams only; every tensor crosses the boundary as a raw device pointer.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# "lib" = the product build.  MOSS_AMD_LIB_DIR=lib_diag selects the DIAGNOSTIC build (python -m moss_amd.build --diag: -DMOSS_DIAG,
# environment knobs that pick kernel variants, stamp buffers) -- for the A/B scripts under scripts/, never for results.
_LIB_DIR = os.path.join(_HERE, os.environ.get("MOSS_AMD_LIB_DIR", "lib"))
LIB_PATH = os.path.join(_LIB_DIR, "libmoss_raster.so")
EXT_PATH = os.path.join(_LIB_DIR, "_moss_C.so")          # the compiled PyTorch extension (csrc/torch_binding.cpp) over the same C ABI
ABI_VERSION = 7                                          # include/moss_raster.h MOSS_ABI_VERSION this binding was written against

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

_lib = None
_lock = threading.Lock()

ERR_NAMES = {-1: "invalid argument", -2: "HIP error", -3: "allocation failed", -4: "prefiltered point culled", -5: "unsupported"}

_f = C.c_float
_d = C.c_double
_i = C.c_int
_p = C.c_void_p


def _declare(lib):
    lib.moss_abi_version.restype = _i
    lib.moss_last_error.restype = C.c_char_p
    lib.moss_raster_geometry_bytes.restype = C.c_size_t
    lib.moss_raster_geometry_bytes.argtypes = [_i]
    lib.moss_raster_image_bytes.restype = C.c_size_t
    lib.moss_raster_image_bytes.argtypes = [_i, _i]
    lib.moss_raster_binning_bytes.restype = C.c_size_t
    lib.moss_raster_binning_bytes.argtypes = [_i]
    lib.moss_raster_binning_bytes_forward_only.restype = C.c_size_t
    lib.moss_raster_binning_bytes_forward_only.argtypes = [_i]
    lib.moss_raster_frame_state_bytes.restype = C.c_size_t
    lib.moss_raster_frame_state_bytes.argtypes = [_i, _i]
    lib.moss_build_has_diagnostics.restype = _i
    lib.moss_adamw_state_bytes.restype = C.c_size_t
    lib.moss_raster_read_status.restype = _i
    lib.moss_raster_read_status.argtypes = [_p, _p, _p]
    lib.moss_raster_mark_visible.restype = _i
    lib.moss_raster_mark_visible.argtypes = [_i, _p, _p, _p, _p, _p]
    lib.moss_knn_workspace_bytes.restype = C.c_size_t
    lib.moss_knn_workspace_bytes.argtypes = [_i]
    lib.moss_knn_dist2.restype = _i
    lib.moss_knn_dist2.argtypes = [_i, _p, _p, _p, C.c_size_t, _p]
    lib.moss_knn_query.restype = _i
    lib.moss_knn_query.argtypes = [_i, _i, _i, _p, _p, _p, _p, _p]
    lib.moss_knn_grid_workspace_bytes.restype = C.c_size_t
    lib.moss_knn_grid_workspace_bytes.argtypes = [_i]
    lib.moss_knn_grid_build.restype = _i
    lib.moss_knn_grid_build.argtypes = [_i, _p, _p, C.c_size_t, _p]
    lib.moss_knn_grid_query.restype = _i
    lib.moss_knn_grid_query.argtypes = [_i, _i, _i, _p, C.c_size_t, _p, _p, _p, _p]
    lib.moss_nearest_vertex_index_bytes.restype = C.c_size_t
    lib.moss_nearest_vertex_index_bytes.argtypes = [_i]
    lib.moss_nearest_vertex_build.restype = _i
    lib.moss_nearest_vertex_build.argtypes = [_i, _p, _p, C.c_size_t, _p]
    lib.moss_nearest_vertex_query.restype = _i
    lib.moss_nearest_vertex_query.argtypes = [_i, _i, _p, C.c_size_t, _p, _p, _p, _p]
    lib.moss_densify_stats.restype = _i
    lib.moss_densify_stats.argtypes = [_i, _p, _p, _i, _p, _p, _p, _p]
    lib.moss_neighbour_kl.restype = _i
    lib.moss_neighbour_kl.argtypes = [_i, _i, _p, _p, _p, _p, _p, _p]
    lib.moss_densify_joint_table.restype = _i
    lib.moss_densify_joint_table.argtypes = [_p, _p, _p, _p]
    lib.moss_densify_select_workspace_bytes.restype = C.c_size_t
    lib.moss_densify_select_workspace_bytes.argtypes = [_i]
    lib.moss_densify_select.restype = _i
    lib.moss_densify_select.argtypes = [_p, _p]
    lib.moss_densify_emit.restype = _i
    lib.moss_densify_emit.argtypes = [_p, _p]
    lib.moss_rows_map_workspace_bytes.restype = C.c_size_t
    lib.moss_rows_map_workspace_bytes.argtypes = [_i]
    lib.moss_rows_keep_map.restype = _i
    lib.moss_rows_keep_map.argtypes = [_i, _p, _i, _p, _p, _p, C.c_size_t, _p]
    lib.moss_rows_relayout.restype = _i
    lib.moss_rows_relayout.argtypes = [_p, _p]
    lib.moss_loss_workspace_bytes.restype = C.c_size_t
    lib.moss_loss_workspace_bytes.argtypes = [_i, _i, _i]
    lib.moss_photometric_loss.restype = _i
    lib.moss_photometric_loss.argtypes = [_i, _i, _i, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, C.c_size_t, _p]
    lib.moss_photometric_loss_weighted.restype = _i
    lib.moss_photometric_loss_weighted.argtypes = [_i, _i, _i, _p, _p, _p, _p, _f, _f, _f, _p, _p, _p, _p, C.c_size_t, _p]
    lib.moss_adamw_multi.restype = _i
    lib.moss_adamw_multi.argtypes = [_p, _p]
    lib.moss_metrics_workspace_bytes.restype = C.c_size_t
    lib.moss_metrics_workspace_bytes.argtypes = [_i, _i, _i, _i]
    lib.moss_metrics_state_bytes.restype = C.c_size_t
    lib.moss_metrics_state_bytes.argtypes = []
    lib.moss_eval_metrics.restype = _i
    lib.moss_eval_metrics.argtypes = [_p, _p]
    lib.moss_frames_to_u8.restype = _i
    lib.moss_frames_to_u8.argtypes = [_p, _p]
    lib.moss_view_images_prepare.restype = _i
    lib.moss_view_images_prepare.argtypes = [_p, _p]
    lib.moss_view_images_load.restype = _i
    lib.moss_view_images_load.argtypes = [_p, _p]
    lib.moss_lbs_workspace_bytes.restype = C.c_size_t
    lib.moss_lbs_workspace_bytes.argtypes = [_i, _i]
    lib.moss_lbs_deform_forward.restype = _i
    lib.moss_lbs_deform_forward.argtypes = [_p, _p]
    lib.moss_lbs_deform_backward.restype = _i
    lib.moss_lbs_deform_backward.argtypes = [_p, _p]
    lib.moss_lbs_frame_workspace_bytes.restype = C.c_size_t
    lib.moss_lbs_frame_workspace_bytes.argtypes = [_i, _i]
    lib.moss_lbs_deform_backward_frame.restype = _i
    lib.moss_lbs_deform_backward_frame.argtypes = [_p, _p]
    lib.moss_smpl_frame_backward_pose.restype = _i
    lib.moss_smpl_frame_backward_pose.argtypes = [_p, _p]
    lib.moss_smpl_frame_workspace_bytes.restype = C.c_size_t
    lib.moss_smpl_frame_workspace_bytes.argtypes = [_i, _i, _i]
    lib.moss_smpl_frame_forward.restype = _i
    lib.moss_smpl_frame_forward.argtypes = [_p, _p]
    lib.moss_smpl_frame_backward.restype = _i
    lib.moss_smpl_frame_backward.argtypes = [_p, _p]
    lib.moss_smpl_vertices_workspace_bytes.restype = C.c_size_t
    lib.moss_smpl_vertices_workspace_bytes.argtypes = [_i, _i]
    lib.moss_smpl_vertices.restype = _i
    lib.moss_smpl_vertices.argtypes = [_p, _p]
    lib.moss_bound_mask_workspace_bytes.restype = C.c_size_t
    lib.moss_bound_mask_workspace_bytes.argtypes = [_i, _i, _i]
    lib.moss_bound_mask.restype = _i
    lib.moss_bound_mask.argtypes = [_p, _p]
    lib.moss_smpl_vertices_backward_workspace_bytes.restype = C.c_size_t
    lib.moss_smpl_vertices_backward_workspace_bytes.argtypes = [_i, _i]
    lib.moss_smpl_vertices_backward.restype = _i
    lib.moss_smpl_vertices_backward.argtypes = [_p, _p]
    lib.moss_keypoint_loss_workspace_bytes.restype = C.c_size_t
    lib.moss_keypoint_loss_workspace_bytes.argtypes = [_i, _i]
    lib.moss_keypoint_loss.restype = _i
    lib.moss_keypoint_loss.argtypes = [_p, _p]
    lib.moss_s3im_workspace_bytes.restype = C.c_size_t
    lib.moss_s3im_workspace_bytes.argtypes = [_i, _i, _i]
    lib.moss_s3im_loss.restype = _i
    lib.moss_s3im_loss.argtypes = [_i, _i, _i, _p, _p, _p, _i, _p, _p, _p, C.c_size_t, _p]
    lib.moss_pose_head_forward.restype = _i
    lib.moss_pose_head_forward.argtypes = [_p, _p]
    lib.moss_pose_head_backward.restype = _i
    lib.moss_pose_head_backward.argtypes = [_p, _p]
    lib.moss_matrix_fisher_nll.restype = _i
    lib.moss_matrix_fisher_nll.argtypes = [_i, _p, _p, _f, _p, _p, _p]
    lib.moss_lbs_weight_net_forward.restype = _i
    lib.moss_lbs_weight_net_forward.argtypes = [_p, _p]
    lib.moss_lbs_weight_net_backward.restype = _i
    lib.moss_lbs_weight_net_backward.argtypes = [_p, _p]
    lib.moss_lbs_weight_net_forward_bf16x3.restype = _i
    lib.moss_lbs_weight_net_forward_bf16x3.argtypes = [_p, _p]
    lib.moss_lbs_weight_net_backward_bf16x3.restype = _i
    lib.moss_lbs_weight_net_backward_bf16x3.argtypes = [_p, _p]
    lib.moss_lbs_weight_net_workspace_bytes.restype = C.c_size_t
    lib.moss_lbs_weight_net_workspace_bytes.argtypes = [_i]
    lib.moss_lbs_weight_net_saved_bytes.restype = C.c_size_t
    lib.moss_lbs_weight_net_saved_bytes.argtypes = [_i]
    lib.moss_lpips_vgg_forward.restype = _i
    lib.moss_lpips_vgg_forward.argtypes = [_p, _p]
    lib.moss_lpips_vgg_backward.restype = _i
    lib.moss_lpips_vgg_backward.argtypes = [_p, _p]
    lib.moss_lpips_vgg_workspace_bytes.restype = C.c_size_t
    lib.moss_lpips_vgg_workspace_bytes.argtypes = [_i, _i]
    lib.moss_lpips_vgg_saved_bytes.restype = C.c_size_t
    lib.moss_lpips_vgg_saved_bytes.argtypes = [_i, _i]
    lib.moss_lpips_vgg_pack_weights.restype = _i
    lib.moss_lpips_vgg_pack_weights.argtypes = [_i, _i, _p, _p, _p, _p]
    lib.moss_lpips_vgg_forward_bf16.restype = _i
    lib.moss_lpips_vgg_forward_bf16.argtypes = [_p, _p]
    lib.moss_lpips_vgg_backward_bf16.restype = _i
    lib.moss_lpips_vgg_backward_bf16.argtypes = [_p, _p]
    lib.moss_lpips_vgg_pack_weights_bf16.restype = _i
    lib.moss_lpips_vgg_pack_weights_bf16.argtypes = [_i, _i, _p, _p, _p, _p]
    lib.moss_lpips_vgg_conv3x3.restype = _i
    lib.moss_lpips_vgg_conv3x3.argtypes = [_p, _p]
    lib.moss_lpips_vgg_forward_bf16x3.restype = _i
    lib.moss_lpips_vgg_forward_bf16x3.argtypes = [_p, _p]
    lib.moss_lpips_vgg_backward_bf16x3.restype = _i
    lib.moss_lpips_vgg_backward_bf16x3.argtypes = [_p, _p]
    lib.moss_lpips_vgg_pack_weights_bf16x3.restype = _i
    lib.moss_lpips_vgg_pack_weights_bf16x3.argtypes = [_i, _i, _p, _p, _p, _p]
    lib.moss_lpips_vgg_conv3x3_bf16x3.restype = _i
    lib.moss_lpips_vgg_conv3x3_bf16x3.argtypes = [_p, _p]
    lib.moss_lpips_vgg_reference_bytes.restype = C.c_size_t
    lib.moss_lpips_vgg_reference_bytes.argtypes = [_i, _i]
    for suffix in ("", "_bf16", "_bf16x3"):
        for name in ("moss_lpips_vgg_reference", "moss_lpips_vgg_forward_ref"):
            fn = getattr(lib, name + suffix)
            fn.restype = _i
            fn.argtypes = [_p, _p]
    lib.moss_photometric_loss_roi.restype = _i
    lib.moss_photometric_loss_roi.argtypes = [_i, _i, _i, _p, _p, _p, _p, _p, _p, _f, _f, _f, _p, _p, _p, _p, C.c_size_t, _p]
    lib.moss_adamw_flat_ex.restype = _i
    lib.moss_adamw_flat_ex.argtypes = [_p, _p]
    lib.moss_gaussian_activate_forward.restype = _i
    lib.moss_gaussian_activate_forward.argtypes = [_i, _i] + [_p] * 12
    lib.moss_gaussian_activate_backward.restype = _i
    lib.moss_gaussian_activate_backward.argtypes = [_i, _i] + [_p] * 15
    lib.moss_raster_profile_enable.restype = None
    lib.moss_raster_profile_enable.argtypes = [C.c_uint32]
    lib.moss_raster_profile_read.restype = _i
    lib.moss_raster_profile_read.argtypes = [_p, _p]
    lib.moss_raster_export_geometry.restype = _i
    lib.moss_raster_export_geometry.argtypes = [_p, _i, _p, _p, _p, _p, _p, _p, _p, _p]
    lib.moss_raster_export_binning.restype = _i
    lib.moss_raster_export_binning.argtypes = [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p]


class FusedAdamWStruct(C.Structure):
    """``moss_fused_adamw`` of include/moss_raster.h (host struct handed to ``moss_raster_backward_ex`` as ``opt``, through the extension)."""
    _fields_ = [("tensors", C.c_uint32), ("exp_avg", C.c_void_p * 5), ("exp_avg_sq", C.c_void_p * 5), ("lr", C.c_float * 5),
                ("lr_sh_rest", C.c_float), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("step_state", C.c_void_p), ("lr_segment", C.c_int32 * 5), ("sh_active_degree", C.c_int32), ("sh_inactive_zero", C.c_int32)]


class AdamWFlatArgs(C.Structure):
    """``moss_adamw_flat_args`` of include/moss_raster.h (``moss_adamw_flat_ex``: every form of the flat update + the degree-aware SH update)."""
    _fields_ = [("first", C.c_longlong), ("count", C.c_longlong), ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p),
                ("exp_avg_sq", C.c_void_p), ("num_segments", C.c_int), ("segment_end", C.c_void_p), ("segment_lr", C.c_void_p),
                ("segment_period", C.c_void_p), ("segment_split", C.c_void_p), ("segment_lr2", C.c_void_p), ("segment_active", C.c_void_p),
                ("inactive_zero", C.c_int), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("step", C.c_int), ("step_state", C.c_void_p), ("skip_word", C.c_void_p), ("skip_mask", C.c_uint32),
                ("num_grads_extra", C.c_int), ("grads_extra", C.c_void_p * 3), ("grad_scale", C.c_float)]


class AdamWMultiArgs(C.Structure):
    """``moss_adamw_multi_args`` of include/moss_raster.h (``moss_adamw_multi``: up to eight tensors with buffers of their own, one launch)."""
    _fields_ = [("num_tensors", C.c_int32), ("numel", C.c_longlong * 8), ("params", C.c_void_p * 8), ("grads", C.c_void_p * 8),
                ("exp_avg", C.c_void_p * 8), ("exp_avg_sq", C.c_void_p * 8), ("lr", C.c_float * 8), ("step", C.c_int32 * 8),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float), ("weight_decay", C.c_float)]


class EvalMetricsArgs(C.Structure):
    """``moss_eval_metrics_args`` of include/moss_raster.h (``moss_eval_metrics``: the evaluation metrics of up to eight views, one call)."""
    _fields_ = [("num_views", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("image", C.c_void_p * 8),
                ("gt", C.c_void_p * 8), ("bound", C.c_void_p * 8), ("out_image", C.c_void_p * 8), ("fill", C.c_float),
                ("state", C.c_void_p), ("per_view", C.c_void_p), ("per_view_capacity", C.c_int32), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


class FramesToU8Args(C.Structure):
    """``moss_frames_to_u8_args`` of include/moss_raster.h (``moss_frames_to_u8``: up to eight float32 frames to 8-bit pixels, one launch)."""
    _fields_ = [("num_views", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels_out", C.c_int32), ("rounding", C.c_int32),
                ("image", C.c_void_p * 8), ("alpha", C.c_void_p * 8), ("bound", C.c_void_p * 8), ("fill", C.c_float),
                ("out", C.c_void_p * 8)]


class ViewImagesPrepareArgs(C.Structure):
    """``moss_view_images_prepare_args`` of include/moss_raster.h (``moss_view_images_prepare``: up to eight views' raw image and mask
    bytes to their packed 8-bit ground truth, one launch).  ``K[b]`` / ``D[b]`` are host doubles."""
    _fields_ = [("num_views", C.c_int32), ("H0", C.c_int32), ("W0", C.c_int32), ("scale", C.c_int32), ("background", C.c_int32),
                ("mask_mode", C.c_int32), ("rgb", C.c_void_p * 8), ("mask", C.c_void_p * 8), ("K", C.c_double * 9 * 8),
                ("D", C.c_double * 5 * 8), ("gt_u8", C.c_void_p * 8), ("bkgd_u8", C.c_void_p * 8)]


class ViewImagesLoadArgs(C.Structure):
    """``moss_view_images_load_args`` of include/moss_raster.h (``moss_view_images_load``: one view's packed bytes / 255 to float32)."""
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("gt_u8", C.c_void_p), ("bkgd_u8", C.c_void_p), ("gt_image", C.c_void_p),
                ("bkgd_mask", C.c_void_p)]


_LBS_INPUTS = [("P", C.c_int32), ("J", C.c_int32), ("V", C.c_int32), ("vert_ids", C.c_void_p), ("weights", C.c_void_p),
               ("lbs_offsets", C.c_void_p), ("A_big", C.c_void_p), ("A_obs", C.c_void_p), ("d", C.c_void_p), ("R", C.c_void_p),
               ("Th", C.c_void_p), ("x", C.c_void_p)]


class LbsForwardArgs(C.Structure):
    """``moss_lbs_forward_args`` of include/moss_raster.h (``moss_lbs_deform_forward``: per-Gaussian LBS transforms of a frame)."""
    _fields_ = _LBS_INPUTS + [("T", C.c_void_p), ("t", C.c_void_p), ("p", C.c_void_p), ("w", C.c_void_p)]


class LbsBackwardArgs(C.Structure):
    """``moss_lbs_backward_args`` of include/moss_raster.h (``moss_lbs_deform_backward``)."""
    _fields_ = _LBS_INPUTS + [("g_T", C.c_void_p), ("g_t", C.c_void_p), ("g_p", C.c_void_p), ("g_L", C.c_void_p),
                              ("g_A_obs", C.c_void_p), ("g_d", C.c_void_p), ("g_x", C.c_void_p), ("workspace", C.c_void_p),
                              ("workspace_bytes", C.c_size_t)]


class LbsBackwardFrameArgs(C.Structure):
    """``moss_lbs_backward_frame_args`` of include/moss_raster.h (``moss_lbs_deform_backward_frame``: the backward with ``g_R``, ``g_Th``)."""
    _fields_ = LbsBackwardArgs._fields_ + [("g_R", C.c_void_p), ("g_Th", C.c_void_p)]


SMPL_FRAME_MAX_JOINTS = 64                               # MOSS_SMPL_FRAME_MAX_JOINTS
SMPL_FRAME_SAVED_FLOATS_PER_JOINT = 33                   # MOSS_SMPL_FRAME_SAVED_FLOATS_PER_JOINT


class SmplFrameArgs(C.Structure):
    """``moss_smpl_frame_args`` of include/moss_raster.h (``moss_smpl_frame_forward``: the per-frame SMPL skeleton and offsets)."""
    _fields_ = [("P", C.c_int32), ("V", C.c_int32), ("J", C.c_int32), ("num_betas_big", C.c_int32), ("num_betas", C.c_int32),
                ("shapedirs_stride", C.c_int32), ("parents", C.c_int32 * 64), ("v_template", C.c_void_p), ("shapedirs", C.c_void_p),
                ("posedirs", C.c_void_p), ("J_regressor", C.c_void_p), ("poses_big", C.c_void_p), ("shapes_big", C.c_void_p),
                ("poses", C.c_void_p), ("shapes", C.c_void_p), ("correct_Rs", C.c_void_p), ("vert_ids", C.c_void_p),
                ("A_big", C.c_void_p), ("A_obs", C.c_void_p), ("d", C.c_void_p), ("rot_mats", C.c_void_p), ("saved", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class SmplFrameBackwardArgs(C.Structure):
    """``moss_smpl_frame_backward_args`` of include/moss_raster.h (``moss_smpl_frame_backward``)."""
    _fields_ = [("P", C.c_int32), ("V", C.c_int32), ("J", C.c_int32), ("parents", C.c_int32 * 64), ("posedirs", C.c_void_p),
                ("vert_ids", C.c_void_p), ("saved", C.c_void_p), ("g_A_obs", C.c_void_p), ("g_d", C.c_void_p),
                ("g_correct_Rs", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class SmplFrameBackwardPoseArgs(C.Structure):
    """``moss_smpl_frame_backward_pose_args`` of include/moss_raster.h (``moss_smpl_frame_backward_pose``: the backward with ``g_poses``)."""
    _fields_ = SmplFrameBackwardArgs._fields_ + [("poses", C.c_void_p), ("correct_Rs", C.c_void_p), ("g_poses", C.c_void_p)]


class SmplVerticesArgs(C.Structure):
    """``moss_smpl_vertices_args`` of include/moss_raster.h (``moss_smpl_vertices``: a frame's posed SMPL vertices in the world and
    their padded box)."""
    _fields_ = [("V", C.c_int32), ("J", C.c_int32), ("num_betas", C.c_int32), ("shapedirs_stride", C.c_int32),
                ("parents", C.c_int32 * 64), ("v_template", C.c_void_p), ("shapedirs", C.c_void_p), ("posedirs", C.c_void_p),
                ("J_regressor", C.c_void_p), ("weights", C.c_void_p), ("poses", C.c_void_p), ("shapes", C.c_void_p), ("R", C.c_void_p),
                ("Th", C.c_void_p), ("pad", C.c_void_p), ("world_vertex", C.c_void_p), ("world_bound", C.c_void_p),
                ("joints", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class BoundMaskArgs(C.Structure):
    """``moss_bound_mask_args`` of include/moss_raster.h (``moss_bound_mask``: the bound masks and rectangles of one box for C cameras)."""
    _fields_ = [("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("world_bound", C.c_void_p), ("K", C.c_void_p), ("RT", C.c_void_p),
                ("bound", C.c_void_p), ("rect", C.c_void_p), ("corners", C.c_void_p), ("flags", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


class SmplVerticesBackwardArgs(C.Structure):
    """``moss_smpl_vertices_backward_args`` of include/moss_raster.h (``moss_smpl_vertices_backward``: the gradients of a frame's posed
    vertices to ``poses``, ``R`` and ``Th``)."""
    _fields_ = [("V", C.c_int32), ("J", C.c_int32), ("num_betas", C.c_int32), ("shapedirs_stride", C.c_int32),
                ("parents", C.c_int32 * 64), ("v_template", C.c_void_p), ("shapedirs", C.c_void_p), ("posedirs", C.c_void_p),
                ("J_regressor", C.c_void_p), ("weights", C.c_void_p), ("poses", C.c_void_p), ("shapes", C.c_void_p), ("R", C.c_void_p),
                ("Th", C.c_void_p), ("g_world_vertex", C.c_void_p), ("g_poses", C.c_void_p), ("g_R", C.c_void_p), ("g_Th", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


KEYPOINTS_MAX = 128                                      # MOSS_KEYPOINTS_MAX


class KeypointLossArgs(C.Structure):
    """``moss_keypoint_loss_args`` of include/moss_raster.h (``moss_keypoint_loss``: a keypoint loss on posed vertices, value and vertex
    gradient in one call)."""
    _fields_ = [("V", C.c_int32), ("Kp", C.c_int32), ("C", C.c_int32), ("world_vertex", C.c_void_p), ("regressor", C.c_void_p),
                ("K", C.c_void_p), ("RT", C.c_void_p), ("uv", C.c_void_p), ("conf", C.c_void_p), ("xyz", C.c_void_p),
                ("conf3", C.c_void_p), ("sigma", C.c_float), ("sigma3", C.c_float), ("weight2d", C.c_float), ("weight3d", C.c_float),
                ("loss", C.c_void_p), ("g_world_vertex", C.c_void_p), ("keypoints", C.c_void_p), ("flags", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


POSE_HEAD_SAVED_FLOATS = 896                            # MOSS_POSE_HEAD_SAVED_FLOATS
_POSE_INPUTS = [("poses", C.c_void_p), ("target_R", C.c_void_p), ("params", C.c_void_p * 52), ("parents", C.c_int32 * 24),
                ("fc_in", C.c_int32 * 23), ("overreg", C.c_float)]


class PoseHeadArgs(C.Structure):
    """``moss_pose_head_args`` of include/moss_raster.h (``moss_pose_head_forward``: MOSS's pose-refinement head + matrix-Fisher NLL)."""
    _fields_ = _POSE_INPUTS + [("Rs", C.c_void_p), ("S", C.c_void_p), ("nll", C.c_void_p), ("saved", C.c_void_p)]


class PoseHeadBackwardArgs(C.Structure):
    """``moss_pose_head_backward_args`` of include/moss_raster.h (``moss_pose_head_backward``)."""
    _fields_ = _POSE_INPUTS + [("S", C.c_void_p), ("saved", C.c_void_p), ("g_Rs", C.c_void_p), ("g_nll", C.c_void_p),
                               ("grads", C.c_void_p * 52)]


class LbsWeightNetArgs(C.Structure):
    """``moss_lbs_weight_net_args`` of include/moss_raster.h (``moss_lbs_weight_net_forward``: MOSS's CrossAttention_lbs)."""
    _fields_ = [("P", C.c_int32), ("x", C.c_void_p), ("Rs", C.c_void_p), ("params", C.c_void_p * 16), ("out", C.c_void_p),
                ("saved", C.c_void_p)]


class LbsWeightNetBackwardArgs(C.Structure):
    """``moss_lbs_weight_net_backward_args`` of include/moss_raster.h (``moss_lbs_weight_net_backward``)."""
    _fields_ = [("P", C.c_int32), ("Rs", C.c_void_p), ("params", C.c_void_p * 16), ("saved", C.c_void_p), ("g_out", C.c_void_p),
                ("g_x", C.c_void_p), ("g_Rs", C.c_void_p), ("grads", C.c_void_p * 16), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


class LpipsVggArgs(C.Structure):
    """``moss_lpips_vgg_args`` of include/moss_raster.h (``moss_lpips_vgg_forward``: MOSS's LPIPS term, VGG16)."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("frame_H", C.c_int32), ("frame_W", C.c_int32),
                ("rect", C.c_void_p), ("weights", C.c_void_p * 13), ("biases", C.c_void_p * 13), ("lin", C.c_void_p * 5),
                ("shift", C.c_void_p), ("scale", C.c_void_p), ("out", C.c_void_p), ("terms", C.c_void_p), ("saved", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("cap_H", C.c_int32), ("cap_W", C.c_int32)]


class LpipsVggBackwardArgs(C.Structure):
    """``moss_lpips_vgg_backward_args`` of include/moss_raster.h (``moss_lpips_vgg_backward``)."""
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("frame_H", C.c_int32), ("frame_W", C.c_int32), ("rect", C.c_void_p),
                ("weights_bwd", C.c_void_p * 13), ("scale", C.c_void_p), ("saved", C.c_void_p), ("g_out", C.c_void_p),
                ("dL_dx", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("cap_H", C.c_int32),
                ("cap_W", C.c_int32)]


class LpipsVggReferenceArgs(C.Structure):
    """``moss_lpips_vgg_reference_args`` of include/moss_raster.h (``moss_lpips_vgg_reference``: the ground truth's tapped activations,
    once)."""
    _fields_ = [("y", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("frame_H", C.c_int32), ("frame_W", C.c_int32),
                ("rect", C.c_void_p), ("weights", C.c_void_p * 13), ("biases", C.c_void_p * 13), ("shift", C.c_void_p),
                ("scale", C.c_void_p), ("reference", C.c_void_p), ("reference_bytes", C.c_size_t), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("cap_H", C.c_int32), ("cap_W", C.c_int32)]


class LpipsVggForwardRefArgs(C.Structure):
    """``moss_lpips_vgg_forward_ref_args`` of include/moss_raster.h (``moss_lpips_vgg_forward_ref``: the forward on x alone against a
    reference)."""
    _fields_ = [("x", C.c_void_p), ("reference", C.c_void_p), ("reference_bytes", C.c_size_t), ("H", C.c_int32), ("W", C.c_int32),
                ("frame_H", C.c_int32), ("frame_W", C.c_int32), ("rect", C.c_void_p), ("weights", C.c_void_p * 13),
                ("biases", C.c_void_p * 13), ("lin", C.c_void_p * 5), ("shift", C.c_void_p), ("scale", C.c_void_p), ("out", C.c_void_p),
                ("terms", C.c_void_p), ("saved", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("cap_H", C.c_int32), ("cap_W", C.c_int32)]


class LpipsConv3x3Args(C.Structure):
    """``moss_lpips_conv3x3_args`` of include/moss_raster.h (``moss_lpips_vgg_conv3x3``: one wide convolution of the LPIPS term, the
    kernel shape named by the caller)."""
    _fields_ = [("in_", C.c_void_p), ("weights", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("mask_in", C.c_void_p),
                ("mask_out", C.c_void_p), ("nimg", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("cin", C.c_int32),
                ("cout", C.c_int32), ("mode", C.c_int32), ("shape", C.c_int32), ("bf16", C.c_int32), ("rect", C.c_void_p),
                ("cap_H", C.c_int32), ("cap_W", C.c_int32), ("level", C.c_int32)]


LPIPS_CONV_MODES = {"fwd": 0, "bwd_mask": 1, "bwd_plain": 2}                        # moss_lpips_conv3x3_args.mode
LPIPS_CONV_SHAPES = {"auto": 0, "rows128": 1, "rows32": 2}                          # moss_lpips_conv3x3_args.shape


DENSIFY_MODES = {"clone": 0, "split": 1, "merge": 2, "prune": 3}                    # MOSS_DENSIFY_*


class DensifySelectArgs(C.Structure):
    """``moss_densify_select_args`` of include/moss_raster.h (``moss_densify_select``: one phase's mask, index list and count)."""
    _fields_ = [("mode", C.c_int32), ("P", C.c_int32), ("n_grads", C.c_int32), ("xyz_gradient_accum", C.c_void_p), ("denom", C.c_void_p),
                ("xyz", C.c_void_p), ("rotation", C.c_void_p), ("scaling", C.c_void_p), ("opacity", C.c_void_p), ("ids", C.c_void_p),
                ("surface_mask", C.c_void_p), ("max_radii2D", C.c_void_p), ("vertex_dist", C.c_void_p), ("max_grad", C.c_float),
                ("scale_limit", C.c_float), ("kl_threshold", C.c_float), ("min_opacity", C.c_float), ("max_screen_size", C.c_float),
                ("world_scale_limit", C.c_float), ("vertex_dist_limit", C.c_float), ("use_screen_size", C.c_int32), ("mask", C.c_void_p),
                ("index", C.c_void_p), ("count", C.c_void_p), ("count_host", C.c_void_p), ("kl_out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class DensifyEmitArgs(C.Structure):
    """``moss_densify_emit_args`` of include/moss_raster.h (``moss_densify_emit``: one phase's new rows)."""
    _fields_ = [("mode", C.c_int32), ("P", C.c_int32), ("n_sel", C.c_int32), ("n_new", C.c_int32), ("rest_floats", C.c_int32),
                ("dc_stride", C.c_int32), ("rest_stride", C.c_int32), ("index", C.c_void_p), ("ids", C.c_void_p), ("xyz", C.c_void_p), ("features_dc", C.c_void_p),
                ("features_rest", C.c_void_p), ("opacity", C.c_void_p), ("scaling", C.c_void_p), ("rotation", C.c_void_p),
                ("lbs_weights", C.c_void_p), ("denom", C.c_void_p), ("table", C.c_void_p), ("noise", C.c_void_p), ("new_xyz", C.c_void_p),
                ("new_features_dc", C.c_void_p), ("new_features_rest", C.c_void_p), ("new_opacity", C.c_void_p), ("new_scaling", C.c_void_p),
                ("new_rotation", C.c_void_p), ("prune_mask", C.c_void_p)]


ROWS_MAX_TENSORS = 12                                                               # MOSS_ROWS_MAX_TENSORS


class RowsTensor(C.Structure):
    """``moss_rows_tensor`` of include/moss_raster.h: one tensor of a ``moss_rows_relayout`` call."""
    _fields_ = [("src", C.c_void_p), ("src_m", C.c_void_p), ("src_v", C.c_void_p), ("app", C.c_void_p), ("dst", C.c_void_p),
                ("dst_m", C.c_void_p), ("dst_v", C.c_void_p), ("width", C.c_int32), ("pad_after", C.c_int32), ("use_map", C.c_int32),
                ("reserved", C.c_int32)]


class RowsRelayoutArgs(C.Structure):
    """``moss_rows_relayout_args`` of include/moss_raster.h (``moss_rows_relayout``: an event's row changes in one gather pass)."""
    _fields_ = [("rows_old", C.c_int32), ("rows_app", C.c_int32), ("rows_new", C.c_int32), ("num_tensors", C.c_int32), ("map", C.c_void_p),
                ("tensors", RowsTensor * ROWS_MAX_TENSORS)]


OPT_BITS = {"means3D": 1, "sh": 2, "opacity": 4, "scales": 8, "rotations": 16}      # MOSS_OPT_*; position = index in the struct's arrays


def lib() -> C.CDLL:
    """Load (once) and return the HIP library.  Raises ImportError if it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise ImportError(
                        f"{LIB_PATH} is missing: the MI355X HIP library has not been built "
                        "(run `python -m moss_amd.build`); there is no CPU/PyTorch fallback for this op")
                handle = C.CDLL(LIB_PATH)
                handle.moss_abi_version.restype = _i
                if handle.moss_abi_version() != ABI_VERSION:
                    raise ImportError(f"{LIB_PATH} implements ABI version {handle.moss_abi_version()}, this binding needs {ABI_VERSION}: "
                                      "rebuild it (python -m moss_amd.build --force)")
                _declare(handle)
                _lib = handle
    return _lib


_ext = None


def ext():
    """Load (once) and return the compiled PyTorch-ROCm extension module ``_moss_C`` (rasterize_gaussians,
    rasterize_gaussians_backward, mark_visible: the reference's ``_C``).  Raises ImportError if it has not been built."""
    global _ext
    if _ext is None:
        with _lock:
            if _ext is None:
                if not os.path.exists(EXT_PATH):
                    raise ImportError(
                        f"{EXT_PATH} is missing: the PyTorch extension of the MI355X rasterizer has not been built "
                        "(run `python -m moss_amd.build`); there is no CPU/PyTorch fallback for this op")
                lib()                                        # libmoss_raster.so first: _moss_C.so links against it
                import importlib.machinery
                import importlib.util
                loader = importlib.machinery.ExtensionFileLoader("_moss_C", EXT_PATH)
                spec = importlib.util.spec_from_loader("_moss_C", loader)
                mod = importlib.util.module_from_spec(spec)
                loader.exec_module(mod)
                # abi_version() is the extension's COMPILE-TIME MOSS_ABI_VERSION: a stale _moss_C.so next to a rebuilt library is caught
                if mod.abi_version() != lib().moss_abi_version():
                    raise ImportError(f"{EXT_PATH} was compiled against ABI version {mod.abi_version()}, libmoss_raster.so implements "
                                      f"{lib().moss_abi_version()}: rebuild both (python -m moss_amd.build --force)")
                _ext = mod
    return _ext


STAGES = ["preprocess_fwd", "scan", "scatter", "chunk_sort", "blend_fwd", "blend_bwd", "preprocess_bwd", "merge_gather"]    # (every stage is ONE kernel)


def profile_enable(stages=None):
    """Enable HIP-event timing for the named stages (None = all, [] = off)."""
    names = STAGES if stages is None else stages
    mask = 0
    for n in names:
        mask |= 1 << STAGES.index(n)
    lib().moss_raster_profile_enable(mask)


def profile_read():
    """{stage: (total_ms, count)} since the last read (synchronises the recorded events)."""
    ms = (C.c_float * 8)()
    cnt = (C.c_uint32 * 8)()
    check(lib().moss_raster_profile_read(ms, cnt), "profile_read")
    return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(STAGES)}


def check(rc: int, what: str) -> int:
    if rc < 0:
        msg = lib().moss_last_error().decode(errors="replace")
        raise RuntimeError(f"{what}: {ERR_NAMES.get(rc, rc)}: {msg}")
    return rc


def ptr(t):
    """The device address of tensor ``t``; None (NULL across the boundary) for None."""
    return None if t is None else t.data_ptr()


def stream(dev):
    """The handle of the current stream of ``dev``: the last argument of every entry point that enqueues work."""
    return torch.cuda.current_stream(dev).cuda_stream


def call(name: str, dev, *args) -> int:
    """``lib().<name>(*args, <the current stream of dev>)`` with ``dev`` as the current device, checked: THE way an op enqueues one
    entry point.  (A site that makes several calls under one device guard writes the guard itself and uses :func:`stream` and
    :func:`check`.)"""
    with torch.cuda.device(dev):
        return check(getattr(lib(), name)(*args, stream(dev)), name)
