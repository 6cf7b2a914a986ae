"""ctypes binding of libisr_hip.so (the C ABI declared in include/isr_hip.h).

There is no CPU fallback: if the library is missing or a call fails this module raises.
torch is imported first so that the library binds to the same libamdhip64 instance as torch —
streams and device pointers are then shared.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import torch  # noqa: F401  (must be loaded before libisr_hip.so: shared HIP runtime)

import os

_PKG = Path(__file__).resolve().parent
# ISR_HIP_LIB: tooling only (A/B timing of two builds of the library in one GPU session)
LIB_PATH = Path(os.environ["ISR_HIP_LIB"]) if os.environ.get("ISR_HIP_LIB") else _PKG / "libisr_hip.so"

ISR_OK = 0
ABI_VERSION = 6
DTYPE_BF16 = 0
DTYPE_F32 = 1
DTYPE_BF16_LOG2 = 2
DTYPE_BF16_LOG2_SCREENED = 3
RANSAC_STAGED = 0          # ISR_RANSAC_* / ISR_INLIERS_* of include/isr_hip.h
RANSAC_SEQUENTIAL = 1
INLIERS_REFIT = 0
INLIERS_RANSAC = 1
FINAL_REFIT = 0            # ISR_FINAL_*
FINAL_EPNP = 1
# ISR_TUNE_* knobs of include/isr_hip.h
TUNE = {"nn_path": 0, "nn_filter": 1, "icp_warm": 2, "nn_plan_rq": 3, "nn_plan_blocks": 4,
        "nn_tile_st": 5, "nn_tile_sq": 6, "nn_tile_tb": 7, "ep_wsum_valu": 8, "k1_f32_chain": 9, "k1_split": 10}


class IsrError(RuntimeError):
    pass


_lib = None

_vp = C.c_void_p
_i = C.c_int
_sz = C.c_size_t
_d = C.c_double
_f = C.c_float
_u64 = C.c_uint64
_i64 = C.c_int64

# name -> (restype, argtypes); kept in one table so tests can check it against the header.
SIGNATURES = {
    "isr_abi_version": (_i, []),
    "isr_last_error": (C.c_char_p, []),
    "isr_device_count": (_i, []),
    "isr_tuning_set": (_i, [_i, _i]),
    "isr_tuning_get": (_i, [_i]),
    "isr_corr_argmax_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "isr_corr_argmax": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_corr_argmax_digits": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "isr_corr_argmax_phase": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _sz, _vp]),
    "isr_corr_argmax_recheck_count": (_i, [_vp, _sz, _i, _i, _i, _vp, _vp]),
    "isr_corr_argmax_recheck_count_f32": (_i, [_vp, _sz, _i, _i, _i, _vp, _vp]),
    "isr_corr_argmax_screen_redone": (_i, [_vp, _sz, _i, _i, _i, _vp, _vp]),
    "isr_corr_quantize_fp6": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "isr_corr_argmax_clock_mhz": (_i, [_vp, _sz, _i, _i, _i, _vp, _vp]),
    "isr_adds_bounds": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _d, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "isr_corr_topk_workspace_bytes": (_sz, [_i, _i]),
    "isr_corr_topk": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_corr_logsoftmax_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "isr_corr_logsoftmax": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp, _sz, _vp]),
    "isr_ep_corr_matrices": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "isr_mask_bbox": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "isr_crop_normalize": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "isr_select_top_batch_workspace_bytes": (_sz, [_i, _i]),
    "isr_select_top_batch": (_i, [_vp, _i, _i, _vp, _d, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_select_top_batch_digits": (_i, [_vp, _i, _i, _vp, _d, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_gather_corr_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "isr_pnp_ransac_batch_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "isr_pnp_ransac_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _f, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp,
                                  _i, _i, _i, _i]),
    "isr_ransac_seq_host": (_i, [_vp, _vp, _i, _i, _d, _vp, _vp]),
    "isr_epnp_batch_workspace_bytes": (_sz, [_i, _i]),
    "isr_epnp_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_epnp_host": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "isr_epnp_jacobi_host": (_i, [_vp, _i, _vp, _vp]),
    "isr_prep_queries_batch_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "isr_prep_queries_batch": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_p3p_all_roots": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "isr_p3p_hypotheses": (_i, [_vp, _vp, _vp, _i, _vp, _i, _u64, _vp, _vp, _vp, _vp]),
    "isr_ransac_score": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_pnp_refine": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "isr_nn_batched_workspace_bytes": (_sz, [_i, _i, _i]),
    "isr_nn_batched": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _sz, _vp]),
    "isr_ep_prepare": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_ep_pool_corr": (_i, [_vp, _i, _i, _vp, _vp]),
    "isr_ep_patch_corr_workspace_bytes": (_sz, [_i, _i, _i]),
    "isr_ep_patch_corr": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "isr_ep_patch_corr_cells": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "isr_ep_sample_workspace_bytes": (_sz, [_i, _i]),
    "isr_ep_sample": (_i, [_vp, _vp, _i, _i, _d, _i, _u64, _vp, _vp, _sz, _vp]),
    "isr_ep_sample_direct": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _d, _i, _u64, _vp, _vp, _sz, _vp]),
    "isr_ep_sample_weights": (_i, [_vp, _vp, _i, _i, _d, _vp, _vp, _sz, _vp]),
    "isr_ep_p3p": (_i, [_vp, _i, _i, _vp, _vp, _i, _u64, _vp, _vp, _vp]),
    "isr_ep_prune": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _d, _d, _d, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "isr_zbuf_score_workspace_bytes": (_sz, [_i, _i]),
    "isr_zbuf_score": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_estimate_pose_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "isr_estimate_pose": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _d, _vp, _i, _i, _i, _d, _d, _i, _i, _i, _u64,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_zbuf_score_direct": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_refine_objective": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_refine_objective_full": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_refine_objective_batch_workspace_bytes": (_sz, [_i]),
    "isr_refine_objective_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp,
                                        _sz, _vp]),
    "isr_refine_bfgs_batch_workspace_bytes": (_sz, [_i]),
    "isr_refine_bfgs_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _d, _i, _i, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_bfgs_state_bytes": (_sz, []),
    "isr_bfgs_host_init": (_i, [_vp, _sz, _i, _vp, _d, _i, _vp]),
    "isr_bfgs_host_step": (_i, [_vp, _d, _vp, _vp, _vp, _vp]),
    "isr_add_metric": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp]),
    "isr_icp_workspace_bytes": (_sz, [_i, _i]),
    "isr_icp_point_to_point": (_i, [_vp, _i, _vp, _i, _d, _i, _d, _d, _vp, _vp, _vp, _sz, _vp]),
    "isr_icp_point_to_point_batch_workspace_bytes": (_sz, [_i, _i, _i]),
    "isr_icp_point_to_point_batch": (_i, [_vp, _sz, _i, _vp, _i, _i, _d, _i, _d, _d, _vp, _vp, _sz, _vp]),
    "isr_rel_pose_table": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "isr_render_coords_batch_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "isr_render_coords_batch": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _f, _d, _d, _i, _vp, _vp, _sz, _vp]),
    "isr_render_coords_host": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _f, _d, _d, _i, _vp]),
}

# include/isr_field.h (the key field), bound beside SIGNATURES: isr_hip.h's entry list stays what it is
FIELD_SIGNATURES = {
    "isr_field_pack_bytes": (_sz, [_i, _vp]),
    "isr_field_pack": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "isr_field_eval": (_i, [_vp, _sz, _i, _vp, _vp, _i, _vp, _i, _vp]),
    "isr_field_eval_host": (_i, [_vp, _sz, _i, _vp, _vp, _i, _vp, _i]),
    "isr_field_sin_host": (_i, [_vp, _sz, _vp]),
}

# include/isr_fps.h (farthest-point sampling), bound the same way
FPS_SIGNATURES = {
    "isr_fps_workspace_bytes": (_sz, [_i, _i]),
    "isr_fps_sample": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "isr_fps_sample_host": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "isr_fps_launch_floor": (_i, [_i, _vp]),
}

# include/isr_density.h (the density field and its ray march), bound the same way
DENSITY_SIGNATURES = {
    "isr_density_pack_bytes": (_sz, [_i, _vp, _i]),
    "isr_density_pack": (_i, [_i, _vp, _i, _vp, _f, _vp, _vp, _vp, _sz]),
    "isr_density_eval": (_i, [_vp, _sz, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "isr_density_march": (_i, [_vp, _sz, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "isr_density_eval_host": (_i, [_vp, _sz, _i, _vp, _i, _vp, _i, _vp]),
    "isr_density_march_host": (_i, [_vp, _sz, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "isr_density_sincos_host": (_i, [_vp, _sz, _vp, _vp]),
    "isr_density_activations_host": (_i, [_vp, _sz, _f, _vp, _vp]),
}

# include/isr_density_dir.h (the march with a direction), bound the same way
DENSITY_DIR_SIGNATURES = {
    "isr_density_march_dir": (_i, [_vp, _sz, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "isr_density_march_dir_host": (_i, [_vp, _sz, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "isr_density_march_given_host": (_i, [_vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp]),
}

# include/isr_radius.h (the fixed-radius neighbour count), bound the same way
RADIUS_SIGNATURES = {
    "isr_radius_workspace_bytes": (_sz, [_i]),
    "isr_radius_count": (_i, [_vp, _i, _d, _i, _vp, _vp, _sz, _vp]),
    "isr_radius_count_host": (_i, [_vp, _i, _d, _i, _vp]),
}

# include/isr_knn.h (k nearest neighbours and local frames), bound the same way
KNN_SIGNATURES = {
    "isr_knn_workspace_bytes": (_sz, [_i, _i, _i]),
    "isr_knn": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "isr_knn_host": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp]),
    "isr_local_frames": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "isr_local_frames_host": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp]),
}

# include/isr_rays.h (ray bundles from cameras), bound the same way
_RAYS_SPEC = [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _i, _u64]      # mode .. seed: the arguments every isr_rays_* entry starts with
RAYS_SIGNATURES = {
    "isr_rays_workspace_bytes": (_sz, [_i, _i]),
    "isr_rays_bundle": (_i, [*_RAYS_SPEC, _vp, _vp, _vp, _vp, _vp]),
    "isr_rays_bundle_host": (_i, [*_RAYS_SPEC, _vp, _vp, _vp, _vp]),
    "isr_rays_select_count": (_i, [*_RAYS_SPEC, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "isr_rays_select_emit": (_i, [*_RAYS_SPEC, _vp, _i, _i, _vp, _sz, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "isr_rays_select_count_host": (_i, [*_RAYS_SPEC, _vp, _i, _i, _vp]),
    "isr_rays_select_emit_host": (_i, [*_RAYS_SPEC, _vp, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp]),
    "isr_sample_nearest": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "isr_sample_nearest_host": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "isr_rays_philox_host": (_i, [_vp, _vp, _vp, _vp]),
}

# include/isr_radiance.h (the radiance field's render and the emission-absorption march), bound the same way
_RADIANCE_FIELD = [_vp, _sz, _i, _vp, _i, _i, _i]      # pack .. C: the arguments both render entries start with
RADIANCE_SIGNATURES = {
    "isr_radiance_pack_bytes": (_sz, [_i, _vp, _i, _i, _i]),
    "isr_radiance_pack": (_i, [_i, _vp, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _sz]),
    "isr_radiance_workspace_bytes": (_sz, [_i, _i]),
    "isr_radiance_render": (_i, [*_RADIANCE_FIELD, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_ea_march": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "isr_radiance_render_host": (_i, [*_RADIANCE_FIELD, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "isr_ea_march_host": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "isr_radiance_sigmoid_host": (_i, [_vp, _sz, _vp]),
    "isr_radiance_normalize_host": (_i, [_vp, _sz, _vp]),
}

# include/isr_resample.h (the fine pass's ray sampling), bound the same way
RESAMPLE_SIGNATURES = {
    "isr_sample_pdf": (_i, [_vp, _vp, _i64, _i, _i, _i, _f, _u64, _vp, _vp, _vp]),
    "isr_sample_pdf_host": (_i, [_vp, _vp, _i64, _i, _i, _i, _f, _u64, _vp, _vp]),
    "isr_resample_lengths": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _f, _u64, _vp, _vp, _vp]),
    "isr_resample_lengths_host": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _f, _u64, _vp, _vp]),
    "isr_resample_rays_per_group": (_i, [_i, _i, _i, _i]),
}

# include/isr_contrastive.h (the contrastive key loss and its gradient), bound the same way
_CONTRASTIVE_SHAPE = [_vp, _vp, _vp, _i64, _i64, _i64, _i, _i64, _d]      # q, k, n, B, S, M, D, Bn, scale
CONTRASTIVE_SIGNATURES = {
    "isr_contrastive_workspace_bytes": (_sz, [_i64, _i64, _i64, _i, _i64]),
    "isr_contrastive_forward": (_i, [*_CONTRASTIVE_SHAPE, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_contrastive_backward": (_i, [*_CONTRASTIVE_SHAPE, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "isr_contrastive_forward_host": (_i, [*_CONTRASTIVE_SHAPE, _vp, _vp, _vp, _vp, _vp]),
    "isr_contrastive_backward_host": (_i, [*_CONTRASTIVE_SHAPE, _vp, _vp, _vp, _vp, _vp, _vp]),
    "isr_contrastive_geometry": (_i, [_i]),
    "isr_contrastive_column_splits": (_i64, [_i64, _i64, _i64, _i, _i64]),
}

# include/isr_field_grad.h (the key field's backward and the device-side packing), bound the same way
FIELD_GRAD_SIGNATURES = {
    "isr_field_grad_pack_bytes": (_sz, [_i, _vp]),
    "isr_field_pack_device": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "isr_field_grad_workspace_bytes": (_sz, [_i, _vp, _i]),
    "isr_field_backward": (_i, [_vp, _sz, _vp, _sz, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "isr_field_backward_host": (_i, [_vp, _sz, _i, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "isr_field_cos_host": (_i, [_vp, _sz, _vp]),
    "isr_field_grad_geometry": (_i, [_i]),
}

# include/isr_sample_grad.h (the backward of isr_sample_nearest), bound the same way
SAMPLE_GRAD_SIGNATURES = {
    "isr_sample_grad_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "isr_sample_nearest_backward": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "isr_sample_nearest_backward_host": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "isr_sample_grad_geometry": (_i, [_i]),
}

# include/isr_ea_grad.h (the backward of isr_ea_march), bound the same way
EA_GRAD_SIGNATURES = {
    "isr_ea_march_backward": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "isr_ea_march_backward_host": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "isr_ea_grad_geometry": (_i, [_i]),
    "isr_ea_grad_rays_per_group": (_i, [_i]),
}

# include/isr_radiance_grad.h (the radiance field's backward and the device-side packing), bound the same way
_RADIANCE_SHAPE = [_i, _vp, _i, _i, _i]      # n_hidden, widths, H, Wc, C
_RADIANCE_RAYS = [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]      # origins, directions, lengths, N, P, d_densities, d_colours, dW, db
RADIANCE_GRAD_SIGNATURES = {
    "isr_radiance_grad_pack_bytes": (_sz, [*_RADIANCE_SHAPE]),
    "isr_radiance_pack_device": (_i, [*_RADIANCE_SHAPE, _vp, _f, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "isr_radiance_grad_workspace_bytes": (_sz, [*_RADIANCE_SHAPE, _i, _i]),
    "isr_radiance_backward": (_i, [_vp, _sz, _vp, _sz, *_RADIANCE_SHAPE, *_RADIANCE_RAYS, _vp, _sz, _vp]),
    "isr_radiance_backward_host": (_i, [_vp, _sz, *_RADIANCE_SHAPE, *_RADIANCE_RAYS]),
    "isr_radiance_grad_slopes_host": (_i, [_vp, _sz, _f, _vp, _vp]),
    "isr_radiance_grad_geometry": (_i, [_i]),
}

# include/isr_mc.h (iso-surface extraction), bound the same way
MC_SIGNATURES = {
    "isr_mc_workspace_bytes": (_sz, [_i, _i, _i]),
    "isr_mc_count": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "isr_mc_emit": (_i, [_vp, _i, _i, _i, _f, _vp, _sz, _vp, _i64, _vp, _i64, _vp]),
    "isr_mc_count_host": (_i, [_vp, _i, _i, _i, _f, _vp]),
    "isr_mc_emit_host": (_i, [_vp, _i, _i, _i, _f, _vp, _i64, _vp, _i64]),
}

# include/isr_augment.h (training batches: the image warps and the ray remap and sample), bound the same way
_AUGMENT_IMAGES = [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]      # rgb .. mask_out
_AUGMENT_RAYS = [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
AUGMENT_SIGNATURES = {
    "isr_augment_images": (_i, [*_AUGMENT_IMAGES, _vp]),
    "isr_augment_images_host": (_i, _AUGMENT_IMAGES),
    "isr_augment_rays": (_i, [*_AUGMENT_RAYS, _vp]),
    "isr_augment_rays_host": (_i, _AUGMENT_RAYS),
}

# include/isr_adam.h (the fused multi-tensor Adam), bound the same way
ADAM_SIGNATURES = {
    "isr_adam_geometry": (_i, [_i]),
    "isr_adam_table_host": (_i, [_vp, _i, _i, _i64, _vp, _vp]),
    "isr_adam_step": (_i, [_vp, _vp, _i, _i64, _vp, _i, _vp, _i, _vp]),
    "isr_adam_zero_grads": (_i, [_vp, _vp, _i, _i64, _vp]),
    "isr_adam_step_host": (_i, [_vp, _i, _vp, _i, _vp, _i64, _i]),
    "isr_adam_scalars_host": (_i, [_vp, _i64, _vp, _vp]),
}

# include/isr_ray_losses.h (the distortion loss and the render loss, with their gradients), bound the same way
_RENDER_LOSS = [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _d]      # rendered, target_images, target_silhouettes, xys, B, n, F, H, W, scaling
RAY_LOSSES_SIGNATURES = {
    "isr_distortion_workspace_bytes": (_sz, [_i64, _i]),
    "isr_distortion_forward": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp, _sz, _vp]),
    "isr_distortion_backward": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "isr_distortion_forward_host": (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    "isr_distortion_backward_host": (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    "isr_render_loss_workspace_bytes": (_sz, [_i64, _i64]),
    "isr_render_loss_forward": (_i, [*_RENDER_LOSS, _vp, _vp, _sz, _vp]),
    "isr_render_loss_backward": (_i, [*_RENDER_LOSS, _vp, _vp, _vp]),
    "isr_render_loss_forward_host": (_i, [*_RENDER_LOSS, _vp]),
    "isr_render_loss_backward_host": (_i, [*_RENDER_LOSS, _vp, _vp]),
    "isr_ray_losses_geometry": (_i, [_i]),
}

# include/isr_color_aug.h (the colour augmentation pass), bound the same way
_COLOR_AUG = [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]      # in, B, H, W, programs .. std3, out
COLOR_AUG_SIGNATURES = {
    "isr_color_aug_workspace_bytes": (_sz, [_i, _i, _i]),
    "isr_augment_color": (_i, [*_COLOR_AUG, _vp, _sz, _vp]),
    "isr_augment_color_host": (_i, _COLOR_AUG),
    "isr_color_aug_draws_host": (_i, [_u64, _i, _d, _vp, _vp]),
    "isr_color_aug_geometry": (_i, [_i]),
}

# include/isr_ingest.h (sequence ingest: BOP frames to training views and cameras), bound the same way
_INGEST = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]      # rgb, mask, K_in, n .. sil_mode, images .. status
INGEST_SIGNATURES = {
    "isr_ingest_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "isr_ingest_views": (_i, [*_INGEST, _vp, _sz, _vp]),
    "isr_ingest_views_host": (_i, _INGEST),
    "isr_ingest_geometry": (_i, [_i]),
    "isr_ingest_strip_rows": (_i, [_i, _i, _i]),
    "isr_ingest_strips": (_i, [_i, _i, _i]),
    "isr_ingest_launch_floor": (_i, [_i, _i, _i, _i, _i, _vp]),
}

# include/isr_icp_plane.h (point-to-plane ICP with robust weights), bound the same way
ICP_L2, ICP_HUBER, ICP_TUKEY = 0, 1, 2       # ISR_ICP_*
ICP_PLANE_STATE_DOUBLES = 24
_ICP_PLANE = [_vp, _sz, _i, _vp, _vp, _i, _i, _d, _i, _d, _d, _i, _d, _vp]      # src .. state
ICP_PLANE_SIGNATURES = {
    "isr_icp_point_to_plane_batch_workspace_bytes": (_sz, [_i, _i, _i]),
    "isr_icp_point_to_plane_batch": (_i, [*_ICP_PLANE, _vp, _sz, _vp]),
    "isr_icp_point_to_plane_batch_host": (_i, _ICP_PLANE),
}

# include/isr_seq_refit.h (the sequence-level pose: one robust refit over every frame's matches), bound the same way
SEQ_REFIT_STATE_DOUBLES = 24
SEQ_REFIT_FRAME_STATS = 4
_SEQ_REFIT = [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _d, _i, _d, _d, _vp, _vp]      # p3d .. frame_stats
SEQ_REFIT_SIGNATURES = {
    "isr_seq_refit_workspace_bytes": (_sz, [_i, _i]),
    "isr_seq_refit": (_i, [*_SEQ_REFIT, _vp, _sz, _vp]),
    "isr_seq_refit_host": (_i, _SEQ_REFIT),
    "isr_seq_refit_sums_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _d, _vp, _vp, _vp]),
}


def lib() -> C.CDLL:
    """Load libisr_hip.so (once).  Raises IsrError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise IsrError(
            f"{LIB_PATH} is missing: build it with "
            "`python -m imagesequenceregistrationfor6dposeestimationlabeling_amd.build` "
            "(there is no CPU fallback)")
    try:
        L = C.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover
        raise IsrError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in {**SIGNATURES, **FIELD_SIGNATURES, **FPS_SIGNATURES, **DENSITY_SIGNATURES,
                               **DENSITY_DIR_SIGNATURES, **RADIUS_SIGNATURES, **MC_SIGNATURES, **KNN_SIGNATURES,
                               **RAYS_SIGNATURES, **RADIANCE_SIGNATURES, **RESAMPLE_SIGNATURES,
                               **CONTRASTIVE_SIGNATURES, **FIELD_GRAD_SIGNATURES, **SAMPLE_GRAD_SIGNATURES,
                               **EA_GRAD_SIGNATURES, **RADIANCE_GRAD_SIGNATURES, **AUGMENT_SIGNATURES,
                               **ADAM_SIGNATURES, **RAY_LOSSES_SIGNATURES, **COLOR_AUG_SIGNATURES, **INGEST_SIGNATURES,
                               **ICP_PLANE_SIGNATURES, **SEQ_REFIT_SIGNATURES}.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            raise IsrError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if L.isr_abi_version() != ABI_VERSION:
        raise IsrError(f"ABI version {L.isr_abi_version()} != {ABI_VERSION}")
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != ISR_OK:
        msg = lib().isr_last_error()
        raise IsrError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t) -> int | None:
    """Device (or host) address of a tensor, None for None."""
    if t is None:
        return None
    return t.data_ptr()


def current_stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(*tensors) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise IsrError(
                "libisr_hip operates on device tensors only (got a CPU tensor); "
                "there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise IsrError(f"tensors on different devices: {dev} vs {t.device}")
    if dev is None:
        raise IsrError("no device tensor given")
    return dev
