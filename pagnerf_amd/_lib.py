"""ctypes binding of libpagnerf_hip.so (include/pagnerf_hip.h).

The product path has NO CPU fallback: if the library is missing or a GPU tensor is not handed
in, calls raise.  Import of this module alone never touches the GPU.
"""
import ctypes
import os

import torch

from . import build as _build

F32, F16, BF16 = 0, 1, 2
I32, I64 = 3, 4
ACT_NONE, ACT_SIGMOID, ACT_SOFTMAX = 0, 1, 2
MLP_MFMA_BF16, MLP_FP32 = 0, 1
BG_BLACK, BG_WHITE = 0, 1
LAYOUT_STRIDED, LAYOUT_XCD8 = 0, 1
ENC_HALF_COORDS = 1
ABI_VERSION = 15
MLP_FUSED_WIDE_MAX_M = 1 << 24      # PAG_MLP_FUSED_WIDE_MAX_M

_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}

c_i64, c_i32, c_u32, c_f32, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p
c_fp = ctypes.POINTER(ctypes.c_float)
c_ip = ctypes.POINTER(ctypes.c_int)


class HeadCompositeArgs(ctypes.Structure):
    """pag_head_composite_args (include/pagnerf_hip.h)."""
    _fields_ = [("pack_start", c_vp), ("ray_of_pack", c_vp), ("P", c_i64), ("weights", c_vp), ("alpha", c_vp), ("out", c_vp), ("n_samples", c_i64)]


class MlpFwdArgs(ctypes.Structure):
    pass


MlpFwdArgs._fields_ = [("x1", c_vp), ("x1_dtype", c_i32), ("k1", c_i32),
                ("x1_layout", c_i32), ("x1_levels", c_i32), ("x1_feats", c_i32),
                ("x2", c_vp), ("k2p", c_i32), ("x2_index", c_vp),
                ("in_dim", c_i32), ("n_layers", c_i32), ("out_dim", c_i32),
                ("W", c_vp * 3), ("b", c_vp * 3),
                ("out_act", c_i32),
                ("out", c_vp), ("out_dtype", c_i32),
                ("hidden_save", c_vp * 2),
                ("mode", c_i32),
                ("softmax_stats", c_vp), ("x1_col0_relu", c_vp), ("pair", ctypes.POINTER(MlpFwdArgs)),
                ("composite", ctypes.POINTER(HeadCompositeArgs)), ("x1_producer", ctypes.POINTER(MlpFwdArgs))]


class WgradLayer(ctypes.Structure):
    """pag_wgrad_layer (include/pagnerf_hip.h)."""
    _fields_ = [("dz", c_vp), ("dz_cols", c_i32), ("n_out", c_i32),
                ("a1", c_vp), ("a1_dtype", c_i32), ("a1_layout", c_i32), ("k1", c_i32),
                ("a2", c_vp), ("k2p", c_i32), ("a2_index", c_vp), ("n_in", c_i32),
                ("slabs", c_vp), ("n_blocks", c_i32), ("a1_levels", c_i32), ("a1_feats", c_i32),
                ("dW", c_vp), ("db", c_vp)]


class MlpBwdArgs(ctypes.Structure):
    pass


MlpBwdArgs._fields_ = [("grad_out", c_vp), ("out", c_vp), ("out_dtype", c_i32), ("out_act", c_i32),
                ("k1", c_i32), ("in_dim", c_i32), ("n_layers", c_i32), ("out_dim", c_i32),
                ("x1_layout", c_i32), ("x1_levels", c_i32), ("x1_feats", c_i32),
                ("W", c_vp * 3),
                ("hidden_save", c_vp * 2),
                ("dz", c_vp * 3),
                ("dx1", c_vp), ("dx1_dtype", c_i32),
                ("mode", c_i32),
                ("g_ray", c_vp), ("g_scale", c_vp), ("g_index", c_vp),
                ("softmax_stats", c_vp), ("b_last", c_vp), ("dx1_accumulate", c_i32), ("dx1_col0_add", c_vp),
                ("dx1_col0_gate", c_vp), ("g_ray_scale", c_vp),
                ("x1", c_vp), ("x1_dtype", c_i32), ("x2", c_vp), ("k2p", c_i32), ("x2_index", c_vp),
                ("wgrad_workspace", c_vp), ("wgrad_workspace_bytes", c_i64),
                ("dW", c_vp * 3), ("db", c_vp * 3), ("b", c_vp * 3),
                ("pair", ctypes.POINTER(MlpBwdArgs)), ("dz0_slots", c_vp)]


class DeepMlpArgs(ctypes.Structure):
    """pag_deep_mlp_args (include/pagnerf_hip.h)."""
    _fields_ = [("coords", c_vp), ("ray_d", c_vp), ("hidden", c_i32), ("num_classes", c_i32), ("channels", c_i32), ("save", c_i32),
                ("W", c_vp * 14), ("b", c_vp * 14), ("density", c_vp), ("rgb", c_vp), ("semantics", c_vp),
                ("workspace", c_vp), ("workspace_bytes", c_i64),
                ("g_density", c_vp), ("g_rgb", c_vp), ("g_semantics", c_vp), ("dW", c_vp * 14), ("db", c_vp * 14),
                ("bwd_workspace", c_vp), ("bwd_workspace_bytes", c_i64)]


MLP128_MAX_M = 1 << 26              # PAG_MLP128_MAX_M
MLP128_BATCH, MLP128_MAX_GRID = 256, 256      # samples per workgroup batch, workgroups per launch (the forward / backward grid-stride beyond their product)


class Mlp128FwdArgs(ctypes.Structure):
    """pag_mlp128_fwd_args (include/pagnerf_hip.h)."""
    _fields_ = [("x1", c_vp), ("x1_dtype", c_i32), ("k1", c_i32), ("x1_layout", c_i32), ("x1_levels", c_i32), ("x1_feats", c_i32),
                ("x2", c_vp), ("k2p", c_i32), ("x2_index", c_vp),
                ("in_dim", c_i32), ("n_hidden", c_i32), ("hidden", c_i32), ("out_dim", c_i32),
                ("W", c_vp * 4), ("b", c_vp * 4), ("out_act", c_i32), ("out", c_vp), ("out_dtype", c_i32),
                ("workspace", c_vp), ("workspace_bytes", c_i64)]


class Mlp128BwdArgs(ctypes.Structure):
    """pag_mlp128_bwd_args (include/pagnerf_hip.h)."""
    _fields_ = [("grad_out", c_vp), ("out", c_vp), ("out_dtype", c_i32), ("out_act", c_i32),
                ("k1", c_i32), ("k2p", c_i32), ("in_dim", c_i32), ("n_hidden", c_i32), ("hidden", c_i32), ("out_dim", c_i32),
                ("x1_layout", c_i32), ("x1_levels", c_i32), ("x1_feats", c_i32),
                ("W", c_vp * 4), ("workspace", c_vp), ("workspace_bytes", c_i64), ("bwd_workspace", c_vp), ("bwd_workspace_bytes", c_i64),
                ("dx1", c_vp), ("dx1_dtype", c_i32), ("dx1_accumulate", c_i32), ("dW", c_vp * 4), ("db", c_vp * 4)]


class VmArgs(ctypes.Structure):
    """pag_vm_args (include/pagnerf_hip.h)."""
    _fields_ = [("density_plane", c_vp * 3), ("density_line", c_vp * 3), ("app_plane", c_vp * 3), ("app_line", c_vp * 3), ("basis", c_vp),
                ("density_n_comp", c_i32), ("app_n_comp", c_i32), ("app_dim", c_i32), ("res", c_i32),
                ("xyz", c_vp), ("sigma", c_vp), ("app", c_vp), ("g_sigma", c_vp), ("g_app", c_vp),
                ("g_density_plane", c_vp * 3), ("g_density_line", c_vp * 3), ("g_app_plane", c_vp * 3), ("g_app_line", c_vp * 3), ("g_basis", c_vp),
                ("workspace", c_vp), ("workspace_bytes", c_i64)]


class SampleMode(ctypes.Structure):
    """pag_sample_mode (include/pagnerf_hip.h)."""
    _fields_ = [("src", c_vp), ("dst", c_vp), ("row_bytes", c_i64), ("per_view", c_i32), ("convert", c_i32)]


SAMPLE_MAX_MODES = 12
SAMPLE_COPY, SAMPLE_U8_TO_F32 = 0, 1

class LabelPlane(ctypes.Structure):
    """pag_label_plane (include/pagnerf_hip.h)."""
    _fields_ = [("src", c_vp), ("dst", c_vp)]


PREPARE_MAX_PLANES = 8


class CocoTables(ctypes.Structure):
    """pag_coco_tables (include/pagnerf_hip.h)."""
    _fields_ = [("verts", c_vp), ("part_vert_begin", c_vp), ("point_begin", c_vp), ("part_key_begin", c_vp), ("part_key_count", c_vp), ("keys", c_vp),
                ("ann_part_begin", c_vp), ("ann_label", c_vp), ("ann_cover", c_vp), ("cand", c_vp), ("frame_ann_begin", c_vp), ("frame_labelled", c_vp),
                ("n_verts", c_i32), ("n_parts", c_i32), ("n_anns", c_i32), ("n_cand", c_i32), ("B", c_i32), ("max_part_keys", c_i32)]


class Bup20PrepareArgs(ctypes.Structure):
    """pag_bup20_prepare_args (include/pagnerf_hip.h)."""
    _fields_ = [("img", c_vp), ("depth", c_vp), ("sem", c_vp), ("inst", c_vp), ("sem_conf", c_vp), ("inst_conf", c_vp), ("counts", c_vp),
                ("B", c_i32), ("H0", c_i32), ("W0", c_i32), ("C0", c_i32), ("mip", c_i32), ("bg", c_i32), ("n_ids", c_i32),
                ("view_offset", c_i64), ("V", c_i64), ("imgs", c_vp), ("masks", c_vp), ("depths", c_vp), ("semantics_pred", c_vp),
                ("instance_pred", c_vp), ("sem_conf_out", c_vp), ("inst_conf_out", c_vp)]


COCO_MAX_PART_KEYS = 4096           # PAG_COCO_MAX_PART_KEYS

VIS_PICTURES, VIS_LABELS, VIS_MAX_ID = 15, 6, 1023


class VisArgs(ctypes.Structure):
    """pag_vis_args (include/pagnerf_hip.h): the validation pictures of pc_nerf/trainer.py:710-829, :855-896."""
    _fields_ = [("H", c_i32), ("W", c_i32), ("rgb", c_vp), ("rgb_is_u8", c_i32), ("rgb_stride", c_i32), ("gt", c_vp), ("gt_stride", c_i32), ("phase", c_i32),
                ("depth", c_vp), ("labels", c_vp * VIS_LABELS), ("label_bytes", c_i32 * VIS_LABELS), ("conf", c_vp * 2), ("table", c_vp),
                ("max_id", c_i32), ("box_width", c_i32), ("blend_keep", c_f32), ("blend_alpha", c_f32), ("overlay_keep", c_f32), ("overlay_alpha", c_f32),
                ("conf_min", c_f32), ("conf_max", c_f32), ("workspace", c_vp), ("workspace_bytes", c_i64), ("out", c_vp * VIS_PICTURES)]


_SIGS = {
    "pag_abi_version": (c_i32, []),
    "pag_last_error_string": (ctypes.c_char_p, []),
    "pag_encode_bwd_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32, c_i32, c_i64]),
    "pag_mlp_fwd": (c_i32, [ctypes.POINTER(MlpFwdArgs), c_i64, c_vp]),
    "pag_mlp_fwd_pair_supported": (c_i32, [ctypes.POINTER(MlpFwdArgs), ctypes.POINTER(MlpFwdArgs)]),
    "pag_mlp_fwd_composite_supported": (c_i32, [ctypes.POINTER(MlpFwdArgs), c_i64]),
    "pag_mlp_fwd_producer_supported": (c_i32, [ctypes.POINTER(MlpFwdArgs), ctypes.POINTER(MlpFwdArgs), c_i64]),
    "pag_mlp_bwd": (c_i32, [ctypes.POINTER(MlpBwdArgs), c_i64, c_vp]),
    "pag_mlp_bwd_fused_supported": (c_i32, [ctypes.POINTER(MlpBwdArgs)]),
    "pag_mlp_bwd_fused_workspace_bytes": (c_i64, [ctypes.POINTER(MlpBwdArgs), c_i64]),
    "pag_mlp_bwd_pair_supported": (c_i32, [ctypes.POINTER(MlpBwdArgs), ctypes.POINTER(MlpBwdArgs)]),
    "pag_head_composite_fwd": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "pag_mlp_wgrad_blocks": (c_i32, [c_i64]),
    "pag_mlp_wgrad_batch": (c_i32, [ctypes.POINTER(WgradLayer), c_i32, c_i64, c_vp]),
    "pag_mlp_wgrad_finish": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "pag_mlp_wgrad": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i64, c_vp]),
    "pag_raymarch_count": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_f32, c_f32, c_vp, c_i32, c_vp, c_vp]),
    "pag_pack_offsets": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "pag_pad_packed": (c_i32, [c_vp, c_i64, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_view_embed": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "pag_raymarch_pack": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_f32, c_f32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_raymarch_voxel_nugget_capacity": (c_i64, [c_i32]),
    "pag_raymarch_voxel_count_nuggets": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_f32, c_f32, c_vp, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp]),
    "pag_raymarch_voxel_pack_nuggets": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_ray_sample_grad": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "pag_affine_xcd8_fwd": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "pag_affine_xcd8_bwd_dx": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "pag_occupancy_update": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i64, c_f32, c_f32, c_vp]),
    "pag_label_sums": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "pag_assign_cost": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_float, ctypes.c_float, c_i32,
                                c_vp, c_vp, c_vp, c_vp]),
    "pag_sparse_rows_mask": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_vp, c_vp]),
    "pag_sparse_rows_plan": (c_i32, [c_vp, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "pag_sparse_rows_pack": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_sparse_rows_unpack": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_assign_solve": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_assign_nll_fwd": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_assign_nll_bwd": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_render_loss_workspace_bytes": (c_i64, []),
    "pag_render_loss_fwd": (c_i32, [c_vp, c_vp, c_i64, c_f32, c_vp, c_i32, c_vp, c_vp, c_f32, c_f32, c_i32, c_vp, c_i32, c_vp, c_vp, c_f32, c_f32, c_i32, c_f32, c_vp, c_vp, c_vp]),
    "pag_render_loss_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_vp, c_i32, c_vp, c_vp, c_f32, c_f32, c_i32, c_vp, c_i32, c_vp, c_vp, c_f32, c_f32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp]),
    "pag_composite_fwd": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "pag_composite_bwd": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "pag_composite_feats_fwd": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "pag_composite_feats_bwd": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp]),
    "pag_pack_offsets_pad": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_copy_batch": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_vp]),
    "pag_adam_step": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, c_i64, c_vp]),
    "pag_pose_rays_fwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "pag_pose_rays_bwd_workspace_bytes": (c_i64, [c_i64]),
    "pag_pose_rays_bwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "pag_view_embed_bwd": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "pag_pose_points": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "pag_segment_reg_workspace_bytes": (c_i64, [c_i32, c_i64]),
    "pag_segment_reg_fwd": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i32, ctypes.c_float, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "pag_segment_reg_bwd": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i32, ctypes.c_float, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "pag_supcon_workspace_bytes": (c_i64, [c_i32, c_i64, c_i32]),
    "pag_supcon_fwd": (c_i32, [c_vp, c_i32, c_i32, c_i64, c_i32, c_i64, c_i64, c_vp, c_vp, c_f32, c_f32, c_f32, c_f32, c_vp, c_i64, c_vp, c_vp]),
    "pag_supcon_bwd": (c_i32, [c_i32, c_i32, c_i64, c_i32, c_f32, c_f32, c_f32, c_f32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "pag_meanshift_workspace_bytes": (c_i64, [c_i32, c_i64, c_i32]),
    "pag_meanshift_fit": (c_i32, [c_vp, c_i32, c_i32, c_i64, c_i32, c_i64, c_i64, c_vp, ctypes.c_double, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp,
                                  c_vp]),
    "pag_meanshift_predict": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_i64, c_vp, c_i32, c_vp, c_vp]),
    "pag_panoptic_pq_workspace_bytes": (c_i64, [c_i32, c_i64, c_i64, c_i32]),
    "pag_panoptic_pq_update": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp,
                                       c_vp, c_vp, c_vp, c_vp]),
    "pag_panoptic_clean_workspace_bytes": (c_i64, [c_i64, c_i64]),
    "pag_panoptic_clean": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i64, c_i32, c_i32, c_i64, ctypes.c_double, c_vp, c_i64, c_vp, c_vp]),
    "pag_confusion_matrix": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "pag_mask_ap_workspace_bytes": (c_i64, [c_i64, c_i64, c_i32]),
    "pag_mask_ap_update": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_i64, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp,
                                   c_i64, c_vp, c_vp, c_vp, c_vp]),
    "pag_map_workspace_bytes": (c_i64, [c_i64]),
    "pag_map_points": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_vp,
                               c_f32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "pag_map_select": (c_i32, [c_vp, c_i64, c_vp, c_f32, c_vp, c_i32, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "pag_mesh_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "pag_mesh_vertices": (c_i32, [c_vp, c_i64, c_i64, c_i64, c_f32, c_fp, c_f32, c_ip, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "pag_mesh_faces": (c_i32, [c_vp, c_i64, c_i64, c_i64, c_f32, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "pag_voxel_workspace_bytes": (c_i64, [c_i64]),
    "pag_voxel_keys": (c_i32, [c_vp, c_i64, c_fp, c_f32, c_fp, c_vp, c_vp]),
    "pag_voxel_fuse": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "pag_label_table": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, ctypes.POINTER(ctypes.c_int64), c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp,
                                c_vp, c_i64, c_vp]),
    "pag_voxel_components_workspace_bytes": (c_i64, [c_i64]),
    "pag_voxel_components": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, ctypes.POINTER(ctypes.c_int64), c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "pag_voxel_overlap": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_i32, c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_overlap_cost": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "pag_voxel_merge": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "pag_mlp_dz0_slots_bytes": (c_i64, [c_i64, c_i64]),
    "pag_mlp_dz0_slots_sum": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "pag_encode_bwd_rays_workspace_bytes": (c_i64, [c_i64, c_i64]),
    "pag_deep_mlp_supported": (c_i32, [c_i32, c_i32]),
    "pag_deep_mlp_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32, c_i32]),
    "pag_deep_mlp_fwd": (c_i32, [ctypes.POINTER(DeepMlpArgs), c_i64, c_vp]),
    "pag_deep_mlp_bwd": (c_i32, [ctypes.POINTER(DeepMlpArgs), c_i64, c_vp]),
    "pag_mlp128_supported": (c_i32, [c_i32, c_i32, c_i32, c_i32]),
    "pag_mlp128_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32, c_i32]),
    "pag_mlp128_fwd": (c_i32, [ctypes.POINTER(Mlp128FwdArgs), c_i64, c_vp]),
    "pag_mlp128_bwd": (c_i32, [ctypes.POINTER(Mlp128BwdArgs), c_i64, c_vp]),
    "pag_vm_supported": (c_i32, [c_i32, c_i32, c_i32, c_i32]),
    "pag_vm_bwd_workspace_bytes": (c_i64, [c_i64]),
    "pag_vm_fwd": (c_i32, [ctypes.POINTER(VmArgs), c_i64, c_vp]),
    "pag_vm_bwd": (c_i32, [ctypes.POINTER(VmArgs), c_i64, c_vp]),
    "pag_triplanar_fwd": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i32, c_ip, c_fp, c_vp, c_i32, c_i64, c_i64, c_vp]),
    "pag_triplanar_bwd_tables": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_ip, c_fp, c_vp, c_vp]),
    "pag_triplanar_bwd_xyz": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_ip, c_fp, c_vp, c_vp]),
    "pag_tv_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_i64]),
    "pag_tv_fwd": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp]),
    "pag_tv_bwd": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "pag_sample_copy_width": (c_i32, [c_vp, c_vp, c_i64, c_i32]),
    "pag_sample_batch": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i64, c_i64, c_i64, c_i64, ctypes.POINTER(SampleMode), c_i32, c_vp, c_vp, c_vp]),
    "pag_sample_advance": (c_i32, [c_vp, c_vp]),
    "pag_vis_workspace_bytes": (c_i64, [c_i32]),
    "pag_vis_stats": (c_i32, [ctypes.POINTER(VisArgs), c_vp]),
    "pag_vis_paint": (c_i32, [ctypes.POINTER(VisArgs), c_vp]),
    "pag_prepare_views": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_f32, c_f32, c_f32, c_f32, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pag_prepare_labels": (c_i32, [ctypes.POINTER(LabelPlane), c_i32, c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_vp]),
    "pag_coco_keys": (c_i32, [ctypes.POINTER(CocoTables), c_i32, c_i32, c_vp]),
    "pag_coco_labels": (c_i32, [ctypes.POINTER(CocoTables), c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp]),
    "pag_bup20_pred_stats": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp, c_vp]),
    "pag_bup20_prepare": (c_i32, [ctypes.POINTER(Bup20PrepareArgs), c_vp]),
}

# The twelve grid-encoder entry points, pag_{hash,permuto}_encode_{fwd,fwd_add,bwd,bwd_set,bwd_xyz,bwd_rays}: the operation's leading arguments, the
# kind-specific middle (ops._EncodeSpec.mid() supplies its values in this order), the operation's trailing arguments.
_ENC_MID = {"hash": [c_i32, c_fp, c_fp],                    # log2_T, resolutions_host, feat_scale_host
            "permuto": [c_u32, c_fp, c_fp, c_fp]}           # capacity, scale_factor_host, shift_host, feat_scale_host
_ENC_FWD = [c_vp, c_i64, c_vp, c_i32, c_i32, c_i32]         # xyz, M, tables, table_dtype, n_levels, n_feat
_ENC_BWD = [c_vp, c_i64, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_i32]                  # xyz, M, grad_out, grad_dtype, g_stride_m, g_stride_c, layout, n_levels, n_feat
_ENC_XYZ = [c_vp, c_i64, c_vp, c_i32, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_i32]     # xyz, M, tables, table_dtype, then as _ENC_BWD from grad_out on
_ENC_OPS = {
    "fwd": (_ENC_FWD, [c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp]),                   # out, out_dtype, out_stride_m, out_stride_c, layout, flags, stream
    "fwd_add": (_ENC_FWD, [c_vp, c_vp, c_i32, c_vp]),                                     # addend, out, flags, stream
    "bwd": (_ENC_BWD, [c_vp, c_vp, c_i64, c_i32, c_vp]),                                  # grad_tables, workspace, workspace_bytes, flags, stream
    "bwd_set": (_ENC_BWD, [c_vp, c_vp, c_i64, c_i32, c_vp]),
    "bwd_xyz": (_ENC_XYZ, [c_vp, c_vp, c_i64, c_i32, c_vp]),                              # d_xyz, workspace, workspace_bytes, flags, stream
    "bwd_rays": (_ENC_XYZ, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_i32, c_vp]),    # ridx, depths, pack_start, N, out, workspace, workspace_bytes, flags, stream
}
_SIGS.update({"pag_%s_encode_%s" % (kind, op): (c_i32, head + mid + tail) for op, (head, tail) in _ENC_OPS.items() for kind, mid in _ENC_MID.items()})

EXPORTS = tuple(_SIGS)
_lib = None


def load():
    """dlopen the C-ABI library (building is __graft_entry__.build()'s job); raises if absent."""
    global _lib
    if _lib is None:
        path = _build.LIB
        if not os.path.exists(path):
            raise RuntimeError("libpagnerf_hip.so not found at %s - run `python -m pagnerf_amd.build` "
                               "(there is no CPU fallback for the HIP path)" % path)
        lib = ctypes.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.pag_abi_version() != ABI_VERSION:
            raise RuntimeError("libpagnerf_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def check(rc, name):
    if rc != 0:
        msg = load().pag_last_error_string().decode("utf-8", "replace")
        raise RuntimeError("%s failed (%d): %s" % (name, rc, msg))


def dtype_code(t):
    return _DT[t.dtype]


def ptr(t):
    """Device pointer of a contiguous GPU tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("pagnerf_amd: expected a GPU tensor (the HIP path has no CPU fallback), got %s" % t.device)
    if not t.is_contiguous():
        raise RuntimeError("pagnerf_amd: tensor must be contiguous")
    return t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """The raw handle of torch's current stream on the current device.  torch.cuda.current_stream() builds a Stream object per call (~10 us: a tenth of
    the host time of a forward-only trace, which asks nine times); the C-level getter returns the same handle in well under a microsecond."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def host_floats(values):
    """python/numpy/torch-CPU float sequence -> ctypes float array (kept alive by the caller)."""
    if values is None:
        return None
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().float().reshape(-1).tolist()
    else:
        import numpy as np
        values = np.asarray(values, dtype=np.float32).reshape(-1).tolist()
    return (ctypes.c_float * len(values))(*values)
