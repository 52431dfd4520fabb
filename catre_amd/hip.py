"""ctypes binding of ``libcatre_hip.so`` (C ABI declared in ``include/catre_hip.h``).

PyTorch is only plumbing here: device memory (``tensor.data_ptr()``), the current HIP stream
and, elsewhere, ``torch.distributed``.  There is NO fallback: if the library is missing or a
tensor is not on a HIP device, the call raises.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CATRE_HIP_LIB selects another build of the same ABI (the instrumented `make TRACE=1` library for profiles/trace_*.py)
LIB_PATH = os.environ.get("CATRE_HIP_LIB") or os.path.join(_HERE, "csrc", "libcatre_hip.so")

# state_dict keys in the order of `enum catre_param` (include/catre_hip.h)
PARAM_KEYS = (
    [f"pcl_net.stn.{l}.{p}" for l in ("conv1", "conv2", "conv3", "fc1", "fc2", "fc3") for p in ("weight", "bias")]
    + [f"pcl_net.{l}.{p}" for l in ("conv1", "conv2", "conv3", "conv4") for p in ("weight", "bias")]
    + [f"pcl_net.fstn.{l}.{p}" for l in ("conv1", "conv2", "conv3", "fc1", "fc2", "fc3") for p in ("weight", "bias")]
    + [
        f"rot_head.rot_head_{a}.{l}.{p}"
        for a in ("x", "y")
        for l in ("layers.0", "layers.1", "layers.3", "layers.4", "neck.0", "conv_p")
        for p in ("weight", "bias")
    ]
    + [
        f"ts_head.{l}.{p}"
        for l in ("linears.0", "linears.1", "linears.3", "linears.4", "fc_t", "fc_s")
        for p in ("weight", "bias")
    ]
)
CATRE_P_COUNT = len(PARAM_KEYS)
assert CATRE_P_COUNT == 68, CATRE_P_COUNT


class CatreOpts(ctypes.Structure):
    _fields_ = [
        ("feature_transform", ctypes.c_int32),
        ("with_kps_feature", ctypes.c_int32),
        ("with_init_scale", ctypes.c_int32),
        ("with_init_trans", ctypes.c_int32),
        ("delta_t_space_3d", ctypes.c_int32),
        ("delta_z_deepim", ctypes.c_int32),
        ("k_aware", ctypes.c_int32),
        ("scale_mul", ctypes.c_int32),
        ("scale_base_mean", ctypes.c_int32),
        ("is_allo", ctypes.c_int32),
        ("refine_scale", ctypes.c_int32),
        ("zero_center", ctypes.c_int32),
        ("delta_t_weight", ctypes.c_float),
        ("allo_eps", ctypes.c_float),
        ("ts_in_dim", ctypes.c_int32),
        ("rot_input_is_matrix", ctypes.c_int32),
        ("compute_dtype", ctypes.c_int32),
        ("rot_type", ctypes.c_int32),
    ]


DTYPE_F32, DTYPE_BF16, DTYPE_SPLIT, DTYPE_F16 = 0, 1, 2, 3
ROWS_BF16 = 0x100   # CATRE_ROWS_BF16
PACK_F32_ENCODER, PACK_F32_HEADS, PACK_BF16, PACK_SPLIT, PACK_F32_TAILS, PACK_ALL = 1, 2, 4, 8, 16, 31
PACK_F16 = 32       # CATRE_PACK_F16: the fp16 packs DTYPE_F16 reads (not part of PACK_ALL)
ROT_6D, ROT_QUAT, ROT_LOG_QUAT, ROT_LIE_VEC = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SILU, ACT_GELU, ACT_MISH = range(6)   # CATRE_ACT_*
ROT_DIMS = {ROT_6D: 6, ROT_QUAT: 4, ROT_LOG_QUAT: 3, ROT_LIE_VEC: 3}
OUT_DIMS = (64, 128, 256, 512, 1024)   # PCLNET.INIT_CFG.out_dim (conv4's width) the kernels are built for; 1024: every shipped config


def rot_type_id(rot_type):
    """'{ego,allo}_{rot6d,quat,log_quat,lie_vec}' -> CATRE_ROT_* (reference models/model_utils.py:11-40)."""
    for suffix, v in (("_rot6d", ROT_6D), ("_log_quat", ROT_LOG_QUAT), ("_quat", ROT_QUAT), ("_lie_vec", ROT_LIE_VEC)):
        if rot_type in ("ego" + suffix, "allo" + suffix):
            return v
    raise ValueError(f"Unknown rot_type: {rot_type}")  # model_utils.py:24


class CatreLossCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("pm_on", "pm_sym", "pm_with_scale", "rot_on", "rot_l2", "yaxis_smooth",
                                             "trans_on", "trans_mse", "trans_split", "scale_on", "scale_mse")] + \
               [(n, ctypes.c_float) for n in ("pm_lw", "rot_lw", "trans_lw", "scale_lw")]


class CatreLossCfg2(ctypes.Structure):
    """catre_loss_cfg2: the fields of catre_loss_cfg (reached by their own names) + the point-matching form."""
    _anonymous_ = ("base",)
    _fields_ = [("base", CatreLossCfg), ("pm_mode", ctypes.c_int32), ("pm_elem", ctypes.c_int32),
                ("pm_use_bbox", ctypes.c_int32), ("pm_beta", ctypes.c_float)]


# CATRE_PM_* / CATRE_PM_ELEM_* of include/catre_hip.h
PM_R_ONLY, PM_RT, PM_R_T_POINTS, PM_R_T_DIRECT, PM_R_XY_Z_POINTS, PM_R_XY_Z_DIRECT = range(6)
PM_ELEM_L1, PM_ELEM_SMOOTH_L1, PM_ELEM_MSE, PM_ELEM_L2 = range(4)
LOSS2_TERMS, LOSS2_PART = 8, 10


class CatrePoints(ctypes.Structure):
    _fields_ = [
        ("obs", ctypes.c_void_p), ("obs_sb", ctypes.c_int64), ("obs_sn", ctypes.c_int64), ("obs_sc", ctypes.c_int64),
        ("kps", ctypes.c_void_p), ("kps_sb", ctypes.c_int64), ("kps_sn", ctypes.c_int64), ("kps_sc", ctypes.c_int64),
        ("pose", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("apply_pose", ctypes.c_int32), ("zero_center", ctypes.c_int32),
    ]


_P = ctypes.c_void_p
_I = ctypes.c_int
_SZ = ctypes.c_size_t
_SIGS = {
    "catre_workspace_bytes": (_SZ, [_I, _I, _I]),
    "catre_packed_floats": (_SZ, [_I, _I, _I]),
    "catre_pack_weights": (_I, [_P, _I, _I, _I, _P, _SZ, _P]),
    "catre_pack_weights_sel": (_I, [_P, _I, _I, _I, _P, _SZ, _I, _P]),
    "catre_op_rows_compact": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "catre_op_maxlin_bwd_x_compact": (_I, [_P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "catre_op_maxlin_bwd_x_compact_h": (_I, [_P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "catre_op_maxlin_bwd_x_compact_cm": (_I, [_P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "catre_op_maxlin_bwd_w_c": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "catre_op_stn_recompute": (_I, [_I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "catre_op_gather_rows": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "catre_op_scatter_rows": (_I, [_P, _I, _P, _P, _I, _I, _I, _P]),
    "catre_op_scatter_rows_merge": (_I, [_P, _I, _P, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "catre_op_gemm_rows_n": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "catre_op_gemm_tn_bias_n": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _SZ, _P, _I, _P]),
    "catre_op_gemm_rows_nr": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "catre_op_gemm_tn_bias_nr": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _SZ, _P, _I, _P]),
    "catre_train_stn3d_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _I, _P]),
    "catre_train_stnkd_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _I, _P]),
    "catre_train_trunk_fwd": (_I, [_P] * 12 + [_P, _SZ, _I, _I, _I, _I, _P]),
    "catre_pose_apply": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "catre_stn3d_pool": (_I, [_P, _P, _P, _P, _P, _SZ, _I, _I, _I, _P]),
    "catre_linear": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "catre_linear_t": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    "catre_stnkd_pool": (_I, [_P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _P]),
    "catre_trunk": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _P]),
    "catre_packed_floats_w": (_SZ, [_I]),
    "catre_pack_encoder_w": (_I, [_P, _I, _P, _SZ, _P]),
    "catre_trunk_w": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _SZ, _I, _I, _I, _P]),
    "catre_trunk_screen_probe": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _P]),
    "catre_ts_head": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _P]),
    "catre_rot_head": (_I, [_P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _P]),
    "catre_rot_head_dim": (_I, [_P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _I, _P]),
    "catre_rot_to_mat": (_I, [_P, _I, _P, _I, _P]),
    "catre_rot_to_mat_bwd": (_I, [_P, _I, _P, _P, _I, _P]),
    "catre_pose_update": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "catre_refine_iter": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _P]),
    "catre_refine_k": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _I, _P]),
    "catre_stn_screen_probe": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _P]),
    "catre_form_switch": (_I, [_I, _I]),
    "catre_screen_run_len": (_I, [_I]),
    "catre_screen_run_rule": (_I, [_I, _I, _I, _I]),
    "catre_form_decision": (_I, [_I] * 12 + [ctypes.POINTER(ctypes.c_int)]),
    "catre_refine_k_from": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _I, _P]),
    "catre_colmax": (_I, [_P, _P, _I, _I, _I, _P]),
    # training ops (include/catre_hip.h "training ops")
    "catre_op_pack": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "catre_op_gemm_rows": (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "catre_op_linear_maxpool_ws_bytes": (_SZ, [_I, _I]),
    "catre_op_linear_maxpool": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "catre_op_pack_bf16": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "catre_op_gemm_rows_bf16": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "catre_op_linear_maxpool_bf16": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "catre_op_gemm_rows_cloudbias": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "catre_op_gemm_rows_gn": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "catre_op_gnp_gelu_fwd_pre": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "catre_op_pack_split": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "catre_op_gemm_rows_split": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "catre_op_linear_maxpool_split": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "catre_op_gemm_tn_ws_bytes": (_SZ, [_I, _I, _I]),
    "catre_op_gemm_tn": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _SZ, _P]),
    "catre_op_gemm_rows_m": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "catre_op_gemm_tn_bias_m": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _SZ, _P]),
    "catre_op_gemm_tn_bias_lp": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _SZ, _I, _P]),
    "catre_op_gemm_tn_bias_ws_bytes": (_SZ, [_I, _I, _I]),
    "catre_op_fc_bwd": (_I, [_P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "catre_op_skinny_bwd": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _I, _P, _SZ, _P]),
    "catre_op_gemm_tn_bias": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _SZ, _P]),
    "catre_op_colsum": (_I, [_P, _I, _I, _I, _P, _I, _P, _SZ, _P]),
    "catre_op_reduce_splits": (_I, [_P, _P, _I, _I, _I, _P]),
    "catre_op_rowbias_add": (_I, [_P, _I, _P, _I, _I, _I, _I, _P]),
    "catre_op_rowbias_bwd": (_I, [_P, _I, _P, _I, _I, _I, _I, _P]),
    "catre_op_maxpool_fwd": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "catre_op_maxpool_scatter": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "catre_op_maxlin_bwd_w": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "catre_op_maxlin_bwd_w_h": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "catre_op_maxlin_bwd_x": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    "catre_op_maxlin_bwd_x_rows": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "catre_op_cloud_matmul": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "catre_op_cloud_matmul_tpw": (_I, [_I, _I, _I]),
    "catre_op_cloud_matmul_bwd_t": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    "catre_op_relu_bwd": (_I, [_P, _P, _P, _SZ, _P]),
    "catre_op_sum_rows": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "catre_op_gnp_gelu_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _P]),
    "catre_op_gnp_gelu_neck_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "catre_op_gnp_gelu_neck_bwd_ws_bytes": (_SZ, [_I, _I]),
    "catre_op_gnp_gelu_neck_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _SZ, _I, _I, _P]),
    "catre_op_rot_l0_bwd_ws_bytes": (_SZ, [_I, _I, _I]),
    "catre_op_rot_l0_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _SZ, _I, _I, _I, _P]),
    "catre_op_rot_l0_bwd_lp": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _SZ, _I, _I, _I, _P]),
    "catre_op_rot_l0_bwd_sp": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _SZ, _I, _I, _I, _P]),
    "catre_op_gnp_gelu_neck_fwd_s": (_I, [_P] * 10 + [_I, _I, _P]),
    "catre_op_rot_l1_bwd_s": (_I, [_P] * 14 + [_SZ, _I, _I, _P]),
    "catre_op_rot_l1_bwd_lp": (_I, [_P] * 14 + [_SZ, _I, _I, _P]),
    "catre_op_rot_l1_bwd_sp": (_I, [_P] * 14 + [_SZ, _I, _I, _P]),
    "catre_op_rot_l1_bwd_h": (_I, [_P] * 14 + [_SZ, _I, _I, _P]),
    "catre_op_rot_l0_bwd_h": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _SZ, _I, _I, _I, _P]),
    "catre_op_gemm_rows_gn_h": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "catre_op_gnp_gelu_fwd_pre_h": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "catre_op_gnp_gelu_neck_fwd_s_h": (_I, [_P] * 10 + [_I, _I, _P]),
    "catre_op_gn_gelu_gemm_rows_h": (_I, [_P] * 10 + [_I, _I, _I, _P]),
    "catre_op_gnp_gelu_neck_bwd_s": (_I, [_P] * 11 + [_SZ, _I, _I, _P]),
    "catre_op_pad_cols": (_I, [_P, ctypes.c_long, ctypes.c_long, _I, _I, _P, _I, _P]),
    "catre_op_rot_l1_bwd_ws_bytes": (_SZ, [_I, _I]),
    "catre_op_rot_l1_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _P]),
    "catre_op_gnp_gelu_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _SZ, _I, _I, _P]),
    "catre_op_gnr_gelu_fwd": (_I, [_P, _P, _P, _P, _I, _P]),
    "catre_op_gnr_gelu_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _SZ, _I, _P]),
    "catre_op_gnp_act_fwd": (_I, [_P] * 5 + [_I] * 6 + [_P]),
    "catre_op_gnp_act_bwd_ws_bytes": (_SZ, [_I, _I, _I, _I]),
    "catre_op_gnp_act_bwd": (_I, [_P] * 8 + [_I, _P, _SZ] + [_I] * 6 + [_P]),
    "catre_op_gnr_act_fwd": (_I, [_P] * 4 + [_I] * 5 + [_P]),
    "catre_op_gnr_act_bwd_ws_bytes": (_SZ, [_I, _I]),
    "catre_op_gnr_act_bwd": (_I, [_P] * 7 + [_I, _P, _SZ] + [_I] * 5 + [_P]),
    "catre_op_gnp_act_neck_wsum_ws_bytes": (_SZ, [_I, _I, _I]),
    "catre_op_gnp_act_neck_wsum": (_I, [_P] * 9 + [_SZ] + [_I] * 7 + [_P]),
    "catre_op_wsum_fwd": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "catre_op_wsum_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _SZ, _I, _I, _P]),
    "catre_op_wsum_bwd_n": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _SZ, _I, _I, _P]),
    "catre_op_pose_update_bwd": (_I, [_P] * 13 + [_I, _P]),
    "catre_train_rot_fwd_ws_bytes": (_SZ, [_I]),
    "catre_train_rot_fwd": (_I, [_P] * 10 + [_SZ, _I, _I, _I, _I, _P]),
    "catre_op_ranger_step": (_I, [_P, _I, _P, _I, _P, _I, _P, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                  ctypes.c_float, _I, ctypes.c_float, _P]),
    "catre_op_optim_step": (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _P, _SZ, _I, ctypes.c_float, _P]),
    "catre_aug_points": (_I, [_P] * 10 + [_I, _I, _P]),
    "catre_init_noise": (_I, [_P, _P, _P, ctypes.c_float, ctypes.c_float, _P, _P, _P, ctypes.c_float, ctypes.c_float, _P, _I,
                              _P]),
    "catre_pcl_workspace_bytes": (_SZ, [_I, _I, _I]),
    "catre_pcl_candidates": (_I, [_P, _P, _P, _P, _P, ctypes.c_float, _I, _I, _I, _I, _P, _SZ, _P, _P]),
    "catre_pcl_sample": (_I, [_P, _P, _P, _SZ, _P, ctypes.c_uint64, _I, _I, _I, _I, _P, _P, _P]),
    "catre_pcl_fps": (_I, [_P, _P, _P, _SZ, _I, _I, _I, _I, _P, _I, _P, _P]),
    "catre_pclf_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "catre_pclf_candidates": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, ctypes.c_float, _I, _I, _I, _I, _I, _P, _SZ, _P, _P]),
    "catre_pclf_sample": (_I, [_P, _P, _P, _P, _P, _SZ, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "catre_pclf_fps": (_I, [_P, _P, _P, _P, _SZ, _I, _I, _I, _I, _I, _P, _I, _P, _P]),
    "catre_depth_augment": (_I, [_P, _I, ctypes.c_float, _P, _I, _P, _P, _P, ctypes.c_uint64, _P, _I, _I, _I, _P]),
    # initial poses from a NOCS map (include/catre_hip.h "batched RANSAC Umeyama", catre_amd/nocs_align.py)
    "catre_umeyama": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "catre_nocs_align_workspace_bytes": (_SZ, [_I, _I, _I]),
    "catre_nocs_align": (_I, [_P, _P, _P, _P, ctypes.c_uint64, _P, _I, _I, _I, ctypes.c_double, ctypes.c_double, _P, _SZ]
                         + [_P] * 9),
    "catre_nocs_align_draws": (_I, [_P, ctypes.c_uint64, _P, _I, _I, _P, _P]),
    # tracking (include/catre_hip.h "tracking: nearest-neighbour statistics and the track gate", catre_amd/tracking.py)
    "catre_nn_stats_workspace_bytes": (_SZ, [_I, _I, _I]),
    "catre_nn_stats": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "catre_track_gate": (_I, [_P] * 7 + [ctypes.c_float, _I, _I] + [_P] * 5),
    # trimmed ICP (include/catre_hip.h "trimmed ICP", catre_amd/icp.py)
    "catre_icp_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "catre_icp_step": (_I, [_P, _I, _P, _P, _I] + [_P] * 5 + [ctypes.c_float, _I, _I, _I] + [_P] * 7),
    "catre_icp": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, ctypes.c_float, _I, _I, _I] + [_P] * 6 + [_SZ, _P]),
    # splat render of the posed prior (include/catre_hip.h "splat render of the posed prior", catre_amd/render.py)
    "catre_splat_workspace_bytes": (_SZ, [_I, _I, _I]),
    "catre_splat_render": (_I, [_P] * 7 + [ctypes.c_float, ctypes.c_float] + [_I] * 5 + [_P, _SZ] + [_P] * 8),
    # mesh rasteriser (include/catre_hip.h "rasteriser of posed triangle meshes", catre_amd/render.py render_mesh)
    "catre_mesh_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "catre_mesh_render": (_I, [_P] * 12 + [ctypes.c_float] + [_I] * 10 + [_P, _SZ] + [_P] * 10),
    # BOP pose errors (include/catre_hip.h "BOP pose errors: MSSD, MSPD, proj_sym and VSD", catre_amd/pose_errors.py)
    "catre_sym_err_workspace_bytes": (_SZ, [_I, _I]),
    "catre_sym_err": (_I, [_P, _I, _I] + [_P] * 8 + [_I] * 4 + [_P, _SZ] + [_P] * 4),
    "catre_vsd": (_I, [_P] * 8 + [ctypes.c_float] + [_I] * 8 + [_P] * 3),
    "catre_loss_fwd": (_I, [_P] * 15 + [_I, _I, _I, _P]),
    "catre_loss_bwd": (_I, [_P] * 14 + [_I, _I, _I, _P]),
    "catre_loss_fwd_sums": (_I, [_P] * 16 + [_I, _P, _I, _I, _I, _P]),
    "catre_loss_bwd_sums": (_I, [_P] * 13 + [_I, _P, _P, _P, _I, _I, _I, _P]),
    "catre_loss_fwd2": (_I, [_P] * 16 + [_I, _P, _I, _I, _I, _P]),
    "catre_loss_bwd2": (_I, [_P] * 13 + [_I, _P, _P, _P, _I, _I, _I, _P]),
    "catre_loss_fwd3": (_I, [_P] * 16 + [_I, _P, _I, _I, _I, _P, _P]),
    "catre_loss_bwd3": (_I, [_P] * 13 + [_I, _P, _P, _P, _I, _I, _I, _P, _P]),
    # evaluation (include/catre_hip.h "evaluation of refined poses", catre_amd/evaluation.py)
    "catre_eval_overlaps": (_I, [_P] * 14 + [_I] * 6 + [_P]),
    "catre_eval_match_iou": (_I, [_P] * 7 + [_I] * 6 + [_P]),
    "catre_eval_match_pose": (_I, [_P] * 6 + [_I, _I] + [_P] * 4 + [_I] * 7 + [_P]),
    "catre_profile_enable": (_I, [_I, _I]),
    "catre_profile_collect": (_I, [_P, _I, _P]),
    "catre_debug_trunk_trace": (_I, [_P]),
    "catre_debug_knob": (_I, [_I, _I]),
    "catre_debug_screen_counts": (_I, [_P, _I]),
    "catre_stream_capture_id": (_I, [_P, _P]),
    "catre_status_string": (ctypes.c_char_p, [_I]),
    "catre_version": (ctypes.c_char_p, []),
}
EXPORTED_SYMBOLS = tuple(_SIGS)

KERNEL_IDS = {"stn3d": 0, "stnkd": 1, "trunk": 2, "ts_head": 3, "rot_l0_stats": 4, "rot_l1": 5, "rot_out": 6, "colmax": 7}

_lib = None

# Parameters updated through raw pointers (the fused Ranger step) do not bump torch's per-tensor version counter, so
# everything that caches a derived form of the weights (HipRuntime's packed images) also keys on this epoch.
_param_epoch = [0]


def bump_param_epoch():
    """Tell every runtime that parameters may have been rewritten out of band.

    The packed weight images are rebuilt when a parameter's ``(data_ptr, _version)`` changes - what ``load_state_dict``,
    ``p.copy_()`` and the optimizers do.  Writes through ``p.data`` (EMA updates, some third-party optimizers) bump neither;
    INFERENCE callers that do that call this once afterwards.  The training forward does not depend on it: its first
    kernel re-packs every image the forward reads on every call (``HipRuntime.train_stn3d``; with ``PCLNET.FREEZE`` the
    frozen-encoder branch of ``train_forward.forward_train`` does the same before the inference encoder kernels)."""
    _param_epoch[0] += 1


FORM_IDS = {"trunk4": 0, "stn4": 1, "stn_pair": 2, "rotw": 3, "fc_tail": 4, "screen": 5, "screen_stn": 6, "screen_pool": 7,
            "screen_run": 8, "screen_f16": 9,
            # no bit of the form word (ids 10 - 12 are the raw bits of the env-only STN arms): the epilogue of the `screen_f16` kernels
            "screen_epi": 13,
            # likewise no bits of the form word: the bound the `screen_f16` kernels select with (eps from the measured
            # activation rounding and the sign-split weight error), and its arm for the two STN kernels
            "screen_da": 14, "screen_da_stn": 15}


def form_switch(name, value=None):
    """Kernel-form switch `name` (``FORM_IDS``) of the loaded library: set it (True / False) or just query (None);
    returns the previous setting.  All forms of a stage give the same bits - for A/B measurements and form-vs-form tests."""
    r = load().catre_form_switch(FORM_IDS[name], -1 if value is None else int(bool(value)))
    if r < 0:
        raise CatreHipError(f"unknown kernel-form switch {name!r}")
    return bool(r)


def screen_run_len(value=None):
    """Run length of the `screen_run` form (tiles of one cloud a workgroup of k_trunk4sr walks): an int 1 .. 16 forces it,
    0 returns to the library's rule (``screen_run_rule``), None only queries; returns the previous value (0: the rule)."""
    return load().catre_screen_run_len(-1 if value is None else int(value))


def screen_run_rule(B, N, M, cus=256):
    """The run length the library's rule picks for a (B, N, M) grid on `cus` compute units (a pure host function)."""
    return load().catre_screen_run_rule(B, N, M, cus)


def cloud_matmul_tpw(B, N, M):
    """The 64-row tiles of one cloud a workgroup of the kd = 64 ``catre_op_cloud_matmul`` launch takes (4 or 1) for a
    (B, N, M) batch: a pure host function of the library, the one the launch calls."""
    r = load().catre_op_cloud_matmul_tpw(B, N, M)
    if r < 0:
        raise CatreHipError(f"catre_op_cloud_matmul_tpw: no launch takes B, N, M = {B}, {N}, {M}")
    return r


# catre_kernel_form, in the order the launches try them
KERNEL_FORMS = ("unsupported", "split_rs", "run_f16", "run", "screen_f16", "screen_pool", "screen", "pair", "wave4", "rs8",
                "bf_pair", "bf", "train_split", "train_pair", "train_wave4", "train_rs1", "train_bf_pair", "train_bf")
# bits of `switches`: ``FORM_IDS`` and the STN arms, which follow the environment only (CATRE_SCREEN_POOL_STN / _RUN_STN / _F16_STN)
SWITCH_BITS = dict({k: v for k, v in FORM_IDS.items() if v < 10}, screen_pool_stn=10, screen_run_stn=11, screen_f16_stn=12)
STAGES = {"stn3d": 0, "stnkd": 1, "trunk": 2}
MODES = {"fp32": 0, "split": 1, "bf16": 2}


def form_decision(stage, mode, B, N, M, switches, save=False, rows=False, probe=False, cus=256, run_len=0, bf_pair_min=512):
    """The kernel form one launch of `stage` (``STAGES``) in `mode` (``MODES``) takes under the switch word `switches`
    (``SWITCH_BITS``): (form name of ``KERNEL_FORMS``, workgroups per tile, tiles - STN stages: pairs - per run, grid).
    A pure host function of the library, the one its launches call; None for arguments no caller can produce."""
    out = (ctypes.c_int * 4)()
    if load().catre_form_decision(STAGES[stage], MODES[mode], int(save), int(rows), int(probe), B, N, M, switches, cus, run_len,
                                  bf_pair_min, out):
        return None
    return KERNEL_FORMS[out[0]], out[1], out[2], out[3]


def capture_id(device):
    """Identity of the capture the current stream of ``device`` is recording into (0: not capturing)."""
    out = ctypes.c_ulonglong(0)
    check(load().catre_stream_capture_id(stream_ptr(device), ctypes.byref(out)), "catre_stream_capture_id")
    return int(out.value)


def param_epoch():
    return _param_epoch[0]


class CatreHipError(RuntimeError):
    pass


def load():
    """Load the HIP library (once).  Raises ``CatreHipError`` if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CatreHipError(
            f"{LIB_PATH} not found - build it with `make -C catre_amd/csrc` (or `python -c "
            "'import __graft_entry__ as g; g.build()'`).  catre_amd has no CPU or PyTorch fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library drifted apart
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().catre_status_string(status).decode()
        raise CatreHipError(f"{what} failed: {msg} (status {status})")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device=None):
    """The current stream of `device` (a torch.device, an index or None = the current device) as a `void*`.  Through torch's
    raw-stream accessor when it exists: `torch.cuda.current_stream()` builds a Stream object per call - 5 us, ~70 times per
    training iteration."""
    if _raw_stream is not None:
        if device is None:
            idx = torch.cuda.current_device()
        elif isinstance(device, int):
            idx = device
        else:
            if isinstance(device, str):
                device = torch.device(device)
            idx = device.index if device.index is not None else torch.cuda.current_device()
        return ctypes.c_void_p(_raw_stream(idx))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def require_dev_f32(t, name, shape=None, contiguous=True):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise CatreHipError(
            f"{name} is on {t.device}; catre_amd runs on HIP devices only (no CPU fallback - the CPU "
            "restatement lives in oracle/ and is test infrastructure)"
        )
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if shape is not None:
        if t.dim() != len(shape) or any(e is not None and int(a) != int(e) for a, e in zip(t.shape, shape)):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def points_desc(x, tfd_kps):
    """Describe the reference's ``x [B,3,N]`` / ``tfd_kps [B,3,M]`` inputs (arbitrary strides, e.g. the
    permuted views produced by ``engine/batch_test.py:91-94``) for the kernels - no copy."""
    require_dev_f32(x, "x", (None, 3, None), contiguous=False)
    require_dev_f32(tfd_kps, "tfd_kps", (x.shape[0], 3, None), contiguous=False)
    d = CatrePoints()
    d.obs, d.obs_sb, d.obs_sc, d.obs_sn = x.data_ptr(), x.stride(0), x.stride(1), x.stride(2)
    d.kps, d.kps_sb, d.kps_sc, d.kps_sn = tfd_kps.data_ptr(), tfd_kps.stride(0), tfd_kps.stride(1), tfd_kps.stride(2)
    return d


def param_array(tensors):
    """``tensors``: list in ``PARAM_KEYS`` order (``None`` allowed only for conv_p.bias)."""
    arr = (ctypes.c_void_p * CATRE_P_COUNT)()
    for i, t in enumerate(tensors):
        if t is None:
            arr[i] = None
        else:
            require_dev_f32(t, PARAM_KEYS[i])
            arr[i] = t.data_ptr()
    return arr


def profile_kernel(name, max_records):
    """Start recording HIP-event pairs around every launch of kernel ``name`` (``None`` disables)."""
    check(load().catre_profile_enable(-1 if name is None else KERNEL_IDS[name], int(max_records)), "catre_profile_enable")


def profile_collect(max_records):
    """-> list of per-launch durations in ms (synchronises on the recorded events)."""
    buf = (ctypes.c_float * max_records)()
    n = ctypes.c_int(0)
    check(load().catre_profile_collect(buf, max_records, ctypes.byref(n)), "catre_profile_collect")
    return [buf[i] for i in range(n.value)]
