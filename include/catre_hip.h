/*
 * catre_hip.h - C ABI of the MI355X (gfx950) implementation of CATRE's pose-refine hot path.
 *
 * The reference (THU-DA-6D-Pose-Group/CATRE) is 100 % Python on stock torch ops and has no FFI
 * of its own; each entry point below names the reference Python function (file:line, relative
 * to the reference root) whose arithmetic it replaces.  Host code binds these with ctypes
 * (catre_amd/hip.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless noted; tensors are dense row-major
 *     unless strides are passed explicitly (strides are in ELEMENTS);
 *   - B objects, N observed points, M shape-prior points per object; "cloud" c in [0,2B):
 *     c <  B -> observed cloud of object c      (N points)
 *     c >= B -> transformed prior of object c-B (M points)
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*); nothing
 *     allocates, frees or synchronises; scratch comes from the caller's `workspace`;
 *   - return value: CATRE_OK (0) or a negative catre_status; kernels never abort.
 */
#ifndef CATRE_HIP_H
#define CATRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum catre_status {
  CATRE_OK = 0,
  CATRE_ERR_BAD_ARG = -1,      /* null pointer, non-positive size, unsupported option */
  CATRE_ERR_WORKSPACE = -2,    /* workspace / packed buffer too small */
  CATRE_ERR_LAUNCH = -3,       /* hipGetLastError() != hipSuccess after a launch */
  CATRE_ERR_UNSUPPORTED = -4   /* configuration outside what the kernels implement */
} catre_status;

/* Parameter tensors, in the reference's state_dict layout.  Conv1d weights
 * are [out,in,1] == [out,in] row-major.  `params[CATRE_P_xxx]` is the device pointer. */
typedef enum catre_param {
  CATRE_P_STN_CONV1_W = 0, CATRE_P_STN_CONV1_B,   /* pcl_net.stn.conv1   [64,3]      */
  CATRE_P_STN_CONV2_W, CATRE_P_STN_CONV2_B,       /* pcl_net.stn.conv2   [128,64]    */
  CATRE_P_STN_CONV3_W, CATRE_P_STN_CONV3_B,       /* pcl_net.stn.conv3   [1024,128]  */
  CATRE_P_STN_FC1_W, CATRE_P_STN_FC1_B,           /* pcl_net.stn.fc1     [512,1024]  */
  CATRE_P_STN_FC2_W, CATRE_P_STN_FC2_B,           /* pcl_net.stn.fc2     [256,512]   */
  CATRE_P_STN_FC3_W, CATRE_P_STN_FC3_B,           /* pcl_net.stn.fc3     [9,256]     */
  CATRE_P_CONV1_W, CATRE_P_CONV1_B,               /* pcl_net.conv1       [64,3]      */
  CATRE_P_CONV2_W, CATRE_P_CONV2_B,               /* pcl_net.conv2       [128,64]    */
  CATRE_P_CONV3_W, CATRE_P_CONV3_B,               /* pcl_net.conv3       [512,128]   */
  CATRE_P_CONV4_W, CATRE_P_CONV4_B,               /* pcl_net.conv4       [1024,512]  */
  CATRE_P_FSTN_CONV1_W, CATRE_P_FSTN_CONV1_B,     /* pcl_net.fstn.conv1  [64,64]     */
  CATRE_P_FSTN_CONV2_W, CATRE_P_FSTN_CONV2_B,     /* pcl_net.fstn.conv2  [128,64]    */
  CATRE_P_FSTN_CONV3_W, CATRE_P_FSTN_CONV3_B,     /* pcl_net.fstn.conv3  [1024,128]  */
  CATRE_P_FSTN_FC1_W, CATRE_P_FSTN_FC1_B,         /* pcl_net.fstn.fc1    [512,1024]  */
  CATRE_P_FSTN_FC2_W, CATRE_P_FSTN_FC2_B,         /* pcl_net.fstn.fc2    [256,512]   */
  CATRE_P_FSTN_FC3_W, CATRE_P_FSTN_FC3_B,         /* pcl_net.fstn.fc3    [4096,256]  */
  /* rot_head.rot_head_x.* then rot_head.rot_head_y.* (12 tensors each) */
  CATRE_P_ROTX_L0_W, CATRE_P_ROTX_L0_B,           /* layers.0  [256,1088]            */
  CATRE_P_ROTX_GN0_W, CATRE_P_ROTX_GN0_B,         /* layers.1  [256]                 */
  CATRE_P_ROTX_L1_W, CATRE_P_ROTX_L1_B,           /* layers.3  [256,256]             */
  CATRE_P_ROTX_GN1_W, CATRE_P_ROTX_GN1_B,         /* layers.4  [256]                 */
  CATRE_P_ROTX_NECK_W, CATRE_P_ROTX_NECK_B,       /* neck.0    [3,256]               */
  CATRE_P_ROTX_CONVP_W, CATRE_P_ROTX_CONVP_B,     /* conv_p    [1,N+M] , [1] (bias may be NULL) */
  CATRE_P_ROTY_L0_W, CATRE_P_ROTY_L0_B,
  CATRE_P_ROTY_GN0_W, CATRE_P_ROTY_GN0_B,
  CATRE_P_ROTY_L1_W, CATRE_P_ROTY_L1_B,
  CATRE_P_ROTY_GN1_W, CATRE_P_ROTY_GN1_B,
  CATRE_P_ROTY_NECK_W, CATRE_P_ROTY_NECK_B,
  CATRE_P_ROTY_CONVP_W, CATRE_P_ROTY_CONVP_B,
  CATRE_P_TS_L0_W, CATRE_P_TS_L0_B,               /* ts_head.linears.0 [256,ts_in]   */
  CATRE_P_TS_GN0_W, CATRE_P_TS_GN0_B,             /* ts_head.linears.1 [256]         */
  CATRE_P_TS_L1_W, CATRE_P_TS_L1_B,               /* ts_head.linears.3 [256,256]     */
  CATRE_P_TS_GN1_W, CATRE_P_TS_GN1_B,             /* ts_head.linears.4 [256]         */
  CATRE_P_TS_FCT_W, CATRE_P_TS_FCT_B,             /* ts_head.fc_t      [3,256]       */
  CATRE_P_TS_FCS_W, CATRE_P_TS_FCS_B,             /* ts_head.fc_s      [3,256]       */
  CATRE_P_COUNT
} catre_param;

/* Options of one refine iteration: the flags `CATRE_disR_shared.forward` reads from
 * cfg.MODEL.CATRE.{ROT_HEAD,TS_HEAD} and cfg.INPUT (core/catre/models/CATRE_disR_shared.py:57-120). */
typedef struct catre_opts {
  int32_t feature_transform;   /* PCLNET.INIT_CFG.feature_transform (pointnet.py:105)            */
  int32_t with_kps_feature;    /* TS_HEAD.WITH_KPS_FEATURE  (CATRE_disR_shared.py:71-75)         */
  int32_t with_init_scale;     /* TS_HEAD.WITH_INIT_SCALE   (:78-79)                             */
  int32_t with_init_trans;     /* TS_HEAD.WITH_INIT_TRANS   (:80-82)                             */
  int32_t delta_t_space_3d;    /* 0: "image", 1: "3D"  (pose_scale_from_delta_init.py:51,72)     */
  int32_t delta_z_deepim;      /* 0: "cosypose", 1: "deepim" (:55-61)                            */
  int32_t k_aware;             /* T_TRANSFORM_K_AWARE (:63-69)                                   */
  int32_t scale_mul;           /* 0: "add" in SCLAE_TYPE, 1: multiplicative exp (:79-84)          */
  int32_t scale_base_mean;     /* 0: "iter" in SCLAE_TYPE (base = current scale), 1: mean_scales  */
  int32_t is_allo;             /* "allo" in ROT_TYPE (:87-90)                                    */
  int32_t refine_scale;        /* cfg.MODEL.REFINE_SCLAE (CATRE_disR_shared.py:119-120)          */
  int32_t zero_center;         /* cfg.INPUT.ZERO_CENTER_INPUT (engine/batch_test.py:84-97)       */
  float   delta_t_weight;      /* DELTA_T_WEIGHT (:48)                                           */
  float   allo_eps;            /* eps of allo_to_ego_mat_torch, 1e-4 (CATRE_disR_shared.py:112)  */
  int32_t ts_in_dim;           /* TS_HEAD.INIT_CFG.in_dim; must equal the gathered feature width */
  int32_t rot_input_is_matrix; /* catre_pose_update only: `rot6d` holds [B,3,3] matrices (get_rot_mat already applied) */
  int32_t compute_dtype;       /* catre_refine_iter / catre_refine_k: CATRE_DTYPE_F32 (default) or CATRE_DTYPE_BF16 -
                                * what torch.cuda.amp.autocast selects in the reference (engine.py:304, TEST.AMP_TEST):
                                * bf16 GEMM operands, fp32 accumulation / GroupNorm statistics / SO(3) update;
                                * CATRE_DTYPE_SPLIT; or CATRE_DTYPE_F16 - the bf16 path's structure with fp16 operands
                                * (the dtype of the reference's autocast on "cuda").  F16 is inference only:
                                * catre_refine_iter, catre_refine_k and catre_refine_k_from accept it, and their
                                * `packed` image must have been made with CATRE_PACK_F16; every other entry point that
                                * takes a compute_dtype returns CATRE_ERR_UNSUPPORTED for it                            */
  int32_t rot_type;            /* parametrisation of the rotation residual, the part of ROT_HEAD.ROT_TYPE after ego_/allo_
                                * (get_rot_mat, core/catre/models/model_utils.py:28-40): CATRE_ROT_6D (default, [B,6]),
                                * CATRE_ROT_QUAT ([B,4]), CATRE_ROT_LOG_QUAT ([B,3]), CATRE_ROT_LIE_VEC ([B,3]).  The fused
                                * drivers take the two rot heads' concatenated output [B, 2*rot_dim], so they accept the
                                * types whose width is even: 6D (rot_dim 3) and QUAT (rot_dim 2) - exactly the ones the
                                * reference's ConvOutPerRotHead can feed to get_rot_mat                                 */
} catre_opts;

enum { CATRE_ROT_6D = 0, CATRE_ROT_QUAT = 1, CATRE_ROT_LOG_QUAT = 2, CATRE_ROT_LIE_VEC = 3 };

/* CATRE_DTYPE_SPLIT: fp32 results from split-bf16 (hi + lo, three products) MFMAs on the layers holding 98 % of the FLOPs;
 * same parity bound as CATRE_DTYPE_F32 */
enum { CATRE_DTYPE_F32 = 0, CATRE_DTYPE_BF16 = 1, CATRE_DTYPE_SPLIT = 2, CATRE_DTYPE_F16 = 3 };
/* OR-ed into the compute_dtype of catre_op_gemm_rows_nr / catre_op_gemm_tn_bias_nr (with CATRE_DTYPE_BF16): the row-indexed
 * dense tensor - `mask` / `X` - holds bf16 rows (leading dimension in ELEMENTS): the activation rows the autocast encoder
 * forward saves (catre_train_*_fwd with CATRE_DTYPE_BF16) */
enum { CATRE_ROWS_BF16 = 0x100 };

/* ---- sizes ---------------------------------------------------------------------------- */

/* Bytes of scratch one refine iteration needs for (B,N,M).  0 on bad arguments. */
size_t catre_workspace_bytes(int B, int N, int M);

/* Floats of the fragment-packed weight image produced by catre_pack_weights. */
size_t catre_packed_floats(int N, int M, int ts_in_dim);

/* Re-lay the weights the MFMA kernels stream (conv / head GEMM operands) into wave-fragment
 * order, transpose the ts-head matrices and pre-reduce conv_p.  Must be re-run whenever the
 * parameters change (e.g. after an optimizer step).  No reference counterpart (layout only). */
int catre_pack_weights(const float* const* params, int N, int M, int ts_in_dim,
                       float* packed, size_t packed_floats, void* stream);

/* Same, restricted to the packs a caller needs (a training step that re-packs after every optimizer step only needs
 * the fp32 encoder image): OR of CATRE_PACK_*. */
enum {
  CATRE_PACK_F32_ENCODER = 1,
  CATRE_PACK_F32_HEADS = 2,  /* the rotation heads' two linears as fp32 fragments */
  CATRE_PACK_BF16 = 4,
  CATRE_PACK_SPLIT = 8,
  CATRE_PACK_F32_TAILS = 16, /* with _F32_HEADS: the ts head's transposed weights and the conv_p weight sums - read by the
                                inference tail kernels only, so a training forward (which re-packs every iteration) leaves
                                these four launches out */
  CATRE_PACK_ALL = 31,       /* every pack of the fp32 / bf16 / split modes */
  CATRE_PACK_F16 = 32        /* the fp16 fragments of the bf16 packs' matrices (CATRE_DTYPE_F16; not part of _ALL) */
};
int catre_pack_weights_sel(const float* const* params, int N, int M, int ts_in_dim, float* packed, size_t packed_floats,
                           int sel, void* stream);

/* ---- single stages (each also usable on its own; tests check them one by one) ---------- */

/* a1: batch_updater_test core (core/catre/engine/batch_test.py:81-97) with
 * transform_normed_pts_batch (lib/pysixd/misc.py:1001-1026).
 * x_out [B,N,3] point-major = pcl - t (or pcl if !zero_center); kps_out [B,M,3] = R (kps*s) (+t). */
int catre_pose_apply(const float* pcl, const float* kps, const float* pose /*[B,3,4]*/,
                     const float* scale /*[B,3]*/, float* x_out, float* kps_out,
                     int B, int N, int M, int zero_center, void* stream);

/* Point arrays are described by a base pointer and element strides (batch, point, coord), so the
 * permuted [B,3,N] views the reference passes (SURVEY.md 8b "forward") are consumed in place. */
typedef struct catre_points {
  const float* obs;  int64_t obs_sb, obs_sn, obs_sc;   /* observed cloud  x        [B,N,3] */
  const float* kps;  int64_t kps_sb, kps_sn, kps_sc;   /* transformed prior tfd_kps [B,M,3] */
  /* apply_pose != 0: obs / kps describe the RAW batch["pcl"] / batch["obj_kps"] and the pose-apply of
   * batch_updater_test (engine/batch_test.py:81-97: x = pcl - t, tfd_kps = R (kps * s) [+ t]) is done on the fly as
   * the points are loaded, with pose [B,3,4] / scale [B,3] - what catre_refine_k does instead of materialising x and
   * tfd_kps every iteration.  0 (and NULL pointers): the arrays already hold x / tfd_kps. */
  const float* pose;  const float* scale;
  int32_t apply_pose, zero_center;
} catre_points;

/* a2: STN3d conv stack + max-pool (core/catre/models/pointnets/pointnet.py:24-29).
 * pooled [2B,1024]. */
int catre_stn3d_pool(const catre_points* pts, const float* const* params, const float* packed,
                     float* pooled, void* workspace, size_t ws_bytes, int B, int N, int M, void* stream);

/* a2/a4 tails: y = act(x W^T + b) (+ I_k flattened), torch.nn.functional.linear as used by
 * pointnet.py:31-40,64-77.  x [R,K] (ldx), W [J,K] (ldw), y [R,J] (ldy). K % 8 == 0. */
int catre_linear(const float* x, int ldx, const float* W, int ldw, const float* bias, float* y, int ldy,
                 int R, int J, int K, int relu, int add_identity_k, void* stream);
/* y[R,J] = x[R,K] W with W [K][J] row-major (ldw): catre_linear on the transposed weight without a transposed copy - the
 * data gradient of a small linear layer (autograd of the FC tails / FC_TransSizeHead, heads/fc_trans_size_head.py:98-116)
 * from the layer's own [out][in] weight.  K % 8 == 0.  xmask (optional, laid out like x): x .* (xmask > 0) replaces x (the
 * ReLU backward of the layer's output folded into the operand load). */
int catre_linear_t(const float* x, int ldx, const float* xmask, const float* W, int ldw, float* y, int ldy, int R, int J,
                   int K, void* stream);

/* a3+a4: x' = x T3, relu(conv1), STNkd conv stack + max-pool (pointnet.py:98-103,57-62).
 * trans3 [2B,3,3] -> pooled [2B,1024]. */
int catre_stnkd_pool(const catre_points* pts, const float* trans3, const float* const* params,
                     const float* packed, float* pooled, void* workspace, size_t ws_bytes,
                     int B, int N, int M, void* stream);

/* a3+a5: point feature transform, conv2..conv4, max-pool (pointnet.py:98-116).
 * trans64 [2B,64,64] (NULL when !feature_transform) -> gfeat [2B,1088] = [max_n conv4 | max_n pointfeat],
 * pointfeat written point-major: obs [B,N,64] then prior [B,M,64] (one buffer of B*(N+M)*64 floats). */
int catre_trunk(const catre_points* pts, const float* trans3, const float* trans64,
                const float* const* params, const float* packed, float* gfeat, float* pointfeat,
                void* workspace, size_t ws_bytes, int B, int N, int M, void* stream);

/* ---- the encoder at PCLNET.INIT_CFG.out_dim = 64, 128, 256, 512 or 1024 (csrc/catre_trunkw.h) --------------------------
 * The reference builds conv4 = Conv1d(512, out_dim) (pointnet.py:93); the entry points above read conv4 as [1024,512]
 * and cannot know another width, so a model with out_dim != 1024 uses the three below for its encoder image and trunk
 * and never hands its parameters to catre_pack_weights[_sel], catre_trunk, catre_refine_* or catre_train_*_fwd.
 * The STNs are 1024 wide at any out_dim (pointnet.py:13-78): catre_stn3d_pool / catre_stnkd_pool read this image as is.
 * Status: CATRE_ERR_BAD_ARG on NULL pointers / non-positive sizes (decided before any HIP call), CATRE_ERR_UNSUPPORTED
 * for an out_dim outside the set, CATRE_ERR_WORKSPACE when `packed` / `workspace` is short. */

/* Floats of the image catre_pack_encoder_w writes; grows with out_dim; 0 for an out_dim outside the set. */
size_t catre_packed_floats_w(int out_dim);

/* The fp32 encoder image: what catre_pack_weights_sel(CATRE_PACK_F32_ENCODER) writes for STN3d, STNkd and conv1..conv3
 * (a NULL source is skipped), and conv4 as out_dim rows of fp32 fragments - exactly out_dim x 512 floats of
 * params[CATRE_P_CONV4_W] are read (pointnet.py:93,114; layout only, no arithmetic).  The head slots of `params` are
 * not read. */
int catre_pack_encoder_w(const float* const* params, int out_dim, float* packed, size_t packed_floats, void* stream);

/* catre_trunk at conv4 width out_dim (pointnet.py:98-116): x T3 -> relu(conv1) -> pointfeat = h1^T T64 (h1 when trans64
 * is NULL) -> relu(conv2) -> relu(conv3) -> conv4 (no ReLU) -> max over the points, dense fp32 with an exact max-pool.
 * gfeat [2B, out_dim + 64] = [max_n conv4 | max_n pointfeat], pointfeat as catre_trunk.  `packed`: catre_pack_encoder_w's
 * image for the same out_dim; `workspace`: catre_workspace_bytes(B,N,M).  Every output equals, bit for bit, what
 * catre_trunk gives for a 1024-row conv4 whose first out_dim rows are these. */
int catre_trunk_w(const catre_points* pts, const float* trans3, const float* trans64, const float* const* params,
                  const float* packed, int out_dim, float* gfeat, float* pointfeat, void* workspace, size_t ws_bytes,
                  int B, int N, int M, void* stream);

/* Tests only - the error bound of the screened max-pool (kernel-form switch 5, csrc/catre_screen.h): one catre_trunk
 * launch on the screened form of the trunk (full grids only, else CATRE_ERR_UNSUPPORTED; `packed` must hold
 * CATRE_PACK_F32_ENCODER) that also writes, for conv4 and every (tile, channel, point), the split-bf16 screen value and
 * the bound eps the device computed for it: screen, eps [tiles][1024][64] (tiles as in the workspace: B*ceil(N/64)
 * observed tiles, then B*ceil(M/64) prior tiles; a ragged tile's points beyond its cloud repeat the last point).
 * |conv4 output before bias - screen| <= eps must hold for every entry.  gfeat / pointfeat as catre_trunk. */
int catre_trunk_screen_probe(const catre_points* pts, const float* trans3, const float* trans64,
                             const float* const* params, const float* packed, float* screen, float* eps, float* gfeat,
                             float* pointfeat, void* workspace, size_t ws_bytes, int B, int N, int M, void* stream);

/* Tests only - the same for conv3 of an STN on the screened full-grid pair kernels (kernel-form switch 6): `which` 0 =
 * STN3d (trans3 unused), 1 = STNkd.  One catre_stn3d_pool / catre_stnkd_pool launch on k_stn3d_pair_s / k_stnkd_pair_s
 * (CATRE_ERR_UNSUPPORTED where the full-grid pair form does not apply) that also writes screen, eps [tiles][1024][64] and
 * rows [tiles][64][128]: the fp32 conv2 image rows the screen read (rows of points beyond a ragged tile repeat the last
 * point; the rows of a second tile that does not exist are not written).  |conv3 output before bias - screen| <= eps
 * must hold for every entry.  pooled as catre_stn3d_pool / catre_stnkd_pool. */
int catre_stn_screen_probe(int which, const catre_points* pts, const float* trans3, const float* const* params,
                           const float* packed, float* screen, float* eps, float* rows, float* pooled, void* workspace,
                           size_t ws_bytes, int B, int N, int M, void* stream);

/* a7+a8: feature gather + FC_TransSizeHead.forward (CATRE_disR_shared.py:69-84,
 * heads/fc_trans_size_head.py:61-70).  -> trans_deltas [B,3], scale_deltas [B,3]. */
int catre_ts_head(const float* gfeat, const float* init_pose, const float* init_scale,
                  const float* const* params, const float* packed, const catre_opts* opts,
                  float* trans_deltas, float* scale_deltas, void* workspace, size_t ws_bytes, int B, void* stream);

/* a7+a9: ConvOutPerRotHead.forward on cat(pcl_feat,kps_feat,dim=2) without materialising it
 * (CATRE_disR_shared.py:86-88, heads/conv_out_per_rot_head.py:62-71,126-140). -> rot6d [B,6]. */
int catre_rot_head(const float* gfeat, const float* pointfeat, const float* const* params,
                   const float* packed, float* rot6d, void* workspace, size_t ws_bytes,
                   int B, int N, int M, void* stream);
/* Same with neck width rot_dim in {1,2,3} per head (RotHead's `rot_dim` constructor argument,
 * conv_out_per_rot_head.py:80,109) -> rot [B, 2*rot_dim]. */
int catre_rot_head_dim(const float* gfeat, const float* pointfeat, const float* const* params,
                       const float* packed, float* rot, void* workspace, size_t ws_bytes,
                       int B, int N, int M, int rot_dim, void* stream);

/* a10 on its own: get_rot_mat (core/catre/models/model_utils.py:28-40): rot [B,d] -> R [B,3,3] for
 * rot_type in CATRE_ROT_* (d = 6 / 4 / 3 / 3): rot6d_to_mat_batch (core/utils/rot_reps.py:34-55), quat2mat_torch
 * (core/utils/pose_utils.py:349-412), quat2mat_torch(qexp(.)) (core/utils/quaternion_lf.py:294-317), lie_vec_to_rot
 * (core/utils/lie_algebra.py:7-77); and its backward grad_R [B,3,3] -> grad_rot [B,d]. */
int catre_rot_to_mat(const float* rot, int rot_type, float* R_out, int B, void* stream);
int catre_rot_to_mat_bwd(const float* rot, int rot_type, const float* grad_R, float* grad_rot, int B, void* stream);

/* a10+a11+a12: rot6d_to_mat_batch (core/utils/rot_reps.py:34-55) and pose_scale_from_delta_init
 * (core/catre/models/pose_scale_from_delta_init.py:8-95).  Ks / mean_scales may be NULL when unused.
 * rot6d is [B,d] in the parametrisation opts->rot_type names (d = 6 / 4 / 3 / 3), or [B,3,3] rotation matrices when
 * opts->rot_input_is_matrix.
 * -> pose_out [B,3,4], scale_out [B,3]. */
int catre_pose_update(const float* rot6d, const float* trans_deltas, const float* scale_deltas,
                      const float* init_pose, const float* init_scale, const float* mean_scales,
                      const float* Ks, const catre_opts* opts, float* pose_out, float* scale_out,
                      int B, void* stream);

/* ---- fused drivers ------------------------------------------------------------------------ */

/* One CATRE_disR_shared.forward (test path, CATRE_disR_shared.py:57-124) on given x / tfd_kps.
 * Batches of up to 8 objects (the evaluator's one-image calls, catre_evaluator.py:292-311) take a latency path of 14-17
 * launches instead of 22 (csrc/catre_small.h); the result of an object does not depend on which path its batch took,
 * bit for bit. */
int catre_refine_iter(const catre_points* pts, const float* init_pose, const float* init_scale,
                      const float* mean_scales, const float* Ks, const float* const* params,
                      const float* packed, const catre_opts* opts, float* pose_out, float* scale_out,
                      void* workspace, size_t ws_bytes, int B, int N, int M, void* stream);

/* The K-loop of catre_inference_on_dataset (core/catre/engine/catre_evaluator.py:292-311):
 * for i in 1..n_iter: pose-apply (batch_test.py:63-99) -> forward -> feed back.
 * poses [n_iter+1,B,3,4] / scales [n_iter+1,B,3]: slot 0 holds the initial estimate on entry,
 * slots 1..n_iter are written.  pcl [B,N,3], kps [B,M,3] point-major contiguous. */
int catre_refine_k(const float* pcl, const float* kps, const float* mean_scales, const float* Ks,
                   const float* const* params, const float* packed, const catre_opts* opts,
                   float* poses, float* scales, void* workspace, size_t ws_bytes,
                   int B, int N, int M, int n_iter, void* stream);

/* The same loop with slot 0 as an OUTPUT: iteration 1 reads the caller's init_pose [B,3,4] / init_scale [B,3]
 * (`out_dict["pose_0"]`, catre_evaluator.py:292) and its pose-update kernel copies them into slot 0 - no copy launch
 * in front of the loop (n_iter == 0: two device-to-device copies). */
int catre_refine_k_from(const float* pcl, const float* kps, const float* init_pose, const float* init_scale,
                        const float* mean_scales, const float* Ks, const float* const* params, const float* packed,
                        const catre_opts* opts, float* poses, float* scales, void* workspace, size_t ws_bytes,
                        int B, int N, int M, int n_iter, void* stream);

/* ---- stand-alone memory-bound kernels (HBM roofline figures of SURVEY.md 8d) --------------- */

/* torch.max(x, 2)[0] for x [B,C,N] contiguous -> out [B,C]  (pointnet.py:28,61,115). */
int catre_colmax(const float* x, float* out, int B, int C, int N, void* stream);

/* ---- opt-in kernel timing: a MEASUREMENT AID for bench.py, fenced off from the data path's contract ---------------
 * Everything above keeps no state between calls and is re-entrant.  The two functions below are the exception and are
 * kept apart for that reason: they hold one process-global record table (mutex-guarded), do nothing unless
 * catre_profile_enable was called, and a product build may drop them altogether (-DCATRE_NO_PROFILING: both return
 * CATRE_ERR_UNSUPPORTED and the launch hooks compile to nothing).  catre_debug_trunk_trace (per-phase cycle stamps) only
 * works in the instrumented library (`make TRACE=1` -> libcatre_hip_trace.so); the product library returns
 * CATRE_ERR_UNSUPPORTED and its kernels carry no stamp code. */
typedef enum catre_kernel_id {
  CATRE_K_STN3D = 0, CATRE_K_STNKD, CATRE_K_TRUNK, CATRE_K_TS_HEAD, CATRE_K_ROT_L0_STATS, CATRE_K_ROT_L1,
  CATRE_K_ROT_OUT, CATRE_K_COLMAX, CATRE_K_COUNT
} catre_kernel_id;

/* Record a HIP event pair around every launch of `kernel_id` on its launch stream (up to max_records).
 * kernel_id < 0 or max_records <= 0 disables and frees the events. */
int catre_profile_enable(int kernel_id, int max_records);
/* Kernel-form switches (A/B measurements, tests): where a stage has more than one kernel form for full grids - all forms
 * give the same bits - `id` selects the switch (0: one-wave-per-SIMD trunk k_trunk4, 1: one-wave STN kernels, 2: STN kernels
 * on pairs of tiles, 3: one-wave rotation-head kernel k_rot_l1w, 4: one-launch FC tails of small batches k_fc_tail,
 * 5: conv4's max-pool of the fp32 one-wave trunk screened with split-bf16 products and replayed in fp32 only where the
 * error bound cannot rule a point out, k_trunk4s - same bits for FINITE activations; where the dense form returns Inf / NaN
 * this one may return another value, 6: the same screen for conv3 of the two STNs on the full-grid pair kernels,
 * k_stn3d_pair_s / k_stnkd_pair_s - it refines 5: the STN kernels are screened only while 5 and 6 are both on, so switch 5
 * off turns every screened form off; the caveat about non-finite activations covers the STN layers too,
 * 7: the screened kernels replay their candidates from ONE list per wave (all 256 channels of the wave, rounds of 64
 * entries) instead of per-channel trips sized by the worst channel of a 32-channel block, k_trunk4sp - same bits as 5; it
 * refines 5 and has no effect while 5 is off; catre_trunk_screen_probe follows it,
 * 8: the pooled trunk as k_trunk4sr - a workgroup walks a RUN of up to S consecutive tiles of one cloud (S:
 * catre_screen_run_len) and carries the exact running maximum, so that a tile replays only the points that can still beat
 * it - same bits; likewise the pooled STN pair kernels as k_stn3d_pair_sr / k_stnkd_pair_sr on runs of S / 2 pairs (their
 * own arm: CATRE_SCREEN_RUN_STN = 0, read once per process, leaves them on one pair); it refines 7 and so 5;
 * catre_trunk_screen_probe follows it, catre_stn_screen_probe keeps the one-pair kernels),
 * 9: the pooled and run kernels screen with ONE row-scaled fp16 product per chunk instead of three bf16 ones (a third of
 * the MFMA issue, half the weight stream, a wider error bound and so more replayed points), k_trunk4sp16 / k_trunk4sr16 -
 * same bits for finite activations, the caveat of 5 holds; tiles or weight rows whose norm is 2^75 or more (activations: a
 * sum of squares past the fp32 range) cannot be scaled into fp16 and replay every point; likewise k_stn3d_pair_sp16 / _sr16
 * and k_stnkd_pair_sp16 / _sr16 (their own arm: CATRE_SCREEN_F16_STN = 0, read once per process, leaves the STN kernels on
 * the split-bf16 screen); it refines 7 and so 5; both probes follow it and return the fp16 screen value and its bound,
 * 13 (`screen_epi`, CATRE_SCREEN_EPI = 0; ids 10 - 12 are the raw bits of the env-only STN arms and stay refused): the fp16-
 * screen kernels of 9 with a leaner epilogue behind the sweep - each accumulator read once, the candidate mask built through
 * the carry, the wave prefix on the DPP path, one scan loop - k_trunk4sr16e / k_trunk4sp16e and the four STN kernels of the
 * same suffix; the same candidates and the same bits.  No form of its own (catre_form_decision does not read it); these
 * kernels carry no probe code, a probe call takes the kernels of 9 (the trunk's: the one-tile kernel), default on,
 * 14 (`screen_da`, CATRE_SCREEN_DA = 0) and 15 (`screen_da_stn`, CATRE_SCREEN_DA_STN = 1; it counts while 14 is on): the
 * error bound the fp16-screen kernels of 9 and 13 select with takes the activations' fp16 rounding as MEASURED per tile
 * (in the pass that takes the row norms) instead of its worst case, and the weights' rounding error split by sign (the
 * screened layers read post-ReLU images) - a runtime flag of the same kernels, no form and no kernel of its own; fewer
 * candidates reach the fp32 replay, the outputs keep their bits; 14 is the trunk's conv4, 15 the two STN kernels' conv3;
 * both probes follow them and return the bound in use,
 * `value` 1 / 0 sets it, value < 0 only queries.  Returns
 * the PREVIOUS setting (1 / 0), -1 for an unknown id.  Process-wide (an atomic word; defaults: 0-2 and 5-9 on, 3 and 4 off -
 * they measured slower - or what the environment says: CATRE_TRUNK4 / CATRE_STN4 / CATRE_STN_PAIR / CATRE_SCREEN /
 * CATRE_SCREEN_STN / CATRE_SCREEN_POOL / CATRE_SCREEN_RUN / CATRE_SCREEN_F16 = 0,
 * CATRE_ROTW / CATRE_FC_TAIL = 1); calls in flight keep the form they were
 * launched with. */
int catre_form_switch(int id, int value);
/* Run length S of form 8 (tiles of one cloud a workgroup of k_trunk4sr walks).  value > 0 forces S = min(value, 16) for
 * every later call (1: the one-tile kernel), 0 returns to the rule (catre_screen_run_rule with the device's CU count),
 * value < 0 only queries.  Returns the previous value (0: the rule).  Process-wide, like the switches.  Any S gives the
 * same bits. */
int catre_screen_run_len(int value);
/* The rule, a pure host function: the largest S in 2 .. 16 whose grid of B (ceil(TN / S) + ceil(TM / S)) workgroups,
 * each up to S tiles long, takes no more tile slots on `cus` compute units (one workgroup per unit) than the one-tile
 * grid - ceil(runs / cus) S <= ceil(tiles / cus) - else 1.  TN, TM: 64-point tiles of a cloud.  -1 for bad arguments. */
int catre_screen_run_rule(int B, int N, int M, int cus);
/* The kernel form one launch of an encoder stage takes - every branch the launches have, in the order they are tried:
 * fp32 / split inference (SPLIT_RS: the split kernels on 1 / 2 / 4 workgroups per tile; RUN_F16 .. SCREEN: the screened
 * max-pool of switches 5 - 9 on the wide kernels; PAIR: the STN kernels on pairs of tiles; WAVE4: one wave per SIMD;
 * RS8: the 8-wave kernels on 1 .. 8 workgroups per tile), the bf16 / fp16-operand kernels on pairs of tiles or on single
 * tiles, and the training forwards (with saves).  UNSUPPORTED: a probe on a grid that takes no screened form. */
typedef enum catre_kernel_form {
  CATRE_FORM_UNSUPPORTED = 0, CATRE_FORM_SPLIT_RS, CATRE_FORM_RUN_F16, CATRE_FORM_RUN, CATRE_FORM_SCREEN_F16,
  CATRE_FORM_SCREEN_POOL, CATRE_FORM_SCREEN, CATRE_FORM_PAIR, CATRE_FORM_WAVE4, CATRE_FORM_RS8, CATRE_FORM_BF_PAIR,
  CATRE_FORM_BF, CATRE_FORM_TRAIN_SPLIT, CATRE_FORM_TRAIN_PAIR, CATRE_FORM_TRAIN_WAVE4, CATRE_FORM_TRAIN_RS1,
  CATRE_FORM_TRAIN_BF_PAIR, CATRE_FORM_TRAIN_BF
} catre_kernel_form;
/* The form decision, a pure host function (the launches call it with the process's switches, the device's CU count,
 * catre_screen_run_len and CATRE_BF_PAIR_MIN).  stage 0 STN3d / 1 STNkd / 2 trunk; mode 0 fp32 / 1 split / 2 bf16 (and fp16
 * operands); save: a training forward, rows: it writes the activation rows; probe: a catre_*_screen_probe call; switches:
 * bit id of catre_form_switch, bits 10 - 12 the STN arms CATRE_SCREEN_POOL_STN / _RUN_STN / _F16_STN - a switch counts as off
 * while one it refines is off; run_len 0 .. 16 (0: catre_screen_run_rule on `cus`).  Writes out[0] the catre_kernel_form,
 * out[1] workgroups per tile, out[2] tiles per run (STN stages: pairs per run; 1 outside the run forms), out[3] the grid
 * in workgroups and returns 0; -1 for arguments no caller can produce. */
int catre_form_decision(int stage, int mode, int save, int rows, int probe, int B, int N, int M, int switches, int cus,
                        int run_len, int bf_pair_min, int* out);
/* Experiment knobs of the instrumented library (id 0: start offset in cycles between the co-resident workgroups of the
 * STN kernels' first dispatch round, id 2: the screened kernels' counters of catre_debug_screen_counts on (1, default) / off
 * (0) - their atomics distort the phase stamps, id 3: the screened epilogues' sub-phase stamps into the buffer of
 * catre_debug_trunk_trace on (1) / off (0, default)); CATRE_ERR_UNSUPPORTED in the product library. */
int catre_debug_knob(int id, int value);
/* Wait for the recorded events, write per-launch durations (ms) and reset the record counter. */
int catre_profile_collect(float* ms_out, int max_out, int* n_out);

/* Debug aid: when non-NULL, every k_trunk workgroup writes 8 waves x 8 shader-clock stamps (u64) at its phase
 * boundaries into `device_buffer` ([tiles][8 waves][8]); NULL disables.  Process-global.  After catre_debug_knob(3, 1)
 * the pooled screened kernels also stamp their epilogue's sub-phases there (layer L at entry L << 22, rows 4 - 7 of a tile:
 * profiles/trace_screen_epi.py); the buffer then holds at least 1 << 24 entries, and every call of this function turns
 * those stamps off again. */
int catre_debug_trunk_trace(void* device_buffer);
/* Instrumented library only (CATRE_ERR_UNSUPPORTED in the product): the screened forms' counters since the last reset,
 * three rows of 64 (trunk conv4, stn.conv3, fstn.conv3) -
 * row[0..31] candidates per (tile, channel) (31: >= 31), [32..47] replay trips per (wave, tile, m-block) (47: >= 15),
 * [48] (wave, tile) units in which an m-block needed more than one round of 4 trips, [49] all units.
 * With switch 7 on: [32..47] rounds of 64 list entries per (wave, tile), [48] units whose list filled up and was replayed
 * in more than one batch, [50] sum of list entries, [51] sum of rounds. */
int catre_debug_screen_counts(unsigned long long* out192, int reset);

/* Identity of the stream capture `stream` is currently recording into (hipStreamGetCaptureInfo; 0 when the stream is not
 * capturing).  The host mirror keys its "this capture already recorded a weight-pack node" shortcut on it
 * (catre_amd/runtime.py; the reference has no counterpart: torch packs nothing). */
int catre_stream_capture_id(void* stream, unsigned long long* id_out);

const char* catre_status_string(int status);

/* ---- training ops (forward with saved activations + backward), chained by torch.autograd ------------------
 * The training path runs the layers unfused on point-major activation matrices [rows, channels] in HBM; each
 * op has a hand-written forward and backward kernel.  Replaced reference arithmetic: torch.nn.functional
 * conv1d(k=1)/linear, relu, max over points, bmm with the STN transforms, group_norm, gelu, the conv_p
 * weighted sum and the autograd of rot6d_to_mat_batch / pose_scale_from_delta_init - i.e. what
 * `losses.backward()` (core/catre/engine/engine.py:349) differentiates through.  Row orders: "cloud-major" =
 * B*N observed rows then B*M prior rows; "object-major" = [N observed | M prior] per object. */
int catre_op_pack(const float* src, int ld, int J, int K, int transpose, float* dst, void* stream);
int catre_op_gemm_rows(const float* X, int ldx, const float* Wp, const float* bias, const float* mask, int ldm,
                       float* Y, int ldy, int R, int J, int K, int relu, void* stream);
/* linear + max-pool over the points of each cloud, fused (no [R,J] intermediate); N, M multiples of 64 */
size_t catre_op_linear_maxpool_ws_bytes(int R, int J);
int catre_op_linear_maxpool(const float* X, int ldx, const float* Wp, const float* bias, float* out, int* idx, int J,
                            int K, int B, int N, int M, void* ws, size_t ws_bytes, void* stream);
/* catre_op_gemm_rows with the left operand masked on load, (X .* (xmask > 0)) Wl^T: the ReLU backward folded in */
int catre_op_gemm_rows_m(const float* X, int ldx, const float* xmask, int ldxm, const float* Wp, const float* bias,
                         const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu, void* stream);
/* mixed precision (torch.autocast around the training forward, core/catre/engine/engine.py:304): the row GEMMs with
 * bf16 operands and fp32 accumulation / outputs.  Wp from catre_op_pack_bf16 (J*K bf16); K in {64,128,256,512}. */
int catre_op_pack_bf16(const float* src, int ld, int J, int K, int transpose, void* dst, void* stream);
int catre_op_gemm_rows_bf16(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                            const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu, void* stream);
int catre_op_linear_maxpool_bf16(const float* X, int ldx, const void* Wp, const float* bias, float* out, int* idx, int J,
                                 int K, int B, int N, int M, void* ws, size_t ws_bytes, void* stream);
/* split mode (hi + lo bf16 operands, three products: fp32-grade results on the bf16 pipe) of the three entry points
 * above; dst / Wp hold 2 * J * K bf16 (hi pack, then lo pack) */
int catre_op_pack_split(const float* src, int ld, int J, int K, int transpose, void* dst, void* stream);
int catre_op_gemm_rows_split(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                             const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu, void* stream);
int catre_op_linear_maxpool_split(const float* X, int ldx, const void* Wp, const float* bias, float* out, int* idx, int J,
                                  int K, int B, int N, int M, void* ws, size_t ws_bytes, void* stream);
/* Y = X Wl^T + bias2d[cloud(row)]: row GEMM with a per-cloud bias (rot-head layer 0: the global-feature half of the
 * 1088 -> 256 conv, conv_out_per_rot_head.py:126-128, is constant per cloud).  Rows object-major (N observed then M prior
 * rows per object), N and M multiples of 64, bias2d [2B][J]; Wp packed for compute_dtype (catre_op_pack / _bf16 / _split). */
int catre_op_gemm_rows_cloudbias(const float* X, int ldx, const void* Wp, const float* bias2d, float* Y, int ldy, int J,
                                 int K, int B, int N, int M, int compute_dtype, void* stream);
/* The rot-head linears (conv_out_per_rot_head.py:126-134) with two optional epilogue extras: per_cloud != 0 - bias is
 * [2B][J], indexed by the row's cloud; gn_part != NULL (J == 256) - the per-64-row-tile GroupNorm(32,256) partials
 * [B*(N+M)/64][32][2] of Y, consumed by catre_op_gnp_gelu_fwd_pre instead of a statistics pass over Y. */
int catre_op_gemm_rows_gn(const float* X, int ldx, const void* Wp, const float* bias, int per_cloud, float* Y, int ldy,
                          int J, int K, int B, int N, int M, float* gn_part, int compute_dtype, void* stream);
int catre_op_gnp_gelu_fwd_pre(const float* Y, const float* part64, const float* gamma, const float* beta, float* A,
                              float* stat, int B, int P, void* stream);
size_t catre_op_gemm_tn_ws_bytes(int J, int K, int R);
int catre_op_gemm_tn(const float* dY, int ldy, const float* X, int ldx, float* dW, int J, int K, int R,
                     int accumulate, void* ws, size_t ws_bytes, void* stream);
/* weight AND bias gradient of y = x W^T + b in one pass over dY: dW = dY^T X, db = column sums of dY (db may be NULL) */
size_t catre_op_gemm_tn_bias_ws_bytes(int J, int K, int R);
int catre_op_gemm_tn_bias(const float* dY, int ldy, const float* X, int ldx, float* dW, float* db, int J, int K, int R,
                          int accumulate, void* ws, size_t ws_bytes, void* stream);
int catre_op_gemm_tn_bias_m(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx, float* dW,
                            float* db, int J, int K, int R, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* ... with the products on the matrix pipe compute_dtype names (CATRE_DTYPE_F32 / _BF16: operands rounded to bf16, the
 * backward of a layer that ran under torch.autocast / _SPLIT: hi + lo bf16 operands, three products); fp32 accumulation
 * and an fp32 bias gradient in every case */
int catre_op_gemm_tn_bias_lp(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx, float* dW,
                             float* db, int J, int K, int R, int accumulate, void* ws, size_t ws_bytes,
                             int compute_dtype, void* stream);
/* whole backward of a 64-channel layer fed by <= 4 live input columns (conv1 on 3-d points; the reference's autograd of
 * pointnet.py:103 `F.relu(self.conv1(x))`) in one pass over the rows: dv = (dY (+ dY2)) .* (ymask > 0); dW[64,4] = dv^T X,
 * db[64] = column sums (db must be dW + 256), dX[R,dxcols] = dv W[64,Kw] (columns >= Kw zero, dxcols 4 or 8).  dY2, ymask
 * and dX optional; ws >= catre_op_gemm_tn_bias_ws_bytes(64, 4, R) */
int catre_op_skinny_bwd(const float* dY, int ldy, const float* dY2, int ldy2, const float* ymask, int ldym, const float* X,
                        int ldx, const float* W, int ldw, int Kw, float* dW, float* db, float* dX, int lddx, int dxcols,
                        int R, void* ws, size_t ws_bytes, void* stream);
/* whole backward of a linear layer on few rows (R < 2048: the reference's autograd of the F.linear / nn.Linear layers whose
 * rows are clouds or objects - pointnet.py:31-33,64-66 fc1-fc3, fc_trans_size_head.py:61-70, the global half of
 * conv_out_per_rot_head.py:126) in ONE launch: dv = dY .* (YM > 0) (YM: the layer's output behind a ReLU, laid out like dY,
 * or NULL); dX[R,Kx] = dv W[J,Kw] (columns >= Kw zero), dW[J,Kw] = dv^T X[R,Kx] (columns >= Kx zero), db[J] = column sums
 * of dv.  dX, dW, db optional (db needs dW) and contiguous; any J, Kx, Kw, leading dimensions.  compute_dtype as
 * catre_op_gemm_tn_bias_lp for dW (dX in fp32).  Deterministic, no workspace. */
int catre_op_fc_bwd(const float* dY, int ldy, const float* YM, const float* X, int ldx, const float* W, int ldw, float* dX,
                    float* dW, float* db, int R, int J, int Kx, int Kw, int compute_dtype, void* stream);
int catre_op_colsum(const float* dY, int ld, int R, int J, float* out, int accumulate, void* ws, size_t ws_bytes,
                    void* stream);
int catre_op_reduce_splits(const float* part, float* out, int n, int splits, int accumulate, void* stream);
int catre_op_rowbias_add(float* Y, int ld, const float* bias, int J, int B, int N, int M, void* stream);
int catre_op_rowbias_bwd(const float* dY, int ld, float* dbias, int J, int B, int N, int M, void* stream);
int catre_op_maxpool_fwd(const float* Y, int ld, float* out, int* idx, int J, int B, int N, int M, void* stream);
int catre_op_maxpool_scatter(const float* dout, const int* idx, float* dY, int ld, int C, int J, void* stream);
int catre_op_maxlin_bwd_w(const float* dg, const int* idx, const float* X, int ldx, float* dW, float* db, int C,
                          int J, int K, void* stream);
int catre_op_maxlin_bwd_x(const float* dg, const int* idx, const float* W, int ldw, float* dX, int ldx, int C, int J,
                          int K, void* stream);
/* the same gradient written row by row (every row of dX[:, :K] exactly once, zeros included: no memset, no
 * read-modify-write); points per cloud <= 4096 */
int catre_op_maxlin_bwd_x_rows(const float* dg, const int* idx, const float* W, int ldw, float* dX, int ldx, int J, int K,
                               int B, int N, int M, void* stream);
int catre_op_cloud_matmul(const float* X, int ldx, const float* T, float* Y, int ldy, int kd, int B, int N, int M,
                          int transpose, void* stream);
/* the 64-row tiles of one cloud a workgroup of the kd = 64 launch above takes (4 or 1): a pure host function, the rule the
 * launch itself calls; -1 for sizes it refuses */
int catre_op_cloud_matmul_tpw(int B, int N, int M);
int catre_op_cloud_matmul_bwd_t(const float* X, int ldx, const float* dY, int ldy, float* dT, int kd, int B, int N,
                                int M, void* stream);
/* out[R,K] = a + b + (c on its first Rc rows): a, b [R,K] contiguous, c [Rc,K] with leading dimension ldc, each optional
 * (NULL = zeros) - the
 * gradient of a tensor whose consumers include a row slice (the pooled feature: CATRE_disR_shared.py:69 feeds `[:B]` of it
 * to the ts head and all of it to both rotation heads), which autograd assembles from a zero-fill, a copy and an add per
 * further consumer */
int catre_op_sum_rows(const float* a, const float* b, const float* c, int ldc, float* out, int R, int Rc, int K,
                      void* stream);
int catre_op_relu_bwd(const float* dY, const float* Y, float* dX, size_t n, void* stream);
int catre_op_gnp_gelu_fwd(const float* Y, const float* gamma, const float* beta, float* A, float* stat, int B, int P,
                          void* stream);
int catre_op_gnp_gelu_bwd(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                          float* dY, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, int B,
                          int P, void* stream);
/* GroupNorm + GELU + neck Conv1d(256 -> rot_dim <= 3) of a RotHead in one op (conv_out_per_rot_head.py:132-137): the [R,256]
 * activation between them is never stored.  Wn [3][256] (rows >= rot_dim zero), bn [3] or NULL, Y3 / dY3 [B*P][3],
 * part64 as catre_op_gnp_gelu_fwd_pre (P % 64 == 0).  Backward: dY [B*P,256], dparams [5][256] = dgamma, dbeta, dWn. */
int catre_op_gnp_gelu_neck_fwd(const float* Y, const float* part64, const float* gamma, const float* beta,
                               const float* Wn, const float* bn, float* Y3, float* stat, int B, int P, void* stream);
size_t catre_op_gnp_gelu_neck_bwd_ws_bytes(int B, int P);
int catre_op_gnp_gelu_neck_bwd(const float* dY3, const float* Y, const float* stat, const float* gamma,
                               const float* beta, const float* Wn, float* dY, float* dparams, int accumulate, void* ws,
                               size_t ws_bytes, int B, int P, void* stream);
/* Backward of a RotHead's first block - Conv1d(1088 -> 256) on cat(point feature, global feature) = a 64 -> 256 linear with
 * a per-cloud bias, GroupNorm(32,256), GELU (conv_out_per_rot_head.py:126-131) - from dA [R,256] in two passes over (dA, Y):
 * the [R,256] gradient of the linear's output stays in LDS.  X [R,64], W [256][64], rows object-major, N, M % 64 == 0.
 * accumulate_dx bit 0: dX += (the two RotHeads share X; the second head's call adds into the first one's result);
 * bit 1: the rows of X are cloud-major (B*N observed rows, then B*M prior rows - pointfeat as the encoder writes it), dX
 * stays object-major. */
size_t catre_op_rot_l0_bwd_ws_bytes(int B, int N, int M);
int catre_op_rot_l0_bwd(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                        const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                        float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                        void* stream);
/* ... with dX = dY W and dW = dY^T X on the bf16 matrix pipe (bf16 operands, fp32 accumulation; everything else fp32): the
 * backward torch.autocast gives the bf16 Conv1d (engine.py:304).  Same arguments, same workspace. */
int catre_op_rot_l0_bwd_lp(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                           const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                           float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                           void* stream);
/* ... and in split mode: hi + lo bf16 operands, three products - fp32-grade dX and dW (k_rot_l0_bwd_sp). */
int catre_op_rot_l0_bwd_sp(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                           const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                           float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                           void* stream);
/* Backward of a RotHead's second block - Conv1d(256 -> 256), GroupNorm, GELU, neck (conv_out_per_rot_head.py:129-137) - from
 * dY3 [R,3]: the sums pass, then one pass over (Y, A) that keeps the linear's output gradient in LDS.  A [R,256] the block's
 * input, W [256][256]; dA [R,256], dWb [256*256 + 256] = dW then db, dparams [5][256] = dgamma, dbeta, dWn.  P % 64 == 0. */
size_t catre_op_rot_l1_bwd_ws_bytes(int B, int P);
int catre_op_rot_l1_bwd(const float* dY3, const float* Y, const float* stat, const float* gamma, const float* beta,
                        const float* Wn, const float* A, const float* W, float* dA, float* dWb, float* dparams, void* ws,
                        size_t ws_bytes, int B, int P, void* stream);
/* The pair used when the neck output feeds conv_p only (out[b][j] = sum_p wp[p] Y3[b,p,j] + b, conv_out_per_rot_head.py:
 * 138-140, so dY3[b,p,:] = wp[p] dout[b,:]): the forward also leaves per-tile moments Spart [B*P/64][3][256]
 * (sum_p wp gelu', sum_p wp gelu' xhat, sum_p wp gelu per channel); the backward takes the GroupNorm-1 sums and dgamma /
 * dbeta / dWn from them and dout [B][3] instead of a reduction pass over Y.  dY3 must be catre_op_wsum_bwd's dY. */
int catre_op_gnp_gelu_neck_fwd_s(const float* Y, const float* part64, const float* gamma, const float* beta,
                                 const float* Wn, const float* bn, const float* wp, float* Y3, float* stat, float* Spart,
                                 int B, int P, void* stream);
int catre_op_rot_l1_bwd_s(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                          const float* gamma, const float* beta, const float* Wn, const float* A, const float* W, float* dA,
                          float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream);
/* catre_op_rot_l1_bwd / _s with the two GEMMs (dA = dY W, dW = dY^T A) on the bf16 matrix pipe: bf16 operands, fp32
 * accumulation - the backward torch.autocast gives a bf16 Conv1d (engine.py:304); GroupNorm / GELU', the bias gradient and all
 * outputs stay fp32.  dout and Spart: both (sums from the forward's moments) or both NULL (sums pass over Y). */
int catre_op_rot_l1_bwd_lp(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                           const float* gamma, const float* beta, const float* Wn, const float* A, const float* W, float* dA,
                           float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream);
/* ... and in split mode: hi + lo bf16 operands, three products per block - fp32-grade dA and dW on the bf16 pipe
 * (k_rot_l1_bwd_sp, 32-row half tiles). */
int catre_op_rot_l1_bwd_sp(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                           const float* gamma, const float* beta, const float* Wn, const float* A, const float* W, float* dA,
                           float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream);
/* The all-bf16-activation form of the autocast rotation heads: the [rows,256] tensors that travel between these kernels -
 * y0, a0, y1, dA - are bf16 rows (256 bf16 per row; `void*`), what torch.autocast's Conv1d outputs are (engine.py:304), so
 * every pass over them moves half the bytes; statistics, GroupNorm / GELU arithmetic, accumulation and every other output
 * stay fp32.  catre_op_gemm_rows_gn_h: catre_op_gemm_rows_gn on bf16 operands (Wp: catre_op_pack_bf16) with io bit 0: X is
 * bf16 rows, bit 1: Y is bf16 rows (ldx / ldy in elements); J = 256, K in {64, 256}; per_cloud == 2 (fp32 X only): per-cloud bias
 * and X rows in CLOUD-major order (pointfeat where the trunk kernel wrote it: no object-major copy), Y object-major.  The others: the op of the same name
 * without _h / with _lp, with the named tensors as bf16 rows (catre_op_rot_l1_bwd_h: Y, A, dA; catre_op_rot_l0_bwd_h: dA, Y). */
int catre_op_gemm_rows_gn_h(const void* X, int ldx, const void* Wp, const float* bias, int per_cloud, void* Y, int ldy, int J,
                            int K, int B, int N, int M, float* gn_part, int io, void* stream);
int catre_op_gnp_gelu_fwd_pre_h(const void* Y, const float* part64, const float* gamma, const float* beta, void* A,
                                float* stat, int B, int P, void* stream);
/* catre_op_gnp_gelu_fwd_pre_h followed by catre_op_gemm_rows_gn_h (K = 256, bf16 rows in and out) as one kernel behind the
 * statistics merge: the GroupNorm + GELU is applied while the GEMM stages its operand tile; A (bf16 rows) is still written
 * for the backward.  Same values as the two calls. */
int catre_op_gn_gelu_gemm_rows_h(const void* Y0, const float* part64, const float* gamma, const float* beta, void* A,
                                 float* stat, const void* Wp, const float* bias, void* Y1, float* gn_part, int B, int N, int M,
                                 void* stream);
int catre_op_gnp_gelu_neck_fwd_s_h(const void* Y, const float* part64, const float* gamma, const float* beta, const float* Wn,
                                   const float* bn, const float* wp, float* Y3, float* stat, float* Spart, int B, int P,
                                   void* stream);
int catre_op_rot_l1_bwd_h(const float* dY3, const float* dout, const float* Spart, const void* Y, const float* stat,
                          const float* gamma, const float* beta, const float* Wn, const void* A, const float* W, void* dA,
                          float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream);
int catre_op_rot_l0_bwd_h(const void* dA, const void* Y, const float* stat, const float* gamma, const float* beta,
                          const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                          float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                          void* stream);
/* ... and the per-head form for the modes whose linear backward is not fused (autocast, split): sums and dparams from dout
 * and Spart, then the apply pass -> dY [B*P,256] (what catre_op_gnp_gelu_neck_bwd returns, without its reduction pass over Y).
 * ws as catre_op_gnp_gelu_neck_bwd_ws_bytes. */
int catre_op_gnp_gelu_neck_bwd_s(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                                 const float* gamma, const float* beta, const float* Wn, float* dY, float* dparams, void* ws,
                                 size_t ws_bytes, int B, int P, void* stream);
/* dst [rows][cols_pad] (contiguous) = src [rows][cols] (element strides: transposed views too) followed by zero columns:
 * the padding of small operands to the GEMM kernels' granularity in one launch (F.pad of the reference-side glue). */
int catre_op_pad_cols(const float* src, long stride_row, long stride_col, int rows, int cols, float* dst, int cols_pad,
                      void* stream);
int catre_op_gnr_gelu_fwd(const float* Y, const float* gamma, const float* beta, float* A, int R, void* stream);
int catre_op_gnr_gelu_bwd(const float* dA, const float* Y, const float* gamma, const float* beta, float* dY,
                          float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, int R, void* stream);
/* Norm + activation stage of a head of any configured width (catre_amd/csrc/catre_heads.h): C channels (a multiple of 8,
 * 8..1024), G GroupNorm groups (a divisor of C), act one of CATRE_ACT_*, norm 1 = GroupNorm(G, C) in front of the
 * activation, 0 = the activation alone (gamma, beta, stat, dgamma, dbeta unused: NULL).  fp32, no atomics: bit-identical
 * from run to run, and an object's rows do not depend on the batch around them.
 *   gnp: rows [B*P, C] object-major, statistics over the P points of an object x the group's channels; forward writes A and
 *        stat [B,G,2] = (mean, rstd) (needs P*C >= 2*G*ceil(P/64)); backward writes dY and dgamma, dbeta [C] (=|+=).
 *   gnr: FC rows [R, C], statistics per (row, group).
 *   neck_wsum: inference tail of a RotHead - the last layer's norm + act, the neck Conv1d(C -> rot_dim <= 3) (Wn
 *        [rot_dim][C], bn [rot_dim] or NULL) and conv_p (wp [P], bp [1] or NULL): out [B][rot_dim] =
 *        sum_p wp[p] y3[b,p,:] + bp.  Neither the [B*P, C] activation nor [B*P, 3] is stored. */
enum { CATRE_ACT_NONE = 0, CATRE_ACT_RELU = 1, CATRE_ACT_LRELU = 2, CATRE_ACT_SILU = 3, CATRE_ACT_GELU = 4,
       CATRE_ACT_MISH = 5 };
int catre_op_gnp_act_fwd(const float* Y, const float* gamma, const float* beta, float* A, float* stat, int B, int P, int C,
                         int G, int act, int norm, void* stream);
size_t catre_op_gnp_act_bwd_ws_bytes(int B, int P, int C, int G);
int catre_op_gnp_act_bwd(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta, float* dY,
                         float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, int B, int P, int C, int G,
                         int act, int norm, void* stream);
int catre_op_gnr_act_fwd(const float* Y, const float* gamma, const float* beta, float* A, int R, int C, int G, int act,
                         int norm, void* stream);
size_t catre_op_gnr_act_bwd_ws_bytes(int R, int C);
int catre_op_gnr_act_bwd(const float* dA, const float* Y, const float* gamma, const float* beta, float* dY, float* dgamma,
                         float* dbeta, int accumulate, void* ws, size_t ws_bytes, int R, int C, int G, int act, int norm,
                         void* stream);
size_t catre_op_gnp_act_neck_wsum_ws_bytes(int B, int P, int G);
int catre_op_gnp_act_neck_wsum(const float* Y, const float* gamma, const float* beta, const float* Wn, const float* bn,
                               const float* wp, const float* bp, float* out, void* ws, size_t ws_bytes, int B, int P, int C,
                               int G, int rot_dim, int act, int norm, void* stream);
int catre_op_wsum_fwd(const float* Y, const float* w, const float* bias, float* out, int B, int P, void* stream);
int catre_op_wsum_bwd(const float* dout, const float* Y, const float* w, float* dY, float* dw, float* dbias,
                      int accumulate, void* ws, size_t ws_bytes, int B, int P, void* stream);
/* ... plus dbn[3] = column sums of dY - the bias gradient of the 256 -> 3 neck whose output gradient dY is
 * (conv_out_per_rot_head.py:131-140: neck, then conv_p) - as (sum_p w[p]) (sum_b dout[b][:]), in the launch that sums dbias */
int catre_op_wsum_bwd_n(const float* dout, const float* Y, const float* w, float* dY, float* dw, float* dbias, float* dbn,
                        int accumulate, void* ws, size_t ws_bytes, int B, int P, void* stream);
int catre_op_pose_update_bwd(const float* d_pose, const float* d_scale, const float* rot6d, const float* trans_deltas,
                             const float* scale_deltas, const float* init_pose, const float* init_scale,
                             const float* mean_scales, const float* Ks, const catre_opts* opts, float* d_rot6d,
                             float* d_dt, float* d_ds, int B, void* stream);

/* Row-sparse backward of linear + max-pool chains (the backward of core/catre/models/pointnets/pointnet.py:24-28, 57-61,
 * 112-116 as torch.autograd runs it, minus the zeros): only the arg-max row of a (cloud, channel) carries gradient, so the
 * gradient in front of a pool - and of every layer further up the conv stack until a dense side input joins - is zero on
 * every row that is nobody's arg-max (~70 % of the rows at N = M = 1024).  catre_op_rows_compact builds the ascending list of
 * live rows, the dense -> compact map and the live-row COUNT on the device (no host sync); catre_op_maxlin_bwd_x_compact
 * writes the pool's data gradient for the live rows only; catre_op_gemm_rows_n / catre_op_gemm_tn_bias_n are the row GEMMs
 * of catre_op_gemm_rows_m / catre_op_gemm_tn_bias_m on the first nrows_dev[0] rows; catre_op_gather_rows /
 * catre_op_scatter_rows move rows between the dense and the compact order.  rows, rowpos: [R] int32; count: [1] int32;
 * scratch: [2 * clouds] int32; clouds of at most 4096 points.  compute_dtype selects the matrix pipe of the two GEMMs
 * (CATRE_DTYPE_F32 / _BF16 / _SPLIT; Wp = the weight pack of that dtype: catre_op_pack / _pack_bf16 / _pack_split). */
int catre_op_rows_compact(const float* dg, const int32_t* idx, int J, int B, int N, int M, int32_t* rows, int32_t* rowpos,
                          int32_t* count, int32_t* scratch, void* stream);
int catre_op_maxlin_bwd_x_compact(const float* dg, const int32_t* idx, const float* W, int ldw, const int32_t* rowpos,
                                  const float* ymask, int ldym, float* dXc, int ldx, int J, int K, int B, int N, int M,
                                  void* stream);
/* catre_op_maxlin_bwd_x_compact / catre_op_maxlin_bwd_w with the saved activation - the ReLU mask / the gathered operand -
 * as bf16 rows (leading dimension in elements): the backward of the pooled layer behind the autocast encoder forward */
int catre_op_maxlin_bwd_x_compact_h(const float* dg, const int32_t* idx, const float* W, int ldw, const int32_t* rowpos,
                                    const void* ymask, int ldym, float* dXc, int ldx, int J, int K, int B, int N, int M,
                                    void* stream);
int catre_op_maxlin_bwd_w_h(const float* dg, const int32_t* idx, const void* X, int ldx, float* dW, float* db, int C, int J,
                            int K, void* stream);
/* Recompute instead of save (the STN stacks' row-sparse backward, fp32): catre_op_stn_recompute rebuilds
 * y1 = relu(conv1 x) [cap,64] and y2 = relu(conv2 y1) [cap,128] for the count[0] live rows as COMPACT rows with the forward
 * kernels' own device code (same bits), so catre_train_stn3d_fwd / _stnkd_fwd may be called without row buffers.
 * kind 0: STN3d (pointnet.py:24-26) - X point rows [R][ldx >= 3], w1 = conv1.weight [64,3], wp1 NULL; kind 1: STNkd
 * (:57-59) - X = relu(conv1) rows [R][64] as the trunk kernel saves them, wp1 = catre_op_pack of fstn.conv1.weight, w1 NULL.
 * wp2 = catre_op_pack of conv2.weight [128,64].  catre_op_maxlin_bwd_w_c / catre_op_maxlin_bwd_x_compact_cm are
 * catre_op_maxlin_bwd_w / catre_op_maxlin_bwd_x_compact reading those compact rows (dense row r at rowpos[r]). */
int catre_op_stn_recompute(int kind, const float* X, int ldx, const int32_t* rows, const int32_t* count, const float* w1,
                           const float* wp1, const float* b1, const float* wp2, const float* b2, float* y1c, float* y2c,
                           int cap, void* stream);
int catre_op_maxlin_bwd_w_c(const float* dg, const int32_t* idx, const int32_t* rowpos, const float* Xc, int ldx, float* dW,
                            float* db, int C, int J, int K, void* stream);
int catre_op_maxlin_bwd_x_compact_cm(const float* dg, const int32_t* idx, const float* W, int ldw, const int32_t* rowpos,
                                     const float* ymask_c, int ldym, float* dXc, int ldx, int J, int K, int B, int N, int M,
                                     void* stream);
int catre_op_gather_rows(const float* src, int lds, const int32_t* rows, const int32_t* count, float* dst, int ldd, int cols,
                         int cap, void* stream);
int catre_op_scatter_rows(const float* srcc, int lds, const int32_t* rowpos, float* dst, int ldd, int cols, int R,
                          void* stream);
/* catre_op_scatter_rows plus objsrc[object-major row of r] (the rows of B objects, [N observed | M prior] each - the order
 * the rotation heads work in, CATRE_disR_shared.py:86) and then dst[idx_max[c][j]][j] += dmax[c][j] (the backward of
 * max over points, :69): the three gradients pointfeat receives summed in two launches.  objsrc / dmax may be NULL. */
int catre_op_scatter_rows_merge(const float* srcc, int lds, const int32_t* rowpos, const float* objsrc, int ldo,
                                const float* dmax, const int32_t* idx_max, int Jm, float* dst, int ldd, int cols, int B, int N,
                                int M, void* stream);
int catre_op_gemm_rows_n(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                         const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu,
                         const int32_t* nrows_dev, int compute_dtype, void* stream);
int catre_op_gemm_tn_bias_n(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx, float* dW,
                            float* db, int J, int K, int R, int accumulate, void* ws, size_t ws_bytes,
                            const int32_t* nrows_dev, int compute_dtype, void* stream);
/* the two above with row indirection against DENSE tensors (no gathered copies of the saved activations in the row-sparse
 * backward): output row r of catre_op_gemm_rows_nr is masked with row mask_rows[r] of `mask`; catre_op_gemm_tn_bias_nr
 * contracts dY row r with row x_rows[r] of X.  Every compute_dtype; a null index array is the identity.
 * compute_dtype = CATRE_DTYPE_BF16 | CATRE_ROWS_BF16: `mask` / `X` are bf16 rows (ldm / ldx in elements) */
int catre_op_gemm_rows_nr(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                          const float* mask, int ldm, const int32_t* mask_rows, float* Y, int ldy, int R, int J, int K,
                          int relu, const int32_t* nrows_dev, int compute_dtype, void* stream);
int catre_op_gemm_tn_bias_nr(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx,
                             const int32_t* x_rows, float* dW, float* db, int J, int K, int R, int accumulate, void* ws,
                             size_t ws_bytes, const int32_t* nrows_dev, int compute_dtype, void* stream);

/* Training forward of the three encoder blocks on the FUSED kernels (the inference kernels with extra stores): the
 * pooled feature g [2B,1024] (bias added, no activation) with its arg-max rows idx [2B,1024], plus the activations the
 * layer-wise backward ops above read, as cloud-major point rows (B*N observed rows, then B*M prior rows):
 *   stn3d: a1 = relu(stn.conv1) [R,64], a2 = relu(stn.conv2) [R,128]            (pointnet.py:24-28)
 *   stnkd: f1 = relu(fstn.conv1) [R,64], f2 = relu(fstn.conv2) [R,128]           (pointnet.py:57-61)
 *   trunk: x1 = x T3 [R,8] (zero-padded), h1 = relu(conv1) [R,64], pf = h1 T64 [R,64], a2 = relu(conv2) [R,128],
 *          a3 = relu(conv3) [R,512]                                               (pointnet.py:98-116)
 * N and M multiples of 64; `workspace` as catre_workspace_bytes.  compute_dtype = CATRE_DTYPE_F32 (fp32 packs,
 * CATRE_PACK_F32_ENCODER, in `packed`) or CATRE_DTYPE_BF16 (what torch.autocast selects, engine.py:304: the bf16-operand
 * kernels, CATRE_PACK_BF16 packs; a1 / a2, f1 / f2 and the trunk's a2 / a3 are then bf16 ROWS - [R,width] bf16, half the
 * bytes, the values the reduced-precision dgrad / wgrad ops round their operands to anyway - which the row-sparse
 * backward reads in place (catre_op_maxlin_bwd_w_h / _x_compact_h, CATRE_ROWS_BF16); x1, h1 and pf stay fp32 rows holding
 * bf16-rounded values; trans64 required) or CATRE_DTYPE_SPLIT (the
 * split-bf16 kernels, CATRE_PACK_SPLIT | CATRE_PACK_F32_ENCODER packs - conv2 of the trunk stays an fp32 MFMA layer; the saved rows
 * hold hi + lo; trans64 required).
 * catre_train_stn3d_fwd / _stnkd_fwd, CATRE_DTYPE_F32 only: a1 = a2 = NULL (f1 = f2 = NULL) stores no activation rows - the
 * backward recomputes them on its live rows (catre_op_stn_recompute) - and full grids then run on the one-wave pair kernels
 * of the inference path with an arg-max epilogue. */
int catre_train_stn3d_fwd(const catre_points* pts, const float* const* params, const float* packed, float* a1, float* a2,
                          float* g, int32_t* idx, void* workspace, size_t ws_bytes, int B, int N, int M, int compute_dtype,
                          void* stream);
int catre_train_stnkd_fwd(const catre_points* pts, const float* trans3, const float* const* params, const float* packed,
                          float* f1, float* f2, float* g, int32_t* idx, void* workspace, size_t ws_bytes, int B, int N,
                          int M, int compute_dtype, void* stream);
int catre_train_trunk_fwd(const catre_points* pts, const float* trans3, const float* trans64, const float* const* params,
                          const float* packed, float* x1, float* h1, float* pf, float* a2, float* a3, float* g,
                          int32_t* idx, void* workspace, size_t ws_bytes, int B, int N, int M, int compute_dtype,
                          void* stream);

/* Training forward of both rotation heads up to the GroupNorm-1 input (heads/conv_out_per_rot_head.py:126-134) on the fused
 * inference kernels with saves: GN0 statistics from second moments of pointfeat, then layer 0 + GN0 + GELU + layer 1 per
 * 64-point tile.  pointfeat: cloud-major [B*N + B*M][64]; bias0 [2 heads][2B clouds][256] = W0[:, :1024] g_cloud + b0;
 * prm / packed: the parameter pointer array and a weight image holding CATRE_PACK_F32_HEADS (compute_dtype CATRE_DTYPE_F32)
 * or CATRE_PACK_SPLIT (CATRE_DTYPE_SPLIT: the two linears as split-bf16 MFMAs, everything stored is fp32).  Outputs, head-major:
 * y0, a0, y1 [2][B*(N+M)][256] (rows object-major), gn1_part [2][B*(N+M)/64][32][2] (what catre_op_gnp_gelu_neck_fwd takes),
 * stat0 [2][B][32][2] (mean, rstd).  N and M multiples of 64.  The per-head backward ops (catre_op_rot_l1_bwd,
 * catre_op_rot_l0_bwd) consume the head slices unchanged. */
size_t catre_train_rot_fwd_ws_bytes(int B);
int catre_train_rot_fwd(const float* pointfeat, const float* bias0, const float* const* params, const float* packed, float* y0,
                        float* a0, float* y1, float* gn1_part, float* stat0, void* workspace, size_t ws_bytes, int B, int N,
                        int M, int compute_dtype, void* stream);

/* f4: one fused multi-tensor Ranger step = RAdam + Lookahead + gradient centralization
 * (lib/torch_utils/solver/ranger.py:102-202) with the train loop's grad nan_to_num folded in
 * (core/catre/engine/engine.py:351-353).  `tensors`: device array of n_tensors 72-byte records
 * {float* p; const float* g; float* exp_avg; float* exp_avg_sq; float* slow; int numel, row_len, row_off;
 *  float lr_step, wd_lr; int adaptive, lookahead, pad;}; `chunks`: device array of {int tensor, offset} pairs
 * (4096 elements each); `row_tensor[total_rows]`: tensor index of every centralized gradient row.
 * beta1 / beta2 are doubles: the reference forms `1 - beta` in Python double precision before torch rounds it to the
 * tensors' fp32 (ranger.py:141-143), so the decay and the (1 - beta) weights are rounded separately here too. */
int catre_op_ranger_step(const void* tensors, int n_tensors, const void* chunks, int n_chunks, const int* row_tensor,
                         int total_rows, float* rowmean_ws, double beta1, double beta2, float eps, float alpha,
                         int clean_grads, float grad_limit, void* stream);

/* f4, the reference's other optimizers (core/utils/solver_utils.py:28-87): one fused multi-tensor step of
 *   CATRE_OPTIM_ADABELIEF        lib/torch_utils/solver/AdaBelief.py:113-218
 *   CATRE_OPTIM_RANGER_ADABELIEF lib/torch_utils/solver/ranger_adabelief.py:133-265
 *   CATRE_OPTIM_MADGRAD          lib/torch_utils/solver/madgrad.py:72-175
 *   CATRE_OPTIM_NADAMW           lib/torch_utils/solver/nadamw.py:58-134
 *   CATRE_OPTIM_ADAMP            lib/torch_utils/solver/adamp.py:48-123
 *   CATRE_OPTIM_SGDP             lib/torch_utils/solver/sgdp.py:50-113
 *   CATRE_OPTIM_SGD_GC           lib/torch_utils/solver/sgd_gc.py:42-180 (SGD_GC and SGD_GCC: the host decides which
 *                                tensors are centralized)
 * with the train loop's grad nan_to_num folded in like catre_op_ranger_step.  `tensors`: device array of n_tensors
 * 112-byte records {float* p; const float* g; float* state[4]; int numel, row_len, row_off, flags; float f[12];} -
 * every hyper-parameter and every scalar term of the step (bias corrections, rectification, `1 - beta`, ...) is formed
 * on the host in double like the reference and passed per tensor in f[] (catre_amd/csrc/catre_optim.h lists the slots
 * and flags of each kind; catre_amd/optimizers.py fills them).  `chunks`: {int tensor, offset} pairs of 4096 elements;
 * `row_tensor[n_rows]`: tensor of every row of the tensors with row_len > 0.  `phases`: bit 0 = run the reductions over
 * the inputs (row means of the gradient / the projection's cosine similarities and its choice of view, made on the
 * device), bit 1 = run the reductions over the update direction; the elementwise update always runs.  ws holds
 * (5 * n_rows + 4 * n_tensors) floats.  Stream-ordered, no atomics, nothing copied back.
 * CATRE_ERR_BAD_ARG on null pointers / bad sizes, CATRE_ERR_UNSUPPORTED on an unknown kind. */
enum catre_optim_kind {
  CATRE_OPTIM_ADABELIEF = 0,
  CATRE_OPTIM_RANGER_ADABELIEF = 1,
  CATRE_OPTIM_MADGRAD = 2,
  CATRE_OPTIM_NADAMW = 3,
  CATRE_OPTIM_ADAMP = 4,
  CATRE_OPTIM_SGDP = 5,
  CATRE_OPTIM_SGD_GC = 6
};
int catre_op_optim_step(int kind, const void* tensors, int n_tensors, const void* chunks, int n_chunks, const int* row_tensor,
                        int n_rows, int phases, float* ws, size_t ws_bytes, int clean_grads, float grad_limit, void* stream);

/* Build identification: "catre_hip gfx950 <version>" */
const char* catre_version(void);

/* ---- train-time batch glue on the device ----------------------------------------------- */

/* aug_3d_bbox followed by aug_RT (core/catre/engine/engine_utils.py:107-172; called from batch_data,
 * core/catre/engine/batching.py:84-88) over all B*N points in one launch:
 *   p' = dR (R (ratios .* R^T (p - t)) + t + dt),  pose' = [dR R | dR (t + dt)],  scale' = scale .* ratios.
 * bbox_ratios = HOST pointer to (ex, ey, ez) or NULL (no bbox aug); objects with sym_flags[b] != 0 use
 * ((ex+ez)/2, ey, (ex+ez)/2) (:126-128).  delta_r[9] / delta_t[3] = HOST pointers (get_rotation_torch output and
 * the translation shift) or both NULL.  pcl, pose, scale, sym_flags and the outputs are device pointers;
 * pcl_out may alias pcl; pose_out / scale_out must NOT alias pose / scale (other threads still read them). */
int catre_aug_points(const float* pcl, const float* pose, const float* scale, const int32_t* sym_flags,
                     const float* bbox_ratios, const float* delta_r, const float* delta_t, float* pcl_out,
                     float* pose_out, float* scale_out, int B, int N, void* stream);

/* aug_poses_normal (core/utils/pose_aug.py:59-101) and aug_scale_normal (:10-35) given the normal noise the caller
 * drew: euler_deg [B,3] ~ N(0, std_rot) (clamped to +-max_rot_deg here unless max_rot_deg < 0), trans_noise [B,3],
 * scale_noise [B,3].  Either half may be skipped with pose == NULL / scale == NULL. */
int catre_init_noise(const float* pose, const float* euler_deg, const float* trans_noise, float max_rot_deg,
                     float min_z, float* pose_out, const float* scale, const float* scale_noise, float min_s,
                     float max_s, float* scale_out, int B, void* stream);

/* ---- point-cloud preparation (the step before the path) -------------------------------- */

/* Candidate pixels of I instances of one depth map, all instances at once - replaces, per instance,
 * backproject_th (lib/pysixd/misc.py:360-378) + sample_bp_depth (core/utils/cat_data_utils.py:209-226) + the
 * radius search of crop_ball_from_pts (:289-304) as called from crop_ball_from_depth_image (:380-400) by the data
 * loader (core/catre/datasets/data_loader.py:576-603):
 *   valid = mask & (depth > 0);  radius = max(ratio * ||R s||, 0.05) grown x1.1 (at most 9 times) until >= 10 valid
 *   points lie within it of the pose centre; no point at all -> every valid pixel (the `distance <= 1e9` fallback).
 * use_ball = 0 keeps every valid pixel (crop_mask_depth_image, :352-377).  depth [H,W] fp32 metres (device),
 * K9 = HOST 3x3 intrinsics row-major, masks [I,H,W] bytes (device) or NULL, poses [I,3,4], scales [I,3] (device).
 * The ordered (row-major, = torch.nonzero order) candidate lists stay in `workspace`
 * (catre_pcl_workspace_bytes); counts_out [I] (device, optional) receives their lengths.
 * Pixels are indexed in int: H * W < 2^30 (the product taken in size_t).  catre_pcl_workspace_bytes returns 0 for
 * I, H or W <= 0 and for a frame at or over that limit; the three entry points below refuse such a frame. */
size_t catre_pcl_workspace_bytes(int I, int H, int W);
int catre_pcl_candidates(const float* depth, const float* K9, const unsigned char* masks, const float* poses,
                         const float* scales, float ratio, int use_ball, int I, int H, int W, void* workspace,
                         size_t ws_bytes, int32_t* counts_out, void* stream);

/* N points per instance out of the candidate lists: the tail of crop_ball_from_pts (:305-320) - the list is tiled
 * by doubling to a length L >= N, slot i takes element sample_idx[inst][i] of it (sample_idx [I,N] int64 on the
 * device = the caller's torch.randperm(L)[:N], which reproduces the reference's random stream), or, with
 * sample_idx == NULL, element perm_seed(i) of a keyed pseudo-random permutation of [0,L) evaluated on the device
 * (no host round trip).  pcl_out [I,N,3]; pix_out [I,N] (optional) = the flat pixel index of every sample, for
 * gathering rgb / NOCS maps.  Instances without any candidate produce zeros and pix -1. */
int catre_pcl_sample(const float* depth, const float* K9, const void* workspace, size_t ws_bytes,
                     const long long* sample_idx, unsigned long long seed, int I, int H, int W, int N, float* pcl_out,
                     int32_t* pix_out, void* stream);
/* INPUT.FPS_SAMPLE (crop_ball_from_pts(..., fps_sample=True), core/utils/cat_data_utils.py:305-306 ->
 * core/utils/farthest_points_torch.py:6-62, init_center=True, pairwise_distance): farthest-point order of each
 * instance's tiled candidate list -> sample_idx_out [I][N] for catre_pcl_sample.  scratch: I * 4 * slot_cap floats
 * with slot_cap >= the largest tiled list (count doubled until >= N). */
int catre_pcl_fps(const float* depth, const float* K9, const void* workspace, size_t ws_bytes, int I, int H, int W, int N,
                  float* scratch, int slot_cap, long long* sample_idx_out, void* stream);

/* ---- row f3 for a data batch: I instances spread over F depth maps, all frames at once ------------------- */

/* The three entry points above with a frame per instance.  depth [F,H,W] fp32 metres (device); K = HOST [F][9]
 * intrinsics, row-major, one per frame; frame_of = HOST [I], the frame of every instance (any order).  The pixels of
 * instance i are either masks[i] != 0 (masks [I,H,W] bytes, device, may be NULL = the whole frame) or
 * labels[frame_of[i]][pix] == label_of[i]: labels [F,H,W] on the device with label_bytes = 1 (uint8) or 4 (int32),
 * one label image per frame, label_of = HOST [I].  Giving both masks and labels is an error.
 * Every entry point checks its host arrays before anything is launched - 0 <= frame_of[i] < F, fx and fy of every
 * frame non-zero, H * W < 2^30, I <= 65535 - and returns CATRE_ERR_BAD_ARG otherwise, so no index it did not check
 * reaches a kernel; it then stages them to the head of `workspace` with one hipMemcpyAsync on `stream` (from pageable
 * memory: the host arrays may be reused when the call returns, the call waits for that copy, and it cannot be captured
 * into a graph).  Per frame the arithmetic is that of the single-frame kernels - the same
 * device functions on the frame's depth map and camera - so a frame gives the bits catre_pcl_* give for it alone.
 * catre_pclf_workspace_bytes: >= catre_pcl_workspace_bytes(I, H, W), growing with I; 0 for F, I, H or W <= 0 and for
 * H * W >= 2^30.  counts_out [I] (device, optional) as above. */
size_t catre_pclf_workspace_bytes(int F, int I, int H, int W);
int catre_pclf_candidates(const float* depth, const float* K, const int32_t* frame_of, const unsigned char* masks,
                          const void* labels, int label_bytes, const int32_t* label_of, const float* poses,
                          const float* scales, float ratio, int use_ball, int F, int I, int H, int W, void* workspace,
                          size_t ws_bytes, int32_t* counts_out, void* stream);

/* catre_pcl_sample for the lists catre_pclf_candidates left in `workspace`.  sample_idx [I,N] (device) as there, or
 * NULL: the keyed permutation, keyed by (seeds[frame_of[i]], rank of instance i within its frame), seeds = HOST [F] -
 * a frame gets the cloud catre_pcl_sample gives it alone under that seed, whatever else is in the batch.  rank_of =
 * HOST [I] or NULL (the rank is then counted in the order given; a caller that splits a batch into several calls
 * passes the ranks of the whole batch).  pix_out [I,N] (optional): pixel index inside the instance's frame.  Instances
 * without any candidate produce zeros and pix -1. */
int catre_pclf_sample(const float* depth, const float* K, const int32_t* frame_of, const int32_t* rank_of,
                      void* workspace, size_t ws_bytes, const long long* sample_idx, const unsigned long long* seeds,
                      int F, int I, int H, int W, int N, float* pcl_out, int32_t* pix_out, void* stream);
/* catre_pcl_fps for the lists catre_pclf_candidates left in `workspace` (scratch, slot_cap: as there). */
int catre_pclf_fps(const float* depth, const float* K, const int32_t* frame_of, void* workspace, size_t ws_bytes, int F,
                   int I, int H, int W, int N, float* scratch, int slot_cap, long long* sample_idx_out, void* stream);

/* INPUT.AUG_DEPTH: the loader's depth augmentation (core/catre/datasets/data_loader.py:530-543,
 * core/utils/depth_aug.py:5-23) of F depth maps in one pass, in the loader's order:
 *   fill   depth == 0 -> a draw from N(0, 0.1) (the median the reference adds is that of a set of zeros); a negative
 *          fill stays and fails the `depth > 0` test of the sampling, as in the reference
 *   drop   depth *= (u > drop_ratio), u ~ U(0,1)
 *   noise  where depth > 0 after both: depth += noise_level * g, g ~ N(0,1)
 * depth_in [F,H,W]: fp32 metres, or uint16 (in_is_u16) converted as (float)v / depth_div with an IEEE division
 * (= depth.astype("float32") / 1000.0 bit for bit); depth_out [F,H,W] fp32, may be depth_in for fp32 input.
 * frames [F] (DEVICE): per frame which steps run (CATRE_DAUG_* flags), drop_ratio, noise_level and a 64-bit key.
 * use_draws != 0: draw_fill / draw_keep / draw_gauss [F,H,W] float64 (device) hold the reference's draws at the pixels
 *   that consume one; a NULL array turns its step off.  The arithmetic is numpy's (float64 where numpy promotes, one
 *   rounding to fp32): bit-identical to the reference given its draws.
 * use_draws == 0: Philox4x32-10 at (seed, frames[f].key, pixel, step), Box-Muller normals, fp32 arithmetic - equally
 *   distributed, a different stream.  A frame's result depends on (seed, key) only: not on F, not on its slot.
 * F <= 65535, H * W < 2^30. */
#define CATRE_DAUG_FILL 1
#define CATRE_DAUG_DROP 2
#define CATRE_DAUG_NOISE 4
typedef struct catre_depth_aug_frame {
  double drop_ratio, noise_level;
  uint64_t key;
  int32_t flags, reserved;
} catre_depth_aug_frame;
int catre_depth_augment(const void* depth_in, int in_is_u16, float depth_div, const catre_depth_aug_frame* frames,
                        int use_draws, const double* draw_fill, const double* draw_keep, const double* draw_gauss,
                        unsigned long long seed, float* depth_out, int F, int H, int W, void* stream);

/* ---- initial poses from a NOCS coordinate map: batched RANSAC Umeyama ------------------------------------- */

/* The similarity (scale s, rotation R, translation t) that takes NOCS coordinates onto camera points, as the reference
 * computes it per instance on the CPU (preprocess/pose_data.py: estimateSimilarityUmeyama :56-87,
 * estimateSimilarityTransform :109-165, fallback of align_nocs_to_depth :38-47) - for I instances at once.
 * src [I,Nmax,3] fp32 (device): NOCS coordinates in [-0.5, 0.5]; dst [I,Nmax,3] fp32 (device): camera points, in the
 * unit t is wanted in; counts [I] int32 (device, NULL = Nmax everywhere): instance i uses its first counts[i] rows, the
 * others are never read (a count outside [0, Nmax] selects nothing).  Arithmetic is fp64; outputs (device): scale [I],
 * R [I,3,3] row-major, t [I,3] float64.  Nothing is copied to the host and nothing waits: all work is ordered on
 * `stream`.  Nmax * 3 < 2^31.
 *
 * catre_umeyama: the plain least-squares fit  C = (1/m) sum (dst - mu_t)(src - mu_s)^T = U diag(D) V^T (D descending;
 * if det(U) det(V) < 0, D[2] and U[:,2] are negated), R = U V^T, s = sum(D) / sum_axes var(src) (population variance),
 * t = mu_t - s R mu_s, over the rows k < counts[i] with mask[i][k] != 0 (mask [I,Nmax] bytes, device, NULL = all).
 * valid_out [I] int32 (optional): 0 - and s = 1, R = I, t = 0 - where no row is kept or the result is not finite. */
int catre_umeyama(const float* src, const float* dst, const int32_t* counts, const unsigned char* mask, int I, int Nmax,
                  double* scale_out, double* R_out, double* t_out, int32_t* valid_out, void* stream);

/* catre_nocs_align: RANSAC around that fit.  With n = counts[i] and InlierT = 2 max_k |src_k - mean(src)| / 10, for
 * it = 0 .. max_iter - 1: five indices in [0, n) with replacement -> (s_h, R_h, t_h) = the fit of those five pairs; the
 * inliers are the k with |dst_k - (s_h R_h src_k + t_h)| < s_h InlierT (strict); the hypothesis replaces the best one if
 * it has strictly more inliers; the loop stops after this iteration if 1 - (1 - best^5)^it > confidence (best = inliers
 * of the best hypothesis / n; zero-based it, so never after iteration 0).  If best < min_inlier_ratio the instance is
 * invalid: s = 1, R = I, t = 0, valid = 0 (what the reference's caller substitutes).  Also invalid - the reference
 * raises or returns NaN there, which is not reproduced - n < 5 and a non-finite value in the first n rows.  Otherwise the
 * result is catre_umeyama over the inliers of the best hypothesis.  The reference's constants: max_iter 128, confidence
 * 0.99, min_inlier_ratio 0.1.
 * draws [I,max_iter,5] int32 (device): the indices, e.g. a replayed np.random.randint(n, size=5) stream - given the
 * reference's draws the discrete outputs are the reference's (wherever no residual sits on its threshold and the
 * 5-point covariances have sigma_2 > 0).  A draw outside [0, n) makes its hypothesis empty.
 * draws == NULL: index j of iteration it = mulhi32(word j, n) of Philox4x32-10 at counter (keys[i] low word, high word,
 * it, word block) under key `seed` (words 0..3 of block 0, word 0 of block 1); keys [I] int64 (device, NULL = 0..I-1).
 * The bias of mulhi32 is at most n / 2^32 per index.  An instance's result depends on its rows, count, seed and key
 * only: not on I, Nmax, its slot in the batch or the launch.
 * Further outputs (device, int32 [I]): valid, n_inliers (of the best hypothesis; 0 if none had any), iters (iterations
 * evaluated; 0 for n < 5 / non-finite input), best_it (-1: none); mask_out [I,Nmax] bytes (optional): the inlier set of
 * the best hypothesis, zeros beyond counts[i] and where there is none.
 * workspace: catre_nocs_align_workspace_bytes(I, Nmax, max_iter) bytes of device memory (0 for sizes <= 0 and
 * max_iter outside 1..128).  Status: CATRE_ERR_BAD_ARG for a NULL array or a non-positive size (before anything is
 * dereferenced), CATRE_ERR_UNSUPPORTED for max_iter outside 1..128, CATRE_ERR_WORKSPACE, CATRE_ERR_LAUNCH.
 * catre_nocs_align_draws writes the indices the draws == NULL route uses to draws_out [I,max_iter,5] (counts required). */
size_t catre_nocs_align_workspace_bytes(int I, int Nmax, int max_iter);
int catre_nocs_align(const float* src, const float* dst, const int32_t* counts, const int32_t* draws,
                     unsigned long long seed, const long long* keys, int I, int Nmax, int max_iter, double confidence,
                     double min_inlier_ratio, void* workspace, size_t ws_bytes, double* scale_out, double* R_out,
                     double* t_out, int32_t* valid_out, int32_t* n_inliers_out, int32_t* iters_out, int32_t* best_it_out,
                     unsigned char* mask_out, void* stream);
int catre_nocs_align_draws(const int32_t* counts, unsigned long long seed, const long long* keys, int I, int max_iter,
                           int32_t* draws_out, void* stream);

/* ---- tracking: nearest-neighbour statistics and the track gate ------------------------------------------- */

/* catre_nn_stats: for I pairs of point sets, the distance from every src point to its nearest dst point.
 * src [I,n_src,3], dst [I,n_dst,3] fp32 (device).  A point x of a set with (pose [I,3,4] row-major [R | t], scale [I,3])
 * stands at R (s * x) + t - the prior branch of catre_pose_apply; a NULL pose is the identity, a NULL scale is 1.
 * paired != 0: the neighbour of src point n is dst point n (n_src == n_dst; ADD of lib/pysixd/pose_error.py:256-271);
 * paired == 0: the dst point at the smallest squared distance, the lowest index on an exact tie (ADD-S, :274-296).
 * Squared distances are fp32 from coordinate differences: dx = px - qx, ..., fmaf(dx,dx, fmaf(dy,dy, dz*dz)).
 * Outputs (device): mean_d [I] = mean over the src points of sqrt(d^2); inlier [I] (optional, needs tau) = the share of
 * src points with d^2 <= tau[i]^2 (tau [I] fp32, device, same unit as the points; tau^2 is one fp32 product; equality is
 * inside); nn_d [I,n_src] (optional) = the SQUARED distances; nn_j [I,n_src] int32 (optional) = the neighbours.
 * The sum over src points is a fixed tree accumulated in double, without atomics: an instance's results depend on its own
 * rows only - the same bits alone and inside any batch.  Non-finite input is not special-cased: a NaN src point or a NaN
 * dst point 0 gives NaN in mean_d, a NaN dst point elsewhere is never a neighbour.
 * ws: catre_nn_stats_workspace_bytes(I, n_src, n_dst) bytes of device memory (0 for a size < 1, n * 3 >= 2^31 or
 * I * ceil(n_src / 256) >= 2^24: the launch has one 256-thread workgroup per instance and 256 src points and stays
 * below 2^32 threads).  Two launches on `stream`, nothing read back.  Status, decided before any launch:
 * CATRE_ERR_BAD_ARG (NULL src / dst / mean_d, inlier without tau, sizes as above), CATRE_ERR_UNSUPPORTED (paired with
 * n_src != n_dst), CATRE_ERR_WORKSPACE (ws NULL or short). */
size_t catre_nn_stats_workspace_bytes(int I, int n_src, int n_dst);
int catre_nn_stats(const float* src, int n_src, const float* dst, int n_dst, const float* src_pose, const float* src_scale,
                   const float* dst_pose, const float* dst_scale, int paired, const float* tau, int I, float* mean_d,
                   float* inlier, float* nn_d, int32_t* nn_j, void* ws, size_t ws_bytes, void* stream);

/* catre_track_gate: which pose a track carries into the next frame.  pose_new / scale_new: the refined estimate,
 * pose_prev / scale_prev: what the frame started from ([I,3,4], [I,3] fp32); counts [I] int32: candidate pixels of the
 * crop; inlier, mean_d [I]: catre_nn_stats of observed points -> posed prior.  status [I] int32 is a bit set:
 *   CATRE_TRACK_EMPTY      counts[i] == 0
 *   CATRE_TRACK_LOW_FIT    inlier[i] < min_inlier (equality passes)
 *   CATRE_TRACK_NONFINITE  a NaN or infinity in pose_new, scale_new, inlier or mean_d
 * status == 0: pose_out / scale_out = the new estimate, age[i] = 0.  Otherwise age[i] += 1 (age [I] int32, in/out) and
 * the outputs are the previous estimate if `hold` != 0 or CATRE_TRACK_NONFINITE is set, else the new one.  The outputs
 * must not overlap the inputs.  One launch, nothing read back.  CATRE_ERR_BAD_ARG: a NULL array, I < 1. */
enum { CATRE_TRACK_EMPTY = 1, CATRE_TRACK_LOW_FIT = 2, CATRE_TRACK_NONFINITE = 4 };
int catre_track_gate(const float* pose_new, const float* scale_new, const float* pose_prev, const float* scale_prev,
                     const int32_t* counts, const float* inlier, const float* mean_d, float min_inlier, int hold, int I,
                     float* pose_out, float* scale_out, int32_t* status, int32_t* age, void* stream);

/* ---- trimmed ICP: move a pose towards the observed points without the network ------------------------------ */

/* Direction: observed point -> nearest posed prior point (the observation is partial and cluttered, the prior complete:
 * the clutter is what gets trimmed).  pcl [I,n_src,3] observed points, kps [I,n_dst,3] prior, pose [I,3,4], scale [I,3]:
 * fp32 on the device, a prior point x standing at R (s * x) + t as in catre_nn_stats.  counts [I] int32 (device, NULL =
 * n_src everywhere): instance i uses its first counts[i] rows of pcl / nn_d2 / nn_j; k_icp_step never reads the others (a
 * count outside [0, n_src] selects nothing).  tau [I] fp32 (device, optional): absolute, in the unit of the points.
 *
 * catre_icp_step: one step from given neighbours.  nn_d2 [I,n_src] fp32, nn_j [I,n_src] int32: exactly what
 * catre_nn_stats writes to nn_d / nn_j for src = pcl, dst = kps, dst_pose = pose, dst_scale = scale.
 *   candidates: rows k < counts[i] with 0 <= d2_k <= tau[i]^2 (one fp32 product, equality inside; tau NULL: every finite
 *     d2_k) and 0 <= nn_j[k] < n_dst.  A NaN or infinite d2 is never a candidate, nor is any row under a NaN tau.  c = their
 *     number.
 *   kept set: the m = ceil((double)trim * c) candidates smallest under the total order (d2, then k): exact ties at the
 *     boundary go to the lower indices.  trim in (0, 1].
 *   fit, in fp64: source = prior point nn_j[k] at (pose, scale), target = pcl[k], over the kept rows; the least-squares
 *     similarity of catre_umeyama (sigma, dR, dt); with_scale == 0: sigma = 1, dt = mu_T - dR mu_S.
 *   update: R' = dR R, t' = sigma dR t + dt, s' = sigma s, each rounded once to fp32 -> pose_out [I,3,4], scale_out [I,3]
 *     (pose_out / scale_out may be pose / scale themselves).
 *   rmse [I] fp32 = sqrt(sum over kept of (double)d2 / m), summed in a fixed order (NaN when m == 0); kept [I] int32 = m;
 *   mask [I,n_src] bytes (optional): 1 on the kept rows, 0 elsewhere (rows >= counts[i] included).
 *   status [I] int32, in and out: the bits below are OR-ed into what it holds, so they are sticky over a sequence of steps.
 *     CATRE_ICP_FEW         m < 3
 *     CATRE_ICP_DEGENERATE  second singular value of the kept covariance <= 1e-12 * the first: no unique rotation
 *     CATRE_ICP_NONFINITE   a NaN or infinity in the incoming pose or scale, or in the fit
 *   With any bit set, now or earlier, pose_out / scale_out are pose / scale bit for bit; rmse and kept are still reported.
 *   update == 0: rmse, kept and mask only; pose_out, scale_out and status are not touched (and may be NULL).
 * One 256-thread workgroup per instance, one launch, nothing read back; an instance's outputs depend on its own rows only.
 *
 * catre_icp: for it = 0 .. n_iter: the two launches of catre_nn_stats at the current pose, then the step with
 * update = (it < n_iter).  rmse, kept: [n_iter + 1, I]; row it is measured BEFORE update it, the last row is the fit of
 * the returned pose.  status [I]: in and out as above (zero it for a fresh run).  tau stays fixed over the iterations.
 * Bit-identical to the same sequence issued as catre_nn_stats (with nn_d, nn_j) and catre_icp_step calls.  No host
 * synchronisation; 3 (n_iter + 1) launches (n_iter == 0: and two device-to-device copies of pose and scale).
 * pose_out / scale_out must not overlap pose / scale.  ws: catre_icp_workspace_bytes(I, n_src, n_dst, n_iter) bytes of
 * device memory (0 for sizes catre_nn_stats refuses and n_iter outside 0 .. CATRE_ICP_MAX_ITER).
 * Status, decided before any launch: CATRE_ERR_BAD_ARG (a NULL required array, sizes as catre_nn_stats, trim outside
 * (0, 1] or NaN, n_iter outside 0 .. CATRE_ICP_MAX_ITER), CATRE_ERR_WORKSPACE (ws NULL or short). */
enum { CATRE_ICP_FEW = 1, CATRE_ICP_DEGENERATE = 2, CATRE_ICP_NONFINITE = 4 };
#define CATRE_ICP_MAX_ITER 256
size_t catre_icp_workspace_bytes(int I, int n_src, int n_dst, int n_iter);
int catre_icp_step(const float* pcl, int n_src, const int32_t* counts, const float* kps, int n_dst, const float* pose,
                   const float* scale, const float* nn_d2, const int32_t* nn_j, const float* tau, float trim, int with_scale,
                   int update, int I, float* pose_out, float* scale_out, float* rmse, int32_t* kept, unsigned char* mask,
                   int32_t* status, void* stream);
int catre_icp(const float* pcl, int n_src, const int32_t* counts, const float* kps, int n_dst, const float* pose,
              const float* scale, const float* tau, float trim, int with_scale, int n_iter, int I, float* pose_out,
              float* scale_out, float* rmse, int32_t* kept, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- splat render of the posed prior: instance masks, a depth image and visibility ----------------------- */

/* catre_splat_render: a z-buffered disc splat of I posed point priors into the F frames they are seen in.
 * kps [I,M,3], pose [I,3,4], scale [I,3], rho [I] (metres: the disc radius of every splat of instance i), depth
 * [F,H,W] (metres, may be NULL): fp32 on the device.  K = HOST [F][9], frame_of = HOST [I], as catre_pclf_candidates
 * takes them, checked and staged the same way (one hipMemcpyAsync of F * 4 + I ints from pageable memory; nothing is
 * ever copied back and nothing waits on the device's work; like that entry point the call cannot be captured into a
 * graph, because of this copy).
 * A point is p = R (s * x) + t (catre_nn_stats' arithmetic).  With the frame's fx, fy, cx, cy and an integer pixel being
 * its own centre: u0 = fx * p.x / p.z + cx, v0 = fy * p.y / p.z + cy, r = min(fx * rho[i] / p.z, r_max) (r_max: pixels),
 * each operation rounded to fp32 in that order.  A point with !(p.z > 0) or a non-finite u0, v0 or r draws nothing.  Its
 * footprint is every pixel 0 <= u < W, 0 <= v < H with fmaf(du, du, dv * dv) <= r * r, du = u - u0, dv = v - v0
 * (equality is inside; empty for a small r between pixel centres).  Every covered pixel keeps the minimum of the key
 * (bits(p.z) << 32) | (i << 16) | m: the nearest depth, then the lower instance, then the lower point.  Integer min does
 * not depend on the order of arrival: the outputs are bit-reproducible, and a frame's outputs do not depend on the other
 * frames of the call.
 * Outputs (device; labels, zbuf and counts are required, the others may be NULL):
 *   labels [F,H,W] int32      i + 1, 0 = background
 *   zbuf [F,H,W] fp32         the winner's p.z, 0 = background
 *   point [F,H,W] int32       the winner's m, -1 = background
 *   cls [F,H,W] uint8         CATRE_SPLAT_*: with an observed depth d and diff = zbuf - d (one fp32 subtraction)
 *                               HOLE if !(d > 0), OCCLUDED if diff > delta, FREE if diff < -delta, else AGREE;
 *                             depth == NULL: every rendered pixel is AGREE.  lib/pysixd/visibility.py:9-41 with the visible
 *                             set split: its bop18 mask is AGREE | FREE, its bop19 mask AGREE | FREE | HOLE
 *   labels_fit [F,H,W] int32  labels where cls == AGREE, else 0
 *   counts [I,5] int32        pixels instance i won, then how many of them are AGREE, OCCLUDED, FREE, HOLE (column = class)
 *   vis [I,M] uint8           1 iff the point was drawn, its centre pixel (rintf(u0), rintf(v0)) is inside the image,
 *                             labels there is i + 1, p.z - zbuf <= delta there and the pixel is not OCCLUDED
 * workspace: catre_splat_workspace_bytes(F, H, W) bytes of device memory (0 for a size < 1 or F * H * W >= 2^30).
 * Launches on `stream`: clear, splat, resolve, and visible if vis != NULL - the same for any I and F.
 * Status, decided before any launch: CATRE_ERR_BAD_ARG (a NULL required array, a size < 1, F * H * W >= 2^30, r_max
 * negative or NaN, delta NaN, frame_of[i] outside [0, F), fx or fy zero or NaN), CATRE_ERR_UNSUPPORTED (I > 65535 or
 * M > 65536: the key holds 16 bits of each), CATRE_ERR_WORKSPACE (workspace NULL or short). */
enum {
  CATRE_SPLAT_BACKGROUND = 0,
  CATRE_SPLAT_AGREE = 1,
  CATRE_SPLAT_OCCLUDED = 2,
  CATRE_SPLAT_FREE = 3,
  CATRE_SPLAT_HOLE = 4
};
size_t catre_splat_workspace_bytes(int F, int H, int W);
int catre_splat_render(const float* kps, const float* pose, const float* scale, const float* rho, const float* depth,
                       const float* K, const int32_t* frame_of, float r_max, float delta, int F, int I, int M, int H, int W,
                       void* workspace, size_t ws_bytes, int32_t* labels, float* zbuf, int32_t* point, unsigned char* cls,
                       int32_t* labels_fit, int32_t* counts, unsigned char* vis, void* stream);

/* ---- rasteriser of posed triangle meshes: depth, labels, model coordinates ------------------------------ */

/* catre_mesh_render: the meshes of I instances, posed and projected into the F frames they are seen in, z-buffered per pixel.
 * The meshes form a ragged table on the device: verts [V_tot,3] fp32, faces [T_tot,3] int32 (indices LOCAL to the mesh),
 * vert_off, face_off [G+1] int32 (mesh g is rows off[g] .. off[g+1] - 1), mesh_of [I] int32 (the mesh of instance i), and the
 * instance-major offsets of what is posed: inst_vert_off, inst_face_off [I+1] int32 (running sums of the vertex / face counts
 * of mesh_of[i]; their last entries are n_posed_vertices and n_posed_faces, both < 2^31).  pose [I,3,4], scale [I,3], depth
 * [F,H,W] (metres, may be NULL): fp32 on the device.  K = HOST [F][9], frame_of = HOST [I], checked and staged as
 * catre_splat_render does (one hipMemcpyAsync from pageable memory; nothing is copied back, nothing waits on the device;
 * the call cannot be captured into a graph because of this copy).  pixel_center_half: 0 = an integer pixel is its own
 * centre (the convention of catre_splat_render and the point-cloud prep), 1 = pixel (px, py) is sampled at (px + 0.5,
 * py + 0.5), where the GL renderers of lib/pysixd sample.
 * Vertices: p = R (s * x) + t (catre_nn_stats' arithmetic); u = fx * p.x / p.z + cx, v = fy * p.y / p.z + cy, each operation
 * rounded to fp32 in that order; xi = (int)rintf(u * 256), yi likewise (8 fractional bits).  A vertex is ok iff p.z > 0, u
 * and v are finite and |xi|, |yi| < 2^23.  Everything below is a function of the records (xi, yi, p.z, ok) alone.
 * Faces: a face with a vertex that is not ok, or with an index outside [0, V_mesh), is culled whole and counted once in
 * culled[i] - there is no clipping, a face that reaches the camera plane draws nothing - and never indexes out of bounds; a
 * face of zero doubled area is dropped without being counted.  Either winding draws: the face is oriented so that its
 * doubled area is positive.  Coverage by int64 edge functions of the snapped corners at the sample (256 px + c, 256 py + c),
 * c = 0 or 128: strictly inside is covered; a sample exactly on an edge is covered iff the edge is top (horizontal, interior
 * at larger v) or left (not horizontal, interior at larger u), so a sample on an edge or vertex shared by the faces of a
 * consistently tessellated surface belongs to exactly one of them.  Depth, perspective-correct, in fp64, every operation
 * rounded: w_k = (double)E_k * (1.0 / (double)z_k), W = (w_0 + w_1) + w_2, z = (float)((double)area2 / W), E_k the edge function
 * opposite corner k.  Every covered pixel keeps the minimum of the key (bits(z) << 32) | g, g = inst_face_off[i] + the face's
 * local index: the nearest depth, then the lower instance, then the lower face.  Integer min does not depend on the order
 * of arrival: the outputs are bit-reproducible, and a frame's outputs do not depend on the other frames of the call.
 * Outputs (device; labels, zbuf, counts and culled are required, the others may be NULL):
 *   labels [F,H,W] int32      i + 1, 0 = background
 *   zbuf [F,H,W] fp32         the winner's z, 0 = background
 *   face [F,H,W] int32        the winner's local face index, -1 = background
 *   cls, labels_fit, counts   as catre_splat_render writes them (CATRE_SPLAT_*, the same constants; counts [I,5])
 *   culled [I] int32          faces of instance i that were culled
 *   coord [F,H,W,3] fp32      the model-space point under the pixel, per component (float)(((w_0 a_0 + w_1 a_1) + w_2 a_2) / W)
 *                             in fp64 with a_k the UNPOSED, UNSCALED vertex coordinate; 0 on background
 *   projected [NV,4] int32    the vertex records (xi, yi, bits(p.z), ok), instance-major
 * workspace: catre_mesh_workspace_bytes(F, H, W, n_posed_vertices) bytes of device memory (0 for a size < 1 or
 * F * H * W >= 2^30).  Four launches on `stream` - clear, project, raster, resolve - the same for any I, F and mesh.
 * Status, decided before any launch: CATRE_ERR_BAD_ARG (a NULL required array, a size < 1, F * H * W >= 2^30, fewer posed
 * vertices or faces than instances, delta NaN, pixel_center_half not 0 or 1, frame_of[i] outside [0, F), fx or fy zero or
 * NaN), CATRE_ERR_UNSUPPORTED (I > 2^27), CATRE_ERR_WORKSPACE (workspace NULL or short). */
size_t catre_mesh_workspace_bytes(int F, int H, int W, int n_posed_vertices);
int catre_mesh_render(const float* verts, const int32_t* faces, const int32_t* vert_off, const int32_t* face_off,
                      const int32_t* mesh_of, const int32_t* inst_vert_off, const int32_t* inst_face_off, const float* pose,
                      const float* scale, const float* depth, const float* K, const int32_t* frame_of, float delta,
                      int pixel_center_half, int G, int V_tot, int T_tot, int F, int I, int n_posed_vertices, int n_posed_faces,
                      int H, int W, void* workspace, size_t ws_bytes, int32_t* labels, float* zbuf, int32_t* face,
                      unsigned char* cls, int32_t* labels_fit, int32_t* counts, int32_t* culled, float* coord,
                      int32_t* projected, void* stream);

/* ---- BOP pose errors: MSSD, MSPD, proj_sym and VSD -------------------------------------------------------- */

/* catre_sym_err: lib/pysixd/pose_error.py mssd (:131-153), mspd (:156-179) and proj_sym (:196-217) of I instances in one
 * sweep.  pts [I,n,3] (pts_shared != 0: [n,3], the same model for all), pose_est, pose_gt [I,3,4] row-major [R | t],
 * scale_est, scale_gt [I,3] (may be NULL: ones), K [I,3,3]: fp32 on the device.  The symmetry sets form a ragged table on
 * the device: syms [S_tot,3,4] fp32 ([R_s | t_s]), sym_off [G+1] int32 (set g is rows sym_off[g] .. sym_off[g+1] - 1),
 * sym_of [I] int32 (the set of instance i).  S_max >= the largest set any instance reads (the width of the tables).
 * For symmetry s of instance i's set and model point p:
 *   x_est = R_est (s_est * p) + t_est,  x_gt = R_gt (s_gt * (R_s p + t_s)) + t_gt  (without scales the reference's
 *   R_gt R_s, R_gt t_s + t_gt),  pi(x) = (fx x / z + cx, fy y / z + cy) with K[i]
 *   e3[i,s] = max_n |x_est - x_gt|,  e2[i,s] = max_n |pi(x_est) - pi(x_gt)|,  p2[i,s] = mean_n of the same pixel distance
 * Arithmetic: the 3x4 composites are formed in double and rounded once per entry to fp32; a posed point is three fmas per
 * coordinate starting at the translation; a projection is product, quotient, sum, each rounded; distances come from
 * coordinate differences (fma(dx, dx, fma(dy, dy, dz dz)), fma(du, du, dv dv)), the maxima are taken over the squares and
 * rooted once, the mean adds the fp32 roots in a fixed tree in double and is rounded to fp32 once.  An instance's results
 * depend on its own rows only - the same bits alone and inside any batch.  Points behind the camera are not special.
 * Outputs (device): err [3,I] fp32 = min_s of e3 (MSSD), e2 (MSPD), p2 (proj_sym); best [3,I] int32 = the index of the
 * winning symmetry within the set, the lowest on an exact tie; tables [3,I,S_max] fp32 (may be NULL) = e3, e2, p2, +inf
 * behind the end of a set.  A NaN in a pose, scale or point of an instance makes its three errors NaN (the reference's
 * python min() over a list with NaNs depends on their order and is not reproduced).  An instance whose sym_of / sym_off
 * entries lie outside the table gets NaN and index -1; nothing is read out of bounds.
 * workspace: catre_sym_err_workspace_bytes(I, S_max) bytes of device memory (0 for a size < 1 or beyond what is indexed);
 * not needed when `tables` is given.  Two launches on `stream`, nothing read back.  Status, decided before any launch:
 * CATRE_ERR_BAD_ARG (a NULL required array, a size < 1, S_max > S_tot, n * 3 >= 2^31), CATRE_ERR_WORKSPACE. */
size_t catre_sym_err_workspace_bytes(int I, int S_max);
int catre_sym_err(const float* pts, int pts_shared, int n, const float* pose_est, const float* pose_gt, const float* scale_est,
                  const float* scale_gt, const float* K, const float* syms, const int32_t* sym_off, const int32_t* sym_of,
                  int G, int S_tot, int S_max, int I, void* workspace, size_t ws_bytes, float* err, int32_t* best,
                  float* tables, void* stream);

/* catre_vsd: lib/pysixd/pose_error.py vsd (:22-128, cost_type "step") after its two renders.  depth_est, depth_gt [I,h,w]
 * (0: nothing rendered), depth_test [F,H,W], K [I,3,3] (of the full image): fp32 on the device; frame_of [I] int32 (device,
 * NULL: frame 0), origin [I,2] int32 (device, (u0, v0); NULL: zeros): window pixel (col, row) of instance i is pixel
 * (u0 + col, v0 + row) of frame frame_of[i]; window pixels outside the frame - and every pixel of an instance whose frame
 * is outside [0, F) - are ignored.  diameter [I] fp64 (device, may be NULL: normalized_by_diameter off); taus = HOST [T]
 * fp64, T <= CATRE_VSD_MAX_TAUS; delta: the visibility tolerance; visib_mode CATRE_VSD_BOP19 / _BOP18.
 * Per pixel, in the reference's precisions: the distances sqrt(((x - cx) / fx d)^2 + ((y - cy) / fy d)^2 + d^2) in double,
 * every operation rounded, added in that order (misc.py:628-647); the visibility masks (visibility.py:9-74) from
 * fl32(dist_model) - fl32(dist_test) <= delta in fp32, dist_test == 0 and dist_model > 0 in double (the splat render's
 * HOLE is !(d > 0): the two differ for a negative or NaN observed depth only); the cost |dist_gt - dist_est| / diameter
 * >= tau in double on the intersection.
 * Outputs (device): counts [I,2+T] int32 = pixels of the union, of the intersection, and of cost 1 per tau; errors [I,T]
 * fp64 = (cost + union - inter) / union, 1.0 for an empty union.  Integer sums: bit-reproducible.
 * A memset and two launches on `stream`, nothing read back.  Status, decided before any launch: CATRE_ERR_BAD_ARG (a NULL
 * required array, a size < 1, h * w or H * W >= 2^30, a NaN delta or tau, an unknown visib_mode), CATRE_ERR_UNSUPPORTED
 * (T > CATRE_VSD_MAX_TAUS). */
enum { CATRE_VSD_BOP19 = 0, CATRE_VSD_BOP18 = 1, CATRE_VSD_MAX_TAUS = 16 };
int catre_vsd(const float* depth_est, const float* depth_gt, const float* depth_test, const float* K, const int32_t* frame_of,
              const int32_t* origin, const double* diameter, const double* taus, float delta, int visib_mode, int I, int h,
              int w, int F, int H, int W, int T, int32_t* counts, double* errors, void* stream);

/* ---- the training loss on the device --------------------------------------------------- */

/* Flags of cfg.MODEL.CATRE.LOSS_CFG that CATRE_disR_shared.catre_loss reads
 * (core/catre/models/CATRE_disR_shared.py:168-288; PyPMLoss core/catre/losses/pm_loss.py:85-194, L1 / R-only form -
 * catre_loss_cfg2 below selects the other forms). */
typedef struct catre_loss_cfg {
  int32_t pm_on, pm_sym, pm_with_scale;     /* PM_LW > 0, PM_LOSS_SYM, PM_WITH_SCALE                              */
  int32_t rot_on, rot_l2, yaxis_smooth;     /* ROT_LW > 0, ROT_LOSS_TYPE == "L2" (else angular), ROT_YAXIS_LOSS_TYPE: 0 "L1",
                                             * 1 "smoothL1", 2 "L2", 3 "angular" (CATRE_disR_shared.py:232-243)           */
  int32_t trans_on, trans_mse, trans_split; /* TRANS_LW > 0, TRANS_LOSS_TYPE: 0 "L1", 1 "MSE", 2 "L2" (L2Loss,
                                             * core/catre/losses/l2_loss.py:5-28), TRANS_LOSS_DISENTANGLE                 */
  int32_t scale_on, scale_mse;              /* SCALE_LW > 0, SCALE_LOSS_TYPE: 0 "L1", 1 "MSE", 2 "L2"                      */
  float pm_lw, rot_lw, trans_lw, scale_lw;
} catre_loss_cfg;

/* losses[20]: [0..6) = {loss_PM_R, loss_rot, loss_yaxis_rot, loss_trans_xy (or loss_trans_LPnP), loss_trans_z,
 * loss_scale}; [6..20) = the scalars CATRE_disR_shared.forward logs per training iteration
 * (core/catre/models/CATRE_disR_shared.py:127-164, compute_mean_re_te models/model_utils.py:226-238), in its order:
 * error_R [deg], error_t [cm], |t_pred - t_gt| x,y,z of object 0 [cm], t_pred x,y,z, trans_deltas x,y,z
 * (trans_deltas [B,3] may be NULL -> 0), t_gt x,y,z - computed with the loss, so logging costs no launch and one copy.
 * pose [B,3,4] = [R|t] estimate, scale [B,3]; cands [B,S1,3,3] = symmetry rotations per object with the identity
 * first, valid [B,S1] bytes, is_sym [B]; the ground-truth rotation closest to the estimate among R_gt S_k
 * (get_closest_rot_batch, core/utils/pose_utils.py:472-528) is chosen on the device, its index kept in best [B] for
 * the backward, and counts [2] = {objects with, without symmetry info} (counted on the device, so nothing about the
 * batch composition is baked into a captured graph).  part_ws: B*8 floats of scratch.  All pointers are device pointers. */
int catre_loss_fwd(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                   const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                   const int32_t* is_sym, const catre_loss_cfg* cfg, int32_t* best, int32_t* counts, float* part_ws,
                   float* losses, const float* trans_deltas, int B, int M, int S1, void* stream);
/* dpose [B,3,4], dscale [B,3] = gradient of sum_i upstream[i] * losses[i] (upstream: 6 floats on the device) */
int catre_loss_bwd(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                   const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                   const int32_t* best, const int32_t* counts, const float* upstream, const catre_loss_cfg* cfg,
                   float* dpose, float* dscale, int B, int M, int S1, void* stream);
/* The reference's train loop adds the loss dict up with python's sum() (core/catre/engine/engine.py:318
 * `losses = sum(loss_dict.values())`): one add kernel per term, and autograd's per-term bookkeeping on the way back.
 * catre_loss_fwd_sums also writes prefix[k] = ((0 + losses[terms[0]]) + losses[terms[1]]) + ... + losses[terms[k]] for
 * k < n_terms <= 6 (terms: HOST array of loss indices in the dict's order) - every intermediate that sum() builds, same
 * operations, same bits - and catre_loss_bwd_sums takes the upstream gradients of those prefix sums (up_prefix: HOST array
 * of n_terms device pointers to one float each, NULL entries = zero) next to the six per-loss ones (upstream [6], device);
 * either argument may be NULL (= zeros).  catre_amd/losses.py hands the dict's
 * values out as tensors that answer `a + b` along that chain with the precomputed prefix. */
int catre_loss_fwd_sums(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                        const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                        const int32_t* is_sym, const catre_loss_cfg* cfg, int32_t* best, int32_t* counts, float* part_ws,
                        float* losses, const float* trans_deltas, const int32_t* terms, int n_terms, float* prefix, int B,
                        int M, int S1, void* stream);
int catre_loss_bwd_sums(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                        const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                        const int32_t* best, const int32_t* counts, const float* upstream,
                        const float* const* up_prefix, const int32_t* terms, int n_terms, const catre_loss_cfg* cfg,
                        float* dpose, float* dscale, int B, int M, int S1, void* stream);

/* ---- every form of the point-matching loss (PyPMLoss, core/catre/losses/pm_loss.py:21-194) -------------------------
 * The four entry points above keep their layout, meaning and result bits (L1 / R-only point-matching term).  The *2
 * entry points below run the same three kernels for every form CATRE_disR_shared.catre_loss can select
 * (core/catre/models/CATRE_disR_shared.py:185-210). */

/* Structural mode, as PyPMLoss.__init__ resolves its switches (pm_loss.py:56-68: disentangle_z forces disentangle_t;
 * without any disentangling t_loss_use_points is forced on), and the dict keys of each (pm_loss.py:126-192). */
enum {
  CATRE_PM_R_ONLY = 0,        /* PM_R_ONLY (pm_loss.py:126-128):                                  loss_PM_R                */
  CATRE_PM_RT = 1,            /* none of the switches (:187-191):                                 loss_PM_RT               */
  CATRE_PM_R_T_POINTS = 2,    /* PM_DISENTANGLE_T, PM_T_USE_POINTS (:168-178):                    loss_PM_R, loss_PM_T     */
  CATRE_PM_R_T_DIRECT = 3,    /* PM_DISENTANGLE_T (:179-185):                                     loss_PM_R, loss_PM_T_noP */
  CATRE_PM_R_XY_Z_POINTS = 4, /* PM_DISENTANGLE_Z, PM_T_USE_POINTS (:132-156):      loss_PM_R, loss_PM_xy, loss_PM_z       */
  CATRE_PM_R_XY_Z_DIRECT = 5, /* PM_DISENTANGLE_Z (:157-165):               loss_PM_R, loss_PM_xy_noP, loss_PM_z_noP       */
  CATRE_PM_MODE_COUNT = 6
};
/* Element loss, PM_LOSS_TYPE.lower() (pm_loss.py:70-82). */
enum {
  CATRE_PM_ELEM_L1 = 0,        /* "l1": nn.L1Loss                                                                          */
  CATRE_PM_ELEM_SMOOTH_L1 = 1, /* "smooth_l1": fvcore.nn.smooth_l1_loss with PM_SMOOTH_L1_BETA (below 1e-5: L1)             */
  CATRE_PM_ELEM_MSE = 2,       /* "mse": nn.MSELoss                                                                        */
  CATRE_PM_ELEM_L2 = 3,        /* "l2": L2Loss (core/catre/losses/l2_loss.py:5-28): one norm per object over all of its
                                * differences, mean over objects                                                           */
  CATRE_PM_ELEM_COUNT = 4
};
#define CATRE_LOSS2_TERMS 8 /* loss slots of the *2 entry points (a loss dict holds at most eight terms)                   */
#define CATRE_LOSS2_PART 10 /* floats of part_ws per object                                                                */

typedef struct catre_loss_cfg2 {
  catre_loss_cfg base; /* every field above, unchanged (CATRE_disR_shared.py:168-288)                                      */
  int32_t pm_mode;     /* CATRE_PM_*: PM_R_ONLY / PM_DISENTANGLE_T / PM_DISENTANGLE_Z / PM_T_USE_POINTS (pm_loss.py:56-68) */
  int32_t pm_elem;     /* CATRE_PM_ELEM_*: PM_LOSS_TYPE (pm_loss.py:70-82)                                                 */
  int32_t pm_use_bbox; /* PM_USE_BBOX (pm_loss.py:114-117): the points are the eight corners of the unit cube in the order
                        * of get_normed_bbox (core/catre/engine/engine_utils.py:66-80), generated in the kernel: kps is not
                        * read and M must be 8                                                                             */
  float pm_beta;       /* PM_SMOOTH_L1_BETA (CATRE_disR_shared.py:189; read by CATRE_PM_ELEM_SMOOTH_L1 only)               */
} catre_loss_cfg2;

/* losses[22]: [0..8) = the six terms of catre_loss_fwd, where slot 0 is the first PM term (loss_PM_R, or loss_PM_RT in
 * CATRE_PM_RT), then 6 = the second PM term (loss_PM_T / loss_PM_T_noP / loss_PM_xy / loss_PM_xy_noP) and 7 = the third
 * (loss_PM_z / loss_PM_z_noP); a slot the mode does not have is 0.  [8..22) = the 14 logging scalars of catre_loss_fwd.
 * The point terms carry 3 * PM_LW, the `_noP` terms neither (pm_loss.py:160-164,181-184).  part_ws: B * CATRE_LOSS2_PART
 * floats.  terms / prefix as in catre_loss_fwd_sums with n_terms <= 8 and indices < 8 (both may be NULL / 0).
 * An unknown pm_mode / pm_elem returns CATRE_ERR_BAD_ARG before anything is launched.  With pm_mode ==
 * CATRE_PM_R_ONLY, CATRE_PM_ELEM_L1 and no bbox, slots 0..5, the scalars, dpose and dscale carry the bits of the
 * first entry points. */
int catre_loss_fwd2(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                    const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                    const int32_t* is_sym, const catre_loss_cfg2* cfg, int32_t* best, int32_t* counts, float* part_ws,
                    float* losses, const float* trans_deltas, const int32_t* terms, int n_terms, float* prefix, int B,
                    int M, int S1, void* stream);
/* dpose [B,3,4], dscale [B,3] = gradient of sum_i upstream[i] * losses[i] (upstream: 8 floats on the device, may be NULL)
 * plus the prefix sums' upstreams as in catre_loss_bwd_sums (up_prefix: HOST array of n_terms device pointers).  The PM
 * terms' gradient reaches the translation column of dpose in every mode but CATRE_PM_R_ONLY. */
int catre_loss_bwd2(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                    const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                    const int32_t* best, const int32_t* counts, const float* upstream, const float* const* up_prefix,
                    const int32_t* terms, int n_terms, const catre_loss_cfg2* cfg, float* dpose, float* dscale, int B,
                    int M, int S1, void* stream);

/* ---- the same loss for a batch padded to a fixed capacity (a captured HIP graph whose object count changes per replay) --
 * The arguments of the *2 pair plus n_obj: ONE int32 on the device, 1 <= *n_obj <= B, read when the kernels run.  B stays
 * the capacity that sizes the launches, part_ws, best, dpose and dscale.  Only objects b < *n_obj enter the sums and the
 * counts (counts[1] = *n_obj - counts[0]) and *n_obj stands wherever the *2 pair divides by B: losses, scalars and prefix
 * sums carry the bits of a *2 call on the first *n_obj rows, and so do dpose / dscale of those rows.  Rows b >= *n_obj
 * of dpose / dscale are written as +0; what the inputs hold there does not matter as long as it can be read. */
int catre_loss_fwd3(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                    const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                    const int32_t* is_sym, const catre_loss_cfg2* cfg, int32_t* best, int32_t* counts, float* part_ws,
                    float* losses, const float* trans_deltas, const int32_t* terms, int n_terms, float* prefix, int B,
                    int M, int S1, const int32_t* n_obj, void* stream);
int catre_loss_bwd3(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                    const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                    const int32_t* best, const int32_t* counts, const float* upstream, const float* const* up_prefix,
                    const int32_t* terms, int n_terms, const catre_loss_cfg2* cfg, float* dpose, float* dscale, int B,
                    int M, int S1, const int32_t* n_obj, void* stream);

/* ---- evaluation of refined poses: 3D IoU, degree / cm, greedy matching (core/catre/engine/test_utils.py:523-757) ------
 * What compute_independent_mAP (test_utils.py:760-924) does per image and class, for every image, class, evaluated refine
 * iteration and threshold in three launches.  The per-class AP integration (:112-137) and every ordering by score stay on
 * the host (catre_amd/evaluation.py): the device receives permutations.
 *
 * A GROUP is one (image, class) pair.  Group g holds the predictions pred_off[g] .. pred_off[g+1] (in the order the
 * reference matches them: np.argsort(scores)[::-1] of the group, :557) and the GTs gt_off[g] .. gt_off[g+1]; its np x ng
 * pairs start at pair_off[g], prediction-major.  pred_off / gt_off / pair_off: G + 1 int32 each, non-decreasing, ending at
 * P / NG / Q.  pair_group [Q]: the group of each pair.  pred_idx [P]: the row (< N) of each prediction in pred_pose
 * [T, N, 3, 4] / pred_scale [T, N, 3], T = evaluated iterations (GTs are shared by all of them).  gt_pose [NG, 3, 4],
 * gt_scale [NG, 3], gt_hv [NG] = mug handle visibility.  All poses and scales are float32 as the model returns them and
 * are widened to double; every result below is computed in double. */
enum {
  CATRE_EVAL_GENERIC = 0, /* trace formula with the clip (:681-683), plain IoU                                            */
  CATRE_EVAL_YSYM = 1,    /* bottle / bowl / can: y-axis angle (:665-669), IoU maximised over 20 y rotations of the
                           * PREDICTION (:178-201)                                                                         */
  CATRE_EVAL_MUG = 2,     /* mug: as YSYM for a GT with handle visibility 0 (:179, :671), as GENERIC otherwise             */
  CATRE_EVAL_FLIP = 3,    /* phone / eggbox / glue: min over a 180 degree y flip (:676-680), plain IoU                     */
  CATRE_EVAL_MODE_COUNT = 4
};
#define CATRE_EVAL_NROT 20 /* y rotations of a symmetric prediction (:197) */

/* iou [T, Q] float32 (the reference stores it in a float32 array, :567, and compares that) and degcm [T, Q, 2] double =
 * (degree, cm) of every pair (compute_3d_iou_new :140-205, compute_RT_degree_cm_symmetry :619-689; both rotation blocks
 * divided by cbrt(det), cm = 100 |t1 - t2|).  group_mode [G]: CATRE_EVAL_* of the group's class.  cos_sin: device
 * array of CATRE_EVAL_NROT (cos, sin) double pairs of 2 pi i / 20, computed by the caller with the reference's own
 * numpy calls (:187-200) so that they are its bits.  Deviation: the arccos argument is clamped to [-1, 1] in every
 * branch (the reference clamps the generic one only and returns NaN elsewhere when rounding pushes it past 1).
 * Q == 0 launches nothing.  CATRE_ERR_BAD_ARG: a null array that would be read or written, T / G < 1, a negative size,
 * T * Q beyond int32. */
int catre_eval_overlaps(const float* pred_pose, const float* pred_scale, const int32_t* pred_idx, const float* gt_pose,
                        const float* gt_scale, const int32_t* gt_hv, const int32_t* pred_off, const int32_t* gt_off,
                        const int32_t* pair_off, const int32_t* pair_group, const int32_t* group_mode,
                        const double* cos_sin, float* iou, double* degcm, int T, int N, int P, int NG, int G, int Q,
                        void* stream);
/* Greedy IoU matching of every (iteration, group, threshold) (compute_3d_matches :582-616): predictions in their stored
 * order; each takes the not-yet-matched GT of largest IoU if that IoU is STRICTLY above thres[s]; an IoU equal to the
 * threshold leaves prediction and GT free (:605-614); among equal IoUs the later GT wins (the reversed argsort of :591).
 * thres: S doubles on the device.  pred_match [T, S, P] / gt_match [T, S, NG] int32: in-group index of the partner, -1
 * without one; every element is written. */
int catre_eval_match_iou(const float* iou, const int32_t* pred_off, const int32_t* gt_off, const int32_t* pair_off,
                         const double* thres, int32_t* pred_match, int32_t* gt_match, int T, int S, int P, int NG, int G,
                         int Q, void* stream);
/* Pose matching of every (iteration, group, degree threshold, shift threshold) (compute_match_from_degree_cm :715-757)
 * among the predictions and GTs that catre_eval_match_iou paired at threshold index sel < S (use_matches_for_pose,
 * :855-880); sel = -1: among all (iou_pred_match / iou_gt_match are then not read and may be NULL).  Each prediction, in
 * order, takes the unmatched GT of smallest degree + cm among those with degree <= deg_thres[d] and cm <= cm_thres[c]
 * (equal sums: the earlier GT).  pose_pred_match [T, D, C, P] / pose_gt_match [T, D, C, NG] int32: index of the partner
 * WITHIN THE SELECTED SUBSET of its group (the reference's compacted arrays), -1 without one, -2 for an object outside
 * the subset; every element is written. */
int catre_eval_match_pose(const double* degcm, const int32_t* pred_off, const int32_t* gt_off, const int32_t* pair_off,
                          const int32_t* iou_pred_match, const int32_t* iou_gt_match, int S, int sel,
                          const double* deg_thres, const double* cm_thres, int32_t* pose_pred_match,
                          int32_t* pose_gt_match, int T, int D, int C, int P, int NG, int G, int Q, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CATRE_HIP_H */
