// NOCS-style evaluation of refined poses on the device (the reference's compute_independent_mAP,
// core/catre/engine/test_utils.py:760-924, up to the per-class AP integration, which stays on the host).
//
// The unit of work is a GROUP: the predictions and ground truths (GTs) of one (image, class) pair, addressed through CSR
// offsets (pred_off / gt_off / pair_off, G + 1 entries each).  The evaluated refine iteration t < T is an outer batch
// dimension: GTs are shared by all iterations.  Groups are ragged and tiny, so every kernel below gives ONE THREAD one
// independent piece of serial work and keeps its state in the output arrays - no LDS, no private indexed arrays:
//   k_eval_overlaps    one thread per (t, pred, gt) pair:  IoU (float32, as test_utils.py:567 stores it) + (degree, cm)
//   k_eval_match_iou   one thread per (t, group, IoU threshold):  the greedy rule of compute_3d_matches (:582-616)
//   k_eval_match_pose  one thread per (t, group, degree thr, shift thr):  compute_match_from_degree_cm (:715-757)
// Three launches whatever the number of images.  All arithmetic is double on float32 inputs.
#pragma once
#include "catre_device.h"

#include "../../include/catre_hip.h"

constexpr int EVAL_NROT = 20;   // y rotations of a symmetric prediction (test_utils.py:197)
constexpr int EVAL_THREADS = 128;

// axis-aligned bounds of the 8 corners (+-h0, +-h1, +-h2) under x -> M x + t   (get_3d_bbox + transform_coordinates_3d,
// test_utils.py:50-109); m = 3x4 row-major
__device__ __forceinline__ void eval_aabb(const double (&m)[12], const double (&h)[3], double (&lo)[3], double (&hi)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    lo[r] = INFINITY;
    hi[r] = -INFINITY;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const double x = (c & 2) ? -h[0] : h[0], y = (c & 4) ? -h[1] : h[1], z = (c & 1) ? -h[2] : h[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double v = m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3];
      lo[r] = v < lo[r] ? v : lo[r];
      hi[r] = v > hi[r] ? v : hi[r];
    }
  }
}

// asymmetric_3d_iou (test_utils.py:146-173) of two bounds
__device__ __forceinline__ double eval_aabb_iou(const double (&lo1)[3], const double (&hi1)[3], const double (&lo2)[3],
                                                const double (&hi2)[3]) {
  double d[3], mn = INFINITY;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a = lo1[r] > lo2[r] ? lo1[r] : lo2[r], b = hi1[r] < hi2[r] ? hi1[r] : hi2[r];
    d[r] = b - a;
    mn = d[r] < mn ? d[r] : mn;
  }
  const double inter = mn < 0.0 ? 0.0 : d[0] * d[1] * d[2];
  const double uni = (hi1[0] - lo1[0]) * (hi1[1] - lo1[1]) * (hi1[2] - lo1[2]) +
                     (hi2[0] - lo2[0]) * (hi2[1] - lo2[1]) * (hi2[2] - lo2[2]) - inter;
  return inter / uni;
}

// the 3x3 block of m divided by cbrt(det)   (test_utils.py:658, 661)
__device__ __forceinline__ void eval_unit_rot(const double (&m)[12], double (&r)[9]) {
  const double det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) +
                     m[2] * (m[4] * m[9] - m[5] * m[8]);
  const double c = cbrt(det);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r[3 * i + j] = m[4 * i + j] / c;
}

// arccos in degrees with the argument clamped to [-1, 1] in EVERY branch (the reference clamps the generic branch only,
// test_utils.py:669-683, and returns NaN elsewhere when rounding pushes the argument past 1); NaN stays NaN
__device__ __forceinline__ double eval_acos_deg(double x) {
  x = x > 1.0 ? 1.0 : (x < -1.0 ? -1.0 : x);
  return acos(x) * (180.0 / 3.14159265358979323846);
}

// group_mode: how a class is compared (test_utils.py:178-180, 665-683)
//   CATRE_EVAL_GENERIC  trace formula, plain IoU
//   CATRE_EVAL_YSYM     bottle / bowl / can: y-axis angle, IoU maximised over the y rotations
//   CATRE_EVAL_MUG      as YSYM where the GT's handle visibility is 0, else GENERIC
//   CATRE_EVAL_FLIP     phone / eggbox / glue: min over a 180 degree y flip, plain IoU
__global__ void __launch_bounds__(EVAL_THREADS)
    k_eval_overlaps(const float* __restrict__ pred_pose, const float* __restrict__ pred_scale,
                    const int32_t* __restrict__ pred_idx, const float* __restrict__ gt_pose,
                    const float* __restrict__ gt_scale, const int32_t* __restrict__ gt_hv,
                    const int32_t* __restrict__ pred_off, const int32_t* __restrict__ gt_off,
                    const int32_t* __restrict__ pair_off, const int32_t* __restrict__ pair_group,
                    const int32_t* __restrict__ group_mode, const double* __restrict__ cos_sin, float* __restrict__ iou,
                    double* __restrict__ degcm, int T, int N, int P, int NG, int G, int Q) {
  const long idx = (long)blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (idx >= (long)T * Q) return;
  const int t = (int)(idx / Q), q = (int)(idx % Q);
  const int g = pair_group[q];
  if ((unsigned)g >= (unsigned)G) return;
  const int ng = gt_off[g + 1] - gt_off[g], l = q - pair_off[g];
  if (ng <= 0 || l < 0) return;
  const int pi = pred_off[g] + l / ng, gj = gt_off[g] + l % ng;
  if ((unsigned)pi >= (unsigned)P || (unsigned)gj >= (unsigned)NG) return;
  const int row = pred_idx[pi];
  if ((unsigned)row >= (unsigned)N) return;

  double m1[12], m2[12], h1[3], h2[3];
  const float* pp = pred_pose + ((size_t)t * N + row) * 12;
  const float* gp = gt_pose + (size_t)gj * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    m1[i] = (double)pp[i];
    m2[i] = (double)gp[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    h1[i] = (double)pred_scale[((size_t)t * N + row) * 3 + i] / 2;
    h2[i] = (double)gt_scale[(size_t)gj * 3 + i] / 2;
  }
  const int mode = group_mode[g];
  const bool ysym = mode == CATRE_EVAL_YSYM || (mode == CATRE_EVAL_MUG && gt_hv[gj] == 0);

  // ---- IoU (compute_3d_iou_new, test_utils.py:140-205): the prediction is RT_1, rotated about its y axis when symmetric
  double lo2[3], hi2[3];
  eval_aabb(m2, h2, lo2, hi2);
  const int nrot = ysym ? EVAL_NROT : 1;   // rotation 0 is the identity (cos 0 = 1, sin 0 = 0 exactly)
  double best = 0.0;
#pragma unroll 1
  for (int r = 0; r < nrot; ++r) {
    const double c = cos_sin[2 * r], s = cos_sin[2 * r + 1];
    double mr[12], lo1[3], hi1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // RT_1 @ y_rotation_matrix(theta)
      mr[4 * i] = m1[4 * i] * c - m1[4 * i + 2] * s;
      mr[4 * i + 1] = m1[4 * i + 1];
      mr[4 * i + 2] = m1[4 * i] * s + m1[4 * i + 2] * c;
      mr[4 * i + 3] = m1[4 * i + 3];
    }
    eval_aabb(mr, h1, lo1, hi1);
    const double v = eval_aabb_iou(lo1, hi1, lo2, hi2);
    if (!ysym)
      best = v;
    else if (v > best)   // max(max_iou, v) starting from 0
      best = v;
  }
  iou[(size_t)t * Q + q] = (float)best;

  // ---- (degree, cm) (compute_RT_degree_cm_symmetry, test_utils.py:619-689)
  double r1[9], r2[9];
  eval_unit_rot(m1, r1);
  eval_unit_rot(m2, r2);
  double theta;
  if (ysym) {
    const double dot = r1[1] * r2[1] + r1[4] * r2[4] + r1[7] * r2[7];
    const double n1 = sqrt(r1[1] * r1[1] + r1[4] * r1[4] + r1[7] * r1[7]);
    const double n2 = sqrt(r2[1] * r2[1] + r2[4] * r2[4] + r2[7] * r2[7]);
    theta = eval_acos_deg(dot / (n1 * n2));
  } else {
    double tr = 0.0, trf = 0.0;   // trace(R1 R2^T), trace(R1 diag(-1, 1, -1) R2^T)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double a = r1[3 * i] * r2[3 * i], b = r1[3 * i + 1] * r2[3 * i + 1], c = r1[3 * i + 2] * r2[3 * i + 2];
      tr += a + b + c;
      trf += b - a - c;
    }
    theta = eval_acos_deg((tr - 1.0) / 2);
    if (mode == CATRE_EVAL_FLIP) {
      const double tf = eval_acos_deg((trf - 1.0) / 2);
      theta = tf < theta ? tf : theta;
    }
  }
  const double d0 = m1[3] - m2[3], d1 = m1[7] - m2[7], d2 = m1[11] - m2[11];
  degcm[((size_t)t * Q + q) * 2] = theta;
  degcm[((size_t)t * Q + q) * 2 + 1] = sqrt(d0 * d0 + d1 * d1 + d2 * d2) * 100.0;
}

// Greedy IoU matching (compute_3d_matches, test_utils.py:582-616).  Predictions in their stored (score) order; each takes the
// not-yet-matched GT of largest IoU (equal IoUs: the later GT, as the reversed stable argsort of :591 has it) if that IoU,
// a float32, is strictly above the threshold.  An IoU equal to the threshold leaves both free (:605-614).
// pred_match [T, S, P] / gt_match [T, S, NG]: in-group index of the partner, -1 = none; the thread owns its slices.
__global__ void __launch_bounds__(EVAL_THREADS)
    k_eval_match_iou(const float* __restrict__ iou, const int32_t* __restrict__ pred_off,
                     const int32_t* __restrict__ gt_off, const int32_t* __restrict__ pair_off,
                     const double* __restrict__ thres, int32_t* pred_match, int32_t* gt_match, int T, int S, int P,
                     int NG, int G, int Q) {
  const long idx = (long)blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (idx >= (long)T * S * G) return;
  const int g = (int)(idx % G), s = (int)((idx / G) % S), t = (int)(idx / ((long)G * S));
  const int p0 = pred_off[g], np = pred_off[g + 1] - p0, g0 = gt_off[g], ng = gt_off[g + 1] - g0;
  if (p0 < 0 || np < 0 || p0 + np > P || g0 < 0 || ng < 0 || g0 + ng > NG) return;
  const int q0 = pair_off[g];
  if (q0 < 0 || (long)q0 + (long)np * ng > Q) return;
  const float* ov = iou + (size_t)t * Q + q0;
  int32_t* pm = pred_match + ((size_t)t * S + s) * P + p0;
  int32_t* gm = gt_match + ((size_t)t * S + s) * NG + g0;
  const double th = thres[s];
  for (int j = 0; j < ng; ++j) gm[j] = -1;
  for (int i = 0; i < np; ++i) {
    int bj = -1;
    float bv = 0.f;
    for (int j = 0; j < ng; ++j) {
      if (gm[j] >= 0) continue;
      const float v = ov[(size_t)i * ng + j];
      if (bj < 0 || v >= bv) {
        bj = j;
        bv = v;
      }
    }
    const bool hit = bj >= 0 && (double)bv > th;
    pm[i] = hit ? bj : -1;
    if (hit) gm[bj] = i;
  }
}

// Pose matching (compute_match_from_degree_cm, test_utils.py:715-757) among the predictions and GTs that IoU matching paired
// at threshold index `sel` (use_matches_for_pose, :855-880; sel < 0: among all).  Predictions keep their order; each takes the
// unmatched GT of smallest degree + cm among those with degree <= thr and cm <= thr (equal sums: the earlier GT).
// pose_pred_match [T, D, C, P] / pose_gt_match [T, D, C, NG]: index of the partner IN THE SELECTED SUBSET of its group (what
// the reference's compacted arrays hold), -1 = none, -2 = the object is not in the subset.
__global__ void __launch_bounds__(EVAL_THREADS)
    k_eval_match_pose(const double* __restrict__ degcm, const int32_t* __restrict__ pred_off,
                      const int32_t* __restrict__ gt_off, const int32_t* __restrict__ pair_off,
                      const int32_t* __restrict__ iou_pred_match, const int32_t* __restrict__ iou_gt_match, int S, int sel,
                      const double* __restrict__ deg_thres, const double* __restrict__ cm_thres, int32_t* pose_pred_match,
                      int32_t* pose_gt_match, int T, int D, int C, int P, int NG, int G, int Q) {
  const long idx = (long)blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (idx >= (long)T * D * C * G) return;
  const int g = (int)(idx % G), c = (int)((idx / G) % C), d = (int)((idx / ((long)G * C)) % D);
  const int t = (int)(idx / ((long)G * C * D));
  const int p0 = pred_off[g], np = pred_off[g + 1] - p0, g0 = gt_off[g], ng = gt_off[g + 1] - g0;
  if (p0 < 0 || np < 0 || p0 + np > P || g0 < 0 || ng < 0 || g0 + ng > NG) return;
  const int q0 = pair_off[g];
  if (q0 < 0 || (long)q0 + (long)np * ng > Q) return;
  const double* dc = degcm + ((size_t)t * Q + q0) * 2;
  const int32_t* ipm = sel < 0 ? nullptr : iou_pred_match + ((size_t)t * S + sel) * P + p0;
  const int32_t* igm = sel < 0 ? nullptr : iou_gt_match + ((size_t)t * S + sel) * NG + g0;
  int32_t* pm = pose_pred_match + (((size_t)t * D + d) * C + c) * P + p0;
  int32_t* gm = pose_gt_match + (((size_t)t * D + d) * C + c) * NG + g0;
  const double dth = deg_thres[d], cth = cm_thres[c];
  for (int j = 0; j < ng; ++j) gm[j] = (!igm || igm[j] >= 0) ? -1 : -2;
  int ci = 0;   // index of prediction i in the subset
  for (int i = 0; i < np; ++i) {
    if (ipm && ipm[i] < 0) {
      pm[i] = -2;
      continue;
    }
    int bj = -1, bc = -1, cj = 0;
    double bs = 0.0;
    for (int j = 0; j < ng; ++j) {
      const int32_t m = gm[j];
      if (m == -2) continue;
      const int cjj = cj++;
      if (m >= 0) continue;
      const double de = dc[((size_t)i * ng + j) * 2], cm = dc[((size_t)i * ng + j) * 2 + 1];
      if (de > dth || cm > cth) continue;
      const double sum = de + cm;
      if (bj < 0 || sum < bs) {
        bj = j;
        bc = cjj;
        bs = sum;
      }
    }
    pm[i] = bc;
    if (bj >= 0) gm[bj] = ci;
    ++ci;
  }
}
