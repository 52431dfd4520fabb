// catre_loss.h - SURVEY.md row f1: the training loss of CATRE_disR_shared.catre_loss
// (core/catre/models/CATRE_disR_shared.py:168-288) with the whole of PyPMLoss (core/catre/losses/pm_loss.py:85-194:
// six structural modes x {l1, smooth_l1, mse, l2} x with_scale x symmetric x bbox points) and the symmetry-aware
// choice of the ground-truth rotation (core/utils/pose_utils.py:472-528), forward and backward, one workgroup per
// object.  The reference evaluates up to 314 candidate rotations per symmetric object in a numpy loop on the host and
// syncs ~20 scalars per iteration; the first device version used ~150 small torch kernels per iteration.  Here:
// k_loss_fwd + k_loss_reduce, and k_loss_bwd - the same three launches for every form.
//
// The shipped form (l1, R only, key points) runs the loop it always ran, statement for statement, in a branch of its
// own: its bits are pinned by tests/golden/loss_abi_shipped.npz.  Every other form takes the general loop below it.
#pragma once
#include "catre_device.h"

#include "../../include/catre_hip.h"

typedef catre_loss_cfg2 LossCfg;  // include/catre_hip.h: catre_loss_cfg (first member `base`) + the PM form

// per-object partial sums: 0 PM term 0 (loss_PM_R or loss_PM_RT), 1 rot (non-sym), 2 y-axis (sym), 3 trans xy (or xyz),
// 4 trans z, 5 scale, 6 rotation error re() in degrees, 7 translation error te() (lib/pysixd/pose_error.py:359-374,
// 406-417) - these two feed the forward-side logging scalars of CATRE_disR_shared.forward (reference :127-164) -,
// 8 PM term 1 (loss_PM_T / _T_noP / _xy / _xy_noP), 9 PM term 2 (loss_PM_z / _z_noP).  For the element loss l2
// (L2Loss, core/catre/losses/l2_loss.py:5-28) a PM column holds the object's Euclidean norm, else its sum.
// The row is `np` floats wide: LOSS_NP for the catre_loss_{fwd,bwd}{,_sums} entry points (whose callers allocate B * 8
// floats and have one PM term), LOSS_NP2 for the *2 entry points.
#define LOSS_NP 8
#define LOSS_NP2 10
#define LOSS_NVIS 14
// loss slots: 6 for the first entry points (losses[6 + 14]), 8 for the *2 ones (losses[8 + 14]): 6 = PM term 1, 7 = PM term 2
#define LOSS_NL 6
#define LOSS_NL2 8
static_assert(LOSS_NP2 == CATRE_LOSS2_PART && LOSS_NL2 == CATRE_LOSS2_TERMS, "include/catre_hip.h documents these sizes");

// PM element loss on one difference (pm_loss.py:70-82); l2 accumulates squares, the root is taken per object
__device__ __forceinline__ float pm_elem(float d, int elem, float beta) {
  const float a = fabsf(d);
  switch (elem) {
    case CATRE_PM_ELEM_SMOOTH_L1: return (beta < 1e-5f) ? a : (a < beta ? 0.5f * d * d / beta : a - 0.5f * beta);  // fvcore
    case CATRE_PM_ELEM_MSE:
    case CATRE_PM_ELEM_L2: return d * d;
    default: return a;
  }
}
// its derivative; l2: d / norm (inv_norm = 1 / the object's norm, 0 for a zero norm)
__device__ __forceinline__ float pm_elem_grad(float d, int elem, float beta, float inv_norm) {
  const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);  // torch: sign(0) = 0
  switch (elem) {
    case CATRE_PM_ELEM_SMOOTH_L1: return (beta < 1e-5f) ? sg : (fabsf(d) < beta ? d / beta : sg);
    case CATRE_PM_ELEM_MSE: return 2.f * d;
    case CATRE_PM_ELEM_L2: return d * inv_norm;
    default: return sg;
  }
}
// the model point m of object b: a key point, or corner m of the unit cube in the order of get_normed_bbox
// (core/catre/engine/engine_utils.py:66-80)
__device__ __forceinline__ void pm_point(const float* __restrict__ kps, int use_bbox, int b, int M, int m, float (&q)[3]) {
  if (use_bbox) {
    const int c = m & 3;
    q[0] = (c == 0 || c == 3) ? 0.5f : -0.5f;
    q[1] = c < 2 ? 0.5f : -0.5f;
    q[2] = m < 4 ? 0.5f : -0.5f;
  } else {
    const float* p = kps + ((size_t)b * M + m) * 3;
    q[0] = p[0], q[1] = p[1], q[2] = p[2];
  }
}
// which point terms a mode has besides term 0, and what term 0 / 1 / 2 compare (pm_loss.py:126-192)
__device__ __forceinline__ bool pm_points_t(int mode) { return mode == CATRE_PM_R_T_POINTS || mode == CATRE_PM_R_XY_Z_POINTS; }
__device__ __forceinline__ bool pm_shipped(const LossCfg& c) {
  return c.pm_mode == CATRE_PM_R_ONLY && c.pm_elem == CATRE_PM_ELEM_L1 && !c.pm_use_bbox;
}
// the three differences of point component i in the general loop: e, g = rotated (scaled) point under the estimate /
// the target rotation; t, tg = estimated / true translation.  d0: term 0; d1, d2: the point forms of terms 1 and 2
// (est = target points + a translation whose replaced components are the true ones: those differences are exact zeros)
__device__ __forceinline__ void pm_diffs(int mode, int i, float e, float g, float t, float tg, float& d0, float& d1, float& d2) {
  d1 = d2 = 0.f;
  if (mode == CATRE_PM_RT) {
    d0 = (e + t) - (g + tg);
  } else if (pm_points_t(mode)) {
    const float tgt = g + tg;
    d0 = (e + tg) - tgt;
    if (mode == CATRE_PM_R_T_POINTS) {
      d1 = (g + t) - tgt;
    } else {
      d1 = (g + (i < 2 ? t : tg)) - tgt;
      d2 = (g + (i < 2 ? tg : t)) - tgt;
    }
  } else {
    d0 = e - g;
  }
}

__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// R_gt @ S_k for candidate k (k = 0 is the identity)
__device__ __forceinline__ void sym_candidate(const float* __restrict__ G, const float* __restrict__ S, float (&C)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = G[i * 3] * S[j] + G[i * 3 + 1] * S[3 + j] + G[i * 3 + 2] * S[6 + j];
}

// best[b] = arg-max over the valid candidates of clamp((min(trace(P C^T), 3) - 1) / 2, -1, 1), first maximum
// (== the reference's strict `<` scan over re() that starts at the un-rotated ground truth)
__device__ __forceinline__ int closest_candidate(const float* __restrict__ P, const float* __restrict__ G,
                                                 const float* __restrict__ cands, const unsigned char* __restrict__ valid,
                                                 int S1, float* sval, int* sidx) {
  float bv = -3.f;
  int bi = 0x7fffffff;
  for (int k = threadIdx.x; k < S1; k += 256) {
    if (!valid[k]) continue;
    float C[9];
    sym_candidate(G, cands + (size_t)k * 9, C);
    float tr = 0.f;
#pragma unroll
    for (int e = 0; e < 9; ++e) tr = fmaf(P[e], C[e], tr);
    const float v = fminf(fmaxf(0.5f * (fminf(tr, 3.0f) - 1.0f), -1.0f), 1.0f);
    if (v > bv) {  // k increases within a thread: strict > keeps the first
      bv = v;
      bi = k;
    }
  }
  sval[threadIdx.x] = bv;
  sidx[threadIdx.x] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const float v2 = sval[threadIdx.x + o];
      const int i2 = sidx[threadIdx.x + o];
      if (v2 > sval[threadIdx.x] || (v2 == sval[threadIdx.x] && i2 < sidx[threadIdx.x])) {
        sval[threadIdx.x] = v2;
        sidx[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  return sidx[0];
}

__device__ __forceinline__ float smooth_l1(float d) {  // beta = 1
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

__global__ __launch_bounds__(256) void k_loss_fwd(const float* __restrict__ pose /*[B,3,4]*/,
                                                  const float* __restrict__ scale, const float* __restrict__ gt_rot,
                                                  const float* __restrict__ gt_trans, const float* __restrict__ gt_scale,
                                                  const float* __restrict__ kps /*[B,M,3]*/,
                                                  const float* __restrict__ cands /*[B,S1,3,3]*/,
                                                  const unsigned char* __restrict__ valid /*[B,S1]*/,
                                                  const int* __restrict__ is_sym, LossCfg cfg, int* __restrict__ best,
                                                  float* __restrict__ part /*[B][np]*/, int B, int M, int S1,
                                                  int np = LOSS_NP) {
  __shared__ float sval[256];
  __shared__ int sidx[256];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* Pp = pose + b * 12;
  const float P[9] = {Pp[0], Pp[1], Pp[2], Pp[4], Pp[5], Pp[6], Pp[8], Pp[9], Pp[10]};
  const float t[3] = {Pp[3], Pp[7], Pp[11]};
  const float* G = gt_rot + b * 9;
  float out[LOSS_NP2];
#pragma unroll
  for (int i = 0; i < LOSS_NP2; ++i) out[i] = 0.f;
  if (cfg.base.pm_on) {
    int k = 0;
    if (cfg.base.pm_sym) k = closest_candidate(P, G, cands + (size_t)b * S1 * 9, valid + (size_t)b * S1, S1, sval, sidx);
    if (tid == 0) best[b] = k;
    float C[9];
    sym_candidate(G, cands + ((size_t)b * S1 + k) * 9, C);
    float se[3], sg[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      se[j] = cfg.base.pm_with_scale ? scale[b * 3 + j] : 1.f;
      sg[j] = cfg.base.pm_with_scale ? gt_scale[b * 3 + j] : 1.f;
    }
    if (pm_shipped(cfg)) {  // (the loop as it always was, its indentation included)
    float acc = 0.f;
    for (int m = tid; m < M; m += 256) {
      const float* q = kps + ((size_t)b * M + m) * 3;
      const float pe[3] = {q[0] * se[0], q[1] * se[1], q[2] * se[2]}, pt[3] = {q[0] * sg[0], q[1] * sg[1], q[2] * sg[2]};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float e = P[i * 3] * pe[0] + P[i * 3 + 1] * pe[1] + P[i * 3 + 2] * pe[2];
        const float g = C[i * 3] * pt[0] + C[i * 3 + 1] * pt[1] + C[i * 3 + 2] * pt[2];
        acc += fabsf(e - g);
      }
    }
    out[0] = block_sum256(acc, red);
    } else {
      // every other form: up to three point sums per object (pm_diffs), then the `_noP` terms on the translation itself
      const int mode = cfg.pm_mode, elem = cfg.pm_elem;
      const float beta = cfg.pm_beta;
      const float tg[3] = {gt_trans[b * 3], gt_trans[b * 3 + 1], gt_trans[b * 3 + 2]};
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      for (int m = tid; m < M; m += 256) {
        float q[3];
        pm_point(kps, cfg.pm_use_bbox, b, M, m, q);
        const float pe[3] = {q[0] * se[0], q[1] * se[1], q[2] * se[2]}, pt[3] = {q[0] * sg[0], q[1] * sg[1], q[2] * sg[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float e = P[i * 3] * pe[0] + P[i * 3 + 1] * pe[1] + P[i * 3 + 2] * pe[2];
          const float g = C[i * 3] * pt[0] + C[i * 3 + 1] * pt[1] + C[i * 3 + 2] * pt[2];
          float d0, d1, d2;
          pm_diffs(mode, i, e, g, t[i], tg[i], d0, d1, d2);
          a0 += pm_elem(d0, elem, beta);
          a1 += pm_elem(d1, elem, beta);
          a2 += pm_elem(d2, elem, beta);
        }
      }
      const bool l2 = elem == CATRE_PM_ELEM_L2;
      a0 = block_sum256(a0, red);
      out[0] = l2 ? sqrtf(a0) : a0;
      if (pm_points_t(mode)) {
        a1 = block_sum256(a1, red);
        out[8] = l2 ? sqrtf(a1) : a1;
        if (mode == CATRE_PM_R_XY_Z_POINTS) {
          a2 = block_sum256(a2, red);
          out[9] = l2 ? sqrtf(a2) : a2;
        }
      } else if (mode == CATRE_PM_R_T_DIRECT || mode == CATRE_PM_R_XY_Z_DIRECT) {
        // the element loss on [B,3] (T_noP) or on [B,2] and [B] (xy_noP, z_noP): l2 = the norm over 3, 2 and 1 numbers
        const float f0 = pm_elem(t[0] - tg[0], elem, beta), f1 = pm_elem(t[1] - tg[1], elem, beta),
                    f2 = pm_elem(t[2] - tg[2], elem, beta);
        if (mode == CATRE_PM_R_T_DIRECT) {
          out[8] = l2 ? sqrtf(f0 + f1 + f2) : f0 + f1 + f2;
        } else {
          out[8] = l2 ? sqrtf(f0 + f1) : f0 + f1;
          out[9] = l2 ? sqrtf(f2) : f2;
        }
      }
    }
  }
  if (tid == 0) {
    if (cfg.base.rot_on) {
      if (!is_sym[b]) {
        if (cfg.base.rot_l2) {
          float s = 0.f;
#pragma unroll
          for (int e = 0; e < 9; ++e) s += (P[e] - G[e]) * (P[e] - G[e]);
          out[1] = s;
        } else {
          float tr = 0.f;
#pragma unroll
          for (int e = 0; e < 9; ++e) tr += P[e] * G[e];
          out[1] = (1.f - (tr - 1.f) / 2.f) / 2.f;
        }
      } else {
        float s = 0.f;
        if (cfg.base.yaxis_smooth >= 2) {  // 2: L2Loss (l2_loss.py:5-28, per-object norm); 3: angular_distance_vec (rot_loss.py:33-42)
          float dd = 0.f, pg = 0.f, pp = 0.f, gg = 0.f;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const float p = P[i * 3 + 1], g = G[i * 3 + 1];
            dd += (p - g) * (p - g);
            pg += p * g;
            pp += p * p;
            gg += g * g;
          }
          s = cfg.base.yaxis_smooth == 2 ? sqrtf(dd) : (1.f - pg / (sqrtf(pp) * sqrtf(gg))) * 0.5f;
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const float d = P[i * 3 + 1] - G[i * 3 + 1];
            s += cfg.base.yaxis_smooth ? smooth_l1(d) : fabsf(d);
          }
        }
        out[2] = s;
      }
    }
    if (cfg.base.trans_on) {
      const float d[3] = {t[0] - gt_trans[b * 3], t[1] - gt_trans[b * 3 + 1], t[2] - gt_trans[b * 3 + 2]};
      float f[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) f[i] = cfg.base.trans_mse == 1 ? d[i] * d[i] : fabsf(d[i]);
      if (cfg.base.trans_mse == 2) {  // L2Loss: per-object Euclidean norm
        out[3] = sqrtf(cfg.base.trans_split ? d[0] * d[0] + d[1] * d[1] : d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      } else {
        out[3] = cfg.base.trans_split ? f[0] + f[1] : f[0] + f[1] + f[2];
      }
      out[4] = f[2];
    }
    if (cfg.base.scale_on) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float d = scale[b * 3 + i] - gt_scale[b * 3 + i];
        s += cfg.base.scale_mse ? d * d : fabsf(d);
      }
      out[5] = cfg.base.scale_mse == 2 ? sqrtf(s) : s;
    }
    {  // compute_mean_re_te (models/model_utils.py:226-238): re against the plain ground truth, te
      float tr = 0.f;
#pragma unroll
      for (int e = 0; e < 9; ++e) tr = fmaf(P[e], G[e], tr);  // trace(R_est R_gt^T)
      tr = fminf(tr, 3.0f);
      out[6] = acosf(fminf(1.0f, fmaxf(-1.0f, 0.5f * (tr - 1.0f)))) * 57.29577951308232f;
      const float d0 = gt_trans[b * 3] - t[0], d1 = gt_trans[b * 3 + 1] - t[1], d2 = gt_trans[b * 3 + 2] - t[2];
      out[7] = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    }
#pragma unroll
    for (int i = 0; i < LOSS_NP2; ++i)
      if (i < np) part[(size_t)b * np + i] = out[i];
  }
}

// losses[6] = PM_R, rot, yaxis_rot, trans_xy (or trans), trans_z, scale: objects summed in order, then normalised
// counts[2] = {objects with symmetry info, without}: taken from is_sym on the device, so a captured graph stays valid
// when the mix of objects changes from batch to batch
// losses[6 .. 6+14) = the reference's vis/ scalars in its own order: error_R [deg], error_t [cm], |t_pred - t_gt| of
// object 0 [cm] x3, t_pred x3, trans_deltas x3 (0 when no deltas are passed), t_gt x3 - all of object 0 like the
// reference (`pred_trans[0, 0]` ...)
// column sums of part [B][np] and the symmetric-object count: wave w of the 8 adds column w, and column 8 + w where the row
// has one (lane l: objects l, l + 64, ... in order, then the butterfly over lanes - a fixed order), wave 0 also counts
// is_sym.  (A single wave walking the objects in order was 2 x 16 dependent L2 round trips: 13.5 us.)
// nl = LOSS_NL: losses[6 + 14] as the first entry points lay it out; LOSS_NL2: losses[8 + 14], slots 6, 7 = PM terms 1, 2.
__global__ __launch_bounds__(512) void k_loss_reduce(const float* __restrict__ part, const int* __restrict__ is_sym, LossCfg cfg,
                                                     float* __restrict__ losses, int* __restrict__ counts, int B_cap, int M,
                                                     const float* __restrict__ pose, const float* __restrict__ gt_trans,
                                                     const float* __restrict__ trans_deltas, unsigned term_order = 0,
                                                     int n_terms = 0, float* __restrict__ prefix = nullptr, int np = LOSS_NP,
                                                     int nl = LOSS_NL, const int* __restrict__ n_obj = nullptr) {
  static_assert(LOSS_NP == 8 && LOSS_NP2 <= 16, "eight waves: one per column of the first eight, one more pass for the rest");
  static_assert(LOSS_NL2 * 4 <= 32, "term_order packs four bits per term");
  __shared__ float colsum[LOSS_NP2];
  __shared__ float lossv[LOSS_NL2];
  __shared__ int nsym_s;
  // the *3 entry points: objects 0 .. *n_obj - 1 of the B rows count (one plain load, the same value in every lane); the
  // walk below is then the walk of a plain call on those rows, addition for addition
  const int B = n_obj ? min(*n_obj, B_cap) : B_cap;  // (a count above the capacity must not walk off the buffers)
  {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float s = 0.f, c = 0.f;
    for (int b = lane; b < B; b += 64) {
      s += part[(size_t)b * np + w];
      if (w == 0) c += is_sym[b] != 0 ? 1.f : 0.f;
    }
    s = wave_sum(s);
    if (w == 0) c = wave_sum(c);
    if (lane == 0) colsum[w] = s;
    if (lane == 0 && w == 0) nsym_s = (int)c;
    if (LOSS_NP + w < np) {
      float s2 = 0.f;
      for (int b = lane; b < B; b += 64) s2 += part[(size_t)b * np + LOSS_NP + w];
      s2 = wave_sum(s2);
      if (lane == 0) colsum[LOSS_NP + w] = s2;
    }
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= nl && i < nl + LOSS_NVIS) {
    const int k = i - nl;
    float v;
    if (k < 2) {
      const float s = colsum[6 + k];
      v = s / (float)B * (k == 1 ? 100.f : 1.f);
    } else {
      const int c = (k - 2) % 3, what = (k - 2) / 3;
      const float tp = pose[c * 4 + 3], tg = gt_trans[c];
      v = what == 0 ? fabsf(tp - tg) * 100.f : what == 1 ? tp : what == 2 ? (trans_deltas ? trans_deltas[c] : 0.f) : tg;
    }
    losses[i] = v;
  }
  // prefix[k] = ((0 + l[t0]) + l[t1]) + ... + l[tk] over the terms the caller's loss dict holds, in its order: what python's
  // `sum(loss_dict.values())` (engine.py:318) builds one add kernel at a time - same operations, same bits
  if (i < nl) {
  const int n_sym = nsym_s;
  const int n_nonsym = B - n_sym;
  if (i == 0) {
    counts[0] = n_sym;
    counts[1] = n_nonsym;
  }
  const float s = i < 6 ? colsum[i] : (np > LOSS_NP ? colsum[LOSS_NP + (i - 6)] : 0.f);
  const bool pm_l2 = cfg.pm_elem == CATRE_PM_ELEM_L2;
  float v = 0.f;
  switch (i) {
    // a point term: 3 * mean * PM_LW ("3 is for mean reduction on the point dim", pm_loss.py:193); l2: mean over objects
    case 0: v = 3.f * (s / (pm_l2 ? (float)B : (float)B * M * 3.f)) * cfg.base.pm_lw; break;
    case 1: v = n_nonsym > 0 ? s / ((float)n_nonsym * (cfg.base.rot_l2 ? 9.f : 1.f)) * cfg.base.rot_lw : 0.f; break;
    case 2: v = n_sym > 0 ? s / ((float)n_sym * (cfg.base.yaxis_smooth >= 2 ? 1.f : 3.f)) * cfg.base.rot_lw : 0.f; break;
    case 3: v = s / ((float)B * (cfg.base.trans_mse == 2 ? 1.f : cfg.base.trans_split ? 2.f : 3.f)) * cfg.base.trans_lw; break;
    case 4: v = s / (float)B * cfg.base.trans_lw; break;
    case 5: v = s / ((float)B * (cfg.base.scale_mse == 2 ? 1.f : 3.f)) * cfg.base.scale_lw; break;
    case 6:  // loss_PM_T / loss_PM_xy (point terms), loss_PM_T_noP / loss_PM_xy_noP (plain means: no 3, no PM_LW)
      if (pm_points_t(cfg.pm_mode)) v = 3.f * (s / (pm_l2 ? (float)B : (float)B * M * 3.f)) * cfg.base.pm_lw;
      else if (cfg.pm_mode == CATRE_PM_R_T_DIRECT) v = s / (pm_l2 ? (float)B : (float)B * 3.f);
      else if (cfg.pm_mode == CATRE_PM_R_XY_Z_DIRECT) v = s / (pm_l2 ? (float)B : (float)B * 2.f);
      break;
    case 7:  // loss_PM_z, loss_PM_z_noP
      if (cfg.pm_mode == CATRE_PM_R_XY_Z_POINTS) v = 3.f * (s / (pm_l2 ? (float)B : (float)B * M * 3.f)) * cfg.base.pm_lw;
      else if (cfg.pm_mode == CATRE_PM_R_XY_Z_DIRECT) v = s / (float)B;
      break;
  }
  losses[i] = v;
  lossv[i] = v;
  }
  if (n_terms <= 0 || !prefix) return;
  __syncthreads();
  if (i == 0) {
    float acc = 0.f;
    for (int k = 0; k < n_terms; ++k) {
      acc += lossv[(term_order >> (4 * k)) & 15u];
      prefix[k] = acc;
    }
  }
}

// upstream gradients of the running sums (one device scalar each, null = zero)
struct LossUpPrefix {
  const float* p[LOSS_NL2] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

// d(sum_i up[i] * losses[i]) / d(pose, scale);  up = the nl (six or eight) upstream gradients (device)
__global__ __launch_bounds__(256) void k_loss_bwd(const float* __restrict__ pose, const float* __restrict__ scale,
                                                  const float* __restrict__ gt_rot, const float* __restrict__ gt_trans,
                                                  const float* __restrict__ gt_scale, const float* __restrict__ kps,
                                                  const float* __restrict__ cands, const int* __restrict__ is_sym,
                                                  const int* __restrict__ best, const float* __restrict__ up_, LossCfg cfg,
                                                  const int* __restrict__ counts, float* __restrict__ dpose /*[B,3,4]*/,
                                                  float* __restrict__ dscale, int B_cap, int M, int S1,
                                                  const LossUpPrefix up_prefix = LossUpPrefix{}, unsigned term_order = 0,
                                                  int n_terms = 0, int nl = LOSS_NL,
                                                  const int* __restrict__ n_obj = nullptr) {
  __shared__ float red[4];
  // the *3 entry points: *n_obj objects count (uniform over the workgroup); a row past them gets exact +0 - it is written,
  // not skipped, because the caller's dpose / dscale are uninitialised
  const int B = n_obj ? min(*n_obj, B_cap) : B_cap;  // (a count above the capacity must not walk off the buffers)
  if ((int)blockIdx.x >= B) {
    if (threadIdx.x < 12) dpose[blockIdx.x * 12 + threadIdx.x] = 0.f;
    if (threadIdx.x < 3) dscale[blockIdx.x * 3 + threadIdx.x] = 0.f;
    return;
  }
  // effective upstream of loss i: its own (up_in, optional) plus that of every prefix sum it is part of (k >= its position)
  float up[LOSS_NL2];
  {
    const float* up_in = up_;
#pragma unroll
    for (int i = 0; i < LOSS_NL2; ++i) up[i] = (up_in && i < nl) ? up_in[i] : 0.f;
    {
      float tail = 0.f;
      for (int k = n_terms - 1; k >= 0; --k) {
        if (up_prefix.p[k]) tail += up_prefix.p[k][0];
        const int t = (term_order >> (4 * k)) & 15u;
#pragma unroll
        for (int i = 0; i < LOSS_NL2; ++i)
          if (i == t) up[i] += tail;
      }
    }
  }
  const int n_sym = counts[0], n_nonsym = counts[1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* Pp = pose + b * 12;
  const float P[9] = {Pp[0], Pp[1], Pp[2], Pp[4], Pp[5], Pp[6], Pp[8], Pp[9], Pp[10]};
  const float t[3] = {Pp[3], Pp[7], Pp[11]};
  const float* G = gt_rot + b * 9;
  float dR[9], ds[3];
  float dtp[3] = {0.f, 0.f, 0.f};  // the PM terms' gradient of t: every form but R-only has one
#pragma unroll
  for (int e = 0; e < 9; ++e) dR[e] = 0.f;
  ds[0] = ds[1] = ds[2] = 0.f;
  if (cfg.base.pm_on) {
    float C[9];
    sym_candidate(G, cands + ((size_t)b * S1 + best[b]) * 9, C);
    float se[3], sg[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      se[j] = cfg.base.pm_with_scale ? scale[b * 3 + j] : 1.f;
      sg[j] = cfg.base.pm_with_scale ? gt_scale[b * 3 + j] : 1.f;
    }
    if (pm_shipped(cfg)) {  // (as it always was)
    const float c = up[0] * 3.f * cfg.base.pm_lw / ((float)B * M * 3.f);
    for (int m = tid; m < M; m += 256) {
      const float* q = kps + ((size_t)b * M + m) * 3;
      const float pe[3] = {q[0] * se[0], q[1] * se[1], q[2] * se[2]}, pt[3] = {q[0] * sg[0], q[1] * sg[1], q[2] * sg[2]};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float e = P[i * 3] * pe[0] + P[i * 3 + 1] * pe[1] + P[i * 3 + 2] * pe[2];
        const float g = C[i * 3] * pt[0] + C[i * 3 + 1] * pt[1] + C[i * 3 + 2] * pt[2];
        const float d = e - g;
        const float sgn = d > 0.f ? c : (d < 0.f ? -c : 0.f);  // torch: sign(0) = 0
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          dR[i * 3 + j] = fmaf(sgn, pe[j], dR[i * 3 + j]);
          ds[j] = fmaf(sgn * P[i * 3 + j], q[j], ds[j]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) dR[e] = block_sum256(dR[e], red);
#pragma unroll
    for (int j = 0; j < 3; ++j) ds[j] = cfg.base.pm_with_scale ? block_sum256(ds[j], red) : 0.f;
    } else {
      // every other form (the forward's general loop, differentiated): term 0 reaches R, the scale and - in the R+t form -
      // t; the point forms of terms 1 and 2 reach only the translation components they did not replace
      const int mode = cfg.pm_mode, elem = cfg.pm_elem;
      const float beta = cfg.pm_beta;
      const bool l2 = elem == CATRE_PM_ELEM_L2, pts_t = pm_points_t(mode);
      const float tg[3] = {gt_trans[b * 3], gt_trans[b * 3 + 1], gt_trans[b * 3 + 2]};
      float inv0 = 0.f, inv1 = 0.f, inv2 = 0.f;
      if (l2) {  // L2Loss: d norm / d d_i = d_i / norm - the object's norms once more (the forward keeps only their means)
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int m = tid; m < M; m += 256) {
          float q[3];
          pm_point(kps, cfg.pm_use_bbox, b, M, m, q);
          const float pe[3] = {q[0] * se[0], q[1] * se[1], q[2] * se[2]}, pt[3] = {q[0] * sg[0], q[1] * sg[1], q[2] * sg[2]};
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const float e = P[i * 3] * pe[0] + P[i * 3 + 1] * pe[1] + P[i * 3 + 2] * pe[2];
            const float g = C[i * 3] * pt[0] + C[i * 3 + 1] * pt[1] + C[i * 3 + 2] * pt[2];
            float d0, d1, d2;
            pm_diffs(mode, i, e, g, t[i], tg[i], d0, d1, d2);
            a0 += d0 * d0;
            a1 += d1 * d1;
            a2 += d2 * d2;
          }
        }
        a0 = block_sum256(a0, red);
        inv0 = a0 > 0.f ? 1.f / sqrtf(a0) : 0.f;
        if (pts_t) {
          a1 = block_sum256(a1, red);
          a2 = block_sum256(a2, red);
          inv1 = a1 > 0.f ? 1.f / sqrtf(a1) : 0.f;
          inv2 = a2 > 0.f ? 1.f / sqrtf(a2) : 0.f;
        }
      }
      const float den = l2 ? (float)B : (float)B * M * 3.f;
      const float c0 = up[0] * 3.f * cfg.base.pm_lw / den;
      const float c1 = pts_t ? up[6] * 3.f * cfg.base.pm_lw / den : 0.f;
      const float c2 = mode == CATRE_PM_R_XY_Z_POINTS ? up[7] * 3.f * cfg.base.pm_lw / den : 0.f;
      for (int m = tid; m < M; m += 256) {
        float q[3];
        pm_point(kps, cfg.pm_use_bbox, b, M, m, q);
        const float pe[3] = {q[0] * se[0], q[1] * se[1], q[2] * se[2]}, pt[3] = {q[0] * sg[0], q[1] * sg[1], q[2] * sg[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float e = P[i * 3] * pe[0] + P[i * 3 + 1] * pe[1] + P[i * 3 + 2] * pe[2];
          const float g = C[i * 3] * pt[0] + C[i * 3 + 1] * pt[1] + C[i * 3 + 2] * pt[2];
          float d0, d1, d2;
          pm_diffs(mode, i, e, g, t[i], tg[i], d0, d1, d2);
          const float w0 = c0 * pm_elem_grad(d0, elem, beta, inv0);
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            dR[i * 3 + j] = fmaf(w0, pe[j], dR[i * 3 + j]);
            ds[j] = fmaf(w0 * P[i * 3 + j], q[j], ds[j]);
          }
          // d1 / d2 of a replaced component is an exact zero and every element loss has derivative 0 there
          float wt = mode == CATRE_PM_RT ? w0 : 0.f;
          wt += c1 * pm_elem_grad(d1, elem, beta, inv1) + c2 * pm_elem_grad(d2, elem, beta, inv2);
          dtp[i] += wt;
        }
      }
#pragma unroll
      for (int e = 0; e < 9; ++e) dR[e] = block_sum256(dR[e], red);
#pragma unroll
      for (int j = 0; j < 3; ++j) ds[j] = cfg.base.pm_with_scale ? block_sum256(ds[j], red) : 0.f;
      if (mode == CATRE_PM_RT || pts_t) {
#pragma unroll
        for (int i = 0; i < 3; ++i) dtp[i] = block_sum256(dtp[i], red);
      } else if (mode == CATRE_PM_R_T_DIRECT || mode == CATRE_PM_R_XY_Z_DIRECT) {
        // the `_noP` terms: plain means of the element loss over [B,3] / [B,2] and [B] (l2: norms over 3 / 2 and 1 numbers)
        const float d[3] = {t[0] - tg[0], t[1] - tg[1], t[2] - tg[2]};
        const bool xyz = mode == CATRE_PM_R_T_DIRECT;
        const float n01 = xyz ? d[0] * d[0] + d[1] * d[1] + d[2] * d[2] : d[0] * d[0] + d[1] * d[1];
        const float i01 = n01 > 0.f ? 1.f / sqrtf(n01) : 0.f, i2 = xyz ? i01 : (d[2] != 0.f ? 1.f / fabsf(d[2]) : 0.f);
        const float cA = up[6] / (l2 ? (float)B : (float)B * (xyz ? 3.f : 2.f)), cB = xyz ? cA : up[7] / (float)B;
        dtp[0] = cA * pm_elem_grad(d[0], elem, beta, i01);
        dtp[1] = cA * pm_elem_grad(d[1], elem, beta, i01);
        dtp[2] = cB * pm_elem_grad(d[2], elem, beta, i2);
      }
    }
  }
  if (tid != 0) return;
  float dt[3] = {0.f, 0.f, 0.f};
  if (cfg.base.rot_on) {
    if (!is_sym[b]) {
      if (n_nonsym > 0) {
        if (cfg.base.rot_l2) {
          const float c = up[1] * cfg.base.rot_lw * 2.f / ((float)n_nonsym * 9.f);
#pragma unroll
          for (int e = 0; e < 9; ++e) dR[e] += c * (P[e] - G[e]);
        } else {
          const float c = -up[1] * cfg.base.rot_lw / (4.f * (float)n_nonsym);
#pragma unroll
          for (int e = 0; e < 9; ++e) dR[e] += c * G[e];
        }
      }
    } else if (n_sym > 0 && cfg.base.yaxis_smooth >= 2) {
      const float c = up[2] * cfg.base.rot_lw / (float)n_sym;
      float dd = 0.f, pg = 0.f, pp = 0.f, gg = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float p = P[i * 3 + 1], g = G[i * 3 + 1];
        dd += (p - g) * (p - g);
        pg += p * g;
        pp += p * p;
        gg += g * g;
      }
      if (cfg.base.yaxis_smooth == 2) {
        const float nrm = sqrtf(dd);
#pragma unroll
        for (int i = 0; i < 3; ++i) dR[i * 3 + 1] += nrm > 0.f ? c * (P[i * 3 + 1] - G[i * 3 + 1]) / nrm : 0.f;
      } else {
        const float np_ = sqrtf(pp), ng = sqrtf(gg), cs = pg / (np_ * ng);
#pragma unroll
        for (int i = 0; i < 3; ++i) dR[i * 3 + 1] += -0.5f * c * (G[i * 3 + 1] / (np_ * ng) - cs * P[i * 3 + 1] / pp);
      }
    } else if (n_sym > 0) {
      const float c = up[2] * cfg.base.rot_lw / ((float)n_sym * 3.f);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float d = P[i * 3 + 1] - G[i * 3 + 1];
        float gd;
        if (cfg.base.yaxis_smooth)
          gd = fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f);
        else
          gd = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        dR[i * 3 + 1] += c * gd;
      }
    }
  }
  if (cfg.base.trans_on) {
    const float d[3] = {t[0] - gt_trans[b * 3], t[1] - gt_trans[b * 3 + 1], t[2] - gt_trans[b * 3 + 2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float sg = d[i] > 0.f ? 1.f : (d[i] < 0.f ? -1.f : 0.f);
      float gd = cfg.base.trans_mse == 1 ? 2.f * d[i] : sg;
      float c;
      if (cfg.base.trans_mse == 2) {  // d ||d|| / d d_i = d_i / ||d|| over the components the norm spans
        const bool in_norm = !cfg.base.trans_split || i < 2;
        const float nrm = sqrtf(cfg.base.trans_split ? d[0] * d[0] + d[1] * d[1] : d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        gd = in_norm ? (nrm > 0.f ? d[i] / nrm : 0.f) : sg;
        c = (in_norm ? up[3] : up[4]) * cfg.base.trans_lw / (float)B;
      } else if (cfg.base.trans_split) {
        c = i < 2 ? up[3] * cfg.base.trans_lw / ((float)B * 2.f) : up[4] * cfg.base.trans_lw / (float)B;
      } else {
        c = up[3] * cfg.base.trans_lw / ((float)B * 3.f);
      }
      dt[i] = c * gd;
    }
  }
  if (cfg.base.scale_on) {
    const float c = up[5] * cfg.base.scale_lw / ((float)B * (cfg.base.scale_mse == 2 ? 1.f : 3.f));
    const float d3[3] = {scale[b * 3] - gt_scale[b * 3], scale[b * 3 + 1] - gt_scale[b * 3 + 1],
                         scale[b * 3 + 2] - gt_scale[b * 3 + 2]};
    const float nrm = sqrtf(d3[0] * d3[0] + d3[1] * d3[1] + d3[2] * d3[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float d = d3[i];
      ds[i] += c * (cfg.base.scale_mse == 2 ? (nrm > 0.f ? d / nrm : 0.f)
                                       : cfg.base.scale_mse == 1 ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)));
    }
  }
  float* o = dpose + b * 12;
  const bool pm_t = cfg.base.pm_on && cfg.pm_mode != CATRE_PM_R_ONLY;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o[i * 4] = dR[i * 3];
    o[i * 4 + 1] = dR[i * 3 + 1];
    o[i * 4 + 2] = dR[i * 3 + 2];
    o[i * 4 + 3] = pm_t ? dt[i] + dtp[i] : dt[i];  // (R only: dt as it is, a -0 stays a -0)
  }
  dscale[b * 3] = ds[0];
  dscale[b * 3 + 1] = ds[1];
  dscale[b * 3 + 2] = ds[2];
}
