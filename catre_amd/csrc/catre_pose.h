// catre_pose.h - the tail of a refine iteration: the rotation heads' final sum, a10-a12 (rotation parameters -> R, pose and
// scale update), get_rot_mat as a stand-alone launch, and the stand-alone channel-wise max-pool.
#pragma once
#include "catre_device.h"
#include "catre_so3.h"

// rot[b][hd*rd+c] = sum_tiles rpart + neck_b[c] * sum_p w_p + conv_p.bias   (rd = RotHead.rot_dim: 3 for rot6d, 2 for quat)
__global__ void k_rot_finish(const float* __restrict__ rpart, const float* __restrict__ neckbx,
                             const float* __restrict__ neckby, const float* __restrict__ sumwp /*[2]*/,
                             const float* __restrict__ cpbx, const float* __restrict__ cpby, float* __restrict__ rot6d,
                             int B, int T, int rd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 2 * rd) return;
  const int b = i / (2 * rd), hd = (i % (2 * rd)) / rd, c = i % rd;
  const float* rp = rpart + ((size_t)b * 2 + hd) * T * 4 + c;
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += rp[t * 4];
  const float nb = (hd ? neckby : neckbx)[c];
  const float* cpb = hd ? cpby : cpbx;
  s = fmaf(nb, sumwp[hd], s);
  if (cpb) s += cpb[0];
  rot6d[i] = s;
}

// get_rot_mat as a stand-alone launch: rot [B,d] -> R [B,3,3]; and its backward gR [B,3,3] -> g [B,d]
__global__ void k_rot_to_mat(const float* __restrict__ rot, int rot_type, float* __restrict__ R, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int d = catre_rot_dim(rot_type);
  float r[6], m[9];
#pragma unroll
  for (int i = 0; i < 6; ++i) r[i] = i < d ? rot[(size_t)b * d + i] : 0.f;  // fixed trip count: r stays in registers
  rot_param_to_mat(r, rot_type, m);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[(size_t)b * 9 + i] = m[i];
}

__global__ void k_rot_to_mat_bwd(const float* __restrict__ rot, int rot_type, const float* __restrict__ gR,
                                 float* __restrict__ g, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int d = catre_rot_dim(rot_type);
  float r[6], gm[9], go[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 6; ++i) r[i] = i < d ? rot[(size_t)b * d + i] : 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) gm[i] = gR[(size_t)b * 9 + i];
  rot_param_to_mat_bwd(r, rot_type, gm, go);
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (i < d) g[(size_t)b * d + i] = go[i];
}

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void normalize3(float* v) {  // F.normalize(p=2, eps=1e-12)
  const float nrm = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-12f);
  v[0] /= nrm;
  v[1] /= nrm;
  v[2] /= nrm;
}

// one object b; rotp: this object's rotation parameters (catre_rot_dim values, or 9 when rot_input_is_matrix) - global
// memory or LDS (k_finish_update, catre_small.h)
__device__ __forceinline__ void pose_update_obj(const float* rotp, const float* __restrict__ dtr,
                                                const float* __restrict__ dsr, const float* __restrict__ pose0,
                                                const float* __restrict__ scale0, const float* __restrict__ mean_scales,
                                                const float* __restrict__ Ks, const catre_opts& o,
                                                float* __restrict__ pose_out, float* __restrict__ scale_out, int b,
                                                float* __restrict__ pose_echo = nullptr,
                                                float* __restrict__ scale_echo = nullptr) {
  if (pose_echo) {  // catre_refine_k_from: slot 0 of the K-loop's output = the caller's initial estimate, no copy launch
#pragma unroll
    for (int i = 0; i < 12; ++i) pose_echo[b * 12 + i] = pose0[b * 12 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) scale_echo[b * 3 + i] = scale0[b * 3 + i];
  }
  float dR[9];
  if (o.rot_input_is_matrix) {
#pragma unroll
    for (int i = 0; i < 9; ++i) dR[i] = rotp[i];
  } else {  // get_rot_mat, models/model_utils.py:28-40
    const int rd = catre_rot_dim(o.rot_type);
    float r[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) r[i] = i < rd ? rotp[i] : 0.f;
    rot_param_to_mat(r, o.rot_type, dR);
  }

  const float* p0 = pose0 + b * 12;
  const float t0[3] = {p0[3], p0[7], p0[11]};
  float d[3] = {dtr[b * 3] * o.delta_t_weight, dtr[b * 3 + 1] * o.delta_t_weight, dtr[b * 3 + 2] * o.delta_t_weight};
  float t[3];
  if (!o.delta_t_space_3d) {
    const float zsrc = t0[2];
    const float ztgt = o.delta_z_deepim ? zsrc / expf(d[2]) : d[2] * zsrc;
    const float fx = o.k_aware ? Ks[b * 9 + 0] : 1.f, fy = o.k_aware ? Ks[b * 9 + 4] : 1.f;
    t[0] = ztgt * (d[0] / fx + t0[0] / zsrc);
    t[1] = ztgt * (d[1] / fy + t0[1] / zsrc);
    t[2] = ztgt;
  } else {
    t[0] = t0[0] + d[0];
    t[1] = t0[1] + d[1];
    t[2] = t0[2] + d[2];
  }
  const float* sb = o.scale_base_mean ? mean_scales + b * 3 : scale0 + b * 3;
  float s[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) s[i] = o.scale_mul ? sb[i] * expf(dsr[b * 3 + i]) : sb[i] + dsr[b * 3 + i];

  if (o.is_allo) {  // allo_to_ego_mat_torch, core/utils/utils.py:200-231
    const float nrm = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) + o.allo_eps;
    const float ray[3] = {t[0] / nrm, t[1] / nrm, t[2] / nrm};
    const float angle = acosf(ray[2]);
    float ax[3] = {-ray[1], ray[0], 0.f};  // (0,0,1) x ray
    const float an = sqrtf(ax[0] * ax[0] + ax[1] * ax[1]) + o.allo_eps;
    ax[0] /= an;
    ax[1] /= an;
    const float sh = sinf(angle * 0.5f);
    float q[4] = {cosf(angle * 0.5f), ax[0] * sh, ax[1] * sh, 0.f * sh};
    const float qn = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] /= qn;  // quat2mat_torch, core/utils/pose_utils.py:349-412
    const float X = q[1] * 2.f, Y = q[2] * 2.f, Z = q[3] * 2.f;
    const float wX = q[0] * X, wY = q[0] * Y, wZ = q[0] * Z, xX = q[1] * X, xY = q[1] * Y, xZ = q[1] * Z;
    const float yY = q[2] * Y, yZ = q[2] * Z, zZ = q[3] * Z;
    const float A[9] = {1.f - (yY + zZ), xY - wZ, xZ + wY, xY + wZ, 1.f - (xX + zZ), yZ - wX,
                        xZ - wY,         yZ + wX, 1.f - (xX + yY)};
    float E[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) E[i * 3 + j] = A[i * 3] * dR[j] + A[i * 3 + 1] * dR[3 + j] + A[i * 3 + 2] * dR[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) dR[i] = E[i];
  }
  float* po = pose_out + b * 12;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      po[i * 4 + j] = dR[i * 3] * p0[j] + dR[i * 3 + 1] * p0[4 + j] + dR[i * 3 + 2] * p0[8 + j];  // dR @ R0
    po[i * 4 + 3] = t[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) scale_out[b * 3 + i] = o.refine_scale ? s[i] : scale0[b * 3 + i];
}

__global__ void k_pose_update(const float* __restrict__ rot6d, const float* __restrict__ dtr,
                              const float* __restrict__ dsr, const float* __restrict__ pose0,
                              const float* __restrict__ scale0, const float* __restrict__ mean_scales,
                              const float* __restrict__ Ks, catre_opts o, float* __restrict__ pose_out,
                              float* __restrict__ scale_out, int B, float* __restrict__ pose_echo = nullptr,
                              float* __restrict__ scale_echo = nullptr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  pose_update_obj(rot6d + (size_t)b * (o.rot_input_is_matrix ? 9 : catre_rot_dim(o.rot_type)), dtr, dsr, pose0, scale0,
                  mean_scales, Ks, o, pose_out, scale_out, b, pose_echo, scale_echo);
}

// ------------------------------------------------------------------------------------------
// stand-alone channel-wise max-pool [B,C,N] -> [B,C]: one wave per row, float4 streaming loads
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_colmax(const float* __restrict__ x, float* __restrict__ out, int rows,
                                                int N) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int nwaves = gridDim.x * wpb;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < rows; row += nwaves) {
    const float* r = x + (size_t)row * N;
    float m = -INFINITY;
    if ((N & 3) == 0) {
      const f32x4* r4 = reinterpret_cast<const f32x4*>(r);
      const int n4 = N >> 2;
#pragma unroll 4
      for (int i = lane; i < n4; i += 64) {
        const f32x4 v = __builtin_nontemporal_load(r4 + i);
        m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
      }
    } else {
      for (int i = lane; i < N; i += 64) m = fmaxf(m, r[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) out[row] = m;
  }
}
