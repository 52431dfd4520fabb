// Tracking support on the device: nearest-neighbour statistics of a batch of point-set pairs (the fit score of a refined
// pose, ADD / ADD-S of lib/pysixd/pose_error.py:256-296) and the gate that decides which pose a track carries on.
//
// k_nn_stats   one workgroup per (instance, tile of NN_THREADS src points), one src point per thread.  The dst points are
//              brought to their pose once per workgroup, NN_CHUNK at a time, into LDS as float4; every lane of a wave then
//              reads the SAME element per step (a broadcast: no bank conflict) against its own src point in registers.
//              8 FLOP per pair (10 VALU instructions as compiled: 3 sub, mul, 2 fma, compare, 2 selects and a move that
//              materialises the index), no matrix form.  Distances are differences first - dx = px - qx, then
//              fmaf(dx,dx, fmaf(dy,dy, dz*dz)) - never |a|^2 + |b|^2 - 2ab, which cancels at the millimetre distances this
//              is used for.  A strict `<` in ascending dst order keeps the lowest index on an exact tie.
//              The running minimum starts at dst point 0, so a NaN src point (or a NaN dst point 0) stays NaN and reaches
//              mean_d; a NaN dst point further on never compares below and is never a neighbour.  No special case.
// k_nn_finish  one thread per instance adds the tile partials in tile order.
// The reduction over src points is a fixed tree: xor butterfly in the wave, the four waves in order, the tiles in order,
// accumulated in double (the distances themselves are fp32).  The tiling depends on n_src only, so an instance gives the
// same bits alone and inside any batch.  No floating-point atomics.
// k_track_gate one thread per instance: status bits, carried pose / scale, age.
#pragma once
#include "catre_device.h"
#include "catre_host.h"

constexpr int NN_THREADS = 256;  // src points per workgroup
constexpr int NN_CHUNK = 1024;   // dst points staged in LDS at a time (16 KiB as float4)

constexpr int TRACK_EMPTY = CATRE_TRACK_EMPTY, TRACK_LOW_FIT = CATRE_TRACK_LOW_FIT, TRACK_NONFINITE = CATRE_TRACK_NONFINITE;

// point n of a cloud at (pose, scale): R (s * x) + t, the prior branch of pose_apply_point; NULL = identity
__device__ __forceinline__ void nn_load_point(const float* __restrict__ pts, size_t n, const float* __restrict__ pose,
                                              const float* __restrict__ scale, float& x, float& y, float& z) {
  const float* s = pts + n * 3;
  x = s[0];
  y = s[1];
  z = s[2];
  if (scale) {
    x *= scale[0];
    y *= scale[1];
    z *= scale[2];
  }
  if (pose) {
    const float ox = fmaf(pose[2], z, fmaf(pose[1], y, pose[0] * x)) + pose[3];
    const float oy = fmaf(pose[6], z, fmaf(pose[5], y, pose[4] * x)) + pose[7];
    const float oz = fmaf(pose[10], z, fmaf(pose[9], y, pose[8] * x)) + pose[11];
    x = ox;
    y = oy;
    z = oz;
  }
}

__device__ __forceinline__ float nn_dist2(float px, float py, float pz, float qx, float qy, float qz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}

__global__ __launch_bounds__(NN_THREADS) void k_nn_stats(const float* __restrict__ src, int n_src,
                                                         const float* __restrict__ dst, int n_dst,
                                                         const float* __restrict__ src_pose,
                                                         const float* __restrict__ src_scale,
                                                         const float* __restrict__ dst_pose,
                                                         const float* __restrict__ dst_scale, int paired,
                                                         const float* __restrict__ tau, int tiles,
                                                         float* __restrict__ nn_d, int32_t* __restrict__ nn_j,
                                                         double* __restrict__ psum, int32_t* __restrict__ pcnt) {
  __shared__ f32x4 sd[NN_CHUNK];
  __shared__ double rs[NN_THREADS / 64];
  __shared__ int rc[NN_THREADS / 64];
  const int tid = threadIdx.x;
  const int inst = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int n = tile * NN_THREADS + tid;
  const bool live = n < n_src;
  const int nc = live ? n : n_src - 1;  // idle lanes repeat the last point: every thread reaches every barrier
  const float* sp = src_pose ? src_pose + (size_t)inst * 12 : nullptr;
  const float* ss = src_scale ? src_scale + (size_t)inst * 3 : nullptr;
  const float* dp = dst_pose ? dst_pose + (size_t)inst * 12 : nullptr;
  const float* ds = dst_scale ? dst_scale + (size_t)inst * 3 : nullptr;
  const size_t s0 = (size_t)inst * n_src, d0 = (size_t)inst * n_dst;
  float px, py, pz;
  nn_load_point(src, s0 + nc, sp, ss, px, py, pz);
  float best;
  int bj;
  {
    float qx, qy, qz;
    bj = paired ? nc : 0;
    nn_load_point(dst, d0 + bj, dp, ds, qx, qy, qz);
    best = nn_dist2(px, py, pz, qx, qy, qz);
  }
  if (!paired) {
    for (int c0 = 0; c0 < n_dst; c0 += NN_CHUNK) {
      const int cnt = min(NN_CHUNK, n_dst - c0);
      if (c0) __syncthreads();  // the previous chunk has been read by every wave
      for (int k = tid; k < cnt; k += NN_THREADS) {
        float qx, qy, qz;
        nn_load_point(dst, d0 + c0 + k, dp, ds, qx, qy, qz);
        sd[k] = f32x4{qx, qy, qz, 0.f};
      }
      __syncthreads();
#pragma unroll 8
      for (int j = 0; j < cnt; ++j) {
        const f32x4 q = sd[j];
        const float d = nn_dist2(px, py, pz, q[0], q[1], q[2]);
        if (d < best) {
          best = d;
          bj = c0 + j;
        }
      }
    }
  }
  if (live) {
    if (nn_d) nn_d[s0 + n] = best;
    if (nn_j) nn_j[s0 + n] = bj;
  }
  double s = live ? (double)sqrtf(best) : 0.0;
  int c = 0;
  if (tau) {
    const float t = tau[inst];
    c = (live && best <= __fmul_rn(t, t)) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    c += __shfl_xor(c, o);
  }
  if ((tid & 63) == 0) {
    rs[tid >> 6] = s;
    rc[tid >> 6] = c;
  }
  __syncthreads();
  if (tid == 0) {
    psum[blockIdx.x] = ((rs[0] + rs[1]) + rs[2]) + rs[3];
    pcnt[blockIdx.x] = rc[0] + rc[1] + rc[2] + rc[3];
  }
}

__global__ void k_nn_finish(const double* __restrict__ psum, const int32_t* __restrict__ pcnt, int tiles, int n_src, int I,
                            float* __restrict__ mean_d, float* __restrict__ inlier) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  double s = 0.0;
  int c = 0;
  for (int t = 0; t < tiles; ++t) {
    s += psum[(size_t)i * tiles + t];
    c += pcnt[(size_t)i * tiles + t];
  }
  mean_d[i] = (float)(s / (double)n_src);
  if (inlier) inlier[i] = (float)((double)c / (double)n_src);
}

__device__ __forceinline__ bool track_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN and inf

__global__ void k_track_gate(const float* __restrict__ pose_new, const float* __restrict__ scale_new,
                             const float* __restrict__ pose_prev, const float* __restrict__ scale_prev,
                             const int32_t* __restrict__ counts, const float* __restrict__ inlier,
                             const float* __restrict__ mean_d, float min_inlier, int hold, int I,
                             float* __restrict__ pose_out, float* __restrict__ scale_out, int32_t* __restrict__ status,
                             int32_t* __restrict__ age) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  float pn[12], sn[3];
  bool fin = track_finite(inlier[i]) && track_finite(mean_d[i]);
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    pn[k] = pose_new[(size_t)i * 12 + k];
    fin = fin && track_finite(pn[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    sn[k] = scale_new[(size_t)i * 3 + k];
    fin = fin && track_finite(sn[k]);
  }
  int st = 0;
  if (counts[i] == 0) st |= TRACK_EMPTY;
  if (inlier[i] < min_inlier) st |= TRACK_LOW_FIT;
  if (!fin) st |= TRACK_NONFINITE;
  const bool keep_prev = st != 0 && (hold || (st & TRACK_NONFINITE));
#pragma unroll
  for (int k = 0; k < 12; ++k) pose_out[(size_t)i * 12 + k] = keep_prev ? pose_prev[(size_t)i * 12 + k] : pn[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) scale_out[(size_t)i * 3 + k] = keep_prev ? scale_prev[(size_t)i * 3 + k] : sn[k];
  status[i] = st;
  age[i] = st ? age[i] + 1 : 0;
}


// ---- host side: grid and workspace sizing of catre_nn_stats, shared by its ABI (catre_track_api.inc) and the ICP ABI
// (catre_icp_api.inc), which runs the same neighbour search
namespace {
inline int nn_tiles(int n_src) { return (n_src + NN_THREADS - 1) / NN_THREADS; }
// one launch covers every (instance, tile): I * tiles workgroups of NN_THREADS threads, kept below 2^32 threads in all
constexpr size_t NN_MAX_GROUPS = ((size_t)1 << 32) / NN_THREADS - 1;
inline bool nn_dims_ok(int I, int n_src, int n_dst) {
  return I > 0 && n_src > 0 && n_dst > 0 && (size_t)n_src * 3 < ((size_t)1 << 31) && (size_t)n_dst * 3 < ((size_t)1 << 31) &&
         (size_t)I * nn_tiles(n_src) <= NN_MAX_GROUPS;
}
// [I * tiles] double partial sums, then [I * tiles] int32 partial counts
inline size_t nn_ws_bytes(int I, int n_src) { return catre_host::align_up((size_t)I * nn_tiles(n_src) * 12, 16); }
}  // namespace
