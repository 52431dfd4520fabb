// catre_pclf.h - SURVEY.md row f3 for a whole data batch: the kernels of catre_pcl.h with a frame per instance, and
// the depth augmentation the loader applies before any cloud is cut (INPUT.AUG_DEPTH).
//
// Frame batch.  Instance i reads depth + frame_of[i] * H * W, the camera cams[frame_of[i]] and the sampling seed
// seeds[frame_of[i]]; grid and work split are those of the single-frame kernels (per (instance, 4096-pixel chunk)).
// The per-pixel arithmetic is NOT restated: every kernel here calls pcl_point / pcl_radii / pcl_bin / pcl_perm /
// pcl_pdist of catre_pcl.h on the frame's own depth pointer and camera, k_pcl_pick is launched as it is, so a frame
// gives the bits the single-frame kernels give.  The pixel-membership test has a second form next to the byte mask:
// labels[frame][pix] == label_of[inst] on one label image per frame (uint8 or int32).
//   k_pclf_count   = k_pcl_count   with a frame per instance
//   k_pclf_compact = k_pcl_compact with a frame per instance
//   k_pclf_gather  = k_pcl_gather; the keyed permutation is keyed by (seed of the frame, rank of the instance within
//                    its frame), so a frame gets the cloud it gets alone whatever else is in the batch
//   k_pclf_fps     = k_pcl_fps     with a frame per instance
// The tables (frame_of, rank_of, label_of, cams, seeds) are validated on the host and staged by the entry points
// (catre_pclf_api.inc); the kernels that read a frame index from device memory still refuse one outside [0, F).
#pragma once
#include "catre_pcl.h"

// MODE 0: byte masks [I,H,W] (or none); MODE 1: label images [F,H,W] of LT + label_of [I]
template <int MODE, typename LT>
__device__ __forceinline__ int pclf_bin(const float* __restrict__ depth_f, const unsigned char* __restrict__ mask_i,
                                        const LT* __restrict__ labels_f, int label, int pix, int W, const PclCam& cam,
                                        const float* centre, const float (&r)[PCL_NR], int use_ball) {
  if (MODE == 1) {
    if ((int)labels_f[pix] != label) return -1;
    return pcl_bin(depth_f, nullptr, pix, W, cam, centre, r, use_ball);
  }
  return pcl_bin(depth_f, mask_i, pix, W, cam, centre, r, use_ball);
}

template <int MODE, typename LT>
__global__ __launch_bounds__(256) void k_pclf_count(const float* __restrict__ depth, const unsigned char* __restrict__ masks,
                                                    const LT* __restrict__ labels, const int* __restrict__ frame_of,
                                                    const int* __restrict__ label_of, const PclCam* __restrict__ cams,
                                                    const float* __restrict__ poses, const float* __restrict__ scales,
                                                    float ratio, int use_ball, int H, int W, int nchunks,
                                                    int* __restrict__ bins /*[I][nchunks][12]*/) {
  __shared__ int cnt[12];
  const int inst = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  if (tid < 12) cnt[tid] = 0;
  __syncthreads();
  const int HW = H * W, frame = frame_of[inst];
  const PclCam cam = cams[frame];
  const float* depth_f = depth + (size_t)frame * HW;
  const unsigned char* m = (MODE == 0 && masks) ? masks + (size_t)inst * HW : nullptr;
  const LT* lab_f = MODE == 1 ? labels + (size_t)frame * HW : nullptr;
  const int label = MODE == 1 ? label_of[inst] : 0;
  float r[PCL_NR];
  pcl_radii(poses + inst * 12, scales + inst * 3, ratio, r);
  const float centre[3] = {poses[inst * 12 + 3], poses[inst * 12 + 7], poses[inst * 12 + 11]};
  const int p0 = chunk * PCL_CHUNK + tid * 16;
  int local[PCL_NR + 1];
#pragma unroll
  for (int i = 0; i <= PCL_NR; ++i) local[i] = 0;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int pix = p0 + k;
    if (pix < HW) {
      const int b = pclf_bin<MODE, LT>(depth_f, m, lab_f, label, pix, W, cam, centre, r, use_ball);
#pragma unroll
      for (int i = 0; i <= PCL_NR; ++i) local[i] += (b == i);
    }
  }
#pragma unroll
  for (int i = 0; i <= PCL_NR; ++i)
    if (local[i]) atomicAdd(&cnt[i], local[i]);
  __syncthreads();
  if (tid < 12) bins[((size_t)inst * nchunks + chunk) * 12 + tid] = tid <= PCL_NR ? cnt[tid] : 0;
}

template <int MODE, typename LT>
__global__ __launch_bounds__(256) void k_pclf_compact(const float* __restrict__ depth,
                                                      const unsigned char* __restrict__ masks,
                                                      const LT* __restrict__ labels, const int* __restrict__ frame_of,
                                                      const int* __restrict__ label_of, const PclCam* __restrict__ cams,
                                                      const float* __restrict__ poses, const float* __restrict__ scales,
                                                      float ratio, int use_ball, int H, int W, int nchunks,
                                                      const int* __restrict__ choose, const int* __restrict__ offsets,
                                                      int* __restrict__ cand /*[I][H*W]*/) {
  __shared__ int wsum[4];
  const int inst = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W, frame = frame_of[inst];
  const PclCam cam = cams[frame];
  const float* depth_f = depth + (size_t)frame * HW;
  const unsigned char* m = (MODE == 0 && masks) ? masks + (size_t)inst * HW : nullptr;
  const LT* lab_f = MODE == 1 ? labels + (size_t)frame * HW : nullptr;
  const int label = MODE == 1 ? label_of[inst] : 0;
  float r[PCL_NR];
  pcl_radii(poses + inst * 12, scales + inst * 3, ratio, r);
  const float centre[3] = {poses[inst * 12 + 3], poses[inst * 12 + 7], poses[inst * 12 + 11]};
  const int k = choose[inst];
  const int p0 = chunk * PCL_CHUNK + tid * 16;
  unsigned keep = 0;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int pix = p0 + j;
    if (pix < HW) {
      const int b = pclf_bin<MODE, LT>(depth_f, m, lab_f, label, pix, W, cam, centre, r, use_ball);
      if (b >= 0 && b <= k) keep |= 1u << j;
    }
  }
  const int mine = __popc(keep);
  // exclusive scan over the 256 threads (thread order = pixel order)
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = offsets[(size_t)inst * nchunks + chunk];
  for (int w = 0; w < wave; ++w) base += wsum[w];
  int pos = base + incl - mine;
  int* out = cand + (size_t)inst * HW;
#pragma unroll 4
  for (int j = 0; j < 16; ++j)
    if (keep & (1u << j)) out[pos++] = p0 + j;
}

// candidate count of an instance as the sampling kernels may trust it: the workspace is the caller's memory, so a count
// or a frame index that candidates() did not write there (a workspace used out of order) selects nothing instead of
// reading outside the depth maps
__device__ __forceinline__ int pclf_count_ok(int cnt, int frame, int F, int HW) {
  return ((unsigned)frame < (unsigned)F && cnt > 0 && cnt <= HW) ? cnt : 0;
}

__global__ __launch_bounds__(256) void k_pclf_gather(const float* __restrict__ depth, const int* __restrict__ frame_of,
                                                     const int* __restrict__ rank_of, const PclCam* __restrict__ cams,
                                                     const unsigned long long* __restrict__ seeds, int F, int H, int W,
                                                     const int* __restrict__ cand, const int* __restrict__ total,
                                                     const long long* __restrict__ sample /*[I][N] or null*/, int N,
                                                     float* __restrict__ pcl_out, int* __restrict__ pix_out) {
  const int inst = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int HW = H * W, frame = frame_of[inst];
  const int cnt = pclf_count_ok(total[inst], frame, F, HW);
  float x = 0.f, y = 0.f, z = 0.f;
  int pix = -1;
  if (cnt > 0) {
    unsigned L = (unsigned)cnt;  // `while len(idx) < num_points: idx = cat([idx, idx])` -> idx tiled to length L
    while (L < (unsigned)N) L <<= 1;
    const unsigned j =
        sample ? (unsigned)sample[(size_t)inst * N + i] : pcl_perm((unsigned)i, L, seeds[frame], (unsigned)rank_of[inst]);
    pix = cand[(size_t)inst * HW + (j % (unsigned)cnt)];
    if ((unsigned)pix < (unsigned)HW) {
      const PclCam cam = cams[frame];
      pcl_point(depth + (size_t)frame * HW, pix, W, cam, x, y, z);
    } else {
      pix = -1;
    }
  }
  float* o = pcl_out + ((size_t)inst * N + i) * 3;
  o[0] = x;
  o[1] = y;
  o[2] = z;
  if (pix_out) pix_out[(size_t)inst * N + i] = pix;
}

// k_pcl_fps with a frame per instance (see there for the algorithm and the reference lines)
__global__ __launch_bounds__(1024) void k_pclf_fps(const float* __restrict__ depth, const int* __restrict__ frame_of,
                                                   const PclCam* __restrict__ cams, int F, int H, int W,
                                                   const int* __restrict__ cand, const int* __restrict__ total, int N,
                                                   float* __restrict__ scratch, int Lcap,
                                                   long long* __restrict__ sample_out) {
  __shared__ float red_v[16];
  __shared__ int red_i[16];
  __shared__ float red_s[3][16];
  __shared__ float cen[3];
  const int inst = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W, frame = frame_of[inst];
  const int cnt = pclf_count_ok(total[inst], frame, F, HW);
  long long* out = sample_out + (size_t)inst * N;
  unsigned L = cnt > 0 ? (unsigned)cnt : 0u;
  while (L && L < (unsigned)N) L <<= 1;
  if (L == 0 || (unsigned)N >= L || L > (unsigned)Lcap) {  // nothing to choose from / everything is chosen
    for (int i = tid; i < N; i += 1024) out[i] = L ? (long long)((unsigned)i % L) : 0;
    return;
  }
  const PclCam cam = cams[frame];
  const float* depth_f = depth + (size_t)frame * HW;
  float* px = scratch + (size_t)inst * 4 * Lcap;
  float* py = px + Lcap;
  float* pz = py + Lcap;
  float* dist = pz + Lcap;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (unsigned j = tid; j < L; j += 1024) {
    float x = 0.f, y = 0.f, z = 0.f;
    const int pix = cand[(size_t)inst * HW + (j % (unsigned)cnt)];
    if ((unsigned)pix < (unsigned)HW) pcl_point(depth_f, pix, W, cam, x, y, z);
    px[j] = x;
    py[j] = y;
    pz[j] = z;
    sx += x;
    sy += y;
    sz += z;
  }
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  sz = wave_sum(sz);
  if (lane == 0) {
    red_s[0][wave] = sx;
    red_s[1][wave] = sy;
    red_s[2][wave] = sz;
  }
  __syncthreads();
  if (tid < 3) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red_s[tid][w];
    cen[tid] = t / (float)L;
  }
  __syncthreads();
  {
    const float cx = cen[0], cy = cen[1], cz = cen[2];
    for (unsigned j = tid; j < L; j += 1024) dist[j] = pcl_pdist(cx, cy, cz, px[j], py[j], pz[j]);
  }
  for (int it = 0; it < N; ++it) {
    // arg-max with "first maximum wins": per thread in increasing j, then (value, index) pairs
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (unsigned j = tid; j < L; j += 1024) {
      const float v = dist[j];
      if (v > bv) {
        bv = v;
        bi = (int)j;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      red_v[wave] = bv;
      red_i[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      float v = red_v[0];
      int i = red_i[0];
      for (int w = 1; w < 16; ++w)
        if (red_v[w] > v || (red_v[w] == v && red_i[w] < i)) {
          v = red_v[w];
          i = red_i[w];
        }
      if ((unsigned)i >= L) i = 0;  // every distance NaN (non-finite depth): no maximum was found
      out[it] = i;
      cen[0] = px[i];
      cen[1] = py[i];
      cen[2] = pz[i];
    }
    __syncthreads();
    const float cx = cen[0], cy = cen[1], cz = cen[2];
    for (unsigned j = tid; j < L; j += 1024) dist[j] = fminf(dist[j], pcl_pdist(cx, cy, cz, px[j], py[j], pz[j]));
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// INPUT.AUG_DEPTH: what the loader does to the depth map before any cloud is cut from it
// (core/catre/datasets/data_loader.py:530-543, core/utils/depth_aug.py:5-23), in the loader's order:
//   1. fill   a pixel with depth == 0 becomes a draw from N(0, 0.1).  The reference writes
//             np.random.normal(np.median(depth[zeros]), 0.1): the median of a set of zeros is 0.  A negative fill stays
//             negative and is dropped later by the `depth > 0` test of the sampling, as in the reference.
//   2. drop   depth *= (u > drop_ratio), u ~ U(0,1)   (a product, so a dropped negative fill is -0.0 as in numpy)
//   3. noise  where depth > 0 after 1 and 2: depth += noise_level * g, g ~ N(0,1), one noise_level per frame
// One thread per pixel, blockIdx.y = frame.  Input fp32 metres or uint16 millimetres ((float)v / depth_div with an IEEE
// division = depth.astype("float32") / 1000.0); output fp32.
// Draws mode (DRAWS): the caller passes the reference's float64 draws [F,H,W]; a step whose array is null is off.  The
//   arithmetic is numpy's - float64 where numpy promotes, one rounding to fp32 on assignment - with the product and the sum
//   rounded separately, so the result is the reference's bit for bit.
// Device mode: Philox4x32-10 evaluated at counter (pixel, step, frame_key) under key (seed): nothing depends on launch
//   geometry, on F or on the frame's slot in the batch.  Uniforms are taken from (0,1], normals by Box-Muller; fp32.
// ------------------------------------------------------------------------------------------------
#define DAUG_FILL 1
#define DAUG_DROP 2
#define DAUG_NOISE 4

struct DaugFrame {  // = catre_depth_aug_frame
  double drop_ratio, noise_level;
  unsigned long long key;
  int flags, reserved;
};

struct DaugRand {
  unsigned v[4];
};
__device__ __forceinline__ DaugRand daug_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                unsigned k1) {
#pragma unroll
  for (int rd = 0; rd < 10; ++rd) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return DaugRand{{c0, c1, c2, c3}};
}
__device__ __forceinline__ float daug_uniform(unsigned x) { return (float)((x >> 8) + 1u) * (1.f / 16777216.f); }  // (0,1]
__device__ __forceinline__ float daug_normal(unsigned a, unsigned b) {
  const float rad = sqrtf(-2.f * __logf(daug_uniform(a)));
  return rad * __cosf(6.28318530717958647692f * daug_uniform(b));
}

// numpy's `depth[mask] + gauss[mask]` with gauss = noise_level * randn: a float64 product, a float64 sum, one rounding to
// fp32 on assignment.  Contraction is off in this block, so the product is rounded before the sum (no fused multiply-add).
__device__ __forceinline__ float daug_noise_f64(float d, double level, double g) {
#pragma clang fp contract(off)
  const double gauss = level * g;
  const double sum = (double)d + gauss;
  return (float)sum;
}

template <typename IT, bool DRAWS>
__global__ __launch_bounds__(256) void k_depth_augment(const IT* __restrict__ in, float depth_div,
                                                       const DaugFrame* __restrict__ frames,
                                                       const double* __restrict__ draw_fill,
                                                       const double* __restrict__ draw_keep,
                                                       const double* __restrict__ draw_gauss, unsigned long long seed,
                                                       int HW, float* __restrict__ out) {
  const int frame = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const DaugFrame fr = frames[frame];
  const size_t at = (size_t)frame * HW + pix;
  float d;
  if (sizeof(IT) == 2)
    d = __fdiv_rn((float)in[at], depth_div);
  else
    d = (float)in[at];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  const unsigned f0 = (unsigned)fr.key, f1 = (unsigned)(fr.key >> 32);
  if (DRAWS) {
    if ((fr.flags & DAUG_FILL) && draw_fill && d == 0.f) d = (float)draw_fill[at];
    if ((fr.flags & DAUG_DROP) && draw_keep) d = __fmul_rn(d, draw_keep[at] > fr.drop_ratio ? 1.f : 0.f);
    if ((fr.flags & DAUG_NOISE) && draw_gauss && d > 0.f)
      d = daug_noise_f64(d, fr.noise_level, draw_gauss[at]);
  } else {
    if ((fr.flags & DAUG_FILL) && d == 0.f) {
      const DaugRand q = daug_philox((unsigned)pix, 0u, f0, f1, k0, k1);
      d = 0.1f * daug_normal(q.v[0], q.v[1]);
    }
    if (fr.flags & DAUG_DROP) {
      const DaugRand q = daug_philox((unsigned)pix, 1u, f0, f1, k0, k1);
      d = __fmul_rn(d, daug_uniform(q.v[0]) > (float)fr.drop_ratio ? 1.f : 0.f);
    }
    if ((fr.flags & DAUG_NOISE) && d > 0.f) {
      const DaugRand q = daug_philox((unsigned)pix, 2u, f0, f1, k0, k1);
      d += (float)fr.noise_level * daug_normal(q.v[0], q.v[1]);
    }
  }
  out[at] = d;
}
