// Splat render of the posed prior: a z-buffered disc splat of every instance's prior points into the frame the instance is
// seen in -> instance labels, a depth image, the winning point, a visibility class per pixel against an observed depth map
// (the BOP visibility test, lib/pysixd/visibility.py:9-41, with its visible set split in two) and per-point visibility.
//
// k_splat_clear    key image := all ones (background), counts := 0.
// k_splat          one workgroup of four waves per (instance, tile of 4 * ppw points).  The first ppw lanes of a wave project
//                  one point each; the wave then walks its live points one after the other with all 64 lanes spread over the
//                  pixels of the point's bounding box (footprints vary from 0 to (2 r_max + 1)^2 pixels: a thread per point
//                  would diverge by that factor).  ppw (a power of two, 4 .. 64) is the host's choice: 64 for a full grid,
//                  fewer for a handful of objects, whose points then spread over more waves - the walk of a wave is a
//                  chain of load -> compare -> atomic round trips.  The image does not depend on it (integer min).
//                  A covered pixel gets atomicMin of the 64-bit key (bits(z) << 32 | instance << 16 | point) - a single
//                  global_atomic_umin_x2.  Unsigned integer min does not depend on the order of arrival, so the
//                  image is bit-reproducible; z > 0 makes the fp32 bit pattern order like the value.  A plain load in front
//                  of the atomic drops it where the pixel already holds a smaller key: min is monotone, so a stale value
//                  read there only costs an atomic that changes nothing, never a result.
// k_splat_resolve  one thread per pixel: key -> labels / zbuf / point / class; counts by integer atomics after a wave-level
//                  merge of equal (instance, class) codes (integer sums: exact in any order).
// k_splat_visible  one thread per point: is the point the surface at its centre pixel?
// The projection is ONE device function (splat_project) for the splat and the visibility launch: same bits.  Every product,
// quotient and sum in it is spelled with a rounding intrinsic so that nothing is contracted or reordered.
#pragma once
#include "catre_device.h"

#include "../../include/catre_hip.h"
#include "catre_pcl.h"
#include "catre_track.h"

constexpr int SPLAT_THREADS = 256;
constexpr unsigned long long SPLAT_BG = ~0ull;
constexpr int SPLAT_BACKGROUND = CATRE_SPLAT_BACKGROUND, SPLAT_AGREE = CATRE_SPLAT_AGREE, SPLAT_OCCLUDED = CATRE_SPLAT_OCCLUDED,
              SPLAT_FREE = CATRE_SPLAT_FREE, SPLAT_HOLE = CATRE_SPLAT_HOLE;

// point n of instance data at (pose, scale) -> depth z, centre (u0, v0) in pixels (an integer pixel is its own centre, as
// in pcl_point) and disc radius r in pixels.  false: the point draws nothing.
__device__ __forceinline__ bool splat_project(const float* __restrict__ kps, size_t n, const float* __restrict__ pose,
                                              const float* __restrict__ scale, const PclCam& cam, float rho, float r_max,
                                              float& z, float& u0, float& v0, float& r) {
  float x, y;
  nn_load_point(kps, n, pose, scale, x, y, z);
  u0 = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fx, x), z), cam.cx);
  v0 = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fy, y), z), cam.cy);
  const float rr = __fdiv_rn(__fmul_rn(cam.fx, rho), z);
  r = rr > r_max ? r_max : rr;  // min(rr, r_max) that keeps a NaN rr
  return z > 0.f && track_finite(u0) && track_finite(v0) && track_finite(r);
}

// observed depth d against rendered depth z
__device__ __forceinline__ int splat_class(float z, float d, float delta) {
  if (!(d > 0.f)) return SPLAT_HOLE;
  const float diff = __fsub_rn(z, d);
  return diff > delta ? SPLAT_OCCLUDED : diff < -delta ? SPLAT_FREE : SPLAT_AGREE;
}

__global__ __launch_bounds__(256) void k_splat_clear(unsigned long long* __restrict__ keys, int n, int32_t* __restrict__ counts,
                                                     int n_counts) {
  const int gi = blockIdx.x * 256 + threadIdx.x;
  if (gi < n) keys[gi] = SPLAT_BG;
  if (gi < n_counts) counts[gi] = 0;
}

__device__ __forceinline__ int splat_bcast(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ float splat_bcast(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

__global__ __launch_bounds__(SPLAT_THREADS) void k_splat(const float* __restrict__ kps, const float* __restrict__ pose,
                                                         const float* __restrict__ scale, const float* __restrict__ rho,
                                                         const int* __restrict__ frame_of, const PclCam* __restrict__ cams,
                                                         int M, int tiles, int ppw, int H, int W, float r_max,
                                                         unsigned long long* keys) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int inst = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int m = (tile * (SPLAT_THREADS / 64) + (tid >> 6)) * ppw + lane;
  const int frame = frame_of[inst];
  const PclCam cam = cams[frame];
  // this lane's point: bounding box [x0, x0 + bw) x [y0, y0 + bh), bw == 0 = nothing to draw
  int x0 = 0, y0 = 0, bw = 0, bh = 0;
  float z = 0.f, u0 = 0.f, v0 = 0.f, r2 = 0.f;
  if (lane < ppw && m < M) {
    float r;
    if (splat_project(kps, (size_t)inst * M + m, pose + (size_t)inst * 12, scale + (size_t)inst * 3, cam, rho[inst], r_max,
                      z, u0, v0, r)) {
      // one pixel of slack on every side (floor / ceil outwards): the footprint is decided by the distance test alone.
      // Clamped to the image in float: a point a hair in front of the camera has u0 beyond any int.
      const float ulo = fmaxf(floorf(__fsub_rn(u0, r)), 0.f), uhi = fminf(ceilf(__fadd_rn(u0, r)), (float)(W - 1));
      const float vlo = fmaxf(floorf(__fsub_rn(v0, r)), 0.f), vhi = fminf(ceilf(__fadd_rn(v0, r)), (float)(H - 1));
      if (ulo <= uhi && vlo <= vhi) {
        x0 = (int)ulo;
        y0 = (int)vlo;
        bw = (int)uhi - x0 + 1;
        bh = (int)vhi - y0 + 1;
      }
      r2 = __fmul_rn(r, r);
    }
  }
  unsigned long long* kf = keys + (size_t)frame * H * W;
  const unsigned lo = ((unsigned)inst << 16) | (unsigned)m;
  unsigned long long todo = __ballot(bw > 0);
  while (todo) {
    const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    todo &= todo - 1;
    const int jx0 = splat_bcast(x0, j), jy0 = splat_bcast(y0, j), jbw = splat_bcast(bw, j), jbh = splat_bcast(bh, j);
    const float ju0 = splat_bcast(u0, j), jv0 = splat_bcast(v0, j), jr2 = splat_bcast(r2, j);
    const unsigned long long key = ((unsigned long long)(unsigned)splat_bcast(__float_as_int(z), j) << 32) |
                                   (unsigned)splat_bcast((int)lo, j);
    const int total = jbw * jbh;  // <= H * W
    const int q = 64 / jbw, rem = 64 % jbw;
    int u = lane % jbw, v = lane / jbw;
    for (int k = lane; k < total; k += 64) {
      const int px = jx0 + u, py = jy0 + v;
      const float du = __fsub_rn((float)px, ju0), dv = __fsub_rn((float)py, jv0);
      if (fmaf(du, du, __fmul_rn(dv, dv)) <= jr2) {
        unsigned long long* p = kf + (size_t)py * W + px;
        if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
      }
      u += rem;
      v += q;
      if (u >= jbw) {
        u -= jbw;
        ++v;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_splat_resolve(const unsigned long long* __restrict__ keys,
                                                       const float* __restrict__ depth, float delta, int n,
                                                       int32_t* __restrict__ labels, float* __restrict__ zbuf,
                                                       int32_t* __restrict__ point, unsigned char* __restrict__ cls,
                                                       int32_t* __restrict__ labels_fit, int32_t* __restrict__ counts) {
  const int gi = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  int code = -1;  // instance * 8 + class of a rendered pixel
  if (gi < n) {
    const unsigned long long key = keys[gi];
    const bool bg = key == SPLAT_BG;
    const int inst = (int)((key >> 16) & 0xffffu), m = (int)(key & 0xffffu);
    const float z = bg ? 0.f : __uint_as_float((unsigned)(key >> 32));
    const int c = bg ? SPLAT_BACKGROUND : depth ? splat_class(z, depth[gi], delta) : SPLAT_AGREE;
    const int lab = bg ? 0 : inst + 1;
    labels[gi] = lab;
    zbuf[gi] = z;
    if (point) point[gi] = bg ? -1 : m;
    if (cls) cls[gi] = (unsigned char)c;
    if (labels_fit) labels_fit[gi] = c == SPLAT_AGREE ? lab : 0;
    if (!bg) code = inst * 8 + c;
  }
  // neighbouring pixels mostly share (instance, class): one pair of atomics per distinct code of the wave
  unsigned long long todo = __ballot(code >= 0);
  while (todo) {
    const int j = __ffsll((long long)todo) - 1;
    const int cj = __shfl(code, j);
    const unsigned long long same = __ballot(code == cj);
    if (lane == j) {
      const int cnt = __popcll(same);
      int32_t* row = counts + (size_t)(cj >> 3) * 5;
      atomicAdd(row, cnt);
      atomicAdd(row + (cj & 7), cnt);
    }
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void k_splat_visible(const float* __restrict__ kps, const float* __restrict__ pose,
                                                       const float* __restrict__ scale, const float* __restrict__ rho,
                                                       const int* __restrict__ frame_of, const PclCam* __restrict__ cams,
                                                       const float* __restrict__ depth, const int32_t* __restrict__ labels,
                                                       const float* __restrict__ zbuf, int M, int tiles, int H, int W,
                                                       float r_max, float delta, unsigned char* __restrict__ vis) {
  const int inst = blockIdx.x / tiles, m = (blockIdx.x % tiles) * 256 + threadIdx.x;
  if (m >= M) return;
  const int frame = frame_of[inst];
  float z, u0, v0, r;
  bool v = splat_project(kps, (size_t)inst * M + m, pose + (size_t)inst * 12, scale + (size_t)inst * 3, cams[frame],
                         rho[inst], r_max, z, u0, v0, r);
  if (v) {
    const float uc = rintf(u0), vc = rintf(v0);
    v = uc >= 0.f && uc <= (float)(W - 1) && vc >= 0.f && vc <= (float)(H - 1);  // in float: no index overflows
    if (v) {
      const size_t pix = ((size_t)frame * H + (int)vc) * W + (int)uc;
      const float zb = zbuf[pix];
      v = labels[pix] == inst + 1 && __fsub_rn(z, zb) <= delta;
      if (v && depth) v = splat_class(zb, depth[pix], delta) != SPLAT_OCCLUDED;
    }
  }
  vis[(size_t)inst * M + m] = v ? 1 : 0;
}
