// Splat render of the posed prior: a z-buffered disc splat of every instance's prior points into the frame the instance is
// seen in -> instance labels, a depth image, the winning point, a visibility class per pixel against an observed depth map
// and per-point visibility.  The key image, its tie rule, the classes, the projection, the box walk, the clear kernel and
// the common part of the resolve are the z-buffer core's (catre_zbuf.h); this header holds what is the splat's own.
//
// k_splat          one workgroup of four waves per (instance, tile of 4 * ppw points).  The first ppw lanes of a wave project
//                  one point each; the wave then walks its live points one after the other with all 64 lanes spread over the
//                  pixels of the point's bounding box (footprints vary from 0 to (2 r_max + 1)^2 pixels).  ppw (a power of
//                  two, 4 .. 64) is the host's choice: 64 for a full grid, fewer for a handful of objects, whose points then
//                  spread over more waves.  The image does not depend on it (integer min).  A pixel inside the disc gets
//                  zbuf_min of the key bits(z) << 32 | instance << 16 | point.
// k_splat_resolve  one thread per pixel: the core's resolve, and the winning point.
// k_splat_visible  one thread per point: is the point the surface at its centre pixel?
// The projection is ONE device function (splat_project, around zbuf_project) for the splat and the visibility launch: same bits.
#pragma once
#include "catre_device.h"

#include "catre_track.h"
#include "catre_zbuf.h"

constexpr int SPLAT_THREADS = 256;

// point n of instance data at (pose, scale) -> depth z, centre (u0, v0) in pixels and disc radius r in pixels.  false: the
// point draws nothing.
__device__ __forceinline__ bool splat_project(const float* __restrict__ kps, size_t n, const float* __restrict__ pose,
                                              const float* __restrict__ scale, const PclCam& cam, float rho, float r_max,
                                              float& z, float& u0, float& v0, float& r) {
  float x, y;
  nn_load_point(kps, n, pose, scale, x, y, z);
  zbuf_project(cam, x, y, z, u0, v0);
  const float rr = __fdiv_rn(__fmul_rn(cam.fx, rho), z);
  r = rr > r_max ? r_max : rr;  // min(rr, r_max) that keeps a NaN rr
  return z > 0.f && track_finite(u0) && track_finite(v0) && track_finite(r);
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
  zbuf_each_live(bw > 0, [&](int j) {
    const int jx0 = zbuf_bcast(x0, j), jy0 = zbuf_bcast(y0, j), jbw = zbuf_bcast(bw, j), jbh = zbuf_bcast(bh, j);
    const float ju0 = zbuf_bcast(u0, j), jv0 = zbuf_bcast(v0, j), jr2 = zbuf_bcast(r2, j);
    const unsigned long long key = zbuf_key(zbuf_bcast(z, j), (unsigned)zbuf_bcast((int)lo, j));
    zbuf_walk_box(lane, jx0, jy0, jbw, jbh, [&](int px, int py) {
      const float du = __fsub_rn((float)px, ju0), dv = __fsub_rn((float)py, jv0);
      if (fmaf(du, du, __fmul_rn(dv, dv)) <= jr2) zbuf_min(kf + (size_t)py * W + px, key);
    });
  });
}

__global__ __launch_bounds__(256) void k_splat_resolve(const unsigned long long* __restrict__ keys,
                                                       const float* __restrict__ depth, float delta, int n,
                                                       int32_t* __restrict__ labels, float* __restrict__ zbuf,
                                                       int32_t* __restrict__ point, unsigned char* __restrict__ cls,
                                                       int32_t* __restrict__ labels_fit, int32_t* __restrict__ counts) {
  const int gi = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  int code = -1;
  if (gi < n) {
    const unsigned long long key = keys[gi];
    code = zbuf_resolve_pixel(key, (int)((key >> 16) & 0xffffu), depth, delta, gi, labels, zbuf, cls, labels_fit, [&] {
      if (point) point[gi] = key == ZBUF_BG ? -1 : (int)(key & 0xffffu);
    });
  }
  zbuf_count(code, lane, counts);
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
      if (v && depth) v = zbuf_class(zb, depth[pix], delta) != SPLAT_OCCLUDED;
    }
  }
  vis[(size_t)inst * M + m] = v ? 1 : 0;
}
