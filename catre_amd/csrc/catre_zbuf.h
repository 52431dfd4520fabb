// The z-buffer core the splat render (catre_render.h) and the mesh rasteriser (catre_mesh.h) share: what a pixel holds, who
// wins it, how a wave walks the pixels of an item, and how the finished key image becomes labels, depth, classes and counts.
//
// Key image     one 64-bit key per pixel, bits(z) << 32 | low word (the renderer's: instance and point, or the posed face).
//               z > 0 makes the fp32 bit pattern order like the value, so the unsigned minimum is the nearest depth, then the
//               lower low word: ONE tie rule.  Unsigned integer min does not depend on the order of arrival, so the image is
//               bit-reproducible.  All ones is the background (no z > 0 has those bits).
// Classes       rendered depth against an observed depth (the BOP visibility test, lib/pysixd/visibility.py:9-41, with its
//               visible set split in two): zbuf_class.
// Projection    zbuf_project, the pinhole projection of both renderers: same bits.  Every product, quotient and sum in it is
//               spelled with a rounding intrinsic so that nothing is contracted or reordered.
// Box walk      a wave draws its live items one after the other (zbuf_each_live), all 64 lanes spread over the pixels of the
//               item's bounding box (zbuf_walk_box): footprints run from nothing to the whole image, a thread per item would
//               diverge by that factor.  The walk of a wave is a chain of load -> compare -> atomic round trips.
// k_zbuf_clear  key image := background, counts := 0, and one more int array of the renderer's := 0.
// Resolve       one thread per pixel: zbuf_resolve_pixel (key -> labels / zbuf / class / labels_fit), then zbuf_count: counts
//               by integer atomics after a wave-level merge of equal (instance, class) codes (integer sums: exact in any
//               order).  The renderers' resolve kernels call both and add what is their own (the point; the face and coord).
#pragma once
#include "catre_device.h"

#include "../../include/catre_hip.h"
#include "catre_pcl.h"

constexpr unsigned long long ZBUF_BG = ~0ull;
constexpr int SPLAT_BACKGROUND = CATRE_SPLAT_BACKGROUND, SPLAT_AGREE = CATRE_SPLAT_AGREE, SPLAT_OCCLUDED = CATRE_SPLAT_OCCLUDED,
              SPLAT_FREE = CATRE_SPLAT_FREE, SPLAT_HOLE = CATRE_SPLAT_HOLE;

__device__ __forceinline__ unsigned long long zbuf_key(float z, unsigned lo) {
  return ((unsigned long long)(unsigned)__float_as_int(z) << 32) | lo;
}
__device__ __forceinline__ float zbuf_key_z(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }
__device__ __forceinline__ unsigned zbuf_key_lo(unsigned long long key) { return (unsigned)(key & 0xffffffffull); }

// *p = min(*p, key): a single global_atomic_umin_x2, behind a plain load that drops it where the pixel already holds a smaller
// key.  min is monotone, so a stale value read there only costs an atomic that changes nothing, never a result.
__device__ __forceinline__ void zbuf_min(unsigned long long* p, unsigned long long key) {
  if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

// observed depth d against rendered depth z
__device__ __forceinline__ int zbuf_class(float z, float d, float delta) {
  if (!(d > 0.f)) return SPLAT_HOLE;
  const float diff = __fsub_rn(z, d);
  return diff > delta ? SPLAT_OCCLUDED : diff < -delta ? SPLAT_FREE : SPLAT_AGREE;
}

// camera-space (x, y, z) -> pixel (u, v); an integer pixel is its own centre, as in pcl_point
__device__ __forceinline__ void zbuf_project(const PclCam& cam, float x, float y, float z, float& u, float& v) {
  u = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fx, x), z), cam.cx);
  v = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fy, y), z), cam.cy);
}

// lane j's v, to every lane (j wave-uniform)
__device__ __forceinline__ int zbuf_bcast(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ float zbuf_bcast(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
__device__ __forceinline__ long long zbuf_bcast(long long v, int j) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffll), j);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), j);
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double zbuf_bcast(double v, int j) {
  return __longlong_as_double(zbuf_bcast(__double_as_longlong(v), j));
}

// f(j) for every lane j of the wave with `live`, in lane order, the whole wave at each: f broadcasts what lane j's item needs
// (zbuf_bcast) and walks it
template <class F>
__device__ __forceinline__ void zbuf_each_live(bool live, F&& f) {
  unsigned long long todo = __ballot(live);
  while (todo) {
    const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    todo &= todo - 1;
    f(j);
  }
}

// f(px, py) for every pixel of the box [x0, x0 + bw) x [y0, y0 + bh) (wave-uniform, bw > 0), row-major, sample k by lane
// k % 64: (u, v) = (k % bw, k / bw) is stepped by 64 with one division per box, none per sample
template <class F>
__device__ __forceinline__ void zbuf_walk_box(int lane, int x0, int y0, int bw, int bh, F&& f) {
  const int total = bw * bh;  // <= H * W
  const int q = 64 / bw, rem = 64 % bw;
  int u = lane % bw, v = lane / bw;
  for (int k = lane; k < total; k += 64) {
    f(x0 + u, y0 + v);
    u += rem;
    v += q;
    if (u >= bw) {
      u -= bw;
      ++v;
    }
  }
}

__global__ __launch_bounds__(256) void k_zbuf_clear(unsigned long long* __restrict__ keys, int n, int32_t* __restrict__ counts,
                                                    int n_counts, int32_t* __restrict__ extra, int n_extra) {
  const int gi = blockIdx.x * 256 + threadIdx.x;
  if (gi < n) keys[gi] = ZBUF_BG;
  if (gi < n_counts) counts[gi] = 0;
  if (gi < n_extra) extra[gi] = 0;  // n_extra == 0 with extra == nullptr
}

// pixel gi holds `key`, instance `inst`'s unless it is the background -> labels / zbuf / cls / labels_fit; returns
// instance * 8 + class of a rendered pixel, -1 for the background.  own(): the renderer's store of what won the pixel, which
// keeps its place among the stores (the order of the outputs in the ABI)
template <class Own>
__device__ __forceinline__ int zbuf_resolve_pixel(unsigned long long key, int inst, const float* __restrict__ depth, float delta,
                                                  int gi, int32_t* __restrict__ labels, float* __restrict__ zbuf,
                                                  unsigned char* __restrict__ cls, int32_t* __restrict__ labels_fit, Own&& own) {
  const bool bg = key == ZBUF_BG;
  const float z = bg ? 0.f : zbuf_key_z(key);
  const int c = bg ? SPLAT_BACKGROUND : depth ? zbuf_class(z, depth[gi], delta) : SPLAT_AGREE;
  const int lab = bg ? 0 : inst + 1;
  labels[gi] = lab;
  zbuf[gi] = z;
  own();
  if (cls) cls[gi] = (unsigned char)c;
  if (labels_fit) labels_fit[gi] = c == SPLAT_AGREE ? lab : 0;
  return bg ? -1 : inst * 8 + c;
}

// counts [I,5] += this wave's codes (-1: none).  Neighbouring pixels mostly share (instance, class): one pair of atomics per
// distinct code of the wave
__device__ __forceinline__ void zbuf_count(int code, int lane, int32_t* __restrict__ counts) {
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
