// catre_pclf.h - the depth augmentation the loader applies to a data batch before any cloud is cut (INPUT.AUG_DEPTH).
// The frame-batch point-cloud kernels are those of catre_pcl.h on its PclFrameTable source (C ABI: catre_pclf_api.inc).
#pragma once
#include "catre_pcl.h"

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
