// BOP pose errors on the device (lib/pysixd/pose_error.py): MSSD (:131-153), MSPD (:156-179), proj_sym (:196-217) in one
// sweep over (point, symmetry), and everything of VSD (:22-128) that follows the two renders.
//
// k_sym_err    one workgroup of four waves per (instance, tile of BOP_SYM_TILE symmetries).  The estimate's posed and
//              projected points are staged once per workgroup in LDS, BOP_CHUNK model points at a time, as two float4
//              {p.x, p.y, p.z, u_est} and {x_est, y_est, z_est, v_est}.  A wave owns BOP_SPW symmetries of the tile (s = tile
//              start + k * 4 + wave: a set of one symmetry - half the objects - keeps one wave busy, not a quarter of
//              each) and spreads its lanes over the points.  The composite A = R_gt diag(s_gt) [R_s | t_s] + [0 | t_gt] is
//              formed once per (wave, symmetry) in double and rounded once per entry; a point is then three fmas per
//              coordinate, t + A0 p.x first.  Distances are differences first: dx = x_est - x_gt, ..., d3 = fma(dx, dx,
//              fma(dy, dy, dz dz)); du = u_est - u_gt, dv alike, d2 = fma(du, du, dv dv).  The maxima are taken over the
//              SQUARED distances and rooted once (a correctly rounded root is monotone: the same bits); the mean adds
//              sqrt(d2) per lane in ascending point order in double, then an xor butterfly - a fixed tree that depends
//              on n alone, so an instance gives the same bits alone and inside any batch.  bop_max keeps a NaN: a NaN in
//              a pose, scale or point reaches all three results of the instance.  No MFMA (VALU work), no atomics.
//              Roots are sqrtf, which the compiler's default rounds correctly (k_nn_stats' choice); the __fsqrt_rn intrinsic
//              is the native instruction here, one ulp off in places.
// k_sym_min    one wave per (error, instance): the minimum over the set under a total order - a NaN first, then the smaller
//              value, then the lower index - so the lowest index wins an exact tie whatever the order of the reduction.
// k_vsd        one thread per window pixel.  The three distance images are lib/pysixd/misc.py:628-647 in double with
//              every rounding spelled out, the visibility tests lib/pysixd/visibility.py:9-74 on their fp32 casts, the
//              cost in double.  A workgroup walks up to BOP_VSD_PASSES rows of 256 pixels of one window.  Counts: ballot +
//              popcount per wave and row, kept in LDS, the four waves added at the end, one integer atomic per (workgroup,
//              count) - integer sums, exact in any order.
// k_vsd_finish one thread per (instance, tau): (cost + union - inter) / union in double, 1.0 for an empty union.
// Rounding: the fmas that are meant are written as fmas; elsewhere no product feeds a sum directly (a division or a root stands
// between), except in bop_dist, which turns contraction off for its plain operators (see there).
#pragma once
#include "catre_device.h"

#include "../../include/catre_hip.h"

constexpr int BOP_THREADS = 256;
constexpr int BOP_WAVES = BOP_THREADS / 64;
constexpr int BOP_SPW = 2;                         // symmetries per wave
constexpr int BOP_SYM_TILE = BOP_WAVES * BOP_SPW;  // symmetries per workgroup
constexpr int BOP_CHUNK = 512;                     // model points staged in LDS at a time (16 KiB as two float4 each)
constexpr int BOP_MAX_TAUS = CATRE_VSD_MAX_TAUS;
constexpr int BOP_VSD_PASSES = 8;                  // rows of 256 window pixels one workgroup of k_vsd walks

struct BopTaus {
  double v[BOP_MAX_TAUS];
};

// the rows [lo, lo + S) of the ragged symmetry table that instance `inst` reads; S = 0 for an index outside the table
__device__ __forceinline__ int bop_sym_range(const int32_t* __restrict__ sym_of, const int32_t* __restrict__ sym_off, int inst,
                                             int G, int S_tot, int S_max, int& lo) {
  lo = 0;
  const int g = sym_of[inst];
  if (g < 0 || g >= G) return 0;
  const int a = sym_off[g], b = sym_off[g + 1];
  if (a < 0 || b < a || b > S_tot || b - a > S_max) return 0;
  lo = a;
  return b - a;
}

// A [3][4] = R diag(scale) [Rs | ts] + [0 | t], pose = [R | t]; sym == NULL: the identity; scale == NULL: ones.  Formed in
// double (R * scale is exact there), one rounding to fp32 per entry.
__device__ __forceinline__ void bop_compose(const float* __restrict__ pose, const float* __restrict__ scale,
                                            const float* __restrict__ sym, float* A) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double L[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = __dmul_rn((double)pose[r * 4 + c], scale ? (double)scale[c] : 1.0);
    const double t = (double)pose[r * 4 + 3];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double a;
      if (sym) {
        a = __fma_rn(L[2], (double)sym[8 + c], __fma_rn(L[1], (double)sym[4 + c], __dmul_rn(L[0], (double)sym[c])));
        if (c == 3) a = __dadd_rn(a, t);
      } else {
        a = c == 3 ? t : L[c];
      }
      A[r * 4 + c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((float)a)));  // the same in every lane
    }
  }
}

__device__ __forceinline__ void bop_apply(const float* A, float px, float py, float pz, float& x, float& y, float& z) {
  x = __fmaf_rn(A[2], pz, __fmaf_rn(A[1], py, __fmaf_rn(A[0], px, A[3])));
  y = __fmaf_rn(A[6], pz, __fmaf_rn(A[5], py, __fmaf_rn(A[4], px, A[7])));
  z = __fmaf_rn(A[10], pz, __fmaf_rn(A[9], py, __fmaf_rn(A[8], px, A[11])));
}

// pi(x) = (fx x / z + cx, fy y / z + cy): product, quotient, sum, each rounded (splat_project's order)
__device__ __forceinline__ void bop_project(float fx, float fy, float cx, float cy, float x, float y, float z, float& u,
                                            float& v) {
  u = __fadd_rn(__fdiv_rn(__fmul_rn(fx, x), z), cx);
  v = __fadd_rn(__fdiv_rn(__fmul_rn(fy, y), z), cy);
}

__device__ __forceinline__ float bop_max(float m, float d) { return (d > m || d != d) ? d : m; }  // keeps a NaN on either side

__global__ __launch_bounds__(BOP_THREADS) void k_sym_err(const float* __restrict__ pts, int pts_shared, int n,
                                                         const float* __restrict__ pose_est,
                                                         const float* __restrict__ pose_gt,
                                                         const float* __restrict__ scale_est,
                                                         const float* __restrict__ scale_gt, const float* __restrict__ K,
                                                         const float* __restrict__ syms,
                                                         const int32_t* __restrict__ sym_off,
                                                         const int32_t* __restrict__ sym_of, int G, int S_tot, int S_max,
                                                         int stiles, int I, float* __restrict__ tab) {
  __shared__ f32x4 sp[BOP_CHUNK];  // model point, u_est
  __shared__ f32x4 se[BOP_CHUNK];  // posed estimate, v_est
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int inst = blockIdx.x / stiles, s0 = (blockIdx.x % stiles) * BOP_SYM_TILE;
  int s_lo;
  const int S = bop_sym_range(sym_of, sym_off, inst, G, S_tot, S_max, s_lo);
  const size_t plane = (size_t)I * S_max;
  float* t3 = tab + (size_t)inst * S_max;  // e3, then e2 and p2 one plane each further on
  if (tid < BOP_SYM_TILE) {  // the padding behind the set: +inf
    const int s = s0 + tid;
    if (s >= S && s < S_max) t3[s] = t3[plane + s] = t3[2 * plane + s] = __int_as_float(0x7f800000);
  }
  if (s0 >= S) return;  // the whole workgroup: S depends on the instance alone
  const float* kk = K + (size_t)inst * 9;
  const float fx = kk[0], fy = kk[4], cx = kk[2], cy = kk[5];
  const float* pp = pts + (pts_shared ? (size_t)0 : (size_t)inst * n * 3);
  float Ae[12], Ag[BOP_SPW][12];
  bop_compose(pose_est + (size_t)inst * 12, scale_est ? scale_est + (size_t)inst * 3 : nullptr, nullptr, Ae);
  bool live[BOP_SPW];
#pragma unroll
  for (int k = 0; k < BOP_SPW; ++k) {
    const int s = s0 + k * BOP_WAVES + wave;
    live[k] = s < S;
    bop_compose(pose_gt + (size_t)inst * 12, scale_gt ? scale_gt + (size_t)inst * 3 : nullptr,
                syms + (size_t)(s_lo + (live[k] ? s : S - 1)) * 12, Ag[k]);
  }
  float m3[BOP_SPW], m2[BOP_SPW];
  double sum[BOP_SPW];
#pragma unroll
  for (int k = 0; k < BOP_SPW; ++k) {
    m3[k] = m2[k] = 0.f;
    sum[k] = 0.0;
  }
  for (int c0 = 0; c0 < n; c0 += BOP_CHUNK) {
    const int cnt = min(BOP_CHUNK, n - c0);
    if (c0) __syncthreads();  // the previous chunk has been read by every wave
    for (int j = tid; j < cnt; j += BOP_THREADS) {
      const float* p = pp + (size_t)(c0 + j) * 3;
      const float px = p[0], py = p[1], pz = p[2];
      float x, y, z, u, v;
      bop_apply(Ae, px, py, pz, x, y, z);
      bop_project(fx, fy, cx, cy, x, y, z, u, v);
      sp[j] = f32x4{px, py, pz, u};
      se[j] = f32x4{x, y, z, v};
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BOP_SPW; ++k) {
      if (!live[k]) continue;  // the whole wave
      for (int j = lane; j < cnt; j += 64) {
        const f32x4 a = sp[j], b = se[j];
        float x, y, z, u, v;
        bop_apply(Ag[k], a[0], a[1], a[2], x, y, z);
        bop_project(fx, fy, cx, cy, x, y, z, u, v);
        const float dx = __fsub_rn(b[0], x), dy = __fsub_rn(b[1], y), dz = __fsub_rn(b[2], z);
        m3[k] = bop_max(m3[k], __fmaf_rn(dx, dx, __fmaf_rn(dy, dy, __fmul_rn(dz, dz))));
        const float du = __fsub_rn(a[3], u), dv = __fsub_rn(b[3], v);
        const float d2 = __fmaf_rn(du, du, __fmul_rn(dv, dv));
        m2[k] = bop_max(m2[k], d2);
        sum[k] = __dadd_rn(sum[k], (double)sqrtf(d2));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < BOP_SPW; ++k) {
    if (!live[k]) continue;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      m3[k] = bop_max(m3[k], __shfl_xor(m3[k], o));
      m2[k] = bop_max(m2[k], __shfl_xor(m2[k], o));
      sum[k] = __dadd_rn(sum[k], __shfl_xor(sum[k], o));
    }
    if (lane == 0) {
      const int s = s0 + k * BOP_WAVES + wave;
      t3[s] = sqrtf(m3[k]);
      t3[plane + s] = sqrtf(m2[k]);
      t3[2 * plane + s] = (float)__ddiv_rn(sum[k], (double)n);
    }
  }
}

// does (b, ib) come before (a, ia)?  A NaN before any number, then the smaller value, then the lower index: a total order, so
// the minimum does not depend on the order it is taken in
__device__ __forceinline__ bool bop_before(float b, int ib, float a, int ia) {
  const bool an = a != a, bn = b != b;
  if (an != bn) return bn;
  if (an || a == b) return ib < ia;
  return b < a;
}

__global__ __launch_bounds__(64) void k_sym_min(const float* __restrict__ tab, const int32_t* __restrict__ sym_off,
                                                const int32_t* __restrict__ sym_of, int G, int S_tot, int S_max, int I,
                                                float* __restrict__ err, int32_t* __restrict__ best) {
  const int i = blockIdx.x % I, q = blockIdx.x / I, lane = threadIdx.x;  // one wave per (error, instance)
  int lo;
  const int S = bop_sym_range(sym_of, sym_off, i, G, S_tot, S_max, lo);
  const float* row = tab + ((size_t)q * I + i) * S_max;
  float b = __int_as_float(0x7f800000);  // behind every entry of the table, +inf included: its index loses the tie
  int bj = 0x7fffffff;
  for (int s = lane; s < S; s += 64) {
    const float e = row[s];
    if (bop_before(e, s, b, bj)) {
      b = e;
      bj = s;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(b, o);
    const int oj = __shfl_xor(bj, o);
    if (bop_before(ob, oj, b, bj)) {
      b = ob;
      bj = oj;
    }
  }
  if (lane == 0) {  // no set: NaN, index -1
    err[(size_t)q * I + i] = S > 0 ? b : __int_as_float(0x7fc00000);
    best[(size_t)q * I + i] = S > 0 ? bj : -1;
  }
}

// misc.py:643-645: sqrt((px d)^2 + (py d)^2 + d^2), every square and every sum rounded, added in that order.  Plain operators
// with contraction off in this block (as daug_noise_f64): the __dmul_rn / __dadd_rn intrinsics are `*` and `+` inside a header
// that is compiled with contraction on, so a pragma here does not reach them and the compiler fused them into the sum.
__device__ __forceinline__ double bop_dist(double px, double py, float d) {
#pragma clang fp contract(off)
  const double dd = (double)d;
  const double a = px * dd, b = py * dd;
  const double aa = a * a, bb = b * b, d2 = dd * dd;
  const double s1 = aa + bb;
  const double s2 = s1 + d2;
  return __dsqrt_rn(s2);
}

// visibility.py:29-36 on the distances: the difference and the comparison with delta in fp32, the rest in double
__device__ __forceinline__ bool bop_visib(double d_test, double d_model, float delta, int bop18) {
  const bool near = __fsub_rn((float)d_model, (float)d_test) <= delta;
  return bop18 ? (d_test > 0.0 && d_model > 0.0 && near) : ((near || d_test == 0.0) && d_model > 0.0);
}

__global__ __launch_bounds__(BOP_THREADS) void k_vsd(const float* __restrict__ depth_est, const float* __restrict__ depth_gt,
                                                     const float* __restrict__ depth_test, const float* __restrict__ K,
                                                     const int32_t* __restrict__ frame_of,
                                                     const int32_t* __restrict__ origin, const double* __restrict__ diameter,
                                                     BopTaus taus, float delta, int bop18, int tiles, int h, int w, int F,
                                                     int H, int W, int T, int32_t* __restrict__ counts) {
  __shared__ int wc[BOP_WAVES][2 + BOP_MAX_TAUS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int inst = blockIdx.x / tiles, base = (blockIdx.x % tiles) * (BOP_THREADS * BOP_VSD_PASSES);
  const int frame = frame_of ? frame_of[inst] : 0;
  const int u0 = origin ? origin[inst * 2] : 0, v0 = origin ? origin[inst * 2 + 1] : 0;
  if (lane == 0)  // a wave's row of counts is its lane 0's alone until the barrier
    for (int q = 0; q < 2 + T; ++q) wc[wave][q] = 0;
  const float* kk = K + (size_t)inst * 9;
  for (int k = 0; k < BOP_VSD_PASSES && base + k * BOP_THREADS < h * w; ++k) {
    const int pix = base + k * BOP_THREADS + tid;
    unsigned bits = 0;  // bit 0: union, bit 1: intersection, bit 2 + t: cost at tau t
    if (pix < h * w && frame >= 0 && frame < F) {
      const long long x = (long long)u0 + pix % w, y = (long long)v0 + pix / w;
      if (x >= 0 && x < W && y >= 0 && y < H) {  // window pixels outside the frame are ignored
        const double px = __ddiv_rn(__dsub_rn((double)x, (double)kk[2]), (double)kk[0]);
        const double py = __ddiv_rn(__dsub_rn((double)y, (double)kk[5]), (double)kk[4]);
        const size_t wi = (size_t)inst * h * w + pix;
        const double d_test = bop_dist(px, py, depth_test[((size_t)frame * H + y) * W + x]);
        const double d_gt = bop_dist(px, py, depth_gt[wi]), d_est = bop_dist(px, py, depth_est[wi]);
        const bool vis_gt = bop_visib(d_test, d_gt, delta, bop18);
        const bool vis_est = bop_visib(d_test, d_est, delta, bop18) || (vis_gt && d_est > 0.0);
        if (vis_gt || vis_est) bits |= 1u;
        if (vis_gt && vis_est) {
          bits |= 2u;
          double d = fabs(__dsub_rn(d_gt, d_est));
          if (diameter) d = __ddiv_rn(d, diameter[inst]);
          for (int t = 0; t < T; ++t)
            if (d >= taus.v[t]) bits |= 4u << t;
        }
      }
    }
    for (int q = 0; q < 2 + T; ++q) {
      const int c = __popcll(__ballot((bits >> q) & 1u));
      if (lane == 0) wc[wave][q] += c;
    }
  }
  __syncthreads();
  if (tid < 2 + T) {
    const int c = wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
    if (c) atomicAdd(counts + (size_t)inst * (2 + T) + tid, c);
  }
}

__global__ void k_vsd_finish(const int32_t* __restrict__ counts, int I, int T, double* __restrict__ errors) {
  const int gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= I * T) return;
  const int32_t* row = counts + (size_t)(gi / T) * (2 + T);
  const int uni = row[0], inter = row[1], cost = row[2 + gi % T];
  errors[gi] = uni == 0 ? 1.0 : __ddiv_rn((double)(cost + uni - inter), (double)uni);
}
