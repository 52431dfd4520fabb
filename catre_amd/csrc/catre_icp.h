// Trimmed ICP on the device: one step moves a pose towards the observed points without the network.
//
// Direction: observed point -> nearest posed prior point.  The observation is partial and cluttered, the prior is complete:
// every true observed point has a counterpart, and the clutter is what the trim removes.
//
// k_icp_step  one 256-thread workgroup per instance, any n_src; rows >= counts[i] are never read.  Given the neighbours
//             catre_nn_stats wrote for (src = pcl, dst = kps at pose / scale):
//   candidates  rows k < n with 0 <= d2_k <= tau^2 (tau NULL: every finite d2_k) and a neighbour index inside [0, n_dst);
//               a NaN or infinite d2 is never one.  c = their number.
//   kept set    the m = ceil((double)trim * c) candidates smallest under the total order (d2, then k): a radix select on
//               the fp32 bit pattern (non-negative floats order like unsigned integers), four passes of eight bits with a
//               256-bin histogram in LDS (integer atomics: order-free), then the m-th key's ties are resolved by a prefix
//               count in index order, which yields the index k_cut of the last tie kept.  From there on "kept" is a
//               predicate of the row alone: (key_k, k) <= (key_m, k_cut).  No sort, no data-dependent trip count.
//   fit         fp64, as catre_align.h: source = prior point nn_j[k] posed in double from the fp32 inputs, R (s * x) + t;
//               target = pcl[k]; means, then centred moments, each by align_block_sum in its fixed order; align_solve_sv.
//               with_scale == 0 takes sigma = 1 and dt = mu_T - dR mu_S.
//   update      R' = dR R, t' = sigma dR t + dt, s' = sigma s, each rounded once to fp32.
//   status      FEW (m < 3) | DEGENERATE (sigma_2 <= 1e-12 sigma_1 of the kept covariance: the rotation is not unique) |
//               NONFINITE (incoming pose / scale or the fit).  OR-ed into what status held; with any bit set, now or
//               earlier, pose and scale pass through bit for bit.  rmse and kept are reported regardless.
// Nothing depends on the launch geometry or on the batch around an instance.  No floating-point atomics, no matrix form.
#pragma once
#include "catre_track.h"
#include "catre_align.h"

constexpr int ICP_FEW = CATRE_ICP_FEW, ICP_DEGENERATE = CATRE_ICP_DEGENERATE, ICP_NONFINITE = CATRE_ICP_NONFINITE;

// exclusive prefix of v over the 256 threads in thread order, and the total; sc: [4] ints of LDS
__device__ __forceinline__ int icp_block_scan(int v, int* sc, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  __syncthreads();  // sc may still be read from the previous use
  if (lane == 63) sc[wave] = inc;
  __syncthreads();
  const int s0 = sc[0], s1 = sc[1], s2 = sc[2], s3 = sc[3];
  total = s0 + s1 + s2 + s3;
  const int before = (wave > 0 ? s0 : 0) + (wave > 1 ? s1 : 0) + (wave > 2 ? s2 : 0);
  return before + inc - v;
}

// candidate test of one row; key = the bit pattern its d2 is ordered by (-0 counts as +0)
__device__ __forceinline__ bool icp_candidate(float d2, int j, float lim, int n_dst, unsigned& key) {
  key = __float_as_uint(d2) & 0x7fffffffu;
  return d2 >= 0.f && d2 <= lim && d2 <= 3.402823466e+38f && (unsigned)j < (unsigned)n_dst;
}

__global__ __launch_bounds__(256) void k_icp_step(const float* __restrict__ pcl, int n_src, const int* __restrict__ counts,
                                                  const float* __restrict__ kps, int n_dst, const float* pose,
                                                  const float* scale, const float* __restrict__ nn_d2,
                                                  const int* __restrict__ nn_j, const float* __restrict__ tau, float trim,
                                                  int with_scale, int update, float* pose_out, float* scale_out,
                                                  float* __restrict__ rmse_out, int* __restrict__ kept_out,
                                                  unsigned char* __restrict__ mask_out, int* status) {
  __shared__ double red[4 * ALIGN_RED];
  __shared__ int hist[256];
  __shared__ int sc[4];
  __shared__ int wcnt[2][4];
  __shared__ int sel[3];  // selected bin, rank left inside it, k_cut
  const int inst = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = align_count(counts, inst, n_src);
  const float* d2p = nn_d2 + (size_t)inst * n_src;
  const int* jp = nn_j + (size_t)inst * n_src;
  float lim = 3.402823466e+38f;
  if (tau) {
    const float t = tau[inst];
    lim = __fmul_rn(t, t);  // the one fp32 product k_nn_stats forms; NaN: no candidate
  }
  if (tid == 0) sel[0] = 0, sel[1] = 0, sel[2] = -1;

  // ---- the m-th smallest key, eight bits at a time ----
  unsigned prefix = 0;
  int c = 0, m = 0, r = 0;
#pragma unroll
  for (int shift = 24; shift >= 0; shift -= 8) {
    const unsigned himask = shift == 24 ? 0u : ~0u << (shift + 8);
    hist[tid] = 0;
    __syncthreads();
    for (int k = tid; k < n; k += 256) {
      unsigned key;
      if (icp_candidate(d2p[k], jp[k], lim, n_dst, key) && ((key ^ prefix) & himask) == 0)
        atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    const int h = hist[tid];
    int total;
    const int excl = icp_block_scan(h, sc, total);
    if (shift == 24) {
      c = total;
      m = (int)ceil((double)trim * (double)c);
      m = m > c ? c : m;
      r = m;
    }
    if (excl < r && r <= excl + h) sel[0] = tid, sel[1] = r - excl;  // one thread, or none when m == 0
    __syncthreads();
    prefix |= (unsigned)sel[0] << shift;
    r = sel[1];
  }
  // ---- ties of that key: the r lowest indices are kept; k_cut = the index of the last of them ----
  {
    int run = 0, it = 0;
    for (int base = 0; base < n; base += 256, it ^= 1) {
      const int k = base + tid;
      bool tie = false;
      if (k < n) {
        unsigned key;
        tie = icp_candidate(d2p[k], jp[k], lim, n_dst, key) && key == prefix;
      }
      const unsigned long long b = __ballot(tie);
      if (lane == 0) wcnt[it][wave] = __popcll(b);
      __syncthreads();
      const int w0 = wcnt[it][0], w1 = wcnt[it][1], w2 = wcnt[it][2], w3 = wcnt[it][3];
      const int rank = run + (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0) +
                       __popcll(b & ((1ull << lane) - 1ull));
      if (tie && rank == r - 1) sel[2] = k;
      run += w0 + w1 + w2 + w3;
    }
    __syncthreads();
  }
  const int kcut = sel[2];
  auto keep = [&](int k) {
    unsigned key;
    return icp_candidate(d2p[k], jp[k], lim, n_dst, key) && (key < prefix || (key == prefix && k <= kcut));
  };
  if (mask_out) {
    unsigned char* mk = mask_out + (size_t)inst * n_src;
    for (int k = tid; k < n_src; k += 256) mk[k] = (k < n && keep(k)) ? 1 : 0;
  }
  if (!update) {
    double e[1] = {0};
    for (int k = tid; k < n; k += 256)
      if (keep(k)) e[0] += (double)d2p[k];
    align_block_sum<1>(e, red);
    if (tid == 0) {
      rmse_out[inst] = (float)sqrt(e[0] / (double)m);
      kept_out[inst] = m;
    }
    return;
  }

  // ---- pose and scale as they came, and as doubles ----
  float pf[12], sf[3];
  bool fin = true;
#pragma unroll
  for (int q = 0; q < 12; ++q) pf[q] = pose[(size_t)inst * 12 + q], fin = fin && track_finite(pf[q]);
#pragma unroll
  for (int q = 0; q < 3; ++q) sf[q] = scale[(size_t)inst * 3 + q], fin = fin && track_finite(sf[q]);
  const double r00 = pf[0], r01 = pf[1], r02 = pf[2], t0 = pf[3], r10 = pf[4], r11 = pf[5], r12 = pf[6], t1 = pf[7],
               r20 = pf[8], r21 = pf[9], r22 = pf[10], t2 = pf[11], sx = sf[0], sy = sf[1], sz = sf[2];
  const float* P = pcl + (size_t)inst * n_src * 3;
  const float* Q = kps + (size_t)inst * n_dst * 3;
#define ICP_PAIR(K)                                                                                          \
  const int j_ = jp[K];                                                                                      \
  const double x_ = sx * (double)Q[3 * (size_t)j_], y_ = sy * (double)Q[3 * (size_t)j_ + 1],                 \
               z_ = sz * (double)Q[3 * (size_t)j_ + 2];                                                      \
  const double ax = r00 * x_ + r01 * y_ + r02 * z_ + t0, ay = r10 * x_ + r11 * y_ + r12 * z_ + t1,           \
               az = r20 * x_ + r21 * y_ + r22 * z_ + t2;                                                     \
  const double bx = (double)P[3 * (size_t)(K)], by = (double)P[3 * (size_t)(K) + 1], bz = (double)P[3 * (size_t)(K) + 2];

  int st = status[inst];  // read by every thread before the first barrier below; thread 0 writes it after the last
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = tid; k < n; k += 256) {
    if (keep(k)) {
      ICP_PAIR(k)
      a[0] += 1.0;
      a[1] += ax, a[2] += ay, a[3] += az;
      a[4] += bx, a[5] += by, a[6] += bz;
      a[7] += (double)d2p[k];
    }
  }
  align_block_sum<8>(a, red);
  const double md = (double)m;
  if (m < 3) st |= ICP_FEW;
  if (!fin) st |= ICP_NONFINITE;
  double dR00 = 1, dR01 = 0, dR02 = 0, dR10 = 0, dR11 = 1, dR12 = 0, dR20 = 0, dR21 = 0, dR22 = 1, dt0 = 0, dt1 = 0, dt2 = 0,
         sigma = 1;
  if (m >= 3) {  // uniform over the workgroup
    const double msx = a[1] / md, msy = a[2] / md, msz = a[3] / md, mtx = a[4] / md, mty = a[5] / md, mtz = a[6] / md;
    double cv[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = tid; k < n; k += 256) {
      if (keep(k)) {
        ICP_PAIR(k)
        const double ux = ax - msx, uy = ay - msy, uz = az - msz, vx = bx - mtx, vy = by - mty, vz = bz - mtz;
        cv[0] += vx * ux, cv[1] += vx * uy, cv[2] += vx * uz;
        cv[3] += vy * ux, cv[4] += vy * uy, cv[5] += vy * uz;
        cv[6] += vz * ux, cv[7] += vz * uy, cv[8] += vz * uz;
        cv[9] += ux * ux + uy * uy + uz * uz;
      }
    }
    align_block_sum<10>(cv, red);
    double sv0, sv1;
    const AlignFit f = align_solve_sv(cv[0] / md, cv[1] / md, cv[2] / md, cv[3] / md, cv[4] / md, cv[5] / md, cv[6] / md,
                                      cv[7] / md, cv[8] / md, cv[9] / md, msx, msy, msz, mtx, mty, mtz, sv0, sv1);
    if (sv1 <= 1e-12 * sv0) st |= ICP_DEGENERATE;
    dR00 = f.r00, dR01 = f.r01, dR02 = f.r02, dR10 = f.r10, dR11 = f.r11, dR12 = f.r12, dR20 = f.r20, dR21 = f.r21, dR22 = f.r22;
    if (with_scale) {
      sigma = f.s, dt0 = f.t0, dt1 = f.t1, dt2 = f.t2;
    } else {
      dt0 = mtx - (dR00 * msx + dR01 * msy + dR02 * msz);
      dt1 = mty - (dR10 * msx + dR11 * msy + dR12 * msz);
      dt2 = mtz - (dR20 * msx + dR21 * msy + dR22 * msz);
    }
    const double all = sigma + dt0 + dt1 + dt2 + dR00 + dR01 + dR02 + dR10 + dR11 + dR12 + dR20 + dR21 + dR22;
    if (!(all - all == 0.0)) st |= ICP_NONFINITE;
  }
#undef ICP_PAIR
  if (tid == 0) {
    float* po = pose_out + (size_t)inst * 12;
    float* so = scale_out + (size_t)inst * 3;
    if (st) {
#pragma unroll
      for (int q = 0; q < 12; ++q) po[q] = pf[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) so[q] = sf[q];
    } else {
      po[0] = (float)(dR00 * r00 + dR01 * r10 + dR02 * r20), po[1] = (float)(dR00 * r01 + dR01 * r11 + dR02 * r21);
      po[2] = (float)(dR00 * r02 + dR01 * r12 + dR02 * r22);
      po[3] = (float)(sigma * (dR00 * t0 + dR01 * t1 + dR02 * t2) + dt0);
      po[4] = (float)(dR10 * r00 + dR11 * r10 + dR12 * r20), po[5] = (float)(dR10 * r01 + dR11 * r11 + dR12 * r21);
      po[6] = (float)(dR10 * r02 + dR11 * r12 + dR12 * r22);
      po[7] = (float)(sigma * (dR10 * t0 + dR11 * t1 + dR12 * t2) + dt1);
      po[8] = (float)(dR20 * r00 + dR21 * r10 + dR22 * r20), po[9] = (float)(dR20 * r01 + dR21 * r11 + dR22 * r21);
      po[10] = (float)(dR20 * r02 + dR21 * r12 + dR22 * r22);
      po[11] = (float)(sigma * (dR20 * t0 + dR21 * t1 + dR22 * t2) + dt2);
      so[0] = (float)(sigma * sx), so[1] = (float)(sigma * sy), so[2] = (float)(sigma * sz);
    }
    status[inst] = st;
    rmse_out[inst] = (float)sqrt(a[7] / md);
    kept_out[inst] = m;
  }
}
