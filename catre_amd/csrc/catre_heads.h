// ------------------------------------------------------------------------------------------------
// Norm + activation stage of a head of ANY configured width, group count and activation (the heads' config surface:
// feat_dim, num_gn_groups, norm GN | none, act relu | lrelu | silu | gelu | mish | none).  The kernels of catre_train.h
// are written for (256 channels, 32 groups, GELU); these take C (a multiple of 8, <= 1024), G (a divisor of C) at run time
// and the activation and "norm on / off" as template parameters - no per-element branch.
//
// The stage is a pass over [B*P, C] rows that no GEMM absorbs (GroupNorm couples all P points of an object): HBM-bound.
//   * a lane owns 4 consecutive channels of a row (16-byte accesses), consecutive lanes consecutive channels; a 256-thread
//     workgroup covers floor(256 / (C/4)) rows per pass and 64 rows (one tile) in all, four loads in flight per lane;
//   * statistics are per-tile (mean, M2) partials, merged with Chan's formula in tile order; every other reduction is
//     per-tile partial sums merged in tile order - no atomics, so results are bit-identical from run to run and an object's
//     result does not depend on the batch around it.
// ------------------------------------------------------------------------------------------------
#pragma once
#include "catre_train.h"
#define HA_TP 64      // rows per tile
#define HA_MAXC 1024  // widest row

template <int ACT>
__device__ __forceinline__ float ha_act(float v) {
  if constexpr (ACT == CATRE_ACT_RELU) return fmaxf(v, 0.f);
  if constexpr (ACT == CATRE_ACT_LRELU) return v > 0.f ? v : 0.1f * v;  // get_nn_act_func: negative_slope 0.1
  if constexpr (ACT == CATRE_ACT_SILU) return v * __builtin_amdgcn_rcpf(1.f + __expf(-v));
  if constexpr (ACT == CATRE_ACT_GELU) return gelu_erf(v);
  if constexpr (ACT == CATRE_ACT_MISH) {
    // v tanh(softplus(v)) = v n / (n + 2), n = e^v (e^v + 2); beyond 20 (torch's softplus threshold) the ratio is 1 in fp32
    const float e = __expf(fminf(v, 20.f)), n = e * (e + 2.f);
    return v * n * __builtin_amdgcn_rcpf(n + 2.f);
  }
  return v;
}

// d act / dv at the pre-activation v
template <int ACT>
__device__ __forceinline__ float ha_act_grad(float v) {
  if constexpr (ACT == CATRE_ACT_RELU) return v > 0.f ? 1.f : 0.f;
  if constexpr (ACT == CATRE_ACT_LRELU) return v > 0.f ? 1.f : 0.1f;
  if constexpr (ACT == CATRE_ACT_SILU) {
    const float s = __builtin_amdgcn_rcpf(1.f + __expf(-v));
    return s * fmaf(v, 1.f - s, 1.f);
  }
  if constexpr (ACT == CATRE_ACT_GELU) return gelu_grad(v);
  if constexpr (ACT == CATRE_ACT_MISH) {
    // t = n / (n + 2): dt/dv = 2 n' / (n + 2)^2 with n' = 2 e (e + 1)
    const float e = __expf(fminf(v, 20.f)), n = e * (e + 2.f), r = __builtin_amdgcn_rcpf(n + 2.f);
    return fmaf(v * 4.f * e * (e + 1.f) * r, r, n * r);
  }
  return 1.f;
}

// the lane's place in a [rows, C] tile
struct HaLane {
  int c4, rl, rpp;  // float4 column, first row of the lane, rows per pass
  bool on;
};
__device__ __forceinline__ HaLane ha_lane(int C) {
  const int C4 = C >> 2;
  HaLane l;
  l.rpp = 256 / C4;
  l.rl = threadIdx.x / C4;
  l.c4 = threadIdx.x - l.rl * C4;
  l.on = l.rl < l.rpp;
  return l;
}

// (scale, shift) of the lane's four channels: a = act(y * sc + sh)
__device__ __forceinline__ void ha_affine(const float* __restrict__ stat, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, int obj, int G, int cpg, int c0, float sc[4],
                                          float sh[4], float mean[4], float rstd[4], float ga[4]) {
  const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + c0), b4 = *reinterpret_cast<const f32x4*>(beta + c0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int g = (c0 + q) / cpg;
    mean[q] = stat[((size_t)obj * G + g) * 2];
    rstd[q] = stat[((size_t)obj * G + g) * 2 + 1];
    ga[q] = g4[q];
    sc[q] = rstd[q] * g4[q];
    sh[q] = b4[q] - mean[q] * sc[q];
  }
}

// per (object, tile, group): mean and M2 of the tile's rows x the group's channels, from sums shifted by the group's first value
__global__ __launch_bounds__(256) void k_ha_stats_tile(const float* __restrict__ Y, float* __restrict__ part /*[B][nt][G][2]*/,
                                                       int P, int C, int G) {
  __shared__ float rs[HA_MAXC], rq[HA_MAXC];
  const int tile = blockIdx.x, obj = blockIdx.y, nt = gridDim.x, cpg = C / G;
  const HaLane l = ha_lane(C);
  const int p0 = tile * HA_TP, p1 = min(P, p0 + HA_TP), c0 = l.c4 * 4;
  const float* base = Y + (size_t)obj * P * C;
  if (l.on) {
    float shift[4], s[4] = {0.f, 0.f, 0.f, 0.f}, qq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) shift[q] = base[(size_t)p0 * C + ((c0 + q) / cpg) * cpg];
    for (int p = p0 + l.rl; p < p1; p += 4 * l.rpp) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        v[u] = *reinterpret_cast<const f32x4*>(base + (size_t)min(p + u * l.rpp, p1 - 1) * C + c0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (p + u * l.rpp >= p1) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float d = v[u][q] - shift[q];
          s[q] += d;
          qq[q] = fmaf(d, d, qq[q]);
        }
      }
    }
    *reinterpret_cast<f32x4*>(&rs[l.rl * C + c0]) = f32x4{s[0], s[1], s[2], s[3]};
    *reinterpret_cast<f32x4*>(&rq[l.rl * C + c0]) = f32x4{qq[0], qq[1], qq[2], qq[3]};
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) {
    float S = 0.f, Q = 0.f;
    for (int r = 0; r < l.rpp; ++r)
      for (int k = 0; k < cpg; ++k) {
        S += rs[r * C + g * cpg + k];
        Q += rq[r * C + g * cpg + k];
      }
    const float n = (float)cpg * (float)(p1 - p0);
    float* o = part + (((size_t)obj * nt + tile) * G + g) * 2;
    o[0] = base[(size_t)p0 * C + g * cpg] + S / n;
    o[1] = Q - S * S / n;
  }
}

// per object: Chan merge of the tiles in order -> (mean, rstd)
__global__ __launch_bounds__(256) void k_ha_stats_final(const float* __restrict__ part, float* __restrict__ stat, int P,
                                                        int nt, int G, int cpg) {
  const int obj = blockIdx.x;
  for (int g = threadIdx.x; g < G; g += 256) {
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int t = 0; t < nt; ++t) {
      const float nb = (float)cpg * (float)(min(P, (t + 1) * HA_TP) - t * HA_TP);
      const float* o = part + (((size_t)obj * nt + t) * G + g) * 2;
      const float nn = n + nb, delta = o[0] - mean;
      mean += delta * (nb / nn);
      m2 += o[1] + delta * delta * (n * nb / nn);
      n = nn;
    }
    stat[((size_t)obj * G + g) * 2] = mean;
    stat[((size_t)obj * G + g) * 2 + 1] = 1.0f / sqrtf(m2 / n + 1e-5f);
  }
}

template <int ACT, bool NORM>
__global__ __launch_bounds__(256) void k_ha_fwd(const float* __restrict__ Y, const float* __restrict__ stat,
                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                float* __restrict__ A, int P, int C, int G) {
  const int tile = blockIdx.x, obj = blockIdx.y;
  const HaLane l = ha_lane(C);
  if (!l.on) return;
  const int p0 = tile * HA_TP, p1 = min(P, p0 + HA_TP), c0 = l.c4 * 4;
  float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f}, mean[4], rstd[4], ga[4];
  if (NORM) ha_affine(stat, gamma, beta, obj, G, C / G, c0, sc, sh, mean, rstd, ga);
  const size_t o0 = (size_t)obj * P * C + c0;
  for (int p = p0 + l.rl; p < p1; p += 4 * l.rpp) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(Y + o0 + (size_t)min(p + u * l.rpp, p1 - 1) * C);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (p + u * l.rpp >= p1) break;
      f32x4 a;
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = ha_act<ACT>(NORM ? fmaf(v[u][q], sc[q], sh[q]) : v[u][q]);
      *reinterpret_cast<f32x4*>(A + o0 + (size_t)(p + u * l.rpp) * C) = a;
    }
  }
}

// pass 1 of the backward (norm on): per (object, tile, group) S1 = sum dxhat, S2 = sum dxhat * xhat, and per (object, tile,
// channel) partial dgamma / dbeta
template <int ACT>
__global__ __launch_bounds__(256) void k_ha_bwd_sums(const float* __restrict__ dA, const float* __restrict__ Y,
                                                     const float* __restrict__ stat, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ sums_part,
                                                     float* __restrict__ dgb_part, int P, int C, int G) {
  __shared__ float red[4][HA_MAXC];
  const int tile = blockIdx.x, obj = blockIdx.y, nt = gridDim.x, cpg = C / G;
  const HaLane l = ha_lane(C);
  const int p0 = tile * HA_TP, p1 = min(P, p0 + HA_TP), c0 = l.c4 * 4;
  if (l.on) {
    float sc[4], sh[4], mean[4], rstd[4], ga[4];
    ha_affine(stat, gamma, beta, obj, G, cpg, c0, sc, sh, mean, rstd, ga);
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, dga[4] = {0.f, 0.f, 0.f, 0.f},
          dbe[4] = {0.f, 0.f, 0.f, 0.f};
    const size_t o0 = (size_t)obj * P * C + c0;
    for (int p = p0 + l.rl; p < p1; p += 2 * l.rpp) {
      f32x4 yv[2], dv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const size_t o = o0 + (size_t)min(p + u * l.rpp, p1 - 1) * C;
        yv[u] = *reinterpret_cast<const f32x4*>(Y + o);
        dv[u] = *reinterpret_cast<const f32x4*>(dA + o);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (p + u * l.rpp >= p1) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float xh = (yv[u][q] - mean[q]) * rstd[q];
          const float dyh = dv[u][q] * ha_act_grad<ACT>(fmaf(yv[u][q], sc[q], sh[q]));
          dga[q] = fmaf(dyh, xh, dga[q]);
          dbe[q] += dyh;
          const float dxh = dyh * ga[q];
          s1[q] += dxh;
          s2[q] = fmaf(dxh, xh, s2[q]);
        }
      }
    }
    *reinterpret_cast<f32x4*>(&red[0][l.rl * C + c0]) = f32x4{s1[0], s1[1], s1[2], s1[3]};
    *reinterpret_cast<f32x4*>(&red[1][l.rl * C + c0]) = f32x4{s2[0], s2[1], s2[2], s2[3]};
    *reinterpret_cast<f32x4*>(&red[2][l.rl * C + c0]) = f32x4{dga[0], dga[1], dga[2], dga[3]};
    *reinterpret_cast<f32x4*>(&red[3][l.rl * C + c0]) = f32x4{dbe[0], dbe[1], dbe[2], dbe[3]};
  }
  __syncthreads();
  const size_t slot = (size_t)obj * nt + tile;
  for (int g = threadIdx.x; g < G; g += 256) {
    float t1 = 0.f, t2 = 0.f;
    for (int r = 0; r < l.rpp; ++r)
      for (int k = 0; k < cpg; ++k) {
        t1 += red[0][r * C + g * cpg + k];
        t2 += red[1][r * C + g * cpg + k];
      }
    sums_part[(slot * G + g) * 2] = t1;
    sums_part[(slot * G + g) * 2 + 1] = t2;
  }
  for (int c = threadIdx.x; c < C; c += 256) {
    float a = 0.f, b = 0.f;
    for (int r = 0; r < l.rpp; ++r) {
      a += red[2][r * C + c];
      b += red[3][r * C + c];
    }
    dgb_part[(slot * 2) * C + c] = a;
    dgb_part[(slot * 2 + 1) * C + c] = b;
  }
}

// sums[obj][G][2] = sum over the object's tiles, in tile order
__global__ void k_ha_bwd_sums_final(const float* __restrict__ sums_part, float* __restrict__ sums, int B, int nt, int G2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * G2) return;
  const int obj = i / G2, e = i - obj * G2;
  float s = 0.f;
  for (int t = 0; t < nt; ++t) s += sums_part[((size_t)obj * nt + t) * G2 + e];
  sums[i] = s;
}

template <int ACT, bool NORM>
__global__ __launch_bounds__(256) void k_ha_bwd_apply(const float* __restrict__ dA, const float* __restrict__ Y,
                                                      const float* __restrict__ stat, const float* __restrict__ sums,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ dY, int P, int C, int G) {
  const int tile = blockIdx.x, obj = blockIdx.y;
  const HaLane l = ha_lane(C);
  if (!l.on) return;
  const int p0 = tile * HA_TP, p1 = min(P, p0 + HA_TP), c0 = l.c4 * 4, cpg = NORM ? C / G : C;
  float sc[4], sh[4], mean[4], rstd[4], ga[4], m1[4], m2[4];
  if (NORM) {
    ha_affine(stat, gamma, beta, obj, G, cpg, c0, sc, sh, mean, rstd, ga);
    const float inv_m = 1.0f / ((float)cpg * (float)P);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int g = (c0 + q) / cpg;
      m1[q] = sums[((size_t)obj * G + g) * 2] * inv_m;
      m2[q] = sums[((size_t)obj * G + g) * 2 + 1] * inv_m;
    }
  }
  const size_t o0 = (size_t)obj * P * C + c0;
  for (int p = p0 + l.rl; p < p1; p += 2 * l.rpp) {
    f32x4 yv[2], dv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t o = o0 + (size_t)min(p + u * l.rpp, p1 - 1) * C;
      yv[u] = *reinterpret_cast<const f32x4*>(Y + o);
      dv[u] = *reinterpret_cast<const f32x4*>(dA + o);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (p + u * l.rpp >= p1) break;
      f32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (NORM) {
          const float xh = (yv[u][q] - mean[q]) * rstd[q];
          const float dxh = dv[u][q] * ha_act_grad<ACT>(fmaf(yv[u][q], sc[q], sh[q])) * ga[q];
          o[q] = rstd[q] * (dxh - m1[q] - xh * m2[q]);
        } else {
          o[q] = dv[u][q] * ha_act_grad<ACT>(yv[u][q]);
        }
      }
      *reinterpret_cast<f32x4*>(dY + o0 + (size_t)(p + u * l.rpp) * C) = o;
    }
  }
}

// column sums of part [S][W] in two fixed-order stages: 64 rows per split, then the splits in order
__global__ __launch_bounds__(256) void k_ha_colsum(const float* __restrict__ part, float* __restrict__ stage, int S, int W) {
  const int col = blockIdx.x * 256 + threadIdx.x, sp = blockIdx.y;
  if (col >= W) return;
  const int r1 = min(S, sp * 64 + 64);
  float s = 0.f;
  for (int r = sp * 64; r < r1; ++r) s += part[(size_t)r * W + col];
  stage[(size_t)sp * W + col] = s;
}
__global__ __launch_bounds__(256) void k_ha_colmerge(const float* __restrict__ stage, float* __restrict__ dgamma,
                                                     float* __restrict__ dbeta, int nsp, int C, int accumulate) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= 2 * C) return;
  float s = 0.f;
  for (int sp = 0; sp < nsp; ++sp) s += stage[(size_t)sp * 2 * C + col];
  float* o = col < C ? dgamma + col : dbeta + (col - C);
  *o = accumulate ? *o + s : s;
}

// ------------------------------------------------------------------------------------------------
// the same on FC rows [R, C] (ts head): statistics per (row, group); one workgroup per row
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void har_row_stats(const float* lrow, float* gm, float* gr, int G, int cpg) {
  for (int g = threadIdx.x; g < G; g += 256) {
    float s = 0.f;
    for (int k = 0; k < cpg; ++k) s += lrow[g * cpg + k];
    const float mean = s / (float)cpg;
    float q = 0.f;
    for (int k = 0; k < cpg; ++k) {
      const float d = lrow[g * cpg + k] - mean;
      q = fmaf(d, d, q);
    }
    gm[g] = mean;
    gr[g] = 1.0f / sqrtf(q / (float)cpg + 1e-5f);
  }
}

template <int ACT, bool NORM>
__global__ __launch_bounds__(256) void k_har_fwd(const float* __restrict__ Y, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* __restrict__ A, int C, int G) {
  __shared__ float lrow[HA_MAXC], gm[HA_MAXC], gr[HA_MAXC];
  const int r = blockIdx.x, c0 = threadIdx.x * 4, cpg = C / G;
  const bool on = c0 < C;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (on) v = *reinterpret_cast<const f32x4*>(Y + (size_t)r * C + c0);
  if (NORM) {
    if (on) *reinterpret_cast<f32x4*>(&lrow[c0]) = v;
    __syncthreads();
    har_row_stats(lrow, gm, gr, G, cpg);
    __syncthreads();
  }
  if (!on) return;
  f32x4 a;
  if (NORM) {
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + c0), b4 = *reinterpret_cast<const f32x4*>(beta + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int g = (c0 + q) / cpg;
      a[q] = ha_act<ACT>(fmaf((v[q] - gm[g]) * gr[g], g4[q], b4[q]));
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = ha_act<ACT>(v[q]);
  }
  *reinterpret_cast<f32x4*>(A + (size_t)r * C + c0) = a;
}

template <int ACT, bool NORM>
__global__ __launch_bounds__(256) void k_har_bwd(const float* __restrict__ dA, const float* __restrict__ Y,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 float* __restrict__ dY, float* __restrict__ dgb_part, int C, int G) {
  __shared__ float lrow[HA_MAXC], l2[HA_MAXC], gm[HA_MAXC], gr[HA_MAXC], gs1[HA_MAXC], gs2[HA_MAXC];
  const int r = blockIdx.x, c0 = threadIdx.x * 4, cpg = C / G;
  const bool on = c0 < C;
  f32x4 v = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    v = *reinterpret_cast<const f32x4*>(Y + (size_t)r * C + c0);
    d = *reinterpret_cast<const f32x4*>(dA + (size_t)r * C + c0);
  }
  if (!NORM) {
    if (!on) return;
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = d[q] * ha_act_grad<ACT>(v[q]);
    *reinterpret_cast<f32x4*>(dY + (size_t)r * C + c0) = o;
    return;
  }
  if (on) *reinterpret_cast<f32x4*>(&lrow[c0]) = v;
  __syncthreads();
  har_row_stats(lrow, gm, gr, G, cpg);
  __syncthreads();
  float xh[4], dyh[4], dxh[4], rstd[4];
  if (on) {
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + c0), b4 = *reinterpret_cast<const f32x4*>(beta + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int g = (c0 + q) / cpg;
      rstd[q] = gr[g];
      xh[q] = (v[q] - gm[g]) * rstd[q];
      dyh[q] = d[q] * ha_act_grad<ACT>(fmaf(xh[q], g4[q], b4[q]));
      dxh[q] = dyh[q] * g4[q];
    }
    *reinterpret_cast<f32x4*>(&lrow[c0]) = f32x4{dxh[0], dxh[1], dxh[2], dxh[3]};
    *reinterpret_cast<f32x4*>(&l2[c0]) = f32x4{dxh[0] * xh[0], dxh[1] * xh[1], dxh[2] * xh[2], dxh[3] * xh[3]};
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < cpg; ++k) {
      s1 += lrow[g * cpg + k];
      s2 += l2[g * cpg + k];
    }
    gs1[g] = s1 / (float)cpg;
    gs2[g] = s2 / (float)cpg;
  }
  __syncthreads();
  if (!on) return;
  f32x4 o, pa, pb;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int g = (c0 + q) / cpg;
    o[q] = rstd[q] * (dxh[q] - gs1[g] - xh[q] * gs2[g]);
    pa[q] = dyh[q] * xh[q];
    pb[q] = dyh[q];
  }
  *reinterpret_cast<f32x4*>(dY + (size_t)r * C + c0) = o;
  *reinterpret_cast<f32x4*>(dgb_part + ((size_t)r * 2) * C + c0) = pa;
  *reinterpret_cast<f32x4*>(dgb_part + ((size_t)r * 2 + 1) * C + c0) = pb;
}

// ------------------------------------------------------------------------------------------------
// inference tail of a RotHead: last layer's norm + act, neck Conv1d(C -> rot_dim <= 3) and conv_p in one launch behind the
// statistics merge.  out[b][j] = sum_p wp[p] (sum_c Wn[j][c] a[p][c] + bn[j]) + bp: the lane sums wp[p] a[p][c] over its
// rows first, then takes the C -> rot_dim products once - neither a [B*P, C] activation nor [B*P, 3] is stored.
// ------------------------------------------------------------------------------------------------
template <int ACT, bool NORM>
__global__ __launch_bounds__(256) void k_ha_neck_wsum(const float* __restrict__ Y, const float* __restrict__ stat,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ Wn, const float* __restrict__ wp,
                                                      float* __restrict__ part /*[B][nt][3]*/, int P, int C, int G, int rd) {
  __shared__ float red[4][3];
  const int tile = blockIdx.x, obj = blockIdx.y, nt = gridDim.x;
  const HaLane l = ha_lane(C);
  const int p0 = tile * HA_TP, p1 = min(P, p0 + HA_TP), c0 = l.c4 * 4;
  float acc[3] = {0.f, 0.f, 0.f};
  if (l.on) {
    float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f}, mean[4], rstd[4], ga[4];
    if (NORM) ha_affine(stat, gamma, beta, obj, G, C / G, c0, sc, sh, mean, rstd, ga);
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    const size_t o0 = (size_t)obj * P * C + c0;
    for (int p = p0 + l.rl; p < p1; p += 4 * l.rpp) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(Y + o0 + (size_t)min(p + u * l.rpp, p1 - 1) * C);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (p + u * l.rpp >= p1) break;
        const float w = wp[p + u * l.rpp];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = fmaf(w, ha_act<ACT>(NORM ? fmaf(v[u][q], sc[q], sh[q]) : v[u][q]), t[q]);
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < rd) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(Wn + (size_t)j * C + c0);
        acc[j] = fmaf(w4[3], t[3], fmaf(w4[2], t[2], fmaf(w4[1], t[1], w4[0] * t[0])));
      }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) acc[j] = wave_sum(acc[j]);
  if ((threadIdx.x & 63) == 0)
    for (int j = 0; j < 3; ++j) red[threadIdx.x >> 6][j] = acc[j];
  __syncthreads();
  if (threadIdx.x < 3)
    part[((size_t)obj * nt + tile) * 3 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// out[b][j] = sum over tiles (in order) + bn[j] * sum_p wp[p] + bp
__global__ __launch_bounds__(64) void k_ha_wsum_final(const float* __restrict__ part, const float* __restrict__ wp,
                                                      const float* __restrict__ bn, const float* __restrict__ bp,
                                                      float* __restrict__ out, int P, int nt, int rd) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float sw = 0.f;
  for (int p = lane; p < P; p += 64) sw += wp[p];
  sw = wave_sum(sw);
  if (lane < rd) {
    float s = 0.f;
    for (int t = 0; t < nt; ++t) s += part[((size_t)b * nt + t) * 3 + lane];
    out[(size_t)b * rd + lane] = s + (bn ? bn[lane] * sw : 0.f) + (bp ? bp[0] : 0.f);
  }
}
