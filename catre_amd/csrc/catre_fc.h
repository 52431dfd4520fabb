// catre_fc.h - the small dense layers behind the encoder: the tile-partial max merge, the generic linear (FC tails of the
// STNs), a7+a8 the ts head, and the tile bookkeeping / GroupNorm merge the rotation-head kernels (catre_rot.h) share.
#pragma once
#include "catre_enc.h"

// ------------------------------------------------------------------------------------------
// tile partial maxima -> per-cloud max:  out[cloud][c] = max_t pm[row(cloud,t)][c]
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reduce_pm(const float* __restrict__ pm, float* __restrict__ out, int ldo, int C,
                                                   int B, int N, int M, int rpt = 1 /*partial rows per tile*/) {
  // grid (clouds, C / 256): one thread per (cloud, channel), so that a single object still spreads over several CUs
  const int cloud = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const int TN = (N + TP - 1) / TP, TM = (M + TP - 1) / TP;
  const int nt = (cloud < B ? TN : TM) * rpt;
  const size_t row0 = (cloud < B ? (size_t)cloud * TN : (size_t)B * TN + (size_t)(cloud - B) * TM) * rpt;
  const float* src = pm + row0 * PMW + c;
  float m = src[0];
  int t = 1;
  for (; t + 3 < nt; t += 4) {  // four loads in flight
    const float a = src[(size_t)t * PMW], b = src[(size_t)(t + 1) * PMW], d = src[(size_t)(t + 2) * PMW],
                e = src[(size_t)(t + 3) * PMW];
    m = fmaxf(fmaxf(m, fmaxf(a, b)), fmaxf(d, e));
  }
  for (; t < nt; ++t) m = fmaxf(m, src[(size_t)t * PMW]);
  out[(size_t)cloud * ldo + c] = m;
}

// ------------------------------------------------------------------------------------------
// generic y = act(x W^T + b) (+ I_k): one wave per 32x32 output block, operands straight from
// L2 (F.linear in pointnet.py:31-33,64-66 and the global-feature half of RotHead layer 0).
// ------------------------------------------------------------------------------------------
#define LIN_WAVES 8
// The body of k_linear for output block (bx, by): X is a global matrix or an LDS staging buffer (k_linear_pm and
// k_heads_a, catre_small.h) - the same fragment addressing, the same MFMA sequence, the same bits either way.
// `stage()` runs after the first trip's weight fragments have been requested and before X is read: the LDS-staged callers
// fill X there (+ barrier), so that their weight round trip overlaps the staging instead of following it.
// TW: W is given TRANSPOSED - element (output j, input k) at W[k * ldw + j] - and read with four 4-byte loads per chunk
// (consecutive lanes, consecutive j) instead of one 16-byte load: the dgrad of a small linear (dx = dy W) straight from
// the layer's own [J][K] weight, no transposed copy.
// XM (TW instances only): a matrix laid out like X; X is zeroed where XM <= 0 as it is loaded (ReLU backward folded in).
template <bool TW = false, class StageF>
__device__ __forceinline__ void linear_body(const float* X, int ldx, const float* __restrict__ W, int ldw,
                                            const float* __restrict__ bias, float* __restrict__ Y, int ldy, int R, int J,
                                            int K, int relu, int iden_k, int bx, int by, float (*part)[16][64],
                                            StageF stage, const float* __restrict__ XM = nullptr) {
  // 8 waves split K (interleaved 8-wide chunks), each with up to 8 chunk pairs in flight - the kernel is a chain of
  // L2 round trips, so the trip count (K/8/8/8 = 2 for K = 1024) is what sets its time; partial 32x32 blocks are
  // summed through LDS in wave order (deterministic).
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = min(bx * 32 + i, R - 1), j = min(by * 32 + i, J - 1);
  const f32x4* xa = reinterpret_cast<const f32x4*>(X + (size_t)r * ldx + 4 * h);
  const f32x4* xm = reinterpret_cast<const f32x4*>(XM + (size_t)r * ldx + 4 * h);
  auto xload = [&](int c) -> f32x4 {
    f32x4 v = xa[c * 2];
    if constexpr (TW) {
      if (XM) {
        const f32x4 m = xm[c * 2];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = m[q] > 0.f ? v[q] : 0.f;
      }
    }
    return v;
  };
  const f32x4* wb = reinterpret_cast<const f32x4*>(W + (size_t)j * ldw + 4 * h);
  const float* wt = W + (size_t)(4 * h) * ldw + j;  // TW: chunk c of this lane = wt[(8 c + s) * ldw], s = 0..3
  auto wload = [&](int c) -> f32x4 {
    if constexpr (TW) {
      const float* q = wt + (size_t)(8 * c) * ldw;
      return f32x4{q[0], q[ldw], q[2 * (size_t)ldw], q[3 * (size_t)ldw]};
    } else {
      return wb[c * 2];
    }
  };
  f32x16 acc = zero16();
  const int nkc = K / 8;
  int kc = wave;
  f32x4 b[8];
  const bool first = kc + 7 * LIN_WAVES < nkc;
  if (first) {
#pragma unroll
    for (int u = 0; u < 8; ++u) b[u] = wload(kc + LIN_WAVES * u);
  }
  __builtin_amdgcn_sched_barrier(0);
  stage();
  for (; kc + 7 * LIN_WAVES < nkc; kc += 8 * LIN_WAVES) {  // 8 chunks of this wave per trip
    f32x4 a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a[u] = xload(kc + LIN_WAVES * u);
      if (kc != wave) b[u] = wload(kc + LIN_WAVES * u);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma32(a[u][s], b[u][s], acc);  // D[row r][col j]
  }
  for (; kc + 3 * LIN_WAVES < nkc; kc += 4 * LIN_WAVES) {  // K = 256 (fc3 of the STNs): four chunks, one round trip
    f32x4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = xload(kc + LIN_WAVES * u);
      b[u] = wload(kc + LIN_WAVES * u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma32(a[u][s], b[u][s], acc);
  }
  for (; kc < nkc; kc += LIN_WAVES) {
    const f32x4 a = xload(kc), b = wload(kc);
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma32(a[s], b[s], acc);
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) part[wave][reg][lane] = acc[reg];
  __syncthreads();
  const int col = by * 32 + i;
  if (col >= J) return;
  const float bv = bias ? bias[col] : 0.f;
  const float idv = (iden_k > 0 && col < iden_k * iden_k && (col % (iden_k + 1)) == 0) ? 1.f : 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {  // wave w finishes registers 2w, 2w+1 -> rows (reg&3) + 8(reg>>2) + 4h
    const int reg = wave * 2 + q;
    const int row = bx * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    if (row < R) {
      float v = part[0][reg][lane];
#pragma unroll
      for (int w = 1; w < LIN_WAVES; ++w) v += part[w][reg][lane];
      v += bv;
      if (relu) v = fmaxf(v, 0.f);
      Y[(size_t)row * ldy + col] = v + idv;
    }
  }
}


__global__ __launch_bounds__(64 * LIN_WAVES) void k_linear(const float* __restrict__ X, int ldx,
                                                            const float* __restrict__ W, int ldw,
                                                            const float* __restrict__ bias, float* __restrict__ Y,
                                                            int ldy, int R, int J, int K, int relu, int iden_k,
                                                            const float* __restrict__ W_z1 = nullptr,
                                                            const float* __restrict__ bias_z1 = nullptr,
                                                            float* __restrict__ Y_z1 = nullptr) {
  // gridDim.z == 2: a second (W, bias, Y) on the same X in the same launch (the two rotation heads' global halves)
  if (blockIdx.z == 1) {
    W = W_z1;
    bias = bias_z1;
    Y = Y_z1;
  }
  __shared__ float part[LIN_WAVES][16][64];
  linear_body(X, ldx, W, ldw, bias, Y, ldy, R, J, K, relu, iden_k, blockIdx.x, blockIdx.y, part, [] {});
}

// Y = X W for W [K][J] row-major (the transposed-weight form of k_linear: dgrad of the FC tails / ts head in training)
__global__ __launch_bounds__(64 * LIN_WAVES) void k_linear_t(const float* __restrict__ X, int ldx,
                                                              const float* __restrict__ W, int ldw,
                                                              float* __restrict__ Y, int ldy, int R, int J, int K,
                                                              const float* __restrict__ XM) {
  __shared__ float part[LIN_WAVES][16][64];
  linear_body<true>(X, ldx, W, ldw, nullptr, Y, ldy, R, J, K, 0, 0, blockIdx.x, blockIdx.y, part, [] {}, XM);
}

// ------------------------------------------------------------------------------------------
// a7+a8: ts head (heads/fc_trans_size_head.py:61-70) on
// ts_feat = [flat_pcl_feat | (flat_kps_feat) | (init_scale) | (init_trans)] (CATRE_disR_shared.py:69-82)
// 4 objects per workgroup, thread = output channel; weights pre-transposed to [in][256].
// ------------------------------------------------------------------------------------------
#define TS_OB 4


// Layer 0 (in_dim -> 256) split over TS_KS workgroups per group of TS_OB objects: each gathers its K slice of
// ts_feat and writes a partial sum per (object, slice, channel).  With one workgroup the layer is a serial chain of
// ~1100 L2 round trips (33 us for a single object); eight slices cut it to ~140 and put 8x as many CUs to work.
#define TS_KS 8
// max over a cloud's tile partials (what k_reduce_pm writes to gfeat): out = max_t pm[row(cloud, t)][c]
// (rpt partial rows per tile: 2 after the half-tile trunk of catre_small.h, else 1)
__device__ __forceinline__ float cloud_max1(const float* __restrict__ pm, int cloud, int c, int B, int N, int M,
                                            int rpt) {
  const int TN = (N + TP - 1) / TP, TM = (M + TP - 1) / TP;
  const int nt = (cloud < B ? TN : TM) * rpt;
  const size_t row0 = (cloud < B ? (size_t)cloud * TN : (size_t)B * TN + (size_t)(cloud - B) * TM) * rpt;
  const float* src = pm + row0 * PMW + c;
  float m = src[0];
  int t = 1;
  for (; t + 7 < nt; t += 8) {  // eight loads in flight
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(t + u) * PMW];
#pragma unroll
    for (int u = 0; u < 8; ++u) m = fmaxf(m, v[u]);
  }
  for (; t < nt; ++t) m = fmaxf(m, src[(size_t)t * PMW]);
  return m;
}

// Body for object group bx, K slice ks.  pm != nullptr (small batches, k_heads_a): gfeat does not exist yet - the gather
// takes the maximum over the cloud's tile partials itself (max is exact: the same values k_reduce_pm would have written).
__device__ __forceinline__ void ts_l0_body(const float* __restrict__ gfeat, const float* __restrict__ pm,
                                           const float* __restrict__ pose, const float* __restrict__ scale,
                                           const float* __restrict__ W0T, float* __restrict__ part /*[B][TS_KS][256]*/,
                                           int B, int N, int M, int in_dim, int with_kps, int with_scale, int with_trans,
                                           int bx, int ks, float* feat /*LDS [TS_OB][slice length]*/, int rpt = 1) {
  const int tid = threadIdx.x;
  const int b0i = bx * TS_OB;
  const int k0 = (in_dim * ks) / TS_KS, k1 = (in_dim * (ks + 1)) / TS_KS, len = k1 - k0;
  for (int o = 0; o < TS_OB; ++o) {
    const int b = min(b0i + o, B - 1);
    for (int k = k0 + tid; k < k1; k += 256) {
      int kk = k;
      float v;
      if (kk < PMW) {
        v = pm ? cloud_max1(pm, b, kk, B, N, M, rpt) : gfeat[(size_t)b * PMW + kk];
      } else {
        kk -= PMW;
        if (with_kps && kk < PMW) {
          v = pm ? cloud_max1(pm, B + b, kk, B, N, M, rpt) : gfeat[(size_t)(B + b) * PMW + kk];
        } else {
          if (with_kps) kk -= PMW;
          if (with_scale && kk < 3) {
            v = scale[b * 3 + kk];
          } else {
            if (with_scale) kk -= 3;
            v = pose[b * 12 + kk * 4 + 3];  // init_trans (with_trans)
          }
        }
      }
      feat[o * len + k - k0] = v;
    }
  }
  __syncthreads();
  float acc[TS_OB];
#pragma unroll
  for (int o = 0; o < TS_OB; ++o) acc[o] = 0.f;
  // 16 weight rows requested together, then used: left to itself hipcc waits for every row before asking for the next
  // (one L2 round trip, ~150 ns, per row - measured 24 us for 137 rows)
  const float* wcol = W0T + (size_t)k0 * 256 + tid;
  int k = 0;
  for (; k + 16 <= len; k += 16) {
    float w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) w[u] = wcol[(size_t)(k + u) * 256];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int o = 0; o < TS_OB; ++o) acc[o] = fmaf(feat[o * len + k + u], w[u], acc[o]);
  }
  for (; k < len; ++k) {
    const float w = wcol[(size_t)k * 256];
#pragma unroll
    for (int o = 0; o < TS_OB; ++o) acc[o] = fmaf(feat[o * len + k], w, acc[o]);
  }
#pragma unroll
  for (int o = 0; o < TS_OB; ++o)
    if (b0i + o < B) part[((size_t)(b0i + o) * TS_KS + ks) * 256 + tid] = acc[o];
}

__global__ __launch_bounds__(256) void k_ts_l0(const float* __restrict__ gfeat, const float* __restrict__ pose,
                                               const float* __restrict__ scale, const float* __restrict__ W0T,
                                               float* __restrict__ part /*[B][TS_KS][256]*/, int B, int in_dim, int with_kps,
                                               int with_scale, int with_trans) {
  extern __shared__ __attribute__((aligned(16))) float feat[];  // [TS_OB][slice length]
  ts_l0_body(gfeat, nullptr, pose, scale, W0T, part, B, 0, 0, in_dim, with_kps, with_scale, with_trans, blockIdx.x,
             blockIdx.y, feat);
}

struct TsHeadArgs {
  const float *l0part /*[B][TS_KS][256]*/, *b0, *g0, *be0, *W1T, *b1, *g1, *be1, *Wt, *bt, *Ws, *bs;
  float *dt, *ds;
  int B;
};

// body for object group bx (1024 threads); sm: TS_OB * (256 + 4 * 256) floats of LDS
__device__ __forceinline__ void ts_head_body(const TsHeadArgs& A, int bx, float* sm) {
  const float* __restrict__ l0part = A.l0part;
  const float *__restrict__ b0 = A.b0, *__restrict__ g0 = A.g0, *__restrict__ be0 = A.be0, *__restrict__ W1T = A.W1T,
                           *__restrict__ b1 = A.b1, *__restrict__ g1 = A.g1, *__restrict__ be1 = A.be1,
                           *__restrict__ Wt = A.Wt, *__restrict__ bt = A.bt, *__restrict__ Ws = A.Ws,
                           *__restrict__ bs = A.bs;
  float *__restrict__ dt = A.dt, *__restrict__ ds = A.ds;
  const int B = A.B;
  float* hbuf = sm;                          // [TS_OB][256]
  float* kpart = hbuf + TS_OB * 256;         // [4][TS_OB][256] K-slice partial sums
  // 1024 threads: 4 K-slices x 256 output channels; slice partials are merged in slice order
  const int tid = threadIdx.x & 255, ks = threadIdx.x >> 8;
  const int b0i = bx * TS_OB;
  float acc[TS_OB];
  if (ks == 0) {
    const float ga = g0[tid], be = be0[tid], bb = b0[tid];
#pragma unroll
    for (int o = 0; o < TS_OB; ++o) {
      const float* p = l0part + (size_t)min(b0i + o, B - 1) * TS_KS * 256 + tid;
      const float v = bb + (((p[0] + p[256]) + (p[512] + p[768])) + ((p[1024] + p[1280]) + (p[1536] + p[1792])));
      hbuf[o * 256 + tid] = group8_norm_gelu(v, ga, be);
    }
  }
  __syncthreads();
  {
#pragma unroll
    for (int o = 0; o < TS_OB; ++o) acc[o] = 0.f;
#pragma unroll 1
    for (int kb = ks * 64; kb < ks * 64 + 64; kb += 16) {  // 16 rows of W1T in flight (see k_ts_l0)
      float w[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) w[u] = W1T[(kb + u) * 256 + tid];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int o = 0; o < TS_OB; ++o) acc[o] = fmaf(hbuf[o * 256 + kb + u], w[u], acc[o]);
    }
#pragma unroll
    for (int o = 0; o < TS_OB; ++o) kpart[(ks * TS_OB + o) * 256 + tid] = acc[o];
  }
  __syncthreads();
  if (ks == 0) {
    const float ga = g1[tid], be = be1[tid], bb = b1[tid];
#pragma unroll
    for (int o = 0; o < TS_OB; ++o) {
      const float v = bb + (((kpart[o * 256 + tid] + kpart[(TS_OB + o) * 256 + tid]) +
                             kpart[(2 * TS_OB + o) * 256 + tid]) + kpart[(3 * TS_OB + o) * 256 + tid]);
      hbuf[o * 256 + tid] = group8_norm_gelu(v, ga, be);
    }
  }
  __syncthreads();
  // fc_t / fc_s: 32 lanes per output (object, coordinate): lane j takes k = j, j + 32, ... and a fixed shuffle tree adds
  // the 32 partials (a serial 256-term chain per output took most of this kernel's time)
  const int grp = threadIdx.x >> 5, j = threadIdx.x & 31;
  if (grp < TS_OB * 6) {
    const int o = grp / 6, c = grp % 6;
    const int b = b0i + o;
    const float* w = c < 3 ? Wt + c * 256 : Ws + (c - 3) * 256;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) s = fmaf(hbuf[o * 256 + j + 32 * u], w[j + 32 * u], s);
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (j == 0 && b < B) {
      s += c < 3 ? bt[c] : bs[c - 3];
      if (c < 3)
        dt[b * 3 + c] = s;
      else
        ds[b * 3 + c - 3] = s;
    }
  }
}

__global__ __launch_bounds__(1024) void k_ts_head(TsHeadArgs A) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  ts_head_body(A, blockIdx.x, sm);
}

// ------------------------------------------------------------------------------------------
// a9: rotation heads (heads/conv_out_per_rot_head.py:126-140) over the concatenated point
// sequence [observed N | prior M] (CATRE_disR_shared.py:86), never materialised.
//   layer 0 : y0 = W0[:,1024:] . pointfeat + (W0[:,:1024] . g_cloud + b0)      (bias0 from k_linear)
//   GN(32,256) couples all N+M points of an object.  GN0: y0 is linear in pointfeat, so its statistics come from the
//   per-cloud mean and scatter matrix of pointfeat (catre_gram.h) instead of a first pass over layer 0.  GN1: per-tile
//   (mean, M2) partials merged with Chan's formula in tile order (deterministic).
// Tiles never straddle the observed/prior boundary: T = ceil(N/64) + ceil(M/64) per object.
// ------------------------------------------------------------------------------------------
struct RotTile {
  int obj, t, is_obs, cloud, p0, valid, gp0;  // gp0 = index in the concatenated sequence
  size_t pf_off;                              // float offset of the tile inside the pointfeat buffer
};

__device__ __forceinline__ RotTile rot_tile(int bid, int B, int N, int M) {
  const int TN = (N + TP - 1) / TP, TM = (M + TP - 1) / TP, T = TN + TM;
  RotTile r;
  r.obj = bid / T;
  r.t = bid % T;
  r.is_obs = r.t < TN;
  r.cloud = r.is_obs ? r.obj : B + r.obj;
  r.p0 = (r.is_obs ? r.t : r.t - TN) * TP;
  r.valid = min(TP, (r.is_obs ? N : M) - r.p0);
  r.gp0 = r.is_obs ? r.p0 : N + r.p0;
  r.pf_off = r.is_obs ? ((size_t)r.obj * N + r.p0) * 64 : ((size_t)B * N + (size_t)r.obj * M + r.p0) * 64;
  return r;
}

// Merge per-tile (mean, M2) partials of one (object, head, group) in tile order -> (mean, rstd)
__device__ __forceinline__ void merge_gn(const float* __restrict__ part /*[T][64]*/, int group, int T, int TN, int N,
                                         int M, float& mean_out, float& rstd_out) {
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int t = 0; t < T; ++t) {
    const int p0 = (t < TN ? t : t - TN) * TP;
    const float nb = 8.f * (float)min(TP, (t < TN ? N : M) - p0);
    const float mb = part[t * 64 + group * 2], m2b = part[t * 64 + group * 2 + 1];
    const float nn = n + nb, delta = mb - mean;
    mean += delta * (nb / nn);
    m2 += m2b + delta * delta * (n * nb / nn);
    n = nn;
  }
  mean_out = mean;
  rstd_out = 1.0f / sqrtf(m2 / n + 1e-5f);
}
