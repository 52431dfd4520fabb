// catre_enc.h - the fp32 encoder kernels of the refine path: tile bookkeeping, the fp32 weight packing, a1 pose-apply,
// a2 STN3d, a3+a4 STNkd and a3+a5 the trunk (k_trunk, k_trunk4), one 64-point tile (or a pair of tiles) per workgroup.
#pragma once
#include "catre_device.h"

#include "../../include/catre_hip.h"

#define PMW 1088  // row pitch of the tile-partial-max buffer: [1024 conv max | 64 pointfeat max]

// ------------------------------------------------------------------------------------------
// tile bookkeeping
// ------------------------------------------------------------------------------------------
struct TileInfo {
  int obj;     // object index b
  int cloud;   // b (observed) or B+b (prior)
  int is_obs;
  int p0;      // first point of the tile inside its cloud
  int valid;   // number of real points in the tile (1..64); the rest are duplicates of the last one
};

// Tiles are enumerated observed-first: bid in [0, B*TN) -> observed, then B*TM prior tiles.
__device__ __forceinline__ TileInfo tile_info(int bid, int B, int N, int M) {
  const int TN = (N + TP - 1) / TP, TM = (M + TP - 1) / TP;
  TileInfo ti;
  if (bid < B * TN) {
    ti.obj = bid / TN;
    ti.cloud = ti.obj;
    ti.is_obs = 1;
    ti.p0 = (bid % TN) * TP;
    ti.valid = min(TP, N - ti.p0);
  } else {
    const int r = bid - B * TN;
    ti.obj = r / TM;
    ti.cloud = B + ti.obj;
    ti.is_obs = 0;
    ti.p0 = (r % TM) * TP;
    ti.valid = min(TP, M - ti.p0);
  }
  return ti;
}

// a1, one point: x = pcl - t (observed; only when ZERO_CENTER_INPUT) / tfd_kps = R (kps * s) (+ t otherwise)
// (engine/batch_test.py:81-97, lib/pysixd/misc.py:1014-1026).  Shared by k_pose_apply and the on-the-fly form in
// load_point, so both produce the same bits.
__device__ __forceinline__ void pose_apply_point(const float* __restrict__ p, const float* __restrict__ sc, int is_obs,
                                                 int zero_center, float& x, float& y, float& z) {
  if (is_obs) {
    if (zero_center) {
      x -= p[3];
      y -= p[7];
      z -= p[11];
    }
  } else {
    const float sx = x * sc[0], sy = y * sc[1], sz = z * sc[2];      // misc.py:1017
    // misc.py:1021 (row . column); explicit fma chain so that every caller contracts it the same way
    float ox = fmaf(p[2], sz, fmaf(p[1], sy, p[0] * sx));
    float oy = fmaf(p[6], sz, fmaf(p[5], sy, p[4] * sx));
    float oz = fmaf(p[10], sz, fmaf(p[9], sy, p[8] * sx));
    if (!zero_center) {
      ox += p[3];
      oy += p[7];
      oz += p[11];
    }
    x = ox;
    y = oy;
    z = oz;
  }
}

__device__ __forceinline__ void load_point(const catre_points& P, const TileInfo& ti, int p, float& x, float& y,
                                           float& z) {
  const int pi = ti.p0 + min(p, ti.valid - 1);  // clamp: duplicates never change a max-pool
  const float* base;
  int64_t sc;
  if (ti.is_obs) {
    base = P.obs + ti.obj * P.obs_sb + pi * P.obs_sn;
    sc = P.obs_sc;
  } else {
    base = P.kps + ti.obj * P.kps_sb + pi * P.kps_sn;
    sc = P.kps_sc;
  }
  x = base[0];
  y = base[sc];
  z = base[2 * sc];
  if (P.apply_pose) pose_apply_point(P.pose + ti.obj * 12, P.scale + ti.obj * 3, ti.is_obs, P.zero_center, x, y, z);
}

// x' = x^T T3 : u'[j] = sum_i u[i] * T[i][j]   (pointnet.py:100-102)
__device__ __forceinline__ void apply_t3(const float* __restrict__ T, float& x, float& y, float& z) {
  const float nx = fmaf(z, T[6], fmaf(y, T[3], x * T[0]));
  const float ny = fmaf(z, T[7], fmaf(y, T[4], x * T[1]));
  const float nz = fmaf(z, T[8], fmaf(y, T[5], x * T[2]));
  x = nx;
  y = ny;
  z = nz;
}

// ------------------------------------------------------------------------------------------
// weight packing (layout only, no arithmetic)
// ------------------------------------------------------------------------------------------
__global__ void k_pack_frag(const float* __restrict__ src, int ld, int coloff, int rows, int K, float* __restrict__ dst) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * K) return;
  const int s = idx & 3, lane = (idx >> 2) & 63, rest = idx >> 8;
  const int nkc = K / 8;
  const int kc = rest % nkc, mb = rest / nkc;
  const int row = mb * 32 + (lane & 31), col = kc * 8 + 4 * (lane >> 5) + s;
  dst[idx] = src[(size_t)row * ld + coloff + col];
}

// several fp32 fragment packs in one launch (a training step re-packs the eight encoder matrices after every optimizer
// step: eight 5 us launches on the critical path of each iteration)
#define PACK_MAX_JOBS 12
struct PackJobs {
  const float* src[PACK_MAX_JOBS];
  float* dst[PACK_MAX_JOBS];
  int ld[PACK_MAX_JOBS], coloff[PACK_MAX_JOBS], K[PACK_MAX_JOBS];
  int end[PACK_MAX_JOBS];  // exclusive prefix end of the job's elements (rows * K) in the launch's index space
  int n;
};
__global__ void k_pack_frag_multi(PackJobs J) {
  const int gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= J.end[J.n - 1]) return;
  int j = 0;
  while (gi >= J.end[j]) ++j;
  const int idx = gi - (j ? J.end[j - 1] : 0);
  const int s = idx & 3, lane = (idx >> 2) & 63, rest = idx >> 8;
  const int nkc = J.K[j] / 8;
  const int kc = rest % nkc, mb = rest / nkc;
  const int row = mb * 32 + (lane & 31), col = kc * 8 + 4 * (lane >> 5) + s;
  J.dst[j][idx] = J.src[j][(size_t)row * J.ld[j] + J.coloff[j] + col];
}

__global__ void k_pack_transpose(const float* __restrict__ src, int J, int K, float* __restrict__ dst) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // dst[k*J + j] = src[j*K + k]
  if (idx >= J * K) return;
  const int j = idx % J, k = idx / J;
  dst[idx] = src[(size_t)j * K + k];
}

__global__ void k_sum(const float* __restrict__ src, int n, float* __restrict__ dst) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += src[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) dst[0] = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------------------------------
// a1: pose-apply (engine/batch_test.py:81-97, lib/pysixd/misc.py:1014-1026)
// ------------------------------------------------------------------------------------------
__global__ void k_pose_apply(const float* __restrict__ pcl, const float* __restrict__ kps,
                             const float* __restrict__ pose, const float* __restrict__ scale, float* __restrict__ xo,
                             float* __restrict__ ko, int B, int N, int M, int zero_center) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int total_obs = B * N, total = B * (N + M);
  if (i >= total) return;
  const bool obs = i < total_obs;
  const int j = obs ? i : i - total_obs;
  const int b = obs ? j / N : j / M;
  const float* s = (obs ? pcl : kps) + (size_t)j * 3;
  float x = s[0], y = s[1], z = s[2];
  pose_apply_point(pose + b * 12, scale + b * 3, obs, zero_center, x, y, z);
  float* o = (obs ? xo : ko) + (size_t)j * 3;
  o[0] = x;
  o[1] = y;
  o[2] = z;
}

// Experiment knob of the instrumented build (make TRACE=1; catre_debug_knob): the co-resident workgroups of the first
// dispatch round can be started `g_dephase_cycles` apart, to test whether pairs that begin in lock step keep stalling
// in their load / thin-layer prologues at the same time.  Product build: no code.
#ifdef CATRE_DEBUG_TRACE
__device__ int g_ablate = 0;  // knob 1 (instrumented build): bit 0 = no weight loads, bit 1 = no LDS fragment loads in the bf16 pair trunk's conv4
__device__ int g_dephase_cycles = 0;
__device__ __forceinline__ void debug_dephase(int first_round_blocks) {
  const int cyc = g_dephase_cycles;
  if (cyc <= 0 || (int)blockIdx.x >= first_round_blocks) return;
  __shared__ int odd_slot;
  if (threadIdx.x == 0) {
    unsigned hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    odd_slot = hw & 1;  // wave slot on the SIMD: the two co-resident workgroups' first waves sit in different slots
  }
  __syncthreads();
  if (odd_slot) {
    const unsigned long long t0 = __builtin_readcyclecounter();
    while ((long long)(__builtin_readcyclecounter() - t0) < cyc) __builtin_amdgcn_s_sleep(32);
  }
  __syncthreads();
}
#else
__device__ __forceinline__ void debug_dephase(int) {}
#endif

// ------------------------------------------------------------------------------------------
// a2: STN3d conv stack 3->64->128->1024 (+ReLU) and per-tile max  (pointnet.py:24-28)
// 256 threads = 4 waves, 2 workgroups per CU.
// ------------------------------------------------------------------------------------------
#define FCT_BAR_WORDS 4  // arrival counters of k_fc_tail's device-wide barriers (zeroed by the encoder kernel in front of it)

// SAVE (training forward, RS == 1, N and M multiples of 64): additionally writes what the layer-wise backward reads -
// the activation images as point rows (cloud-major: B*N observed rows, then B*M prior rows) and, instead of the tile
// maxima alone, the per-tile (max, arg-max row) pairs of the pooled layer (pitch 1024, merged by k_maxpool_tiles).
struct TrainSave {
  float *s1, *s2, *s3, *s4, *s5;  // kernel-specific activation rows (see the launchers)
  float* pmax;                    // [tiles][1024]
  int* pidx;                      // [tiles][1024]
};

// ONE (full grids, RS == 1): a single workgroup per CU with ONE wave per SIMD, the last layer as an MB8 x NB2 wave tile in
// one pass (256 accumulators) - the power-limited sweep form of k_trunk4; same K order per output element: same bits.
template <int RS, bool SAVE = false, bool ONE = false>
__global__ __launch_bounds__(256, ONE ? 1 : 2) void k_stn3d(catre_points P, const float* __restrict__ W1,
                                               const float* __restrict__ b1, const f32x4* __restrict__ wp2,
                                               const float* __restrict__ b2, const f32x4* __restrict__ wp3,
                                               const float* __restrict__ b3, float* __restrict__ pm, int B, int N,
                                               int M, TrainSave sv = TrainSave{}, unsigned* __restrict__ zero_bar = nullptr) {
  __shared__ __attribute__((aligned(16))) float smem[TP * LD64 + TP * LD128];
  float* a1 = smem;
  float* a2 = smem + TP * LD64;
  const int tid = threadIdx.x, lane = tid & 63;
  if (zero_bar && blockIdx.x == 0 && tid < FCT_BAR_WORDS) zero_bar[tid] = 0u;  // the fused FC tail behind this launch (k_fc_tail) counts arrivals here
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x / RS, part = blockIdx.x % RS;
  const TileInfo ti = tile_info(tile, B, N, M);
  debug_dephase(512);

  // weights / biases of the first MFMA layer are requested before anything else
  GemmPipe<1, 2, false, false, 8, 3> g2;
  g2.prefetch(wp2 + (wave * 8) * 64 + lane, 0);
  f32x4 bv2[1][4];
  load_bias_quads<1>(bv2, b2, wave * 32, lane);
  {  // conv1 3->64 on the VALU: thread = (point, 16-channel group)
    float x, y, z;
    load_point(P, ti, lane, x, y, z);
    conv3_relu_row<16>(x, y, z, W1, b1, wave * 16, a1 + lane * LD64);
  }
  __syncthreads();
  const size_t row0 = (ti.is_obs ? (size_t)ti.obj * N : (size_t)B * N + (size_t)ti.obj * M) + ti.p0;
  if (SAVE && sv.s1) save_tile_rows<64, 256, false>(a1, LD64, sv.s1 + row0 * 64, tid);  // (no rows: the backward recomputes them, k_stn_recompute)
  // conv3 128->1024 + max: wave owns channels [wave*256, +256) in two passes of 4 m-blocks (RS = 1); RS workgroups
  // per tile: 8/RS m-blocks per wave from mb0 in one pass (see k_trunk)
  constexpr int MB3 = ONE ? 8 : RS == 8 ? 1 : RS == 4 ? 2 : 4;
  static_assert(!ONE || RS == 1, "ONE is the full-grid form");
  constexpr bool TWO = RS == 1 && !ONE;  // two passes of 4 m-blocks
  const int mb0 = part * (32 / RS) + wave * (8 / RS);
  GemmPipe<MB3, 2, true, false, 16, RS == 8 ? 3 : 2, 1> g3a, g3b;
  float bl[2][MB3];
  g3a.prefetch(wp3 + ((size_t)mb0 * 16) * 64 + lane, 16 * 64);
  load_bias_lane<MB3>(bl[0], b3, mb0 * 32, lane);
  if (TWO) load_bias_lane<MB3>(bl[1], b3, (mb0 + 4) * 32, lane);
  __builtin_amdgcn_sched_barrier(0);
  {  // conv2 64->128: wave -> m-block `wave`, both point blocks
    f32x16 acc[1][2] = {{zero16(), zero16()}};
    g2.run(acc, a1, LD64, lane);
    store_tile_lds_pre<1, 2, true, false>(acc, a2, LD128, wave * 32, bv2, lane);
  }
  __syncthreads();
  if (SAVE && sv.s2) save_tile_rows<128, 256, false>(a2, LD128, sv.s2 + row0 * 128, tid);
  float* out = pm + (size_t)tile * PMW;
  {
    f32x16 acc[MB3][2];
#pragma unroll
    for (int mb = 0; mb < MB3; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    g3a.run(acc, a2, LD128, lane);
    if (TWO) g3b.prefetch(wp3 + ((size_t)(mb0 + 4) * 16) * 64 + lane, 16 * 64);
    if (SAVE)
      argmax_tile_store<MB3, 2>(acc, sv.pmax + (size_t)tile * 1024, sv.pidx + (size_t)tile * 1024, mb0 * 32, bl[0],
                                (int)row0, lane);
    else
      max_tile_store_pre<MB3, 2>(acc, out, mb0 * 32, bl[0], true, lane);
  }
  if (TWO) {
    f32x16 acc[MB3][2];
#pragma unroll
    for (int mb = 0; mb < MB3; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    g3b.run(acc, a2, LD128, lane);
    if (SAVE)
      argmax_tile_store<MB3, 2>(acc, sv.pmax + (size_t)tile * 1024, sv.pidx + (size_t)tile * 1024, (mb0 + 4) * 32, bl[1],
                                (int)row0, lane);
    else
      max_tile_store_pre<MB3, 2>(acc, out, (mb0 + 4) * 32, bl[1], true, lane);
  }
}

// ------------------------------------------------------------------------------------------
// a3+a4: x' = x T3, relu(conv1), STNkd conv stack 64->64->128->1024 (+ReLU), per-tile max
// (pointnet.py:98-103, 57-61).  256 threads, 2 workgroups per CU.
// ------------------------------------------------------------------------------------------
template <int RS, bool SAVE = false, bool ONE = false>
__global__ __launch_bounds__(256, ONE ? 1 : 2) void k_stnkd(catre_points P, const float* __restrict__ trans3,
                                               const float* __restrict__ Wc1, const float* __restrict__ bc1,
                                               const f32x4* __restrict__ wpf1, const float* __restrict__ bf1,
                                               const f32x4* __restrict__ wpf2, const float* __restrict__ bf2,
                                               const f32x4* __restrict__ wpf3, const float* __restrict__ bf3,
                                               float* __restrict__ pm, int B, int N, int M,
                                               TrainSave sv = TrainSave{}, unsigned* __restrict__ zero_bar = nullptr) {
  __shared__ __attribute__((aligned(16))) float smem[2 * TP * LD64 + TP * LD128];
  float* h1 = smem;
  float* f1 = smem + TP * LD64;
  float* f2 = smem + 2 * TP * LD64;
  const int tid = threadIdx.x, lane = tid & 63;
  if (zero_bar && blockIdx.x == 0 && tid < FCT_BAR_WORDS) zero_bar[tid] = 0u;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x / RS, part = blockIdx.x % RS;
  const TileInfo ti = tile_info(tile, B, N, M);
  debug_dephase(512);

  const int mblk1 = wave >> 1, nb1 = wave & 1;
  GemmPipe<1, 1, false, false, 8, 4> g1;
  g1.prefetch(wpf1 + (mblk1 * 8) * 64 + lane, 0);
  f32x4 bv1[1][4];
  load_bias_quads<1>(bv1, bf1, mblk1 * 32, lane);
  {
    float x, y, z;
    load_point(P, ti, lane, x, y, z);
    apply_t3(trans3 + ti.cloud * 9, x, y, z);
    conv3_relu_row<16>(x, y, z, Wc1, bc1, wave * 16, h1 + lane * LD64);
  }
  __syncthreads();
  GemmPipe<1, 2, false, false, 8, 3> g2;
  g2.prefetch(wpf2 + (wave * 8) * 64 + lane, 0);
  f32x4 bv2[1][4];
  load_bias_quads<1>(bv2, bf2, wave * 32, lane);
  __builtin_amdgcn_sched_barrier(0);
  {  // fstn.conv1 64->64: 2 m-blocks x 2 point blocks, one per wave
    f32x16 acc[1][1] = {{zero16()}};
    g1.run(acc, h1 + nb1 * 32 * LD64, LD64, lane);
    store_tile_lds_pre<1, 1, true, false>(acc, f1 + nb1 * 32 * LD64, LD64, mblk1 * 32, bv1, lane);
  }
  __syncthreads();
  const size_t row0 = (ti.is_obs ? (size_t)ti.obj * N : (size_t)B * N + (size_t)ti.obj * M) + ti.p0;
  if (SAVE && sv.s1) save_tile_rows<64, 256, false>(f1, LD64, sv.s1 + row0 * 64, tid);
  constexpr int MB3 = ONE ? 8 : RS == 8 ? 1 : RS == 4 ? 2 : 4;
  static_assert(!ONE || RS == 1, "ONE is the full-grid form");
  constexpr bool TWO = RS == 1 && !ONE;  // two passes of 4 m-blocks
  const int mb0 = part * (32 / RS) + wave * (8 / RS);
  GemmPipe<MB3, 2, true, false, 16, RS == 8 ? 3 : 2, 1> g3a, g3b;
  float bl[2][MB3];
  g3a.prefetch(wpf3 + ((size_t)mb0 * 16) * 64 + lane, 16 * 64);
  load_bias_lane<MB3>(bl[0], bf3, mb0 * 32, lane);
  if (TWO) load_bias_lane<MB3>(bl[1], bf3, (mb0 + 4) * 32, lane);
  __builtin_amdgcn_sched_barrier(0);
  {  // fstn.conv2 64->128
    f32x16 acc[1][2] = {{zero16(), zero16()}};
    g2.run(acc, f1, LD64, lane);
    store_tile_lds_pre<1, 2, true, false>(acc, f2, LD128, wave * 32, bv2, lane);
  }
  __syncthreads();
  if (SAVE && sv.s2) save_tile_rows<128, 256, false>(f2, LD128, sv.s2 + row0 * 128, tid);
  float* out = pm + (size_t)tile * PMW;
  {  // fstn.conv3 128->1024 + max, two passes of 4 m-blocks (RS = 1) or one pass of 8/RS
    f32x16 acc[MB3][2];
#pragma unroll
    for (int mb = 0; mb < MB3; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    g3a.run(acc, f2, LD128, lane);
    if (TWO) g3b.prefetch(wpf3 + ((size_t)(mb0 + 4) * 16) * 64 + lane, 16 * 64);
    if (SAVE)
      argmax_tile_store<MB3, 2>(acc, sv.pmax + (size_t)tile * 1024, sv.pidx + (size_t)tile * 1024, mb0 * 32, bl[0],
                                (int)row0, lane);
    else
      max_tile_store_pre<MB3, 2>(acc, out, mb0 * 32, bl[0], true, lane);
  }
  if (TWO) {
    f32x16 acc[MB3][2];
#pragma unroll
    for (int mb = 0; mb < MB3; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    g3b.run(acc, f2, LD128, lane);
    if (SAVE)
      argmax_tile_store<MB3, 2>(acc, sv.pmax + (size_t)tile * 1024, sv.pidx + (size_t)tile * 1024, (mb0 + 4) * 32, bl[1],
                                (int)row0, lane);
    else
      max_tile_store_pre<MB3, 2>(acc, out, (mb0 + 4) * 32, bl[1], true, lane);
  }
}

// ------------------------------------------------------------------------------------------
// The ONE form of the two STN kernels on PAIRS of tiles (128 points per workgroup): with one wave per SIMD nothing runs
// under a barrier, a point load or the dependent MFMA chains of the thin layers, so the prologue is done once for two tiles
// (four independent accumulators in conv2 instead of two, half the barriers and load round trips per tile) and the last
// layer sweeps the two tiles one after the other on the same 256 accumulators.  Every output element sees the operands of
// k_stn3d / k_stnkd in the same K order: same bits.  A cloud with an odd number of tiles ends in a pair of one tile: its
// second half holds clamped duplicates and is not swept.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void pair_info32(int bid, int B, int N, int M, TileInfo& ti, int& tile0) {
  const int TN = (N + TP - 1) / TP, TM = (M + TP - 1) / TP, PN = (TN + 1) / 2, PM_ = (TM + 1) / 2;
  if (bid < B * PN) {
    ti.obj = bid / PN;
    ti.cloud = ti.obj;
    ti.is_obs = 1;
    const int pi = bid % PN;
    ti.p0 = pi * 2 * TP;
    ti.valid = min(2 * TP, N - ti.p0);
    tile0 = ti.obj * TN + 2 * pi;
  } else {
    const int r = bid - B * PN;
    ti.obj = r / PM_;
    ti.cloud = B + ti.obj;
    ti.is_obs = 0;
    const int pi = r % PM_;
    ti.p0 = pi * 2 * TP;
    ti.valid = min(2 * TP, M - ti.p0);
    tile0 = B * TN + ti.obj * TM + 2 * pi;
  }
}

// ARGMAX (training forward without activation saves: the row-sparse backward rebuilds the two thin layers on its live rows,
// k_stn_recompute): per tile the (max + bias, arg-max row) pairs of the pooled layer instead of the tile maxima.
// cloud-major row (B*N observed rows, then B*M prior rows) of the first point of a pair
__device__ __forceinline__ int pair_row0(const TileInfo& ti, int B, int N, int M) {
  return (ti.is_obs ? ti.obj * N : B * N + ti.obj * M) + ti.p0;
}

template <bool ARGMAX = false>
__global__ __launch_bounds__(256) void k_stn3d_pair(catre_points P, const float* __restrict__ W1,
                                                    const float* __restrict__ b1, const f32x4* __restrict__ wp2,
                                                    const float* __restrict__ b2, const f32x4* __restrict__ wp3,
                                                    const float* __restrict__ b3, float* __restrict__ pm, int B, int N,
                                                    int M, TrainSave sv = TrainSave{}) {
  __shared__ __attribute__((aligned(16))) float smem[2 * TP * LD64 + 2 * TP * LD128];
  float* a1 = smem;                   // [128][68]
  float* a2 = smem + 2 * TP * LD64;   // [128][132]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  TileInfo ti;
  int tile0;
  pair_info32(blockIdx.x, B, N, M, ti, tile0);
  const bool has2 = ti.valid > TP;

  GemmPipe<1, 4, false, false, 8, 3> g2;  // conv2 64->128: wave -> m-block `wave`, all four point blocks
  g2.prefetch(wp2 + (wave * 8) * 64 + lane, 0);
  f32x4 bv2[1][4];
  load_bias_quads<1>(bv2, b2, wave * 32, lane);
  {  // conv1 3->64 on the VALU: thread = (point, 32-channel half)
    const int p = (wave & 1) * TP + lane;
    float x, y, z;
    load_point(P, ti, p, x, y, z);
    conv3_relu_row<32>(x, y, z, W1, b1, (wave >> 1) * 32, a1 + p * LD64);
  }
  __syncthreads();
  const int mb0 = wave * 8;
  float bl[8];
  GemmPipe<8, 2, true, false, 16, 2, 1> g3;  // first sweep: its first weight chunks are requested in front of conv2
  g3.prefetch(wp3 + ((size_t)mb0 * 16) * 64 + lane, 16 * 64);
  load_bias_lane<8>(bl, b3, mb0 * 32, lane);
  __builtin_amdgcn_sched_barrier(0);
  {
    f32x16 acc[1][4] = {{zero16(), zero16(), zero16(), zero16()}};
    g2.run(acc, a1, LD64, lane);
    store_tile_lds_pre<1, 4, true, false>(acc, a2, LD128, wave * 32, bv2, lane);
  }
  __syncthreads();
  {  // the two tiles one after the other on the same accumulators.  (No weight ring carried across the epilogue - the 256
     // maxima pass through the VGPRs there and 64 prefetched registers next to them spill; a runtime loop over the two
     // sweeps spills as well.)
    f32x16 acc[8][2];
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    g3.run(acc, a2, LD128, lane);
    if constexpr (ARGMAX)
      argmax_tile_store<8, 2>(acc, sv.pmax + (size_t)tile0 * 1024, sv.pidx + (size_t)tile0 * 1024, mb0 * 32, bl,
                              pair_row0(ti, B, N, M), lane);
    else
      max_tile_store_pre<8, 2>(acc, pm + (size_t)tile0 * PMW, mb0 * 32, bl, true, lane);
  }
  if (has2) {
    f32x16 acc[8][2];
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    // opaque: otherwise the second sweep shares the first one's 32 fragment base pointers, which then stay live across the
    // epilogue in between - where the 256 maxima pass through the VGPRs - and spill
    unsigned lane_o = lane;
    asm volatile("" : "+v"(lane_o));
    gemm_core<8, 2, true, false, 16, 2, 1>(acc, wp3 + ((size_t)mb0 * 16) * 64 + lane_o, 16 * 64, a2 + TP * LD128, LD128, lane);
    if constexpr (ARGMAX)
      argmax_tile_store<8, 2>(acc, sv.pmax + (size_t)(tile0 + 1) * 1024, sv.pidx + (size_t)(tile0 + 1) * 1024, mb0 * 32, bl,
                              pair_row0(ti, B, N, M) + TP, lane);
    else
      max_tile_store_pre<8, 2>(acc, pm + (size_t)(tile0 + 1) * PMW, mb0 * 32, bl, true, lane);
  }
}

template <bool ARGMAX = false>
__global__ __launch_bounds__(256) void k_stnkd_pair(catre_points P, const float* __restrict__ trans3,
                                                    const float* __restrict__ Wc1, const float* __restrict__ bc1,
                                                    const f32x4* __restrict__ wpf1, const float* __restrict__ bf1,
                                                    const f32x4* __restrict__ wpf2, const float* __restrict__ bf2,
                                                    const f32x4* __restrict__ wpf3, const float* __restrict__ bf3,
                                                    float* __restrict__ pm, int B, int N, int M,
                                                    TrainSave sv = TrainSave{}) {
  __shared__ __attribute__((aligned(16))) float smem[4 * TP * LD64 + 2 * TP * LD128];
  float* h1 = smem;                   // [128][68]
  float* f1 = smem + 2 * TP * LD64;   // [128][68]
  float* f2 = smem + 4 * TP * LD64;   // [128][132]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  TileInfo ti;
  int tile0;
  pair_info32(blockIdx.x, B, N, M, ti, tile0);
  const bool has2 = ti.valid > TP;

  const int mblk1 = wave >> 1, half1 = wave & 1;
  GemmPipe<1, 2, false, false, 8, 4> g1;  // fstn.conv1 64->64: wave -> (m-block, tile of the pair)
  g1.prefetch(wpf1 + (mblk1 * 8) * 64 + lane, 0);
  f32x4 bv1[1][4];
  load_bias_quads<1>(bv1, bf1, mblk1 * 32, lane);
  {
    const int p = (wave & 1) * TP + lane;
    float x, y, z;
    load_point(P, ti, p, x, y, z);
    apply_t3(trans3 + ti.cloud * 9, x, y, z);
    conv3_relu_row<32>(x, y, z, Wc1, bc1, (wave >> 1) * 32, h1 + p * LD64);
  }
  __syncthreads();
  GemmPipe<1, 4, false, false, 8, 3> g2;
  g2.prefetch(wpf2 + (wave * 8) * 64 + lane, 0);
  f32x4 bv2[1][4];
  load_bias_quads<1>(bv2, bf2, wave * 32, lane);
  __builtin_amdgcn_sched_barrier(0);
  {
    f32x16 acc[1][2] = {{zero16(), zero16()}};
    g1.run(acc, h1 + half1 * TP * LD64, LD64, lane);
    store_tile_lds_pre<1, 2, true, false>(acc, f1 + half1 * TP * LD64, LD64, mblk1 * 32, bv1, lane);
  }
  __syncthreads();
  const int mb0 = wave * 8;
  float bl[8];
  GemmPipe<8, 2, true, false, 16, 2, 1> g3;  // first sweep: its first weight chunks are requested in front of conv2
  g3.prefetch(wpf3 + ((size_t)mb0 * 16) * 64 + lane, 16 * 64);
  load_bias_lane<8>(bl, bf3, mb0 * 32, lane);
  __builtin_amdgcn_sched_barrier(0);
  {
    f32x16 acc[1][4] = {{zero16(), zero16(), zero16(), zero16()}};
    g2.run(acc, f1, LD64, lane);
    store_tile_lds_pre<1, 4, true, false>(acc, f2, LD128, wave * 32, bv2, lane);
  }
  __syncthreads();
  {  // the two tiles one after the other on the same accumulators.  (No weight ring carried across the epilogue - the 256
     // maxima pass through the VGPRs there and 64 prefetched registers next to them spill; a runtime loop over the two
     // sweeps spills as well.)
    f32x16 acc[8][2];
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    g3.run(acc, f2, LD128, lane);
    if constexpr (ARGMAX)
      argmax_tile_store<8, 2>(acc, sv.pmax + (size_t)tile0 * 1024, sv.pidx + (size_t)tile0 * 1024, mb0 * 32, bl,
                              pair_row0(ti, B, N, M), lane);
    else
      max_tile_store_pre<8, 2>(acc, pm + (size_t)tile0 * PMW, mb0 * 32, bl, true, lane);
  }
  if (has2) {
    f32x16 acc[8][2];
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    // opaque: otherwise the second sweep shares the first one's 32 fragment base pointers, which then stay live across the
    // epilogue in between - where the 256 maxima pass through the VGPRs - and spill
    unsigned lane_o = lane;
    asm volatile("" : "+v"(lane_o));
    gemm_core<8, 2, true, false, 16, 2, 1>(acc, wpf3 + ((size_t)mb0 * 16) * 64 + lane_o, 16 * 64, f2 + TP * LD128, LD128, lane);
    if constexpr (ARGMAX)
      argmax_tile_store<8, 2>(acc, sv.pmax + (size_t)(tile0 + 1) * 1024, sv.pidx + (size_t)(tile0 + 1) * 1024, mb0 * 32, bl,
                              pair_row0(ti, B, N, M) + TP, lane);
    else
      max_tile_store_pre<8, 2>(acc, pm + (size_t)(tile0 + 1) * PMW, mb0 * 32, bl, true, lane);
  }
}

// ------------------------------------------------------------------------------------------
// a3+a5: trunk.  x' = x T3 -> relu(conv1) -> pointfeat = h1^T T64 -> relu(conv2) -> relu(conv3)
// -> conv4 -> max  (pointnet.py:98-116).  512 threads = 8 waves, 1 workgroup per CU.
// The whole 64-point x 512-channel conv4 input lives in LDS (128 KiB, XOR-swizzled, no padding) next to
// the conv3 input (32 KiB): exactly the 160 KiB of a CU.  conv4 is then ONE K=512 sweep per wave
// (1024 ch x 64 pts = 128 accumulator VGPRs per lane over 8 waves) with no barrier inside.
// ------------------------------------------------------------------------------------------
// Small grids (tiles * RS <= #CUs): RS workgroups share a tile - each repeats the cheap prologue (conv1-conv3, 12 % of
// the FLOPs) and sweeps 1/RS of conv4's output channels, so a handful of objects still spreads over the chip.  Every
// output channel sees the same K order for any RS: results do not depend on it.
// ------------------------------------------------------------------------------------------
#define TRUNK_SMEM (TP * 512 + TP * 128)

template <int RS, bool SAVE = false>
__global__ __launch_bounds__(512) void k_trunk(catre_points P, const float* __restrict__ trans3,
                                               const float* __restrict__ trans64, const float* __restrict__ Wc1,
                                               const float* __restrict__ bc1, const f32x4* __restrict__ wp2,
                                               const float* __restrict__ b2, const f32x4* __restrict__ wp3,
                                               const float* __restrict__ b3, const f32x4* __restrict__ wp4,
                                               const float* __restrict__ b4, float* __restrict__ pm,
                                               float* __restrict__ pointfeat, int B, int N, int M,
                                               unsigned long long* __restrict__ trace, TrainSave sv = TrainSave{}) {
  __shared__ __attribute__((aligned(16))) float smem[TRUNK_SMEM];
#define TRUNK_STAMP(i)                                                                     \
  do {                                                                                     \
    if (CATRE_TRACE_ON && trace && lane == 0) trace[((size_t)tile * 8 + wave) * 8 + (i)] = __builtin_readcyclecounter(); \
  } while (0)
  // phase-1/2 buffers alias the conv4 input image a3 (dead before a3 is first written)
  float* h1 = smem;                      // [64][68]
  float* t64 = smem + TP * LD64;         // [64][64]
  float* pf = smem + TP * LD64 + 4096;   // [64][68]
  float* a3 = smem;                      // [64][512] swizzled
  float* a2 = smem + TP * 512;           // [64][128] swizzled
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x / RS, part = blockIdx.x % RS;
  const TileInfo ti = tile_info(tile, B, N, M);
  const bool ft = trans64 != nullptr;
  TRUNK_STAMP(0);

  // conv2 64->128: 4 m-blocks x 2 point blocks over 8 waves.  Its first weight chunks and bias are
  // requested now, long before they are needed.
  const int mblk2 = wave >> 1, nb2 = wave & 1;
  GemmPipe<1, 1, false, false, 8, 4> g2;
  g2.prefetch(wp2 + (mblk2 * 8) * 64 + lane, 0);
  f32x4 bv2[1][4];
  load_bias_quads<1>(bv2, b2, mblk2 * 32, lane);
  {
    float x, y, z;
    load_point(P, ti, lane, x, y, z);
    apply_t3(trans3 + ti.cloud * 9, x, y, z);
    if (SAVE && wave == 0) {  // x' = x T3 as a zero-padded 8-wide row: the input of the conv1 row GEMM in the backward
      float* xr = sv.s1 + ((ti.is_obs ? (size_t)ti.obj * N : (size_t)B * N + (size_t)ti.obj * M) + ti.p0 + lane) * 8;
      *reinterpret_cast<f32x4*>(xr) = f32x4{x, y, z, 0.f};
      *reinterpret_cast<f32x4*>(xr + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    conv3_relu_row<8>(x, y, z, Wc1, bc1, wave * 8, h1 + lane * LD64);
    if (ft) {
      const f32x4* src = reinterpret_cast<const f32x4*>(trans64 + (size_t)ti.cloud * 4096);
      f32x4* dst = reinterpret_cast<f32x4*>(t64);
      dst[tid] = src[tid];
      dst[tid + 512] = src[tid + 512];
    }
  }
  __syncthreads();
  TRUNK_STAMP(1);
  const size_t trow0 = (ti.is_obs ? (size_t)ti.obj * N : (size_t)B * N + (size_t)ti.obj * M) + ti.p0;
  if (SAVE) save_tile_rows<64, 512, false>(h1, LD64, sv.s2 + trow0 * 64, tid);
  if (ft) {
    if (wave < 4) {  // pointfeat[j][n] = sum_i T64[i][j] h1[i][n]  (pointnet.py:107-109); A operand from LDS
      const int mblk = wave >> 1, nb = wave & 1;
      const int n = lane & 31, h = lane >> 5;
      f32x16 acc = zero16();
      const float* xr = h1 + (nb * 32 + n) * LD64 + 4 * h;
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) {
        const f32x4 bx = *reinterpret_cast<const f32x4*>(xr + kc * 8);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float a = t64[(kc * 8 + 4 * h + s) * 64 + mblk * 32 + n];
          acc = mfma32(a, bx[s], acc);
        }
      }
      f32x16 accs[1][1] = {{acc}};
      store_tile_lds<1, 1, false>(accs, pf + nb * 32 * LD64, LD64, mblk * 32, nullptr, lane);
    }
    __syncthreads();
  } else {
    pf = h1;
  }
  TRUNK_STAMP(2);
  // conv3 128->512: 16 m-blocks, two per wave; request its first weight chunks and bias now
  GemmPipe<2, 2, false, true, 16, 3, 1> g3;
  g3.prefetch(wp3 + (wave * 2 * 16) * 64 + lane, 16 * 64);
  f32x4 bv3[2][4];
  load_bias_quads<2>(bv3, b3, wave * 64, lane);
  __builtin_amdgcn_sched_barrier(0);
  const int pf_row = tid >> 3, pf_c4 = tid & 7;
  f32x4 pf_out0 = {0.f, 0.f, 0.f, 0.f}, pf_out1 = {0.f, 0.f, 0.f, 0.f};
  float pf_max = 0.f;
  {
    // pointfeat tile -> registers now, -> HBM after the last barrier (a __syncthreads waits for this wave's
    // outstanding stores, so storing here would park all 8 waves behind a write acknowledge)
    if (pf_row < ti.valid) {
      const f32x4* s = reinterpret_cast<const f32x4*>(pf + pf_row * LD64);
      pf_out0 = s[pf_c4];
      pf_out1 = s[pf_c4 + 8];
    }
    {  // max_n pointfeat (second half of flat_pcl_feat, CATRE_disR_shared.py:69): wave w reduces points
       // [8w, 8w+8) for channel `lane`, then 64 threads merge the 8 partials (scratch sits in the still unused
       // tail of the a3 region; the extra barrier is cheap, all waves arrive together)
      float* scratch = smem + 2 * TP * LD64 + 4096;  // [8][64]
      const float* col = pf + (wave * 8) * LD64 + lane;
      float m = col[0];
#pragma unroll
      for (int p = 1; p < 8; ++p) m = fmaxf(m, col[p * LD64]);
      scratch[wave * 64 + lane] = m;
      __syncthreads();
      if (tid < 64) {
        m = scratch[tid];
#pragma unroll
        for (int w = 1; w < 8; ++w) m = fmaxf(m, scratch[w * 64 + tid]);
        pf_max = m;
      }
    }
    f32x16 acc[1][1] = {{zero16()}};
    g2.run(acc, pf + nb2 * 32 * LD64, LD64, lane);
    store_tile_lds_pre<1, 1, true, true>(acc, a2 + nb2 * 32 * 128, 128, mblk2 * 32, bv2, lane);
  }
  __syncthreads();
  TRUNK_STAMP(3);
  if (SAVE) save_tile_rows<128, 512, true>(a2, 128, sv.s3 + trow0 * 128, tid);
  // conv4 512->1024: wave owns MB4 m-blocks from mb0 (RS = 1: out channels [wave*128, +128)); first weight chunks +
  // bias requested now
  // RS = 8 (a single object): four m-blocks per workgroup, wave -> (m-block wave / 2, point block wave % 2); the two point
  // blocks' maxima of a channel meet in LDS before the store (max is exact: same result)
  constexpr int MB4 = RS == 8 ? 1 : 4 / RS, NB4 = RS == 8 ? 1 : 2;
  const int mb0 = RS == 8 ? part * 4 + (wave >> 1) : part * (32 / RS) + wave * MB4;
  GemmPipe<MB4, NB4, true, true, 64, RS == 1 ? 2 : 3, 1> g4;
  g4.prefetch(wp4 + ((size_t)mb0 * 64) * 64 + lane, 64 * 64);
  float bl4[MB4];
  load_bias_lane<MB4>(bl4, b4, mb0 * 32, lane);
  __builtin_amdgcn_sched_barrier(0);
  {
    f32x16 acc3[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) acc3[mb][0] = acc3[mb][1] = zero16();
    g3.run(acc3, a2, 128, lane);
    store_tile_lds_pre<2, 2, true, true>(acc3, a3, 512, wave * 64, bv3, lane);
    TRUNK_STAMP(4);
  }
  __syncthreads();
  TRUNK_STAMP(5);
  {  // deferred stores of the pointfeat tile (point-major [cloud points][64], coalesced 16 KiB) and its max
    float* dstbase = pointfeat + (ti.is_obs ? ((size_t)ti.obj * N + ti.p0) * 64
                                            : ((size_t)B * N + (size_t)ti.obj * M + ti.p0) * 64);
    if (part == 0 && pf_row < ti.valid) {
      f32x4* d = reinterpret_cast<f32x4*>(dstbase + pf_row * 64);
      d[pf_c4] = pf_out0;
      d[pf_c4 + 8] = pf_out1;
    }
    if (part == 0 && tid < 64) pm[(size_t)tile * PMW + 1024 + tid] = pf_max;
  }
  if (SAVE) save_tile_rows<512, 512, true>(a3, 512, sv.s4 + trow0 * 512, tid);
  f32x16 acc4[MB4][NB4];
#pragma unroll
  for (int mb = 0; mb < MB4; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB4; ++nb) acc4[mb][nb] = zero16();
  g4.run(acc4, a3 + (RS == 8 ? (wave & 1) * 32 * 512 : 0), 512, lane);
  TRUNK_STAMP(6);
  if constexpr (RS == 8) {
    float m = acc4[0][0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) m = fmaxf(m, acc4[0][0][r]);
    m = fmaxf(m, __shfl_xor(m, 32));
    float* xch = a2 + (wave >> 1) * 32;  // a2 is dead since the barrier after conv3
    if ((wave & 1) && lane < 32) xch[lane] = m;
    __syncthreads();
    if (!(wave & 1) && lane < 32) pm[(size_t)tile * PMW + mb0 * 32 + lane] = fmaxf(m, xch[lane]) + bl4[0];
  } else if constexpr (SAVE) {
    argmax_tile_store<MB4, 2>(acc4, sv.pmax + (size_t)tile * 1024, sv.pidx + (size_t)tile * 1024, mb0 * 32, bl4,
                              (int)trow0, lane);
  } else {
    max_tile_store_pre<MB4, 2>(acc4, pm + (size_t)tile * PMW, mb0 * 32, bl4, false, lane);
  }
  TRUNK_STAMP(7);
#undef TRUNK_STAMP
}

// ------------------------------------------------------------------------------------------
// The trunk for grids that fill the chip (one workgroup per tile): 256 threads = ONE wave per SIMD, so that a wave may
// hold 512 registers and conv4 becomes an MB8 x NB2 wave tile (256 channels x 64 points = 256 accumulators): every LDS
// fragment feeds 8 MFMAs instead of 4.  The sweep is power-limited, not issue-limited (profiles/ubench/power.hip: the
// 8-wave MB4 x NB2 sweep saturates the matrix pipe and the chip answers with 2.0 GHz, 132-134 TFLOP/s; this form holds
// 2.36 GHz at 147).  Same operands in the same K order as k_trunk for every output element: same bits.
// ------------------------------------------------------------------------------------------
#ifndef TRUNK4_PFD
#define TRUNK4_PFD 2
#endif
#ifndef TRUNK4_PFB
#define TRUNK4_PFB 1
#endif
// conv4 + max-pool of k_trunk4 as a policy of trunk4_body: `prefetch` (first weight chunks + bias, requested behind conv3's
// sweep), `sweep` (after the barrier that completes a3), `store`.  Trunk4Dense is the full fp32 sweep; catre_screen.h adds
// the screened form of the same layer.
template <bool SAVE>
struct Trunk4Dense {
  GemmPipe<8, 2, true, true, 64, TRUNK4_PFD, TRUNK4_PFB> g4;
  float bl4[8];
  f32x16 acc4[8][2];
  __device__ __forceinline__ void prefetch(const f32x4* __restrict__ wp4, const float* __restrict__ b4, int mb0, int lane) {
    g4.prefetch(wp4 + ((size_t)mb0 * 64) * 64 + lane, 64 * 64);
    load_bias_lane<8>(bl4, b4, mb0 * 32, lane);
  }
  __device__ __forceinline__ void sweep(const float* a3, float*, int, int lane) {
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc4[mb][0] = acc4[mb][1] = zero16();
    g4.run(acc4, a3, 512, lane);
  }
  __device__ __forceinline__ void store(const float*, float*, float* __restrict__ pm, int tile, int mb0, int,
                                        int trow0, const TrainSave& sv, int lane) {
    if constexpr (SAVE) {
      argmax_tile_store<8, 2>(acc4, sv.pmax + (size_t)tile * 1024, sv.pidx + (size_t)tile * 1024, mb0 * 32, bl4, trow0, lane);
    } else {
      max_tile_store_pre<8, 2>(acc4, pm + (size_t)tile * PMW, mb0 * 32, bl4, false, lane);
    }
  }
};

template <bool SAVE, class Tail>
__device__ __forceinline__ void trunk4_body(float* smem, catre_points P, const float* __restrict__ trans3,
                                            const float* __restrict__ trans64, const float* __restrict__ Wc1,
                                            const float* __restrict__ bc1, const f32x4* __restrict__ wp2,
                                            const float* __restrict__ b2, const f32x4* __restrict__ wp3,
                                            const float* __restrict__ b3, const f32x4* __restrict__ wp4,
                                            const float* __restrict__ b4, float* __restrict__ pm,
                                            float* __restrict__ pointfeat, int B, int N, int M,
                                            unsigned long long* __restrict__ trace, const TrainSave& sv, Tail& tl,
                                            const int tile, const int tid) {
#define TRUNK_STAMP(i)                                                                     \
  do {                                                                                     \
    if (CATRE_TRACE_ON && trace && lane == 0) trace[((size_t)tile * 8 + wave) * 8 + (i)] = __builtin_readcyclecounter(); \
  } while (0)
  float* h1 = smem;                      // [64][68]
  float* t64 = smem + TP * LD64;         // [64][64]
  float* pf = smem + TP * LD64 + 4096;   // [64][68]
  float* a3 = smem;                      // [64][512] swizzled
  float* a2 = smem + TP * 512;           // [64][128] swizzled
  // (tile, tid): blockIdx.x and threadIdx.x of the one-tile kernels; the run form (k_trunk4sr) walks several tiles
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const TileInfo ti = tile_info(tile, B, N, M);
  const bool ft = trans64 != nullptr;
  TRUNK_STAMP(0);

  // conv2 64->128: wave -> m-block `wave`, both point blocks
  GemmPipe<1, 2, false, false, 8, 3> g2;
  g2.prefetch(wp2 + (wave * 8) * 64 + lane, 0);
  f32x4 bv2[1][4];
  load_bias_quads<1>(bv2, b2, wave * 32, lane);
  const size_t trow0 = (ti.is_obs ? (size_t)ti.obj * N : (size_t)B * N + (size_t)ti.obj * M) + ti.p0;
  {
    float x, y, z;
    load_point(P, ti, lane, x, y, z);
    apply_t3(trans3 + ti.cloud * 9, x, y, z);
    if (SAVE && wave == 0) {
      float* xr = sv.s1 + (trow0 + lane) * 8;
      *reinterpret_cast<f32x4*>(xr) = f32x4{x, y, z, 0.f};
      *reinterpret_cast<f32x4*>(xr + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    conv3_relu_row<16>(x, y, z, Wc1, bc1, wave * 16, h1 + lane * LD64);
    if (ft) {
      const f32x4* src = reinterpret_cast<const f32x4*>(trans64 + (size_t)ti.cloud * 4096);
      f32x4* dst = reinterpret_cast<f32x4*>(t64);
#pragma unroll
      for (int u = 0; u < 4; ++u) dst[tid + 256 * u] = src[tid + 256 * u];
    }
  }
  __syncthreads();
  TRUNK_STAMP(1);
  if (SAVE) save_tile_rows<64, 256, false>(h1, LD64, sv.s2 + trow0 * 64, tid);
  if (ft) {
    {  // pointfeat[j][n] = sum_i T64[i][j] h1[i][n]  (pointnet.py:107-109): 2 m-blocks x 2 point blocks, one per wave
      const int mblk = wave >> 1, nb = wave & 1;
      const int n = lane & 31, h = lane >> 5;
      f32x16 acc = zero16();
      const float* xr = h1 + (nb * 32 + n) * LD64 + 4 * h;
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) {
        const f32x4 bx = *reinterpret_cast<const f32x4*>(xr + kc * 8);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float a = t64[(kc * 8 + 4 * h + s) * 64 + mblk * 32 + n];
          acc = mfma32(a, bx[s], acc);
        }
      }
      f32x16 accs[1][1] = {{acc}};
      store_tile_lds<1, 1, false>(accs, pf + nb * 32 * LD64, LD64, mblk * 32, nullptr, lane);
    }
    __syncthreads();
  } else {
    pf = h1;
  }
  TRUNK_STAMP(2);
  // conv3 128->512: 16 m-blocks, four per wave
  GemmPipe<4, 2, false, true, 16, 2, 1> g3;
  g3.prefetch(wp3 + (wave * 4 * 16) * 64 + lane, 16 * 64);
  f32x4 bv3[4][4];
  load_bias_quads<4>(bv3, b3, wave * 128, lane);
  __builtin_amdgcn_sched_barrier(0);
  f32x4 pf_out[4];
  float pf_max = 0.f;
  {
    // pointfeat tile -> registers now, -> HBM after the last barrier (see k_trunk); 16-byte chunk tid + 256 u of the tile
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + 256 * u;
      pf_out[u] = *reinterpret_cast<const f32x4*>(pf + (i >> 4) * LD64 + (i & 15) * 4);
    }
    {  // max_n pointfeat: wave w reduces points [16w, 16w+16) for channel `lane`, 64 threads merge the 4 partials
      float* scratch = smem + 2 * TP * LD64 + 4096;  // [4][64]
      const float* col = pf + (wave * 16) * LD64 + lane;
      float m = col[0];
#pragma unroll
      for (int p = 1; p < 16; ++p) m = fmaxf(m, col[p * LD64]);
      scratch[wave * 64 + lane] = m;
      __syncthreads();
      if (tid < 64) {
        m = scratch[tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) m = fmaxf(m, scratch[w * 64 + tid]);
        pf_max = m;
      }
    }
    f32x16 acc[1][2] = {{zero16(), zero16()}};
    g2.run(acc, pf, LD64, lane);
    store_tile_lds_pre<1, 2, true, true>(acc, a2, 128, wave * 32, bv2, lane);
  }
  __syncthreads();
  TRUNK_STAMP(3);
  if (SAVE) save_tile_rows<128, 256, true>(a2, 128, sv.s3 + trow0 * 128, tid);
  // conv4 512->1024: wave owns 8 m-blocks (channels [wave*256, +256)); first weight chunks + bias requested now
  const int mb0 = wave * 8;
  {
    f32x16 acc3[4][2];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc3[mb][0] = acc3[mb][1] = zero16();
    g3.run(acc3, a2, 128, lane);
    // conv4's first weight chunks + bias are requested behind conv3's sweep: the L2 round trip hides behind the epilogue
    // and the barrier, and the 64 registers they land in are not live during the sweep
    tl.prefetch(wp4, b4, mb0, lane);
    __builtin_amdgcn_sched_barrier(0);
    store_tile_lds_pre<4, 2, true, true>(acc3, a3, 512, wave * 128, bv3, lane);
    TRUNK_STAMP(4);
  }
  __syncthreads();
  TRUNK_STAMP(5);
  {  // deferred stores of the pointfeat tile (point-major [cloud points][64]: the tile is 16 KiB contiguous) and its max
    float* dstbase = pointfeat + trow0 * 64;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + 256 * u;
      if ((i >> 4) < ti.valid) *reinterpret_cast<f32x4*>(dstbase + (size_t)i * 4) = pf_out[u];
    }
    if (tid < 64) pm[(size_t)tile * PMW + 1024 + tid] = pf_max;
  }
  if (SAVE) save_tile_rows<512, 256, true>(a3, 512, sv.s4 + trow0 * 512, tid);
  tl.sweep(a3, a2, tid, lane);  // (a2 is dead since the barrier: scratch of the screened form)
  TRUNK_STAMP(6);
  tl.store(a3, a2, pm, tile, mb0, ti.valid, (int)trow0, sv, lane);
  TRUNK_STAMP(7);
#undef TRUNK_STAMP
}

template <bool SAVE = false>
__global__ __launch_bounds__(256) void k_trunk4(catre_points P, const float* __restrict__ trans3,
                                                const float* __restrict__ trans64, const float* __restrict__ Wc1,
                                                const float* __restrict__ bc1, const f32x4* __restrict__ wp2,
                                                const float* __restrict__ b2, const f32x4* __restrict__ wp3,
                                                const float* __restrict__ b3, const f32x4* __restrict__ wp4,
                                                const float* __restrict__ b4, float* __restrict__ pm,
                                                float* __restrict__ pointfeat, int B, int N, int M,
                                                unsigned long long* __restrict__ trace, TrainSave sv = TrainSave{}) {
  __shared__ __attribute__((aligned(16))) float smem[TRUNK_SMEM];
  Trunk4Dense<SAVE> tl;
  trunk4_body<SAVE>(smem, P, trans3, trans64, Wc1, bc1, wp2, b2, wp3, b3, wp4, b4, pm, pointfeat, B, N, M, trace, sv, tl,
                    blockIdx.x, threadIdx.x);
}
