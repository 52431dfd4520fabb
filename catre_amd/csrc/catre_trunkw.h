// ------------------------------------------------------------------------------------------
// The dense fp32 trunk at a conv4 width D = PCLNET.INIT_CFG.out_dim in {64, 128, 256, 512, 1024} (pointnet.py:98-116 with
// conv4 = Conv1d(512, D)).  The chain, the LDS plan and every helper are k_trunk<1>'s: x T3 -> relu(conv1) -> pointfeat =
// h1^T T64 -> relu(conv2) -> relu(conv3) stay in LDS (160 KiB), conv4 is one K = 512 sweep per wave with no barrier
// inside, the max-pool is the exact fp32 one (no screen, no bf16 pipe).  One workgroup of 8 waves per 64-point tile.
// conv4's D / 32 m-blocks over the 8 waves:
//   D = 1024, 512, 256: MB = 4, 2, 1 m-blocks per wave, both point blocks (NB = 2)
//   D = 128, 64       : wave -> (m-block wave / 2, point block wave % 2) (NB = 1), as k_trunk<8>; the two point blocks'
//                       maxima of a channel meet in LDS.  D = 64 keeps waves 4..7 out of the sweep by a wave-uniform
//                       branch; they still reach every barrier.
// Every conv4 output element is accumulated from the same operands in the same K order as in k_trunk<1> (GemmPipe's K
// loop does not depend on MB / NB / prefetch depth, and max is exact): the same bits as the shipped kernels' channels
// [0, D) when conv4's first D rows are the same.  The partial-max rows keep the 1088 pitch ([conv max | 64 pointfeat max]
// at column 1024); k_reduce_pm_w gathers them into gfeat [C, D + 64].
// ------------------------------------------------------------------------------------------
#pragma once
#include "catre_enc.h"
template <int MB, int NB>
__global__ __launch_bounds__(512) void k_trunkw(catre_points P, const float* __restrict__ trans3,
                                                const float* __restrict__ trans64, const float* __restrict__ Wc1,
                                                const float* __restrict__ bc1, const f32x4* __restrict__ wp2,
                                                const float* __restrict__ b2, const f32x4* __restrict__ wp3,
                                                const float* __restrict__ b3, const f32x4* __restrict__ wp4,
                                                const float* __restrict__ b4, int nmb4 /* D / 32 */,
                                                float* __restrict__ pm, float* __restrict__ pointfeat, int B, int N,
                                                int M) {
  static_assert(NB == 2 || MB == 1, "the point-block split is the one-m-block form");
  __shared__ __attribute__((aligned(16))) float smem[TRUNK_SMEM];
  // phase-1/2 buffers alias the conv4 input image a3 (dead before a3 is first written), as in k_trunk
  float* h1 = smem;                      // [64][68]
  float* t64 = smem + TP * LD64;         // [64][64]
  float* pf = smem + TP * LD64 + 4096;   // [64][68]
  float* a3 = smem;                      // [64][512] swizzled
  float* a2 = smem + TP * 512;           // [64][128] swizzled
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x;
  const TileInfo ti = tile_info(tile, B, N, M);
  const bool ft = trans64 != nullptr;

  const int mblk2 = wave >> 1, nb2 = wave & 1;
  GemmPipe<1, 1, false, false, 8, 4> g2;
  g2.prefetch(wp2 + (mblk2 * 8) * 64 + lane, 0);
  f32x4 bv2[1][4];
  load_bias_quads<1>(bv2, b2, mblk2 * 32, lane);
  {
    float x, y, z;
    load_point(P, ti, lane, x, y, z);
    apply_t3(trans3 + ti.cloud * 9, x, y, z);
    conv3_relu_row<8>(x, y, z, Wc1, bc1, wave * 8, h1 + lane * LD64);
    if (ft) {
      const f32x4* src = reinterpret_cast<const f32x4*>(trans64 + (size_t)ti.cloud * 4096);
      f32x4* dst = reinterpret_cast<f32x4*>(t64);
      dst[tid] = src[tid];
      dst[tid + 512] = src[tid + 512];
    }
  }
  __syncthreads();
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
    // pointfeat tile -> registers now, -> HBM after the last barrier (see k_trunk)
    if (pf_row < ti.valid) {
      const f32x4* s = reinterpret_cast<const f32x4*>(pf + pf_row * LD64);
      pf_out0 = s[pf_c4];
      pf_out1 = s[pf_c4 + 8];
    }
    {  // max_n pointfeat: wave w reduces points [8w, 8w+8) for channel `lane`, then 64 threads merge the 8 partials
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
  // conv4 512->D: this wave's m-blocks [mb0, mb0 + MB); a wave past the last m-block (D = 64) requests and sweeps nothing
  const int mb0 = NB == 1 ? wave >> 1 : wave * MB;
  const bool sweep = mb0 < nmb4;  // wave-uniform (mb0 + MB <= nmb4 then: nmb4 is a multiple of MB for every launched form)
  GemmPipe<MB, NB, true, true, 64, MB == 4 ? 2 : 3, 1> g4;
  float bl4[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) bl4[mb] = 0.f;
  if (sweep) {
    g4.prefetch(wp4 + ((size_t)mb0 * 64) * 64 + lane, 64 * 64);
    load_bias_lane<MB>(bl4, b4, mb0 * 32, lane);
  }
  __builtin_amdgcn_sched_barrier(0);
  {
    f32x16 acc3[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) acc3[mb][0] = acc3[mb][1] = zero16();
    g3.run(acc3, a2, 128, lane);
    store_tile_lds_pre<2, 2, true, true>(acc3, a3, 512, wave * 64, bv3, lane);
  }
  __syncthreads();
  {  // deferred stores of the pointfeat tile (point-major [cloud points][64], coalesced 16 KiB) and its max
    float* dstbase = pointfeat + (ti.is_obs ? ((size_t)ti.obj * N + ti.p0) * 64
                                            : ((size_t)B * N + (size_t)ti.obj * M + ti.p0) * 64);
    if (pf_row < ti.valid) {
      f32x4* d = reinterpret_cast<f32x4*>(dstbase + pf_row * 64);
      d[pf_c4] = pf_out0;
      d[pf_c4 + 8] = pf_out1;
    }
    if (tid < 64) pm[(size_t)tile * PMW + 1024 + tid] = pf_max;
  }
  f32x16 acc4[MB][NB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc4[mb][nb] = zero16();
  if (sweep) g4.run(acc4, a3 + (NB == 1 ? (wave & 1) * 32 * 512 : 0), 512, lane);
  if constexpr (NB == 1) {
    float m = acc4[0][0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) m = fmaxf(m, acc4[0][0][r]);
    m = fmaxf(m, __shfl_xor(m, 32));
    float* xch = a2 + (wave >> 1) * 32;  // a2 is dead since the barrier after conv3
    if (sweep && (wave & 1) && lane < 32) xch[lane] = m;
    __syncthreads();
    if (sweep && !(wave & 1) && lane < 32) pm[(size_t)tile * PMW + mb0 * 32 + lane] = fmaxf(m, xch[lane]) + bl4[0];
  } else {
    if (sweep) max_tile_store_pre<MB, 2>(acc4, pm + (size_t)tile * PMW, mb0 * 32, bl4, false, lane);
  }
}

// tile partial maxima (pitch 1088, pointfeat maxima at column 1024) -> gfeat [clouds][D + 64] = [max_n conv4 | max_n pointfeat]
__global__ __launch_bounds__(256) void k_reduce_pm_w(const float* __restrict__ pm, float* __restrict__ out, int D, int B,
                                                     int N, int M) {
  const int cloud = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= D + 64) return;
  const int TN = (N + TP - 1) / TP, TM = (M + TP - 1) / TP;
  const int nt = cloud < B ? TN : TM;
  const size_t row0 = cloud < B ? (size_t)cloud * TN : (size_t)B * TN + (size_t)(cloud - B) * TM;
  const float* src = pm + row0 * PMW + (c < D ? c : 1024 + (c - D));
  float m = src[0];
  for (int t = 1; t < nt; ++t) m = fmaxf(m, src[(size_t)t * PMW]);
  out[(size_t)cloud * (D + 64) + c] = m;
}
