// catre_screen.h - exact max-pool of a 1x1-conv layer without computing every output in fp32:
// screen every (channel, point) with the split-bf16 product (catre_split.h, 3/16 of the fp32 MFMA issue), bound its error
// rigorously, and recompute in the fp32 MFMA's own fmaf order only the points the bound cannot rule out.
// Included by catre_kernels.hip after catre_split.h.
//
// The bound
// ---------
// Pooled layer y_c(p) = sum_{k < K} w_ck a_k(p), evaluated today by v_mfma_f32_32x32x2_f32 as an fmaf chain (call the
// result Y).  The screen value S is  sum_k (wh ah + wh al + wl ah)  accumulated in fp32 by v_mfma_f32_32x32x16_bf16, with
// x = xh + xl + rho, xh = bf16(x), xl = bf16(x - xh).  Write u = 2^-24, A = sum_k |w_ck| |a_k(p)| <= ||w_c||_2 ||a(p)||_2.
//   * representation:   |rho| <= 2^-9 2^-9 |x| = 2^-18 |x| for w and for a            -> 2 * 2^-18 A
//   * dropped wl al:    |wl| <= 2^-9 |w| (1 + 2^-9), same for a                        -> 2^-18 A (1 + 2^-8)
//   * screen accumulation: 3K products enter fp32 sums; allowing every add to TRUNCATE (2u relative to a partial sum that
//     never exceeds A (1 + small)), and counting the 17 addends of each of the 3 K/16 MFMAs:  3.19 K 2u A = 3.19 K 2^-23 A
//   * the fp32 chain Y itself: K fused multiply-adds, round to nearest                -> K u A = 0.5 K 2^-23 A
//   * second-order terms ((1 + 2u)^{3.2K} - 1 - 3.2K 2u etc.) are < 2e-4 of the first-order ones for K <= 512.
// Together |Y - S| <= (3 * 2^-18 + 3.7 K 2^-23) A; the code uses
//     gamma_K = 3 * 2^-18 + 4 K 2^-23
// which leaves 8 % of the accumulation term for the second-order terms and the 2^-26 above.
//   * flushed denormals: a bf16 piece, a product or a partial sum below 2^-126 may be flushed to zero on the matrix pipe.
//     Per operand piece that is <= 2^-125 (hi and lo), so sum_k (|w_k| + |a_k|) 2^-125 <= sqrt(K) 2^-125 (||w|| + ||a||),
//     plus <= 7 K 2^-126 for products / partial sums of the three screen products and of the chain.  The code adds
//     delta_K (||w_c|| + ||a(p)|| + 1),  delta_K = K 2^-122, which covers both.
// eps_c(p) = (gamma_K nw_c na_p + delta_K (nw_c + na_p + 1)) * infl with
//   nw_c >= ||w_c||_2 : k_screen_wnorm at pack time, summed in double, rounded up
//   na_p >= ||a(p)||_2: from the fp32 LDS image; fp32 sum of squares (relative error <= K u, a square below 2^-126 may be
//                       lost: <= sqrt(K) 2^-63 absolute), so na_p = sqrt(sum) (1 + 2^-12) + 2^-58
//   infl = 1 + 2^-22 / gamma_K + 2^-20: the selection below evaluates fl(S - eps) and fl(S + eps); each rounding is at most
//         u (|S| + eps), and eps >= gamma_K |y| gives |S| <= eps (1 / gamma_K + 1), so the inflation covers them (and the
//         three roundings of eps itself).
// Not covered: Inf / NaN activations (the dense form gives Inf / NaN there; this form may give a finite other value).
//
// Selection: per (tile, channel) L = max_p fl(S - eps); the candidates are the points with fl(S + eps) >= L.  The true
// maximum's point always is one (Y_max <= S + eps there, and L <= max_p Y).  Points of a ragged tile beyond `valid` are
// copies of the last valid point (load_point clamps) - identical S and eps - and are dropped from the candidate set.
// The tile maximum is fmaxf over the candidates' replayed Y, then bias exactly as max_tile_store_pre.
//
// Run form (kernel-form switch `screen_run`, k_trunk4sr): one workgroup walks consecutive tiles of ONE cloud and carries
// F_c, the exact pre-bias maximum of channel c over the tiles it has finished (-inf before the first).  Tile t selects with
// L = max(F_c, max_p fl(S - eps)), candidates fl(S + eps) >= L.  A dropped point has Y <= fl(S + eps) < L (the roundings are
// inside eps's inflation, as above) and L <= max(F_c, max_p Y): it is not the maximum of the run so far, and
// max(F_c, max over the candidates' Y) is that maximum exactly.  A point that TIES with F_c stays a candidate
// (>=), so the all-ties worst case keeps its size.  The candidate set may now be empty (every point of the tile below
// F_c); the m64 == 0 -> 1 guard remains for the first tile of a run only, where F_c = -inf and only NaN inputs empty it.
// pm[tile] receives fl(F_c + b_c) after the tile: fl(x + b) is monotone in x, so the maximum over a cloud's rows is the
// same float the per-tile maxima give.
//
// Replay: GemmPipe::run feeds output (channel c, point p) the products in the order  kc = 0 .. K/8-1, s = 0 .. 3:
// k = 8 kc + s, then k = 8 kc + 4 + s, starting from 0 - as fmaf (profiles/experiments/screen_mfma_chain.md).
//
// The fp16 screen (kernel-form switch `screen_f16`: ScreenPipeF16, ScreenBoundF16, the k_*16 kernels)
// ---------------------------------------------------------------------------------------------------
// One v_mfma_f32_32x32x16_f16 product instead of the three bf16 ones: a third of the MFMA issue, one weight stream of half
// the bytes, four v_cvt_pk_f16_f32 (RNE) per B fragment instead of the hi / lo split.  Selection, list, replay, running
// maximum and store are the ones above and take eps from this bound; the replay reads the fp32 fragments and the fp32
// image, so the outputs keep their bits.
//   Scaling.  fp16 has a 5-bit exponent, so both operands are moved by exact powers of two:
//     w'_ck = w_ck 2^sw_c, sw_c = min(60, 14 - floor(log2 nw_c))   (pack time, k_pack_screen_f16; uw_c = 2^-sw_c is stored)
//     a'_k(p) = a_k(p) 2^sa, sa = min(60, 14 - floor(log2 max_p na_p))   (one scale per TILE, screen_tile_scale)
//   |w_ck| <= nw_c and nw_c 2^sw_c < 2^15, likewise for a: no element exceeds 2^15 < 65504 after rounding - no overflow, and
//   the largest element of a row is at least 2^14 / sqrt(K).  S' (the accumulator) = 2^(sw + sa) S; the selection evaluates
//   fl(S -+ eps) as fmaf(S', uw_c 2^-sa, -+eps): the product is exact inside the fma (no rounding even where S would be an
//   fp32 denormal), so nothing is rounded outside eps's inflation.  One scale per tile is sound because the selection is
//   absolute; a point far smaller than the tile's largest loses relative accuracy, which delta (below) covers.
//   sw_c < -60 (nw_c >= 2^75, or not finite) or sa < -60 (a row norm >= 2^75 - in effect 2^64, where screen_row_norms' fp32
//   sum of squares becomes inf): the scale cannot keep the operand inside fp16.  Such a channel (uw_c = inf) or tile takes EVERY valid point as a candidate - the replay alone is exact - and its
//   accumulators are ignored.  na_p >= 2^-58 by construction and nw_c = 0 gives sw_c = 60: zero rows need no special case.
//   Rounding.  fp16 carries 11 significant bits: RNE gives |x~ - x'| <= 2^-11 |x'| for a normal result (half an ulp of an
//   11-bit significand - not 2^-12).  A result below 2^-14 (fp16-subnormal) may be rounded to a subnormal, flushed by the
//   conversion or flushed by the matrix pipe; the fp32 multiply by the scale may lose a denormal (2^-126): at most
//   eta = 2^-13 per element on top of the rounding.
//   The weights' rounding is KNOWN at pack time: dw_c = ||fp16(w'_c) - w'_c||_2 2^-sw_c (k_screen_f16_dw, summed in double,
//   rounded up) replaces the worst case 2^-11 nw_c - it measures 0.42 of it on the recipe weights.  The activations' is taken at its
//   worst case here and measured per tile under `screen_da` (next section).  With w~ = w' + dw + zeta_w, a~ = a' (1 + theta) + zeta_a, |theta| <=
//   2^-11, |zeta| <= eta, A' = sum_k |w'| |a'| <= nw' na':
//     * products:  sum_k |w~ a~ - w' a'| <= (1 + 2^-11) dw' na' + 2^-11 nw' na' + eta (1 + 2^-10) sqrt(K) (nw' + na'(p)) + K eta^2
//     * w~ a~ is exact in fp32 (22 significant bits) and, where not zero, >= 2^-48: no fp32 underflow in the screen's sums
//     * screen accumulation: K products, every add may truncate, 17 addends per MFMA:  (17 / 16) K 2u A~, A~ <= A'(1 + 2^-9) + ..
//     * the fp32 chain Y itself: K u A, and <= K 2^-126 where an fmaf result is flushed
//   gamma_K = 2^-11 + 2^-21 + 2 K 2^-23  (1.5625 K 2^-23 of accumulation is needed: 28 % left for the second-order terms),
//   and in the units of S:  delta = 2^-12 sqrt(K) (nw_c 2^-sa + na_p uw_c) + K 2^-24 uw_c 2^-sa + K 2^-122, so
//     eps_c(p) = ((gamma_K nw_c + (1 + 2^-10) dw_c + rk uw_c) na_p + rk nw_c 2^-sa + K 2^-24 uw_c 2^-sa + K 2^-122) * infl
//   with rk >= 2^-12 sqrt(K)  (2^-sa <= 2^-14 max_p na_p and uw_c <= 2^-14 nw_c unless clamped: delta is ~ 3e-4 of the gamma
//   term for the tile's largest point).  infl as above with 2^-19 for the roundings of eps's own operations.
//   An eps that overflows to +inf makes every point a candidate, as it must.
//
// The measured bound (switch `screen_da`, its STN arm `screen_da_stn`: a runtime flag of the same fp16-screen kernels)
// --------------------------------------------------------------------------------------------------------------------
// Two terms of the product error above are replaced by what the operands actually are; accumulation, the chain's own K u,
// eta, delta and the unscalable regime keep their constants.
//   Activations.  screen_row_norms already reads every element of the fp32 image once per tile; in the same pass it forms
//     r_k = a_k - rne11(a_k)      (screen_rne11_err: a_k rounded to 11 significant bits, unbounded exponent)
//   in integer arithmetic - add half an 11-bit ulp to the magnitude, drop 13 bits - and one exact fp32 subtraction: a_k - hi
//   is a multiple of ulp(a_k) of at most 2^12 ulps, so it is representable; nothing can overflow while the row norms are
//   below 2^64, which the scalable regime implies (a carry out of the largest exponent needs |a_k| >= 2^127).  A tie goes
//   away from zero where v_cvt goes to even: the same |r_k|.  The tile scale 2^sa is a power of two and commutes with the
//   rounding unless the scaled element falls below 2^-14 (fp16-subnormal, flushed, or an fp32 denormal): for such an
//   element |a~_k - a'_k| <= eta whatever r_k measured, and eta sqrt(K) is in delta already.  So with
//     da_p = sqrt(fl sum_k r_k^2) (1 + 2^-12)      (the fp32 sum: K u relative; a square below 2^-126 may be lost:
//                                                   <= sqrt(K) 2^-63 <= 2^-58 absolute on da_p, carried as 2^-58 nw_c in e0)
//     ||a~ - a'||_2 <= 2^sa (da_p + 2^-58) + eta sqrt(K),  and always ||rne11(a') - a'||_2 <= 2^-11 na'
//   the term 2^-11 nw' na' becomes nw' da'.  Per tile rho_t = min(2^-11, max_p da_p / na_p) rounded up (screen_tile_rho; the
//   division and the product: 1 + 2^-20), one scalar register across the sweep like sa, and
//     gamma = rho_t + 2^-21 + 2 K 2^-23       (rho_t = 2^-11: the shipped gamma bit for bit)
//   A per-point da_p in eps would cost a seventh instruction on each of the 256 accumulators; how far a point's own
//   da_p / na_p sits below its tile's maximum on the recipe inputs is printed by tests/test_screen_da_host.py.
//   Weights.  The three pooled layers read images written behind ReLU (a3 of the trunk, the conv2 images of both STNs:
//   store_tile_lds_pre<.., RELU = true>), and fp16 rounding keeps the sign: a~_k >= 0.  With dW = fp16(w') - w' split into
//   its positive and negative parts,
//     |sum_k dW_k a~_k| = |sum_k dW^+_k a~_k - sum_k dW^-_k a~_k| <= max(||dW^+||, ||dW^-||) ||a~||  =: dws' ||a~||
//   (both sums are >= 0, each <= its norm times ||a~||).  dws_c is known at pack time (k_screen_f16_dw, behind dw in the
//   uw table) and measures 0.74 - 0.77 of dw_c on the recipe weights.  A layer whose image may hold negative elements must
//   keep dw (tests/test_screen_da_host.py shows the violation); there is none among the screened layers.
//   Together, for the scaled operands:
//     sum_k |w~ a~ - w' a'| <= nw' da' + (1 + 2^-11) dws' na' + eta (1 + 2^-10) sqrt(K) (nw' + na') + K eta^2
//     e1 = ((rho_t + 2^-21 + 2 K 2^-23) nw_c + (1 + 2^-10) dws_c + rk uw_c) infl,   eps = fmaf(e1, na_p, e0)
//   infl divides by gamma: eps >= gamma |y| must hold for the smallest gamma that can occur, rho_t = 0, so
//   infl = 1 + 2^-22 / (2^-21 + 2 K 2^-23) + 2^-18  (the rounding of rho_t + gamma0 is the extra 2^-19).
//   Off: rho_t = 2^-11, dw for dws, the shipped infl and no measuring - the candidate sets of the parent, bit for bit.
#pragma once
#include "catre_split.h"

template <int K>
struct ScreenBound {
  static constexpr float gamma = 3.f * 0x1p-18f + 4.f * K * 0x1p-23f;
  static constexpr float delta = K * 0x1p-122f;
  static constexpr float infl = 1.f + 0x1p-22f / gamma + 0x1p-20f;
};
// eps = fmaf(e1, na, e0) with the per-channel pair (e1, e0)
template <int K>
__device__ __forceinline__ void screen_eps_coef(float nw, float& e1, float& e0) {
  e1 = fmaf(ScreenBound<K>::gamma, nw, ScreenBound<K>::delta) * ScreenBound<K>::infl;
  e0 = ScreenBound<K>::delta * (nw + 1.f) * ScreenBound<K>::infl;
}

// the fp16 screen's bound (see the header)
template <int K>
struct ScreenBoundF16 {
  static_assert(K == 128 || K == 512, "rk is tabulated");
  static constexpr float gamma = 0x1p-11f + 0x1p-21f + 2.f * K * 0x1p-23f;
  static constexpr float rk = (K == 128 ? 11.32f : 22.63f) * 0x1p-12f;  // >= 2^-12 sqrt(K)
  static constexpr float infl = 1.f + 0x1p-22f / gamma + 0x1p-19f;
  // `screen_da`: gamma = rho_t + gamma0 with the tile's measured rho_t in [0, 2^-11] (rho_t = 2^-11 gives `gamma` bit for
  // bit); the inflation for the smallest gamma that can occur, rho_t = 0, and one rounding more (the sum rho_t + gamma0)
  static constexpr float gamma0 = 0x1p-21f + 2.f * K * 0x1p-23f;
  static constexpr float infl_da = 1.f + 0x1p-22f / gamma0 + 0x1p-18f;
  static_assert(0x1p-11f + gamma0 == gamma, "switch off: the shipped gamma");
};
// eps = fmaf(e1, na, e0); uw = 2^-sw_c (k_pack_screen_f16), dw = the row's rounding error (k_screen_f16_dw), ua = 2^-sa
// (screen_tile_scale).  `screen_da` (da, wave-uniform): rho = the tile's measured rho_t (screen_tile_rho) and dw = the row's
// sign-split error dws_c; off: rho = 2^-11 and dw = dw_c, the shipped eps bit for bit.
template <int K>
__device__ __forceinline__ void screen_eps_coef_f16(float nw, float uw, float dw, float ua, float rho, bool da, float& e1,
                                                    float& e0) {
  typedef ScreenBoundF16<K> SB;
  const float infl = da ? SB::infl_da : SB::infl;
  e1 = fmaf(rho + SB::gamma0, nw, fmaf(1.f + 0x1p-10f, dw, SB::rk * uw)) * infl;
  float t = fmaf(K * 0x1p-24f * uw, ua, K * 0x1p-122f);
  if (da) t = fmaf(0x1p-58f, nw, t);  // squares below 2^-126 the measuring sum lost: <= sqrt(K) 2^-63 on da_p
  e0 = fmaf(SB::rk * nw, ua, t) * infl;
}
// scale exponent of an operand whose norm bound is n: n 2^s in [2^14, 2^15), at most 60; below -60 the operand cannot be
// kept inside fp16 (also n = inf / NaN)
__device__ __forceinline__ int screen_f16_exp(float n) {
  const int s = 14 - ((int)((__float_as_uint(n) >> 23) & 0xff) - 127);
  return s > 60 ? 60 : s;
}
__device__ __forceinline__ float screen_pow2(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }  // |e| <= 126

// nw[row] >= ||W[row][0:K]||_2: one wave per row, double accumulation, rounded up
__global__ __launch_bounds__(256) void k_screen_wnorm(const float* __restrict__ W, int ld, int rows, int K,
                                                      float* __restrict__ nw) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  double s = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double w = W[(size_t)row * ld + k];
    s += w * w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) nw[row] = (float)sqrt(s) * (1.f + 0x1p-21f);
}

// The fp16 screen's weights: row-scaled fp16 fragments in the layout of the bf16 hi fragments (u32x4 index
// (mb (K / 16) + kc) 64 + lane: row 32 mb + (lane & 31), the 8 values k = 16 kc + 8 (e >> 2) + 4 (lane >> 5) + (e & 3)), and
// uw[row] = 2^-sw_row (inf: the row cannot be scaled into fp16, its channel takes every point as a candidate).
// After k_screen_wnorm of the same rows.
__global__ __launch_bounds__(256) void k_pack_screen_f16(const float* __restrict__ W, int ld, int rows, int K,
                                                         const float* __restrict__ nw, unsigned short* __restrict__ dst,
                                                         float* __restrict__ uw) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * K) return;
  const int e = idx & 7, lane = (idx >> 3) & 63, rest = idx >> 9;
  const int nkc = K / 16;
  const int kc = rest % nkc, mb = rest / nkc;
  const int row = mb * 32 + (lane & 31), col = kc * 16 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
  const int sw = screen_f16_exp(nw[row]);
  const bool bad = sw < -60;
  const float w = bad ? 0.f : W[(size_t)row * ld + col] * screen_pow2(sw);
  dst[idx] = __builtin_bit_cast(unsigned short, (_Float16)w);  // RNE
  if (col == 0) uw[row] = bad ? INFINITY : screen_pow2(-sw);
}

// dw[row] >= ||fp16(w') - w'||_2 2^-sw of the row as k_pack_screen_f16 rounds it: one wave per row, double accumulation,
// rounded up (0 for a row that cannot be scaled: its channel takes every point).
// dws[row] >= max(||dW^+||_2, ||dW^-||_2) 2^-sw, dW^+ / dW^- the positive / negative parts of the same rounding errors
// (`screen_da`): against an image with no negative element, |sum_k dW_k a_k| <= max(sum_k dW^+_k a_k, sum_k dW^-_k a_k).
__global__ __launch_bounds__(256) void k_screen_f16_dw(const float* __restrict__ W, int ld, int rows, int K,
                                                       const float* __restrict__ nw, float* __restrict__ dw,
                                                       float* __restrict__ dws) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int sw = screen_f16_exp(nw[row]);
  double s = 0.0, sp = 0.0, sn = 0.0;
  if (sw >= -60) {
    const float f = screen_pow2(sw);
    for (int k = lane; k < K; k += 64) {
      const float w = W[(size_t)row * ld + k] * f;
      const double r = (double)w - (double)(float)(_Float16)w;
      s += r * r;
      if (r > 0.0)
        sp += r * r;
      else
        sn += r * r;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    sp += __shfl_xor(sp, o);
    sn += __shfl_xor(sn, o);
  }
  if (lane == 0) {
    dw[row] = sw >= -60 ? (float)(sqrt(s) * (double)screen_pow2(-sw)) * (1.f + 0x1p-21f) : 0.f;
    dws[row] = sw >= -60 ? (float)(sqrt(sp > sn ? sp : sn) * (double)screen_pow2(-sw)) * (1.f + 0x1p-21f) : 0.f;
  }
}

struct ScreenArgs {
  const u32x4* wps;   // hi fragments of the layer ([mb][K/16][lane]), lo fragments rows*K/8 further (k_pack_frag_lp_multi<true>)
                      // fp16 screen: the scaled fp16 fragments (k_pack_screen_f16)
  const float* nw;    // [rows] weight-row norms (k_screen_wnorm)
  float* probe_s;     // tests only (catre_trunk_screen_probe): [tile][channel][point] screen value and bound, or NULL
  float* probe_eps;
  const float* uw;    // fp16 screen: [rows] 2^-sw (k_pack_screen_f16), then [rows] dw and [rows] dws (k_screen_f16_dw)
  int da;             // fp16 screen: `screen_da` - the activations' rounding measured per tile, the sign-split dws for dw
};

#ifdef CATRE_DEBUG_TRACE
// diagnostic build, one row per screened layer (0 trunk conv4, 1 stn conv3, 2 fstn conv3): [0..31] candidates per
// (tile, channel) (31: >= 31), [32..47] trips per (wave, tile, m-block) (47: >= 15), [48] (wave, tile) units with an
// m-block of more than SCREEN_CMAX trips, [49] all units.  Pooled form: [32..47] rounds of 64 entries per (wave, tile),
// [48] units that needed more than one batch, [50] sum of entries, [51] sum of rounds, [52] units with an empty list (run form)
__device__ unsigned long long g_screen_cnt[3][64];
// counting on / off (catre_debug_knob 2): the counters' atomics cost far more than the epilogue they count in, so the
// phase stamps of profiles/trace_trunk.py are taken with them off
__device__ int g_screen_count_on = 1;
#define SCREEN_COUNT(layer, bin, v)                                        \
  do {                                                                     \
    if (g_screen_count_on) atomicAdd(&g_screen_cnt[layer][bin], (unsigned long long)(v)); \
  } while (0)
#endif

#define SCREEN_CMAX 4  // replay chains a lane carries at once; an m-block that needs more trips takes further rounds

// Lane exchanges with the caller's OWN lane id: __shfl_xor / __shfl_up / __shfl compute the lane id themselves, a value the
// compiler hoists out of k_trunk4sr's loop over tiles - and then it is live across the 256-accumulator sweep and spills.
// (`lane` may carry higher bits, e.g. a thread id: ds_bpermute takes the address modulo the wave.)
template <class T>
__device__ __forceinline__ T lane_get(T v, int src_lane) {
  return __builtin_bit_cast(T, __builtin_amdgcn_ds_bpermute(src_lane << 2, __builtin_bit_cast(int, v)));
}

// Inclusive prefix sum over the wave's 64 lanes on the DPP path: four row_shr steps inside each row of 16 lanes, then
// row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3.  No LDS round trip and no lane id; every lane active.
__device__ __forceinline__ int wave_prefix_incl(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}

// Sub-phase stamps of the screened epilogue, instrumented build only (profiles/trace_screen_epi.py; catre_debug_knob 3
// turns them on): the buffer of catre_debug_trunk_trace, layer L at offset L << 22, [tile][8][8] like the trunk's stamps, wave w in the unused row 4 + w:
// [0] entry, [1] behind the selection, [2] behind the list build, [3] behind the replay, [4] behind the scan, [5] end
// (the last batch's, where a list filled up).  The buffer holds 1 << 24 entries in front of the rotation heads' stamps.
#ifdef CATRE_DEBUG_TRACE
__device__ unsigned long long* g_screen_trace = nullptr;
#define SCREEN_STAMP(layer, tile, wave, i)                                                                    \
  do {                                                                                                        \
    unsigned long long* t_ = g_screen_trace;                                                                  \
    if (t_ && lane == 0 && (tile) < (1 << 16))                                                                \
      t_[((size_t)(layer) << 22) + ((size_t)(tile) * 8 + 4 + (wave)) * 8 + (i)] = __builtin_readcyclecounter(); \
  } while (0)
#else
#define SCREEN_STAMP(layer, tile, wave, i) \
  do {                                     \
  } while (0)
#endif

// Row addressing of the fp32 LDS image a screened layer reads: SWZ = the XOR-swizzled [rows][C] image of the trunk (pitch
// C, chunk c of row r at c ^ (r & 15)), otherwise a padded image of pitch `ld` (the STN kernels' [128][LD128]).
// ||a(p)||_2 (rounded up) of the ROWS rows of the image -> na[ROWS]; NT threads, NT/ROWS per row
// `screen_da` (da, workgroup-uniform; rho = LDS [ROWS]): the same pass also measures the fp16 rounding of every element,
// r = x - rne11(x) (screen_rne11_err), and leaves rho[row] >= ||r||_2 / na[row] (see the header; screen_tile_rho reduces it)
__device__ __forceinline__ float screen_rne11_err(float x) {
  // x rounded to 11 significant bits by dropping 13 of the 24 (half an 11-bit ulp added to the magnitude first: a tie
  // goes away from zero where v_cvt_pk_f16_f32 goes to even - the same distance); a carry moves into the exponent
  // field as it should.  x - hi is a multiple of ulp(x) of at most 2^12 ulps: the subtraction is exact.
  return x - __uint_as_float((__float_as_uint(x) + 0x1000u) & 0xffffe000u);
}
template <int C, int NT, int ROWS = 64, bool SWZ = true>
__device__ __forceinline__ void screen_row_norms(const float* __restrict__ img, float* __restrict__ na, int tid, int ld = C,
                                                 bool da = false, float* __restrict__ rho = nullptr) {
  constexpr int PER = NT / ROWS, CH = C / 4 / PER;  // chunks of 4 floats per thread
  static_assert(CH % 16 == 0, "a thread's chunks are whole swizzle groups");
  const int row = tid / PER, part = tid % PER;
  const float* r = img + row * ld + part * CH * 4;
  const int key = SWZ ? row & 15 : 0;
  float s = 0.f;
  if (da) {
    float d = 0.f;
#pragma unroll 8
    for (int j = 0; j < CH; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(r + ((j ^ key) << 2));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float e = screen_rne11_err(v[q]);
        s = fmaf(v[q], v[q], s);
        d = fmaf(e, e, d);
      }
    }
#pragma unroll
    for (int o = 1; o < PER; o <<= 1) {
      s += lane_get(s, tid ^ o);
      d += lane_get(d, tid ^ o);
    }
    if (part == 0) {
      const float n = fmaf(sqrtf(s), 1.f + 0x1p-12f, 0x1p-58f);
      na[row] = n;
      // (1 + 2^-12) as for na: the fp32 sum's K u and the square root; 2^-20: the division and the product
      rho[row] = sqrtf(d) * (1.f + 0x1p-12f) / n * (1.f + 0x1p-20f);
    }
    return;
  }
#pragma unroll 8
  for (int j = 0; j < CH; ++j) {  // physical chunk j ^ (row & 15): the 16 rows of a lane group hit 16 distinct bank slots
    const f32x4 v = *reinterpret_cast<const f32x4*>(r + ((j ^ key) << 2));
    s = fmaf(v[0], v[0], s);
    s = fmaf(v[1], v[1], s);
    s = fmaf(v[2], v[2], s);
    s = fmaf(v[3], v[3], s);
  }
#pragma unroll
  for (int o = 1; o < PER; o <<= 1) s += lane_get(s, tid ^ o);
  if (part == 0) na[row] = fmaf(sqrtf(s), 1.f + 0x1p-12f, 0x1p-58f);
}

// The screen sweep of an MB8 x NB2 wave tile over K = 16 NKC: split-bf16 A fragments from the pack, B fragments split in
// registers from the fp32 LDS image - the trunk's swizzled [64][512] (there is no LDS left for hi / lo images beside it) or
// a padded [64][LD] one (SWZ = false).
// The weight ring works on HALF chunks (4 m-blocks x K=16: 24 MFMAs = 768 cycles), PFD of them in flight.
template <int PFD, int NKC_ = 32, bool SWZ = true, int LD = 512>
struct ScreenPipe8 {
  static constexpr int NKC = NKC_, NT = 2 * NKC, RA = PFD + 1, LO = 1024 * (16 * NKC) / 8;
  u32x4 ah[RA][4], al[RA][4];
  const u32x4* wp;

  __device__ __forceinline__ void issue_a(int t) {
    const int kc = t >> 1, half = t & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      ah[t % RA][m] = wp[((half * 4 + m) * NKC + kc) * 64];
      al[t % RA][m] = wp[LO + ((half * 4 + m) * NKC + kc) * 64];
    }
  }
  __device__ __forceinline__ void prefetch(const u32x4* __restrict__ wp_) {
    wp = wp_;
    // the caller's previous layer is still in its epilogue: PFD - 1 slots now (PFD = 2: one slot, 8 u32x4 = 32
    // registers; the whole ring of RA = 3 slots is 96), the last one at the head of run()
#pragma unroll
    for (int d = 0; d < PFD - 1; ++d) issue_a(d);
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void run(f32x16 (&acc)[8][2], const float* x, int lane) {
    const int n = lane & 31, h = lane >> 5, sw = lane & 15;
    const float* xrow = x + n * LD;
    // k-slot order of the bf16 fragments: element e of lane half h is k = 16 kc + 8 (e >> 2) + 4 h + (e & 3), i.e. the fp32
    // chunks 4 kc + h and 4 kc + 2 + h of the row; the XOR touches the low four chunk bits only (see GemmPipe::run)
    // (padded image: one row pointer, the chunk offsets are immediates)
    const float* xlow[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 2; ++j) xlow[q][j] = SWZ ? xrow + (((4 * q + 2 * j + h) ^ sw) << 2) : xrow + ((2 * j + h) << 2);
    f32x4 braw[2][2];
    u32x4 bh[2][2], bl[2][2];  // [chunk parity][nb]
    auto issue_b = [&](int kc) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          braw[nb][j] = *reinterpret_cast<const f32x4*>((SWZ ? xlow[kc & 3][j] + (kc >> 2) * 64 : xlow[0][j] + kc * 16) +
                                                        nb * 32 * LD);
    };
    auto split_b = [&](int kc) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float v[8] = {braw[nb][0][0], braw[nb][0][1], braw[nb][0][2], braw[nb][0][3],
                            braw[nb][1][0], braw[nb][1][1], braw[nb][1][2], braw[nb][1][3]};
        split_bf8(v, bh[kc & 1][nb], bl[kc & 1][nb]);
      }
    };
    issue_a(PFD - 1);
    issue_b(0);
    split_b(0);
    issue_b(1);
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = 2 * kc + half;
        if (t + PFD < NT) issue_a(t + PFD);
        __builtin_amdgcn_sched_barrier(0);
        // second half: the split of the NEXT chunk's B fragments (~50 VALU ops) rides between this half's MFMAs - issued in
        // one block ahead of them it would leave the matrix pipe idle for its whole length
        if (half == 1 && kc + 1 < NKC) split_b(kc + 1);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            f32x16& c = acc[half * 4 + m][nb];
            c = mfma_bf(bh[kc & 1][nb], al[t % RA][m], c);
            c = mfma_bf(bl[kc & 1][nb], ah[t % RA][m], c);
            c = mfma_bf(bh[kc & 1][nb], ah[t % RA][m], c);
          }
        if (half == 1 && kc + 1 < NKC) {
#pragma unroll
          for (int g = 0; g < 24; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);  // up to three VALU ops behind it
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (half == 1 && kc + 2 < NKC) issue_b(kc + 2);  // braw is free again
      }
    }
  }
};

// fp16 screen: the tile's scale exponent sa from the row norms na[0 .. 64) (LDS), wave-uniform in a scalar register:
// max_p na_p 2^sa in [2^14, 2^15), sa <= 60; -61: the tile cannot be scaled into fp16 (a norm >= 2^75 or not finite)
__device__ __forceinline__ int screen_tile_scale(const float* na, int lane) {
  float m = na[lane & 63];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, lane_get(m, lane ^ o));
  const int s = screen_f16_exp(m);
  return __builtin_amdgcn_readfirstlane(s < -61 ? -61 : s);
}

// `screen_da`: rho_t = min(2^-11, max_p rho[p]) of the tile's 64 rows (screen_row_norms), wave-uniform in a scalar register
// across the sweep like sa; off: 2^-11, the worst case, and rho is not read.  (A NaN row - inputs outside the contract - is
// skipped by fmaxf, all NaN gives 2^-11.)
__device__ __forceinline__ float screen_tile_rho(const float* rho, int lane, bool da) {
  float m = 0x1p-11f;
  if (da) {
    m = rho[lane & 63];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, lane_get(m, lane ^ o));
    m = fminf(m, 0x1p-11f);
  }
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, m)));
}

// The fp16 sweep of the same MB8 x NB2 wave tile: ONE product per (m-block, n-block, K = 16 chunk), one weight stream
// (k_pack_screen_f16), B fragments scaled by 2^sa and rounded to fp16 (RNE) in registers from the same fp32 LDS image.
// The weight ring works on half chunks as ScreenPipe8's (4 m-blocks x K = 16: now 8 MFMAs = 256 cycles, 16 registers a
// slot), PFD of them in flight - the registers of the lo stream and of the lo B fragments went into its depth: the L2
// stream is this sweep's bound.  PRE slots are requested by prefetch() (behind the caller's previous layer, whose epilogue
// has the registers for no more), the rest at the head of run().
template <int PFD, int PRE, int NKC_ = 32, bool SWZ = true, int LD = 512>
struct ScreenPipeF16 {
  static constexpr int NKC = NKC_, NT = 2 * NKC, RA = PFD + 1;
  static_assert(PRE <= PFD && PFD < NT, "ring");
  u32x4 ah[RA][4];
  const u32x4* wp;

  __device__ __forceinline__ void issue_a(int t) {
    const int kc = t >> 1, half = t & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m) ah[t % RA][m] = wp[((half * 4 + m) * NKC + kc) * 64];
  }
  __device__ __forceinline__ void prefetch(const u32x4* __restrict__ wp_) {
    wp = wp_;
#pragma unroll
    for (int d = 0; d < PRE; ++d) issue_a(d);
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void run(f32x16 (&acc)[8][2], const float* x, int lane, int sa) {
    const int n = lane & 31, h = lane >> 5, sw = lane & 15;
    const float fs = screen_pow2(sa < -60 ? -60 : sa);
    const float* xrow = x + n * LD;
    // the k-slot order and the addressing of ScreenPipe8::run
    const float* xlow[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 2; ++j) xlow[q][j] = SWZ ? xrow + (((4 * q + 2 * j + h) ^ sw) << 2) : xrow + ((2 * j + h) << 2);
    f32x4 braw[2][2];
    u32x4 bh[2][2];  // [chunk parity][nb]
    auto issue_b = [&](int kc) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          braw[nb][j] = *reinterpret_cast<const f32x4*>((SWZ ? xlow[kc & 3][j] + (kc >> 2) * 64 : xlow[0][j] + kc * 16) +
                                                        nb * 32 * LD);
    };
    auto cvt_b = [&](int kc) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float v[8] = {braw[nb][0][0] * fs, braw[nb][0][1] * fs, braw[nb][0][2] * fs, braw[nb][0][3] * fs,
                            braw[nb][1][0] * fs, braw[nb][1][1] * fs, braw[nb][1][2] * fs, braw[nb][1][3] * fs};
        bh[kc & 1][nb] = pack8<OpF16>(v);
      }
    };
#pragma unroll
    for (int d = PRE; d < PFD; ++d) issue_a(d);
    issue_b(0);
    cvt_b(0);
    issue_b(1);
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = 2 * kc + half;
        if (t + PFD < NT) issue_a(t + PFD);
        __builtin_amdgcn_sched_barrier(0);
        // second half: scaling and conversion of the NEXT chunk's B fragments (24 VALU ops) ride between this half's MFMAs
        if (half == 1 && kc + 1 < NKC) cvt_b(kc + 1);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            f32x16& c = acc[half * 4 + m][nb];
            c = OpF16::mfma(bh[kc & 1][nb], ah[t % RA][m], c);
          }
        if (half == 1 && kc + 1 < NKC) {
#pragma unroll
          for (int g = 0; g < 8; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);  // up to three VALU ops behind it
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (half == 1 && kc + 2 < NKC) issue_b(kc + 2);  // braw is free again
      }
    }
  }
};

// 16 weight quads = 8 fp32 chunks kc of one channel row: [2 kc] = k 8kc .. 8kc+3, [2 kc + 1] = k 8kc+4 .. 8kc+7
__device__ __forceinline__ void screen_load_w(f32x4 (&wb)[16], const f32x4* __restrict__ w) {
#pragma unroll
  for (int kc = 0; kc < 8; ++kc) {
    wb[2 * kc] = w[kc * 64];
    wb[2 * kc + 1] = w[kc * 64 + 32];
  }
}

// Replay of T outputs of ONE channel (this lane's) at points p[0..T): the fmaf chain of GemmPipe::run over K = 8 NKC8 * 8.
//   w    : fp32 fragment image of the channel's m-block, + (lane & 31)   (float4 (kc * 64 + 32 h') = k 8kc + 4h' ..)
//   wb   : wb[0] holds the first 8 chunks on entry (requested by the previous call); on exit it holds those of `wnext`
//   x    : fp32 LDS image [64][ld], swizzled or padded (SWZ)
// returns the maximum of the T results
template <int T, int NKC8, bool SWZ = true>
__device__ __forceinline__ float screen_replay(const f32x4* __restrict__ w, const f32x4* __restrict__ wnext,
                                               f32x4 (&wb)[2][16], const float* x, int ld, const int (&p)[SCREEN_CMAX]) {
  static_assert(NKC8 % 2 == 0 && (T == 1 || T == 2 || T == 4), "two blocks of 8 chunks per trip");
  // LDS rows are read one STAGE (SB chunks of every chain: 8 float4) ahead of their use, the weights one block of 8
  // chunks ahead; both pinned where they are issued - left alone the compiler hoists a whole block's reads (256 registers)
  constexpr int SB = 4 / T, NS = 8 / SB;
  float y[T];
  const float* row[T];
  int key[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    y[j] = 0.f;
    row[j] = x + p[j] * ld;
    key[j] = SWZ ? p[j] & 15 : 0;
  }
  f32x4 ab[2][SB][T][2];
  auto load_stage = [&](int buf, int b8, int st) {  // chunks kc = 8 b8 + SB st .. + SB
#pragma unroll
    for (int i = 0; i < SB; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e)
          ab[buf][i][j][e] =
              *reinterpret_cast<const f32x4*>(row[j] + b8 * 64 + (((2 * (SB * st + i) + e) ^ key[j]) << 2));
  };
  auto block = [&](const f32x4 (&wv)[16], int b8, int b8next) {
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      if (st + 1 < NS)
        load_stage((st + 1) & 1, b8, st + 1);
      else
        load_stage(0, b8next, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < SB; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            y[j] = fmaf(wv[2 * (SB * st + i)][s], ab[st & 1][i][j][0][s], y[j]);
            y[j] = fmaf(wv[2 * (SB * st + i) + 1][s], ab[st & 1][i][j][1][s], y[j]);
          }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  load_stage(0, 0, 0);
#pragma unroll 1
  for (int it = 0; it < NKC8 / 2; ++it) {
    screen_load_w(wb[1], w + (2 * it + 1) * 8 * 64);
    __builtin_amdgcn_sched_barrier(0);
    block(wb[0], 2 * it, 2 * it + 1);
    screen_load_w(wb[0], it + 1 < NKC8 / 2 ? w + (2 * it + 2) * 8 * 64 : wnext);
    __builtin_amdgcn_sched_barrier(0);
    block(wb[1], 2 * it + 1, (2 * it + 2) % NKC8);  // (after the last block: a read of block 0 that nothing uses)
  }
  float m = y[0];
#pragma unroll
  for (int j = 1; j < T; ++j) m = fmaxf(m, y[j]);
  return m;
}

// ------------------------------------------------------------------------------------------
// Pooled replay (kernel-form switch `screen_pool`): the wave's 256 channels share ONE list of (channel, point) candidates,
// replayed in rounds of 64 T entries - every lane carries T chains of ANY channels, so no lane idles because its own
// channel has fewer candidates than the worst one of its m-block.  Each chain is the same fmaf chain as screen_replay's.
//
// LDS of a wave (its 4 KiB of candidate sets): [0, 2 KiB) one 64-bit set per channel, [2 KiB, 4 KiB) the list of
// SCREEN_POOL_CAP 32-bit entries (channel << 8 | point); a chain's result is written back over its entry.
// ------------------------------------------------------------------------------------------
#define SCREEN_POOL_CAP 512
static_assert(SCREEN_POOL_CAP >= 64 && SCREEN_POOL_CAP * 4 + 256 * 8 <= 8 * 64 * 8, "a channel's 64 candidates fit; list + sets fit the wave's 4 KiB");

// One round: entries [e0 + 64 j + lane], j < T, of list[0 .. total).  A lane without an entry replays entry e0 and drops the
// result.  wbase: fp32 fragment image of the wave's first m-block (no lane offset).
// Weights: ring of RING blocks of WB chunks per chain, requested WL blocks ahead of their use (L2); LDS rows AL blocks ahead.
template <int T, int K, bool SWZ>
__device__ __forceinline__ void screen_replay_pool(const f32x4* __restrict__ wbase, const float* x, int ld, unsigned* list,
                                                   int e0, int total, int lane) {
  // (K = 128, the STN kernels: their epilogue keeps more values live across the replay - a shorter lead, or it spills)
  constexpr int WB = 2, RING = 4, WL = K >= 512 ? 3 : 2, AL = K >= 512 ? 2 : 1, NKC8 = K / 64;
  static_assert(WB * RING == 8, "one trip of the loop is one group of 8 chunks (64 floats of a row)");
  float y[T];
  const f32x4* w[T];
  const float* row[T];
  int key[T];
  bool live[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const int idx = e0 + 64 * j + lane;
    live[j] = idx < total;
    const unsigned ent = list[live[j] ? idx : e0];
    const int cw = ent >> 8, p = ent & 63;
    y[j] = 0.f;
    w[j] = wbase + (size_t)(cw >> 5) * (K / 8) * 64 + (cw & 31);
    row[j] = x + p * ld;
    key[j] = SWZ ? p & 15 : 0;
  }
  f32x4 wv[RING][WB][T][2], ab[RING][WB][T][2];
  auto load_w = [&](int slot, int g8, int b) {  // chunks kc = 8 g8 + WB b .. + WB
#pragma unroll
    for (int i = 0; i < WB; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) wv[slot][i][j][e] = w[j][(g8 * 8 + WB * b + i) * 64 + 32 * e];
  };
  auto load_a = [&](int slot, int g8, int b) {
#pragma unroll
    for (int i = 0; i < WB; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e)
          ab[slot][i][j][e] = *reinterpret_cast<const f32x4*>(row[j] + g8 * 64 + (((2 * (WB * b + i) + e) ^ key[j]) << 2));
  };
#pragma unroll
  for (int b = 0; b < WL; ++b) load_w(b, 0, b);
#pragma unroll
  for (int b = 0; b < AL; ++b) load_a(b, 0, b);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
  for (int g8 = 0; g8 < NKC8; ++g8) {
    const int gn = g8 + 1 < NKC8 ? g8 + 1 : 0;  // (behind the last group: reads of group 0 that nothing uses)
#pragma unroll
    for (int b = 0; b < RING; ++b) {
      load_w((b + WL) % RING, b + WL < RING ? g8 : gn, (b + WL) % RING);
      load_a((b + AL) % RING, b + AL < RING ? g8 : gn, (b + AL) % RING);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < WB; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            y[j] = fmaf(wv[b][i][j][0][s], ab[b][i][j][0][s], y[j]);
            y[j] = fmaf(wv[b][i][j][1][s], ab[b][i][j][1][s], y[j]);
          }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int j = 0; j < T; ++j)
    if (live[j]) list[e0 + 64 * j + lane] = __float_as_uint(y[j]);
}

// Replay + store of the wave's 256 channels from their candidate sets sets[0 .. 256) (channel 32 mb + n of the wave at
// index 32 mb + n).  Lane l owns channels 4 l .. 4 l + 3: counts, list offsets (exclusive prefix in channel order), the scan
// of the results and the store.  A batch is the longest run of whole channels from `start` whose entries fit the list:
// one batch on all but tie-heavy tiles, at most 32 (every channel has <= 64 entries, so a batch holds >= 8 channels).
// RUN: frun[0 .. 1024) is the run's running maximum (pre-bias, the `best` of the tiles before this one; not read when
// `first`): `best` starts from it and is written back.  The list may then be empty and the replay loop is skipped.
// EPI (kernel-form switch `screen_epi`): the same lists, rounds and results with fewer LDS round trips - the lane's four
// sets are read once in two 16-byte reads and masked by `start` afterwards, the prefix runs on the DPP path
// (wave_prefix_incl), the batch total comes through v_readlane, and the scan walks the lane's entries - contiguous in the
// list, channel after channel - in ONE loop of two reads a trip instead of four dependent loops.  (The list BUILD keeps its
// four loops: one loop over the concatenated sets measured slower, profiles/experiments/screen_epi_one_loop.md.)
template <int K, bool SWZ, int LAYER, bool RUN = false, bool EPI = false>
__device__ __forceinline__ void screen_pool_store(const f32x4* __restrict__ wbase, const float* x, int ld,
                                                  unsigned long long* sets, float* __restrict__ out,
                                                  const float* __restrict__ bias, int ch0, bool relu, int lane,
                                                  float* frun = nullptr, bool first = true, int tile = 0) {
  unsigned* list = reinterpret_cast<unsigned*>(sets + 256);
  float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  unsigned long long mset[4] = {0, 0, 0, 0};
  if constexpr (EPI) {
    const u32x4 s01 = *reinterpret_cast<const u32x4*>(sets + 4 * lane), s23 = *reinterpret_cast<const u32x4*>(sets + 4 * lane + 2);
    mset[0] = (unsigned long long)s01[1] << 32 | s01[0];
    mset[1] = (unsigned long long)s01[3] << 32 | s01[2];
    mset[2] = (unsigned long long)s23[1] << 32 | s23[0];
    mset[3] = (unsigned long long)s23[3] << 32 | s23[2];
#ifdef CATRE_DEBUG_TRACE
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // (the selection of this form never holds a channel's whole set)
      const int cj = __popcll(mset[j]);
      SCREEN_COUNT(LAYER, cj < 31 ? cj : 31, 1ull);
    }
#endif
  }
  if constexpr (RUN) {
    if (!first) {
      const f32x4 f = *reinterpret_cast<const f32x4*>(frun + ch0 + 4 * lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) best[j] = f[j];
    }
  }
#ifdef CATRE_DEBUG_TRACE
  int entries = 0, rounds = 0, batches = 0;
#endif
  int start = 0;
#pragma unroll 1
  while (start < 256) {
    int c[4], off[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = 4 * lane + j >= start ? __popcll(EPI ? mset[j] : sets[4 * lane + j]) : 0;
      s += c[j];
    }
    int incl = s;
    if constexpr (EPI) {
      incl = wave_prefix_incl(s);
    } else {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = lane_get(incl, lane - o);
        if (lane >= o) incl += t;
      }
    }
    // channels whose inclusive prefix fits: a prefix [0, end) of the channels (those below `start` count 0 entries)
    int run = incl - s, end = 0, last[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      off[j] = run;
      run += c[j];
      last[j] = run;
      end += __popcll(__ballot(run <= SCREEN_POOL_CAP));
    }
    const int sel = (end - 1) & 3;
    const int lastsel = sel == 0 ? last[0] : sel == 1 ? last[1] : sel == 2 ? last[2] : last[3];
    // (`end` is a sum of ballot counts: wave-uniform)
    const int total = EPI ? __builtin_amdgcn_readlane(lastsel, __builtin_amdgcn_readfirstlane((end - 1) >> 2))
                          : lane_get(lastsel, (end - 1) >> 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cw = 4 * lane + j;
      if (cw >= start && cw < end) {
        unsigned long long m = EPI ? mset[j] : sets[cw];
        int o = off[j];
        while (m) {
          const int bit = __builtin_ctzll(m);
          m &= m - 1;
          const int p = ((bit >> 4) & 1) * 32 + (bit & 3) + 8 * ((bit & 15) >> 2) + 4 * (bit >> 5);
          list[o++] = (unsigned)(cw << 8 | p);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    SCREEN_STAMP(LAYER, tile, ch0 >> 8, 2);
#pragma unroll 1
    for (int e0 = 0; e0 < total; e0 += 128) {
      if (total - e0 > 64)
        screen_replay_pool<2, K, SWZ>(wbase, x, ld, list, e0, total, lane);
      else
        screen_replay_pool<1, K, SWZ>(wbase, x, ld, list, e0, total, lane);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    SCREEN_STAMP(LAYER, tile, ch0 >> 8, 3);
    if constexpr (EPI) {
      // the lane's entries of this batch are list[off[0] .. hi): channel j's end at lim[j] (a channel at or above `end`
      // keeps its count but is not in the batch; one below `start` counts 0)
      int lim[4], hi = off[0];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hi += 4 * lane + j < end ? c[j] : 0;
        lim[j] = hi;
      }
      for (int i = off[0]; i < hi; i += 2) {
        const int i1 = i + 1 < SCREEN_POOL_CAP ? i + 1 : SCREEN_POOL_CAP - 1;  // (past the lane's last entry: dropped below)
        const float v[2] = {__uint_as_float(list[i]), __uint_as_float(list[i1])};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int q = i + e;
          const bool t0 = q < lim[0], t1 = q < lim[1], t2 = q < lim[2], t3 = q < lim[3];
          best[0] = fmaxf(best[0], t0 ? v[e] : -INFINITY);
          best[1] = fmaxf(best[1], t1 && !t0 ? v[e] : -INFINITY);
          best[2] = fmaxf(best[2], t2 && !t1 ? v[e] : -INFINITY);
          best[3] = fmaxf(best[3], t3 && !t2 ? v[e] : -INFINITY);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cw = 4 * lane + j;
        if (cw >= start && cw < end)
          for (int i = 0; i < c[j]; ++i) best[j] = fmaxf(best[j], __uint_as_float(list[off[j] + i]));
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    SCREEN_STAMP(LAYER, tile, ch0 >> 8, 4);
#ifdef CATRE_DEBUG_TRACE
    entries += total;
    rounds += (total + 63) >> 6;
    ++batches;
#endif
    start = end;
  }
  if constexpr (RUN) {
    // read again by THIS wave only (other lanes of it), a tile later and behind the barriers between the tiles: the release
    // at workgroup scope orders the store before them, the acquire in front of the reads is screen_select_store's
    *reinterpret_cast<f32x4*>(frun + ch0 + 4 * lane) = f32x4{best[0], best[1], best[2], best[3]};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  }
  const f32x4 b = *reinterpret_cast<const f32x4*>(bias + ch0 + 4 * lane);
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = best[j] + b[j];
    if (relu) v[j] = fmaxf(v[j], 0.f);
  }
  *reinterpret_cast<f32x4*>(out + ch0 + 4 * lane) = v;
  SCREEN_STAMP(LAYER, tile, ch0 >> 8, 5);
#ifdef CATRE_DEBUG_TRACE
  if (lane == 0) {
    SCREEN_COUNT(LAYER, 32 + (rounds < 15 ? rounds : 15), 1ull);
    if (batches > 1) SCREEN_COUNT(LAYER, 48, 1ull);
    SCREEN_COUNT(LAYER, 49, 1ull);
    SCREEN_COUNT(LAYER, 50, entries);
    SCREEN_COUNT(LAYER, 51, rounds);
    if (entries == 0) SCREEN_COUNT(LAYER, 52, 1ull);
  }
#endif
}

// Epilogue of a screened "swapped" MB x 2 wave tile: select, replay, store.  acc holds the screen values S of channels
// ch0 + 32 mb + (lane & 31) at points 32 nb + (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
//   wf  : fp32 fragment image of the layer, at the wave's first m-block, + (lane & 31);  K / 64 blocks of 8 chunks
//   na  : LDS, [64] row norms (screen_row_norms); x: the fp32 image the screen read, pitch ld, swizzled or padded (SWZ)
//   sets: LDS, this wave's [MB][64] candidate sets - the replay loop over the m-blocks is NOT unrolled (its body is the
//         three replay forms: unrolled MB times it would not fit the instruction cache), so what the selection leaves per
//         m-block goes through LDS instead of a register array
//   LAYER: the row of g_screen_cnt the instrumented build counts into
//   POOL : the candidates of the wave's MB * 32 = 256 channels are replayed from one list (screen_pool_store); the selection is
//          the same, `sets` then holds one set per channel at [mb * 32 + n]
//   RUN  : (POOL only) the run form: frun = the run's running maximum, see screen_pool_store and the header
//   F16  : acc holds the fp16 screen's SCALED values (ScreenPipeF16, tile scale exponent `sa`); see the header
//   EPI  : (POOL and F16 only) the leaner selection, list build and scan of kernel-form switch `screen_epi`: the same
//          candidate sets, lists and results; no probe (sc.probe_s is not read)
template <int MB, int K, bool SWZ = true, int LAYER = 0, bool POOL = false, bool RUN = false, bool F16 = false, bool EPI = false>
__device__ __forceinline__ void screen_select_store(const f32x16 (&acc)[MB][2], const f32x4* __restrict__ wf,
                                                    const float* __restrict__ nw, const float* na, const float* x,
                                                    unsigned long long* sets, float* __restrict__ out,
                                                    const float* __restrict__ bias, int ch0, bool relu, int valid, int tile,
                                                    const ScreenArgs& sc, int lane, int ld = K, float* frun = nullptr,
                                                    bool first = true, int sa = 0, float rho = 0x1p-11f) {
  static_assert(POOL || !RUN, "the run form refines the pooled replay");
  static_assert(POOL || !F16, "the fp16 screen exists for the pooled forms");
  static_assert(!EPI || (POOL && F16), "the lean epilogue exists for the pooled fp16-screen forms");
  constexpr int NKC8 = K / 64;
  const int n = lane & 31, h = lane >> 5;
  if constexpr (POOL) SCREEN_STAMP(LAYER, tile, ch0 >> 8, 0);
  const int partner = (lane ^ 32) << 2;  // ds_bpermute address of the channel's other half-wave lane
  auto swap32 = [&](auto v) { return __builtin_bit_cast(decltype(v), __builtin_amdgcn_ds_bpermute(partner, __builtin_bit_cast(int, v))); };
  // first weight chunks of the replay: requested before the selection arithmetic
  f32x4 wb[2][16];
  if constexpr (!POOL) screen_load_w(wb[0], wf);
  {
    f32x4 na4[2][4];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g) na4[nb][g] = *reinterpret_cast<const f32x4*>(na + nb * 32 + 8 * g + 4 * h);
    unsigned vmask = 0xffffffffu;  // this half's points below `valid`
    if (valid < TP) {
      vmask = 0;
#pragma unroll
      for (int i = 0; i < 32; ++i)
        if ((i >> 4) * 32 + (i & 3) + 8 * ((i & 15) >> 2) + 4 * h < valid) vmask |= 1u << i;
    }
    // run form: the running maxima of the lane's MB channels, requested together in front of the selection
    float fc[RUN ? MB : 1];
    if constexpr (RUN) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) fc[mb] = -INFINITY;
      if (!first) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) fc[mb] = frun[ch0 + mb * 32 + n];
      }
    }
    if constexpr (EPI) {
      // The same predicate with less work per accumulator: each is read once, eps and fl(S + eps) are computed once and the
      // 32 upper values of the m-block wait in registers for L; the mask is built by shift-and-insert through the carry
      // (compare into vcc, own = 2 own + vcc: two chains of 16, from bit 15 down, so that bit nb 16 + r keeps its meaning).
      // Each half-wave writes its own 32-bit half of the channel's set; the exchange of L of m-block mb + 1 is in flight
      // while m-block mb is compared.  No probe in this form: a probe call takes the kernels that carry the probe code.
      float uwv[MB], dwv[MB], nwv[MB];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        uwv[mb] = sc.uw[ch0 + mb * 32 + n];
        dwv[mb] = sc.uw[(sc.da ? 2048 : 1024) + ch0 + mb * 32 + n];
        nwv[mb] = nw[ch0 + mb * 32 + n];
      }
      const float ua = screen_pow2(sa < -60 ? 60 : -sa);
      float hv[2][32], Lown[2], Loth[2];
      auto pass1 = [&](int mb, float(&hi)[32]) {
        float e1, e0;
        screen_eps_coef_f16<K>(nwv[mb], uwv[mb], dwv[mb], ua, rho, sc.da != 0, e1, e0);
        const float u = uwv[mb] * ua;
        float L = -INFINITY;
        if constexpr (RUN) L = fc[mb];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float a = acc[mb][nb][r], eps = fmaf(e1, na4[nb][r >> 2][r & 3], e0);
            L = fmaxf(L, fmaf(a, u, -eps));
            hi[nb * 16 + r] = fmaf(a, u, eps);
          }
        return L;
      };
      Lown[0] = pass1(0, hv[0]);
      Loth[0] = swap32(Lown[0]);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const int cur = mb & 1;
        if (mb + 1 < MB) {
          Lown[cur ^ 1] = pass1(mb + 1, hv[cur ^ 1]);
          Loth[cur ^ 1] = swap32(Lown[cur ^ 1]);
        }
        const float L = fmaxf(Lown[cur], Loth[cur]);
        unsigned m1 = 0, m0 = 0;
#pragma unroll
        for (int r = 15; r >= 0; --r) {
          asm("v_cmp_ge_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(m1) : "v"(hv[cur][16 + r]), "v"(L) : "vcc");
          asm("v_cmp_ge_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(m0) : "v"(hv[cur][r]), "v"(L) : "vcc");
        }
        unsigned own = m1 << 16 | m0;
        if (sa < -60 || !(uwv[mb] <= 0x1p60f)) own = 0xffffffffu;
        own &= vmask;
        // NaN inputs only, as below: the whole set is empty only where L is -inf (a finite L is some point's fl(S - eps),
        // and that point's fl(S + eps) is not below it), so the other half is asked for there alone
        if (L == -INFINITY) {
          const unsigned other = swap32(own);
          if ((own | other) == 0 && h == 0) own = 1;
        }
        reinterpret_cast<unsigned*>(sets)[2 * (mb * 32 + n) + h] = own;
      }
    } else {
    // candidates of the lane's channel as a 64-bit set: bit 32 h' + 16 nb + r, the same word in both half-waves
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      float e1, e0, u = 1.f;  // u: S = u acc (fp16 screen: 2^-(sw + sa), exact)
      bool all = false;       // fp16 screen: the channel or the tile could not be scaled - every point is a candidate
      if constexpr (F16) {
        const float uw = sc.uw[ch0 + mb * 32 + n], ua = screen_pow2(sa < -60 ? 60 : -sa);
        all = sa < -60 || !(uw <= 0x1p60f);
        screen_eps_coef_f16<K>(nw[ch0 + mb * 32 + n], uw, sc.uw[(sc.da ? 2048 : 1024) + ch0 + mb * 32 + n], ua, rho, sc.da != 0, e1, e0);
        u = uw * ua;
      } else {
        screen_eps_coef<K>(nw[ch0 + mb * 32 + n], e1, e0);
      }
      float L = -INFINITY;
      if constexpr (RUN) L = fc[mb];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float eps = fmaf(e1, na4[nb][r >> 2][r & 3], e0);
          L = fmaxf(L, F16 ? fmaf(acc[mb][nb][r], u, -eps) : acc[mb][nb][r] - eps);
        }
      L = fmaxf(L, swap32(L));
      unsigned own = 0;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float eps = fmaf(e1, na4[nb][r >> 2][r & 3], e0);
          own |= ((F16 ? fmaf(acc[mb][nb][r], u, eps) : acc[mb][nb][r] + eps) >= L) ? 1u << (nb * 16 + r) : 0u;
        }
      if (F16 && all) own = 0xffffffffu;
      own &= vmask;
      if (sc.probe_s) {  // tests only
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const size_t o = ((size_t)tile * 1024 + ch0 + mb * 32 + n) * TP + nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            sc.probe_s[o] = F16 ? acc[mb][nb][r] * u : acc[mb][nb][r];
            sc.probe_eps[o] = fmaf(e1, na4[nb][r >> 2][r & 3], e0);
          }
      }
      const unsigned other = swap32(own);
      unsigned long long m64 = h ? ((unsigned long long)own << 32) | other : ((unsigned long long)other << 32) | own;
      // NaN inputs only: keep the replay well defined (run form: empty is legal once the channel has a running maximum)
      if (m64 == 0 && (!RUN || L == -INFINITY)) m64 = 1;
      if constexpr (POOL) {
#ifdef CATRE_DEBUG_TRACE
        const int c = __popcll(m64);
        if (h == 0) SCREEN_COUNT(LAYER, c < 31 ? c : 31, 1ull);
#endif
        sets[mb * 32 + n] = m64;  // (both half-waves: the same word)
      } else {
        sets[mb * 64 + lane] = m64;
      }
    }
    }
  }
  if constexpr (POOL) {
    static_assert(MB == 8, "lane l owns channels 4 l .. 4 l + 3 of the wave's 256");
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    SCREEN_STAMP(LAYER, tile, ch0 >> 8, 1);
    screen_pool_store<K, SWZ, LAYER, RUN, EPI>(wf - n, x, ld, sets, out, bias, ch0, relu, lane, frun, first, tile);
    return;
  }
#ifdef CATRE_DEBUG_TRACE
  int tmax = 0;
#endif
#pragma unroll 1
  for (int mb = 0; mb < MB; ++mb) {
    const unsigned long long m64 = sets[mb * 64 + lane];
    const float b = bias[ch0 + mb * 32 + n];
    // trips of the m-block: wave maximum of ceil(candidates / 2) - lane half h replays the candidates of rank h, h + 2, ...
    // so the two lanes of a channel share its work
    int c = __popcll(m64);
#ifdef CATRE_DEBUG_TRACE
    if (h == 0) SCREEN_COUNT(LAYER, c < 31 ? c : 31, 1ull);
#endif
    int trips = 1;  // (a ballot per step instead of a shuffle tree: no lane-address registers live across the sweep)
    while (trips < TP / 2 && __ballot(c > 2 * trips)) ++trips;
#ifdef CATRE_DEBUG_TRACE
    if (lane == 0) SCREEN_COUNT(LAYER, 32 + (trips < 15 ? trips : 15), 1ull);
    tmax = trips > tmax ? trips : tmax;
#endif
    const int pad = __builtin_ctzll(m64);  // the channel's first candidate: an extra replay of a real point changes no maximum
    unsigned long long m = m64;
    if (h) m &= m - 1;  // rank 0 belongs to the lower half-wave
    const f32x4* w = wf + (size_t)mb * (K / 8) * 64;
    const f32x4* wn = mb + 1 < MB ? w + (K / 8) * 64 : w;
    float best = -INFINITY;
    // at most 64 / 2 / SCREEN_CMAX = 8 rounds (every point of the tile a candidate); one on all but degenerate tiles
#pragma unroll 1
    for (int done = 0; done < trips; done += SCREEN_CMAX) {
      int p[SCREEN_CMAX];
#pragma unroll
      for (int j = 0; j < SCREEN_CMAX; ++j) {
        const int bit = m ? __builtin_ctzll(m) : pad;
        m &= m - 1;
        m &= m - 1;
        p[j] = ((bit >> 4) & 1) * 32 + (bit & 3) + 8 * ((bit & 15) >> 2) + 4 * (bit >> 5);
      }
      const int rem = trips - done;
      const f32x4* nxt = rem > SCREEN_CMAX ? w : wn;
      float v;
      if (rem == 1)
        v = screen_replay<1, NKC8, SWZ>(w, nxt, wb, x, ld, p);
      else if (rem == 2)
        v = screen_replay<2, NKC8, SWZ>(w, nxt, wb, x, ld, p);
      else
        v = screen_replay<SCREEN_CMAX, NKC8, SWZ>(w, nxt, wb, x, ld, p);
      best = fmaxf(best, v);
    }
    best = fmaxf(best, swap32(best));
    if (lane < 32) {
      const float v = best + b;
      out[ch0 + mb * 32 + lane] = relu ? fmaxf(v, 0.f) : v;
    }
  }
#ifdef CATRE_DEBUG_TRACE
  if (lane == 0) {
    if (tmax > SCREEN_CMAX) SCREEN_COUNT(LAYER, 48, 1ull);
    SCREEN_COUNT(LAYER, 49, 1ull);
  }
#endif
}

// ------------------------------------------------------------------------------------------
// k_trunk4 with conv4 512 -> 1024 screened: conv1 .. conv3 and the a3 image are trunk4_body's; the last layer is the
// split-bf16 screen over all 1024 x 64 outputs and the fp32 replay of the candidates.  Same bits as k_trunk4<false>.
// ------------------------------------------------------------------------------------------
template <bool C, class A, class B>
struct ScreenPipeSel { typedef A type; };
template <class A, class B>
struct ScreenPipeSel<false, A, B> { typedef B type; };

template <bool POOL, bool RUN = false, bool F16 = false, bool EPI = false>
struct Trunk4ScreenT {
  ScreenArgs sc;
  float* frun;  // run form: the run's 1024 running maxima (workspace), and whether this is the run's first tile
  bool first;
  const f32x4* wf;  // fp32 fragments of the wave's channels (the replay reads them), + (lane & 31)
  const float* b4;
  typename ScreenPipeSel<F16, ScreenPipeF16<5, 2>, ScreenPipe8<2>>::type g4;
  int sa;  // fp16 screen: the tile's scale exponent (screen_tile_scale), a scalar register across the sweep
  float rho;  // ... and the tile's measured rounding rho_t (screen_tile_rho; 2^-11 with `screen_da` off)
  f32x16 acc4[8][2];
  __device__ __forceinline__ void prefetch(const f32x4* __restrict__ wp4, const float* __restrict__ b4_, int mb0, int lane) {
    wf = wp4 + ((size_t)mb0 * 64) * 64 + (lane & 31);
    b4 = b4_;
    g4.prefetch(sc.wps + ((size_t)mb0 * 32) * 64 + lane);
  }
  // a2 (32 KiB, dead): [0, 64) the row norms, from float 64 on the waves' candidate sets (4 x 4 KiB), behind them
  // [4160, 4224) the rows' rho (`screen_da`).  a3 is written behind ReLU (trunk4_body: store_tile_lds_pre<.., RELU = true>):
  // no negative element, which the sign-split dws needs.
  __device__ __forceinline__ void sweep(const float* a3, float* a2, int tid, int lane) {
    const bool da = F16 && sc.da != 0;
    screen_row_norms<512, 256>(a3, a2, tid, 512, da, a2 + 64 + 4 * 1024);
    __syncthreads();
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc4[mb][0] = acc4[mb][1] = zero16();
    if constexpr (F16) {
      sa = screen_tile_scale(a2, lane);
      rho = screen_tile_rho(a2 + 64 + 4 * 1024, lane, da);
      g4.run(acc4, a3, lane, sa);
    } else {
      g4.run(acc4, a3, lane);
    }
  }
  __device__ __forceinline__ void store(const float* a3, float* a2, float* __restrict__ pm, int tile, int mb0, int valid, int,
                                        const TrainSave&, int lane) {
    unsigned long long* sets = reinterpret_cast<unsigned long long*>(a2 + 64) + (mb0 >> 3) * 8 * 64;
    // The lane id is computed afresh here instead of being kept from the prologue (volatile: the compiler would otherwise merge
    // the two) - the sweep above runs at exactly 256 VGPRs next to its 256 accumulators, and a lane id live across it is one
    // value too many: without this line the kernel spills to scratch, which tests/test_resources.py reports.
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    screen_select_store<8, 512, true, 0, POOL, RUN, F16, EPI>(acc4, wf, sc.nw, a2, a3, sets, pm + (size_t)tile * PMW, b4, mb0 * 32,
                                                         false, valid, tile, sc, lane, 512, frun, first, F16 ? sa : 0,
                                                         F16 ? rho : 0x1p-11f);
  }
};
typedef Trunk4ScreenT<false> Trunk4Screen;

__global__ __launch_bounds__(256) void k_trunk4s(catre_points P, const float* __restrict__ trans3,
                                                 const float* __restrict__ trans64, const float* __restrict__ Wc1,
                                                 const float* __restrict__ bc1, const f32x4* __restrict__ wp2,
                                                 const float* __restrict__ b2, const f32x4* __restrict__ wp3,
                                                 const float* __restrict__ b3, const f32x4* __restrict__ wp4,
                                                 const float* __restrict__ b4, float* __restrict__ pm,
                                                 float* __restrict__ pointfeat, int B, int N, int M,
                                                 unsigned long long* __restrict__ trace, ScreenArgs sc) {
  __shared__ __attribute__((aligned(16))) float smem[TRUNK_SMEM];
  Trunk4Screen tl;
  tl.sc = sc;
  trunk4_body<false>(smem, P, trans3, trans64, Wc1, bc1, wp2, b2, wp3, b3, wp4, b4, pm, pointfeat, B, N, M, trace,
                     TrainSave{}, tl, blockIdx.x, threadIdx.x);
}

// the same kernel with the pooled replay (screen_pool_store); k_trunk4sp16: with the fp16 screen (`screen_f16`)
#define TRUNK4SP_(NAME, F16, EPI)                                                                                            \
  __global__ __launch_bounds__(256) void NAME(                                                                            \
      catre_points P, const float* __restrict__ trans3, const float* __restrict__ trans64, const float* __restrict__ Wc1, \
      const float* __restrict__ bc1, const f32x4* __restrict__ wp2, const float* __restrict__ b2,                         \
      const f32x4* __restrict__ wp3, const float* __restrict__ b3, const f32x4* __restrict__ wp4,                         \
      const float* __restrict__ b4, float* __restrict__ pm, float* __restrict__ pointfeat, int B, int N, int M,           \
      unsigned long long* __restrict__ trace, ScreenArgs sc) {                                                            \
    __shared__ __attribute__((aligned(16))) float smem[TRUNK_SMEM];                                                       \
    Trunk4ScreenT<true, false, F16, EPI> tl;                                                                                \
    tl.sc = sc;                                                                                                           \
    trunk4_body<false>(smem, P, trans3, trans64, Wc1, bc1, wp2, b2, wp3, b3, wp4, b4, pm, pointfeat, B, N, M, trace,      \
                       TrainSave{}, tl, blockIdx.x, threadIdx.x);                                                         \
  }
TRUNK4SP_(k_trunk4sp, false, false)
TRUNK4SP_(k_trunk4sp16, true, false)
TRUNK4SP_(k_trunk4sp16e, true, true)  // `screen_epi`: the lean epilogue, no probe
#undef TRUNK4SP_

// Run -> tiles.  Runs are enumerated like tiles, observed clouds first; a cloud of T tiles has ceil(T / S) runs of S
// consecutive tiles, the last one shorter.  No run crosses a cloud.
__device__ __forceinline__ void run_info(int rid, int B, int N, int M, int S, int& tile0, int& nt) {
  const int TN = (N + TP - 1) / TP, TM = (M + TP - 1) / TP;
  const int RN = (TN + S - 1) / S, RM = (TM + S - 1) / S;
  if (rid < B * RN) {
    const int k = rid % RN;
    tile0 = (rid / RN) * TN + k * S;
    nt = min(S, TN - k * S);
  } else {
    const int r = rid - B * RN, k = r % RM;
    tile0 = B * TN + (r / RM) * TM + k * S;
    nt = min(S, TM - k * S);
  }
}

// The run form of k_trunk4sp: a workgroup walks the run's tiles one after the other and carries the exact running maximum
// (frun: 1024 floats per run in the workspace - the 160 KiB of LDS are taken and no LDS region survives a tile; no register
// survives the 256-accumulator sweep).  Nothing passes between workgroups; the candidate sets are a function of the inputs
// and S alone.
struct TrunkRunArgs {
  catre_points P;
  const float *trans3, *trans64, *Wc1, *bc1;
  const f32x4* wp2;
  const float* b2;
  const f32x4* wp3;
  const float* b3;
  const f32x4* wp4;
  const float* b4;
  float *pm, *pointfeat;
  unsigned long long* trace;
  ScreenArgs sc;
  float* frun;  // [runs][1024]
  int B, N, M, S;
};

template <bool F16, bool EPI = false>
__device__ __forceinline__ void trunk4sr_body() {
  __shared__ __attribute__((aligned(16))) float smem[TRUNK_SMEM];
  // The arguments are read from the kernel-argument segment afresh in every tile (the pointer passes through an empty
  // volatile asm, so the loads cannot leave the loop): held in scalar registers for the whole loop, the 64 dwords of
  // arguments do not fit beside what the sweep needs, the excess goes to a vector register and the kernel spills.
  // For the same reason the wave index stays in a scalar register and the lane id is computed afresh in every tile, so that
  // neither threadIdx.x nor anything derived from a lane id is live across a tile's sweep (Trunk4ScreenT::store).
  typedef const __attribute__((address_space(4))) TrunkRunArgs* ArgPtr;
  ArgPtr ap = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int tile0, nt;
  run_info(blockIdx.x, ap->B, ap->N, ap->M, ap->S, tile0, nt);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    asm volatile("" : "+s"(ap));
    const TrunkRunArgs a = *(const TrunkRunArgs*)ap;  // (generic pointer for the copy; the loads stay scalar)
    Trunk4ScreenT<true, true, F16, EPI> tl;
    tl.sc = a.sc;
    tl.frun = a.frun + (size_t)blockIdx.x * 1024;
    tl.first = t == 0;
    trunk4_body<false>(smem, a.P, a.trans3, a.trans64, a.Wc1, a.bc1, a.wp2, a.b2, a.wp3, a.b3, a.wp4, a.b4, a.pm, a.pointfeat,
                       a.B, a.N, a.M, a.trace, TrainSave{}, tl, tile0 + t, wave * 64 + lane);
    __syncthreads();  // the next tile's prologue overwrites the a3 image the other waves still replay from
  }
}
__global__ __launch_bounds__(256) void k_trunk4sr(TrunkRunArgs args) {
  (void)args;
  trunk4sr_body<false>();
}
__global__ __launch_bounds__(256) void k_trunk4sr16(TrunkRunArgs args) {  // with the fp16 screen (`screen_f16`)
  (void)args;
  trunk4sr_body<true>();
}
__global__ __launch_bounds__(256) void k_trunk4sr16e(TrunkRunArgs args) {  // ... and the lean epilogue (`screen_epi`)
  (void)args;
  trunk4sr_body<true, true>();
}

// ------------------------------------------------------------------------------------------
// k_stn3d_pair / k_stnkd_pair (inference) with conv3 128 -> 1024 screened: conv1 / conv2 (and fstn.conv1) and the fp32
// a2 / f2 image [128][LD128] are the dense kernels'; each tile of the pair is then screened on the MB8 x NB2 wave tile
// (K = 128: 8 K = 16 chunks), selected and replayed like the trunk's conv4.  Same bits as k_stn*_pair<false>.
// The B fragments are split in registers inside every wave, as in the trunk (ScreenPipe8): see DESIGN section 3.
// ------------------------------------------------------------------------------------------
typedef ScreenPipe8<2, 8, false, LD128> StnScreenPipe;
typedef ScreenPipeF16<5, 2, 8, false, LD128> StnScreenPipeF16;  // the fp16 screen (`screen_f16`, k_stn*_pair_sp16 / _sr16)
template <bool F16>
using StnPipeT = typename ScreenPipeSel<F16, StnScreenPipeF16, StnScreenPipe>::type;

// scratch: LDS that is dead after conv2 (a1 / h1, 34 KiB): [0, 128) the row norms of both tiles, from float 128 on the
// waves' candidate sets (4 x 4 KiB), behind them [4224, 4352) the rows' rho (`screen_da`).  img is written behind ReLU
// (store_tile_lds_pre<1, 4, RELU = true> of both callers): no negative element, which the sign-split dws needs.  g holds the first sweep's first weight fragments (requested in front of conv2).
// probe_rows (tests only): the image rows as [tile][64][128]
// RUN: the run form (k_stn*_pair_sr) - frun = the 1024 running maxima of the run (LDS, -inf in front of the first tile;
// first_pair: they are not to be read)
template <int LAYER, bool POOL, bool RUN = false, bool F16 = false, bool EPI = false>
__device__ __forceinline__ void stn_conv3_screened(const float* img, float* scratch, StnPipeT<F16>& g,
                                                   const f32x4* __restrict__ wp3, const float* __restrict__ b3,
                                                   float* __restrict__ pm, int tile0, int valid2, const ScreenArgs& sc,
                                                   float* __restrict__ probe_rows, int wave, int tid, int lane,
                                                   float* frun = nullptr, bool first_pair = true) {
  const int nt = valid2 > TP ? 2 : 1, mb0 = wave * 8;
  const bool da = F16 && sc.da != 0;
  float* rho = scratch + 2 * TP + 4 * 1024;
  SCREEN_STAMP(LAYER, tile0, wave, 6);  // [6] .. [7]: the row norms (with `screen_da`: and the measuring) of both tiles
  screen_row_norms<128, 256, 2 * TP, false>(img, scratch, tid, LD128, da, rho);
  if (probe_rows) {
    for (int i = tid; i < nt * TP * 32; i += 256)
      *reinterpret_cast<f32x4*>(probe_rows + ((size_t)tile0 * TP + (i >> 5)) * 128 + (i & 31) * 4) =
          *reinterpret_cast<const f32x4*>(img + (i >> 5) * LD128 + (i & 31) * 4);
  }
  __syncthreads();
  SCREEN_STAMP(LAYER, tile0, wave, 7);
  unsigned long long* sets = reinterpret_cast<unsigned long long*>(scratch + 2 * TP) + wave * 8 * 64;
  // The two tiles one after the other on the same accumulators, as two copies of the code: in a runtime loop the compiler
  // hoists the selection's ~25 bit-mask constants and the lane-dependent addresses out of it, across the sweep, and spills.
  auto tile = [&](int t, int ln) {
    f32x16 acc[8][2];
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc[mb][0] = acc[mb][1] = zero16();
    const float* x = img + t * TP * LD128;
    int sa = 0;
    float rho_t = 0x1p-11f;
    if constexpr (F16) {
      sa = screen_tile_scale(scratch + t * TP, ln);
      rho_t = screen_tile_rho(rho + t * TP, ln, da);
      g.run(acc, x, ln, sa);
    } else {
      g.run(acc, x, ln);
    }
    // the lane id is computed afresh behind the sweep (see Trunk4Screen::store: the sweep leaves no register for it)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    const f32x4* wf = wp3 + ((size_t)mb0 * 16) * 64 + (ln & 31);
    screen_select_store<8, 128, false, LAYER, POOL, RUN, F16, EPI>(acc, wf, sc.nw, scratch + t * TP, x, sets,
                                                              pm + (size_t)(tile0 + t) * PMW, b3, mb0 * 32, true,
                                                              min(valid2 - t * TP, TP), tile0 + t, sc, ln, LD128, frun,
                                                              first_pair && t == 0, sa, rho_t);
  };
  tile(0, lane);
  if (nt == 2) {  // (again a fresh lane id: nothing lane-dependent of the first tile stays live across its epilogue)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    g.prefetch(sc.wps + ((size_t)mb0 * 8) * 64 + lane);
    tile(1, lane);
  }
}

// POOL: the pooled replay (screen_pool_store) - k_stn3d_pair_sp / k_stnkd_pair_sp
// (bid, tid): blockIdx.x and threadIdx.x of the one-pair kernels; the run form walks several pairs (RUN, frun, first_pair)
template <bool POOL, bool RUN = false, bool F16 = false, bool EPI = false>
__device__ __forceinline__ void stn3d_pair_s_body(catre_points P, const float* __restrict__ W1,
                                                  const float* __restrict__ b1, const f32x4* __restrict__ wp2,
                                                  const float* __restrict__ b2, const f32x4* __restrict__ wp3,
                                                  const float* __restrict__ b3, float* __restrict__ pm, int B, int N,
                                                  int M, const ScreenArgs& sc, float* __restrict__ probe_rows,
                                                  const int bid, const int tid, float* frun = nullptr,
                                                  bool first_pair = true) {
  __shared__ __attribute__((aligned(16))) float smem[2 * TP * LD64 + 2 * TP * LD128];
  float* a1 = smem;                   // [128][68]; after conv2: row norms + candidate sets
  float* a2 = smem + 2 * TP * LD64;   // [128][132]
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  TileInfo ti;
  int tile0;
  pair_info32(bid, B, N, M, ti, tile0);

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
  StnPipeT<F16> g3;
  g3.prefetch(sc.wps + ((size_t)wave * 8 * 8) * 64 + lane);
  {
    f32x16 acc[1][4] = {{zero16(), zero16(), zero16(), zero16()}};
    g2.run(acc, a1, LD64, lane);
    store_tile_lds_pre<1, 4, true, false>(acc, a2, LD128, wave * 32, bv2, lane);
  }
  __syncthreads();
  stn_conv3_screened<1, POOL, RUN, F16, EPI>(a2, a1, g3, wp3, b3, pm, tile0, ti.valid, sc, probe_rows, wave, tid, lane, frun, first_pair);
}
#define STN3D_PAIR_S_(NAME, POOL, F16, EPI)                                                                                     \
  __global__ __launch_bounds__(256) void NAME(catre_points P, const float* __restrict__ W1, const float* __restrict__ b1, \
                                              const f32x4* __restrict__ wp2, const float* __restrict__ b2,                \
                                              const f32x4* __restrict__ wp3, const float* __restrict__ b3,                \
                                              float* __restrict__ pm, int B, int N, int M, ScreenArgs sc,                 \
                                              float* __restrict__ probe_rows) {                                           \
    stn3d_pair_s_body<POOL, false, F16, EPI>(P, W1, b1, wp2, b2, wp3, b3, pm, B, N, M, sc, EPI ? nullptr : probe_rows, blockIdx.x, \
                                             threadIdx.x);                                                              \
  }
STN3D_PAIR_S_(k_stn3d_pair_s, false, false, false)
STN3D_PAIR_S_(k_stn3d_pair_sp, true, false, false)
STN3D_PAIR_S_(k_stn3d_pair_sp16, true, true, false)
STN3D_PAIR_S_(k_stn3d_pair_sp16e, true, true, true)  // `screen_epi`: no probe, probe_rows is not read
#undef STN3D_PAIR_S_

template <bool POOL, bool RUN = false, bool F16 = false, bool EPI = false>
__device__ __forceinline__ void stnkd_pair_s_body(catre_points P, const float* __restrict__ trans3,
                                                  const float* __restrict__ Wc1, const float* __restrict__ bc1,
                                                  const f32x4* __restrict__ wpf1, const float* __restrict__ bf1,
                                                  const f32x4* __restrict__ wpf2, const float* __restrict__ bf2,
                                                  const f32x4* __restrict__ wpf3, const float* __restrict__ bf3,
                                                  float* __restrict__ pm, int B, int N, int M, const ScreenArgs& sc,
                                                  float* __restrict__ probe_rows, const int bid, const int tid,
                                                  float* frun = nullptr, bool first_pair = true) {
  __shared__ __attribute__((aligned(16))) float smem[4 * TP * LD64 + 2 * TP * LD128];
  float* h1 = smem;                   // [128][68]; after conv2: row norms + candidate sets
  float* f1 = smem + 2 * TP * LD64;   // [128][68]
  float* f2 = smem + 4 * TP * LD64;   // [128][132]
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  TileInfo ti;
  int tile0;
  pair_info32(bid, B, N, M, ti, tile0);

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
  StnPipeT<F16> g3;
  g3.prefetch(sc.wps + ((size_t)wave * 8 * 8) * 64 + lane);
  {
    f32x16 acc[1][4] = {{zero16(), zero16(), zero16(), zero16()}};
    g2.run(acc, f1, LD64, lane);
    store_tile_lds_pre<1, 4, true, false>(acc, f2, LD128, wave * 32, bv2, lane);
  }
  __syncthreads();
  stn_conv3_screened<2, POOL, RUN, F16, EPI>(f2, h1, g3, wpf3, bf3, pm, tile0, ti.valid, sc, probe_rows, wave, tid, lane, frun, first_pair);
}
#define STNKD_PAIR_S_(NAME, POOL, F16, EPI)                                                                                 \
  __global__ __launch_bounds__(256) void NAME(                                                                        \
      catre_points P, const float* __restrict__ trans3, const float* __restrict__ Wc1, const float* __restrict__ bc1, \
      const f32x4* __restrict__ wpf1, const float* __restrict__ bf1, const f32x4* __restrict__ wpf2,                  \
      const float* __restrict__ bf2, const f32x4* __restrict__ wpf3, const float* __restrict__ bf3,                   \
      float* __restrict__ pm, int B, int N, int M, ScreenArgs sc, float* __restrict__ probe_rows) {                   \
    stnkd_pair_s_body<POOL, false, F16, EPI>(P, trans3, Wc1, bc1, wpf1, bf1, wpf2, bf2, wpf3, bf3, pm, B, N, M, sc,    \
                                             EPI ? nullptr : probe_rows, blockIdx.x, threadIdx.x);                     \
  }
STNKD_PAIR_S_(k_stnkd_pair_s, false, false, false)
STNKD_PAIR_S_(k_stnkd_pair_sp, true, false, false)
STNKD_PAIR_S_(k_stnkd_pair_sp16, true, true, false)
STNKD_PAIR_S_(k_stnkd_pair_sp16e, true, true, true)
#undef STNKD_PAIR_S_

// ------------------------------------------------------------------------------------------
// Run forms of the pooled STN pair kernels (`screen_run`, its own arm CATRE_SCREEN_RUN_STN): a workgroup walks up to SP
// consecutive PAIRS of one cloud - the loop is over pairs, the two tile copies inside stn_conv3_screened stay - and carries
// the running maximum from tile to tile, the second tile of a pair included.  These kernels have LDS to spare: the 1024
// running maxima live there.  Arguments, wave index and lane id are handled as in k_trunk4sr.
// ------------------------------------------------------------------------------------------
// run -> pairs, in pair_info32's numbering (observed clouds first; a cloud of P pairs has ceil(P / SP) runs)
__device__ __forceinline__ void pair_run_info(int rid, int B, int N, int M, int SP, int& pair0, int& np) {
  const int PN = ((N + TP - 1) / TP + 1) / 2, PM_ = ((M + TP - 1) / TP + 1) / 2;
  const int RN = (PN + SP - 1) / SP, RM = (PM_ + SP - 1) / SP;
  if (rid < B * RN) {
    const int k = rid % RN;
    pair0 = (rid / RN) * PN + k * SP;
    np = min(SP, PN - k * SP);
  } else {
    const int r = rid - B * RN, k = r % RM;
    pair0 = B * PN + (r / RM) * PM_ + k * SP;
    np = min(SP, PM_ - k * SP);
  }
}

struct Stn3dRunArgs {
  catre_points P;
  const float *W1, *b1;
  const f32x4* wp2;
  const float* b2;
  const f32x4* wp3;
  const float* b3;
  float* pm;
  const u32x4* wps;  // ScreenArgs without the probes: the probe calls keep the one-pair kernels
  const float* nw;
  int B, N, M, SP;
  const float* uw;  // fp16 screen (k_stn*_pair_sr16; wps then are its fragments)
  int da;           // ... and its `screen_da` (ScreenArgs::da)
};

template <bool F16, bool EPI = false>
__device__ __forceinline__ void stn3d_pair_sr_body() {
  __shared__ __attribute__((aligned(16))) float frun[1024];
  typedef const __attribute__((address_space(4))) Stn3dRunArgs* ArgPtr;
  ArgPtr ap = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int pair0, np;
  pair_run_info(blockIdx.x, ap->B, ap->N, ap->M, ap->SP, pair0, np);
  // -inf in front of the first tile; every wave reads and writes its own 256 channels only
  *reinterpret_cast<f32x4*>(frun + 4 * threadIdx.x) = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  __syncthreads();
#pragma unroll 1
  for (int bid = pair0, end = pair0 + np; bid < end; ++bid) {
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    asm volatile("" : "+s"(ap));
    const Stn3dRunArgs a = *(const Stn3dRunArgs*)ap;
    stn3d_pair_s_body<true, true, F16, EPI>(a.P, a.W1, a.b1, a.wp2, a.b2, a.wp3, a.b3, a.pm, a.B, a.N, a.M,
                                       ScreenArgs{a.wps, a.nw, nullptr, nullptr, a.uw, a.da}, nullptr, bid, wave * 64 + lane, frun,
                                       false);
    __syncthreads();  // the next pair's conv1 overwrites the candidate sets, its conv2 the image the other waves replay from
  }
}
__global__ __launch_bounds__(256) void k_stn3d_pair_sr(Stn3dRunArgs args) {
  (void)args;
  stn3d_pair_sr_body<false>();
}
__global__ __launch_bounds__(256) void k_stn3d_pair_sr16(Stn3dRunArgs args) {
  (void)args;
  stn3d_pair_sr_body<true>();
}
__global__ __launch_bounds__(256) void k_stn3d_pair_sr16e(Stn3dRunArgs args) {  // `screen_epi`
  (void)args;
  stn3d_pair_sr_body<true, true>();
}

struct StnkdRunArgs {
  catre_points P;
  const float *trans3, *Wc1, *bc1;
  const f32x4* wpf1;
  const float* bf1;
  const f32x4* wpf2;
  const float* bf2;
  const f32x4* wpf3;
  const float* bf3;
  float* pm;
  const u32x4* wps;  // ScreenArgs without the probes: the probe calls keep the one-pair kernels
  const float* nw;
  int B, N, M, SP;
  const float* uw;  // fp16 screen (k_stn*_pair_sr16; wps then are its fragments)
  int da;           // ... and its `screen_da` (ScreenArgs::da)
};

template <bool F16, bool EPI = false>
__device__ __forceinline__ void stnkd_pair_sr_body() {
  __shared__ __attribute__((aligned(16))) float frun[1024];
  typedef const __attribute__((address_space(4))) StnkdRunArgs* ArgPtr;
  ArgPtr ap = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int pair0, np;
  pair_run_info(blockIdx.x, ap->B, ap->N, ap->M, ap->SP, pair0, np);
  // -inf in front of the first tile; every wave reads and writes its own 256 channels only
  *reinterpret_cast<f32x4*>(frun + 4 * threadIdx.x) = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  __syncthreads();
#pragma unroll 1
  for (int bid = pair0, end = pair0 + np; bid < end; ++bid) {
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    asm volatile("" : "+s"(ap));
    const StnkdRunArgs a = *(const StnkdRunArgs*)ap;
    stnkd_pair_s_body<true, true, F16, EPI>(a.P, a.trans3, a.Wc1, a.bc1, a.wpf1, a.bf1, a.wpf2, a.bf2, a.wpf3, a.bf3, a.pm, a.B, a.N,
                                       a.M, ScreenArgs{a.wps, a.nw, nullptr, nullptr, a.uw, a.da}, nullptr, bid, wave * 64 + lane,
                                       frun, false);
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_stnkd_pair_sr(StnkdRunArgs args) {
  (void)args;
  stnkd_pair_sr_body<false>();
}
__global__ __launch_bounds__(256) void k_stnkd_pair_sr16(StnkdRunArgs args) {
  (void)args;
  stnkd_pair_sr_body<true>();
}
__global__ __launch_bounds__(256) void k_stnkd_pair_sr16e(StnkdRunArgs args) {  // `screen_epi`
  (void)args;
  stnkd_pair_sr_body<true, true>();
}
