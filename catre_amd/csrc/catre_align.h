// catre_align.h - initial pose and scale of every instance from a NOCS coordinate map: the RANSAC-wrapped Umeyama
// similarity fit of the reference (preprocess/pose_data.py:109-165 around :56-87, fallback of the caller :38-47), for a
// ragged batch of instances on the device.  Inputs fp32, arithmetic fp64 (the reference computes in float64).
//
//   Umeyama(S, T) on m pairs: C = (1/m) sum (T - mu_t)(S - mu_s)^T = U diag(D) V^T, D descending; if det(U) det(V) < 0
//     negate D[2] and U[:,2]; R = U V^T; s = sum(D) / sum_axes var(S) (population variance); t = mu_t - s R mu_s.
//     The SVD is a one-sided Jacobi iteration on the columns of C (named scalars, no indexed local array: nothing in
//     scratch).  The third left vector is taken as det(V) * (u_1 x u_2), which IS the det rule: the rotation is unique
//     whenever sigma_2 > 0, also for a planar source (sigma_3 = 0).
//   RANSAC (max_iter <= 128 hypotheses of 5 pairs drawn with replacement): InlierT = 2 max_k |src_k - mean(src)| / 10;
//     inliers of hypothesis h: |dst_k - (s_h R_h src_k + t_h)| < s_h InlierT (strict); the first hypothesis with strictly
//     more inliers than every earlier one wins; the loop stops after iteration `it` (zero-based) when
//     1 - (1 - best^5)^it > confidence; best < min_inlier_ratio -> invalid (s = 1, R = I, t = 0), else the fit of the
//     winner's inlier set.  Also invalid, and NOT the reference's behaviour (it raises or returns NaN): n < 5 and a
//     non-finite value in the first n rows.
//
//   k_align_hyp    one thread per hypothesis: its five draws, the 5-point fit -> workspace [I][max_iter][16] doubles
//                  (s R, t, s).  Draws are read from `draws` [I][max_iter][5] or evaluated: Philox4x32-10 (daug_philox of
//                  catre_pclf.h) at counter (key lo, key hi, iteration, word block) under key `seed`; draw j is
//                  mulhi32(word j, n) - words 0..3 of block 0, word 0 of block 1.  mulhi32 maps a uniform 32-bit word to
//                  [0, n) with a bias of at most n / 2^32 per index (2.4e-7 at n = 1024).  Nothing depends on the
//                  launch geometry or on the batch around an instance.  A draw outside [0, n) makes the hypothesis
//                  empty (NaN scale: no inlier) instead of reading outside the instance.
//   k_align_ransac one 256-thread workgroup per instance: the table goes to LDS; hypotheses are counted 32 at a time -
//                  a wave tests 64 points against one hypothesis with one ballot and a popcount - and after every 32 one
//                  thread applies the selection and the stop rule in draw order, so an instance that stops at
//                  iteration 27 counts 32 hypotheses, not 128.  Then the winner's mask is rebuilt (the same device
//                  function, explicit fma: the same bits), its moments are reduced in fp64 in a fixed order and
//                  the final fit is solved (by every thread alike; thread 0 stores it).  Any n: nothing assumes a
//                  multiple of 64; rows >= n are never read.
//   k_umeyama      the plain least-squares fit of the rows an optional byte mask keeps.
//   k_align_draws  writes the evaluated draws out.
#pragma once
#include "catre_device.h"

#include "../../include/catre_hip.h"
#include "catre_pclf.h"  // the Philox draws of the depth augmentation

#define ALIGN_MAX_ITER 128
#define ALIGN_HB 32      // hypotheses counted per pass over the points
#define ALIGN_HYP_W 16   // doubles per hypothesis in the workspace: s R [9], t [3], s, 3 unused

struct AlignFit {
  double s, r00, r01, r02, r10, r11, r12, r20, r21, r22, t0, t1, t2;
};

// one Jacobi rotation that makes columns a and b of the working matrix orthogonal; the same rotation on V
__device__ __forceinline__ bool align_jrot(double& ax, double& ay, double& az, double& bx, double& by, double& bz,
                                           double& vax, double& vay, double& vaz, double& vbx, double& vby, double& vbz) {
  const double alpha = ax * ax + ay * ay + az * az, beta = bx * bx + by * by + bz * bz;
  const double gamma = ax * bx + ay * by + az * bz;
  if (gamma == 0.0 || !(fabs(gamma) > 1e-17 * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  double p, q;
  p = c * ax - s * bx, q = s * ax + c * bx, ax = p, bx = q;
  p = c * ay - s * by, q = s * ay + c * by, ay = p, by = q;
  p = c * az - s * bz, q = s * az + c * bz, az = p, bz = q;
  p = c * vax - s * vbx, q = s * vax + c * vbx, vax = p, vbx = q;
  p = c * vay - s * vby, q = s * vay + c * vby, vay = p, vby = q;
  p = c * vaz - s * vbz, q = s * vaz + c * vbz, vaz = p, vbz = q;
  return true;
}

__device__ __forceinline__ void align_swap(double& a, double& b) {
  const double t = a;
  a = b;
  b = t;
}

// C (c_rc: row r = target axis, column c = source axis), var = sum over axes of the population variance of S,
// mu_s, mu_t -> the similarity; sv0 >= sv1: the two largest singular values of C (the rotation is unique iff sv1 > 0)
__device__ __forceinline__ AlignFit align_solve_sv(double c00, double c01, double c02, double c10, double c11, double c12,
                                                   double c20, double c21, double c22, double var, double msx, double msy,
                                                   double msz, double mtx, double mty, double mtz, double& sv0, double& sv1) {
  // columns of C
  double a0x = c00, a0y = c10, a0z = c20, a1x = c01, a1y = c11, a1z = c21, a2x = c02, a2y = c12, a2z = c22;
  double v0x = 1.0, v0y = 0.0, v0z = 0.0, v1x = 0.0, v1y = 1.0, v1z = 0.0, v2x = 0.0, v2y = 0.0, v2z = 1.0;
  for (int sweep = 0; sweep < 12; ++sweep) {
    bool rot = align_jrot(a0x, a0y, a0z, a1x, a1y, a1z, v0x, v0y, v0z, v1x, v1y, v1z);
    rot |= align_jrot(a0x, a0y, a0z, a2x, a2y, a2z, v0x, v0y, v0z, v2x, v2y, v2z);
    rot |= align_jrot(a1x, a1y, a1z, a2x, a2y, a2z, v1x, v1y, v1z, v2x, v2y, v2z);
    if (!rot) break;
  }
  double s0 = sqrt(a0x * a0x + a0y * a0y + a0z * a0z), s1 = sqrt(a1x * a1x + a1y * a1y + a1z * a1z),
         s2 = sqrt(a2x * a2x + a2y * a2y + a2z * a2z);
#define ALIGN_SORT(SA, SB, A, B, VA, VB)                                                                      \
  if (SA < SB) {                                                                                              \
    align_swap(SA, SB);                                                                                       \
    align_swap(A##x, B##x), align_swap(A##y, B##y), align_swap(A##z, B##z);                                   \
    align_swap(VA##x, VB##x), align_swap(VA##y, VB##y), align_swap(VA##z, VB##z);                             \
  }
  ALIGN_SORT(s0, s1, a0, a1, v0, v1)
  ALIGN_SORT(s1, s2, a1, a2, v1, v2)
  ALIGN_SORT(s0, s1, a0, a1, v0, v1)
#undef ALIGN_SORT
  const double u0x = a0x / s0, u0y = a0y / s0, u0z = a0z / s0, u1x = a1x / s1, u1y = a1y / s1, u1z = a1z / s1;
  const double wx = u0y * u1z - u0z * u1y, wy = u0z * u1x - u0x * u1z, wz = u0x * u1y - u0y * u1x;  // u_1 x u_2
  const double detv = v0x * (v1y * v2z - v1z * v2y) + v0y * (v1z * v2x - v1x * v2z) + v0z * (v1x * v2y - v1y * v2x);
  const double dv = detv >= 0.0 ? 1.0 : -1.0;
  const double du = (a2x * wx + a2y * wy + a2z * wz) >= 0.0 ? 1.0 : -1.0;  // det(U) of the decomposition itself
  const double u2x = dv * wx, u2y = dv * wy, u2z = dv * wz;
  AlignFit f;
  f.r00 = u0x * v0x + u1x * v1x + u2x * v2x, f.r01 = u0x * v0y + u1x * v1y + u2x * v2y, f.r02 = u0x * v0z + u1x * v1z + u2x * v2z;
  f.r10 = u0y * v0x + u1y * v1x + u2y * v2x, f.r11 = u0y * v0y + u1y * v1y + u2y * v2y, f.r12 = u0y * v0z + u1y * v1z + u2y * v2z;
  f.r20 = u0z * v0x + u1z * v1x + u2z * v2x, f.r21 = u0z * v0y + u1z * v1y + u2z * v2y, f.r22 = u0z * v0z + u1z * v1z + u2z * v2z;
  f.s = (s0 + s1 + du * dv * s2) / var;
  f.t0 = mtx - f.s * (f.r00 * msx + f.r01 * msy + f.r02 * msz);
  f.t1 = mty - f.s * (f.r10 * msx + f.r11 * msy + f.r12 * msz);
  f.t2 = mtz - f.s * (f.r20 * msx + f.r21 * msy + f.r22 * msz);
  sv0 = s0, sv1 = s1;
  return f;
}

__device__ __forceinline__ AlignFit align_solve(double c00, double c01, double c02, double c10, double c11, double c12,
                                                double c20, double c21, double c22, double var, double msx, double msy,
                                                double msz, double mtx, double mty, double mtz) {
  double sv0, sv1;
  return align_solve_sv(c00, c01, c02, c10, c11, c12, c20, c21, c22, var, msx, msy, msz, mtx, mty, mtz, sv0, sv1);
}

__device__ __forceinline__ bool align_finite(const AlignFit& f) {
  const double a = f.s + f.r00 + f.r01 + f.r02 + f.r10 + f.r11 + f.r12 + f.r20 + f.r21 + f.r22 + f.t0 + f.t1 + f.t2;
  return a - a == 0.0;
}

// the inlier test of one point against one hypothesis h = {s R [9], t [3], s}: every product written as an fma, so the
// counting pass and the pass that rebuilds the winner's mask round alike
__device__ __forceinline__ bool align_inlier(const double* __restrict__ h, double inlier_t, double sx, double sy, double sz,
                                             double dx, double dy, double dz) {
  const double ex = dx - fma(h[0], sx, fma(h[1], sy, fma(h[2], sz, h[9])));
  const double ey = dy - fma(h[3], sx, fma(h[4], sy, fma(h[5], sz, h[10])));
  const double ez = dz - fma(h[6], sx, fma(h[7], sy, fma(h[8], sz, h[11])));
  return sqrt(fma(ex, ex, fma(ey, ey, ez * ez))) < h[12] * inlier_t;  // false for a NaN scale
}

__device__ __forceinline__ double align_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double align_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// sums of NV values over the 256 threads of the workgroup in a fixed order (lanes by butterfly, then waves 0..3);
// every thread gets the totals.  red: [4][NV] doubles of LDS
template <int NV>
__device__ __forceinline__ void align_block_sum(double (&v)[NV], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from the previous use
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    v[j] = align_wave_sum(v[j]);
    if (lane == 0) red[wave * NV + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = ((red[j] + red[NV + j]) + red[2 * NV + j]) + red[3 * NV + j];
}

#define ALIGN_RED 12  // doubles per wave of the reduction buffer

// Umeyama over the rows k < n of an instance that KEEP(k) keeps, by the whole 256-thread workgroup: two passes (means,
// then centred moments), the solve on every thread (uniform).  m_out = rows kept.
template <typename Keep>
__device__ __forceinline__ AlignFit align_fit_block(const float* __restrict__ src, const float* __restrict__ dst, int n,
                                                    Keep keep, double* red, int& m_out) {
  const int tid = threadIdx.x;
  double a[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int k = tid; k < n; k += 256) {
    if (keep(k)) {
      a[0] += 1.0;
      a[1] += (double)src[3 * k], a[2] += (double)src[3 * k + 1], a[3] += (double)src[3 * k + 2];
      a[4] += (double)dst[3 * k], a[5] += (double)dst[3 * k + 1], a[6] += (double)dst[3 * k + 2];
    }
  }
  align_block_sum<7>(a, red);
  const double m = a[0];
  m_out = (int)m;
  const double msx = a[1] / m, msy = a[2] / m, msz = a[3] / m, mtx = a[4] / m, mty = a[5] / m, mtz = a[6] / m;
  double c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = tid; k < n; k += 256) {
    if (keep(k)) {
      const double sx = (double)src[3 * k] - msx, sy = (double)src[3 * k + 1] - msy, sz = (double)src[3 * k + 2] - msz;
      const double tx = (double)dst[3 * k] - mtx, ty = (double)dst[3 * k + 1] - mty, tz = (double)dst[3 * k + 2] - mtz;
      c[0] += tx * sx, c[1] += tx * sy, c[2] += tx * sz;
      c[3] += ty * sx, c[4] += ty * sy, c[5] += ty * sz;
      c[6] += tz * sx, c[7] += tz * sy, c[8] += tz * sz;
      c[9] += sx * sx + sy * sy + sz * sz;
    }
  }
  align_block_sum<10>(c, red);
  return align_solve(c[0] / m, c[1] / m, c[2] / m, c[3] / m, c[4] / m, c[5] / m, c[6] / m, c[7] / m, c[8] / m, c[9] / m,
                     msx, msy, msz, mtx, mty, mtz);
}

__device__ __forceinline__ void align_store(const AlignFit& f, bool ok, double* __restrict__ scale, double* __restrict__ R,
                                            double* __restrict__ t) {
  scale[0] = ok ? f.s : 1.0;
  R[0] = ok ? f.r00 : 1.0, R[1] = ok ? f.r01 : 0.0, R[2] = ok ? f.r02 : 0.0;
  R[3] = ok ? f.r10 : 0.0, R[4] = ok ? f.r11 : 1.0, R[5] = ok ? f.r12 : 0.0;
  R[6] = ok ? f.r20 : 0.0, R[7] = ok ? f.r21 : 0.0, R[8] = ok ? f.r22 : 1.0;
  t[0] = ok ? f.t0 : 0.0, t[1] = ok ? f.t1 : 0.0, t[2] = ok ? f.t2 : 0.0;
}

__device__ __forceinline__ int align_count(const int* __restrict__ counts, int inst, int Nmax) {
  const int n = counts ? counts[inst] : Nmax;
  return (n < 0 || n > Nmax) ? 0 : n;  // a count the arrays cannot hold selects nothing
}

// the five draws of (instance key, iteration) under `seed`
__device__ __forceinline__ void align_draw5(unsigned long long seed, unsigned long long key, unsigned it, unsigned n,
                                            int& d0, int& d1, int& d2, int& d3, int& d4) {
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), c0 = (unsigned)key, c1 = (unsigned)(key >> 32);
  const DaugRand q0 = daug_philox(c0, c1, it, 0u, k0, k1), q1 = daug_philox(c0, c1, it, 1u, k0, k1);
  d0 = (int)__umulhi(q0.v[0], n), d1 = (int)__umulhi(q0.v[1], n), d2 = (int)__umulhi(q0.v[2], n);
  d3 = (int)__umulhi(q0.v[3], n), d4 = (int)__umulhi(q1.v[0], n);
}

__global__ __launch_bounds__(ALIGN_MAX_ITER) void k_align_draws(const int* __restrict__ counts, unsigned long long seed,
                                                                const long long* __restrict__ keys, int max_iter,
                                                                int* __restrict__ out /*[I][max_iter][5]*/) {
  const int inst = blockIdx.x, h = threadIdx.x;
  if (h >= max_iter) return;
  const int n = counts[inst] > 0 ? counts[inst] : 0;
  const unsigned long long key = keys ? (unsigned long long)keys[inst] : (unsigned long long)inst;
  int d0, d1, d2, d3, d4;
  align_draw5(seed, key, (unsigned)h, (unsigned)n, d0, d1, d2, d3, d4);
  int* o = out + ((size_t)inst * max_iter + h) * 5;
  o[0] = d0, o[1] = d1, o[2] = d2, o[3] = d3, o[4] = d4;
}

__global__ __launch_bounds__(ALIGN_MAX_ITER) void k_align_hyp(const float* __restrict__ src, const float* __restrict__ dst,
                                                              const int* __restrict__ counts,
                                                              const int* __restrict__ draws, unsigned long long seed,
                                                              const long long* __restrict__ keys, int Nmax, int max_iter,
                                                              double* __restrict__ hyp /*[I][max_iter][16]*/) {
  const int inst = blockIdx.x, h = threadIdx.x;
  if (h >= max_iter) return;
  const int n = align_count(counts, inst, Nmax);
  double* o = hyp + ((size_t)inst * max_iter + h) * ALIGN_HYP_W;
  int d0, d1, d2, d3, d4;
  if (draws) {
    const int* d = draws + ((size_t)inst * max_iter + h) * 5;
    d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
  } else {
    const unsigned long long key = keys ? (unsigned long long)keys[inst] : (unsigned long long)inst;
    align_draw5(seed, key, (unsigned)h, (unsigned)n, d0, d1, d2, d3, d4);
  }
  const unsigned un = (unsigned)n;
  if (n < 5 || (unsigned)d0 >= un || (unsigned)d1 >= un || (unsigned)d2 >= un || (unsigned)d3 >= un || (unsigned)d4 >= un) {
#pragma unroll
    for (int j = 0; j < ALIGN_HYP_W; ++j) o[j] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const float* s = src + (size_t)inst * Nmax * 3;
  const float* t = dst + (size_t)inst * Nmax * 3;
#define ALIGN_PT(P, D, J) \
  const double P##J##x = (double)P[3 * D], P##J##y = (double)P[3 * D + 1], P##J##z = (double)P[3 * D + 2];
  ALIGN_PT(s, d0, 0) ALIGN_PT(s, d1, 1) ALIGN_PT(s, d2, 2) ALIGN_PT(s, d3, 3) ALIGN_PT(s, d4, 4)
  ALIGN_PT(t, d0, 0) ALIGN_PT(t, d1, 1) ALIGN_PT(t, d2, 2) ALIGN_PT(t, d3, 3) ALIGN_PT(t, d4, 4)
#undef ALIGN_PT
  const double msx = ((((s0x + s1x) + s2x) + s3x) + s4x) / 5.0, msy = ((((s0y + s1y) + s2y) + s3y) + s4y) / 5.0,
               msz = ((((s0z + s1z) + s2z) + s3z) + s4z) / 5.0;
  const double mtx = ((((t0x + t1x) + t2x) + t3x) + t4x) / 5.0, mty = ((((t0y + t1y) + t2y) + t3y) + t4y) / 5.0,
               mtz = ((((t0z + t1z) + t2z) + t3z) + t4z) / 5.0;
  double c00 = 0, c01 = 0, c02 = 0, c10 = 0, c11 = 0, c12 = 0, c20 = 0, c21 = 0, c22 = 0, var = 0;
#define ALIGN_ACC(J)                                                                              \
  {                                                                                               \
    const double ax = s##J##x - msx, ay = s##J##y - msy, az = s##J##z - msz;                      \
    const double bx = t##J##x - mtx, by = t##J##y - mty, bz = t##J##z - mtz;                      \
    c00 += bx * ax, c01 += bx * ay, c02 += bx * az;                                               \
    c10 += by * ax, c11 += by * ay, c12 += by * az;                                               \
    c20 += bz * ax, c21 += bz * ay, c22 += bz * az;                                               \
    var += ax * ax + ay * ay + az * az;                                                           \
  }
  ALIGN_ACC(0) ALIGN_ACC(1) ALIGN_ACC(2) ALIGN_ACC(3) ALIGN_ACC(4)
#undef ALIGN_ACC
  const AlignFit f = align_solve(c00 / 5.0, c01 / 5.0, c02 / 5.0, c10 / 5.0, c11 / 5.0, c12 / 5.0, c20 / 5.0, c21 / 5.0,
                                 c22 / 5.0, var / 5.0, msx, msy, msz, mtx, mty, mtz);
  o[0] = f.s * f.r00, o[1] = f.s * f.r01, o[2] = f.s * f.r02;
  o[3] = f.s * f.r10, o[4] = f.s * f.r11, o[5] = f.s * f.r12;
  o[6] = f.s * f.r20, o[7] = f.s * f.r21, o[8] = f.s * f.r22;
  o[9] = f.t0, o[10] = f.t1, o[11] = f.t2;
  o[12] = f.s, o[13] = 0.0, o[14] = 0.0, o[15] = 0.0;
}

__global__ __launch_bounds__(256) void k_align_ransac(const float* __restrict__ src, const float* __restrict__ dst,
                                                      const int* __restrict__ counts, const double* __restrict__ hyp,
                                                      int Nmax, int max_iter, double confidence, double min_inlier_ratio,
                                                      double* __restrict__ scale_out, double* __restrict__ R_out,
                                                      double* __restrict__ t_out, int* __restrict__ valid_out,
                                                      int* __restrict__ ninl_out, int* __restrict__ iters_out,
                                                      int* __restrict__ best_it_out, unsigned char* __restrict__ mask_out) {
  __shared__ double sh_hyp[ALIGN_MAX_ITER * ALIGN_HYP_W];
  __shared__ double red[4 * ALIGN_RED];
  __shared__ int sh_cnt[ALIGN_HB];
  __shared__ int sh_state[4];  // best count, best iteration, iterations evaluated, stop
  const int inst = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = align_count(counts, inst, Nmax);
  const float* s = src + (size_t)inst * Nmax * 3;
  const float* t = dst + (size_t)inst * Nmax * 3;
  unsigned char* mask = mask_out ? mask_out + (size_t)inst * Nmax : nullptr;
  AlignFit fit = {};
  bool ok = false;
  int ninl = 0, iters = 0, best_it = -1;
  double inlier_t = 0.0;

  // mean of src, and whether every value of the first n rows is finite
  double a[4] = {0, 0, 0, 0};
  for (int k = tid; k < n; k += 256) {
    const double sx = (double)s[3 * k], sy = (double)s[3 * k + 1], sz = (double)s[3 * k + 2];
    const double all = ((sx + sy) + sz) + (((double)t[3 * k] + (double)t[3 * k + 1]) + (double)t[3 * k + 2]);
    a[0] += sx, a[1] += sy, a[2] += sz;
    a[3] += (all - all == 0.0) ? 0.0 : 1.0;  // inf - inf and NaN - NaN are NaN
  }
  align_block_sum<4>(a, red);
  const bool usable = n >= 5 && a[3] == 0.0;  // uniform over the workgroup
  if (usable) {
    const double cx = a[0] / (double)n, cy = a[1] / (double)n, cz = a[2] / (double)n;
    double far2 = 0.0;
    for (int k = tid; k < n; k += 256) {
      const double ex = (double)s[3 * k] - cx, ey = (double)s[3 * k + 1] - cy, ez = (double)s[3 * k + 2] - cz;
      far2 = fmax(far2, ex * ex + ey * ey + ez * ez);
    }
    far2 = align_wave_max(far2);
    __syncthreads();
    if (lane == 0) red[wave] = far2;
    for (int j = tid; j < max_iter * ALIGN_HYP_W; j += 256) sh_hyp[j] = hyp[(size_t)inst * max_iter * ALIGN_HYP_W + j];
    if (tid == 0) sh_state[0] = 0, sh_state[1] = -1, sh_state[2] = max_iter, sh_state[3] = 0;
    __syncthreads();
    inlier_t = 2.0 * sqrt(fmax(fmax(red[0], red[1]), fmax(red[2], red[3]))) / 10.0;

    for (int h0 = 0; h0 < max_iter; h0 += ALIGN_HB) {
      const int nh = min(ALIGN_HB, max_iter - h0);
      if (tid < ALIGN_HB) sh_cnt[tid] = 0;
      __syncthreads();
      int acc = 0;  // lane hl holds this wave's count of hypothesis h0 + hl
      for (int base = wave * 64; base < n; base += 256) {
        const int k = base + lane;
        const bool in = k < n;
        const int kk = in ? k : 0;
        const double sx = (double)s[3 * kk], sy = (double)s[3 * kk + 1], sz = (double)s[3 * kk + 2];
        const double dx = (double)t[3 * kk], dy = (double)t[3 * kk + 1], dz = (double)t[3 * kk + 2];
        for (int hl = 0; hl < nh; ++hl) {
          const bool inl = in && align_inlier(sh_hyp + (h0 + hl) * ALIGN_HYP_W, inlier_t, sx, sy, sz, dx, dy, dz);
          const int c = __popcll(__ballot(inl));
          acc += lane == hl ? c : 0;
        }
      }
      if (lane < nh && acc) atomicAdd(&sh_cnt[lane], acc);
      __syncthreads();
      if (tid == 0) {  // selection and stop rule, in draw order
        int best = sh_state[0], bit = sh_state[1];
        for (int hl = 0; hl < nh; ++hl) {
          const int it = h0 + hl, c = sh_cnt[hl];
          if (c > best) best = c, bit = it;
          const double r = (double)best / (double)n;
          double base = 1.0 - (r * r) * (r * r) * r, p = 1.0;  // (1 - best^5)^it by squaring
          for (int e = it; e > 0; e >>= 1) {
            if (e & 1) p *= base;
            base *= base;
          }
          if (1.0 - p > confidence) {
            sh_state[2] = it + 1, sh_state[3] = 1;
            break;
          }
        }
        sh_state[0] = best, sh_state[1] = bit;
      }
      __syncthreads();
      if (sh_state[3]) break;
    }
    ninl = sh_state[0], best_it = sh_state[1], iters = sh_state[2];
    ok = best_it >= 0 && !((double)ninl / (double)n < min_inlier_ratio);
  }
  // the winner's inlier set: the mask, and the final fit over it
  const double* hb = sh_hyp + (best_it >= 0 ? best_it : 0) * ALIGN_HYP_W;
  auto keep = [&](int k) {
    return align_inlier(hb, inlier_t, (double)s[3 * k], (double)s[3 * k + 1], (double)s[3 * k + 2], (double)t[3 * k],
                        (double)t[3 * k + 1], (double)t[3 * k + 2]);
  };
  if (mask) {
    const bool have = usable && best_it >= 0;
    for (int k = tid; k < Nmax; k += 256) mask[k] = (have && k < n && keep(k)) ? 1 : 0;
  }
  if (ok) {  // uniform
    int m;
    fit = align_fit_block(s, t, n, keep, red, m);
    ninl = m;
    ok = align_finite(fit);
  }
  if (tid == 0) {
    align_store(fit, ok, scale_out + inst, R_out + inst * 9, t_out + inst * 3);
    valid_out[inst] = ok ? 1 : 0;
    ninl_out[inst] = ninl;
    iters_out[inst] = iters;
    best_it_out[inst] = best_it;
  }
}

__global__ __launch_bounds__(256) void k_umeyama(const float* __restrict__ src, const float* __restrict__ dst,
                                                 const int* __restrict__ counts, const unsigned char* __restrict__ mask,
                                                 int Nmax, double* __restrict__ scale_out, double* __restrict__ R_out,
                                                 double* __restrict__ t_out, int* __restrict__ valid_out) {
  __shared__ double red[4 * ALIGN_RED];
  const int inst = blockIdx.x;
  const int n = align_count(counts, inst, Nmax);
  const float* s = src + (size_t)inst * Nmax * 3;
  const float* t = dst + (size_t)inst * Nmax * 3;
  const unsigned char* mk = mask ? mask + (size_t)inst * Nmax : nullptr;
  auto keep = [&](int k) { return mk ? mk[k] != 0 : true; };
  int m;
  const AlignFit fit = align_fit_block(s, t, n, keep, red, m);
  const bool ok = m > 0 && align_finite(fit);
  if (threadIdx.x == 0) {
    align_store(fit, ok, scale_out + inst, R_out + inst * 9, t_out + inst * 3);
    if (valid_out) valid_out[inst] = ok ? 1 : 0;
  }
}
