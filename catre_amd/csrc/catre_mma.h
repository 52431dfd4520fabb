// catre_mma.h - device helpers of the bf16-pipe kernels (inference forms in catre_bf16.h / catre_split.h, training GEMMs in
// catre_train.h): operand types, bf16 / fp16 packing, the row loads of mixed-precision activations, the swizzled chunk
// addressing and the K-sweep pipes GemmPipeB (bf16 / fp16 operands) and GemmPipeS (hi + lo split operands).  No kernels.
// The LDS image and packed-weight layouts are described at the top of catre_bf16.h.
#pragma once
#include "catre_device.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x16 mfma_bf(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0,
                                                 0, 0);
}

__device__ __forceinline__ unsigned pack_bf2(float lo, float hi) {  // v_cvt_pk_bf16_f32 (RNE)
  typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  f2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf2));
}
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

__device__ __forceinline__ u32x4 pack_bf8(const float (&v)[8]) {
  u32x4 w;
  w[0] = pack_bf2(v[0], v[1]);
  w[1] = pack_bf2(v[2], v[3]);
  w[2] = pack_bf2(v[4], v[5]);
  w[3] = pack_bf2(v[6], v[7]);
  return w;
}

// Operand type of the reduced-precision INFERENCE kernels (template argument OT): its three type-specific pieces - the
// MFMA, narrowing (RNE) and widening of a packed pair.  OpBf16 is the bf16 path above (widening by bits); OpF16 takes
// fp16 operands (COMPUTE_DTYPE="fp16", the dtype of the reference's autocast on "cuda"): the same layouts, the same
// rounding points, v_mfma_f32_32x32x16_f16 at the bf16 form's rate, v_cvt_pk_f16_f32 to narrow (RNE - the pkrtz form
// rounds toward zero) and v_cvt_f32_f16 to widen.  The training (SAVE) forms and the backward kernels stay bf16-only.
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
struct OpBf16 {
  typedef __bf16 T;
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) { return mfma_bf(a, b, c); }
  static __device__ __forceinline__ unsigned pack2(float lo, float hi) { return pack_bf2(lo, hi); }
  static __device__ __forceinline__ float lo(unsigned u) { return bf_lo(u); }
  static __device__ __forceinline__ float hi(unsigned u) { return bf_hi(u); }
};
struct OpF16 {
  typedef _Float16 T;
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0,
                                                  0);
  }
  static __device__ __forceinline__ unsigned pack2(float lo, float hi) {  // v_cvt_pk_f16_f32 (RNE)
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
  }
  static __device__ __forceinline__ float lo(unsigned u) { return (float)__builtin_bit_cast(f16x2_t, u)[0]; }
  static __device__ __forceinline__ float hi(unsigned u) { return (float)__builtin_bit_cast(f16x2_t, u)[1]; }
};
template <class OT>
constexpr bool is_f16_op() {
  return __is_same(OT, OpF16);
}

template <class OT>
__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
  u32x4 w;
  w[0] = OT::pack2(v[0], v[1]);
  w[1] = OT::pack2(v[2], v[3]);
  w[2] = OT::pack2(v[4], v[5]);
  w[3] = OT::pack2(v[6], v[7]);
  return w;
}

// rows of 256 channels stored as fp32 (HB = false) or bf16 (HB = true): four consecutive channels of row-quad index i4
// (= row * 64 + channel / 4).  The reduced-precision training heads keep their [rows,256] activations in bf16 - what
// torch.autocast's Conv1d outputs are (engine.py:304) - and every pass over them moves half the bytes.
template <bool HB>
__device__ __forceinline__ f32x4 ld_row4(const void* __restrict__ p, size_t i4) {
  if constexpr (HB) {
    const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p) + i4);
    return f32x4{bf_lo(v[0]), bf_hi(v[0]), bf_lo(v[1]), bf_hi(v[1])};
  } else {
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i4);
  }
}
// four consecutive channels of a bf16 row as floats, through the caches (operand rows that several workgroups re-read:
// the gathered rows of the row-sparse backward)
__device__ __forceinline__ f32x4 ld_bf4(const void* __restrict__ p, size_t i4) {
  const u32x2 v = reinterpret_cast<const u32x2*>(p)[i4];
  return f32x4{bf_lo(v[0]), bf_hi(v[0]), bf_lo(v[1]), bf_hi(v[1])};
}
template <bool HB>
__device__ __forceinline__ void st_row4(void* __restrict__ p, size_t i4, const f32x4& v) {
  if constexpr (HB)
    reinterpret_cast<u32x2*>(p)[i4] = u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
  else
    reinterpret_cast<f32x4*>(p)[i4] = v;
}

// ... and the form for loads that are requested long before they are used (the prefetch rings of k_rot_l1_bwd_bf /
// k_rot_l0_bwd_bf): the RAW quad stays in the ring - a conversion right behind the load would wait for it - and is widened
// where it is consumed.  rowq_pair: column q of two rows as one packed bf16 pair (first row in the low half).
template <bool HB>
struct RowQ {
  typedef f32x4 T;
};
template <>
struct RowQ<true> {
  typedef u32x2 T;
};
template <bool HB>
__device__ __forceinline__ typename RowQ<HB>::T ld_rowq(const void* __restrict__ p, size_t i4) {
  return __builtin_nontemporal_load(reinterpret_cast<const typename RowQ<HB>::T*>(p) + i4);
}
__device__ __forceinline__ f32x4 rowq_f32(const f32x4& v) { return v; }
__device__ __forceinline__ f32x4 rowq_f32(const u32x2& v) { return f32x4{bf_lo(v[0]), bf_hi(v[0]), bf_lo(v[1]), bf_hi(v[1])}; }
__device__ __forceinline__ unsigned rowq_pair(const f32x4& a, const f32x4& b, int q) { return pack_bf2(a[q], b[q]); }
__device__ __forceinline__ unsigned rowq_pair(const u32x2& a, const u32x2& b, int q) {
  // v_perm_b32: bytes 4-7 = first operand, 0-3 = second
  return (q & 1) ? __builtin_amdgcn_perm(b[q >> 1], a[q >> 1], 0x07060302u) : __builtin_amdgcn_perm(b[q >> 1], a[q >> 1], 0x05040100u);
}

template <int CP>
__device__ __forceinline__ int bf_key(int row) {
  return CP >= 16 ? (row & 15) : ((row >> 1) & (CP - 1));
}
template <int CP>
__device__ __forceinline__ int bf_off(int row, int chunk) {
  return row * CP + (chunk ^ bf_key<CP>(row));
}

// K-sweep of a wave tile of MB x NB 32x32 blocks, K = 8*CP (CP chunks per LDS row, NKC = CP/2 MFMA steps).
// Same software pipeline as GemmPipe: weight fragments stream L2 -> registers PFD steps ahead, activation
// fragments LDS -> registers PFB steps ahead, both pinned with sched_barrier.
// XA (K >= 128 only): the image base is aligned to its row pitch, so the swizzled fragment address is ONE v_xor of a
// per-lane base with a compile-time constant - (chunk ^ key) << 4 == (chunk << 4) ^ (key << 4), and neither overlaps the
// row bits - instead of eight (sixteen past 64 KiB) per-lane pointers held across the sweep.
typedef __attribute__((address_space(3))) const u32x4 lds_cu32x4;
template <int MB, int NB, bool SWAP, int CP, int PFD, int PFB = 1, bool XA = false, class OT = OpBf16>
struct GemmPipeB {
  static constexpr int NKC = CP / 2;
  static_assert(PFD >= 1 && PFD <= NKC && PFB >= 1 && PFB <= PFD, "prefetch depth");
  static constexpr int RA = PFD + 1, RB = PFB + 1;
  u32x4 a[RA][MB], b[RB][NB];
  const u32x4* wp;
  int wp_mb;
  int ablate = 0;  // instrumented build only (catre_debug_knob 1): skip operand loads to price them; always 0 in the product

  __device__ __forceinline__ void issue_a(int kc) {
    if (CATRE_TRACE_ON && (ablate & 1) && kc >= PFD) return;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) a[kc % RA][mb] = wp[mb * wp_mb + kc * 64];
  }
  __device__ __forceinline__ void prefetch(const u32x4* __restrict__ wp_, int wp_mb_) {
    wp = wp_;
    wp_mb = wp_mb_;
#pragma unroll
    for (int d = 0; d < PFD; ++d) issue_a(d);
    __builtin_amdgcn_sched_barrier(0);
  }
  // x: image row of point 0 of this wave tile (a multiple of 32 rows into the image)
  __device__ __forceinline__ void run(f32x16 (&acc)[MB][NB], const u32x4* x, int lane) {
    run(acc, x, lane, [](int) {});
  }
  // hook(kc) runs before the loads of K-step kc are issued (k_trunk_bf2 re-balances the two waves of a SIMD there)
  template <class Hook>
  __device__ __forceinline__ void run(f32x16 (&acc)[MB][NB], const u32x4* x, int lane, Hook hook) {
    const int n = lane & 31, h = lane >> 5, key = bf_key<CP>(n);
    const u32x4* xrow = x + n * CP;
    // rows of >= 256 B: the XOR key (< 16) only touches the low four bits of the chunk index 2*kc + h, so eight per-lane
    // pointers (kc & 7) + compile-time offsets (kc >> 3, nb) address every fragment - no address arithmetic in the sweep
    // (left to itself the compiler keeps one swizzled index per kc in registers: 32 of them for K = 512)
    const u32x4* xl[8];
    if constexpr (CP >= 16 && !XA) {
#pragma unroll
      for (int lo = 0; lo < 8; ++lo) xl[lo] = xrow + ((2 * lo + h) ^ key);
    }
    unsigned xa0 = 0;  // XA: LDS byte address of (row n, chunk h ^ key)
    if constexpr (XA) {
      static_assert(CP >= 16, "XA needs rows of >= 256 B");
      xa0 = (unsigned)(size_t)(lds_cu32x4*)xrow ^ (unsigned)((h ^ key) << 4);
    }
    auto issue_b = [&](int kc) {
      if (CATRE_TRACE_ON && (ablate & 2) && kc >= PFB) return;
      if constexpr (XA) {
        // two point blocks (2 x 32 rows) per 16-bit ds offset window
        unsigned a;
        asm volatile("v_xor_b32 %0, %1, %2" : "=v"(a) : "i"(kc << 5), "v"(xa0));
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          constexpr int WIN = 65536 / (32 * CP * 16);  // point blocks per 64 KiB
          static_assert(WIN >= 1, "row block larger than the ds offset window");
          const unsigned aw = a + (unsigned)((nb / WIN) * WIN * 32 * CP * 16);
          b[kc % RB][nb] = *(lds_cu32x4*)(size_t)(aw + (unsigned)((nb % WIN) * 32 * CP * 16));
        }
      } else {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          if constexpr (CP >= 16)
            b[kc % RB][nb] = xl[kc & 7][nb * 32 * CP + 16 * (kc >> 3)];
          else
            b[kc % RB][nb] = xrow[nb * 32 * CP + ((2 * kc + h) ^ key)];
        }
      }
    };
#pragma unroll
    for (int d = 0; d < PFB; ++d) issue_b(d);
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      hook(kc);
      if (kc + PFD < NKC) issue_a(kc + PFD);
      if (kc + PFB < NKC) issue_b(kc + PFB);
      __builtin_amdgcn_sched_barrier(0);
      const int ca = kc % RA, cb = kc % RB;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          acc[mb][nb] = SWAP ? OT::mfma(b[cb][nb], a[ca][mb], acc[mb][nb]) : OT::mfma(a[ca][mb], b[cb][nb], acc[mb][nb]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
};

__device__ __forceinline__ void split_bf8(const float (&v)[8], u32x4& hi, u32x4& lo) {
  float r[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    hi[i] = pack_bf2(v[2 * i], v[2 * i + 1]);
    r[2 * i] = v[2 * i] - bf_lo(hi[i]);
    r[2 * i + 1] = v[2 * i + 1] - bf_hi(hi[i]);
  }
  lo = pack_bf8(r);
}

// K-sweep with split operands.  wp: hi fragments of the wave's first m-block, the lo fragments sit `lo_off` u32x4
// further; xh / xl: hi and lo images (row of point 0 of the wave tile).  Per K=16 step and (mb, nb): 3 MFMAs.
template <int MB, int NB, bool SWAP, int CP, int PFD>
struct GemmPipeS {
  static constexpr int NKC = CP / 2;
  static_assert(PFD >= 1 && PFD <= NKC, "prefetch depth");
  static constexpr int RA = PFD + 1;
  u32x4 ah[RA][MB], al[RA][MB], bh[2][NB], bl[2][NB];
  const u32x4* wp;
  int wp_mb, lo_off;

  __device__ __forceinline__ void issue_a(int kc) {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      ah[kc % RA][mb] = wp[mb * wp_mb + kc * 64];
      al[kc % RA][mb] = wp[lo_off + mb * wp_mb + kc * 64];
    }
  }
  __device__ __forceinline__ void prefetch(const u32x4* __restrict__ wp_, int wp_mb_, int lo_off_) {
    wp = wp_;
    wp_mb = wp_mb_;
    lo_off = lo_off_;
#pragma unroll
    for (int d = 0; d < PFD; ++d) issue_a(d);
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void run(f32x16 (&acc)[MB][NB], const u32x4* xh, const u32x4* xl, int lane) {
    const int n = lane & 31, h = lane >> 5, key = bf_key<CP>(n);
    const u32x4* rh = xh + n * CP;
    const u32x4* rl = xl + n * CP;
    auto issue_b = [&](int kc) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        bh[kc & 1][nb] = rh[nb * 32 * CP + ((2 * kc + h) ^ key)];
        bl[kc & 1][nb] = rl[nb * 32 * CP + ((2 * kc + h) ^ key)];
      }
    };
    issue_b(0);
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      if (kc + PFD < NKC) issue_a(kc + PFD);
      if (kc + 1 < NKC) issue_b(kc + 1);
      __builtin_amdgcn_sched_barrier(0);
      const int ca = kc % RA, cb = kc & 1;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          if (SWAP) {
            acc[mb][nb] = mfma_bf(bh[cb][nb], al[ca][mb], acc[mb][nb]);
            acc[mb][nb] = mfma_bf(bl[cb][nb], ah[ca][mb], acc[mb][nb]);
            acc[mb][nb] = mfma_bf(bh[cb][nb], ah[ca][mb], acc[mb][nb]);
          } else {
            acc[mb][nb] = mfma_bf(al[ca][mb], bh[cb][nb], acc[mb][nb]);
            acc[mb][nb] = mfma_bf(ah[ca][mb], bl[cb][nb], acc[mb][nb]);
            acc[mb][nb] = mfma_bf(ah[ca][mb], bh[cb][nb], acc[mb][nb]);
          }
        }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
};
