// catre_optim.h - f4: the fused multi-tensor optimizer steps, Ranger first, then the reference's other optimizers.
#pragma once
#include "catre_device.h"

// ------------------------------------------------------------------------------------------------
// f4: fused multi-tensor Ranger step (RAdam + Lookahead + gradient centralization) with the train loop's
// grad nan_to_num folded in.  Replaces the per-tensor Python loop of lib/torch_utils/solver/ranger.py:102-202
// (~70 tensors x ~15 torch ops, K times per data batch) and core/catre/engine/engine.py:351-353.
// The host computes the scalar step sizes; the device table carries one RangerTensor per parameter.
// ------------------------------------------------------------------------------------------------
struct RangerTensor {
  float* p;
  const float* g;
  float* m;      // exp_avg
  float* v;      // exp_avg_sq
  float* slow;   // lookahead slow weights
  int numel;
  int row_len;   // > 0: centralize the gradient over rows of this length (dims 1.. of a conv / fc weight)
  int row_off;   // first slot of this tensor in the row-mean buffer
  float lr_step; // step_size * lr
  float wd_lr;   // weight_decay * lr
  int adaptive;  // N_sma > threshold: divide by sqrt(v) + eps
  int lookahead; // step % k == 0: merge into the slow weights
  int pad;
};
static_assert(sizeof(RangerTensor) == 72, "host packs this struct with the same layout");

__device__ __forceinline__ float ranger_clean(float g, int clean, float lim) {
  // torch.nan_to_num(g, nan=0, posinf=lim, neginf=-lim) (engine.py:351-353): finite values pass unchanged
  if (!clean) return g;
  if (g != g) return 0.f;
  return g == INFINITY ? lim : (g == -INFINITY ? -lim : g);
}

// one wave per (tensor, row): mean of the (cleaned) gradient row
__global__ __launch_bounds__(64) void k_ranger_rowmean(const RangerTensor* __restrict__ T, const int* __restrict__ row_tensor,
                                                       float* __restrict__ rowmean, int clean, float lim) {
  const int row = blockIdx.x;
  const RangerTensor t = T[row_tensor[row]];
  const int r = row - t.row_off;
  const float* g = t.g + (size_t)r * t.row_len;
  float s = 0.f;
  int i = threadIdx.x;
  for (; i + 192 < t.row_len; i += 256) {  // four loads requested together, added in the loop's order (same bits)
    const float a = g[i], b = g[i + 64], c = g[i + 128], d = g[i + 192];
    s += ranger_clean(a, clean, lim);
    s += ranger_clean(b, clean, lim);
    s += ranger_clean(c, clean, lim);
    s += ranger_clean(d, clean, lim);
  }
  for (; i < t.row_len; i += 64) s += ranger_clean(g[i], clean, lim);
  s = wave_sum(s);
  if (threadIdx.x == 0) rowmean[row] = s / (float)t.row_len;
}

#define RANGER_CHUNK 4096
__global__ __launch_bounds__(256) void k_ranger_update(const RangerTensor* __restrict__ T, const int2* __restrict__ chunks,
                                                       const float* __restrict__ rowmean, float beta1, float omb1,
                                                       float beta2, float omb2, float eps, float alpha, int clean,
                                                       float lim) {
  const int2 c = chunks[blockIdx.x];
  const RangerTensor t = T[c.x];
  const int end = min(t.numel, c.y + RANGER_CHUNK);
  // four elements per thread and trip, every load of the trip requested before the first store (the tensors may alias as far
  // as the compiler knows: as a plain loop each element waited for the previous one's stores - 16 dependent round trips)
  for (int i0 = c.y + threadIdx.x; i0 < end; i0 += 1024) {
    float g[4], v[4], m[4], p[4], sl[4], rm[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(i0 + 256 * u, end - 1);
      g[u] = t.g[i], v[u] = t.v[i], m[u] = t.m[i], p[u] = t.p[i];
      sl[u] = t.lookahead ? t.slow[i] : 0.f;
      rm[u] = t.row_len > 0 ? rowmean[t.row_off + i / t.row_len] : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
      if (i < end) {
        float gg = ranger_clean(g[u], clean, lim);
        if (t.row_len > 0) gg -= rm[u];
        // omb = fp32(1 - beta) formed in double on the host like the reference's `1 - beta2` (1.f - 0.999f is off by 4.7e-5)
        const float vv = v[u] * beta2 + omb2 * gg * gg;
        const float mm = m[u] * beta1 + omb1 * gg;
        t.v[i] = vv;
        t.m[i] = mm;
        float pp = p[u];
        if (t.wd_lr != 0.f) pp -= t.wd_lr * pp;
        pp -= t.adaptive ? t.lr_step * (mm / (sqrtf(vv) + eps)) : t.lr_step * mm;
        if (t.lookahead) {
          const float s = sl[u] + alpha * (pp - sl[u]);
          t.slow[i] = s;
          pp = s;
        }
        t.p[i] = pp;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// f4, continued: fused multi-tensor steps for the reference's other optimizers (lib/torch_utils/solver/):
// AdaBelief (AdaBelief.py:113-218), RangerAdaBelief (ranger_adabelief.py:133-265), MADGRAD (madgrad.py:72-175),
// NAdamW (nadamw.py:58-134), AdamP (adamp.py:48-123), SGDP (sgdp.py:50-113), SGD_GC / SGD_GCC (sgd_gc.py:42-180).
// Modelled on k_ranger_rowmean / k_ranger_update (above): a device table with one OptimTensor per parameter,
// chunks of 4096 elements, one wave per (tensor, row) for row reductions.  Every scalar term (bias corrections,
// rectification, NAdamW's mu products, MADGRAD's lamb, `1 - beta`) is formed on the host in double and arrives as fp32
// in OptimTensor::f, per tensor, so param groups may differ in every hyper-parameter.
//
// Three phases, each launched only when a tensor of the step needs it:
//   1. reductions over the inputs: row means of the gradient (centralization), or g.p |g|^2 |p|^2 per row and the
//      channel / layer / none decision of AdamP's and SGDP's projection (one wave per tensor, rows in a fixed order);
//   2. reductions over the update direction, which is recomputed from the inputs without writing state: the row mean of
//      G_grad (RangerAdaBelief gc_loc=False), sum(p_n * perturb) per row and per tensor (projection);
//   3. the elementwise update, which writes parameters and state.
// No atomics: every sum has a fixed order, so a step is deterministic and an element's result does not depend on which
// other tensors share the launch.
// ------------------------------------------------------------------------------------------------
struct OptimTensor {
  float* p;
  const float* g;
  float* s[4];   // state buffers, meaning per kind (see optim_dir)
  int numel;
  int row_len;   // > 0: this tensor has rows in the workspace (centralization or projection)
  int row_off;   // its first row there
  int flags;     // OPT_F_*
  float f[12];   // per-tensor scalars, meaning per kind
};
static_assert(sizeof(OptimTensor) == 112, "host packs this struct with the same layout");

enum { OPT_ADABELIEF = 0, OPT_RANGER_ADABELIEF = 1, OPT_MADGRAD = 2, OPT_NADAMW = 3, OPT_ADAMP = 4, OPT_SGDP = 5, OPT_SGD_GC = 6,
       OPT_KINDS = 7 };
enum {
  OPT_F_ADAPT = 1,     // divide by the denominator (rectified / RAdam branch taken)
  OPT_F_AMS = 2,       // amsgrad: s[2] = running maximum
  OPT_F_PMUL = 4,      // multiply the parameter by f[5] first (decoupled weight decay)
  OPT_F_WDGRAD = 8,    // g += f[6] * p (weight decay into the gradient)
  OPT_F_BELIEF = 16,   // RangerAdaBelief(adabelief=True)
  OPT_F_WDDEC = 32,    // RangerAdaBelief: G_grad += f[5] * p
  OPT_F_GC_IN = 64,    // centralize the gradient with the phase-1 row mean
  OPT_F_GC_OUT = 128,  // centralize G_grad with the phase-2 row mean
  OPT_F_LOOK = 256,    // lookahead merge into s[2]
  OPT_F_MOM = 512,     // momentum != 0
  OPT_F_FIRST = 1024,  // SGD_GC: first step, the buffer becomes a copy of the gradient
  OPT_F_NEST = 2048,   // nesterov
  OPT_F_PROJ = 4096,   // AdamP / SGDP: p.dim() > 1, the projection is considered
};
// workspace: rowA[4 * n_rows] (phase 1: mean | g.p, |g|^2, |p|^2), rowB[n_rows] (phase 2), tens[4 * n_tensors] (view, |p|, sum)
#define OPT_CHUNK 4096

// torch.max(a, b): a NaN in either operand comes out (fmaxf would drop it)
__device__ __forceinline__ float optim_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }

struct OptimElem {
  float g, p, a, b, c;  // gradient, parameter, s[0], s[1], s[2]
};

// New state (in e.a / e.b / e.c) and the update direction of one element, before centralization of the direction or the
// projection.  `e.p` is the parameter after its own decay (what the reference's later lines read).
template <int KIND>
__device__ __forceinline__ float optim_dir(const OptimTensor& t, OptimElem& e, float rm_in) {
  const int fl = t.flags;
  const float* f = t.f;
  if (KIND == OPT_ADABELIEF) {  // a = exp_avg, b = exp_avg_var, c = max_exp_avg_var
    if (fl & OPT_F_PMUL) e.p *= f[5];                // :171-175
    if (fl & OPT_F_WDGRAD) e.g += f[6] * e.p;        // :178
    e.a = e.a * f[0] + f[1] * e.g;                   // :181
    const float r = e.g - e.a;
    e.b = e.b * f[2] + f[3] * r * r;                 // :183
    float den;
    if (fl & OPT_F_AMS) {
      e.c = optim_max(e.c, e.b) + f[4];              // :188-191, eps added in place
      den = sqrtf(e.c) / f[7] + f[4];
    } else {
      e.b += f[4];                                   // :193
      den = sqrtf(e.b) / f[7] + f[4];
    }
    return (fl & OPT_F_ADAPT) ? e.a / den : e.a;     // :198 / :213 / :216
  }
  if (KIND == OPT_RANGER_ADABELIEF) {  // a = exp_avg, b = exp_avg_sq, c = slow_buffer
    if (fl & OPT_F_WDGRAD) e.g += e.p * f[6];        // :151
    if (fl & OPT_F_GC_IN) e.g -= rm_in;              // :183-188
    e.a = e.a * f[0] + f[1] * e.g;                   // :193
    if (fl & OPT_F_BELIEF) {
      const float r = e.g - e.a;
      e.b = e.b * f[2] + f[3] * r * r;               // :197
    } else {
      e.b = e.b * f[2] + f[3] * e.g * e.g;           // :199
    }
    float G = e.a;
    if (fl & OPT_F_ADAPT) {
      if (fl & OPT_F_BELIEF) e.b += f[4];            // :232, in place
      G = e.a / (sqrtf(e.b) + f[4]);                 // :232-236
    }
    if (fl & OPT_F_WDDEC) G += f[5] * e.p;           // :241
    return G;
  }
  if (KIND == OPT_MADGRAD) {  // a = grad_sum_sq, b = s, c = x0
    const float third = (float)(1.0 / 3.0);          // torch's pow(1 / 3) on fp32 rounds the exponent to fp32
    if (fl & OPT_F_WDGRAD) e.g += f[2] * e.p;        // :121
    float x0 = e.c;
    if (!(fl & OPT_F_MOM)) x0 = e.p + e.b / (powf(e.a, third) + f[1]);  // :153-154
    e.a = e.a + f[0] * e.g * e.g;                    // :159
    const float rms = powf(e.a, third) + f[1];       // :160
    e.b = e.b + f[0] * e.g;                          // :163
    return x0 - e.b / rms;                           // z (:167 / :169)
  }
  if (KIND == OPT_NADAMW) {  // a = exp_avg, b = exp_avg_sq, c = max_exp_avg_sq
    e.p *= f[5];                                     // :77
    e.a = e.a * f[0] + f[1] * e.g;                   // :120
    e.b = e.b * f[2] + f[3] * e.g * e.g;             // :121
    float den;
    if (fl & OPT_F_AMS) {
      e.c = optim_max(e.c, e.b);                     // :124
      den = sqrtf(e.c) / f[7] + f[4];
    } else {
      den = sqrtf(e.b) / f[7] + f[4];                // :128
    }
    return den;  // the caller applies both addcdiv_ of :131-132
  }
  if (KIND == OPT_ADAMP) {  // a = exp_avg, b = exp_avg_sq
    e.a = e.a * f[0] + f[1] * e.g;                   // :93
    e.b = e.b * f[2] + f[3] * e.g * e.g;             // :94
    const float den = sqrtf(e.b) / f[7] + f[4];      // :96
    return (fl & OPT_F_NEST) ? (f[0] * e.a + f[1] * e.g) / den : e.a / den;  // :100 / :102
  }
  if (KIND == OPT_SGDP) {  // a = momentum
    e.a = e.a * f[0] + f[1] * e.g;                   // :88
    return (fl & OPT_F_NEST) ? e.g + f[0] * e.a : e.a;  // :90 / :92
  }
  // OPT_SGD_GC / SGD_GCC: a = momentum_buffer
  if (fl & OPT_F_WDGRAD) e.g += f[6] * e.p;          // sgd_gc.py:65 / :153
  if (fl & OPT_F_GC_IN) e.g -= rm_in;                // :68-76 / :156-164
  if (!(fl & OPT_F_MOM)) return e.g;
  e.a = (fl & OPT_F_FIRST) ? e.g : e.a * f[0] + f[1] * e.g;  // :81 / :84
  return (fl & OPT_F_NEST) ? e.g + f[0] * e.a : e.a;  // :86 / :88
}

template <int KIND>
__device__ __forceinline__ OptimElem optim_load(const OptimTensor& t, int i, int clean, float lim) {
  OptimElem e;
  e.g = ranger_clean(t.g[i], clean, lim);
  e.p = t.p[i];
  e.a = e.b = e.c = 0.f;
  if (KIND == OPT_SGD_GC) {
    if ((t.flags & OPT_F_MOM) && !(t.flags & OPT_F_FIRST)) e.a = t.s[0][i];
    return e;
  }
  e.a = t.s[0][i];
  if (KIND == OPT_SGDP) return e;
  e.b = t.s[1][i];
  if (KIND == OPT_ADAMP) return e;
  if (KIND == OPT_RANGER_ADABELIEF) {
    if (t.flags & OPT_F_LOOK) e.c = t.s[2][i];
  } else if (KIND == OPT_MADGRAD) {
    if (t.flags & OPT_F_MOM) e.c = t.s[2][i];
  } else if (t.flags & OPT_F_AMS) {
    e.c = t.s[2][i];
  }
  return e;
}

// ---- phase 1 -------------------------------------------------------------------------------------------------
// one wave per (tensor, row): mean of the cleaned gradient row, with the weight decay that enters the gradient
__global__ __launch_bounds__(64) void k_optim_rowmean(const OptimTensor* __restrict__ T, const int* __restrict__ row_tensor,
                                                      float* __restrict__ rowA, int clean, float lim) {
  const int row = blockIdx.x;
  const OptimTensor t = T[row_tensor[row]];
  if (!(t.flags & OPT_F_GC_IN)) return;
  const size_t base = (size_t)(row - t.row_off) * t.row_len;
  const float* g = t.g + base;
  const float* p = t.p + base;
  const bool wd = t.flags & OPT_F_WDGRAD;
  const float w = t.f[6];
  float s = 0.f;
  for (int i = threadIdx.x; i < t.row_len; i += 64) {
    float v = ranger_clean(g[i], clean, lim);
    if (wd) v += w * p[i];
    s += v;
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) rowA[(size_t)row * 4] = s / (float)t.row_len;
}

// one wave per (tensor, row): g.p, |g|^2, |p|^2 of the row
__global__ __launch_bounds__(64) void k_optim_rowstats(const OptimTensor* __restrict__ T, const int* __restrict__ row_tensor,
                                                       float* __restrict__ rowA, int clean, float lim) {
  const int row = blockIdx.x;
  const OptimTensor t = T[row_tensor[row]];
  if (!(t.flags & OPT_F_PROJ)) return;
  const size_t base = (size_t)(row - t.row_off) * t.row_len;
  const float* g = t.g + base;
  const float* p = t.p + base;
  float gp = 0.f, gg = 0.f, pp = 0.f;
  for (int i = threadIdx.x; i < t.row_len; i += 64) {
    const float a = ranger_clean(g[i], clean, lim), b = p[i];
    gp += a * b, gg += a * a, pp += b * b;
  }
  gp = wave_sum(gp), gg = wave_sum(gg), pp = wave_sum(pp);
  if (threadIdx.x == 0) {
    float* o = rowA + (size_t)row * 4;
    o[0] = gp, o[1] = gg, o[2] = pp;
  }
}

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// |F.cosine_similarity(x, y, eps)| from x.y, |x|^2, |y|^2: each norm is clamped at eps before the division
__device__ __forceinline__ float optim_abs_cos(float xy, float xx, float yy, float eps) {
  return fabsf(xy / (fmaxf(sqrtf(xx), eps) * fmaxf(sqrtf(yy), eps)));
}

// one wave per tensor: the projection's view (adamp.py:48-62): 1 = channel, 2 = layer, 0 = none
__global__ __launch_bounds__(64) void k_optim_decide(const OptimTensor* __restrict__ T, const float* __restrict__ rowA,
                                                     float* __restrict__ tens) {
  const OptimTensor t = T[blockIdx.x];
  if (!(t.flags & OPT_F_PROJ)) return;
  const int rows = t.numel / t.row_len;
  const float eps = t.f[4];
  float mx = 0.f, gp = 0.f, gg = 0.f, pp = 0.f;
  for (int r = threadIdx.x; r < rows; r += 64) {
    const float* a = rowA + (size_t)(t.row_off + r) * 4;
    mx = fmaxf(mx, optim_abs_cos(a[0], a[1], a[2], eps));
    gp += a[0], gg += a[1], pp += a[2];
  }
  mx = wave_max_f(mx), gp = wave_sum(gp), gg = wave_sum(gg), pp = wave_sum(pp);
  if (threadIdx.x == 0) {
    int view = 0;
    if (mx < t.f[10]) view = 1;                                       // delta / sqrt(row length)
    else if (optim_abs_cos(gp, gg, pp, eps) < t.f[11]) view = 2;      // delta / sqrt(numel)
    float* o = tens + (size_t)blockIdx.x * 4;
    o[0] = (float)view, o[1] = sqrtf(pp), o[2] = 0.f;
  }
}

// ---- phase 2 -------------------------------------------------------------------------------------------------
// one wave per (tensor, row): the row's sum over the direction - mean of G_grad (RangerAdaBelief), or
// sum(p_n * perturb) with p_n = p / (|p|_view + eps) (projection)
template <int KIND>
__global__ __launch_bounds__(64) void k_optim_dir_rows(const OptimTensor* __restrict__ T, const int* __restrict__ row_tensor,
                                                       const float* __restrict__ rowA, float* __restrict__ rowB,
                                                       const float* __restrict__ tens, int clean, float lim) {
  const int row = blockIdx.x;
  const int ti = row_tensor[row];
  const OptimTensor t = T[ti];
  float nrm = 0.f;
  if (KIND == OPT_RANGER_ADABELIEF) {
    if (!(t.flags & OPT_F_GC_OUT)) return;
  } else {
    if (!(t.flags & OPT_F_PROJ)) return;
    const int view = (int)tens[(size_t)ti * 4];
    if (view == 0) return;
    nrm = (view == 1 ? sqrtf(rowA[(size_t)row * 4 + 2]) : tens[(size_t)ti * 4 + 1]) + t.f[4];
  }
  const int base = (row - t.row_off) * t.row_len;
  float s = 0.f;
  for (int i = threadIdx.x; i < t.row_len; i += 64) {
    OptimElem e = optim_load<KIND>(t, base + i, clean, lim);
    const float d = optim_dir<KIND>(t, e, 0.f);
    s += KIND == OPT_RANGER_ADABELIEF ? d : (e.p / nrm) * d;
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) rowB[row] = KIND == OPT_RANGER_ADABELIEF ? s / (float)t.row_len : s;
}

// one wave per tensor with the layer view: its rows' sums, in row order
__global__ __launch_bounds__(64) void k_optim_tensor_sum(const OptimTensor* __restrict__ T, const float* __restrict__ rowB,
                                                         float* __restrict__ tens) {
  const OptimTensor t = T[blockIdx.x];
  if (!(t.flags & OPT_F_PROJ) || (int)tens[(size_t)blockIdx.x * 4] != 2) return;
  const int rows = t.numel / t.row_len;
  float s = 0.f;
  for (int r = threadIdx.x; r < rows; r += 64) s += rowB[t.row_off + r];
  s = wave_sum(s);
  if (threadIdx.x == 0) tens[(size_t)blockIdx.x * 4 + 2] = s;
}

// ---- phase 3 -------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void k_optim_update(const OptimTensor* __restrict__ T, const int2* __restrict__ chunks,
                                                      const float* __restrict__ rowA, const float* __restrict__ rowB,
                                                      const float* __restrict__ tens, int clean, float lim) {
  const int2 c = chunks[blockIdx.x];
  const OptimTensor t = T[c.x];
  const int fl = t.flags;
  const int end = min(t.numel, c.y + OPT_CHUNK);
  int view = 0;
  float lnorm = 0.f, lsum = 0.f;
  if ((KIND == OPT_ADAMP || KIND == OPT_SGDP) && (fl & OPT_F_PROJ)) {
    view = (int)tens[(size_t)c.x * 4];
    lnorm = tens[(size_t)c.x * 4 + 1], lsum = tens[(size_t)c.x * 4 + 2];
  }
  // four elements per thread and trip, every load of the trip requested before the first store (k_ranger_update)
  for (int i0 = c.y + threadIdx.x; i0 < end; i0 += 1024) {
    OptimElem e[4];
    float ra[4], rb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(i0 + 256 * u, end - 1);
      e[u] = optim_load<KIND>(t, i, clean, lim);
      ra[u] = rb[u] = 0.f;
      if (t.row_len > 0) {
        const int row = t.row_off + i / t.row_len;
        if (KIND == OPT_RANGER_ADABELIEF || KIND == OPT_SGD_GC) {
          if (fl & OPT_F_GC_IN) ra[u] = rowA[(size_t)row * 4];
          if (KIND == OPT_RANGER_ADABELIEF && (fl & OPT_F_GC_OUT)) rb[u] = rowB[row];
        }
        if ((KIND == OPT_ADAMP || KIND == OPT_SGDP) && view == 1) ra[u] = rowA[(size_t)row * 4 + 2], rb[u] = rowB[row];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
      if (i >= end) continue;
      OptimElem& x = e[u];
      float d = optim_dir<KIND>(t, x, ra[u]);
      float pp = x.p;
      if (KIND == OPT_ADABELIEF) {
        pp += -t.f[8] * d;
        t.s[0][i] = x.a, t.s[1][i] = x.b;
        if (fl & OPT_F_AMS) t.s[2][i] = x.c;
      } else if (KIND == OPT_RANGER_ADABELIEF) {
        if (fl & OPT_F_GC_OUT) d -= rb[u];                       // :244-249
        // outside the adaptive branch G_grad IS exp_avg: the decay and the centralization edited it in place (:238-249)
        t.s[0][i] = (fl & OPT_F_ADAPT) ? x.a : d;
        t.s[1][i] = x.b;
        pp += -t.f[7] * d;                                       // :251
        if (fl & OPT_F_LOOK) {                                   // :257-263
          const float sl = x.c + t.f[8] * (pp - x.c);
          t.s[2][i] = sl;
          pp = sl;
        }
      } else if (KIND == OPT_MADGRAD) {
        t.s[0][i] = x.a, t.s[1][i] = x.b;
        pp = (fl & OPT_F_MOM) ? pp * t.f[4] + t.f[3] * d : d;    // :172 / :167
      } else if (KIND == OPT_NADAMW) {
        t.s[0][i] = x.a, t.s[1][i] = x.b;
        if (fl & OPT_F_AMS) t.s[2][i] = x.c;
        pp += t.f[8] * (x.g / d);                                // :131
        pp += t.f[9] * (x.a / d);                                // :132
      } else if (KIND == OPT_ADAMP || KIND == OPT_SGDP) {
        if (view != 0) {                                         // adamp.py:56-58
          const float nrm = (view == 1 ? sqrtf(ra[u]) : lnorm) + t.f[4];
          d -= (pp / nrm) * (view == 1 ? rb[u] : lsum);
        }
        if (KIND == OPT_ADAMP) {
          t.s[0][i] = x.a, t.s[1][i] = x.b;
        } else {
          t.s[0][i] = (fl & OPT_F_NEST) ? x.a : d;               // without nesterov d_p IS the buffer (sgdp.py:92, :59)
        }
        if (fl & OPT_F_PMUL) pp *= view != 0 ? t.f[6] : t.f[5];  // :118 / sgdp.py:108
        pp += -t.f[8] * d;                                       // :121 / sgdp.py:111
      } else {
        if (fl & OPT_F_MOM) t.s[0][i] = x.a;
        pp += -t.f[8] * d;                                       // sgd_gc.py:90
      }
      t.p[i] = pp;
    }
  }
}
