// catre_host.h - the host helpers every C-ABI file of the library uses (the three translation units and their *_api.inc).
// The part in front of the __HIP__ guard is plain C++: catre_forms.h, which is also built without HIP, takes align_up there.
#pragma once
#include <cstddef>

#include "../../include/catre_hip.h"

namespace catre_host {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline bool dims_ok(int B, int N, int M) { return B > 0 && N > 0 && M > 0; }
// the PointNet stages also run on a single cloud per object (M == 0: PointNetfeat.forward on its own)
inline bool dims_ok1(int B, int N, int M) { return B > 0 && N > 0 && M >= 0; }

}  // namespace catre_host

#define REQUIRE(cond) \
  do {                \
    if (!(cond)) return CATRE_ERR_BAD_ARG; \
  } while (0)

#ifdef __HIP__
#include <hip/hip_runtime.h>

#include <mutex>

#define CATRE_INTERNAL __attribute__((visibility("hidden")))  // shared by the units, not part of the C ABI

namespace catre_host {

inline int check_launch() { return hipGetLastError() == hipSuccess ? CATRE_OK : CATRE_ERR_LAUNCH; }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: one "done" bit per (kernel slot, device),
// taken under a mutex (a process that drives several GPUs, host threads launching concurrently).  An inline function of a
// named namespace: the slots have one definition in the library however many units include this header.
enum { DYN_L0_SP, DYN_L0_BF, DYN_L0_BFH, DYN_L1_SP, DYN_L1_BF, DYN_L1_BFH, DYN_L1, DYN_SLOTS };
CATRE_INTERNAL inline int ensure_dyn_lds(const void* fn, size_t bytes, int slot) {
  static std::mutex mu;
  static unsigned long long done[DYN_SLOTS] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return CATRE_ERR_LAUNCH;
  std::lock_guard<std::mutex> lk(mu);
  if (dev >= 0 && dev < 64 && ((done[slot] >> dev) & 1ull)) return CATRE_OK;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return CATRE_ERR_LAUNCH;
  if (dev >= 0 && dev < 64) done[slot] |= 1ull << dev;
  return CATRE_OK;
}

// catre_debug_trunk_trace's buffer (the kernels of two units stamp into it): defined in catre_kernels.hip
extern CATRE_INTERNAL unsigned long long* g_trunk_trace;

// Entry points of one unit that also need a kernel of another reach it through these plain host functions, each defined
// beside its kernel.
// k_maxpool_tiles (catre_train.h) behind the SAVE forms of the encoder kernels: defined in catre_train.hip
CATRE_INTERNAL int launch_maxpool_tiles(const float* pmax, const int* pidx, float* out, int* idx, int J, int B, int N, int M,
                                        hipStream_t st);

}  // namespace catre_host
#endif  // __HIP__
