// catre_train.hip - the training unit of libcatre_hip.so: the row / wgrad GEMMs and the layer-wise backward kernels
// (catre_train.h), the configurable heads (catre_heads.h), the fused optimizer steps (catre_optim.h) and their C ABI
// (catre_op_*, catre_heads_*).  The training entry points that launch encoder kernels live with those, in catre_kernels.hip.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "catre_train.h"
#include "catre_optim.h"
#include "catre_heads.h"

#include "catre_host.h"
using namespace catre_host;

extern "C" {
#include "catre_train_api.inc"
#include "catre_heads_api.inc"
}  // extern "C"

int catre_host::launch_maxpool_tiles(const float* pmax, const int* pidx, float* out, int* idx, int J, int B, int N, int M,
                                     hipStream_t st) {
  hipLaunchKernelGGL(k_maxpool_tiles, dim3(M > 0 ? 2 * B : B, (J + 255) / 256), dim3(256), 0, st, pmax, pidx, out, idx, J, B, N,
                     M);
  return check_launch();
}
