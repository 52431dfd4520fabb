// Micro-experiment (MI355X): which fp32 VALU sequence reproduces the bits of a v_mfma_f32_32x32x2_f32 accumulation?
//   hipcc --offload-arch=gfx950 -O3 -o mfma_chain mfma_chain.hip && ./mfma_chain
// One wave accumulates D = A B over K = 2 * STEPS with one MFMA per K pair (lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]), exactly as GemmPipe::run does.  The host-side question is the order INSIDE an MFMA: the two
// products of an instruction may be added as  fma(a1, b1, fma(a0, b0, c))  (k ascending),  fma(a0, b0, fma(a1, b1, c))
// (k descending), or as an exactly summed pair rounded once.  The three replays run on the VALU of the same device (so
// the denormal mode is the kernels' own) and every one of the 1024 outputs is compared bit by bit.
// Data: a mix of magnitudes (2^-12 .. 2^12, both signs, some zeros) so that an order difference cannot hide.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int STEPS = 256;  // K = 512, the deepest sweep of the encoder

// a[step][lane], b[step][lane]: the operands lane `lane` feeds to MFMA number `step`
__global__ __launch_bounds__(64) void k_mfma(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d) {
  const int lane = threadIdx.x;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int s = 0; s < STEPS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s * 64 + lane], b[s * 64 + lane], acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), j = lane & 31;
    d[i * 32 + j] = acc[r];
  }
}

// one thread per output element; mode 0: k ascending, 1: k descending, 2: pair summed in double, rounded once
__global__ void k_replay(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d, int mode) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 1024) return;
  const int i = e >> 5, j = e & 31;
  float y = 0.f;
  for (int s = 0; s < STEPS; ++s) {
    const float a0 = a[s * 64 + i], a1 = a[s * 64 + 32 + i], b0 = b[s * 64 + j], b1 = b[s * 64 + 32 + j];
    if (mode == 0) {
      y = fmaf(a0, b0, y);
      y = fmaf(a1, b1, y);
    } else if (mode == 1) {
      y = fmaf(a1, b1, y);
      y = fmaf(a0, b0, y);
    } else {
      y = (float)((double)a0 * (double)b0 + (double)a1 * (double)b1 + (double)y);
    }
  }
  d[e] = y;
}

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return 1;                                                                \
    }                                                                          \
  } while (0)

int main() {
  const size_t n = (size_t)STEPS * 64;
  std::vector<float> ha(n), hb(n);
  std::mt19937 rng(1234);
  std::uniform_real_distribution<float> mant(1.f, 2.f);
  std::uniform_int_distribution<int> ex(-12, 12), coin(0, 15);
  auto draw = [&]() {
    const int c = coin(rng);
    if (c == 0) return 0.f;
    const float v = std::ldexp(mant(rng), ex(rng));
    return (c & 1) ? v : -v;
  };
  for (size_t i = 0; i < n; ++i) {
    ha[i] = draw();
    hb[i] = draw();
  }
  float *a, *b, *d;
  CK(hipMalloc(&a, n * 4));
  CK(hipMalloc(&b, n * 4));
  CK(hipMalloc(&d, 4 * 1024 * 4));
  CK(hipMemcpy(a, ha.data(), n * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(b, hb.data(), n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_mfma, dim3(1), dim3(64), 0, 0, a, b, d);
  for (int m = 0; m < 3; ++m) hipLaunchKernelGGL(k_replay, dim3(4), dim3(256), 0, 0, a, b, d + 1024 * (m + 1), m);
  CK(hipDeviceSynchronize());
  std::vector<float> h(4 * 1024);
  CK(hipMemcpy(h.data(), d, 4 * 1024 * 4, hipMemcpyDeviceToHost));
  const char* names[3] = {"k ascending   fma(a1,b1, fma(a0,b0,c))", "k descending  fma(a0,b0, fma(a1,b1,c))", "pair summed exactly, rounded once    "};
  for (int m = 0; m < 3; ++m) {
    int diff = 0;
    for (int e = 0; e < 1024; ++e) diff += std::memcmp(&h[e], &h[1024 * (m + 1) + e], 4) != 0;
    printf("mfma_chain: %s : %d of 1024 outputs differ from the MFMA\n", names[m], diff);
  }
  return 0;
}
