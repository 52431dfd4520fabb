// catre_pcl_api.inc - C ABI of the point-cloud preparation of catre_pcl.h (included inside extern "C" of catre_extras.hip)
// ---- row f3: point-cloud preparation -----------------------------------------------------------------------
namespace {
struct PclWs {
  size_t bins, choose, offsets, total, cand, total_ints;
  int nchunks;
};
// frames the kernels index in int: H * W < 2^30, the product taken in size_t (65536 x 65536 wraps to 0 in int)
PclWs pcl_ws(int I, int H, int W) {
  PclWs L;
  const size_t HW = (size_t)H * (size_t)W;
  L.nchunks = (int)((HW + PCL_CHUNK - 1) / PCL_CHUNK);
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += align_up(n, 64);
    return r;
  };
  L.bins = take((size_t)I * L.nchunks * 12);
  L.choose = take(I);
  L.offsets = take((size_t)I * L.nchunks);
  L.total = take(I);
  L.cand = take((size_t)I * HW);
  L.total_ints = o;
  return L;
}
inline PclCam pcl_cam(const float* K9) { return PclCam{K9[0], K9[4], K9[2], K9[5]}; }
}  // namespace

// one launch helper per stage for either frame source of catre_pcl.h (templates: C++ linkage inside the ABI block).
// `ws` is the base the layout L counts from.
extern "C++" {
namespace {
template <int MODE, typename LT, class SRC>
int pcl_run_candidates(const SRC& src, const float* depth, const unsigned char* masks, const void* labels,
                       const int* label_of, const float* poses, const float* scales, float ratio, int use_ball, int I,
                       int H, int W, const PclWs& L, int* ws, int32_t* counts_out, hipStream_t st) {
  const dim3 grid(L.nchunks, I), block(256);
  hipLaunchKernelGGL((k_pcl_count<SRC, MODE, LT>), grid, block, 0, st, src, depth, masks, (const LT*)labels, label_of,
                     poses, scales, ratio, use_ball, H, W, L.nchunks, ws + L.bins);
  hipLaunchKernelGGL(k_pcl_pick, dim3(I), dim3(256), 0, st, ws + L.bins, L.nchunks, 1, ws + L.choose, ws + L.offsets,
                     ws + L.total);
  hipLaunchKernelGGL((k_pcl_compact<SRC, MODE, LT>), grid, block, 0, st, src, depth, masks, (const LT*)labels, label_of,
                     poses, scales, ratio, use_ball, H, W, L.nchunks, ws + L.choose, ws + L.offsets, ws + L.cand);
  if (counts_out &&
      hipMemcpyAsync(counts_out, ws + L.total, (size_t)I * sizeof(int), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return CATRE_ERR_LAUNCH;
  return check_launch();
}
template <class SRC>
int pcl_run_gather(const SRC& src, const float* depth, int I, int H, int W, const PclWs& L, const int* ws,
                   const long long* sample_idx, int N, float* pcl_out, int32_t* pix_out, hipStream_t st) {
  hipLaunchKernelGGL(k_pcl_gather<SRC>, dim3((N + 255) / 256, I), dim3(256), 0, st, src, depth, H, W, ws + L.cand,
                     ws + L.total, sample_idx, N, pcl_out, pix_out);
  return check_launch();
}
template <class SRC>
int pcl_run_fps(const SRC& src, const float* depth, int I, int H, int W, const PclWs& L, const int* ws, int N,
                float* scratch, int slot_cap, long long* sample_idx_out, hipStream_t st) {
  hipLaunchKernelGGL(k_pcl_fps<SRC>, dim3(I), dim3(1024), 0, st, src, depth, H, W, ws + L.cand, ws + L.total, N, scratch,
                     slot_cap, sample_idx_out);
  return check_launch();
}
}  // namespace
}  // extern "C++"

size_t catre_pcl_workspace_bytes(int I, int H, int W) {
  if (I <= 0 || !pcl_frame_ok(H, W)) return 0;  // the limit catre_pcl_candidates enforces: no size for a frame it refuses
  return pcl_ws(I, H, W).total_ints * sizeof(int);
}

int catre_pcl_candidates(const float* depth, const float* K9, const unsigned char* masks, const float* poses,
                         const float* scales, float ratio, int use_ball, int I, int H, int W, void* workspace,
                         size_t ws_bytes, int32_t* counts_out, void* stream) {
  REQUIRE(depth && K9 && poses && scales && workspace && I > 0 && pcl_frame_ok(H, W));
  const PclWs L = pcl_ws(I, H, W);
  if (ws_bytes < L.total_ints * sizeof(int)) return CATRE_ERR_WORKSPACE;
  return pcl_run_candidates<0, unsigned char>(PclOneFrame{pcl_cam(K9), 0}, depth, masks, nullptr, nullptr, poses, scales,
                                              ratio, use_ball, I, H, W, L, (int*)workspace, counts_out,
                                              (hipStream_t)stream);
}

int catre_pcl_sample(const float* depth, const float* K9, const void* workspace, size_t ws_bytes,
                     const long long* sample_idx, unsigned long long seed, int I, int H, int W, int N, float* pcl_out,
                     int32_t* pix_out, void* stream) {
  REQUIRE(depth && K9 && workspace && pcl_out && I > 0 && pcl_frame_ok(H, W) && N > 0);
  const PclWs L = pcl_ws(I, H, W);
  if (ws_bytes < L.total_ints * sizeof(int)) return CATRE_ERR_WORKSPACE;
  return pcl_run_gather(PclOneFrame{pcl_cam(K9), seed}, depth, I, H, W, L, (const int*)workspace, sample_idx, N, pcl_out,
                        pix_out, (hipStream_t)stream);
}

// INPUT.FPS_SAMPLE: sample_idx_out [I][N] = farthest-point order of each instance's tiled candidate list (feed it to
// catre_pcl_sample).  scratch: I * 4 * slot_cap floats, slot_cap >= the largest tiled list (count doubled until >= N).
int catre_pcl_fps(const float* depth, const float* K9, const void* workspace, size_t ws_bytes, int I, int H, int W, int N,
                  float* scratch, int slot_cap, long long* sample_idx_out, void* stream) {
  REQUIRE(depth && K9 && workspace && scratch && sample_idx_out && I > 0 && pcl_frame_ok(H, W) && N > 0 && slot_cap > 0);
  const PclWs L = pcl_ws(I, H, W);
  if (ws_bytes < L.total_ints * sizeof(int)) return CATRE_ERR_WORKSPACE;
  return pcl_run_fps(PclOneFrame{pcl_cam(K9), 0}, depth, I, H, W, L, (const int*)workspace, N, scratch, slot_cap,
                     sample_idx_out, (hipStream_t)stream);
}
