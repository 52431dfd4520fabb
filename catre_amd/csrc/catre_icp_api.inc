// C ABI of trimmed ICP (kernel: catre_icp.h, neighbours: catre_track.h; declarations: include/catre_hip.h)
namespace {
constexpr int ICP_MAX_ITER = CATRE_ICP_MAX_ITER;
inline bool icp_trim_ok(float trim) { return trim > 0.f && trim <= 1.f; }  // false for NaN
// the neighbour partials of catre_nn_stats, then mean_d [I] fp32 (required by it, not returned), nn_d2 and nn_j [I * n_src]
struct IcpWs {
  size_t mean, d2, j, total;
};
inline IcpWs icp_ws(int I, int n_src) {
  IcpWs w;
  w.mean = nn_ws_bytes(I, n_src);
  w.d2 = w.mean + align_up((size_t)I * 4, 16);
  w.j = w.d2 + align_up((size_t)I * n_src * 4, 16);
  w.total = w.j + align_up((size_t)I * n_src * 4, 16);
  return w;
}
inline void icp_launch_step(hipStream_t st, const float* pcl, int n_src, const int32_t* counts, const float* kps, int n_dst,
                            const float* pose, const float* scale, const float* nn_d2, const int32_t* nn_j, const float* tau,
                            float trim, int with_scale, int update, int I, float* pose_out, float* scale_out, float* rmse,
                            int32_t* kept, unsigned char* mask, int32_t* status) {
  hipLaunchKernelGGL(k_icp_step, dim3(I), dim3(256), 0, st, pcl, n_src, counts, kps, n_dst, pose, scale, nn_d2, nn_j, tau,
                     trim, with_scale ? 1 : 0, update ? 1 : 0, pose_out, scale_out, rmse, kept, mask, status);
}
}  // namespace

size_t catre_icp_workspace_bytes(int I, int n_src, int n_dst, int n_iter) {
  if (!nn_dims_ok(I, n_src, n_dst) || n_iter < 0 || n_iter > ICP_MAX_ITER) return 0;
  return icp_ws(I, n_src).total;
}

int catre_icp_step(const float* pcl, int n_src, const int32_t* counts, const float* kps, int n_dst, const float* pose,
                   const float* scale, const float* nn_d2, const int32_t* nn_j, const float* tau, float trim, int with_scale,
                   int update, int I, float* pose_out, float* scale_out, float* rmse, int32_t* kept, unsigned char* mask,
                   int32_t* status, void* stream) {
  REQUIRE(pcl && kps && pose && scale && nn_d2 && nn_j && rmse && kept && nn_dims_ok(I, n_src, n_dst) && icp_trim_ok(trim));
  REQUIRE(!update || (pose_out && scale_out && status));
  icp_launch_step((hipStream_t)stream, pcl, n_src, counts, kps, n_dst, pose, scale, nn_d2, nn_j, tau, trim, with_scale,
                  update, I, pose_out, scale_out, rmse, kept, mask, status);
  return check_launch();
}

int catre_icp(const float* pcl, int n_src, const int32_t* counts, const float* kps, int n_dst, const float* pose,
              const float* scale, const float* tau, float trim, int with_scale, int n_iter, int I, float* pose_out,
              float* scale_out, float* rmse, int32_t* kept, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(pcl && kps && pose && scale && pose_out && scale_out && rmse && kept && status && nn_dims_ok(I, n_src, n_dst) &&
          icp_trim_ok(trim) && n_iter >= 0 && n_iter <= ICP_MAX_ITER);
  const IcpWs w = icp_ws(I, n_src);
  if (!ws || ws_bytes < w.total) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = nn_tiles(n_src);
  double* psum = (double*)ws;
  int32_t* pcnt = (int32_t*)(psum + (size_t)I * tiles);
  float* mean_d = (float*)((char*)ws + w.mean);
  float* nn_d2 = (float*)((char*)ws + w.d2);
  int32_t* nn_j = (int32_t*)((char*)ws + w.j);
  for (int it = 0; it <= n_iter; ++it) {
    // iteration 0 reads the caller's pose; every later one the pose the step before it wrote (the step updates in place)
    const float* p = it ? pose_out : pose;
    const float* s = it ? scale_out : scale;
    hipLaunchKernelGGL(k_nn_stats, dim3(I * tiles), dim3(NN_THREADS), 0, st, pcl, n_src, kps, n_dst, (const float*)nullptr,
                       (const float*)nullptr, p, s, 0, (const float*)nullptr, tiles, nn_d2, nn_j, psum, pcnt);
    hipLaunchKernelGGL(k_nn_finish, dim3((I + 63) / 64), dim3(64), 0, st, (const double*)psum, (const int32_t*)pcnt, tiles,
                       n_src, I, mean_d, (float*)nullptr);
    icp_launch_step(st, pcl, n_src, counts, kps, n_dst, p, s, nn_d2, nn_j, tau, trim, with_scale, it < n_iter, I, pose_out,
                    scale_out, rmse + (size_t)it * I, kept + (size_t)it * I, nullptr, status);
  }
  if (n_iter == 0) {  // nothing was updated: the pose goes out as it came
    if (hipMemcpyAsync(pose_out, pose, (size_t)I * 12 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(scale_out, scale, (size_t)I * 3 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return CATRE_ERR_LAUNCH;
  }
  return check_launch();
}
