// C ABI of the tracking kernels (kernels and the nn_* sizing helpers: catre_track.h; declarations: include/catre_hip.h)

size_t catre_nn_stats_workspace_bytes(int I, int n_src, int n_dst) {
  return nn_dims_ok(I, n_src, n_dst) ? nn_ws_bytes(I, n_src) : 0;
}

int catre_nn_stats(const float* src, int n_src, const float* dst, int n_dst, const float* src_pose, const float* src_scale,
                   const float* dst_pose, const float* dst_scale, int paired, const float* tau, int I, float* mean_d,
                   float* inlier, float* nn_d, int32_t* nn_j, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(src && dst && mean_d && nn_dims_ok(I, n_src, n_dst) && (tau || !inlier));
  if (paired && n_src != n_dst) return CATRE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < nn_ws_bytes(I, n_src)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = nn_tiles(n_src);
  double* psum = (double*)ws;
  int32_t* pcnt = (int32_t*)(psum + (size_t)I * tiles);
  hipLaunchKernelGGL(k_nn_stats, dim3(I * tiles), dim3(NN_THREADS), 0, st, src, n_src, dst, n_dst, src_pose, src_scale,
                     dst_pose, dst_scale, paired ? 1 : 0, tau, tiles, nn_d, nn_j, psum, pcnt);
  hipLaunchKernelGGL(k_nn_finish, dim3((I + 63) / 64), dim3(64), 0, st, (const double*)psum, (const int32_t*)pcnt, tiles,
                     n_src, I, mean_d, inlier);
  return check_launch();
}

int catre_track_gate(const float* pose_new, const float* scale_new, const float* pose_prev, const float* scale_prev,
                     const int32_t* counts, const float* inlier, const float* mean_d, float min_inlier, int hold, int I,
                     float* pose_out, float* scale_out, int32_t* status, int32_t* age, void* stream) {
  REQUIRE(pose_new && scale_new && pose_prev && scale_prev && counts && inlier && mean_d && pose_out && scale_out &&
          status && age && I > 0);
  hipLaunchKernelGGL(k_track_gate, dim3((I + 63) / 64), dim3(64), 0, (hipStream_t)stream, pose_new, scale_new, pose_prev,
                     scale_prev, counts, inlier, mean_d, min_inlier, hold ? 1 : 0, I, pose_out, scale_out, status, age);
  return check_launch();
}
