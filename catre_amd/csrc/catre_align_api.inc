// C ABI of the NOCS-map alignment (kernels: catre_align.h; declarations: include/catre_hip.h)
namespace {
inline bool align_dims_ok(int I, int Nmax) { return I > 0 && Nmax > 0 && (size_t)Nmax * 3 < ((size_t)1 << 31); }
inline size_t align_ws_bytes(int I, int max_iter) { return (size_t)I * max_iter * ALIGN_HYP_W * sizeof(double); }
}  // namespace

size_t catre_nocs_align_workspace_bytes(int I, int Nmax, int max_iter) {
  if (!align_dims_ok(I, Nmax) || max_iter < 1 || max_iter > ALIGN_MAX_ITER) return 0;
  return align_ws_bytes(I, max_iter);
}

int catre_umeyama(const float* src, const float* dst, const int32_t* counts, const unsigned char* mask, int I, int Nmax,
                  double* scale_out, double* R_out, double* t_out, int32_t* valid_out, void* stream) {
  REQUIRE(src && dst && scale_out && R_out && t_out && align_dims_ok(I, Nmax));
  hipLaunchKernelGGL(k_umeyama, dim3(I), dim3(256), 0, (hipStream_t)stream, src, dst, counts, mask, Nmax, scale_out, R_out,
                     t_out, valid_out);
  return check_launch();
}

int catre_nocs_align(const float* src, const float* dst, const int32_t* counts, const int32_t* draws,
                     unsigned long long seed, const long long* keys, int I, int Nmax, int max_iter, double confidence,
                     double min_inlier_ratio, void* workspace, size_t ws_bytes, double* scale_out, double* R_out,
                     double* t_out, int32_t* valid_out, int32_t* n_inliers_out, int32_t* iters_out, int32_t* best_it_out,
                     unsigned char* mask_out, void* stream) {
  REQUIRE(src && dst && workspace && scale_out && R_out && t_out && valid_out && n_inliers_out && iters_out &&
          best_it_out && align_dims_ok(I, Nmax));
  if (max_iter < 1 || max_iter > ALIGN_MAX_ITER) return CATRE_ERR_UNSUPPORTED;
  if (ws_bytes < align_ws_bytes(I, max_iter)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* hyp = (double*)workspace;
  hipLaunchKernelGGL(k_align_hyp, dim3(I), dim3(ALIGN_MAX_ITER), 0, st, src, dst, counts, draws, seed, keys, Nmax, max_iter,
                     hyp);
  hipLaunchKernelGGL(k_align_ransac, dim3(I), dim3(256), 0, st, src, dst, counts, (const double*)hyp, Nmax, max_iter,
                     confidence, min_inlier_ratio, scale_out, R_out, t_out, valid_out, n_inliers_out, iters_out,
                     best_it_out, mask_out);
  return check_launch();
}

int catre_nocs_align_draws(const int32_t* counts, unsigned long long seed, const long long* keys, int I, int max_iter,
                           int32_t* draws_out, void* stream) {
  REQUIRE(counts && draws_out && I > 0);
  if (max_iter < 1 || max_iter > ALIGN_MAX_ITER) return CATRE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_align_draws, dim3(I), dim3(ALIGN_MAX_ITER), 0, (hipStream_t)stream, counts, seed, keys, max_iter,
                     draws_out);
  return check_launch();
}
