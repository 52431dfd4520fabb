// C ABI of the BOP pose errors (kernels: catre_bop.h; declarations: include/catre_hip.h)
namespace {
inline int bop_sym_tiles(int S_max) { return (S_max + BOP_SYM_TILE - 1) / BOP_SYM_TILE; }
// the table is indexed by size_t; the grids - one workgroup per (instance, tile of symmetries), one wave per (error,
// instance) - stay below 2^31
inline bool bop_sym_dims_ok(int I, int S_max) {
  return I > 0 && S_max > 0 && (size_t)I * bop_sym_tiles(S_max) < ((size_t)1 << 31) && (size_t)I * 3 < ((size_t)1 << 31) &&
         (size_t)I * S_max < ((size_t)1 << 40);
}
// [3][I][S_max] fp32: e3, e2, p2 per (instance, symmetry)
inline size_t bop_sym_ws_bytes(int I, int S_max) { return align_up((size_t)3 * I * S_max * sizeof(float), 256); }
}  // namespace

size_t catre_sym_err_workspace_bytes(int I, int S_max) { return bop_sym_dims_ok(I, S_max) ? bop_sym_ws_bytes(I, S_max) : 0; }

int catre_sym_err(const float* pts, int pts_shared, int n, const float* pose_est, const float* pose_gt, const float* scale_est,
                  const float* scale_gt, const float* K, const float* syms, const int32_t* sym_off, const int32_t* sym_of,
                  int G, int S_tot, int S_max, int I, void* workspace, size_t ws_bytes, float* err, int32_t* best,
                  float* tables, void* stream) {
  REQUIRE(pts && pose_est && pose_gt && K && syms && sym_off && sym_of && err && best);
  REQUIRE(n > 0 && (size_t)n * 3 < ((size_t)1 << 31) && G > 0 && S_tot > 0 && S_max <= S_tot && bop_sym_dims_ok(I, S_max));
  if (!tables && (!workspace || ws_bytes < bop_sym_ws_bytes(I, S_max))) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* tab = tables ? tables : (float*)workspace;
  const int stiles = bop_sym_tiles(S_max);
  hipLaunchKernelGGL(k_sym_err, dim3(I * stiles), dim3(BOP_THREADS), 0, st, pts, pts_shared ? 1 : 0, n, pose_est, pose_gt,
                     scale_est, scale_gt, K, syms, sym_off, sym_of, G, S_tot, S_max, stiles, I, tab);
  hipLaunchKernelGGL(k_sym_min, dim3(3 * I), dim3(64), 0, st, (const float*)tab, sym_off, sym_of, G, S_tot, S_max, I,
                     err, best);
  return check_launch();
}

int catre_vsd(const float* depth_est, const float* depth_gt, const float* depth_test, const float* K, const int32_t* frame_of,
              const int32_t* origin, const double* diameter, const double* taus, float delta, int visib_mode, int I, int h,
              int w, int F, int H, int W, int T, int32_t* counts, double* errors, void* stream) {
  REQUIRE(depth_est && depth_gt && depth_test && K && taus && counts && errors);
  REQUIRE(I > 0 && h > 0 && w > 0 && F > 0 && H > 0 && W > 0 && T > 0 && delta == delta);
  REQUIRE(visib_mode == CATRE_VSD_BOP19 || visib_mode == CATRE_VSD_BOP18);
  REQUIRE((size_t)h * w < ((size_t)1 << 30) && (size_t)H * W < ((size_t)1 << 30) && I < (1 << 30));
  if (T > BOP_MAX_TAUS) return CATRE_ERR_UNSUPPORTED;
  const int tiles = (h * w + BOP_THREADS * BOP_VSD_PASSES - 1) / (BOP_THREADS * BOP_VSD_PASSES);
  REQUIRE((size_t)I * tiles < ((size_t)1 << 31) && (size_t)I * T < ((size_t)1 << 30));
  BopTaus tt;
  for (int t = 0; t < BOP_MAX_TAUS; ++t) {
    tt.v[t] = t < T ? taus[t] : 0.0;
    REQUIRE(tt.v[t] == tt.v[t]);
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)I * (2 + T) * sizeof(int32_t), st) != hipSuccess) return CATRE_ERR_LAUNCH;
  hipLaunchKernelGGL(k_vsd, dim3(I * tiles), dim3(BOP_THREADS), 0, st, depth_est, depth_gt, depth_test, K, frame_of, origin,
                     diameter, tt, delta, visib_mode == CATRE_VSD_BOP18 ? 1 : 0, tiles, h, w, F, H, W, T, counts);
  hipLaunchKernelGGL(k_vsd_finish, dim3((I * T + 255) / 256), dim3(256), 0, st, (const int32_t*)counts, I, T, errors);
  return check_launch();
}
