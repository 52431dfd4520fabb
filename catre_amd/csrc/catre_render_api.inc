// C ABI of the splat render (kernels: catre_render.h; shared host side: catre_zbuf_api.inc; declarations: include/catre_hip.h)
namespace {
constexpr int SPLAT_MAX_I = 65535, SPLAT_MAX_M = 65536;  // 16 bits each in the key; instance 0xffff + point 0xffff never meet all ones (z > 0)
// [F*H*W] 64-bit keys, then the staged tables with frame_of sized for any I, so that the workspace depends on the frames alone
struct SplatWs {
  size_t keys_bytes, total_bytes;
};
inline SplatWs splat_ws(int F, int H, int W) {
  SplatWs L;
  L.keys_bytes = (size_t)F * H * W * 8;
  L.total_bytes = align_up(L.keys_bytes + zbuf_tab_ints(F, SPLAT_MAX_I) * sizeof(int), 256);
  return L;
}
}  // namespace

size_t catre_splat_workspace_bytes(int F, int H, int W) {
  return splat_frames_ok(F, H, W) ? splat_ws(F, H, W).total_bytes : 0;
}

int catre_splat_render(const float* kps, const float* pose, const float* scale, const float* rho, const float* depth,
                       const float* K, const int32_t* frame_of, float r_max, float delta, int F, int I, int M, int H, int W,
                       void* workspace, size_t ws_bytes, int32_t* labels, float* zbuf, int32_t* point, unsigned char* cls,
                       int32_t* labels_fit, int32_t* counts, unsigned char* vis, void* stream) {
  static_assert(CATRE_SPLAT_BACKGROUND == 0 && CATRE_SPLAT_HOLE == 4, "counts [I,5]: column 0 = pixels won, column c = class c");
  REQUIRE(kps && pose && scale && rho && K && frame_of && labels && zbuf && counts);
  REQUIRE(I > 0 && M > 0 && splat_frames_ok(F, H, W) && r_max >= 0.f && delta == delta);
  if (I > SPLAT_MAX_I || M > SPLAT_MAX_M) return CATRE_ERR_UNSUPPORTED;
  REQUIRE(pclf_tables_ok(K, frame_of, F, I));
  const SplatWs L = splat_ws(F, H, W);
  if (!workspace || ws_bytes < L.total_bytes) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  ZbufTables tab;
  if (const int err = zbuf_stage((int*)((char*)workspace + L.keys_bytes), K, frame_of, F, I, st, tab)) return err;
  const int n = F * H * W, tiles = (M + 255) / 256;  // I * tiles <= 65535 * 256
  const int ppw = zbuf_items_per_wave((size_t)I * M), stiles = (M + 4 * ppw - 1) / (4 * ppw);  // I * stiles <= 65535 * 4096
  hipLaunchKernelGGL(k_zbuf_clear, dim3((std::max(n, I * 5) + 255) / 256), dim3(256), 0, st, keys, n, counts, I * 5,
                     (int32_t*)nullptr, 0);
  hipLaunchKernelGGL(k_splat, dim3(I * stiles), dim3(SPLAT_THREADS), 0, st, kps, pose, scale, rho, tab.frame_of, tab.cams, M,
                     stiles, ppw, H, W, r_max, keys);
  hipLaunchKernelGGL(k_splat_resolve, dim3((n + 255) / 256), dim3(256), 0, st, (const unsigned long long*)keys, depth, delta,
                     n, labels, zbuf, point, cls, labels_fit, counts);
  if (vis)
    hipLaunchKernelGGL(k_splat_visible, dim3(I * tiles), dim3(256), 0, st, kps, pose, scale, rho, tab.frame_of, tab.cams, depth,
                       (const int32_t*)labels, (const float*)zbuf, M, tiles, H, W, r_max, delta, vis);
  return check_launch();
}
