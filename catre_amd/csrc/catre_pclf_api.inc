// C ABI of the frame-batched point-cloud preparation and the depth augmentation (kernels: catre_pcl.h on its
// PclFrameTable source, catre_pclf.h for the augmentation; workspace layout and launch helpers: catre_pcl_api.inc;
// declarations: include/catre_hip.h)
namespace {
// head of the workspace: the per-instance and per-frame tables the entry points stage, then the single-frame layout
struct PclfWs {
  size_t frame_of, rank_of, label_of, cams, seeds, head_ints;  // offsets in ints
  PclWs body;                                                   // offsets relative to head_ints
  size_t total_ints;
};
inline bool pclf_dims_ok(int F, int I, int H, int W) { return F > 0 && I > 0 && pcl_frame_ok(H, W); }
inline bool pclf_grid_ok(int I) { return I <= 65535; }  // instances are the y dimension of the launch grids
PclfWs pclf_ws(int F, int I, int H, int W) {
  PclfWs L;
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += align_up(n, 64);
    return r;
  };
  L.frame_of = take(I);
  L.rank_of = take(I);
  L.label_of = take(I);
  L.cams = take((size_t)F * 4);
  L.seeds = take((size_t)F * 2);
  L.head_ints = o;
  L.body = pcl_ws(I, H, W);
  L.total_ints = o + L.body.total_ints;
  return L;
}
// the checks every frame-batch entry point makes on its HOST arrays before anything is launched
inline bool pclf_tables_ok(const float* K, const int32_t* frame_of, int F, int I) {
  for (int i = 0; i < I; ++i)
    if (frame_of[i] < 0 || frame_of[i] >= F) return false;
  for (int f = 0; f < F; ++f) {
    const float fx = K[f * 9], fy = K[f * 9 + 4];
    if (fx == 0.f || fy == 0.f || fx != fx || fy != fy) return false;  // zero or NaN
  }
  return true;
}
// one host->device copy of the whole head.  rank_of == nullptr: the rank of an instance within its frame, in the order given
int pclf_stage(const PclfWs& L, int* ws, const float* K, const int32_t* frame_of, const int32_t* rank_of,
               const int32_t* label_of, const unsigned long long* seeds, int F, int I, hipStream_t st) {
  std::vector<int> head(L.head_ints, 0);
  std::vector<int> seen(rank_of ? 0 : F, 0);
  for (int i = 0; i < I; ++i) {
    head[L.frame_of + i] = frame_of[i];
    head[L.rank_of + i] = rank_of ? rank_of[i] : seen[frame_of[i]]++;
    if (label_of) head[L.label_of + i] = label_of[i];
  }
  for (int f = 0; f < F; ++f) {
    const PclCam cam = pcl_cam(K + f * 9);
    memcpy(&head[L.cams + (size_t)f * 4], &cam, sizeof cam);
    if (seeds) memcpy(&head[L.seeds + (size_t)f * 2], &seeds[f], sizeof seeds[f]);
  }
  // pageable source: the runtime has consumed it when the call returns
  if (hipMemcpyAsync(ws, head.data(), L.head_ints * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
    return CATRE_ERR_LAUNCH;
  return CATRE_OK;
}
// the staged head as the kernels' frame source
inline PclFrameTable pclf_table(const PclfWs& L, const int* ws, int F) {
  return PclFrameTable{ws + L.frame_of, ws + L.rank_of, (const PclCam*)(ws + L.cams),
                       (const unsigned long long*)(ws + L.seeds), F};
}
}  // namespace

size_t catre_pclf_workspace_bytes(int F, int I, int H, int W) {
  if (!pclf_dims_ok(F, I, H, W)) return 0;
  return pclf_ws(F, I, H, W).total_ints * sizeof(int);
}

int catre_pclf_candidates(const float* depth, const float* K, const int32_t* frame_of, const unsigned char* masks,
                          const void* labels, int label_bytes, const int32_t* label_of, const float* poses,
                          const float* scales, float ratio, int use_ball, int F, int I, int H, int W, void* workspace,
                          size_t ws_bytes, int32_t* counts_out, void* stream) {
  REQUIRE(depth && K && frame_of && poses && scales && workspace && pclf_dims_ok(F, I, H, W) && pclf_grid_ok(I));
  REQUIRE(!(masks && labels) && (labels ? (label_of && (label_bytes == 1 || label_bytes == 4)) : true));
  REQUIRE(pclf_tables_ok(K, frame_of, F, I));
  const PclfWs L = pclf_ws(F, I, H, W);
  if (ws_bytes < L.total_ints * sizeof(int)) return CATRE_ERR_WORKSPACE;
  int* ws = (int*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (int e = pclf_stage(L, ws, K, frame_of, nullptr, labels ? label_of : nullptr, nullptr, F, I, st)) return e;
  const PclFrameTable src = pclf_table(L, ws, F);
  const int* lo = ws + L.label_of;
  int* body = ws + L.head_ints;
#define PCLF_CAND(MODE, LT)                                                                                          \
  pcl_run_candidates<MODE, LT>(src, depth, masks, labels, lo, poses, scales, ratio, use_ball, I, H, W, L.body, body, \
                               counts_out, st)
  if (!labels) return PCLF_CAND(0, unsigned char);
  if (label_bytes == 1) return PCLF_CAND(1, unsigned char);
  return PCLF_CAND(1, int);
#undef PCLF_CAND
}

int catre_pclf_sample(const float* depth, const float* K, const int32_t* frame_of, const int32_t* rank_of,
                      void* workspace, size_t ws_bytes, const long long* sample_idx, const unsigned long long* seeds,
                      int F, int I, int H, int W, int N, float* pcl_out, int32_t* pix_out, void* stream) {
  REQUIRE(depth && K && frame_of && workspace && pcl_out && pclf_dims_ok(F, I, H, W) && pclf_grid_ok(I) && N > 0);
  REQUIRE(sample_idx || seeds);
  REQUIRE(pclf_tables_ok(K, frame_of, F, I));
  const PclfWs L = pclf_ws(F, I, H, W);
  if (ws_bytes < L.total_ints * sizeof(int)) return CATRE_ERR_WORKSPACE;
  int* ws = (int*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (int e = pclf_stage(L, ws, K, frame_of, rank_of, nullptr, seeds, F, I, st)) return e;
  return pcl_run_gather(pclf_table(L, ws, F), depth, I, H, W, L.body, ws + L.head_ints, sample_idx, N, pcl_out, pix_out,
                        st);
}

int catre_pclf_fps(const float* depth, const float* K, const int32_t* frame_of, void* workspace, size_t ws_bytes, int F,
                   int I, int H, int W, int N, float* scratch, int slot_cap, long long* sample_idx_out, void* stream) {
  REQUIRE(depth && K && frame_of && workspace && scratch && sample_idx_out && pclf_dims_ok(F, I, H, W) &&
          pclf_grid_ok(I) && N > 0 && slot_cap > 0);
  REQUIRE(pclf_tables_ok(K, frame_of, F, I));
  const PclfWs L = pclf_ws(F, I, H, W);
  if (ws_bytes < L.total_ints * sizeof(int)) return CATRE_ERR_WORKSPACE;
  int* ws = (int*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (int e = pclf_stage(L, ws, K, frame_of, nullptr, nullptr, nullptr, F, I, st)) return e;
  return pcl_run_fps(pclf_table(L, ws, F), depth, I, H, W, L.body, ws + L.head_ints, N, scratch, slot_cap,
                     sample_idx_out, st);
}

int catre_depth_augment(const void* depth_in, int in_is_u16, float depth_div, const catre_depth_aug_frame* frames,
                        int use_draws, const double* draw_fill, const double* draw_keep, const double* draw_gauss,
                        unsigned long long seed, float* depth_out, int F, int H, int W, void* stream) {
  static_assert(sizeof(catre_depth_aug_frame) == sizeof(DaugFrame) && sizeof(DaugFrame) == 32, "frame table layout");
  static_assert(CATRE_DAUG_FILL == DAUG_FILL && CATRE_DAUG_DROP == DAUG_DROP && CATRE_DAUG_NOISE == DAUG_NOISE, "flags");
  REQUIRE(depth_in && frames && depth_out && F > 0 && F <= 65535 && pcl_frame_ok(H, W));
  REQUIRE(!in_is_u16 || (depth_div != 0.f && depth_div == depth_div));
  const int HW = H * W;
  const dim3 grid((HW + 255) / 256, F), block(256);
  hipStream_t st = (hipStream_t)stream;
  const DaugFrame* fr = (const DaugFrame*)frames;
#define DAUG_LAUNCH(IT, DRAWS)                                                                                     \
  hipLaunchKernelGGL((k_depth_augment<IT, DRAWS>), grid, block, 0, st, (const IT*)depth_in, depth_div, fr, draw_fill, \
                     draw_keep, draw_gauss, seed, HW, depth_out)
  if (in_is_u16) {
    if (use_draws)
      DAUG_LAUNCH(unsigned short, true);
    else
      DAUG_LAUNCH(unsigned short, false);
  } else {
    if (use_draws)
      DAUG_LAUNCH(float, true);
    else
      DAUG_LAUNCH(float, false);
  }
#undef DAUG_LAUNCH
  return check_launch();
}
