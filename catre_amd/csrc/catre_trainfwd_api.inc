// catre_trainfwd_api.inc - the training entry points that launch kernels of the core unit: the SAVE forms of the three encoder
// kernels and the fused rotation-head forward (included inside extern "C" of catre_kernels.hip).  The backward ops and the
// row GEMMs of training are in catre_train_api.inc (catre_train.hip).

// Training forward of BOTH rotation heads up to the GroupNorm-1 input (heads/conv_out_per_rot_head.py:126-134) on the fused
// inference kernels: GroupNorm-0 statistics from second moments of pointfeat (k_pf_moments + k_gn0_from_moments), then the
// SAVE instance of k_rot_l1 - layer 0 recomputed per tile, GN0 + GELU in registers, layer 1 from the LDS image - which
// stores y0 (GN0 input), a0 (layer 1's input) and y1 (GN1 input) head-major, [2][B*(N+M)][256] each, plus the GN1 tile
// partials [2][B*(N+M)/64][32][2] and stat0 [2][B][32][2] = (mean, rstd) of GN0.  compute_dtype: CATRE_DTYPE_F32 (packed holds
// CATRE_PACK_F32_HEADS) or CATRE_DTYPE_SPLIT (k_rot_l1_split<true>, CATRE_PACK_SPLIT).  Replaces, per head, a row GEMM, a
// GroupNorm+GELU pass over y0 and a second row GEMM that re-read those matrices from HBM.
// pointfeat: cloud-major [B*N + B*M][64]; bias0 [2][2B][256]: the global-feature half of layer 0 + its bias per cloud.
size_t catre_train_rot_fwd_ws_bytes(int B) {
  return ((size_t)2 * B * PF_NG * 4096 + (size_t)2 * B * PF_NG * 64 + (size_t)2 * B * 64 + (size_t)B * 2 * 2 * 2 * 256) *
         sizeof(float);
}

int catre_train_rot_fwd(const float* pointfeat, const float* bias0, const float* const* prm, const float* packed, float* y0,
                        float* a0, float* y1, float* gn1_part, float* stat0, void* workspace, size_t ws_bytes, int B, int N,
                        int M, int compute_dtype, void* stream) {
  REQUIRE(pointfeat && bias0 && prm && packed && y0 && a0 && y1 && gn1_part && stat0 && workspace && B > 0 && N > 0 &&
          M > 0 && (N % TP) == 0 && (M % TP) == 0);
  if (compute_dtype != CATRE_DTYPE_F32 && compute_dtype != CATRE_DTYPE_SPLIT) return CATRE_ERR_UNSUPPORTED;
  if (ws_bytes < catre_train_rot_fwd_ws_bytes(B)) return CATRE_ERR_WORKSPACE;
  const PackLayout L = pack_layout(1);
  hipStream_t st = (hipStream_t)stream;
  const int T = (N + M) / TP;
  float* Gc = (float*)workspace;
  float* s1c = Gc + (size_t)2 * B * PF_NG * 4096;
  float* shc = s1c + (size_t)2 * B * PF_NG * 64;
  float* aff0 = shc + (size_t)2 * B * 64;
  hipLaunchKernelGGL(k_pf_moments, dim3(2 * B, pf_groups(B)), dim3(256), 0, st, pointfeat, Gc, s1c, shc,
                     B, N, M);
  hipLaunchKernelGGL(k_gn0_from_moments, dim3(B, gn0_shares(B)), dim3(256), 0, st, Gc, s1c, shc, prm[CATRE_P_ROTX_L0_W],
                     prm[CATRE_P_ROTY_L0_W], PMW, 1024, bias0, prm[CATRE_P_ROTX_GN0_W], prm[CATRE_P_ROTX_GN0_B],
                     prm[CATRE_P_ROTY_GN0_W], prm[CATRE_P_ROTY_GN0_B], aff0, B, N, M, stat0);
  if (compute_dtype == CATRE_DTYPE_SPLIT)
    hipLaunchKernelGGL(k_rot_l1_split<true>, dim3(B * T), dim3(256), 0, st, pointfeat, pkb(packed, L.sp_rot_l0[0]),
                       pkb(packed, L.sp_rot_l0[1]), aff0, pkb(packed, L.sp_rot_l1[0]), pkb(packed, L.sp_rot_l1[1]),
                       prm[CATRE_P_ROTX_L1_B], prm[CATRE_P_ROTY_L1_B], y1, gn1_part, B, N, M, (unsigned long long*)nullptr,
                       bias0, y0, a0);
  else
    hipLaunchKernelGGL((k_rot_l1<1, true>), dim3(B * T), dim3(256), 0, st, pointfeat, pk4(packed, L.rot_l0[0]),
                       pk4(packed, L.rot_l0[1]), aff0, pk4(packed, L.rot_l1[0]), pk4(packed, L.rot_l1[1]),
                       prm[CATRE_P_ROTX_L1_B], prm[CATRE_P_ROTY_L1_B], y1, gn1_part, B, N, M, (unsigned long long*)nullptr,
                       bias0, y0, a0);
  return check_launch();
}

// ---- training forward of the encoder on the fused kernels (k_stn3d / k_stnkd / k_trunk with SAVE): one launch per
// block computes the pooled feature AND writes the activations the layer-wise backward reads (cloud-major point rows),
// instead of one row GEMM per layer with every intermediate streamed through HBM twice.  N, M multiples of 64.
namespace {
// the compute mode and the weight images of a training forward
inline int train_mode(int compute_dtype) {
  return compute_dtype == CATRE_DTYPE_BF16 ? MODE_BF16 : compute_dtype == CATRE_DTYPE_SPLIT ? MODE_SPLIT : MODE_F32;
}
inline PackKind train_pack(int compute_dtype) {
  return compute_dtype == CATRE_DTYPE_BF16 ? PK_BF16 : compute_dtype == CATRE_DTYPE_SPLIT ? PK_SPLIT : PK_F32;
}
inline bool train_dims_ok(int B, int N, int M) { return B > 0 && N > 0 && M > 0 && N % TP == 0 && M % TP == 0; }
struct TrainScratch {
  float* pmax;
  int* pidx;
};
inline TrainScratch train_scratch(float* ws, const WsLayout& W, int tiles) {
  float* pmax = ws + W.y1;  // the rot-head buffer is idle while the encoder runs
  return TrainScratch{pmax, reinterpret_cast<int*>(pmax + (size_t)tiles * 1024)};
}
}  // namespace

int catre_train_stn3d_fwd(const catre_points* pts, const float* const* prm, const float* packed, float* a1, float* a2,
                          float* g, int32_t* idx, void* workspace, size_t ws_bytes, int B, int N, int M, int compute_dtype,
                          void* stream) {
  REQUIRE(pts && prm && packed && g && idx && workspace && train_dims_ok(B, N, M) && (a1 == nullptr) == (a2 == nullptr));
  if (compute_dtype != CATRE_DTYPE_F32 && compute_dtype != CATRE_DTYPE_BF16 && compute_dtype != CATRE_DTYPE_SPLIT)
    return CATRE_ERR_UNSUPPORTED;
  if (!a1 && compute_dtype != CATRE_DTYPE_F32) return CATRE_ERR_UNSUPPORTED;  // only the fp32 backward recomputes its rows
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const TrainScratch sc = train_scratch(ws, W, B * (N + M) / TP);
  TrainSave sv{a1, a2, nullptr, nullptr, nullptr, sc.pmax, sc.pidx};
  FormDecision d;
  if (const int rc = decide(STAGE_STN3D, train_mode(compute_dtype), true, a1 != nullptr, false, B, N, M, &d)) return rc;
  const EncCall c{pts, nullptr, nullptr, ws + W.pm, B, N, M, st};
  const Stn3dW w = stn3d_weights(prm, packed, pack_layout(1), train_pack(compute_dtype));
  const dim3 grid(d.grid), block(256);
  switch (d.form) {
    // grids that fill the chip: the 128-point pair kernel of the inference path with saves (221 -> ~140 us at B = 256)
    case CATRE_FORM_TRAIN_BF_PAIR: hipLaunchKernelGGL((k_stn3d_bf2<true>), grid, block, 0, st, STN3D_ARGS(c, w), sv); break;
    case CATRE_FORM_TRAIN_BF: hipLaunchKernelGGL((k_stn3d_bf<true>), grid, block, 0, st, STN3D_ARGS(c, w), sv); break;
    case CATRE_FORM_TRAIN_SPLIT: hipLaunchKernelGGL((k_stn3d_split<1, true>), grid, block, 0, st, STN3D_ARGS(c, w), sv); break;
    case CATRE_FORM_TRAIN_PAIR: hipLaunchKernelGGL(k_stn3d_pair<true>, grid, block, 0, st, STN3D_ARGS(c, w), sv); break;
    default: hipLaunchKernelGGL((k_stn3d<1, true>), grid, block, 0, st, STN3D_ARGS(c, w), sv);  // CATRE_FORM_TRAIN_RS1
  }
  return launch_maxpool_tiles(sc.pmax, sc.pidx, g, idx, 1024, B, N, M, st);
}

int catre_train_stnkd_fwd(const catre_points* pts, const float* trans3, const float* const* prm, const float* packed,
                          float* f1, float* f2, float* g, int32_t* idx, void* workspace, size_t ws_bytes, int B, int N,
                          int M, int compute_dtype, void* stream) {
  REQUIRE(pts && trans3 && prm && packed && g && idx && workspace && train_dims_ok(B, N, M) && (f1 == nullptr) == (f2 == nullptr));
  if (compute_dtype != CATRE_DTYPE_F32 && compute_dtype != CATRE_DTYPE_BF16 && compute_dtype != CATRE_DTYPE_SPLIT)
    return CATRE_ERR_UNSUPPORTED;
  if (!f1 && compute_dtype != CATRE_DTYPE_F32) return CATRE_ERR_UNSUPPORTED;
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const TrainScratch sc = train_scratch(ws, W, B * (N + M) / TP);
  TrainSave sv{f1, f2, nullptr, nullptr, nullptr, sc.pmax, sc.pidx};
  FormDecision d;
  if (const int rc = decide(STAGE_STNKD, train_mode(compute_dtype), true, f1 != nullptr, false, B, N, M, &d)) return rc;
  const EncCall c{pts, trans3, nullptr, ws + W.pm, B, N, M, st};
  const StnkdW w = stnkd_weights(prm, packed, pack_layout(1), train_pack(compute_dtype));
  const dim3 grid(d.grid), block(256);
  switch (d.form) {
    case CATRE_FORM_TRAIN_BF_PAIR: hipLaunchKernelGGL((k_stnkd_bf2<true>), grid, block, 0, st, STNKD_ARGS(c, w), sv); break;
    case CATRE_FORM_TRAIN_BF: hipLaunchKernelGGL((k_stnkd_bf<true>), grid, block, 0, st, STNKD_ARGS(c, w), sv); break;
    case CATRE_FORM_TRAIN_SPLIT: hipLaunchKernelGGL((k_stnkd_split<1, true>), grid, block, 0, st, STNKD_ARGS(c, w), sv); break;
    case CATRE_FORM_TRAIN_PAIR: hipLaunchKernelGGL(k_stnkd_pair<true>, grid, block, 0, st, STNKD_ARGS(c, w), sv); break;
    default: hipLaunchKernelGGL((k_stnkd<1, true>), grid, block, 0, st, STNKD_ARGS(c, w), sv);  // CATRE_FORM_TRAIN_RS1
  }
  return launch_maxpool_tiles(sc.pmax, sc.pidx, g, idx, 1024, B, N, M, st);
}

int catre_train_trunk_fwd(const catre_points* pts, const float* trans3, const float* trans64, const float* const* prm,
                          const float* packed, float* x1, float* h1, float* pf, float* a2, float* a3, float* g,
                          int32_t* idx, void* workspace, size_t ws_bytes, int B, int N, int M, int compute_dtype,
                          void* stream) {
  REQUIRE(pts && trans3 && prm && packed && x1 && h1 && pf && a2 && a3 && g && idx && workspace && train_dims_ok(B, N, M));
  if (compute_dtype != CATRE_DTYPE_F32 && compute_dtype != CATRE_DTYPE_BF16 && compute_dtype != CATRE_DTYPE_SPLIT)
    return CATRE_ERR_UNSUPPORTED;
  if (compute_dtype != CATRE_DTYPE_F32 && !trans64) return CATRE_ERR_UNSUPPORTED;  // the reduced-precision SAVE instances need the feature transform
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const TrainScratch sc = train_scratch(ws, W, B * (N + M) / TP);
  TrainSave sv{x1, h1, a2, a3, pf, sc.pmax, sc.pidx};
  FormDecision d;
  if (const int rc = decide(STAGE_TRUNK, train_mode(compute_dtype), true, true, false, B, N, M, &d)) return rc;
  const EncCall c{pts, trans3, trans64, ws + W.pm, B, N, M, st};
  const TrunkW w = trunk_weights(prm, packed, pack_layout(1), train_pack(compute_dtype));
  const dim3 grid(d.grid);
  unsigned long long* const no_trace = nullptr;
  switch (d.form) {
    case CATRE_FORM_TRAIN_BF_PAIR:
      hipLaunchKernelGGL((k_trunk_bf2<true>), grid, dim3(512), 0, st, TRUNK_ARGS(c, w, (u32x4*)nullptr), no_trace, sv);
      break;
    case CATRE_FORM_TRAIN_SPLIT: hipLaunchKernelGGL((k_trunk_split<1, true>), grid, dim3(512), 0, st, TRUNK_ARGS(c, w, pf), no_trace, sv); break;
    // k_trunk4 is the form for grids that fill the chip - one wave per SIMD; fewer tiles than workgroup slots keep the
    // 8-wave kernel.  Same bits either way.
    case CATRE_FORM_TRAIN_WAVE4: hipLaunchKernelGGL((k_trunk4<true>), grid, dim3(256), 0, st, TRUNK_ARGS(c, w, pf), no_trace, sv); break;
    default: hipLaunchKernelGGL((k_trunk<1, true>), grid, dim3(512), 0, st, TRUNK_ARGS(c, w, pf), no_trace, sv);  // CATRE_FORM_TRAIN_RS1
  }
  return launch_maxpool_tiles(sc.pmax, sc.pidx, g, idx, 1024, B, N, M, st);
}
