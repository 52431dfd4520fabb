// several two-stage column reductions as two launches (k_colsum_multi + k_reduce_multi, catre_train.h)
namespace {
struct RedPlan {
  RedJobs jobs;
  int sblk = 0, fblk = 0;
  RedPlan() { jobs.n = 0; }
  // out[J] (=|+=) column sums of src [R][ld]; outputs [0, n_a) to out_a, the rest to out_b; stage >= ((R + 63) / 64) * J floats
  void add(const float* src, int ld, int R, int J, float* stage, float* out_a, float* out_b, int n_a, int accumulate) {
    RedJob& j = jobs.j[jobs.n++];
    j.src = src, j.stage = stage, j.out_a = out_a, j.out_b = out_b;
    j.ld = ld, j.R = R, j.J = J, j.n_a = n_a, j.rps = 64, j.nsp = (R + 63) / 64, j.accumulate = accumulate;
    j.sb0 = sblk, j.fb0 = fblk;
    sblk += ((J + 255) / 256) * j.nsp;
    fblk += (J + 255) / 256;
  }
  void launch(hipStream_t st) const {
    hipLaunchKernelGGL(k_colsum_multi, dim3(sblk), dim3(256), 0, st, jobs);
    hipLaunchKernelGGL(k_reduce_multi, dim3(fblk), dim3(256), 0, st, jobs);
  }
};
}  // namespace

// catre_train_api.inc - C-ABI launchers of the training ops (included inside extern "C" of catre_train.hip).
// Every op is stream-ordered, allocation-free (scratch comes in through `ws`) and returns a catre_status.

static inline size_t tn_splits(int R) {
  // rows per split: a multiple of 32, at least 2048 rows, at most 256 splits
  size_t s = ((size_t)R + 2047) / 2048;
  return s > 256 ? 256 : (s < 1 ? 1 : s);
}
// split count of the wgrad GEMM for a J x K gradient: at least one split per 2048 rows, and enough (tile, split)
// workgroups to fill the chip when the row count is small (few objects per batch) - but never slabs under 64 rows
static inline bool tn_skinny(int J, int K) { return K <= 8 && J <= 256 && J >= 4 && 256 % (J / 4) == 0; }
static inline size_t tn_splits_jk(int R, int J, int K) {
  if (tn_skinny(J, K)) {  // k_gemm_tn_skinny: >= 512 rows per workgroup, up to 1024 of them, two-stage merge
    const size_t s = ((size_t)R + 511) / 512;
    return s > 1024 ? 1024 : (s < 1 ? 1 : s);
  }
  const size_t tiles = (size_t)((J + 127) / 128) * ((K + 127) / 128);
  size_t s = tn_splits(R);
  const size_t want = (768 + tiles - 1) / tiles;
  if (s < want) s = want;
  const size_t cap = ((size_t)R + 63) / 64;
  if (s > cap) s = cap;
  // the narrow tile (K <= 64) fits three workgroups per CU: up to 768 of them (merged in two stages beyond 256)
  const size_t most = K <= 64 ? 768 : 256;
  if (s > most) s = most;
  return s < 1 ? 1 : s;
}
static inline int rows_per_split(int R, size_t splits) { return (int)(((R + splits - 1) / splits + 31) / 32 * 32); }

int catre_op_pack(const float* src, int ld, int J, int K, int transpose, float* dst, void* stream) {
  REQUIRE(src && dst && J > 0 && K > 0 && (J % 32) == 0 && (K % 8) == 0);
  const int n = J * K;
  hipLaunchKernelGGL(k_op_pack, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, ld, J, K, transpose, dst);
  return check_launch();
}

// Y[R,J] = act(X[R,K] Wl^T + bias) (then zeroed where mask <= 0).  Wp = catre_op_pack of Wl [J,K].
// J: multiple of 32 with J <= 256 or J % 256 == 0 (J <= 1024); K in {8, 16, 32, 64, 128} or a multiple of 256.
int catre_op_gemm_rows(const float* X, int ldx, const float* Wp, const float* bias, const float* mask, int ldm,
                       float* Y, int ldy, int R, int J, int K, int relu, void* stream) {
  return catre_op_gemm_rows_m(X, ldx, nullptr, 0, Wp, bias, mask, ldm, Y, ldy, R, J, K, relu, stream);
}

// same, with the left operand masked on load: (X .* (xmask > 0)) Wl^T - the dgrad of a layer whose output went
// through a ReLU, without a separate relu-backward pass
static int gemm_rows_f32_launch(const float* X, int ldx, const float* xmask, int ldxm, const float* Wp,
                                const float* bias, const float* mask, int ldm, float* Y, int ldy, int R, int J, int K,
                                int relu, void* stream, CloudBias cb, const int* Rdev = nullptr,
                                const int* mrows = nullptr);

int catre_op_gemm_rows_m(const float* X, int ldx, const float* xmask, int ldxm, const float* Wp, const float* bias,
                         const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu, void* stream) {
  return gemm_rows_f32_launch(X, ldx, xmask, ldxm, Wp, bias, mask, ldm, Y, ldy, R, J, K, relu, stream, CloudBias{0, 0, 0, nullptr});
}

static int gemm_rows_f32_launch(const float* X, int ldx, const float* xmask, int ldxm, const float* Wp,
                                const float* bias, const float* mask, int ldm, float* Y, int ldy, int R, int J, int K,
                                int relu, void* stream, CloudBias cb, const int* Rdev, const int* mrows) {
  REQUIRE(X && Wp && Y && R > 0 && J > 0 && K > 0 && (ldx % 4) == 0 && (ldy % 4) == 0 && (J % 32) == 0);
  REQUIRE(!mrows || mask);
  REQUIRE(!xmask || (ldxm % 4) == 0);
  REQUIRE(J <= 1024 && (J <= 256 || J == 512 || J == 1024));
  REQUIRE(!mask || (ldm % 4) == 0);
  const int mb = J <= 256 ? 1 : J / 256;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((R + TP - 1) / TP), blk(512);
  const f32x4* wp = reinterpret_cast<const f32x4*>(Wp);
#define CATRE_GR(MBV, NKCV)                                                                                   \
  hipLaunchKernelGGL((k_gemm_rows<MBV, NKCV>), grid, blk, 0, st, X, ldx, wp, bias, mask, ldm, Y, ldy, R, J, K, relu, \
                     xmask, ldxm, cb, Rdev, mrows)
#define CATRE_GR_MB(NKCV)          \
  switch (mb) {                    \
    case 1: CATRE_GR(1, NKCV); break; \
    case 2: CATRE_GR(2, NKCV); break; \
    case 4: CATRE_GR(4, NKCV); break; \
    default: return CATRE_ERR_UNSUPPORTED; \
  }
  // (MB = 1 and at most four m-blocks at K = 128: the K-split instance keeps all eight waves on the matrix pipe - 53 -> 43 us
  // on the conv2-class dgrads of the row-sparse chains.  At K = 512 (conv3 dgrad, 244 us) the same split measured 250: that
  // instance waits for its 64 KiB chunk loads, not for issue slots.)
  if (K == 128 && mb == 1 && J <= 128) {
    hipLaunchKernelGGL((k_gemm_rows<1, 16, false, 2>), grid, blk, 0, st, X, ldx, wp, bias, mask, ldm, Y, ldy, R, J, K, relu,
                       xmask, ldxm, cb, Rdev, mrows);
  } else if (K % 256 == 0) {
    CATRE_GR_MB(32)
  } else if (K == 128) {
    CATRE_GR_MB(16)
  } else if (K == 64) {
    CATRE_GR_MB(8)
  } else if (K == 32) {
    CATRE_GR_MB(4)
  } else if (K == 16) {
    CATRE_GR_MB(2)
  } else if (K == 8) {
    CATRE_GR_MB(1)
  } else {
    return CATRE_ERR_UNSUPPORTED;
  }
#undef CATRE_GR_MB
#undef CATRE_GR
  return check_launch();
}

// ---- mixed precision: bf16 operands, fp32 accumulate / outputs (what torch.autocast does to these GEMMs)
int catre_op_pack_bf16(const float* src, int ld, int J, int K, int transpose, void* dst, void* stream) {
  REQUIRE(src && dst && J > 0 && K > 0 && (J % 32) == 0 && (K % 16) == 0);
  const int n = J * K;
  hipLaunchKernelGGL(k_op_pack_bf, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, ld, J, K, transpose,
                     (unsigned short*)dst);
  return check_launch();
}

// catre_op_gemm_rows_m / catre_op_linear_maxpool on bf16 operands.  Wp = catre_op_pack_bf16 of Wl [J,K];
// K in {64, 128, 256, 512}; J as catre_op_gemm_rows.  maxpool != 0: Y = per-tile maxima, mask = int arg-max rows.
static int gemm_rows_bf_launch(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                               const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu, int maxpool,
                               hipStream_t st, bool split = false, CloudBias cb = CloudBias{0, 0, 0, nullptr},
                               const int* Rdev = nullptr, const int* mrows = nullptr, int mask_bf16 = 0) {
  if (mask_bf16) {  // the dgrad of a chain layer behind the autocast encoder forward: J <= 256 outputs, ReLU mask as bf16 rows
    if (split || maxpool || J > 256) return CATRE_ERR_UNSUPPORTED;
    const dim3 gridh((R + TP - 1) / TP);
    const u32x4* wph = reinterpret_cast<const u32x4*>(Wp);
#define CATRE_GBH(CPV)                                                                                                  \
  hipLaunchKernelGGL((k_gemm_rows_bf<1, CPV, false, 8>), gridh, dim3(512), 0, st, X, ldx, wph, bias, mask, ldm, Y, ldy, \
                     R, J, relu, xmask, ldxm, cb, Rdev, mrows)
    switch (K) {
      case 64: CATRE_GBH(8); break;
      case 128: CATRE_GBH(16); break;
      case 256: CATRE_GBH(32); break;
      case 512: CATRE_GBH(64); break;
      default: return CATRE_ERR_UNSUPPORTED;
    }
#undef CATRE_GBH
    return check_launch();
  }
  const int mb = J <= 256 ? 1 : J / 256;
  const dim3 grid((R + TP - 1) / TP), blk(512);
  const u32x4* wp = reinterpret_cast<const u32x4*>(Wp);
#define CATRE_GB(MBV, CPV, MP)                                                                                          \
  do {                                                                                                                  \
    if (split)                                                                                                          \
      hipLaunchKernelGGL((k_gemm_rows_sp<MBV, CPV, MP>), grid, blk, 0, st, X, ldx, wp, bias, mask, ldm, Y, ldy, R, J,   \
                         relu, xmask, ldxm, cb, Rdev, mrows);                                                            \
    else                                                                                                                \
      hipLaunchKernelGGL((k_gemm_rows_bf<MBV, CPV, MP>), grid, blk, 0, st, X, ldx, wp, bias, mask, ldm, Y, ldy, R, J,   \
                         relu, xmask, ldxm, cb, Rdev, mrows);                                                            \
  } while (0)
#define CATRE_GB_MB(CPV)                                                   \
  switch (mb) {                                                            \
    case 1: if (maxpool) CATRE_GB(1, CPV, true); else CATRE_GB(1, CPV, false); break; \
    case 2: if (maxpool) CATRE_GB(2, CPV, true); else CATRE_GB(2, CPV, false); break; \
    case 4: if (maxpool) CATRE_GB(4, CPV, true); else CATRE_GB(4, CPV, false); break; \
    default: return CATRE_ERR_UNSUPPORTED;                                 \
  }
  switch (K) {
    case 64: CATRE_GB_MB(8) break;
    case 128: CATRE_GB_MB(16) break;
    case 256: CATRE_GB_MB(32) break;
    case 512: CATRE_GB_MB(64) break;
    default: return CATRE_ERR_UNSUPPORTED;
  }
#undef CATRE_GB_MB
#undef CATRE_GB
  return check_launch();
}

int catre_op_gemm_rows_bf16(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                            const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu, void* stream) {
  REQUIRE(X && Wp && Y && R > 0 && J > 0 && (ldx % 4) == 0 && (ldy % 4) == 0 && (J % 32) == 0);
  REQUIRE(J <= 1024 && (J <= 256 || J == 512 || J == 1024));
  REQUIRE((!mask || (ldm % 4) == 0) && (!xmask || (ldxm % 4) == 0));
  return gemm_rows_bf_launch(X, ldx, xmask, ldxm, Wp, bias, mask, ldm, Y, ldy, R, J, K, relu, 0, (hipStream_t)stream);
}

// split mode of the three entry points above: Wp = catre_op_pack_split of Wl [J,K] (2 * J * K bf16: hi pack, lo pack)
int catre_op_pack_split(const float* src, int ld, int J, int K, int transpose, void* dst, void* stream) {
  REQUIRE(src && dst && J > 0 && K > 0 && (J % 32) == 0 && (K % 16) == 0);
  const int n = J * K;
  hipLaunchKernelGGL(k_op_pack_split, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, ld, J, K, transpose,
                     (unsigned short*)dst);
  return check_launch();
}

int catre_op_gemm_rows_split(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                             const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu, void* stream) {
  REQUIRE(X && Wp && Y && R > 0 && J > 0 && (ldx % 4) == 0 && (ldy % 4) == 0 && (J % 32) == 0);
  REQUIRE(J <= 1024 && (J <= 256 || J == 512 || J == 1024));
  REQUIRE((!mask || (ldm % 4) == 0) && (!xmask || (ldxm % 4) == 0));
  return gemm_rows_bf_launch(X, ldx, xmask, ldxm, Wp, bias, mask, ldm, Y, ldy, R, J, K, relu, 0, (hipStream_t)stream,
                             true);
}

// Y = X Wl^T + bias2d[cloud(row)]: the row GEMM with a per-cloud bias (rows object-major: N observed then M prior rows
// per object; N, M multiples of 64; bias2d [2B][J]).  Wp: catre_op_pack (F32), catre_op_pack_bf16 or catre_op_pack_split.
int catre_op_gemm_rows_cloudbias(const float* X, int ldx, const void* Wp, const float* bias2d, float* Y, int ldy, int J,
                                 int K, int B, int N, int M, int compute_dtype, void* stream) {
  return catre_op_gemm_rows_gn(X, ldx, Wp, bias2d, 1, Y, ldy, J, K, B, N, M, nullptr, compute_dtype, stream);
}

// The rot-head linears (conv_out_per_rot_head.py:126-134): Y = X Wl^T + bias (per_cloud != 0: bias [2B][J] indexed by the
// row's cloud, else [J] or NULL) and, with gn_part != NULL (J == 256), the per-64-row-tile GroupNorm(32,256) partials
// [B*(N+M)/64][32][2] of Y as a by-product of the epilogue - catre_op_gnp_gelu_fwd_pre consumes them, which saves the
// statistics pass over Y.  Rows object-major, N and M multiples of 64.
int catre_op_gemm_rows_gn(const float* X, int ldx, const void* Wp, const float* bias, int per_cloud, float* Y, int ldy,
                          int J, int K, int B, int N, int M, float* gn_part, int compute_dtype, void* stream) {
  REQUIRE(X && Wp && Y && B > 0 && N > 0 && M >= 0 && (N % TP) == 0 && (M % TP) == 0 && (ldx % 4) == 0 &&
          (ldy % 4) == 0 && (J % 32) == 0 && J <= 1024 && (J <= 256 || J == 512 || J == 1024));
  REQUIRE(!per_cloud || bias);
  REQUIRE(!gn_part || J == 256);
  const int R = B * (N + M);
  const CloudBias cb{per_cloud ? B : 0, N, M, gn_part};
  if (compute_dtype == CATRE_DTYPE_F32)
    return gemm_rows_f32_launch(X, ldx, nullptr, 0, (const float*)Wp, bias, nullptr, 0, Y, ldy, R, J, K, 0, stream, cb);
  if (compute_dtype == CATRE_DTYPE_F16) return CATRE_ERR_UNSUPPORTED;  // fp16 operands: inference (catre_refine_*) only
  REQUIRE(compute_dtype == CATRE_DTYPE_BF16 || compute_dtype == CATRE_DTYPE_SPLIT);
  return gemm_rows_bf_launch(X, ldx, nullptr, 0, Wp, bias, nullptr, 0, Y, ldy, R, J, K, 0, 0, (hipStream_t)stream,
                             compute_dtype == CATRE_DTYPE_SPLIT, cb);
}

static int linear_maxpool_lp(const float* X, int ldx, const void* Wp, const float* bias, float* out, int* idx, int J,
                             int K, int B, int N, int M, void* ws, size_t ws_bytes, void* stream, bool split);

int catre_op_linear_maxpool_split(const float* X, int ldx, const void* Wp, const float* bias, float* out, int* idx, int J,
                                  int K, int B, int N, int M, void* ws, size_t ws_bytes, void* stream) {
  return linear_maxpool_lp(X, ldx, Wp, bias, out, idx, J, K, B, N, M, ws, ws_bytes, stream, true);
}

int catre_op_linear_maxpool_bf16(const float* X, int ldx, const void* Wp, const float* bias, float* out, int* idx, int J,
                                 int K, int B, int N, int M, void* ws, size_t ws_bytes, void* stream) {
  return linear_maxpool_lp(X, ldx, Wp, bias, out, idx, J, K, B, N, M, ws, ws_bytes, stream, false);
}

static int linear_maxpool_lp(const float* X, int ldx, const void* Wp, const float* bias, float* out, int* idx, int J,
                             int K, int B, int N, int M, void* ws, size_t ws_bytes, void* stream, bool split) {
  REQUIRE(X && Wp && out && idx && ws && B > 0 && N > 0 && M >= 0 && (N % TP) == 0 && (M % TP) == 0 && (ldx % 4) == 0 &&
          (J % 32) == 0);
  REQUIRE(J <= 1024 && (J <= 256 || J == 512 || J == 1024));
  const int R = B * (N + M), tiles = R / TP;
  if (ws_bytes < (size_t)2 * tiles * J * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* pmax = (float*)ws;
  int* pidx = (int*)ws + (size_t)tiles * J;
  hipStream_t st = (hipStream_t)stream;
  const int rc = gemm_rows_bf_launch(X, ldx, nullptr, 0, Wp, bias, (const float*)pidx, 0, pmax, J, R, J, K, 0, 1, st, split);
  if (rc) return rc;
  hipLaunchKernelGGL(k_maxpool_tiles, dim3(M > 0 ? 2 * B : B, (J + 255) / 256), dim3(256), 0, st, pmax, pidx, out, idx, J,
                     B, N, M);
  return check_launch();
}

// g[C,J] = max over the points of each cloud of (X Wl^T + bias), idx = arg-max row (first maximum), without the
// [R,J] intermediate: per-64-row-tile partials (ws: 2 * tiles * J 4-byte words) then a per-cloud merge.  Needs
// N % 64 == 0 and M % 64 == 0 (tiles must not straddle clouds), J % 256 == 0 or J <= 256, K as catre_op_gemm_rows.
size_t catre_op_linear_maxpool_ws_bytes(int R, int J) {
  if (R <= 0 || J <= 0) return 0;
  return (size_t)2 * ((R + TP - 1) / TP) * J * sizeof(float);
}

int catre_op_linear_maxpool(const float* X, int ldx, const float* Wp, const float* bias, float* out, int* idx, int J,
                            int K, int B, int N, int M, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(X && Wp && out && idx && ws && B > 0 && N > 0 && M >= 0 && (N % TP) == 0 && (M % TP) == 0 && (ldx % 4) == 0 &&
          (J % 32) == 0);
  REQUIRE(J <= 1024 && (J <= 256 || J == 512 || J == 1024));
  const int R = B * (N + M), tiles = R / TP;
  if (ws_bytes < (size_t)2 * tiles * J * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* pmax = (float*)ws;
  int* pidx = (int*)ws + (size_t)tiles * J;
  const int mb = J <= 256 ? 1 : J / 256;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(tiles), blk(512);
  const f32x4* wp = reinterpret_cast<const f32x4*>(Wp);
#define CATRE_GM(MBV, NKCV)                                                                                    \
  hipLaunchKernelGGL((k_gemm_rows<MBV, NKCV, true>), grid, blk, 0, st, X, ldx, wp, bias, (const float*)pidx, 0, pmax, \
                     J, R, J, K, 0, nullptr, 0, CloudBias{0, 0, 0, nullptr})
#define CATRE_GM_MB(NKCV)             \
  switch (mb) {                       \
    case 1: CATRE_GM(1, NKCV); break; \
    case 2: CATRE_GM(2, NKCV); break; \
    case 4: CATRE_GM(4, NKCV); break; \
    default: return CATRE_ERR_UNSUPPORTED; \
  }
  if (K % 256 == 0) {
    CATRE_GM_MB(32)
  } else if (K == 128) {
    CATRE_GM_MB(16)
  } else if (K == 64) {
    CATRE_GM_MB(8)
  } else {
    return CATRE_ERR_UNSUPPORTED;
  }
#undef CATRE_GM_MB
#undef CATRE_GM
  hipLaunchKernelGGL(k_maxpool_tiles, dim3(M > 0 ? 2 * B : B, (J + 255) / 256), dim3(256), 0, st, pmax, pidx, out, idx, J,
                     B, N, M);
  return check_launch();
}

size_t catre_op_gemm_tn_ws_bytes(int J, int K, int R) {
  if (J <= 0 || K <= 0 || R <= 0) return 0;
  return catre_op_gemm_tn_bias_ws_bytes(J, K, R);
}

// dW[J,K] (=|+=) dY[R,J]^T X[R,K]; deterministic (fixed split order).  J, K multiples of 4.
size_t catre_op_gemm_tn_bias_ws_bytes(int J, int K, int R) {
  if (J <= 0 || K <= 0 || R <= 0) return 0;
  const size_t sp = tn_splits_jk(R, J, K);
  return (sp + (sp + 63) / 64) * ((size_t)J * K + J) * sizeof(float);  // partials + the 64-way stage of the merge
}

int catre_op_gemm_tn_bias(const float* dY, int ldy, const float* X, int ldx, float* dW, float* db, int J, int K, int R,
                          int accumulate, void* ws, size_t ws_bytes, void* stream) {
  return catre_op_gemm_tn_bias_m(dY, ldy, nullptr, 0, X, ldx, dW, db, J, K, R, accumulate, ws, ws_bytes, stream);
}

// same with dY masked on load: (dY .* (ymask > 0))^T X and its column sums
int catre_op_gemm_tn_bias_m(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx, float* dW,
                            float* db, int J, int K, int R, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  return catre_op_gemm_tn_bias_lp(dY, ldy, ymask, ldym, X, ldx, dW, db, J, K, R, accumulate, ws, ws_bytes,
                                  CATRE_DTYPE_F32, stream);
}

// same with the products on the matrix pipe `compute_dtype` names: CATRE_DTYPE_F32 (fp32 MFMA), CATRE_DTYPE_BF16 (operands
// rounded to bf16, fp32 accumulation - the backward of a layer that ran under autocast) or CATRE_DTYPE_SPLIT (hi + lo
// bf16 operands, three products).  The bias gradient is always summed in fp32 from the unrounded dY.
static int gemm_tn_impl(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx, float* dW,
                        float* db, int J, int K, int R, int accumulate, void* ws, size_t ws_bytes, int compute_dtype,
                        void* stream, const int* Rdev, const int* xrows = nullptr, int x_bf16 = 0);

int catre_op_gemm_tn_bias_lp(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx, float* dW,
                             float* db, int J, int K, int R, int accumulate, void* ws, size_t ws_bytes,
                             int compute_dtype, void* stream) {
  return gemm_tn_impl(dY, ldy, ymask, ldym, X, ldx, dW, db, J, K, R, accumulate, ws, ws_bytes, compute_dtype, stream, nullptr);
}

static int gemm_tn_impl(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx, float* dW,
                        float* db, int J, int K, int R, int accumulate, void* ws, size_t ws_bytes, int compute_dtype,
                        void* stream, const int* Rdev, const int* xrows, int x_bf16) {
  if (compute_dtype == CATRE_DTYPE_F16) return CATRE_ERR_UNSUPPORTED;  // fp16 operands: inference (catre_refine_*) only
  REQUIRE(compute_dtype == CATRE_DTYPE_F32 || compute_dtype == CATRE_DTYPE_BF16 || compute_dtype == CATRE_DTYPE_SPLIT);
  REQUIRE(!ymask || (ldym % 4) == 0);
  REQUIRE(dY && X && dW && ws && J > 0 && K > 0 && R > 0 && (ldy % 4) == 0 && (ldx % 4) == 0 && (J % 4) == 0 &&
          (K % 4) == 0);
  // device-side row count (row-compacted operands): about a third of the rows are live (profiles/argmax_row_fraction.py), so
  // the splits are sized for that - fewer partials to merge; the kernels share whatever rows exist among the splits
  const int Rs = Rdev ? (R / 3 > 64 ? R / 3 : 64) : R;
  const size_t splits = tn_splits_jk(Rs, J, K);
  if (ws_bytes < (splits + (splits > 256 ? (splits + 63) / 64 : 0)) * ((size_t)J * K + (db ? J : 0)) * sizeof(float))
    return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int rps = rows_per_split(Rs, splits);
  const int nsp = (Rs + rps - 1) / rps;
  // partials: [split][J*K (+ J column sums)]; when db sits right behind dW one reduction covers both
  const size_t pitch = (size_t)J * K + (db ? J : 0);
  float* colpart = db ? (float*)ws + (size_t)J * K : nullptr;
  const dim3 grid((J + 127) / 128, (K + 127) / 128, nsp);
  if (tn_skinny(J, K)) {  // every compute_dtype: fp32 FMAs, no matrix pipe
    const size_t lds = (size_t)(256 / (J / 4)) * (J / 4) * (4 * (K <= 4 ? 4 : 8) + 4) * sizeof(float);
    if (K <= 4)
      hipLaunchKernelGGL(k_gemm_tn_skinny<4>, dim3(nsp), dim3(256), lds, st, dY, ldy, X, ldx, (float*)ws, J, K, R, rps,
                         colpart, ymask, ldym, pitch, Rdev, xrows);
    else
      hipLaunchKernelGGL(k_gemm_tn_skinny<8>, dim3(nsp), dim3(256), lds, st, dY, ldy, X, ldx, (float*)ws, J, K, R, rps,
                         colpart, ymask, ldym, pitch, Rdev, xrows);
  } else if (compute_dtype == CATRE_DTYPE_BF16)
    if (x_bf16)
      hipLaunchKernelGGL((k_gemm_tn_lp<false, true>), grid, dim3(256), 0, st, dY, ldy, X, ldx, (float*)ws, J, K, R, rps,
                         colpart, ymask, ldym, pitch, Rdev, xrows);
    else
      hipLaunchKernelGGL((k_gemm_tn_lp<false, false>), grid, dim3(256), 0, st, dY, ldy, X, ldx, (float*)ws, J, K, R, rps,
                         colpart, ymask, ldym, pitch, Rdev, xrows);
  else if (compute_dtype == CATRE_DTYPE_SPLIT)
    hipLaunchKernelGGL((k_gemm_tn_lp<true, false>), grid, dim3(256), 0, st, dY, ldy, X, ldx, (float*)ws, J, K, R, rps, colpart,
                       ymask, ldym, pitch, Rdev, xrows);
  else if (K <= 64)
    hipLaunchKernelGGL(k_gemm_tn<1>, dim3((J + 127) / 128, 1, nsp), dim3(512), 0, st, dY, ldy, X, ldx, (float*)ws, J, K, R,
                       rps, colpart, ymask, ldym, pitch, Rdev, xrows);
  else
    hipLaunchKernelGGL(k_gemm_tn<2>, grid, dim3(512), 0, st, dY, ldy, X, ldx, (float*)ws, J, K, R, rps, colpart, ymask,
                       ldym, pitch, Rdev, xrows);
  const int n = J * K;
  const float* parts = (const float*)ws;
  int nmerge = nsp;
  if (nsp > 256) {  // two-stage merge in a fixed order: 64 partials per stage row
    float* stage = (float*)ws + (size_t)nsp * pitch;
    nmerge = (nsp + 63) / 64;
    hipLaunchKernelGGL(k_colsum, dim3((unsigned)((pitch + 255) / 256), nmerge), dim3(256), 0, st, parts, (int)pitch, stage, nsp,
                       (int)pitch, 64);
    parts = stage;
  }
  if (db && db == dW + n) {
    hipLaunchKernelGGL(k_reduce_splits, dim3((n + J + 255) / 256), dim3(256), 0, st, parts, dW, n + J, nmerge,
                       accumulate);
  } else {
    hipLaunchKernelGGL(k_reduce_splits_p, dim3((n + 255) / 256), dim3(256), 0, st, parts, dW, n, nmerge,
                       accumulate, pitch);
    if (db)
      hipLaunchKernelGGL(k_reduce_splits_p, dim3((J + 255) / 256), dim3(256), 0, st, parts + n, db, J, nmerge,
                         accumulate, pitch);
  }
  return check_launch();
}

// Whole backward of a linear layer y = act(x W^T + b) on few rows (R < 2048), one launch (k_fc_bwd): with dv = dY .* (YM > 0)
// (YM: the layer's output when it ends in a ReLU, laid out like dY; or NULL),
//   dX[R,Kx] = dv W[J,Kw] (columns >= Kw zero),  dW[J,Kw] = dv^T X[R,Kx] (columns >= Kx zero),  db[J] = column sums of dv.
// dX, dW, db optional (db needs dW); dX / dW / db contiguous; no alignment or multiple-of-anything demands on J, Kx, Kw or the
// leading dimensions.  compute_dtype CATRE_DTYPE_BF16: the weight gradient's operands rounded to bf16 (fp32 accumulation);
// F32 and SPLIT: fp32 MFMAs.  Deterministic.
int catre_op_fc_bwd(const float* dY, int ldy, const float* YM, const float* X, int ldx, const float* W, int ldw, float* dX,
                    float* dW, float* db, int R, int J, int Kx, int Kw, int compute_dtype, void* stream) {
  if (compute_dtype == CATRE_DTYPE_F16) return CATRE_ERR_UNSUPPORTED;  // fp16 operands: inference (catre_refine_*) only
  REQUIRE(compute_dtype == CATRE_DTYPE_F32 || compute_dtype == CATRE_DTYPE_BF16 || compute_dtype == CATRE_DTYPE_SPLIT);
  REQUIRE(dY && R > 0 && R < 2048 && J > 0 && Kx > 0 && Kw > 0 && ldy >= J && (dX || dW));
  REQUIRE(!dX || (W && ldw >= Kw));
  REQUIRE(!dW || (X && ldx >= Kx));
  REQUIRE(!db || dW);
  FcBwdArgs a;
  a.dY = dY, a.YM = YM, a.X = X, a.W = W, a.dX = dX, a.dW = dW, a.db = db;
  a.ldy = ldy, a.ldx = ldx, a.ldw = ldw, a.R = R, a.J = J, a.Kx = Kx, a.Kw = Kw;
  a.dx_rb = (R + 31) / 32;
  a.ndx = dX ? a.dx_rb * ((Kx + 31) / 32) : 0;
  a.dw_jb = (J + 31) / 32;
  const int ndw = dW ? a.dw_jb * ((Kw + 31) / 32) : 0;
  if (compute_dtype == CATRE_DTYPE_BF16)
    hipLaunchKernelGGL(k_fc_bwd<true>, dim3(a.ndx + ndw), dim3(64 * FCB_WAVES), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_fc_bwd<false>, dim3(a.ndx + ndw), dim3(64 * FCB_WAVES), 0, (hipStream_t)stream, a);
  return check_launch();
}

// Whole backward of a 64-channel layer whose input has <= 4 live columns (conv1 on 3-d points), one pass over the rows:
// dv = (dY (+ dY2)) .* (ymask > 0);  dW[64,4] = dv^T X[:, :4],  db[64] = column sums of dv (db == dW + 256: contiguous),
// dX[R, dxcols] = dv W[64, Kw] (columns >= Kw zero; dxcols 4 or 8).  dY2, ymask, dX (then W unused) optional.
// Workspace as catre_op_gemm_tn_bias_ws_bytes(64, 4, R).  Deterministic (fixed merge order).
int catre_op_skinny_bwd(const float* dY, int ldy, const float* dY2, int ldy2, const float* ymask, int ldym, const float* X,
                        int ldx, const float* W, int ldw, int Kw, float* dW, float* db, float* dX, int lddx, int dxcols,
                        int R, void* ws, size_t ws_bytes, void* stream) {
  const int J = 64, K = 4;
  REQUIRE(dY && X && dW && db == dW + J * K && ws && R > 0 && (ldy % 4) == 0 && (ldx % 4) == 0 && ldx >= 4);
  REQUIRE((!dY2 || (ldy2 % 4) == 0) && (!ymask || (ldym % 4) == 0));
  REQUIRE(!dX || (W && Kw >= 1 && Kw <= 4 && ldw >= Kw && (dxcols == 4 || dxcols == 8) && lddx >= dxcols && (lddx % 4) == 0));
  if (ws_bytes < catre_op_gemm_tn_bias_ws_bytes(J, K, R)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  // three workgroups are resident per CU (130 VGPRs): at most 768 of them, so that the grid is one round on 256 CUs
  size_t splits = tn_splits_jk(R, J, K);
  if (splits > 768) splits = 768;
  const int rps = rows_per_split(R, splits);
  const int nsp = (R + rps - 1) / rps;
  const size_t pitch = (size_t)J * K + J;
  hipLaunchKernelGGL(k_skinny_bwd, dim3(nsp), dim3(256), 0, st, dY, ldy, dY2, ldy2, ymask, ldym, X, ldx, W, ldw, Kw,
                     (float*)ws, (float*)ws + (size_t)J * K, pitch, dX, lddx, dxcols, R, rps);
  const float* parts = (const float*)ws;
  int nmerge = nsp;
  if (nsp > 256) {  // two-stage merge in a fixed order: 64 partials per stage row
    float* stage = (float*)ws + (size_t)nsp * pitch;
    nmerge = (nsp + 63) / 64;
    hipLaunchKernelGGL(k_colsum, dim3((unsigned)((pitch + 255) / 256), nmerge), dim3(256), 0, st, parts, (int)pitch, stage, nsp,
                       (int)pitch, 64);
    parts = stage;
  }
  hipLaunchKernelGGL(k_reduce_splits, dim3((unsigned)((pitch + 255) / 256)), dim3(256), 0, st, parts, dW, (int)pitch, nmerge, 0);
  return check_launch();
}

int catre_op_gemm_tn(const float* dY, int ldy, const float* X, int ldx, float* dW, int J, int K, int R, int accumulate,
                     void* ws, size_t ws_bytes, void* stream) {
  return catre_op_gemm_tn_bias(dY, ldy, X, ldx, dW, nullptr, J, K, R, accumulate, ws, ws_bytes, stream);
}
int catre_op_colsum(const float* dY, int ld, int R, int J, float* out, int accumulate, void* ws, size_t ws_bytes,
                    void* stream) {
  REQUIRE(dY && out && ws && R > 0 && J > 0);
  const size_t splits = tn_splits(R);
  if (ws_bytes < splits * (size_t)J * sizeof(float)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int rps = rows_per_split(R, splits);
  const int nsp = (R + rps - 1) / rps;
  hipLaunchKernelGGL(k_colsum, dim3((J + 255) / 256, nsp), dim3(256), 0, st, dY, ld, (float*)ws, R, J, rps);
  hipLaunchKernelGGL(k_reduce_splits, dim3((J + 255) / 256), dim3(256), 0, st, (const float*)ws, out, J, nsp, accumulate);
  return check_launch();
}

// out[i] (=|+=) sum_s part[s][i]
int catre_op_reduce_splits(const float* part, float* out, int n, int splits, int accumulate, void* stream) {
  REQUIRE(part && out && n > 0 && splits > 0);
  hipLaunchKernelGGL(k_reduce_splits, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, out, n, splits,
                     accumulate);
  return check_launch();
}

// Y[r][:] += bias[cloud(r)][:], rows object-major ([N observed | M prior] per object), J % 4 == 0
int catre_op_rowbias_add(float* Y, int ld, const float* bias, int J, int B, int N, int M, void* stream) {
  REQUIRE(Y && bias && J > 0 && (J % 4) == 0 && (ld % 4) == 0 && B > 0 && N > 0 && M >= 0);
  const int R = B * (N + M);
  const size_t n = (size_t)R * (J / 4);
  hipLaunchKernelGGL(k_rowbias_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Y, ld, bias, R,
                     J, B, N, M);
  return check_launch();
}

int catre_op_rowbias_bwd(const float* dY, int ld, float* dbias, int J, int B, int N, int M, void* stream) {
  REQUIRE(dY && dbias && J > 0 && B > 0 && N > 0 && M >= 0);
  hipLaunchKernelGGL(k_rowbias_bwd, dim3(M > 0 ? 2 * B : B, (J + 63) / 64), dim3(256), 0, (hipStream_t)stream, dY, ld,
                     dbias, J, B, N, M);
  return check_launch();
}

// max over the points of each cloud (rows cloud-major: B*N observed rows, then B*M prior rows) with argmax row index
int catre_op_maxpool_fwd(const float* Y, int ld, float* out, int* idx, int J, int B, int N, int M, void* stream) {
  REQUIRE(Y && out && idx && J > 0 && B > 0 && N > 0 && M >= 0);
  hipLaunchKernelGGL(k_maxpool_fwd, dim3(M > 0 ? 2 * B : B, (J + 63) / 64), dim3(256), 0, (hipStream_t)stream, Y, ld,
                     out, idx, J, B, N, M);
  return check_launch();
}

// dY (pre-zeroed by the caller) [idx[c][j]][j] = dout[c][j]
int catre_op_maxpool_scatter(const float* dout, const int* idx, float* dY, int ld, int C, int J, void* stream) {
  REQUIRE(dout && idx && dY && C > 0 && J > 0);
  hipLaunchKernelGGL(k_maxpool_scatter, dim3((C * J + 255) / 256), dim3(256), 0, (hipStream_t)stream, dout, idx, dY, ld,
                     C, J);
  return check_launch();
}

// sparse backward of a linear layer followed by the max-pool: dW[J,K], db[J] from dg[C,J], idx, X[rows,K] (K <= 1024)
int catre_op_maxlin_bwd_w(const float* dg, const int* idx, const float* X, int ldx, float* dW, float* db, int C, int J,
                          int K, void* stream) {
  REQUIRE(dg && idx && X && dW && C > 0 && J > 0 && K > 0 && K <= 1024);
  const int Q = K / 4;
  if ((K % 4) == 0 && (ldx % 4) == 0 && Q <= 256 && 256 % Q == 0)
    hipLaunchKernelGGL(k_maxlin_bwd_w4<false>, dim3(J), dim3(256), 0, (hipStream_t)stream, dg, idx, X, ldx, dW, db, C, J, K);
  else
    hipLaunchKernelGGL(k_maxlin_bwd_w, dim3(J), dim3(256), 0, (hipStream_t)stream, dg, idx, X, ldx, dW, db, C, J, K);
  return check_launch();
}

// the same with X as bf16 rows (ldx in elements): the saved activations of the autocast encoder forward
int catre_op_maxlin_bwd_w_h(const float* dg, const int32_t* idx, const void* X, int ldx, float* dW, float* db, int C, int J,
                            int K, void* stream) {
  REQUIRE(dg && idx && X && dW && C > 0 && J > 0 && K > 0 && K <= 1024 && (K % 4) == 0 && (ldx % 4) == 0 &&
          256 % (K / 4) == 0);
  hipLaunchKernelGGL(k_maxlin_bwd_w4<true>, dim3(J), dim3(256), 0, (hipStream_t)stream, dg, (const int*)idx, (const float*)X,
                     ldx, dW, db, C, J, K, (const int*)nullptr);
  return check_launch();
}

// the same gradient from COMPACT rows Xc (dense row r at rowpos[r]; K % 4 == 0, 256 % (K / 4) == 0)
int catre_op_maxlin_bwd_w_c(const float* dg, const int32_t* idx, const int32_t* rowpos, const float* Xc, int ldx, float* dW,
                            float* db, int C, int J, int K, void* stream) {
  REQUIRE(dg && idx && rowpos && Xc && dW && C > 0 && J > 0 && K > 0 && K <= 1024 && (K % 4) == 0 && (ldx % 4) == 0 &&
          256 % (K / 4) == 0);
  hipLaunchKernelGGL(k_maxlin_bwd_w4<false>, dim3(J), dim3(256), 0, (hipStream_t)stream, dg, (const int*)idx, Xc, ldx, dW, db, C, J,
                     K, (const int*)rowpos);
  return check_launch();
}

// dX (pre-zeroed) [idx[c][j]][:] += dg[c][j] * W[j][:]
int catre_op_maxlin_bwd_x(const float* dg, const int* idx, const float* W, int ldw, float* dX, int ldx, int C, int J,
                          int K, void* stream) {
  REQUIRE(dg && idx && W && dX && C > 0 && J > 0 && K > 0);
  hipLaunchKernelGGL(k_maxlin_bwd_x, dim3(C), dim3(256), 0, (hipStream_t)stream, dg, idx, W, ldw, dX, ldx, J, K);
  return check_launch();
}

// same gradient, one cloud per workgroup walking its rows: writes EVERY row of dX[:, :K] (zeros where no channel had its
// maximum), so dX needs no memset; points per cloud <= 4096, J <= 1024, K % 4 == 0
int catre_op_maxlin_bwd_x_rows(const float* dg, const int* idx, const float* W, int ldw, float* dX, int ldx, int J, int K,
                               int B, int N, int M, void* stream) {
  REQUIRE(dg && idx && W && dX && J > 0 && J <= 1024 && K > 0 && (K % 4) == 0 && (ldw % 4) == 0 && (ldx % 4) == 0 &&
          B > 0 && N > 0 && M >= 0);
  if (N > MLX_MAXN || M > MLX_MAXN || K > 512) return CATRE_ERR_UNSUPPORTED;
  const int C = M > 0 ? 2 * B : B;
  int rs = (1024 + C - 1) / C;  // workgroups per cloud: the chip's workgroup slots filled once (see catre_op_maxlin_bwd_x_compact)
  rs = rs < 1 ? 1 : (rs > 16 ? 16 : rs);
  hipLaunchKernelGGL(k_maxlin_bwd_x_rows, dim3(C, rs), dim3(512), 0, (hipStream_t)stream, dg, idx, W, ldw, dX, ldx, J, K, B,
                     N, M);
  return check_launch();
}

// ---- row-sparse backward of linear + max-pool chains (kernels: "Row-sparse backward" in catre_train.h) ------------------
// rows [R] int32 (ascending live rows, first count[0] entries valid), rowpos [R] int32 (dense row -> compact row or -1),
// count [1] int32 on the device, scratch [2 * C] int32.  R = B * (N + M) rows, C clouds; clouds of <= 4096 points.
int catre_op_rows_compact(const float* dg, const int32_t* idx, int J, int B, int N, int M, int32_t* rows, int32_t* rowpos,
                          int32_t* count, int32_t* scratch, void* stream) {
  REQUIRE(dg && idx && rows && rowpos && count && scratch && J > 0 && B > 0 && N > 0 && M >= 0);
  if (N > MLX_MAXN || M > MLX_MAXN) return CATRE_ERR_UNSUPPORTED;
  const int C = M > 0 ? 2 * B : B;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rows_count, dim3(C), dim3(512), 0, st, dg, (const int*)idx, J, B, N, M, (int*)scratch);
  hipLaunchKernelGGL(k_rows_fill, dim3(C), dim3(512), 0, st, dg, (const int*)idx, J, B, N, M, (const int*)scratch, C,
                     (int*)rows, (int*)rowpos, (int*)count);
  return check_launch();
}

// catre_op_maxlin_bwd_x_rows into COMPACT rows: dXc[rowpos[r]][:K] for the rows that are somebody's arg-max only, zeroed
// where ymask[r][:] <= 0 (ymask: the ReLU output of the layer in front of the pool, dense rows; may be NULL)
int catre_op_maxlin_bwd_x_compact(const float* dg, const int32_t* idx, const float* W, int ldw, const int32_t* rowpos,
                                  const float* ymask, int ldym, float* dXc, int ldx, int J, int K, int B, int N, int M,
                                  void* stream) {
  REQUIRE(dg && idx && W && rowpos && dXc && J > 0 && J <= 1024 && K > 0 && (K % 4) == 0 && (ldw % 4) == 0 &&
          (ldx % 4) == 0 && B > 0 && N > 0 && M >= 0 && (!ymask || (ldym % 4) == 0));
  if (N > MLX_MAXN || M > MLX_MAXN || K > 512) return CATRE_ERR_UNSUPPORTED;
  const int C = M > 0 ? 2 * B : B;
  // workgroups per cloud: the row walk is a chain of dependent loads per live row (bucket entry -> dg, W row, mask row), so
  // it wants the chip's workgroup slots (4 per CU) filled once, each workgroup repeating the bucketing (measured on one box, B=256: 156 / 131 / 143 us for 512 / 1024 / 2048 slots; two live rows per wave at a time: no gain)
  int rs = (1024 + C - 1) / C;
  rs = rs < 1 ? 1 : (rs > 16 ? 16 : rs);
  hipLaunchKernelGGL(k_maxlin_bwd_x_rows, dim3(C, rs), dim3(512), 0, (hipStream_t)stream, dg, (const int*)idx, W, ldw, dXc,
                     ldx, J, K, B, N, M, (const int*)rowpos, ymask, ldym);
  return check_launch();
}

// catre_op_maxlin_bwd_x_compact with the ReLU mask given as COMPACT rows (row-sparse chains that recompute their activations)
int catre_op_maxlin_bwd_x_compact_cm(const float* dg, const int32_t* idx, const float* W, int ldw, const int32_t* rowpos,
                                     const float* ymask_c, int ldym, float* dXc, int ldx, int J, int K, int B, int N, int M,
                                     void* stream) {
  REQUIRE(dg && idx && W && rowpos && ymask_c && dXc && J > 0 && J <= 1024 && K > 0 && (K % 4) == 0 && (ldw % 4) == 0 &&
          (ldx % 4) == 0 && B > 0 && N > 0 && M >= 0 && (ldym % 4) == 0);
  if (N > MLX_MAXN || M > MLX_MAXN || K > 512) return CATRE_ERR_UNSUPPORTED;
  const int C = M > 0 ? 2 * B : B;
  int rs = (1024 + C - 1) / C;
  rs = rs < 1 ? 1 : (rs > 16 ? 16 : rs);
  hipLaunchKernelGGL(k_maxlin_bwd_x_rows, dim3(C, rs), dim3(512), 0, (hipStream_t)stream, dg, (const int*)idx, W, ldw, dXc,
                     ldx, J, K, B, N, M, (const int*)rowpos, ymask_c, ldym, 1);
  return check_launch();
}

// catre_op_maxlin_bwd_x_compact with the (dense) mask as bf16 rows (ldym in elements)
int catre_op_maxlin_bwd_x_compact_h(const float* dg, const int32_t* idx, const float* W, int ldw, const int32_t* rowpos,
                                    const void* ymask, int ldym, float* dXc, int ldx, int J, int K, int B, int N, int M,
                                    void* stream) {
  REQUIRE(dg && idx && W && rowpos && ymask && dXc && J > 0 && J <= 1024 && K > 0 && (K % 4) == 0 && (ldw % 4) == 0 &&
          (ldx % 4) == 0 && B > 0 && N > 0 && M >= 0 && (ldym % 4) == 0);
  if (N > MLX_MAXN || M > MLX_MAXN || K > 512) return CATRE_ERR_UNSUPPORTED;
  const int C = M > 0 ? 2 * B : B;
  int rs = (1024 + C - 1) / C;
  rs = rs < 1 ? 1 : (rs > 16 ? 16 : rs);
  hipLaunchKernelGGL(k_maxlin_bwd_x_rows, dim3(C, rs), dim3(512), 0, (hipStream_t)stream, dg, (const int*)idx, W, ldw, dXc,
                     ldx, J, K, B, N, M, (const int*)rowpos, (const float*)ymask, ldym, 0, 1);
  return check_launch();
}

// The two thin layers of an STN stack on the count[0] live rows of its row-sparse backward, as compact rows y1c [cap][64],
// y2c [cap][128] (k_stn_recompute).  kind 0: STN3d - X point rows [R][ldx >= 3], w1 = conv1.weight [64][3] raw, wp1 unused;
// kind 1: STNkd - X = h1 rows [R][64], wp1 = fragment pack of fstn.conv1 (catre_op_pack), w1 unused.  wp2: pack of conv2.
int catre_op_stn_recompute(int kind, const float* X, int ldx, const int32_t* rows, const int32_t* count, const float* w1,
                           const float* wp1, const float* b1, const float* wp2, const float* b2, float* y1c, float* y2c,
                           int cap, void* stream) {
  REQUIRE(X && rows && count && b1 && wp2 && b2 && y1c && y2c && cap > 0 && (kind == 0 ? (w1 && ldx >= 3) : (wp1 && ldx >= 64 && (ldx % 4) == 0)));
  const int grid = (cap + TP - 1) / TP;
  if (kind == 0)
    hipLaunchKernelGGL(k_stn_recompute<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, X, ldx, (const int*)rows,
                       (const int*)count, w1, (const f32x4*)nullptr, b1, reinterpret_cast<const f32x4*>(wp2), b2, y1c, y2c);
  else if (kind == 1)
    hipLaunchKernelGGL(k_stn_recompute<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, X, ldx, (const int*)rows,
                       (const int*)count, (const float*)nullptr, reinterpret_cast<const f32x4*>(wp1), b1,
                       reinterpret_cast<const f32x4*>(wp2), b2, y1c, y2c);
  else
    return CATRE_ERR_BAD_ARG;
  return check_launch();
}

// dst[i][:cols] = src[rows[i]][:cols], i < count[0] (cap: upper bound of count[0], sizes the grid)
int catre_op_gather_rows(const float* src, int lds_, const int32_t* rows, const int32_t* count, float* dst, int ldd, int cols,
                         int cap, void* stream) {
  REQUIRE(src && rows && count && dst && cols > 0 && (cols % 4) == 0 && (lds_ % 4) == 0 && (ldd % 4) == 0 && cap > 0);
  const int grid = cap / 4 < 1 ? 1 : (cap / 4 > 16384 ? 16384 : cap / 4);
  hipLaunchKernelGGL(k_gather_rows, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, lds_, (const int*)rows,
                     (const int*)count, dst, ldd, cols);
  return check_launch();
}

// dense[r][:cols] = rowpos[r] >= 0 ? srcc[rowpos[r]][:cols] : 0 for all R rows
int catre_op_scatter_rows(const float* srcc, int lds_, const int32_t* rowpos, float* dst, int ldd, int cols, int R,
                          void* stream) {
  REQUIRE(srcc && rowpos && dst && cols > 0 && (cols % 4) == 0 && (lds_ % 4) == 0 && (ldd % 4) == 0 && R > 0);
  const int grid = R / 4 < 1 ? 1 : (R / 4 > 16384 ? 16384 : R / 4);
  hipLaunchKernelGGL(k_scatter_rows, dim3(grid), dim3(256), 0, (hipStream_t)stream, srcc, lds_, (const int*)rowpos, dst, ldd,
                     cols, R);
  return check_launch();
}

// the same plus objsrc[object-major row of r][:cols] (rows of B objects, [N observed | M prior] each; R = B (N + M)), and
// then dst[idx[c][j]][j] += dmax[c][j] for the C x Jm entries of a max-pool over the same rows (dmax may be NULL): the sum
// of the three gradients pointfeat receives (conv stack, rotation heads, max over points) in two launches
int catre_op_scatter_rows_merge(const float* srcc, int lds_, const int32_t* rowpos, const float* objsrc, int ldo,
                                const float* dmax, const int32_t* idx_max, int Jm, float* dst, int ldd, int cols, int B, int N,
                                int M, void* stream) {
  REQUIRE(srcc && rowpos && dst && cols > 0 && (cols % 4) == 0 && (lds_ % 4) == 0 && (ldd % 4) == 0 && B > 0 && N > 0 &&
          M >= 0 && (!objsrc || (ldo % 4) == 0) && (!dmax || (idx_max && Jm > 0 && Jm <= cols)));
  const int R = B * (N + M), C = M > 0 ? 2 * B : B;
  const int grid = R / 4 < 1 ? 1 : (R / 4 > 16384 ? 16384 : R / 4);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_scatter_rows, dim3(grid), dim3(256), 0, st, srcc, lds_, (const int*)rowpos, dst, ldd, cols, R, objsrc,
                     ldo, B, N, M);
  if (dmax)
    hipLaunchKernelGGL(k_maxpool_scatter, dim3((C * Jm + 255) / 256), dim3(256), 0, st, dmax, (const int*)idx_max, dst, ldd, C,
                       Jm, 1);
  return check_launch();
}

// catre_op_gemm_rows_m / catre_op_gemm_tn_bias_m on the first nrows_dev[0] rows (device-side count, <= R): the tiles /
// splits past it do nothing; compute_dtype as catre_op_gemm_tn_bias_lp (Wp: the pack of that dtype).
int catre_op_gemm_rows_n(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                         const float* mask, int ldm, float* Y, int ldy, int R, int J, int K, int relu,
                         const int32_t* nrows_dev, int compute_dtype, void* stream) {
  REQUIRE(nrows_dev);
  if (compute_dtype == CATRE_DTYPE_F32)
    return gemm_rows_f32_launch(X, ldx, xmask, ldxm, (const float*)Wp, bias, mask, ldm, Y, ldy, R, J, K, relu, stream,
                                CloudBias{0, 0, 0, nullptr}, (const int*)nrows_dev);
  if (compute_dtype == CATRE_DTYPE_F16) return CATRE_ERR_UNSUPPORTED;  // fp16 operands: inference (catre_refine_*) only
  REQUIRE(compute_dtype == CATRE_DTYPE_BF16 || compute_dtype == CATRE_DTYPE_SPLIT);
  REQUIRE(X && Wp && Y && R > 0 && J > 0 && (ldx % 4) == 0 && (ldy % 4) == 0 && (J % 32) == 0);
  REQUIRE(J <= 1024 && (J <= 256 || J == 512 || J == 1024));
  return gemm_rows_bf_launch(X, ldx, xmask, ldxm, Wp, bias, mask, ldm, Y, ldy, R, J, K, relu, 0, (hipStream_t)stream,
                             compute_dtype == CATRE_DTYPE_SPLIT, CloudBias{0, 0, 0, nullptr}, (const int*)nrows_dev);
}
int catre_op_gemm_tn_bias_n(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx, float* dW,
                            float* db, int J, int K, int R, int accumulate, void* ws, size_t ws_bytes,
                            const int32_t* nrows_dev, int compute_dtype, void* stream) {
  REQUIRE(nrows_dev);
  return gemm_tn_impl(dY, ldy, ymask, ldym, X, ldx, dW, db, J, K, R, accumulate, ws, ws_bytes, compute_dtype, stream,
                      (const int*)nrows_dev);
}

// The two above with ROW INDIRECTION against dense tensors, so that the row-sparse backward needs no gathered copies of the
// saved activations: catre_op_gemm_rows_nr masks output row r with row mask_rows[r] of `mask` (a layer's ReLU mask taken
// from its dense saved output while the gradient rows are compact); catre_op_gemm_tn_bias_nr contracts dY row r with row
// x_rows[r] of X.  compute_dtype as catre_op_gemm_rows_n / catre_op_gemm_tn_bias_n; a null index array is the identity.
int catre_op_gemm_rows_nr(const float* X, int ldx, const float* xmask, int ldxm, const void* Wp, const float* bias,
                          const float* mask, int ldm, const int32_t* mask_rows, float* Y, int ldy, int R, int J, int K,
                          int relu, const int32_t* nrows_dev, int compute_dtype, void* stream) {
  REQUIRE(nrows_dev);
  const int mask_bf16 = (compute_dtype & CATRE_ROWS_BF16) != 0;  // `mask` holds bf16 rows (ldm in elements)
  compute_dtype &= ~CATRE_ROWS_BF16;
  if (compute_dtype == CATRE_DTYPE_F16) return CATRE_ERR_UNSUPPORTED;  // fp16 operands: inference (catre_refine_*) only
  REQUIRE(!mask_bf16 || (mask && compute_dtype == CATRE_DTYPE_BF16));
  if (compute_dtype == CATRE_DTYPE_F32)
    return gemm_rows_f32_launch(X, ldx, xmask, ldxm, (const float*)Wp, bias, mask, ldm, Y, ldy, R, J, K, relu, stream,
                                CloudBias{0, 0, 0, nullptr}, (const int*)nrows_dev, (const int*)mask_rows);
  REQUIRE(compute_dtype == CATRE_DTYPE_BF16 || compute_dtype == CATRE_DTYPE_SPLIT);
  REQUIRE(X && Wp && Y && R > 0 && J > 0 && (ldx % 4) == 0 && (ldy % 4) == 0 && (J % 32) == 0);
  REQUIRE(J <= 1024 && (J <= 256 || J == 512 || J == 1024) && (!mask_rows || mask));
  return gemm_rows_bf_launch(X, ldx, xmask, ldxm, Wp, bias, mask, ldm, Y, ldy, R, J, K, relu, 0, (hipStream_t)stream,
                             compute_dtype == CATRE_DTYPE_SPLIT, CloudBias{0, 0, 0, nullptr}, (const int*)nrows_dev,
                             (const int*)mask_rows, mask_bf16);
}
int catre_op_gemm_tn_bias_nr(const float* dY, int ldy, const float* ymask, int ldym, const float* X, int ldx,
                             const int32_t* x_rows, float* dW, float* db, int J, int K, int R, int accumulate, void* ws,
                             size_t ws_bytes, const int32_t* nrows_dev, int compute_dtype, void* stream) {
  REQUIRE(nrows_dev);
  const int x_bf16 = (compute_dtype & CATRE_ROWS_BF16) != 0;  // X holds bf16 rows (ldx in elements)
  compute_dtype &= ~CATRE_ROWS_BF16;
  if (compute_dtype == CATRE_DTYPE_F16) return CATRE_ERR_UNSUPPORTED;  // fp16 operands: inference (catre_refine_*) only
  REQUIRE(!x_bf16 || (compute_dtype == CATRE_DTYPE_BF16 && !tn_skinny(J, K)));
  return gemm_tn_impl(dY, ldy, ymask, ldym, X, ldx, dW, db, J, K, R, accumulate, ws, ws_bytes, compute_dtype, stream,
                      (const int*)nrows_dev, (const int*)x_rows, x_bf16);
}

// dst [rows][cols_pad] (contiguous) = src (element strides stride_row / stride_col) with zero columns behind it
int catre_op_pad_cols(const float* src, long stride_row, long stride_col, int rows, int cols, float* dst, int cols_pad,
                      void* stream) {
  REQUIRE(src && dst && rows > 0 && cols > 0 && cols_pad >= cols);
  const size_t n = (size_t)rows * cols_pad;
  hipLaunchKernelGGL(k_pad_cols, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, stride_row,
                     stride_col, rows, cols, dst, cols_pad);
  return check_launch();
}

// 64-row tiles of one cloud a workgroup of k_cloud_matmul64 takes: 4 once that still leaves >= 4 workgroups per CU, else 1
// (a pure host function: the launch below calls it, tests ask it which route a shape takes); -1 for sizes no launch accepts
int catre_op_cloud_matmul_tpw(int B, int N, int M) {
  if (B <= 0 || N <= 0 || M < 0) return -1;
  const int C = M > 0 ? 2 * B : B, maxn = N > M ? N : M, tiles = (maxn + 63) / 64;
  return (tiles >= 4 && (size_t)C * (tiles / 4) >= 1024) ? 4 : 1;
}

// Y[r][:] = X[r][:] T[cloud(r)] (or T^T), kd in {3, 64}; rows cloud-major
int catre_op_cloud_matmul(const float* X, int ldx, const float* T, float* Y, int ldy, int kd, int B, int N, int M,
                          int transpose, void* stream) {
  REQUIRE(X && T && Y && (kd == 3 || kd == 64) && B > 0 && N > 0 && M >= 0);
  const int C = M > 0 ? 2 * B : B, maxn = N > M ? N : M, R = B * (N + M);
  const dim3 grid((maxn + 63) / 64, C);
  if (kd == 3)
    hipLaunchKernelGGL((k_cloud_matmul<3>), grid, dim3(256), 0, (hipStream_t)stream, X, ldx, T, Y, ldy, R, B, N, M,
                       transpose);
  else if ((ldx % 4) == 0 && (ldy % 4) == 0) {
    const int tiles = (maxn + 63) / 64, tpw = catre_op_cloud_matmul_tpw(B, N, M);
    hipLaunchKernelGGL(k_cloud_matmul64, dim3((tiles + tpw - 1) / tpw, C), dim3(256), 0, (hipStream_t)stream, X, ldx, T, Y,
                       ldy, B, N, M, transpose, tpw);
  }
  else
    hipLaunchKernelGGL((k_cloud_matmul<64>), grid, dim3(256), 0, (hipStream_t)stream, X, ldx, T, Y, ldy, R, B, N, M,
                       transpose);
  return check_launch();
}

// dT[c] = X[c]^T dY[c]
int catre_op_cloud_matmul_bwd_t(const float* X, int ldx, const float* dY, int ldy, float* dT, int kd, int B, int N,
                                int M, void* stream) {
  REQUIRE(X && dY && dT && (kd == 3 || kd == 64) && B > 0 && N > 0 && M >= 0);
  const int C = M > 0 ? 2 * B : B;
  if (kd == 3)
    hipLaunchKernelGGL((k_cloud_matmul_bwd_t<3>), dim3(C), dim3(256), 0, (hipStream_t)stream, X, ldx, dY, ldy, dT, B, N,
                       M);
  else if ((ldx % 4) == 0 && (ldy % 4) == 0)
    hipLaunchKernelGGL(k_cloud_matmul64_bwd_t, dim3(C), dim3(256), 0, (hipStream_t)stream, X, ldx, dY, ldy, dT, B, N, M);
  else
    hipLaunchKernelGGL((k_cloud_matmul_bwd_t<64>), dim3(C), dim3(256), 0, (hipStream_t)stream, X, ldx, dY, ldy, dT, B,
                       N, M);
  return check_launch();
}

// out[R,K] = a + b + (c on its first Rc rows); a, b [R,K] contiguous, c [Rc,K] with leading dimension ldc, each optional
// (null = zeros)
int catre_op_sum_rows(const float* a, const float* b, const float* c, int ldc, float* out, int R, int Rc, int K, void* stream) {
  REQUIRE(out && R > 0 && K > 0 && Rc >= 0 && Rc <= R && (!c || ldc >= K));
  const size_t n = (size_t)R * K;
  hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, c, ldc, out, n,
                     (size_t)Rc * K, K);
  return check_launch();
}

int catre_op_relu_bwd(const float* dY, const float* Y, float* dX, size_t n, void* stream) {
  REQUIRE(dY && Y && dX && n > 0);
  hipLaunchKernelGGL(k_relu_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dY, Y, dX, n);
  return check_launch();
}

// GroupNorm(32,256)+GELU over the P points of each of B objects: A = gelu(GN(Y)), stat [B,32,2] = (mean, rstd)
int catre_op_gnp_gelu_fwd(const float* Y, const float* gamma, const float* beta, float* A, float* stat, int B, int P,
                          void* stream) {
  REQUIRE(Y && gamma && beta && A && stat && B > 0 && P > 0);
  hipStream_t st = (hipStream_t)stream;
  // chunk partials borrow the head of A (overwritten by the normalisation pass right after)
  const int nch = (P + GNS_CH - 1) / GNS_CH;
  if ((size_t)nch * 64 <= (size_t)P * 256) {
    hipLaunchKernelGGL(k_gnp_stats_chunk, dim3(B, nch), dim3(256), 0, st, Y, A, P, nch);
    hipLaunchKernelGGL(k_gnp_stats_final, dim3(B), dim3(256), 0, st, (const float*)A, stat, P, nch, GNS_CH);
  } else {
    hipLaunchKernelGGL(k_gnp_stats, dim3(B, 32), dim3(256), 0, st, Y, stat, P);
  }
  const size_t total4 = (size_t)B * P * 64;
  hipLaunchKernelGGL(k_gnp_gelu_fwd<false>, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, Y, stat, gamma, beta, A,
                     P, total4);
  return check_launch();
}

// ws >= B*64 + C*(64 + 512) + (C/64 + 1)*512 floats with C = B*ceil(P/128).  dgamma/dbeta [256] (=|+=)
int catre_op_gnp_gelu_bwd(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                          float* dY, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, int B,
                          int P, void* stream) {
  REQUIRE(dA && Y && stat && gamma && beta && dY && dgamma && dbeta && ws && B > 0 && P > 0);
  const int nch = (P + GNP_CH - 1) / GNP_CH;
  if (ws_bytes < ((size_t)B * 64 + (size_t)B * nch * (64 + 512) + ((size_t)B * nch / 64 + 1) * 512) * sizeof(float))
    return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* sums = (float*)ws;
  float* sums_part = sums + (size_t)B * 64;
  float* dgb = sums_part + (size_t)B * nch * 64;
  hipLaunchKernelGGL(k_gnp_bwd_sums<false>, dim3(B, nch), dim3(256), 0, st, dA, Y, stat, gamma, beta, sums_part, dgb, P);
  hipLaunchKernelGGL(k_gnp_bwd_sums_finalize, dim3((B * 64 + 255) / 256), dim3(256), 0, st, sums_part, sums, B, nch);
  const size_t total4 = (size_t)B * P * 64;
  hipLaunchKernelGGL(k_gnp_bwd_apply, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dA, Y, stat, sums,
                     gamma, beta, dY, P, total4);
  // dgb [B*nch][512] -> dgamma / dbeta in two stages (64-row column sums, then a fixed-order merge)
  const int S = B * nch, nsp = (S + 63) / 64;
  float* stage = dgb + (size_t)S * 512;
  hipLaunchKernelGGL(k_colsum, dim3(2, nsp), dim3(256), 0, st, dgb, 512, stage, S, 512, 64);
  hipLaunchKernelGGL(k_reduce_splits2, dim3(2), dim3(256), 0, st, stage, dgamma, dbeta, nsp, accumulate);
  return check_launch();
}

// same with the statistics taken from per-64-row-tile partials [B][P/64][32][2] (catre_op_gemm_rows_gn); P % 64 == 0
int catre_op_gnp_gelu_fwd_pre(const float* Y, const float* part64, const float* gamma, const float* beta, float* A,
                              float* stat, int B, int P, void* stream) {
  REQUIRE(Y && part64 && gamma && beta && A && stat && B > 0 && P > 0 && (P % TP) == 0);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gnp_stats_final, dim3(B), dim3(256), 0, st, part64, stat, P, P / TP, TP);
  const size_t total4 = (size_t)B * P * 64;
  hipLaunchKernelGGL(k_gnp_gelu_fwd<false>, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, Y, stat, gamma, beta, A,
                     P, total4);
  return check_launch();
}

// GroupNorm + GELU + neck in one op (training rot head, last stage).  Y [B*P,256], part64 as catre_op_gnp_gelu_fwd_pre,
// Wn [3][256] (rows >= rot_dim zero), bn [3] or NULL -> Y3 [B*P][3], stat [B,32,2].  P % 64 == 0.
int catre_op_gnp_gelu_neck_fwd(const float* Y, const float* part64, const float* gamma, const float* beta,
                               const float* Wn, const float* bn, float* Y3, float* stat, int B, int P, void* stream) {
  REQUIRE(Y && part64 && gamma && beta && Wn && Y3 && stat && B > 0 && P > 0 && (P % TP) == 0);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gnp_stats_final, dim3(B), dim3(256), 0, st, part64, stat, P, P / TP, TP);
  hipLaunchKernelGGL(k_gnp_gelu_neck_fwd, dim3((unsigned)((size_t)B * P / 64)), dim3(256), 0, st, Y, (const float*)stat,
                     gamma, beta, Wn, bn, Y3, P);
  return check_launch();
}

// The same with the conv_p weights wp [P] at hand (the neck output's only consumer, conv_out_per_rot_head.py:138-140):
// additionally leaves the per-tile moments Spart [B*P/64][3][256] from which catre_op_rot_l1_bwd_s takes the GroupNorm-1
// sums, dgamma, dbeta and dWn without reading Y again (k_gnp_gelu_neck_fwd_s).
int catre_op_gnp_gelu_neck_fwd_s(const float* Y, const float* part64, const float* gamma, const float* beta,
                                 const float* Wn, const float* bn, const float* wp, float* Y3, float* stat, float* Spart,
                                 int B, int P, void* stream) {
  REQUIRE(Y && part64 && gamma && beta && Wn && wp && Y3 && stat && Spart && B > 0 && P > 0 && (P % TP) == 0);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gnp_stats_final, dim3(B), dim3(256), 0, st, part64, stat, P, P / TP, TP);
  hipLaunchKernelGGL(k_gnp_gelu_neck_fwd_s<false>, dim3((unsigned)((size_t)B * P / 64)), dim3(256), 0, st, Y, (const float*)stat,
                     gamma, beta, Wn, bn, wp, Y3, Spart, P);
  return check_launch();
}

size_t catre_op_gnp_gelu_neck_bwd_ws_bytes(int B, int P) {
  const size_t S = (size_t)B * ((P + GNP_CH - 1) / GNP_CH);
  return ((size_t)B * 64 + S * (64 + 1280) + (S / 64 + 1) * 1280) * sizeof(float);
}

// dY3 [B*P][3] -> dY [B*P,256] and dparams [5][256] = dgamma, dbeta, dWn[0..2] (=|+=).  (dbn = column sums of dY3.)
int catre_op_gnp_gelu_neck_bwd(const float* dY3, const float* Y, const float* stat, const float* gamma,
                               const float* beta, const float* Wn, float* dY, float* dparams, int accumulate, void* ws,
                               size_t ws_bytes, int B, int P, void* stream) {
  REQUIRE(dY3 && Y && stat && gamma && beta && Wn && dY && dparams && ws && B > 0 && P > 0);
  if (ws_bytes < catre_op_gnp_gelu_neck_bwd_ws_bytes(B, P)) return CATRE_ERR_WORKSPACE;
  const int nch = (P + GNP_CH - 1) / GNP_CH;
  hipStream_t st = (hipStream_t)stream;
  float* sums = (float*)ws;
  float* sums_part = sums + (size_t)B * 64;
  float* dgb = sums_part + (size_t)B * nch * 64;
  hipLaunchKernelGGL(k_gnp_neck_bwd_sums, dim3(B, nch), dim3(256), 0, st, dY3, Y, stat, gamma, beta, Wn, sums_part, dgb, P);
  hipLaunchKernelGGL(k_gnp_bwd_sums_finalize, dim3((B * 64 + 255) / 256), dim3(256), 0, st, sums_part, sums, B, nch);
  const size_t total4 = (size_t)B * P * 64;
  hipLaunchKernelGGL(k_gnp_neck_bwd_apply, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dY3, Y, stat, sums,
                     gamma, beta, Wn, dY, P, total4);
  const int S = B * nch, nsp = (S + 63) / 64;
  float* stage = dgb + (size_t)S * 1280;
  hipLaunchKernelGGL(k_colsum, dim3(5, nsp), dim3(256), 0, st, dgb, 1280, stage, S, 1280, 64);
  hipLaunchKernelGGL(k_reduce_splits, dim3(5), dim3(256), 0, st, stage, dparams, 1280, nsp, accumulate);
  return check_launch();
}

// The same behind catre_op_gnp_gelu_neck_fwd_s when the neck output feeds conv_p only (dY3 [B*P][3] = wp[p] dout[b][:],
// catre_op_wsum_bwd's dY): the GroupNorm sums and dparams come from dout [B][3] and the forward's tile moments Spart - no
// reduction pass over Y (k_gnp_neck_bwd_sums, 0.5 GiB per head) - then the apply pass writes dY.  The per-head form of
// catre_op_rot_l1_bwd_s for the compute modes whose linear backward is not fused (autocast, split, shapes off the 64-grid
// of the fused fp32 kernels but with P % 64 == 0).
int catre_op_gnp_gelu_neck_bwd_s(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                                 const float* gamma, const float* beta, const float* Wn, float* dY, float* dparams, void* ws,
                                 size_t ws_bytes, int B, int P, void* stream) {
  REQUIRE(dY3 && dout && Spart && Y && stat && gamma && beta && Wn && dY && dparams && ws && B > 0 && P > 0 && (P % TP) == 0);
  if (ws_bytes < catre_op_gnp_gelu_neck_bwd_ws_bytes(B, P)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* sums = (float*)ws;
  float* dgb = sums + (size_t)B * 64;  // one slot per object
  hipLaunchKernelGGL(k_neck_sums_from_s, dim3(B), dim3(256), 0, st, dout, Spart, gamma, Wn, sums, dgb, P / TP);
  const size_t total4 = (size_t)B * P * 64;
  hipLaunchKernelGGL(k_gnp_neck_bwd_apply, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dY3, Y, stat, sums,
                     gamma, beta, Wn, dY, P, total4);
  const int nsp = (B + 63) / 64;
  float* stage = dgb + (size_t)B * 1280;
  hipLaunchKernelGGL(k_colsum, dim3(5, nsp), dim3(256), 0, st, dgb, 1280, stage, B, 1280, 64);
  hipLaunchKernelGGL(k_reduce_splits, dim3(5), dim3(256), 0, st, stage, dparams, 1280, nsp, 0);
  return check_launch();
}

// Backward of a rot head's layer-0 block y = x W^T + bias2d[cloud], a = gelu(GroupNorm(y)) from dA in two passes over
// (dA, Y): the GroupNorm sums, then k_rot_l0_bwd (dX, dW, dbias2d without a [R,256] gradient in HBM).  X [R,64] (ldx),
// W [256][64] row-major, rows object-major, N and M multiples of 64.  dX [R,64] (lddx), dW [256][64], dbias2d [2B][256]
// ([B][256] when M == 0), dgamma / dbeta [256].
size_t catre_op_rot_l0_bwd_ws_bytes(int B, int N, int M) {
  const int P = N + M, nch = (P + GNP_CH - 1) / GNP_CH, C = M > 0 ? 2 * B : B;
  const size_t S = (size_t)B * nch;
  return ((size_t)B * 64 + S * (64 + 512) + (S / 64 + 1) * 512 + 256 * 64 + (size_t)C * 16384 + ((size_t)C / 64 + 1) * 16384) *
         sizeof(float);
}
static int rot_l0_bwd_impl(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                           const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                           float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                           void* stream, bool lp, bool hb = false, bool sp = false) {
  REQUIRE(dA && Y && stat && gamma && beta && X && W && dX && dW && dbias2d && dgamma && dbeta && ws);
  REQUIRE(B > 0 && N > 0 && M >= 0 && (N % TP) == 0 && (M % TP) == 0 && (ldx % 4) == 0 && (lddx % 4) == 0);
  if (ws_bytes < catre_op_rot_l0_bwd_ws_bytes(B, N, M)) return CATRE_ERR_WORKSPACE;
  const int P = N + M, nch = (P + GNP_CH - 1) / GNP_CH, C = M > 0 ? 2 * B : B;
  hipStream_t st = (hipStream_t)stream;
  float* sums = (float*)ws;
  float* sums_part = sums + (size_t)B * 64;
  float* dgb = sums_part + (size_t)B * nch * 64;
  const int S = B * nch, nsp = (S + 63) / 64;
  float* stage = dgb + (size_t)S * 512;
  float* wpT = stage + ((size_t)S / 64 + 1) * 512;
  float* wpart = wpT + 256 * 64;
  float* wstage = wpart + (size_t)C * 16384;
  if (hb && !lp) return CATRE_ERR_UNSUPPORTED;
  if (hb)
    hipLaunchKernelGGL(k_gnp_bwd_sums<true>, dim3(B, nch), dim3(256), 0, st, dA, Y, stat, gamma, beta, sums_part, dgb, P);
  else
    hipLaunchKernelGGL(k_gnp_bwd_sums<false>, dim3(B, nch), dim3(256), 0, st, dA, Y, stat, gamma, beta, sums_part, dgb, P);
  hipLaunchKernelGGL(k_gnp_bwd_sums_finalize, dim3((B * 64 + 255) / 256), dim3(256), 0, st, sums_part, sums, B, nch);
  if (sp) {  // split mode: hi + lo operands, three products (k_rot_l0_bwd_sp); the two packs of W^T are the fp32 pack's bytes
    hipLaunchKernelGGL(k_op_pack_split, dim3(64), dim3(256), 0, st, W, 64, 64, 256, 1, reinterpret_cast<unsigned short*>(wpT));
    const size_t lds = (size_t)(4 * L0L_IMG + 2 * 64 * 8) * sizeof(u32x4);
    if (ensure_dyn_lds((const void*)k_rot_l0_bwd_sp, lds, DYN_L0_SP) != CATRE_OK) return CATRE_ERR_LAUNCH;
    hipLaunchKernelGGL(k_rot_l0_bwd_sp, dim3(C), dim3(512), lds, st, dA, Y, stat, (const float*)sums, gamma, beta, X, ldx,
                       reinterpret_cast<const u32x4*>(wpT), dX, lddx, wpart, dbias2d, B, N, M, accumulate_dx);
  } else if (lp) {  // bf16 operands on the matrix pipe (autocast); the bf16 pack of W^T fits the fp32 pack's slot
    hipLaunchKernelGGL(k_op_pack_bf, dim3(64), dim3(256), 0, st, W, 64, 64, 256, 1, reinterpret_cast<unsigned short*>(wpT));
    const size_t lds = (size_t)(2 * L0L_IMG + 64 * 8) * sizeof(u32x4);
    if (ensure_dyn_lds((const void*)k_rot_l0_bwd_bf<false>, lds, DYN_L0_BF) != CATRE_OK ||
        ensure_dyn_lds((const void*)k_rot_l0_bwd_bf<true>, lds, DYN_L0_BFH) != CATRE_OK)
      return CATRE_ERR_LAUNCH;
    if (hb)
      hipLaunchKernelGGL(k_rot_l0_bwd_bf<true>, dim3(C), dim3(512), lds, st, dA, Y, stat, (const float*)sums, gamma, beta, X, ldx,
                         reinterpret_cast<const u32x4*>(wpT), dX, lddx, wpart, dbias2d, B, N, M, accumulate_dx);
    else
      hipLaunchKernelGGL(k_rot_l0_bwd_bf<false>, dim3(C), dim3(512), lds, st, dA, Y, stat, (const float*)sums, gamma, beta, X, ldx,
                         reinterpret_cast<const u32x4*>(wpT), dX, lddx, wpart, dbias2d, B, N, M, accumulate_dx);
  } else {
    hipLaunchKernelGGL(k_op_pack, dim3(64), dim3(256), 0, st, W, 64, 64, 256, 1, wpT);  // logical [J = 64][K = 256] = W^T
    hipLaunchKernelGGL(k_rot_l0_bwd, dim3(C), dim3(512), 0, st, dA, Y, stat, (const float*)sums, gamma, beta, X, ldx,
                       reinterpret_cast<const f32x4*>(wpT), dX, lddx, wpart, dbias2d, B, N, M, accumulate_dx);
  }
  // dgb [S][512] -> dgamma | dbeta and wpart [C][16384] -> dW: two launches for both
  RedPlan red;
  red.add(dgb, 512, S, 512, stage, dgamma, dbeta, 256, 0);
  red.add(wpart, 16384, C, 16384, wstage, dW, nullptr, 16384, 0);
  red.launch(st);
  (void)nsp;
  return check_launch();
}

int catre_op_rot_l0_bwd(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                        const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                        float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                        void* stream) {
  return rot_l0_bwd_impl(dA, Y, stat, gamma, beta, X, ldx, W, dX, lddx, dW, dbias2d, dgamma, dbeta, accumulate_dx, ws, ws_bytes,
                         B, N, M, stream, false);
}
// ... in split mode (k_rot_l0_bwd_sp): hi + lo bf16 operands, three products - fp32-grade dX and dW on the bf16 matrix pipe
int catre_op_rot_l0_bwd_sp(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                           const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                           float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                           void* stream) {
  return rot_l0_bwd_impl(dA, Y, stat, gamma, beta, X, ldx, W, dX, lddx, dW, dbias2d, dgamma, dbeta, accumulate_dx, ws, ws_bytes,
                         B, N, M, stream, false, false, true);
}
// ... with the two GEMMs (dX = dY W, dW = dY^T X) on the bf16 matrix pipe (k_rot_l0_bwd_bf: bf16 operands, fp32 accumulation;
// GroupNorm / GELU', the bias gradient and all outputs fp32): the backward torch.autocast gives a bf16 linear
int catre_op_rot_l0_bwd_lp(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta,
                           const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                           float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                           void* stream) {
  return rot_l0_bwd_impl(dA, Y, stat, gamma, beta, X, ldx, W, dX, lddx, dW, dbias2d, dgamma, dbeta, accumulate_dx, ws, ws_bytes,
                         B, N, M, stream, true);
}

// Backward of a rot head's second block y = a W^T + b, y3 = neck(gelu(GroupNorm(y))) from dY3 [R,3]: the neck / GroupNorm
// sums pass, then k_rot_l1_bwd.  A [R,256] the block's input, W [256][256] row-major, Wn [3][256]; P % 64 == 0.
// dA [R,256], dWb [256*256 + 256] = dW then db, dparams [5][256] = dgamma, dbeta, dWn.
static inline int rot_l1_chunks(int B, int T) {
  int n = (256 + B - 1) / B;  // ~one workgroup per CU
  return n < 1 ? 1 : (n > T ? T : n);
}
size_t catre_op_rot_l1_bwd_ws_bytes(int B, int P) {
  const int nch = (P + GNP_CH - 1) / GNP_CH, T = P / TP, nck = rot_l1_chunks(B, T);
  const size_t S = (size_t)B * nch, G = (size_t)B * nck, pitch = 256 * 256 + 256;
  return ((size_t)B * 64 + S * (64 + 1280) + (S / 64 + 1) * 1280 + 256 * 256 + G * pitch + (G / 64 + 1) * pitch) * sizeof(float);
}
static int rot_l1_bwd_impl(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                           const float* gamma, const float* beta, const float* Wn, const float* A, const float* W, float* dA,
                           float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream,
                           bool lp = false, bool hb = false, bool sp = false) {
  REQUIRE(dY3 && Y && stat && gamma && beta && Wn && A && W && dA && dWb && dparams && ws && B > 0 && P > 0 && (P % TP) == 0);
  if (ws_bytes < catre_op_rot_l1_bwd_ws_bytes(B, P)) return CATRE_ERR_WORKSPACE;
  const int nch = (P + GNP_CH - 1) / GNP_CH, T = P / TP, nck = rot_l1_chunks(B, T), tpw = (T + nck - 1) / nck;
  const int S = B * nch, G = B * nck, gsp = (G + 63) / 64;
  const size_t pitch = 256 * 256 + 256;
  hipStream_t st = (hipStream_t)stream;
  float* sums = (float*)ws;
  float* sums_part = sums + (size_t)B * 64;
  float* dgb = sums_part + (size_t)S * 64;
  float* stage = dgb + (size_t)S * 1280;
  float* wpT = stage + ((size_t)S / 64 + 1) * 1280;
  float* wpart = wpT + 256 * 256;
  float* wstage = wpart + (size_t)G * pitch;
  int dgb_slots = S;
  if (hb && !(lp && Spart)) return CATRE_ERR_UNSUPPORTED;  // bf16 rows: only behind catre_op_gnp_gelu_neck_fwd_s_h
  if (Spart) {  // the sums and the (dgamma, dbeta, dWn) partials from the forward's tile moments: one slot per object
    hipLaunchKernelGGL(k_neck_sums_from_s, dim3(B), dim3(256), 0, st, dout, Spart, gamma, Wn, sums, dgb, T);
    dgb_slots = B;
  } else {
    hipLaunchKernelGGL(k_gnp_neck_bwd_sums, dim3(B, nch), dim3(256), 0, st, dY3, Y, stat, gamma, beta, Wn, sums_part, dgb, P);
    hipLaunchKernelGGL(k_gnp_bwd_sums_finalize, dim3((B * 64 + 255) / 256), dim3(256), 0, st, sums_part, sums, B, nch);
  }
  if (sp) {  // split mode: hi + lo bf16 operands, three products (k_rot_l1_bwd_sp); hi + lo packs of W^T = the fp32 pack's bytes
    hipLaunchKernelGGL(k_op_pack_split, dim3(256), dim3(256), 0, st, W, 256, 256, 256, 1, reinterpret_cast<unsigned short*>(wpT));
    const size_t lds = (size_t)6 * L1S_IMG * sizeof(u32x4);
    if (ensure_dyn_lds((const void*)k_rot_l1_bwd_sp, lds, DYN_L1_SP) != CATRE_OK) return CATRE_ERR_LAUNCH;
    hipLaunchKernelGGL(k_rot_l1_bwd_sp, dim3(B, nck), dim3(256), lds, st, dY3, Y, stat, (const float*)sums, gamma, beta, Wn, A,
                       reinterpret_cast<const u32x4*>(wpT), dA, wpart, P, tpw);
  } else if (lp) {  // bf16 operands on the matrix pipe (autocast): the pack of W^T as bf16 fragments fits the fp32 pack's slot
    hipLaunchKernelGGL(k_op_pack_bf, dim3(256), dim3(256), 0, st, W, 256, 256, 256, 1, reinterpret_cast<unsigned short*>(wpT));
    const size_t lds = (size_t)3 * L1L_IMG * sizeof(u32x4);
    if (ensure_dyn_lds((const void*)k_rot_l1_bwd_bf<false>, lds, DYN_L1_BF) != CATRE_OK ||
        ensure_dyn_lds((const void*)k_rot_l1_bwd_bf<true>, lds, DYN_L1_BFH) != CATRE_OK)
      return CATRE_ERR_LAUNCH;
    if (hb)
      hipLaunchKernelGGL(k_rot_l1_bwd_bf<true>, dim3(B, nck), dim3(256), lds, st, dY3, Y, stat, (const float*)sums, gamma, beta, Wn,
                         A, reinterpret_cast<const u32x4*>(wpT), dA, wpart, P, tpw,
                         g_trunk_trace ? g_trunk_trace + ((size_t)1 << 25) : nullptr);
    else
      hipLaunchKernelGGL(k_rot_l1_bwd_bf<false>, dim3(B, nck), dim3(256), lds, st, dY3, Y, stat, (const float*)sums, gamma, beta, Wn,
                         A, reinterpret_cast<const u32x4*>(wpT), dA, wpart, P, tpw,
                         g_trunk_trace ? g_trunk_trace + ((size_t)1 << 25) : nullptr);
  } else {
  hipLaunchKernelGGL(k_op_pack, dim3(256), dim3(256), 0, st, W, 256, 256, 256, 1, wpT);  // logical [in][out] = W^T
  const size_t lds = (size_t)TP * (L1B_LDY + L1B_LDA) * sizeof(float);
  if (ensure_dyn_lds((const void*)k_rot_l1_bwd, lds, DYN_L1) != CATRE_OK) return CATRE_ERR_LAUNCH;
  hipLaunchKernelGGL(k_rot_l1_bwd, dim3(B, nck), dim3(256), lds, st, dY3, Y, stat, (const float*)sums, gamma, beta, Wn, A,
                     reinterpret_cast<const f32x4*>(wpT), dA, wpart, P, tpw,
                     g_trunk_trace ? g_trunk_trace + ((size_t)1 << 25) : nullptr);
  }
  // dgb [slots][1280] -> dparams and wpart [G][256 * 256 + 256] -> dW | db: two launches for both
  RedPlan red;
  red.add(dgb, 1280, dgb_slots, 1280, stage, dparams, nullptr, 1280, 0);
  red.add(wpart, (int)pitch, G, (int)pitch, wstage, dWb, nullptr, (int)pitch, 0);
  red.launch(st);
  (void)gsp;
  return check_launch();
}

int catre_op_rot_l1_bwd(const float* dY3, const float* Y, const float* stat, const float* gamma, const float* beta,
                        const float* Wn, const float* A, const float* W, float* dA, float* dWb, float* dparams, void* ws,
                        size_t ws_bytes, int B, int P, void* stream) {
  return rot_l1_bwd_impl(dY3, nullptr, nullptr, Y, stat, gamma, beta, Wn, A, W, dA, dWb, dparams, ws, ws_bytes, B, P, stream);
}

// The same behind catre_op_gnp_gelu_neck_fwd_s: dY3 [B*P][3] must be wp[p] * dout[b][:] (catre_op_wsum_bwd's dY), dout [B][3]
// the gradient of the conv_p output; the GroupNorm sums and dparams come from Spart instead of a pass over Y.
int catre_op_rot_l1_bwd_s(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                          const float* gamma, const float* beta, const float* Wn, const float* A, const float* W, float* dA,
                          float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream) {
  REQUIRE(dout && Spart);
  return rot_l1_bwd_impl(dY3, dout, Spart, Y, stat, gamma, beta, Wn, A, W, dA, dWb, dparams, ws, ws_bytes, B, P, stream);
}

// catre_op_rot_l1_bwd / _s in split mode (k_rot_l1_bwd_sp): both GEMMs with hi + lo bf16 operands and three products - fp32-grade
// dA and dW on the bf16 matrix pipe.  dout and Spart: both or neither.
int catre_op_rot_l1_bwd_sp(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                           const float* gamma, const float* beta, const float* Wn, const float* A, const float* W, float* dA,
                           float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream) {
  REQUIRE((dout != nullptr) == (Spart != nullptr));
  return rot_l1_bwd_impl(dY3, dout, Spart, Y, stat, gamma, beta, Wn, A, W, dA, dWb, dparams, ws, ws_bytes, B, P, stream, false,
                         false, true);
}

// catre_op_rot_l1_bwd / _s with the two GEMMs on the bf16 matrix pipe (k_rot_l1_bwd_bf: bf16 operands, fp32 accumulation;
// the GroupNorm / GELU' arithmetic, the bias gradient and every output stay fp32) - the backward torch.autocast gives a bf16
// linear.  dout and Spart: both or neither.
int catre_op_rot_l1_bwd_lp(const float* dY3, const float* dout, const float* Spart, const float* Y, const float* stat,
                           const float* gamma, const float* beta, const float* Wn, const float* A, const float* W, float* dA,
                           float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream) {
  REQUIRE((dout != nullptr) == (Spart != nullptr));
  return rot_l1_bwd_impl(dY3, dout, Spart, Y, stat, gamma, beta, Wn, A, W, dA, dWb, dparams, ws, ws_bytes, B, P, stream, true);
}

// ---- the all-bf16 activation form of the autocast rotation heads (train_ops._RotHeadLP): the [rows,256] tensors between the
// kernels - y0, a0, y1 and dA - are bf16 rows (`void*`, 256 bf16 per row), what torch.autocast's Conv1d outputs are; every
// pass over them moves half the bytes.  Statistics, GroupNorm / GELU arithmetic, accumulation and all other outputs: fp32.
// catre_op_gemm_rows_gn on bf16 operands with io bit 0: X is bf16 rows (ldx in elements), bit 1: Y is bf16 rows (ldy in
// elements).  J = 256, K in {64, 256}.  per_cloud == 2 (fp32 X rows only): per-cloud bias AND the rows of X are cloud-major
// (B*N observed rows, then B*M prior rows - pointfeat as the trunk kernel writes it) while Y stays object-major.
int catre_op_gemm_rows_gn_h(const void* X, int ldx, const void* Wp, const float* bias, int per_cloud, void* Y, int ldy, int J,
                            int K, int B, int N, int M, float* gn_part, int io, void* stream) {
  REQUIRE(X && Wp && Y && B > 0 && N > 0 && M >= 0 && (N % TP) == 0 && (M % TP) == 0 && J == 256 && (K == 64 || K == 256));
  REQUIRE((ldx % 8) == 0 && (ldy % 8) == 0 && (!per_cloud || bias) && io >= 0 && io <= 3 && per_cloud >= 0 && per_cloud <= 2 &&
          (per_cloud != 2 || (io & 1) == 0));
  const int R = B * (N + M);
  const CloudBias cb{per_cloud ? B : 0, N, M, gn_part, per_cloud == 2 ? 1 : 0};
  const dim3 grid(R / TP), blk(512);
  hipStream_t st = (hipStream_t)stream;
  const u32x4* wp = reinterpret_cast<const u32x4*>(Wp);
  const float* x = (const float*)X;
  float* y = (float*)Y;
#define CATRE_GH(CPV, IOV)                                                                                                 \
  hipLaunchKernelGGL((k_gemm_rows_bf<1, CPV, false, IOV>), grid, blk, 0, st, x, ldx, wp, bias, (const float*)nullptr, 0, y, ldy, \
                     R, J, 0, (const float*)nullptr, 0, cb, (const int*)nullptr, (const int*)nullptr)
  if (K == 64) {
    switch (io) {
      case 0: CATRE_GH(8, 0); break;
      case 1: CATRE_GH(8, 1); break;
      case 2: CATRE_GH(8, 2); break;
      default: CATRE_GH(8, 3); break;
    }
  } else {
    switch (io) {
      case 0: CATRE_GH(32, 0); break;
      case 1: CATRE_GH(32, 1); break;
      case 2: CATRE_GH(32, 2); break;
      default: CATRE_GH(32, 3); break;
    }
  }
#undef CATRE_GH
  return check_launch();
}

// catre_op_gnp_gelu_fwd_pre_h + catre_op_gemm_rows_gn_h (K = 256, io = 3) as ONE kernel behind the statistics merge: Y0 (bf16
// rows) -> A = gelu(GroupNorm(Y0)) (bf16 rows, stored for the backward) -> Y1 = A W^T + bias (bf16 rows) + its GroupNorm tile
// partials.  The GroupNorm + GELU is applied while the GEMM stages its operand tile (k_gemm_rows_bf IO bit 2): same values
// as the two calls, no separate pass over [rows,256].  Wp: catre_op_pack_bf16 of W [256][256].
int catre_op_gn_gelu_gemm_rows_h(const void* Y0, const float* part64, const float* gamma, const float* beta, void* A,
                                 float* stat, const void* Wp, const float* bias, void* Y1, float* gn_part, int B, int N, int M,
                                 void* stream) {
  REQUIRE(Y0 && part64 && gamma && beta && A && stat && Wp && Y1 && B > 0 && N > 0 && M >= 0 && (N % TP) == 0 && (M % TP) == 0);
  const int P = N + M, R = B * P;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gnp_stats_final, dim3(B), dim3(256), 0, st, part64, stat, P, P / TP, TP);
  const CloudBias cb{0, N, M, gn_part};
  hipLaunchKernelGGL((k_gemm_rows_bf<1, 32, false, 7>), dim3(R / TP), dim3(512), 0, st, (const float*)Y0, 256,
                     reinterpret_cast<const u32x4*>(Wp), bias, (const float*)nullptr, 0, (float*)Y1, 256, R, 256, 0,
                     (const float*)nullptr, 0, cb, (const int*)nullptr, (const int*)nullptr, (const float*)stat, gamma, beta,
                     (unsigned short*)A, P);
  return check_launch();
}

// catre_op_gnp_gelu_fwd_pre with Y and A as bf16 rows
int catre_op_gnp_gelu_fwd_pre_h(const void* Y, const float* part64, const float* gamma, const float* beta, void* A,
                                float* stat, int B, int P, void* stream) {
  REQUIRE(Y && part64 && gamma && beta && A && stat && B > 0 && P > 0 && (P % TP) == 0);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gnp_stats_final, dim3(B), dim3(256), 0, st, part64, stat, P, P / TP, TP);
  const size_t total4 = (size_t)B * P * 64;
  hipLaunchKernelGGL(k_gnp_gelu_fwd<true>, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, Y, (const float*)stat, gamma,
                     beta, A, P, total4);
  return check_launch();
}

// catre_op_gnp_gelu_neck_fwd_s with Y as bf16 rows
int catre_op_gnp_gelu_neck_fwd_s_h(const void* Y, const float* part64, const float* gamma, const float* beta, const float* Wn,
                                   const float* bn, const float* wp, float* Y3, float* stat, float* Spart, int B, int P,
                                   void* stream) {
  REQUIRE(Y && part64 && gamma && beta && Wn && wp && Y3 && stat && Spart && B > 0 && P > 0 && (P % TP) == 0);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gnp_stats_final, dim3(B), dim3(256), 0, st, part64, stat, P, P / TP, TP);
  hipLaunchKernelGGL(k_gnp_gelu_neck_fwd_s<true>, dim3((unsigned)((size_t)B * P / 64)), dim3(256), 0, st, Y, (const float*)stat,
                     gamma, beta, Wn, bn, wp, Y3, Spart, P);
  return check_launch();
}

// catre_op_rot_l1_bwd_lp behind catre_op_gnp_gelu_neck_fwd_s_h: Y, A and dA are bf16 rows
int catre_op_rot_l1_bwd_h(const float* dY3, const float* dout, const float* Spart, const void* Y, const float* stat,
                          const float* gamma, const float* beta, const float* Wn, const void* A, const float* W, void* dA,
                          float* dWb, float* dparams, void* ws, size_t ws_bytes, int B, int P, void* stream) {
  REQUIRE(dout && Spart);
  return rot_l1_bwd_impl(dY3, dout, Spart, (const float*)Y, stat, gamma, beta, Wn, (const float*)A, W, (float*)dA, dWb, dparams,
                         ws, ws_bytes, B, P, stream, true, true);
}

// catre_op_rot_l0_bwd_lp with dA and Y as bf16 rows
int catre_op_rot_l0_bwd_h(const void* dA, const void* Y, const float* stat, const float* gamma, const float* beta,
                          const float* X, int ldx, const float* W, float* dX, int lddx, float* dW, float* dbias2d,
                          float* dgamma, float* dbeta, int accumulate_dx, void* ws, size_t ws_bytes, int B, int N, int M,
                          void* stream) {
  return rot_l0_bwd_impl((const float*)dA, (const float*)Y, stat, gamma, beta, X, ldx, W, dX, lddx, dW, dbias2d, dgamma, dbeta,
                         accumulate_dx, ws, ws_bytes, B, N, M, stream, true, true);
}

int catre_op_gnr_gelu_fwd(const float* Y, const float* gamma, const float* beta, float* A, int R, void* stream) {
  REQUIRE(Y && gamma && beta && A && R > 0);
  hipLaunchKernelGGL(k_gnr_gelu_fwd, dim3(R), dim3(256), 0, (hipStream_t)stream, Y, gamma, beta, A, R);
  return check_launch();
}

// ws >= R*512 floats
int catre_op_gnr_gelu_bwd(const float* dA, const float* Y, const float* gamma, const float* beta, float* dY,
                          float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, int R, void* stream) {
  REQUIRE(dA && Y && gamma && beta && dY && dgamma && dbeta && ws && R > 0);
  if (ws_bytes < (size_t)R * 512 * sizeof(float)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gnr_gelu_bwd, dim3(R), dim3(256), 0, st, dA, Y, gamma, beta, dY, (float*)ws, R);
  hipLaunchKernelGGL(k_reduce_splits_wide, dim3(8), dim3(1024), 0, st, (const float*)ws, dgamma, dbeta, 512, 256, R, accumulate,
                     (size_t)512);
  return check_launch();
}

// out[B,3] = sum_p w[p] * Y[b*P+p][0:3] + bias
int catre_op_wsum_fwd(const float* Y, const float* w, const float* bias, float* out, int B, int P, void* stream) {
  REQUIRE(Y && w && out && B > 0 && P > 0);
  hipLaunchKernelGGL(k_wsum_fwd, dim3(B), dim3(256), 0, (hipStream_t)stream, Y, w, bias, out, P);
  return check_launch();
}

// dY[B*P,3], dw[P] (=|+=), dbias[1] (=|+=, may be NULL); ws >= B*P floats
int catre_op_wsum_bwd(const float* dout, const float* Y, const float* w, float* dY, float* dw, float* dbias,
                      int accumulate, void* ws, size_t ws_bytes, int B, int P, void* stream) {
  return catre_op_wsum_bwd_n(dout, Y, w, dY, dw, dbias, nullptr, accumulate, ws, ws_bytes, B, P, stream);
}

// ... and dbn[3] = column sums of dY (the bias gradient of the 256 -> 3 neck in front of conv_p: dY is the neck's output
// gradient), taken as (sum_p w[p]) (sum_b dout[b][:]) in the same launch as dbias
int catre_op_wsum_bwd_n(const float* dout, const float* Y, const float* w, float* dY, float* dw, float* dbias, float* dbn,
                        int accumulate, void* ws, size_t ws_bytes, int B, int P, void* stream) {
  REQUIRE(dout && Y && w && dY && dw && ws && B > 0 && P > 0);
  if (ws_bytes < (size_t)B * P * sizeof(float)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_wsum_bwd, dim3((B * P + 255) / 256), dim3(256), 0, st, dout, Y, w, dY, (float*)ws, B, P);
  hipLaunchKernelGGL(k_reduce_splits_wide, dim3((P + 63) / 64), dim3(1024), 0, st, (const float*)ws, dw, (float*)nullptr, P, P, B,
                     accumulate, (size_t)P);
  if (dbn)
    hipLaunchKernelGGL(k_wsum_bias, dim3(1), dim3(256), 0, st, dout, w, B, P, dbias, dbn, accumulate);
  else if (dbias)
    hipLaunchKernelGGL(k_sum_acc, dim3(1), dim3(256), 0, st, dout, B * 3, dbias, accumulate);
  return check_launch();
}

// backward of catre_pose_update (ego and allo rot6d): d_pose [B,3,4], d_scale [B,3] -> d_rot6d [B,6], d_dt, d_ds [B,3]
int catre_op_pose_update_bwd(const float* d_pose, const float* d_scale, const float* rot6d, const float* trans_deltas,
                             const float* scale_deltas, const float* init_pose, const float* init_scale,
                             const float* mean_scales, const float* Ks, const catre_opts* o, float* d_rot6d,
                             float* d_dt, float* d_ds, int B, void* stream) {
  REQUIRE(d_pose && d_scale && rot6d && trans_deltas && scale_deltas && init_pose && init_scale && o && d_rot6d &&
          d_dt && d_ds && B > 0);
  if (o->rot_input_is_matrix) return CATRE_ERR_UNSUPPORTED;
  if (o->k_aware && !o->delta_t_space_3d && !Ks) return CATRE_ERR_BAD_ARG;
  if (o->scale_base_mean && !mean_scales) return CATRE_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_pose_update_bwd, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_pose, d_scale, rot6d,
                     trans_deltas, scale_deltas, init_pose, init_scale, mean_scales, Ks, *o, d_rot6d, d_dt, d_ds, B);
  return check_launch();
}

// f4: one fused Ranger step over every parameter tensor that has a gradient.  `tensors` = device array of
// n_tensors packed 72-byte records {p, g, exp_avg, exp_avg_sq, slow (5 pointers), numel, row_len, row_off,
// lr_step, wd_lr, adaptive, lookahead, pad}; `chunks` = device array of {tensor, offset} int pairs covering
// every tensor in pieces of 4096 elements; `row_tensor[total_rows]` maps each centralized gradient row to its
// tensor; rowmean_ws >= total_rows floats.  clean_grads applies nan_to_num(nan=0, +-inf -> +-grad_limit) first
// (core/catre/engine/engine.py:351-353).
int catre_op_ranger_step(const void* tensors, int n_tensors, const void* chunks, int n_chunks, const int* row_tensor,
                         int total_rows, float* rowmean_ws, double beta1, double beta2, float eps, float alpha,
                         int clean_grads, float grad_limit, void* stream) {
  REQUIRE(tensors && chunks && n_tensors > 0 && n_chunks > 0 && total_rows >= 0 && (total_rows == 0 || (row_tensor && rowmean_ws)));
  hipStream_t st = (hipStream_t)stream;
  if (total_rows > 0)
    hipLaunchKernelGGL(k_ranger_rowmean, dim3(total_rows), dim3(64), 0, st, (const RangerTensor*)tensors, row_tensor,
                       rowmean_ws, clean_grads, grad_limit);
  hipLaunchKernelGGL(k_ranger_update, dim3(n_chunks), dim3(256), 0, st, (const RangerTensor*)tensors,
                     (const int2*)chunks, rowmean_ws, (float)beta1, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), eps, alpha, clean_grads, grad_limit);
  return check_launch();
}


// f4, the reference's other optimizers: one fused step of optimizer `kind` (CATRE_OPTIM_*) over every parameter tensor
// that has a gradient.  `tensors` = device array of n_tensors packed 112-byte records {p, g, state[4] (6 pointers), numel,
// row_len, row_off, flags, f[12]} (catre_optim.h says what each kind keeps in state / flags / f); `chunks` as for
// catre_op_ranger_step; `row_tensor[n_rows]` maps every row of a tensor with row_len > 0 to its tensor.  `phases` bit 0:
// some tensor needs the reductions over the inputs, bit 1: some tensor needs the reductions over the update direction;
// a phase nobody needs is not launched.  ws >= (5 * n_rows + 4 * n_tensors) floats.
int catre_op_optim_step(int kind, const void* tensors, int n_tensors, const void* chunks, int n_chunks, const int* row_tensor,
                        int n_rows, int phases, float* ws, size_t ws_bytes, int clean_grads, float grad_limit, void* stream) {
  REQUIRE(tensors && chunks && n_tensors > 0 && n_chunks > 0 && n_rows >= 0 && ws && (n_rows == 0 || row_tensor));
  REQUIRE(ws_bytes >= ((size_t)5 * n_rows + (size_t)4 * n_tensors) * sizeof(float));
  if (kind < 0 || kind >= OPT_KINDS) return CATRE_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const OptimTensor* T = (const OptimTensor*)tensors;
  const int2* ch = (const int2*)chunks;
  float *rowA = ws, *rowB = ws + (size_t)4 * n_rows, *tens = ws + (size_t)5 * n_rows;
  const bool proj = kind == OPT_ADAMP || kind == OPT_SGDP;
  const bool p1 = (phases & 1) && n_rows > 0, p2 = (phases & 2) && n_rows > 0;
  if (p1 && proj) {
    hipLaunchKernelGGL(k_optim_rowstats, dim3(n_rows), dim3(64), 0, st, T, row_tensor, rowA, clean_grads, grad_limit);
    hipLaunchKernelGGL(k_optim_decide, dim3(n_tensors), dim3(64), 0, st, T, rowA, tens);
  } else if (p1) {
    hipLaunchKernelGGL(k_optim_rowmean, dim3(n_rows), dim3(64), 0, st, T, row_tensor, rowA, clean_grads, grad_limit);
  }
#define OPT_ROWS(K) \
  hipLaunchKernelGGL(k_optim_dir_rows<K>, dim3(n_rows), dim3(64), 0, st, T, row_tensor, rowA, rowB, tens, clean_grads, grad_limit)
#define OPT_UPDATE(K) \
  hipLaunchKernelGGL(k_optim_update<K>, dim3(n_chunks), dim3(256), 0, st, T, ch, rowA, rowB, tens, clean_grads, grad_limit)
  if (p2 && kind == OPT_RANGER_ADABELIEF) OPT_ROWS(OPT_RANGER_ADABELIEF);
  if (p2 && kind == OPT_ADAMP) OPT_ROWS(OPT_ADAMP);
  if (p2 && kind == OPT_SGDP) OPT_ROWS(OPT_SGDP);
  if (p2 && proj) hipLaunchKernelGGL(k_optim_tensor_sum, dim3(n_tensors), dim3(64), 0, st, T, rowB, tens);
  switch (kind) {
    case OPT_ADABELIEF: OPT_UPDATE(OPT_ADABELIEF); break;
    case OPT_RANGER_ADABELIEF: OPT_UPDATE(OPT_RANGER_ADABELIEF); break;
    case OPT_MADGRAD: OPT_UPDATE(OPT_MADGRAD); break;
    case OPT_NADAMW: OPT_UPDATE(OPT_NADAMW); break;
    case OPT_ADAMP: OPT_UPDATE(OPT_ADAMP); break;
    case OPT_SGDP: OPT_UPDATE(OPT_SGDP); break;
    default: OPT_UPDATE(OPT_SGD_GC); break;
  }
#undef OPT_ROWS
#undef OPT_UPDATE
  return check_launch();
}
