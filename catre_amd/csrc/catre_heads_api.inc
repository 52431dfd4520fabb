// C ABI of the generic norm + activation ops (kernels: catre_heads.h; declarations: include/catre_hip.h)
#define HA_SWITCH(act, norm, F)                \
  switch ((act) * 2 + ((norm) ? 1 : 0)) {      \
    case 0: F(CATRE_ACT_NONE, false); break;   \
    case 1: F(CATRE_ACT_NONE, true); break;    \
    case 2: F(CATRE_ACT_RELU, false); break;   \
    case 3: F(CATRE_ACT_RELU, true); break;    \
    case 4: F(CATRE_ACT_LRELU, false); break;  \
    case 5: F(CATRE_ACT_LRELU, true); break;   \
    case 6: F(CATRE_ACT_SILU, false); break;   \
    case 7: F(CATRE_ACT_SILU, true); break;    \
    case 8: F(CATRE_ACT_GELU, false); break;   \
    case 9: F(CATRE_ACT_GELU, true); break;    \
    case 10: F(CATRE_ACT_MISH, false); break;  \
    default: F(CATRE_ACT_MISH, true); break;   \
  }
#define HA_SWITCH_ACT(act, F)               \
  switch (act) {                            \
    case 0: F(CATRE_ACT_NONE); break;       \
    case 1: F(CATRE_ACT_RELU); break;       \
    case 2: F(CATRE_ACT_LRELU); break;      \
    case 3: F(CATRE_ACT_SILU); break;       \
    case 4: F(CATRE_ACT_GELU); break;       \
    default: F(CATRE_ACT_MISH); break;      \
  }

static inline bool ha_shape_ok(int C, int G, int act, int norm) {
  return C >= 8 && C <= HA_MAXC && (C % 8) == 0 && act >= CATRE_ACT_NONE && act <= CATRE_ACT_MISH &&
         (!norm || (G > 0 && (C % G) == 0));
}
static inline size_t ha_stats_floats(int B, int P, int G) {
  return (size_t)B * ((P + HA_TP - 1) / HA_TP) * G * 2;
}
// statistics of Y -> stat [B][G][2]; part: B * ceil(P/64) * G * 2 floats of scratch
static void ha_stats(const float* Y, float* part, float* stat, int B, int P, int C, int G, hipStream_t st) {
  const int nt = (P + HA_TP - 1) / HA_TP;
  hipLaunchKernelGGL(k_ha_stats_tile, dim3(nt, B), dim3(256), 0, st, Y, part, P, C, G);
  hipLaunchKernelGGL(k_ha_stats_final, dim3(B), dim3(256), 0, st, (const float*)part, stat, P, nt, G, C / G);
}

int catre_op_gnp_act_fwd(const float* Y, const float* gamma, const float* beta, float* A, float* stat, int B, int P, int C,
                         int G, int act, int norm, void* stream) {
  REQUIRE(Y && A && B > 0 && B <= 65535 && P > 0 && ha_shape_ok(C, G, act, norm));
  REQUIRE(!norm || (gamma && beta && stat));
  hipStream_t st = (hipStream_t)stream;
  const int nt = (P + HA_TP - 1) / HA_TP;
  if (norm) {
    // the tile partials borrow the head of A (overwritten by the normalisation pass right after)
    if (ha_stats_floats(B, P, G) > (size_t)B * P * C) return CATRE_ERR_UNSUPPORTED;
    ha_stats(Y, A, stat, B, P, C, G, st);
  }
#define HA_F(ACT, NORM) \
  hipLaunchKernelGGL((k_ha_fwd<ACT, NORM>), dim3(nt, B), dim3(256), 0, st, Y, (const float*)stat, gamma, beta, A, P, C, G)
  HA_SWITCH(act, norm, HA_F)
#undef HA_F
  return check_launch();
}

// floats: sums [B][G][2] | sums_part [S][G][2] | dgb_part [S][2][C] | stage [ceil(S/64)][2][C], S = B * ceil(P/64)
size_t catre_op_gnp_act_bwd_ws_bytes(int B, int P, int C, int G) {
  if (B <= 0 || P <= 0 || C <= 0 || G <= 0) return 0;
  const size_t S = (size_t)B * ((P + HA_TP - 1) / HA_TP);
  return ((size_t)B * G * 2 + S * G * 2 + S * 2 * C + ((S + 63) / 64) * 2 * C) * sizeof(float);
}

int catre_op_gnp_act_bwd(const float* dA, const float* Y, const float* stat, const float* gamma, const float* beta, float* dY,
                         float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, int B, int P, int C, int G,
                         int act, int norm, void* stream) {
  REQUIRE(dA && Y && dY && B > 0 && B <= 65535 && P > 0 && ha_shape_ok(C, G, act, norm));
  REQUIRE(!norm || (stat && gamma && beta && dgamma && dbeta && ws));
  hipStream_t st = (hipStream_t)stream;
  const int nt = (P + HA_TP - 1) / HA_TP;
  float* sums = (float*)ws;
  if (norm) {
    if (ws_bytes < catre_op_gnp_act_bwd_ws_bytes(B, P, C, G)) return CATRE_ERR_WORKSPACE;
    const int S = B * nt, nsp = (S + 63) / 64;
    float* sums_part = sums + (size_t)B * G * 2;
    float* dgb = sums_part + (size_t)S * G * 2;
    float* stage = dgb + (size_t)S * 2 * C;
#define HA_F(ACT) \
  hipLaunchKernelGGL((k_ha_bwd_sums<ACT>), dim3(nt, B), dim3(256), 0, st, dA, Y, stat, gamma, beta, sums_part, dgb, P, C, G)
    HA_SWITCH_ACT(act, HA_F)
#undef HA_F
    hipLaunchKernelGGL(k_ha_bwd_sums_final, dim3((B * G * 2 + 255) / 256), dim3(256), 0, st, (const float*)sums_part, sums, B,
                       nt, G * 2);
    hipLaunchKernelGGL(k_ha_colsum, dim3((2 * C + 255) / 256, nsp), dim3(256), 0, st, (const float*)dgb, stage, S, 2 * C);
    hipLaunchKernelGGL(k_ha_colmerge, dim3((2 * C + 255) / 256), dim3(256), 0, st, (const float*)stage, dgamma, dbeta, nsp, C,
                       accumulate);
  }
#define HA_F(ACT, NORM)                                                                                               \
  hipLaunchKernelGGL((k_ha_bwd_apply<ACT, NORM>), dim3(nt, B), dim3(256), 0, st, dA, Y, stat, (const float*)sums, gamma, \
                     beta, dY, P, C, G)
  HA_SWITCH(act, norm, HA_F)
#undef HA_F
  return check_launch();
}

int catre_op_gnr_act_fwd(const float* Y, const float* gamma, const float* beta, float* A, int R, int C, int G, int act,
                         int norm, void* stream) {
  REQUIRE(Y && A && R > 0 && ha_shape_ok(C, G, act, norm) && (!norm || (gamma && beta)));
  hipStream_t st = (hipStream_t)stream;
#define HA_F(ACT, NORM) hipLaunchKernelGGL((k_har_fwd<ACT, NORM>), dim3(R), dim3(256), 0, st, Y, gamma, beta, A, C, G)
  HA_SWITCH(act, norm, HA_F)
#undef HA_F
  return check_launch();
}

// floats: dgb_part [R][2][C] | stage [ceil(R/64)][2][C]
size_t catre_op_gnr_act_bwd_ws_bytes(int R, int C) {
  if (R <= 0 || C <= 0) return 0;
  return ((size_t)R * 2 * C + ((size_t)(R + 63) / 64) * 2 * C) * sizeof(float);
}

int catre_op_gnr_act_bwd(const float* dA, const float* Y, const float* gamma, const float* beta, float* dY, float* dgamma,
                         float* dbeta, int accumulate, void* ws, size_t ws_bytes, int R, int C, int G, int act, int norm,
                         void* stream) {
  REQUIRE(dA && Y && dY && R > 0 && ha_shape_ok(C, G, act, norm));
  REQUIRE(!norm || (gamma && beta && dgamma && dbeta && ws));
  if (norm && ws_bytes < catre_op_gnr_act_bwd_ws_bytes(R, C)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* dgb = (float*)ws;
#define HA_F(ACT, NORM) hipLaunchKernelGGL((k_har_bwd<ACT, NORM>), dim3(R), dim3(256), 0, st, dA, Y, gamma, beta, dY, dgb, C, G)
  HA_SWITCH(act, norm, HA_F)
#undef HA_F
  if (norm) {
    const int nsp = (R + 63) / 64;
    float* stage = dgb + (size_t)R * 2 * C;
    hipLaunchKernelGGL(k_ha_colsum, dim3((2 * C + 255) / 256, nsp), dim3(256), 0, st, (const float*)dgb, stage, R, 2 * C);
    hipLaunchKernelGGL(k_ha_colmerge, dim3((2 * C + 255) / 256), dim3(256), 0, st, (const float*)stage, dgamma, dbeta, nsp, C,
                       accumulate);
  }
  return check_launch();
}

// floats: statistics partials [B][nt][G][2] | stat [B][G][2] | tile sums [B][nt][3]
size_t catre_op_gnp_act_neck_wsum_ws_bytes(int B, int P, int G) {
  if (B <= 0 || P <= 0 || G < 0) return 0;
  const size_t nt = (P + HA_TP - 1) / HA_TP;
  return ((size_t)B * nt * G * 2 + (size_t)B * G * 2 + (size_t)B * nt * 3) * sizeof(float);
}

int catre_op_gnp_act_neck_wsum(const float* Y, const float* gamma, const float* beta, const float* Wn, const float* bn,
                               const float* wp, const float* bp, float* out, void* ws, size_t ws_bytes, int B, int P, int C,
                               int G, int rot_dim, int act, int norm, void* stream) {
  REQUIRE(Y && Wn && wp && out && ws && B > 0 && B <= 65535 && P > 0 && rot_dim >= 1 && rot_dim <= 3 &&
          ha_shape_ok(C, G, act, norm) && (!norm || (gamma && beta)));
  const int Gs = norm ? G : 0;
  if (ws_bytes < catre_op_gnp_act_neck_wsum_ws_bytes(B, P, Gs)) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nt = (P + HA_TP - 1) / HA_TP;
  float* spart = (float*)ws;
  float* stat = spart + (size_t)B * nt * Gs * 2;
  float* tpart = stat + (size_t)B * Gs * 2;
  if (norm) ha_stats(Y, spart, stat, B, P, C, G, st);
#define HA_F(ACT, NORM)                                                                                                   \
  hipLaunchKernelGGL((k_ha_neck_wsum<ACT, NORM>), dim3(nt, B), dim3(256), 0, st, Y, (const float*)stat, gamma, beta, Wn, wp, \
                     tpart, P, C, G, rot_dim)
  HA_SWITCH(act, norm, HA_F)
#undef HA_F
  hipLaunchKernelGGL(k_ha_wsum_final, dim3(B), dim3(64), 0, st, (const float*)tpart, wp, bn, bp, out, P, nt, rot_dim);
  return check_launch();
}
