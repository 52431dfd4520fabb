// catre_loss_api.inc - C ABI of the training loss of catre_loss.h (included inside extern "C" of catre_extras.hip)
// ---- row f1: training loss ---------------------------------------------------------------------------------
// One implementation behind both generations of entry points: nl loss slots (LOSS_NL: losses[6 + 14], part rows of
// LOSS_NP floats, the L1 / R-only PM term; LOSS_NL2: losses[8 + 14], rows of LOSS_NP2 floats, every PM form).
}  // extern "C"
static catre_loss_cfg2 loss_cfg_shipped_pm(const catre_loss_cfg* cfg) {
  catre_loss_cfg2 c;
  c.base = *cfg;
  c.pm_mode = CATRE_PM_R_ONLY, c.pm_elem = CATRE_PM_ELEM_L1, c.pm_use_bbox = 0, c.pm_beta = 1.f;
  return c;
}
static int loss_fwd_impl(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                         const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                         const int32_t* is_sym, const catre_loss_cfg2& cfg, int32_t* best, int32_t* counts, float* part_ws,
                         float* losses, const float* trans_deltas, const int32_t* terms, int n_terms, float* prefix, int B,
                         int M, int S1, void* stream, int nl, int np, const int32_t* n_obj = nullptr) {
  REQUIRE(pose && scale && gt_rot && gt_trans && gt_scale && is_sym && best && counts && part_ws && losses && B > 0 && S1 > 0);
  REQUIRE(cfg.pm_mode >= 0 && cfg.pm_mode < CATRE_PM_MODE_COUNT && cfg.pm_elem >= 0 && cfg.pm_elem < CATRE_PM_ELEM_COUNT);
  if (cfg.base.pm_on) {
    REQUIRE(cands && valid && M > 0);
    REQUIRE(cfg.pm_use_bbox ? M == 8 : kps != nullptr);
  }
  REQUIRE(n_terms >= 0 && n_terms <= nl && (n_terms == 0 || (terms && prefix)));
  unsigned order = 0;
  for (int k = 0; k < n_terms; ++k) {
    REQUIRE(terms[k] >= 0 && terms[k] < nl);
    order |= (unsigned)terms[k] << (4 * k);
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_loss_fwd, dim3(B), dim3(256), 0, st, pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, valid,
                     is_sym, cfg, best, part_ws, B, M, S1, np);
  hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(512), 0, st, (const float*)part_ws, is_sym, cfg, losses, counts, B, M,
                     pose, gt_trans, trans_deltas, order, n_terms, prefix, np, nl, n_obj);
  return check_launch();
}
static int loss_bwd_impl(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                         const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                         const int32_t* best, const int32_t* counts, const float* upstream, const float* const* up_prefix,
                         const int32_t* terms, int n_terms, const catre_loss_cfg2& cfg, float* dpose, float* dscale, int B,
                         int M, int S1, void* stream, int nl, const int32_t* n_obj = nullptr) {
  REQUIRE(pose && scale && gt_rot && gt_trans && gt_scale && is_sym && best && counts && (upstream || up_prefix) && dpose &&
          dscale && B > 0 && S1 > 0);
  REQUIRE(cfg.pm_mode >= 0 && cfg.pm_mode < CATRE_PM_MODE_COUNT && cfg.pm_elem >= 0 && cfg.pm_elem < CATRE_PM_ELEM_COUNT);
  if (cfg.base.pm_on) {
    REQUIRE(cands && M > 0);
    REQUIRE(cfg.pm_use_bbox ? M == 8 : kps != nullptr);
  }
  REQUIRE(n_terms >= 0 && n_terms <= nl && (!up_prefix || (terms && n_terms > 0)));
  unsigned order = 0;
  LossUpPrefix upp;
  for (int k = 0; k < n_terms; ++k) {
    REQUIRE(terms[k] >= 0 && terms[k] < nl);
    order |= (unsigned)terms[k] << (4 * k);
    if (up_prefix) upp.p[k] = up_prefix[k];
  }
  hipLaunchKernelGGL(k_loss_bwd, dim3(B), dim3(256), 0, (hipStream_t)stream, pose, scale, gt_rot, gt_trans, gt_scale, kps,
                     cands, is_sym, best, upstream, cfg, counts, dpose, dscale, B, M, S1, upp, order, up_prefix ? n_terms : 0,
                     nl, n_obj);
  return check_launch();
}
extern "C" {

int catre_loss_fwd(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                   const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                   const int32_t* is_sym, const catre_loss_cfg* cfg, int32_t* best, int32_t* counts, float* part_ws,
                   float* losses, const float* trans_deltas, int B, int M, int S1, void* stream) {
  return catre_loss_fwd_sums(pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, valid, is_sym, cfg, best, counts, part_ws,
                             losses, trans_deltas, nullptr, 0, nullptr, B, M, S1, stream);
}

// ... plus prefix[k] = ((0 + losses[terms[0]]) + losses[terms[1]]) + ... + losses[terms[k]], k < n_terms <= 6 (terms: host
// array of loss indices in the order the caller's loss dict holds them): every intermediate of `sum(loss_dict.values())`
int catre_loss_fwd_sums(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                        const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                        const int32_t* is_sym, const catre_loss_cfg* cfg, int32_t* best, int32_t* counts, float* part_ws,
                        float* losses, const float* trans_deltas, const int32_t* terms, int n_terms, float* prefix, int B,
                        int M, int S1, void* stream) {
  REQUIRE(cfg);
  return loss_fwd_impl(pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, valid, is_sym, loss_cfg_shipped_pm(cfg), best,
                       counts, part_ws, losses, trans_deltas, terms, n_terms, prefix, B, M, S1, stream, LOSS_NL, LOSS_NP);
}

int catre_loss_bwd(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                   const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                   const int32_t* best, const int32_t* counts, const float* upstream, const catre_loss_cfg* cfg,
                   float* dpose, float* dscale, int B, int M, int S1, void* stream) {
  REQUIRE(upstream);
  return catre_loss_bwd_sums(pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, is_sym, best, counts, upstream, nullptr,
                             nullptr, 0, cfg, dpose, dscale, B, M, S1, stream);
}

// ... with the upstream gradients of the prefix sums of catre_loss_fwd_sums added to those of the six losses (upstream [6]):
// up_prefix = HOST array of n_terms device pointers to one float each (NULL entries = zero); either argument may be NULL
int catre_loss_bwd_sums(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                        const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                        const int32_t* best, const int32_t* counts, const float* upstream,
                        const float* const* up_prefix, const int32_t* terms, int n_terms, const catre_loss_cfg* cfg,
                        float* dpose, float* dscale, int B, int M, int S1, void* stream) {
  REQUIRE(cfg);
  return loss_bwd_impl(pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, is_sym, best, counts, upstream, up_prefix, terms,
                       n_terms, loss_cfg_shipped_pm(cfg), dpose, dscale, B, M, S1, stream, LOSS_NL);
}

// every PM form (catre_loss_cfg2), eight loss slots
int catre_loss_fwd2(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                    const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                    const int32_t* is_sym, const catre_loss_cfg2* cfg, int32_t* best, int32_t* counts, float* part_ws,
                    float* losses, const float* trans_deltas, const int32_t* terms, int n_terms, float* prefix, int B,
                    int M, int S1, void* stream) {
  REQUIRE(cfg);
  return loss_fwd_impl(pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, valid, is_sym, *cfg, best, counts, part_ws, losses,
                       trans_deltas, terms, n_terms, prefix, B, M, S1, stream, LOSS_NL2, LOSS_NP2);
}

int catre_loss_bwd2(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                    const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                    const int32_t* best, const int32_t* counts, const float* upstream, const float* const* up_prefix,
                    const int32_t* terms, int n_terms, const catre_loss_cfg2* cfg, float* dpose, float* dscale, int B,
                    int M, int S1, void* stream) {
  REQUIRE(cfg);
  return loss_bwd_impl(pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, is_sym, best, counts, upstream, up_prefix, terms,
                       n_terms, *cfg, dpose, dscale, B, M, S1, stream, LOSS_NL2);
}

// ... with the object count on the device: B is the capacity the launches are sized for, *n_obj (1 .. B) the objects that count
int catre_loss_fwd3(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                    const float* gt_scale, const float* kps, const float* cands, const unsigned char* valid,
                    const int32_t* is_sym, const catre_loss_cfg2* cfg, int32_t* best, int32_t* counts, float* part_ws,
                    float* losses, const float* trans_deltas, const int32_t* terms, int n_terms, float* prefix, int B,
                    int M, int S1, const int32_t* n_obj, void* stream) {
  REQUIRE(cfg && n_obj);
  return loss_fwd_impl(pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, valid, is_sym, *cfg, best, counts, part_ws, losses,
                       trans_deltas, terms, n_terms, prefix, B, M, S1, stream, LOSS_NL2, LOSS_NP2, n_obj);
}

int catre_loss_bwd3(const float* pose, const float* scale, const float* gt_rot, const float* gt_trans,
                    const float* gt_scale, const float* kps, const float* cands, const int32_t* is_sym,
                    const int32_t* best, const int32_t* counts, const float* upstream, const float* const* up_prefix,
                    const int32_t* terms, int n_terms, const catre_loss_cfg2* cfg, float* dpose, float* dscale, int B,
                    int M, int S1, const int32_t* n_obj, void* stream) {
  REQUIRE(cfg && n_obj);
  return loss_bwd_impl(pose, scale, gt_rot, gt_trans, gt_scale, kps, cands, is_sym, best, counts, upstream, up_prefix, terms,
                       n_terms, *cfg, dpose, dscale, B, M, S1, stream, LOSS_NL2, n_obj);
}
