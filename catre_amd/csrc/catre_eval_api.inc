// catre_eval_api.inc - C ABI of the device evaluator of catre_eval.h (included inside extern "C" of catre_extras.hip)
// ---- evaluation (catre_eval.h): one thread per pair / per (group, threshold); three launches whatever the image count
static inline bool eval_fits(long n) { return n >= 0 && n <= 0x7fffffffL; }

int catre_eval_overlaps(const float* pred_pose, const float* pred_scale, const int32_t* pred_idx, const float* gt_pose,
                        const float* gt_scale, const int32_t* gt_hv, const int32_t* pred_off, const int32_t* gt_off,
                        const int32_t* pair_off, const int32_t* pair_group, const int32_t* group_mode,
                        const double* cos_sin, float* iou, double* degcm, int T, int N, int P, int NG, int G, int Q,
                        void* stream) {
  REQUIRE(T > 0 && G > 0 && N >= 0 && P >= 0 && NG >= 0 && Q >= 0 && P <= N);
  REQUIRE(pred_off && gt_off && pair_off && group_mode && cos_sin);
  REQUIRE(eval_fits((long)T * Q) && eval_fits((long)T * N));
  REQUIRE((long)Q <= (long)P * NG);
  if (Q == 0) return CATRE_OK;
  REQUIRE(pred_pose && pred_scale && pred_idx && gt_pose && gt_scale && gt_hv && pair_group && iou && degcm);
  const long n = (long)T * Q;
  hipLaunchKernelGGL(k_eval_overlaps, dim3((unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0,
                     (hipStream_t)stream, pred_pose, pred_scale, pred_idx, gt_pose, gt_scale, gt_hv, pred_off, gt_off,
                     pair_off, pair_group, group_mode, cos_sin, iou, degcm, T, N, P, NG, G, Q);
  return check_launch();
}

int catre_eval_match_iou(const float* iou, const int32_t* pred_off, const int32_t* gt_off, const int32_t* pair_off,
                         const double* thres, int32_t* pred_match, int32_t* gt_match, int T, int S, int P, int NG, int G,
                         int Q, void* stream) {
  REQUIRE(T > 0 && G > 0 && S > 0 && P >= 0 && NG >= 0 && Q >= 0);
  REQUIRE(pred_off && gt_off && pair_off && thres);
  REQUIRE((iou || Q == 0) && (pred_match || P == 0) && (gt_match || NG == 0));
  REQUIRE(eval_fits((long)T * S * G) && eval_fits((long)T * S * P) && eval_fits((long)T * S * NG) && eval_fits((long)T * Q));
  const long n = (long)T * S * G;
  hipLaunchKernelGGL(k_eval_match_iou, dim3((unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0,
                     (hipStream_t)stream, iou, pred_off, gt_off, pair_off, thres, pred_match, gt_match, T, S, P, NG, G, Q);
  return check_launch();
}

int catre_eval_match_pose(const double* degcm, const int32_t* pred_off, const int32_t* gt_off, const int32_t* pair_off,
                          const int32_t* iou_pred_match, const int32_t* iou_gt_match, int S, int sel,
                          const double* deg_thres, const double* cm_thres, int32_t* pose_pred_match,
                          int32_t* pose_gt_match, int T, int D, int C, int P, int NG, int G, int Q, void* stream) {
  REQUIRE(T > 0 && G > 0 && D > 0 && C > 0 && P >= 0 && NG >= 0 && Q >= 0);
  REQUIRE(pred_off && gt_off && pair_off && deg_thres && cm_thres);
  REQUIRE(sel >= -1 && (sel < 0 || (S > 0 && sel < S)));
  if (sel >= 0) REQUIRE((iou_pred_match || P == 0) && (iou_gt_match || NG == 0));
  REQUIRE((degcm || Q == 0) && (pose_pred_match || P == 0) && (pose_gt_match || NG == 0));
  REQUIRE(eval_fits((long)T * D * C * G) && eval_fits((long)T * D * C * P) && eval_fits((long)T * D * C * NG) &&
          eval_fits((long)T * Q) && (sel < 0 || (eval_fits((long)T * S * P) && eval_fits((long)T * S * NG))));
  const long n = (long)T * D * C * G;
  hipLaunchKernelGGL(k_eval_match_pose, dim3((unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0,
                     (hipStream_t)stream, degcm, pred_off, gt_off, pair_off, iou_pred_match, iou_gt_match, S, sel, deg_thres,
                     cm_thres, pose_pred_match, pose_gt_match, T, D, C, P, NG, G, Q);
  return check_launch();
}
