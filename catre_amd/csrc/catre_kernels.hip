// catre_kernels.hip - the core unit of libcatre_hip.so: the hand-written gfx950 kernels of CATRE's pose-refine hot path in
// every compute mode (the headers below) + their C ABI, the form switches, the weight packing and the profiling hooks.
// The training kernels are catre_train.hip, everything around the refine path catre_extras.hip (see Makefile).
// Reference citations (file:line) are relative to the CATRE tree; see include/catre_hip.h.
#include <algorithm>
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <cstring>
#include <vector>

#include "catre_device.h"

#include "../../include/catre_hip.h"

#define CATRE_VERSION_STR "catre_hip gfx950 r1"

#include "catre_enc.h"
#include "catre_trunkw.h"
#include "catre_fc.h"
#include "catre_rot.h"
#include "catre_pose.h"
#include "catre_bf16.h"
#include "catre_split.h"
#include "catre_screen.h"
#include "catre_gram.h"
#include "catre_small.h"

// ==========================================================================================
// host side: packed-weight and workspace layouts, launchers, C ABI
// ==========================================================================================
#include "catre_host.h"
#include "catre_forms.h"  // the switch table, the form decision, PackLayout and the stages' weight bundles (no HIP in there)
using namespace catre_host;
static_assert(TILE == TP, "catre_forms.h counts tiles of TP points");
unsigned long long* catre_host::g_trunk_trace = nullptr;  // catre_debug_trunk_trace

namespace {

struct WsLayout {
  size_t tspart, xbuf, kbuf, pm, pool, h1, h2, trans3, trans64, gfeat, pointfeat, dt, ds, rot6d, bias0, gn0, gn1, aff0, gn1stat, y1, rpart,
      bar, frun, total;  // offsets in floats
};

WsLayout ws_layout(int B, int N, int M) {
  const size_t TN = (N + TP - 1) / TP, TM = (M + TP - 1) / TP, T = TN + TM;
  const size_t b = B, P = (size_t)N + M;
  WsLayout L;
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += align_up(n, 64);
    return r;
  };
  L.tspart = take(b * 8 * 256);  // first: catre_ts_head finds it without knowing N, M (TS_KS = 8 layer-0 partials)
  L.xbuf = take(b * N * 3);
  L.kbuf = take(b * M * 3);
  L.pm = take((2 * b <= SMALL_ROWS ? 2 : 1) * b * T * PMW);  // small batches: a partial row per HALF tile (k_trunk_h, catre_small.h)
  L.pool = take(2 * b * 1024);
  L.h1 = take(2 * b * 512);
  L.h2 = take(2 * b * 256);
  L.trans3 = take(2 * b * 9);
  L.trans64 = take(2 * b * 4096);
  L.gfeat = take(2 * b * PMW);
  L.pointfeat = take(b * P * 64);
  L.dt = take(b * 3);
  L.ds = take(b * 3);
  L.rot6d = take(b * 6);
  L.bias0 = take(2 * 2 * b * 256);
  L.gn0 = take(b * 2 * T * 64);
  L.gn1 = take(b * 2 * T * 64);
  L.aff0 = take(b * 2 * 2 * 2 * 256);
  L.gn1stat = take(b * 2 * 64);
  {  // y1 [b][2][P][256]; before it is written the region holds the pointfeat moments (catre_gram.h)
    const size_t y1n = b * 2 * P * 256, mom = b * 2 * (4 * (4096 + 64) + 64);  // PF_NG partial moments per cloud
    const size_t y1t = b * 2 * T * 256 * 32;  // bf16 mode: [b][2][T tiles][256 channels][64 points] bf16 (whole tiles)
    L.y1 = take(std::max(std::max(y1n, mom), y1t));
  }
  L.rpart = take(b * 2 * T * 4);
  L.bar = take(64);  // k_fc_tail's barrier counters
  // k_trunk4sr: 1024 running maxima per run; the most runs a grid can have is at run length 2
  L.frun = take(b * ((TN + 1) / 2 + (TM + 1) / 2) * 1024);
  L.total = o;
  return L;
}

inline int n_clouds(int B, int M) { return M > 0 ? 2 * B : B; }
// RS_DISPATCH(rs, L): expands the launch macro L(RS) for the compile-time RS matching rs (row_split, catre_forms.h)
#define RS_DISPATCH(rs, L) \
  switch (rs) {            \
    case 4: L(4); break;   \
    case 2: L(2); break;   \
    default: L(1);         \
  }
// the fp32 encoder kernels also come with eight workgroups per tile (row_split8)
#define RS_DISPATCH8(rs, L) \
  switch (rs) {             \
    case 8: L(8); break;    \
    case 4: L(4); break;    \
    case 2: L(2); break;    \
    default: L(1);          \
  }
// workgroups per object of k_gn0_from_moments (catre_gram.h): its 8 (head, channel block) combinations on 8 / 4 / 2 / 1
inline int gn0_shares(int B) { return B * 8 <= 512 ? 8 : B * 4 <= 512 ? 4 : B * 2 <= 512 ? 2 : 1; }
// workgroups per HALF tile of k_trunk_h (0: too many tiles for it)
inline int trunk_h_split(int tiles) { return tiles * 8 <= 256 ? 4 : tiles * 4 <= 256 ? 2 : tiles * 2 <= 256 ? 1 : 0; }

inline const f32x4* pk4(const float* packed, size_t off) { return reinterpret_cast<const f32x4*>(packed + off); }
inline const u32x4* pkb(const float* packed, size_t off) { return reinterpret_cast<const u32x4*>(packed + off); }

inline TsHeadArgs ts_head_args(const float* l0part, const float* const* prm, const float* packed, const PackLayout& L,
                               float* dt, float* ds, int B) {
  return TsHeadArgs{l0part, prm[CATRE_P_TS_L0_B], prm[CATRE_P_TS_GN0_W], prm[CATRE_P_TS_GN0_B], packed + L.ts_w1t,
                    prm[CATRE_P_TS_L1_B], prm[CATRE_P_TS_GN1_W], prm[CATRE_P_TS_GN1_B], prm[CATRE_P_TS_FCT_W],
                    prm[CATRE_P_TS_FCT_B], prm[CATRE_P_TS_FCS_W], prm[CATRE_P_TS_FCS_B], dt, ds, B};
}

int stn_fc_tail(const float* pooled, const float* const* prm, int base /*CATRE_P_*_FC1_W*/, float* h1, float* h2,
                float* out, int k, int R, hipStream_t st, const float* pm = nullptr, int B = 0, int N = 0, int M = 0,
                unsigned* bar = nullptr) {
  // relu(fc1) -> relu(fc2) -> fc3 + I_k   (pointnet.py:31-40 / 64-77)
  if (bar) {  // small batches: the three layers in ONE launch (k_fc_tail, catre_small.h)
    const int nb3 = (k * k + 31) / 32, grid = nb3 > 16 ? nb3 : 16;
    hipLaunchKernelGGL(k_fc_tail, dim3(grid), dim3(64 * LIN_WAVES), 0, st, pooled, pm, B, N, M, prm[base], prm[base + 1],
                       prm[base + 2], prm[base + 3], prm[base + 4], prm[base + 5], h1, h2, out, k, R, bar);
    return check_launch();
  }
  if (pm)  // small batches (catre_small.h): fc1 pools the tile partials itself, no k_reduce_pm launch in front
    hipLaunchKernelGGL(k_linear_pm, dim3(1, 512 / 32), dim3(64 * LIN_WAVES), 0, st, pm, B, N, M, prm[base], 1024,
                       prm[base + 1], h1, 512, R, 512, 1, nullptr, nullptr, nullptr);
  else
    hipLaunchKernelGGL(k_linear, dim3((R + 31) / 32, 512 / 32), dim3(64 * LIN_WAVES), 0, st, pooled, 1024, prm[base], 1024,
                       prm[base + 1], h1, 512, R, 512, 1024, 1, 0);
  hipLaunchKernelGGL(k_linear, dim3((R + 31) / 32, 256 / 32), dim3(64 * LIN_WAVES), 0, st, h1, 512, prm[base + 2], 512,
                     prm[base + 3], h2, 256, R, 256, 512, 1, 0);
  hipLaunchKernelGGL(k_linear, dim3((R + 31) / 32, (k * k + 31) / 32), dim3(64 * LIN_WAVES), 0, st, h2, 256, prm[base + 4], 256,
                     prm[base + 5], out, k * k, R, k * k, 256, 0, k);
  return check_launch();
}

// ---- opt-in per-kernel timing with HIP events recorded on the launch stream -----------------
// bench.py uses this to measure the dominant kernel's average launch duration inside its timed
// region.  Process-global and not re-entrant by design (a measurement aid, off by default).
struct ProfState {
  int kernel = -1;
  int cap = 0, n = 0;
  hipEvent_t* ev = nullptr;  // 2 per record
};
ProfState g_prof;

static int device_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}
static bool form_on(int id) { return effective_forms(forms()) >> id & 1; }
// the form one launch takes (form_decision of catre_forms.h on this process's switches); CATRE_OK or the status to return
static int decide(int stage, int mode, bool save, bool rows, bool probe, int B, int N, int M, FormDecision* d) {
  if (!form_decision(stage, mode, save, rows, probe, B, N, M, effective_forms(forms()), device_cus(),
                     g_run_len.load(std::memory_order_relaxed), bf_pair_min(), d))
    return CATRE_ERR_BAD_ARG;
  return d->form == CATRE_FORM_UNSUPPORTED ? CATRE_ERR_UNSUPPORTED : CATRE_OK;
}

// The measurement hooks are the library's only process-global mutable state.  They are fenced: compiled out entirely
// with -DCATRE_NO_PROFILING (catre_profile_* then return CATRE_ERR_UNSUPPORTED), off unless catre_profile_enable was
// called, and the record table is guarded by a mutex so that concurrent callers of the data path cannot corrupt it.
#ifndef CATRE_NO_PROFILING
std::mutex g_prof_mu;
struct ProfScope {
  hipStream_t st;
  int slot = -1;
  ProfScope(int kernel_id, hipStream_t s) : st(s) {
    if (g_prof.kernel != kernel_id) return;  // the common case: one relaxed read, no lock
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof.kernel == kernel_id && g_prof.n < g_prof.cap) {
      slot = g_prof.n++;
      (void)hipEventRecord(g_prof.ev[2 * slot], st);
    }
  }
  ~ProfScope() {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (slot < g_prof.cap) (void)hipEventRecord(g_prof.ev[2 * slot + 1], st);
  }
};
#else
struct ProfScope {
  ProfScope(int, hipStream_t) {}
};
#endif

// what every kernel of an encoder stage is handed besides its weights
struct EncCall {
  const catre_points* pts;
  const float *trans3, *trans64;  // STNkd: trans3; trunk: both
  float* pm;                      // tile partial maxima (ws + W.pm)
  int B, N, M;
  hipStream_t st;
};
// the positional arguments every kernel form of a stage starts with: call c, weight bundle w (catre_forms.h)
#define STN3D_ARGS(c, w) *(c).pts, (w).w1, (w).b1, (w).w2, (w).b2, (w).w3, (w).b3, (c).pm, (c).B, (c).N, (c).M
#define STNKD_ARGS(c, w) \
  *(c).pts, (c).trans3, (w).wc1, (w).bc1, (w).w1, (w).b1, (w).w2, (w).b2, (w).w3, (w).b3, (c).pm, (c).B, (c).N, (c).M
#define TRUNK_ARGS(c, w, pointfeat)                                                                                        \
  *(c).pts, (c).trans3, (c).trans64, (w).w1, (w).b1, (w).w2, (w).b2, (w).w3, (w).b3, (w).w4, (w).b4, (c).pm, pointfeat, (c).B, \
      (c).N, (c).M
inline bool f16_screen(const FormDecision& d) { return d.form == CATRE_FORM_RUN_F16 || d.form == CATRE_FORM_SCREEN_F16; }

// The three encoder kernels of one iteration (fp32 or split compute), tile partial maxima -> c.pm.  The probes
// (catre_*_screen_probe) get CATRE_ERR_UNSUPPORTED where the grid takes no screened form.
int launch_stn3d(const EncCall& c, const float* const* prm, const float* packed, bool split, unsigned* zero_bar = nullptr,
                 float* probe_s = nullptr, float* probe_eps = nullptr, float* probe_rows = nullptr) {
  FormDecision d;
  if (const int rc = decide(STAGE_STN3D, split ? MODE_SPLIT : MODE_F32, false, false, probe_s != nullptr, c.B, c.N, c.M, &d)) return rc;
  const Stn3dW w = stn3d_weights(prm, packed, pack_layout(1), split ? PK_SPLIT : PK_F32, f16_screen(d));  // conv offsets do not depend on ts_in
  const ScreenArgs sc{w.sc.wps, w.sc.nw, probe_s, probe_eps, w.sc.uw, screen_da_stn()};
  const Stn3dRunArgs run{*c.pts, w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, c.pm, w.sc.wps, w.sc.nw, c.B, c.N, c.M, d.S, w.sc.uw, sc.da};
  const dim3 grid(d.grid), block(256);
  ProfScope ps(CATRE_K_STN3D, c.st);
  switch (d.form) {
    case CATRE_FORM_SPLIT_RS:
#define LAUNCH_(RS) hipLaunchKernelGGL(k_stn3d_split<RS>, grid, block, 0, c.st, STN3D_ARGS(c, w))
      RS_DISPATCH(d.row_split, LAUNCH_)
#undef LAUNCH_
      break;
    case CATRE_FORM_RUN_F16:
      if (screen_epi())
        hipLaunchKernelGGL(k_stn3d_pair_sr16e, grid, block, 0, c.st, run);
      else
        hipLaunchKernelGGL(k_stn3d_pair_sr16, grid, block, 0, c.st, run);
      break;
    case CATRE_FORM_RUN: hipLaunchKernelGGL(k_stn3d_pair_sr, grid, block, 0, c.st, run); break;
    case CATRE_FORM_SCREEN_F16:  // (a probe keeps the kernel that carries the probe code)
      if (screen_epi() && !probe_s)
        hipLaunchKernelGGL(k_stn3d_pair_sp16e, grid, block, 0, c.st, STN3D_ARGS(c, w), sc, probe_rows);
      else
        hipLaunchKernelGGL(k_stn3d_pair_sp16, grid, block, 0, c.st, STN3D_ARGS(c, w), sc, probe_rows);
      break;
    case CATRE_FORM_SCREEN_POOL: hipLaunchKernelGGL(k_stn3d_pair_sp, grid, block, 0, c.st, STN3D_ARGS(c, w), sc, probe_rows); break;
    case CATRE_FORM_SCREEN: hipLaunchKernelGGL(k_stn3d_pair_s, grid, block, 0, c.st, STN3D_ARGS(c, w), sc, probe_rows); break;
    case CATRE_FORM_PAIR: hipLaunchKernelGGL(k_stn3d_pair<false>, grid, block, 0, c.st, STN3D_ARGS(c, w)); break;
    case CATRE_FORM_WAVE4:
      hipLaunchKernelGGL((k_stn3d<1, false, true>), grid, block, 0, c.st, STN3D_ARGS(c, w), TrainSave{}, zero_bar);
      break;
    default:  // CATRE_FORM_RS8
#define LAUNCH_(RS) hipLaunchKernelGGL(k_stn3d<RS>, grid, block, 0, c.st, STN3D_ARGS(c, w), TrainSave{}, zero_bar)
      RS_DISPATCH8(d.row_split, LAUNCH_)
#undef LAUNCH_
  }
  return CATRE_OK;
}

int launch_stnkd(const EncCall& c, const float* const* prm, const float* packed, bool split, unsigned* zero_bar = nullptr,
                 float* probe_s = nullptr, float* probe_eps = nullptr, float* probe_rows = nullptr) {
  FormDecision d;
  if (const int rc = decide(STAGE_STNKD, split ? MODE_SPLIT : MODE_F32, false, false, probe_s != nullptr, c.B, c.N, c.M, &d)) return rc;
  const StnkdW w = stnkd_weights(prm, packed, pack_layout(1), split ? PK_SPLIT : PK_F32, f16_screen(d));
  const ScreenArgs sc{w.sc.wps, w.sc.nw, probe_s, probe_eps, w.sc.uw, screen_da_stn()};
  const StnkdRunArgs run{*c.pts, c.trans3, w.wc1, w.bc1, w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, c.pm, w.sc.wps, w.sc.nw,
                         c.B, c.N, c.M, d.S, w.sc.uw, sc.da};
  const dim3 grid(d.grid), block(256);
  ProfScope ps(CATRE_K_STNKD, c.st);
  switch (d.form) {
    case CATRE_FORM_SPLIT_RS:
#define LAUNCH_(RS) hipLaunchKernelGGL(k_stnkd_split<RS>, grid, block, 0, c.st, STNKD_ARGS(c, w))
      RS_DISPATCH(d.row_split, LAUNCH_)
#undef LAUNCH_
      break;
    case CATRE_FORM_RUN_F16:
      if (screen_epi())
        hipLaunchKernelGGL(k_stnkd_pair_sr16e, grid, block, 0, c.st, run);
      else
        hipLaunchKernelGGL(k_stnkd_pair_sr16, grid, block, 0, c.st, run);
      break;
    case CATRE_FORM_RUN: hipLaunchKernelGGL(k_stnkd_pair_sr, grid, block, 0, c.st, run); break;
    case CATRE_FORM_SCREEN_F16:
      if (screen_epi() && !probe_s)
        hipLaunchKernelGGL(k_stnkd_pair_sp16e, grid, block, 0, c.st, STNKD_ARGS(c, w), sc, probe_rows);
      else
        hipLaunchKernelGGL(k_stnkd_pair_sp16, grid, block, 0, c.st, STNKD_ARGS(c, w), sc, probe_rows);
      break;
    case CATRE_FORM_SCREEN_POOL: hipLaunchKernelGGL(k_stnkd_pair_sp, grid, block, 0, c.st, STNKD_ARGS(c, w), sc, probe_rows); break;
    case CATRE_FORM_SCREEN: hipLaunchKernelGGL(k_stnkd_pair_s, grid, block, 0, c.st, STNKD_ARGS(c, w), sc, probe_rows); break;
    case CATRE_FORM_PAIR: hipLaunchKernelGGL(k_stnkd_pair<false>, grid, block, 0, c.st, STNKD_ARGS(c, w)); break;
    case CATRE_FORM_WAVE4:
      hipLaunchKernelGGL((k_stnkd<1, false, true>), grid, block, 0, c.st, STNKD_ARGS(c, w), TrainSave{}, zero_bar);
      break;
    default:  // CATRE_FORM_RS8
#define LAUNCH_(RS) hipLaunchKernelGGL(k_stnkd<RS>, grid, block, 0, c.st, STNKD_ARGS(c, w), TrainSave{}, zero_bar)
      RS_DISPATCH8(d.row_split, LAUNCH_)
#undef LAUNCH_
  }
  return CATRE_OK;
}

int launch_trunk(const EncCall& c, const float* const* prm, const float* packed, float* pointfeat, float* frun, bool split,
                 float* probe_s = nullptr, float* probe_eps = nullptr) {
  FormDecision d;
  if (const int rc = decide(STAGE_TRUNK, split ? MODE_SPLIT : MODE_F32, false, false, probe_s != nullptr, c.B, c.N, c.M, &d)) return rc;
  const TrunkW w = trunk_weights(prm, packed, pack_layout(1), split ? PK_SPLIT : PK_F32, f16_screen(d));
  const ScreenArgs sc{w.sc.wps, w.sc.nw, probe_s, probe_eps, w.sc.uw, screen_da()};
  const TrunkRunArgs run{*c.pts, c.trans3, c.trans64, w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, w.w4, w.b4, c.pm, pointfeat,
                         g_trunk_trace, sc, frun, c.B, c.N, c.M, d.S};
  const dim3 grid(d.grid);
  ProfScope ps(CATRE_K_TRUNK, c.st);
  switch (d.form) {
    case CATRE_FORM_SPLIT_RS:
#define LAUNCH_(RS) hipLaunchKernelGGL(k_trunk_split<RS>, grid, dim3(512), 0, c.st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace)
      RS_DISPATCH(d.row_split, LAUNCH_)
#undef LAUNCH_
      break;
    case CATRE_FORM_RUN_F16:
      // `screen_epi`: the lean kernels carry no probe code; a probe takes the one-tile kernel of the same screen arithmetic
      // (S and eps are functions of the tile alone, and the cloud maxima of the tile maxima are the run form's)
      if (screen_epi() && probe_s)
        hipLaunchKernelGGL(k_trunk4sp16, dim3(c.B * (tiles_of(c.N) + tiles_of(c.M))), dim3(256), 0, c.st, TRUNK_ARGS(c, w, pointfeat),
                           g_trunk_trace, sc);
      else if (screen_epi())
        hipLaunchKernelGGL(k_trunk4sr16e, grid, dim3(256), 0, c.st, run);
      else
        hipLaunchKernelGGL(k_trunk4sr16, grid, dim3(256), 0, c.st, run);
      break;
    case CATRE_FORM_RUN: hipLaunchKernelGGL(k_trunk4sr, grid, dim3(256), 0, c.st, run); break;
    case CATRE_FORM_SCREEN_F16:
      if (screen_epi() && !probe_s)
        hipLaunchKernelGGL(k_trunk4sp16e, grid, dim3(256), 0, c.st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace, sc);
      else
        hipLaunchKernelGGL(k_trunk4sp16, grid, dim3(256), 0, c.st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace, sc);
      break;
    case CATRE_FORM_SCREEN_POOL:
      hipLaunchKernelGGL(k_trunk4sp, grid, dim3(256), 0, c.st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace, sc);
      break;
    case CATRE_FORM_SCREEN: hipLaunchKernelGGL(k_trunk4s, grid, dim3(256), 0, c.st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace, sc); break;
    case CATRE_FORM_WAVE4: hipLaunchKernelGGL(k_trunk4<false>, grid, dim3(256), 0, c.st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace); break;
    default:  // CATRE_FORM_RS8
#define LAUNCH_(RS) hipLaunchKernelGGL(k_trunk<RS>, grid, dim3(512), 0, c.st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace)
      RS_DISPATCH8(d.row_split, LAUNCH_)
#undef LAUNCH_
  }
  return CATRE_OK;
}

}  // namespace

extern "C" {

const char* catre_version(void) { return CATRE_VERSION_STR; }

const char* catre_status_string(int s) {
  switch (s) {
    case CATRE_OK: return "ok";
    case CATRE_ERR_BAD_ARG: return "bad argument";
    case CATRE_ERR_WORKSPACE: return "workspace or packed-weight buffer too small";
    case CATRE_ERR_LAUNCH: return "kernel launch failed";
    case CATRE_ERR_UNSUPPORTED: return "unsupported configuration";
    default: return "unknown status";
  }
}

size_t catre_workspace_bytes(int B, int N, int M) {
  if (!dims_ok1(B, N, M)) return 0;
  return ws_layout(B, N, M).total * sizeof(float);
}

size_t catre_packed_floats(int N, int M, int ts_in_dim) {
  if (N <= 0 || M <= 0 || ts_in_dim <= 0) return 0;
  return pack_layout(ts_in_dim).total;
}

int catre_pack_weights(const float* const* prm, int N, int M, int ts_in, float* packed, size_t packed_floats,
                       void* stream) {
  return catre_pack_weights_sel(prm, N, M, ts_in, packed, packed_floats, CATRE_PACK_ALL, stream);
}

int catre_pack_weights_sel(const float* const* prm, int N, int M, int ts_in, float* packed, size_t packed_floats, int sel,
                           void* stream) {
  REQUIRE(prm && packed && N > 0 && M > 0 && ts_in > 0);
  const PackLayout L = pack_layout(ts_in);
  if (packed_floats < L.total) return CATRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  // a NULL source is skipped, so a sub-module (e.g. PointNetfeat alone) can pack just its own layers
  const bool enc32 = sel & CATRE_PACK_F32_ENCODER, head32 = sel & CATRE_PACK_F32_HEADS, bf = sel & CATRE_PACK_BF16,
             sp = sel & CATRE_PACK_SPLIT, tails = sel & CATRE_PACK_F32_TAILS, hf = sel & CATRE_PACK_F16;
  PackJobs jobs;
  jobs.n = 0;
  auto flush = [&]() {
    if (jobs.n) hipLaunchKernelGGL(k_pack_frag_multi, dim3((jobs.end[jobs.n - 1] + 255) / 256), dim3(256), 0, st, jobs);
    jobs.n = 0;
  };
  auto frag = [&](const float* src, int ld, int coloff, int rows, int K, size_t off) {  // queued: one launch for all
    if (!src) return;
    if (jobs.n == PACK_MAX_JOBS) flush();
    const int j = jobs.n++;
    jobs.src[j] = src;
    jobs.dst[j] = packed + off;
    jobs.ld[j] = ld;
    jobs.coloff[j] = coloff;
    jobs.K[j] = K;
    jobs.end[j] = (j ? jobs.end[j - 1] : 0) + rows * K;
  };
  PackJobs lpjobs;   // the bf16 / split / fp16 packs: queued like the fp32 ones, one launch per kind
  lpjobs.n = 0;
  enum { LP_BF16, LP_SPLIT, LP_F16 };
  auto flush_lp = [&](int kind) {
    if (lpjobs.n) {
      const dim3 grid((lpjobs.end[lpjobs.n - 1] + 255) / 256);
      if (kind == LP_SPLIT)
        hipLaunchKernelGGL(k_pack_frag_lp_multi<true>, grid, dim3(256), 0, st, lpjobs);
      else if (kind == LP_F16)
        hipLaunchKernelGGL(k_pack_frag_hf_multi, grid, dim3(256), 0, st, lpjobs);
      else
        hipLaunchKernelGGL(k_pack_frag_lp_multi<false>, grid, dim3(256), 0, st, lpjobs);
    }
    lpjobs.n = 0;
  };
  auto frag_lp = [&](int kind, const float* src, int ld, int coloff, int rows, int K, size_t off) {
    if (!src) return;
    if (lpjobs.n == PACK_MAX_JOBS) flush_lp(kind);
    const int j = lpjobs.n++;
    lpjobs.src[j] = src;
    lpjobs.dst[j] = packed + off;
    lpjobs.ld[j] = ld;
    lpjobs.coloff[j] = coloff;
    lpjobs.K[j] = K;
    lpjobs.end[j] = (j ? lpjobs.end[j - 1] : 0) + rows * K;
  };
  auto frag_bf = [&](const float* src, int ld, int coloff, int rows, int K, size_t off) {
    frag_lp(LP_BF16, src, ld, coloff, rows, K, off);
  };
  if (bf) {
  frag_bf(prm[CATRE_P_STN_CONV2_W], 64, 0, 128, 64, L.bf_stn_c2);
  frag_bf(prm[CATRE_P_STN_CONV3_W], 128, 0, 1024, 128, L.bf_stn_c3);
  frag_bf(prm[CATRE_P_FSTN_CONV1_W], 64, 0, 64, 64, L.bf_fstn_c1);
  frag_bf(prm[CATRE_P_FSTN_CONV2_W], 64, 0, 128, 64, L.bf_fstn_c2);
  frag_bf(prm[CATRE_P_FSTN_CONV3_W], 128, 0, 1024, 128, L.bf_fstn_c3);
  frag_bf(prm[CATRE_P_CONV2_W], 64, 0, 128, 64, L.bf_c2);
  frag_bf(prm[CATRE_P_CONV3_W], 128, 0, 512, 128, L.bf_c3);
  frag_bf(prm[CATRE_P_CONV4_W], 512, 0, 1024, 512, L.bf_c4);
  for (int h = 0; h < 2; ++h) {
    const int base = h ? CATRE_P_ROTY_L0_W : CATRE_P_ROTX_L0_W;
    frag_bf(prm[base], PMW, 1024, 256, 64, L.bf_rot_l0[h]);
    frag_bf(prm[base + 4], 256, 0, 256, 256, L.bf_rot_l1[h]);
  }
  flush_lp(LP_BF16);
  }
  if (hf) {  // the same matrices as the bf16 packs, as fp16
    auto frag_hf = [&](const float* src, int ld, int coloff, int rows, int K, size_t off) {
      frag_lp(LP_F16, src, ld, coloff, rows, K, off);
    };
    frag_hf(prm[CATRE_P_STN_CONV2_W], 64, 0, 128, 64, L.f16_stn_c2);
    frag_hf(prm[CATRE_P_STN_CONV3_W], 128, 0, 1024, 128, L.f16_stn_c3);
    frag_hf(prm[CATRE_P_FSTN_CONV1_W], 64, 0, 64, 64, L.f16_fstn_c1);
    frag_hf(prm[CATRE_P_FSTN_CONV2_W], 64, 0, 128, 64, L.f16_fstn_c2);
    frag_hf(prm[CATRE_P_FSTN_CONV3_W], 128, 0, 1024, 128, L.f16_fstn_c3);
    frag_hf(prm[CATRE_P_CONV2_W], 64, 0, 128, 64, L.f16_c2);
    frag_hf(prm[CATRE_P_CONV3_W], 128, 0, 512, 128, L.f16_c3);
    frag_hf(prm[CATRE_P_CONV4_W], 512, 0, 1024, 512, L.f16_c4);
    for (int h = 0; h < 2; ++h) {
      const int base = h ? CATRE_P_ROTY_L0_W : CATRE_P_ROTX_L0_W;
      frag_hf(prm[base], PMW, 1024, 256, 64, L.f16_rot_l0[h]);
      frag_hf(prm[base + 4], 256, 0, 256, 256, L.f16_rot_l1[h]);
    }
    flush_lp(LP_F16);
  }
  auto frag_sp = [&](const float* src, int ld, int rows, int K, size_t off, int coloff = 0) {
    frag_lp(LP_SPLIT, src, ld, coloff, rows, K, off);
  };
  if (sp) {
  frag_sp(prm[CATRE_P_STN_CONV2_W], 64, 128, 64, L.sp_stn_c2);
  frag_sp(prm[CATRE_P_STN_CONV3_W], 128, 1024, 128, L.sp_stn_c3);
  frag_sp(prm[CATRE_P_FSTN_CONV1_W], 64, 64, 64, L.sp_fstn_c1);
  frag_sp(prm[CATRE_P_FSTN_CONV2_W], 64, 128, 64, L.sp_fstn_c2);
  frag_sp(prm[CATRE_P_FSTN_CONV3_W], 128, 1024, 128, L.sp_fstn_c3);
  frag_sp(prm[CATRE_P_CONV3_W], 128, 512, 128, L.sp_c3);
  frag_sp(prm[CATRE_P_CONV4_W], 512, 1024, 512, L.sp_c4);
  frag_sp(prm[CATRE_P_ROTX_L0_W], PMW, 256, 64, L.sp_rot_l0[0], 1024);
  frag_sp(prm[CATRE_P_ROTY_L0_W], PMW, 256, 64, L.sp_rot_l0[1], 1024);
  frag_sp(prm[CATRE_P_ROTX_L0_W + 4], 256, 256, 256, L.sp_rot_l1[0]);
  frag_sp(prm[CATRE_P_ROTY_L0_W + 4], 256, 256, 256, L.sp_rot_l1[1]);
  flush_lp(LP_SPLIT);
  }
  if (enc32) {
  frag(prm[CATRE_P_STN_CONV2_W], 64, 0, 128, 64, L.stn_c2);
  frag(prm[CATRE_P_STN_CONV3_W], 128, 0, 1024, 128, L.stn_c3);
  frag(prm[CATRE_P_FSTN_CONV1_W], 64, 0, 64, 64, L.fstn_c1);
  frag(prm[CATRE_P_FSTN_CONV2_W], 64, 0, 128, 64, L.fstn_c2);
  frag(prm[CATRE_P_FSTN_CONV3_W], 128, 0, 1024, 128, L.fstn_c3);
  frag(prm[CATRE_P_CONV2_W], 64, 0, 128, 64, L.c2);
  frag(prm[CATRE_P_CONV3_W], 128, 0, 512, 128, L.c3);
  frag(prm[CATRE_P_CONV4_W], 512, 0, 1024, 512, L.c4);
  if (prm[CATRE_P_CONV4_W]) {  // the screen's operands of conv4 (k_trunk4s)
    frag_sp(prm[CATRE_P_CONV4_W], 512, 1024, 512, L.scr_c4);
    flush_lp(LP_SPLIT);
    hipLaunchKernelGGL(k_screen_wnorm, dim3(1024 / 4), dim3(256), 0, st, prm[CATRE_P_CONV4_W], 512, 1024, 512,
                       packed + L.scr_nw4);
    hipLaunchKernelGGL(k_pack_screen_f16, dim3(1024 * 512 / 256), dim3(256), 0, st, prm[CATRE_P_CONV4_W], 512, 1024, 512,
                       packed + L.scr_nw4, reinterpret_cast<unsigned short*>(packed + L.s16_c4), packed + L.s16_uw4);
    hipLaunchKernelGGL(k_screen_f16_dw, dim3(1024 / 4), dim3(256), 0, st, prm[CATRE_P_CONV4_W], 512, 1024, 512,
                       packed + L.scr_nw4, packed + L.s16_uw4 + 1024, packed + L.s16_uw4 + 2048);
  }
  // the same of the two STNs' conv3 (k_stn3d_pair_s / k_stnkd_pair_s)
  frag_sp(prm[CATRE_P_STN_CONV3_W], 128, 1024, 128, L.scr_stn_c3);
  frag_sp(prm[CATRE_P_FSTN_CONV3_W], 128, 1024, 128, L.scr_fstn_c3);
  flush_lp(LP_SPLIT);
  if (prm[CATRE_P_STN_CONV3_W]) {
    hipLaunchKernelGGL(k_screen_wnorm, dim3(1024 / 4), dim3(256), 0, st, prm[CATRE_P_STN_CONV3_W], 128, 1024, 128,
                       packed + L.scr_nw_stn);
    hipLaunchKernelGGL(k_pack_screen_f16, dim3(1024 * 128 / 256), dim3(256), 0, st, prm[CATRE_P_STN_CONV3_W], 128, 1024, 128,
                       packed + L.scr_nw_stn, reinterpret_cast<unsigned short*>(packed + L.s16_stn_c3), packed + L.s16_uw_stn);
    hipLaunchKernelGGL(k_screen_f16_dw, dim3(1024 / 4), dim3(256), 0, st, prm[CATRE_P_STN_CONV3_W], 128, 1024, 128,
                       packed + L.scr_nw_stn, packed + L.s16_uw_stn + 1024, packed + L.s16_uw_stn + 2048);
  }
  if (prm[CATRE_P_FSTN_CONV3_W]) {
    hipLaunchKernelGGL(k_screen_wnorm, dim3(1024 / 4), dim3(256), 0, st, prm[CATRE_P_FSTN_CONV3_W], 128, 1024, 128,
                       packed + L.scr_nw_fstn);
    hipLaunchKernelGGL(k_pack_screen_f16, dim3(1024 * 128 / 256), dim3(256), 0, st, prm[CATRE_P_FSTN_CONV3_W], 128, 1024, 128,
                       packed + L.scr_nw_fstn, reinterpret_cast<unsigned short*>(packed + L.s16_fstn_c3),
                       packed + L.s16_uw_fstn);
    hipLaunchKernelGGL(k_screen_f16_dw, dim3(1024 / 4), dim3(256), 0, st, prm[CATRE_P_FSTN_CONV3_W], 128, 1024, 128,
                       packed + L.scr_nw_fstn, packed + L.s16_uw_fstn + 1024, packed + L.s16_uw_fstn + 2048);
  }
  }
  for (int h = 0; h < 2 && head32; ++h) {
    const int base = h ? CATRE_P_ROTY_L0_W : CATRE_P_ROTX_L0_W;
    frag(prm[base], PMW, 1024, 256, 64, L.rot_l0[h]);  // W0[:, 1024:1088]
    frag(prm[base + 4], 256, 0, 256, 256, L.rot_l1[h]);
    if (prm[base + 10] && tails)
      hipLaunchKernelGGL(k_sum, dim3(1), dim3(256), 0, st, prm[base + 10], N + M, packed + L.sumwp + h);
  }
  flush();
  if (head32 && tails && prm[CATRE_P_TS_L0_W] && prm[CATRE_P_TS_L1_W]) {
    int n = ts_in * 256;
    hipLaunchKernelGGL(k_pack_transpose, dim3((n + 255) / 256), dim3(256), 0, st, prm[CATRE_P_TS_L0_W], 256, ts_in,
                       packed + L.ts_w0t);
    n = 256 * 256;
    hipLaunchKernelGGL(k_pack_transpose, dim3((n + 255) / 256), dim3(256), 0, st, prm[CATRE_P_TS_L1_W], 256, 256,
                       packed + L.ts_w1t);
  }
  return check_launch();
}

int catre_pose_apply(const float* pcl, const float* kps, const float* pose, const float* scale, float* x_out,
                     float* kps_out, int B, int N, int M, int zero_center, void* stream) {
  REQUIRE(pcl && kps && pose && scale && x_out && kps_out && dims_ok(B, N, M));
  const int total = B * (N + M);
  hipLaunchKernelGGL(k_pose_apply, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, pcl, kps, pose, scale,
                     x_out, kps_out, B, N, M, zero_center);
  return check_launch();
}

int catre_stn3d_pool(const catre_points* pts, const float* const* prm, const float* packed, float* pooled,
                     void* workspace, size_t ws_bytes, int B, int N, int M, void* stream) {
  REQUIRE(pts && prm && packed && pooled && workspace && dims_ok1(B, N, M));
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_stn3d(EncCall{pts, nullptr, nullptr, ws + W.pm, B, N, M, st}, prm, packed, false)) return rc;
  hipLaunchKernelGGL(k_reduce_pm, dim3(n_clouds(B, M), (1024 + 255) / 256), dim3(256), 0, st, ws + W.pm, pooled, 1024, 1024, B, N, M);
  return check_launch();
}

int catre_linear(const float* x, int ldx, const float* Wt, int ldw, const float* bias, float* y, int ldy, int R, int J,
                 int K, int relu, int add_identity_k, void* stream) {
  REQUIRE(x && Wt && y && R > 0 && J > 0 && K > 0 && (K % 8) == 0 && (ldx % 4) == 0 && (ldw % 4) == 0);
  hipLaunchKernelGGL(k_linear, dim3((R + 31) / 32, (J + 31) / 32), dim3(64 * LIN_WAVES), 0, (hipStream_t)stream, x, ldx, Wt, ldw,
                     bias, y, ldy, R, J, K, relu, add_identity_k);
  return check_launch();
}

// y[R,J] = x[R,K] W for W [K][J] row-major (ldw): the data gradient of a small linear from its own weight, no transposed copy
// xmask (optional, [R,K] with x's row pitch): x .* (xmask > 0) replaces x - the ReLU backward of the layer's output
int catre_linear_t(const float* x, int ldx, const float* xmask, const float* W, int ldw, float* y, int ldy, int R, int J,
                   int K, void* stream) {
  REQUIRE(x && W && y && R > 0 && J > 0 && K > 0 && (K % 8) == 0 && (ldx % 4) == 0 && ldw >= J);
  hipLaunchKernelGGL(k_linear_t, dim3((R + 31) / 32, (J + 31) / 32), dim3(64 * LIN_WAVES), 0, (hipStream_t)stream, x, ldx, W,
                     ldw, y, ldy, R, J, K, xmask);
  return check_launch();
}

int catre_stnkd_pool(const catre_points* pts, const float* trans3, const float* const* prm, const float* packed,
                     float* pooled, void* workspace, size_t ws_bytes, int B, int N, int M, void* stream) {
  REQUIRE(pts && trans3 && prm && packed && pooled && workspace && dims_ok1(B, N, M));
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_stnkd(EncCall{pts, trans3, nullptr, ws + W.pm, B, N, M, st}, prm, packed, false)) return rc;
  hipLaunchKernelGGL(k_reduce_pm, dim3(n_clouds(B, M), (1024 + 255) / 256), dim3(256), 0, st, ws + W.pm, pooled, 1024, 1024, B, N, M);
  return check_launch();
}

int catre_trunk(const catre_points* pts, const float* trans3, const float* trans64, const float* const* prm,
                const float* packed, float* gfeat, float* pointfeat, void* workspace, size_t ws_bytes, int B, int N,
                int M, void* stream) {
  REQUIRE(pts && trans3 && prm && packed && gfeat && pointfeat && workspace && dims_ok1(B, N, M));
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_trunk(EncCall{pts, trans3, trans64, ws + W.pm, B, N, M, st}, prm, packed, pointfeat, ws + W.frun, false))
    return rc;
  hipLaunchKernelGGL(k_reduce_pm, dim3(n_clouds(B, M), (PMW + 255) / 256), dim3(256), 0, st, ws + W.pm, gfeat, PMW, PMW, B, N, M);
  return check_launch();
}

// ---- the encoder at conv4 width out_dim (catre_trunkw.h) --------------------------------------------------------------
// image: [the layout of catre_pack_weights for ts_in = 1 - the STN entry points read their packs at its offsets; its conv4
// slots stay unwritten][conv4 as out_dim rows of fp32 fragments]
static bool out_dim_ok(int d) { return d == 64 || d == 128 || d == 256 || d == 512 || d == 1024; }

size_t catre_packed_floats_w(int out_dim) {
  if (!out_dim_ok(out_dim)) return 0;
  return pack_layout(1).total + (size_t)out_dim * 512;
}

int catre_pack_encoder_w(const float* const* prm, int out_dim, float* packed, size_t packed_floats, void* stream) {
  REQUIRE(prm && packed);
  if (!out_dim_ok(out_dim)) return CATRE_ERR_UNSUPPORTED;
  REQUIRE(prm[CATRE_P_CONV4_W]);
  const size_t base = pack_layout(1).total;
  if (packed_floats < base + (size_t)out_dim * 512) return CATRE_ERR_WORKSPACE;
  const float* enc[CATRE_P_COUNT];
  for (int i = 0; i < CATRE_P_COUNT; ++i) enc[i] = prm[i];
  enc[CATRE_P_CONV4_W] = nullptr;  // skipped there: catre_pack_weights_sel reads conv4 as [1024,512]
  const int s = catre_pack_weights_sel(enc, 1, 1, 1, packed, packed_floats, CATRE_PACK_F32_ENCODER, stream);
  if (s != CATRE_OK) return s;
  const int n = out_dim * 512;
  hipLaunchKernelGGL(k_pack_frag, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, prm[CATRE_P_CONV4_W], 512, 0,
                     out_dim, 512, packed + base);
  return check_launch();
}

int catre_trunk_w(const catre_points* pts, const float* trans3, const float* trans64, const float* const* prm,
                  const float* packed, int out_dim, float* gfeat, float* pointfeat, void* workspace, size_t ws_bytes, int B,
                  int N, int M, void* stream) {
  REQUIRE(pts && trans3 && prm && packed && gfeat && pointfeat && workspace && dims_ok1(B, N, M));
  if (!out_dim_ok(out_dim)) return CATRE_ERR_UNSUPPORTED;
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const PackLayout L = pack_layout(1);
  const int tiles = B * ((N + TP - 1) / TP + (M + TP - 1) / TP);
  const TrunkW w = trunk_weights(prm, packed, L, PK_F32);  // conv4: the out_dim rows behind the layout
#define LAUNCH_(MB, NB)                                                                                                   \
  hipLaunchKernelGGL((k_trunkw<MB, NB>), dim3(tiles), dim3(512), 0, st, *pts, trans3, trans64, w.w1, w.b1, w.w2, w.b2, w.w3, \
                     w.b3, pk4(packed, L.total), w.b4, out_dim / 32, ws + W.pm, pointfeat, B, N, M)
  switch (out_dim) {
    case 1024: LAUNCH_(4, 2); break;
    case 512: LAUNCH_(2, 2); break;
    case 256: LAUNCH_(1, 2); break;
    default: LAUNCH_(1, 1);  // 128, 64
  }
#undef LAUNCH_
  hipLaunchKernelGGL(k_reduce_pm_w, dim3(n_clouds(B, M), (out_dim + 64 + 255) / 256), dim3(256), 0, st, ws + W.pm, gfeat,
                     out_dim, B, N, M);
  return check_launch();
}

int catre_trunk_screen_probe(const catre_points* pts, const float* trans3, const float* trans64, const float* const* prm,
                             const float* packed, float* screen, float* eps, float* gfeat, float* pointfeat, void* workspace,
                             size_t ws_bytes, int B, int N, int M, void* stream) {
  REQUIRE(pts && trans3 && prm && packed && screen && eps && gfeat && pointfeat && workspace && dims_ok1(B, N, M));
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  // (CATRE_ERR_UNSUPPORTED: the screened form exists for full grids only)
  if (const int rc = launch_trunk(EncCall{pts, trans3, trans64, ws + W.pm, B, N, M, st}, prm, packed, pointfeat, ws + W.frun, false,
                                  screen, eps))
    return rc;
  hipLaunchKernelGGL(k_reduce_pm, dim3(n_clouds(B, M), (PMW + 255) / 256), dim3(256), 0, st, ws + W.pm, gfeat, PMW, PMW, B, N, M);
  return check_launch();
}

int catre_stn_screen_probe(int which, const catre_points* pts, const float* trans3, const float* const* prm,
                           const float* packed, float* screen, float* eps, float* rows, float* pooled, void* workspace,
                           size_t ws_bytes, int B, int N, int M, void* stream) {
  REQUIRE((which == 0 || which == 1) && pts && (which == 0 || trans3) && prm && packed && screen && eps && rows && pooled &&
          workspace && dims_ok1(B, N, M));
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const EncCall c{pts, trans3, nullptr, ws + W.pm, B, N, M, st};
  // (CATRE_ERR_UNSUPPORTED: the screened form exists for the full-grid pair kernels only)
  if (const int rc = which == 0 ? launch_stn3d(c, prm, packed, false, nullptr, screen, eps, rows)
                                : launch_stnkd(c, prm, packed, false, nullptr, screen, eps, rows))
    return rc;
  hipLaunchKernelGGL(k_reduce_pm, dim3(n_clouds(B, M), (1024 + 255) / 256), dim3(256), 0, st, ws + W.pm, pooled, 1024, 1024, B, N, M);
  return check_launch();
}

int catre_ts_head(const float* gfeat, const float* init_pose, const float* init_scale, const float* const* prm,
                  const float* packed, const catre_opts* o, float* trans_deltas, float* scale_deltas, void* workspace,
                  size_t ws_bytes, int B, void* stream) {
  REQUIRE(gfeat && init_pose && init_scale && prm && packed && o && trans_deltas && scale_deltas && B > 0);
  const int expect = PMW * (o->with_kps_feature ? 2 : 1) + (o->with_init_scale ? 3 : 0) + (o->with_init_trans ? 3 : 0);
  if (o->ts_in_dim != expect) return CATRE_ERR_BAD_ARG;
  const PackLayout L = pack_layout(o->ts_in_dim);
  hipStream_t st = (hipStream_t)stream;
  if (!workspace || ws_bytes < (size_t)B * TS_KS * 256 * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* l0part = (float*)workspace;  // WsLayout::tspart sits at offset 0 for every (N, M)
  const int groups = (B + TS_OB - 1) / TS_OB;
  {
    ProfScope ps(CATRE_K_TS_HEAD, st);
    const size_t smem0 = (size_t)TS_OB * (o->ts_in_dim / TS_KS + 2) * sizeof(float);
    hipLaunchKernelGGL(k_ts_l0, dim3(groups, TS_KS), dim3(256), smem0, st, gfeat, init_pose, init_scale, packed + L.ts_w0t,
                       l0part, B, o->ts_in_dim, o->with_kps_feature, o->with_init_scale, o->with_init_trans);
    const size_t smem = (size_t)TS_OB * (256 + 4 * 256) * sizeof(float);
    hipLaunchKernelGGL(k_ts_head, dim3(groups), dim3(1024), smem, st,
                       ts_head_args(l0part, prm, packed, L, trans_deltas, scale_deltas, B));
  }
  return check_launch();
}

static int rot_head_impl(const float* gfeat, const float* pointfeat, const float* const* prm, const float* packed,
                         float* rot6d, float* ws, const WsLayout& W, int B, int N, int M, hipStream_t st,
                         bool split = false, int rd = 3) {
  const PackLayout L = pack_layout(1);
  const int T = (N + TP - 1) / TP + (M + TP - 1) / TP;
  float* bias0 = ws + W.bias0;
  // global-feature half of layer 0 for every cloud: bias0[hd][cloud][:] = W0[:, :1024] g_cloud + b0
  hipLaunchKernelGGL(k_linear, dim3((2 * B + 31) / 32, 256 / 32, 2), dim3(64 * LIN_WAVES), 0, st, gfeat, PMW,
                     prm[CATRE_P_ROTX_L0_W], PMW, prm[CATRE_P_ROTX_L0_W + 1], bias0, 256, 2 * B, 256, 1024, 0, 0,
                     prm[CATRE_P_ROTY_L0_W], prm[CATRE_P_ROTY_L0_W + 1], bias0 + (size_t)2 * B * 256);
  // GN0 statistics from second moments of pointfeat (catre_gram.h); the moment buffers borrow y1, which is only
  // written by k_rot_l1 afterwards
  float* Gc = ws + W.y1;
  float* s1c = Gc + (size_t)2 * B * PF_NG * 4096;
  float* shc = s1c + (size_t)2 * B * PF_NG * 64;
  {
    ProfScope ps(CATRE_K_ROT_L0_STATS, st);
    // a handful of clouds: the four tile groups of a cloud on four workgroups (same partial sums, same result)
    hipLaunchKernelGGL(k_pf_moments, dim3(2 * B, pf_groups(B)), dim3(256), 0, st, pointfeat, Gc, s1c,
                       shc, B, N, M);
    hipLaunchKernelGGL(k_gn0_from_moments, dim3(B, gn0_shares(B)), dim3(256), 0, st, Gc, s1c, shc, prm[CATRE_P_ROTX_L0_W],
                       prm[CATRE_P_ROTY_L0_W], PMW, 1024, bias0, prm[CATRE_P_ROTX_GN0_W], prm[CATRE_P_ROTX_GN0_B],
                       prm[CATRE_P_ROTY_GN0_W], prm[CATRE_P_ROTY_GN0_B], ws + W.aff0, B, N, M);
  }
  {
    ProfScope ps(CATRE_K_ROT_L1, st);
    if (split)
      hipLaunchKernelGGL(k_rot_l1_split<false>, dim3(B * T), dim3(256), 0, st, pointfeat, pkb(packed, L.sp_rot_l0[0]),
                         pkb(packed, L.sp_rot_l0[1]), ws + W.aff0, pkb(packed, L.sp_rot_l1[0]), pkb(packed, L.sp_rot_l1[1]),
                         prm[CATRE_P_ROTX_L1_B], prm[CATRE_P_ROTY_L1_B], ws + W.y1, ws + W.gn1, B, N, M,
                         g_trunk_trace ? g_trunk_trace + ((size_t)1 << 24) : nullptr);
    else if (B * T >= ROTW_MIN_TILES && form_on(SW_ROTW)) {
      // grids that fill the chip: one wave per SIMD, a tile per wave (same bits as k_rot_l1)
      hipLaunchKernelGGL(k_rot_l1w, dim3((B * T + 3) / 4), dim3(256), 0, st, pointfeat, pk4(packed, L.rot_l0[0]),
                         pk4(packed, L.rot_l0[1]), ws + W.aff0, pk4(packed, L.rot_l1[0]), pk4(packed, L.rot_l1[1]),
                         prm[CATRE_P_ROTX_L1_B], prm[CATRE_P_ROTY_L1_B], ws + W.y1, ws + W.gn1, B, N, M,
                         g_trunk_trace ? g_trunk_trace + ((size_t)1 << 24) : nullptr);
    } else {
#define LAUNCH_ROT_L1(RS)                                                                                               \
  hipLaunchKernelGGL(k_rot_l1<RS>, dim3(B * T * RS), dim3(256), 0, st, pointfeat, pk4(packed, L.rot_l0[0]),               \
                     pk4(packed, L.rot_l0[1]), ws + W.aff0, pk4(packed, L.rot_l1[0]), pk4(packed, L.rot_l1[1]),         \
                     prm[CATRE_P_ROTX_L1_B], prm[CATRE_P_ROTY_L1_B], ws + W.y1, ws + W.gn1, B, N, M,                     \
                     g_trunk_trace ? g_trunk_trace + ((size_t)1 << 24) : nullptr)
      RS_DISPATCH(row_split(B * T), LAUNCH_ROT_L1)
#undef LAUNCH_ROT_L1
    }
  }
  hipLaunchKernelGGL(k_gn_finalize, dim3(B * 2), dim3(256), (size_t)T * 64 * sizeof(float), st, ws + W.gn1, ws + W.gn1stat,
                     N, M);
  {
    ProfScope ps(CATRE_K_ROT_OUT, st);
    hipLaunchKernelGGL(k_rot_out, dim3(B * T, 2), dim3(256), 0, st, ws + W.y1, ws + W.gn1stat,
                       prm[CATRE_P_ROTX_GN1_W], prm[CATRE_P_ROTX_GN1_B], prm[CATRE_P_ROTY_GN1_W],
                       prm[CATRE_P_ROTY_GN1_B], prm[CATRE_P_ROTX_NECK_W], prm[CATRE_P_ROTY_NECK_W],
                       prm[CATRE_P_ROTX_CONVP_W], prm[CATRE_P_ROTY_CONVP_W], ws + W.rpart, B, N, M, rd);
  }
  hipLaunchKernelGGL(k_rot_finish, dim3((B * 6 + 255) / 256), dim3(256), 0, st, ws + W.rpart, prm[CATRE_P_ROTX_NECK_B],
                     prm[CATRE_P_ROTY_NECK_B], packed + L.sumwp, prm[CATRE_P_ROTX_CONVP_B], prm[CATRE_P_ROTY_CONVP_B],
                     rot6d, B, T, rd);
  return check_launch();
}

int catre_rot_head_dim(const float* gfeat, const float* pointfeat, const float* const* prm, const float* packed,
                       float* rot, void* workspace, size_t ws_bytes, int B, int N, int M, int rot_dim, void* stream) {
  REQUIRE(gfeat && pointfeat && prm && packed && rot && workspace && dims_ok(B, N, M) && rot_dim >= 1 && rot_dim <= 3);
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  return rot_head_impl(gfeat, pointfeat, prm, packed, rot, (float*)workspace, W, B, N, M, (hipStream_t)stream, false,
                       rot_dim);
}

int catre_rot_to_mat(const float* rot, int rot_type, float* R_out, int B, void* stream) {
  REQUIRE(rot && R_out && B > 0 && rot_type >= CATRE_ROT_6D && rot_type <= CATRE_ROT_LIE_VEC);
  hipLaunchKernelGGL(k_rot_to_mat, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, rot, rot_type, R_out, B);
  return check_launch();
}

int catre_rot_to_mat_bwd(const float* rot, int rot_type, const float* grad_R, float* grad_rot, int B, void* stream) {
  REQUIRE(rot && grad_R && grad_rot && B > 0 && rot_type >= CATRE_ROT_6D && rot_type <= CATRE_ROT_LIE_VEC);
  hipLaunchKernelGGL(k_rot_to_mat_bwd, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, rot, rot_type, grad_R,
                     grad_rot, B);
  return check_launch();
}

int catre_rot_head(const float* gfeat, const float* pointfeat, const float* const* prm, const float* packed,
                   float* rot6d, void* workspace, size_t ws_bytes, int B, int N, int M, void* stream) {
  REQUIRE(gfeat && pointfeat && prm && packed && rot6d && workspace && dims_ok(B, N, M));
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  return rot_head_impl(gfeat, pointfeat, prm, packed, rot6d, (float*)workspace, W, B, N, M, (hipStream_t)stream);
}

static int pose_update_impl(const float* rot6d, const float* trans_deltas, const float* scale_deltas,
                            const float* init_pose, const float* init_scale, const float* mean_scales, const float* Ks,
                            const catre_opts* o, float* pose_out, float* scale_out, int B, void* stream,
                            float* pose_echo, float* scale_echo) {
  REQUIRE(rot6d && trans_deltas && scale_deltas && init_pose && init_scale && o && pose_out && scale_out && B > 0);
  if (o->k_aware && !o->delta_t_space_3d && !Ks) return CATRE_ERR_BAD_ARG;
  if (o->scale_base_mean && !mean_scales) return CATRE_ERR_BAD_ARG;
  if (o->rot_type < CATRE_ROT_6D || o->rot_type > CATRE_ROT_LIE_VEC) return CATRE_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_pose_update, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, rot6d, trans_deltas,
                     scale_deltas, init_pose, init_scale, mean_scales, Ks, *o, pose_out, scale_out, B, pose_echo,
                     scale_echo);
  return check_launch();
}

int catre_pose_update(const float* rot6d, const float* trans_deltas, const float* scale_deltas, const float* init_pose,
                      const float* init_scale, const float* mean_scales, const float* Ks, const catre_opts* o,
                      float* pose_out, float* scale_out, int B, void* stream) {
  return pose_update_impl(rot6d, trans_deltas, scale_deltas, init_pose, init_scale, mean_scales, Ks, o, pose_out, scale_out,
                          B, stream, nullptr, nullptr);
}

// One refine iteration on the bf16-operand kernels (catre_bf16.h); same launch chain, same workspace (pointfeat and
// y1 hold bf16 in their fp32-sized slots), fp32 FC tails / ts head / pose update shared with the fp32 path.
// OT = OpF16 (CATRE_DTYPE_F16): the same chain on the fp16-operand forms of the five kernels and the CATRE_PACK_F16 packs.
// LP_LAUNCH(bf16 kernel, fp16 kernel, launch arguments...)
#define LP_LAUNCH(KBF, KHF, ...)                 \
  do {                                           \
    if constexpr (is_f16_op<OT>())               \
      hipLaunchKernelGGL(KHF, __VA_ARGS__);      \
    else                                         \
      hipLaunchKernelGGL(KBF, __VA_ARGS__);      \
  } while (0)
extern "C++" {  // (a template inside the C-ABI block)
template <class OT>
static int refine_iter_bf(const catre_points* pts, const float* init_pose, const float* init_scale,
                          const float* mean_scales, const float* Ks, const float* const* prm, const float* packed,
                          const catre_opts* o, float* pose_out, float* scale_out, float* ws, const WsLayout& W, int B,
                          int N, int M, hipStream_t st, float* pose_echo, float* scale_echo) {
  const PackLayout L = pack_layout(1);
  // the operand pack of a layer: its bf16 or its fp16 image
  constexpr PackKind PK = is_f16_op<OT>() ? PK_F16 : PK_BF16;
  auto pk = [&](size_t bf, size_t hf) { return pkb(packed, is_f16_op<OT>() ? hf : bf); };
  const int T = (N + TP - 1) / TP + (M + TP - 1) / TP;
  const int rd = catre_rot_dim(o->rot_type) / 2;
  int rc;
  // all three encoder kernels take the same form (pairs of tiles or single tiles: catre_forms.h) and so the same grid
  FormDecision d;
  if ((rc = decide(STAGE_STN3D, MODE_BF16, false, false, false, B, N, M, &d))) return rc;
  const bool paired = d.form == CATRE_FORM_BF_PAIR;
  EncCall c{pts, nullptr, nullptr, ws + W.pm, B, N, M, st};
  {
    const Stn3dW w = stn3d_weights(prm, packed, L, PK);
    ProfScope ps(CATRE_K_STN3D, st);
    if (paired)
      LP_LAUNCH((k_stn3d_bf2<false>), k_stn3d_hf2, dim3(d.grid), dim3(256), 0, st, STN3D_ARGS(c, w));
    else
      LP_LAUNCH((k_stn3d_bf<false>), k_stn3d_hf, dim3(d.grid), dim3(256), 0, st, STN3D_ARGS(c, w));
  }
  c.trans3 = ws + W.trans3;
  hipLaunchKernelGGL(k_reduce_pm, dim3(2 * B, (1024 + 255) / 256), dim3(256), 0, st, ws + W.pm, ws + W.pool, 1024, 1024, B, N, M);
  if ((rc = stn_fc_tail(ws + W.pool, prm, CATRE_P_STN_FC1_W, ws + W.h1, ws + W.h2, ws + W.trans3, 3, 2 * B, st)))
    return rc;
  const float* t64 = nullptr;
  if (o->feature_transform) {
    {
      const StnkdW w = stnkd_weights(prm, packed, L, PK);
      ProfScope ps(CATRE_K_STNKD, st);
      if (paired)
        LP_LAUNCH((k_stnkd_bf2<false>), k_stnkd_hf2, dim3(d.grid), dim3(256), 0, st, STNKD_ARGS(c, w));
      else
        LP_LAUNCH((k_stnkd_bf<false>), k_stnkd_hf, dim3(d.grid), dim3(256), 0, st, STNKD_ARGS(c, w));
    }
    hipLaunchKernelGGL(k_reduce_pm, dim3(2 * B, (1024 + 255) / 256), dim3(256), 0, st, ws + W.pm, ws + W.pool, 1024, 1024, B, N, M);
    if ((rc = stn_fc_tail(ws + W.pool, prm, CATRE_P_FSTN_FC1_W, ws + W.h1, ws + W.h2, ws + W.trans64, 64, 2 * B, st)))
      return rc;
    t64 = ws + W.trans64;
  }
  u32x4* pointfeat = reinterpret_cast<u32x4*>(ws + W.pointfeat);
  {
    c.trans64 = t64;
    const TrunkW w = trunk_weights(prm, packed, L, PK);
    ProfScope ps(CATRE_K_TRUNK, st);
    if (paired)
      LP_LAUNCH((k_trunk_bf2<false>), k_trunk_hf2, dim3(d.grid), dim3(512), 0, st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace);
    else
      LP_LAUNCH(k_trunk_bf, k_trunk_hf, dim3(d.grid), dim3(256), 0, st, TRUNK_ARGS(c, w, pointfeat), g_trunk_trace);
  }
  hipLaunchKernelGGL(k_reduce_pm, dim3(2 * B, (PMW + 255) / 256), dim3(256), 0, st, ws + W.pm, ws + W.gfeat, PMW, PMW, B, N, M);
  if ((rc = catre_ts_head(ws + W.gfeat, init_pose, init_scale, prm, packed, o, ws + W.dt, ws + W.ds, ws,
                          W.total * sizeof(float), B, (void*)st)))
    return rc;
  float* bias0 = ws + W.bias0;
  hipLaunchKernelGGL(k_linear, dim3((2 * B + 31) / 32, 256 / 32, 2), dim3(64 * LIN_WAVES), 0, st, ws + W.gfeat, PMW,
                     prm[CATRE_P_ROTX_L0_W], PMW, prm[CATRE_P_ROTX_L0_W + 1], bias0, 256, 2 * B, 256, 1024, 0, 0,
                     prm[CATRE_P_ROTY_L0_W], prm[CATRE_P_ROTY_L0_W + 1], bias0 + (size_t)2 * B * 256);
  {
    // GN0 statistics from second moments of the (bf16) pointfeat like the fp32 path (catre_gram.h) instead of a recompute of
    // layer 0 over every point: the statistics are those of W0 pf in fp32 on the bf16-rounded pointfeat - layer 0's own
    // bf16 weight rounding moves them by ~1e-4 relative, a fraction of what rounding a0 to bf16 does next.  The moment
    // buffers borrow y1, which k_rot_l1_bf writes afterwards.
    float* Gc = ws + W.y1;
    float* s1c = Gc + (size_t)2 * B * PF_NG * 4096;
    float* shc = s1c + (size_t)2 * B * PF_NG * 64;
    ProfScope ps(CATRE_K_ROT_L0_STATS, st);
    LP_LAUNCH(k_pf_moments_bf, k_pf_moments_hf, dim3(2 * B, pf_groups(B)), dim3(256), 0, st, pointfeat, Gc, s1c,
              shc, B, N, M);
    hipLaunchKernelGGL(k_gn0_from_moments, dim3(B, gn0_shares(B)), dim3(256), 0, st, Gc, s1c, shc, prm[CATRE_P_ROTX_L0_W],
                       prm[CATRE_P_ROTY_L0_W], PMW, 1024, bias0, prm[CATRE_P_ROTX_GN0_W], prm[CATRE_P_ROTX_GN0_B],
                       prm[CATRE_P_ROTY_GN0_W], prm[CATRE_P_ROTY_GN0_B], ws + W.aff0, B, N, M);
  }
  unsigned short* y1 = reinterpret_cast<unsigned short*>(ws + W.y1);
  {
    ProfScope ps(CATRE_K_ROT_L1, st);
    LP_LAUNCH(k_rot_l1_bf, k_rot_l1_hf, dim3(B * T), dim3(256), 0, st, pointfeat, pk(L.bf_rot_l0[0], L.f16_rot_l0[0]),
              pk(L.bf_rot_l0[1], L.f16_rot_l0[1]), ws + W.aff0, pk(L.bf_rot_l1[0], L.f16_rot_l1[0]),
              pk(L.bf_rot_l1[1], L.f16_rot_l1[1]), prm[CATRE_P_ROTX_L1_B], prm[CATRE_P_ROTY_L1_B], y1, ws + W.gn1, B,
              N, M, g_trunk_trace ? g_trunk_trace + ((size_t)1 << 24) : nullptr);
  }
  hipLaunchKernelGGL(k_gn_finalize, dim3(B * 2), dim3(256), (size_t)T * 64 * sizeof(float), st, ws + W.gn1, ws + W.gn1stat,
                     N, M);
  {
    ProfScope ps(CATRE_K_ROT_OUT, st);
    LP_LAUNCH(k_rot_out_bf, k_rot_out_hf, dim3(B * T, 2), dim3(256), 0, st, y1, ws + W.gn1stat, prm[CATRE_P_ROTX_GN1_W],
              prm[CATRE_P_ROTX_GN1_B], prm[CATRE_P_ROTY_GN1_W], prm[CATRE_P_ROTY_GN1_B],
              prm[CATRE_P_ROTX_NECK_W], prm[CATRE_P_ROTY_NECK_W], prm[CATRE_P_ROTX_CONVP_W],
              prm[CATRE_P_ROTY_CONVP_W], ws + W.rpart, B, N, M, rd);
  }
  hipLaunchKernelGGL(k_rot_finish, dim3((B * 6 + 255) / 256), dim3(256), 0, st, ws + W.rpart, prm[CATRE_P_ROTX_NECK_B],
                     prm[CATRE_P_ROTY_NECK_B], packed + L.sumwp, prm[CATRE_P_ROTX_CONVP_B], prm[CATRE_P_ROTY_CONVP_B],
                     ws + W.rot6d, B, T, rd);
  if ((rc = check_launch())) return rc;
  return pose_update_impl(ws + W.rot6d, ws + W.dt, ws + W.ds, init_pose, init_scale, mean_scales, Ks, o, pose_out,
                          scale_out, B, (void*)st, pose_echo, scale_echo);
}
}  // extern "C++"
#undef LP_LAUNCH

static int refine_iter_impl(const catre_points* pts, const float* init_pose, const float* init_scale,
                            const float* mean_scales, const float* Ks, const float* const* prm, const float* packed,
                            const catre_opts* o, float* pose_out, float* scale_out, void* workspace, size_t ws_bytes, int B,
                            int N, int M, void* stream, float* pose_echo, float* scale_echo) {
  REQUIRE(pts && pts->obs && pts->kps && init_pose && init_scale && prm && packed && o && pose_out && scale_out &&
          workspace && dims_ok(B, N, M));
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  // the two rot heads emit rot_dim values each: only even-width parametrisations can come out of them
  if (o->rot_type != CATRE_ROT_6D && o->rot_type != CATRE_ROT_QUAT) return CATRE_ERR_UNSUPPORTED;
  if (o->compute_dtype == CATRE_DTYPE_BF16)
    return refine_iter_bf<OpBf16>(pts, init_pose, init_scale, mean_scales, Ks, prm, packed, o, pose_out, scale_out, ws, W, B,
                                  N, M, st, pose_echo, scale_echo);
  if (o->compute_dtype == CATRE_DTYPE_F16)  // packed must hold CATRE_PACK_F16
    return refine_iter_bf<OpF16>(pts, init_pose, init_scale, mean_scales, Ks, prm, packed, o, pose_out, scale_out, ws, W, B,
                                 N, M, st, pose_echo, scale_echo);
  if (o->compute_dtype != CATRE_DTYPE_F32 && o->compute_dtype != CATRE_DTYPE_SPLIT) return CATRE_ERR_UNSUPPORTED;
  const bool split = o->compute_dtype == CATRE_DTYPE_SPLIT;
  const int T = (N + TP - 1) / TP + (M + TP - 1) / TP, R = 2 * B;
  const int rd = catre_rot_dim(o->rot_type) / 2;
  // Small batches take the latency path (catre_small.h): the same arithmetic on fewer launches.
  const size_t smem_d = sizeof(float) * (size_t)std::max(T * 64 + 64 + 16, TS_OB * (256 + 4 * 256));
  const bool small = R <= SMALL_ROWS && smem_d <= 64 * 1024;
  // ... and while a consumer of a pooled feature can take the maximum over the tile partials itself: every one of fc1's
  // 16 workgroups stages all R rows x 16 tiles, which beats a k_reduce_pm launch up to R = 4 clouds (B = 4: 15 vs 5 + 5.5 us)
  const bool fold = small && R <= SMALL_FOLD_ROWS;
  const float* pm = fold ? ws + W.pm : nullptr;
  auto reduce_pm = [&](float* out, int ldo, int C, int rpt = 1) {
    hipLaunchKernelGGL(k_reduce_pm, dim3(R, (C + 255) / 256), dim3(256), 0, st, ws + W.pm, out, ldo, C, B, N, M, rpt);
  };
  // STN3d (pointnet.py:98) on both clouds
  // small fp32 batches: each FC tail as ONE launch (k_fc_tail); its barrier counters are zeroed by the encoder kernel in front
  unsigned* bar = small && !split && form_on(SW_FC_TAIL) ? reinterpret_cast<unsigned*>(ws + W.bar) : nullptr;
  EncCall c{pts, nullptr, nullptr, ws + W.pm, B, N, M, st};
  if ((rc = launch_stn3d(c, prm, packed, split, bar))) return rc;
  c.trans3 = ws + W.trans3;
  if (!fold) reduce_pm(ws + W.pool, 1024, 1024);
  if ((rc = stn_fc_tail(ws + W.pool, prm, CATRE_P_STN_FC1_W, ws + W.h1, ws + W.h2, ws + W.trans3, 3, R, st, pm, B, N, M,
                        bar)))
    return rc;
  const float* t64 = nullptr;
  if (o->feature_transform) {  // STNkd (pointnet.py:105-106)
    if ((rc = launch_stnkd(c, prm, packed, split, bar))) return rc;
    if (!fold) reduce_pm(ws + W.pool, 1024, 1024);
    if ((rc = stn_fc_tail(ws + W.pool, prm, CATRE_P_FSTN_FC1_W, ws + W.h1, ws + W.h2, ws + W.trans64, 64, R, st, pm, B, N,
                          M, bar)))
      return rc;
    t64 = ws + W.trans64;
  }
  c.trans64 = t64;
  // a handful of objects, fp32: the trunk on HALF tiles (32 points per workgroup: half the per-tile prologue)
  const int rsh = small && !split ? trunk_h_split(B * T) : 0;
  if (rsh) {
    const TrunkW w = trunk_weights(prm, packed, pack_layout(1), PK_F32);
    ProfScope ps(CATRE_K_TRUNK, st);
#define LAUNCH_(RSH) \
  hipLaunchKernelGGL(k_trunk_h<RSH>, dim3(B * T * 2 * RSH), dim3(512), 0, st, TRUNK_ARGS(c, w, ws + W.pointfeat))
    RS_DISPATCH(rsh, LAUNCH_)
#undef LAUNCH_
  } else if ((rc = launch_trunk(c, prm, packed, ws + W.pointfeat, ws + W.frun, split))) {
    return rc;
  }
  if (!small) {
    reduce_pm(ws + W.gfeat, PMW, PMW);
    if ((rc = check_launch())) return rc;
    if ((rc = catre_ts_head(ws + W.gfeat, init_pose, init_scale, prm, packed, o, ws + W.dt, ws + W.ds, workspace, ws_bytes,
                            B, stream)))
      return rc;
    if ((rc = rot_head_impl(ws + W.gfeat, ws + W.pointfeat, prm, packed, ws + W.rot6d, ws, W, B, N, M, st, split, rd)))
      return rc;
    return pose_update_impl(ws + W.rot6d, ws + W.dt, ws + W.ds, init_pose, init_scale, mean_scales, Ks, o, pose_out,
                            scale_out, B, stream, pose_echo, scale_echo);
  }
  // ---- latency path after the trunk: 5 launches (catre_small.h), 6 when the pooled feature is reduced by its own ----
  if (!fold) reduce_pm(ws + W.gfeat, PMW, PMW, rsh ? 2 : 1);
  {
    const int expect = PMW * (o->with_kps_feature ? 2 : 1) + (o->with_init_scale ? 3 : 0) + (o->with_init_trans ? 3 : 0);
    if (o->ts_in_dim != expect) return CATRE_ERR_BAD_ARG;
    if (o->k_aware && !o->delta_t_space_3d && !Ks) return CATRE_ERR_BAD_ARG;
    if (o->scale_base_mean && !mean_scales) return CATRE_ERR_BAD_ARG;
  }
  const PackLayout L = pack_layout(o->ts_in_dim);
  float* bias0 = ws + W.bias0;
  float* Gc = ws + W.y1;  // the moment buffers borrow y1 (see rot_head_impl)
  float* s1c = Gc + (size_t)2 * B * PF_NG * 4096;
  float* shc = s1c + (size_t)2 * B * PF_NG * 64;
  const int groups = (B + TS_OB - 1) / TS_OB;
  {
    HeadsAArgs A;
    A.pointfeat = ws + W.pointfeat;
    A.Gc = Gc;
    A.s1c = s1c;
    A.shc = shc;
    A.pose = init_pose;
    A.scale = init_scale;
    A.W0T = packed + L.ts_w0t;
    A.tspart = ws + W.tspart;
    A.in_dim = o->ts_in_dim;
    A.with_kps = o->with_kps_feature;
    A.with_scale = o->with_init_scale;
    A.with_trans = o->with_init_trans;
    A.w0x = prm[CATRE_P_ROTX_L0_W];
    A.b0x = prm[CATRE_P_ROTX_L0_W + 1];
    A.w0y = prm[CATRE_P_ROTY_L0_W];
    A.b0y = prm[CATRE_P_ROTY_L0_W + 1];
    A.bias0 = bias0;
    A.pm = fold ? ws + W.pm : nullptr;
    A.gfeat = ws + W.gfeat;
    A.B = B;
    A.N = N;
    A.M = M;
    A.rpt = rsh ? 2 : 1;
    A.n_mom = R * PF_NG;
    A.n_ts = groups * TS_KS;
    ProfScope ps(CATRE_K_ROT_L0_STATS, st);
    hipLaunchKernelGGL(k_heads_a, dim3(A.n_mom + A.n_ts + 2 * 8), dim3(64 * LIN_WAVES), 0, st, A);
    hipLaunchKernelGGL(k_gn0_from_moments, dim3(B, gn0_shares(B)), dim3(256), 0, st, Gc, s1c, shc, prm[CATRE_P_ROTX_L0_W],
                       prm[CATRE_P_ROTY_L0_W], PMW, 1024, bias0, prm[CATRE_P_ROTX_GN0_W], prm[CATRE_P_ROTX_GN0_B],
                       prm[CATRE_P_ROTY_GN0_W], prm[CATRE_P_ROTY_GN0_B], ws + W.aff0, B, N, M);
  }
  {
    ProfScope ps(CATRE_K_ROT_L1, st);
    if (split)
      hipLaunchKernelGGL(k_rot_l1_split<false>, dim3(B * T), dim3(256), 0, st, ws + W.pointfeat, pkb(packed, L.sp_rot_l0[0]),
                         pkb(packed, L.sp_rot_l0[1]), ws + W.aff0, pkb(packed, L.sp_rot_l1[0]), pkb(packed, L.sp_rot_l1[1]),
                         prm[CATRE_P_ROTX_L1_B], prm[CATRE_P_ROTY_L1_B], ws + W.y1, ws + W.gn1, B, N, M,
                         g_trunk_trace ? g_trunk_trace + ((size_t)1 << 24) : nullptr);
    else {
#define LAUNCH_ROT_L1(RS)                                                                                               \
  hipLaunchKernelGGL(k_rot_l1<RS>, dim3(B * T * RS), dim3(256), 0, st, ws + W.pointfeat, pk4(packed, L.rot_l0[0]),        \
                     pk4(packed, L.rot_l0[1]), ws + W.aff0, pk4(packed, L.rot_l1[0]), pk4(packed, L.rot_l1[1]),         \
                     prm[CATRE_P_ROTX_L1_B], prm[CATRE_P_ROTY_L1_B], ws + W.y1, ws + W.gn1, B, N, M,                     \
                     g_trunk_trace ? g_trunk_trace + ((size_t)1 << 24) : nullptr)
      RS_DISPATCH(row_split(B * T), LAUNCH_ROT_L1)
#undef LAUNCH_ROT_L1
    }
  }
  {
    HeadsDArgs D;
    D.y1 = ws + W.y1;
    D.gn1 = ws + W.gn1;
    D.gam1x = prm[CATRE_P_ROTX_GN1_W];
    D.bet1x = prm[CATRE_P_ROTX_GN1_B];
    D.gam1y = prm[CATRE_P_ROTY_GN1_W];
    D.bet1y = prm[CATRE_P_ROTY_GN1_B];
    D.neckx = prm[CATRE_P_ROTX_NECK_W];
    D.necky = prm[CATRE_P_ROTY_NECK_W];
    D.wpx = prm[CATRE_P_ROTX_CONVP_W];
    D.wpy = prm[CATRE_P_ROTY_CONVP_W];
    D.rpart = ws + W.rpart;
    D.B = B;
    D.N = N;
    D.M = M;
    D.rd = rd;
    D.n_rot = B * T * 2;
    D.ts = ts_head_args(ws + W.tspart, prm, packed, L, ws + W.dt, ws + W.ds, B);
    ProfScope ps(CATRE_K_ROT_OUT, st);
    hipLaunchKernelGGL(k_heads_d, dim3(D.n_rot + groups), dim3(1024), smem_d, st, D);
  }
  hipLaunchKernelGGL(k_finish_update, dim3((B + 7) / 8), dim3(64), 0, st, ws + W.rpart, prm[CATRE_P_ROTX_NECK_B],
                     prm[CATRE_P_ROTY_NECK_B], packed + L.sumwp, prm[CATRE_P_ROTX_CONVP_B], prm[CATRE_P_ROTY_CONVP_B], T, rd,
                     ws + W.dt, ws + W.ds, init_pose, init_scale, mean_scales, Ks, *o, pose_out, scale_out, B, pose_echo,
                     scale_echo);
  return check_launch();
}

int catre_refine_iter(const catre_points* pts, const float* init_pose, const float* init_scale,
                      const float* mean_scales, const float* Ks, const float* const* prm, const float* packed,
                      const catre_opts* o, float* pose_out, float* scale_out, void* workspace, size_t ws_bytes, int B,
                      int N, int M, void* stream) {
  return refine_iter_impl(pts, init_pose, init_scale, mean_scales, Ks, prm, packed, o, pose_out, scale_out, workspace,
                          ws_bytes, B, N, M, stream, nullptr, nullptr);
}

// init_pose / init_scale == nullptr: slot 0 of poses / scales holds the initial estimate (catre_refine_k); otherwise the
// first iteration reads the caller's buffers and its pose-update kernel copies them into slot 0 (catre_refine_k_from)
static int refine_k_impl(const float* pcl, const float* kps, const float* init_pose, const float* init_scale,
                         const float* mean_scales, const float* Ks, const float* const* prm, const float* packed,
                         const catre_opts* o, float* poses, float* scales, void* workspace, size_t ws_bytes, int B, int N,
                         int M, int n_iter, void* stream) {
  REQUIRE(pcl && kps && prm && packed && o && poses && scales && workspace && dims_ok(B, N, M) && n_iter >= 0);
  REQUIRE((init_pose == nullptr) == (init_scale == nullptr));
  const WsLayout W = ws_layout(B, N, M);
  if (ws_bytes < W.total * sizeof(float)) return CATRE_ERR_WORKSPACE;
  float* ws = (float*)workspace;
  // Small batches (latency-bound: every launch counts): the raw clouds go straight to the encoder kernels and the
  // pose-apply of batch_updater_test happens as they load a point.  Large batches: x / tfd_kps are materialised once per
  // iteration (5 us) - three kernels x eight waves re-deriving every point's transform costs more than that there.
  // Same device function either way: same bits.
#ifndef CATRE_OTF_POINTS
#define CATRE_OTF_POINTS (64 * 1024)
#endif
  const bool on_the_fly = (size_t)B * (N + M) <= (size_t)CATRE_OTF_POINTS;
  catre_points pts;
  pts.obs = on_the_fly ? pcl : ws + W.xbuf;
  pts.obs_sb = (int64_t)N * 3;
  pts.obs_sn = 3;
  pts.obs_sc = 1;
  pts.kps = on_the_fly ? kps : ws + W.kbuf;
  pts.kps_sb = (int64_t)M * 3;
  pts.kps_sn = 3;
  pts.kps_sc = 1;
  pts.apply_pose = on_the_fly ? 1 : 0;
  pts.zero_center = o->zero_center;
  pts.pose = pts.scale = nullptr;
  if (init_pose && n_iter == 0) {  // nothing to ride on: plain copies
    if (hipMemcpyAsync(poses, init_pose, (size_t)B * 12 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
            hipSuccess ||
        hipMemcpyAsync(scales, init_scale, (size_t)B * 3 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
            hipSuccess)
      return CATRE_ERR_LAUNCH;
  }
  for (int i = 1; i <= n_iter; ++i) {
    const bool first = init_pose && i == 1;
    const float* pose_in = first ? init_pose : poses + (size_t)(i - 1) * B * 12;
    // batch_test.py:74-75: the scale estimate is only fed back when REFINE_SCLAE
    const float* scale_in = first ? init_scale : scales + (size_t)(o->refine_scale ? i - 1 : 0) * B * 3;
    if (on_the_fly) {
      pts.pose = pose_in;
      pts.scale = scale_in;
    } else {
      const int rc0 =
          catre_pose_apply(pcl, kps, pose_in, scale_in, ws + W.xbuf, ws + W.kbuf, B, N, M, o->zero_center, stream);
      if (rc0) return rc0;
    }
    const int rc = refine_iter_impl(&pts, pose_in, scale_in, mean_scales, Ks, prm, packed, o, poses + (size_t)i * B * 12,
                                    scales + (size_t)i * B * 3, workspace, ws_bytes, B, N, M, stream,
                                    first ? poses : nullptr, first ? scales : nullptr);
    if (rc) return rc;
  }
  return CATRE_OK;
}

int catre_refine_k(const float* pcl, const float* kps, const float* mean_scales, const float* Ks,
                   const float* const* prm, const float* packed, const catre_opts* o, float* poses, float* scales,
                   void* workspace, size_t ws_bytes, int B, int N, int M, int n_iter, void* stream) {
  return refine_k_impl(pcl, kps, nullptr, nullptr, mean_scales, Ks, prm, packed, o, poses, scales, workspace, ws_bytes, B, N,
                       M, n_iter, stream);
}

int catre_refine_k_from(const float* pcl, const float* kps, const float* init_pose, const float* init_scale,
                        const float* mean_scales, const float* Ks, const float* const* prm, const float* packed,
                        const catre_opts* o, float* poses, float* scales, void* workspace, size_t ws_bytes, int B, int N,
                        int M, int n_iter, void* stream) {
  REQUIRE(init_pose && init_scale);
  return refine_k_impl(pcl, kps, init_pose, init_scale, mean_scales, Ks, prm, packed, o, poses, scales, workspace, ws_bytes,
                       B, N, M, n_iter, stream);
}


int catre_form_switch(int id, int value) {
  if (id == SW_EPI) {  // not a bit of the form word: it picks the epilogue of the fp16-screen forms, not a form
    const int cur = screen_epi();
    if (value >= 0) g_screen_epi.store(value != 0, std::memory_order_relaxed);
    return cur;
  }
  if (id == SW_DA || id == SW_DA_STN) {  // likewise: they pick the bound the same kernels select with
    std::atomic<int>& g = id == SW_DA ? g_screen_da : g_screen_da_stn;
    const int cur = env_switch(g, id == SW_DA ? "CATRE_SCREEN_DA" : "CATRE_SCREEN_DA_STN",
                               id == SW_DA ? CATRE_SCREEN_DA_DEFAULT : CATRE_SCREEN_DA_STN_DEFAULT);
    if (value >= 0) g.store(value != 0, std::memory_order_relaxed);
    return cur;
  }
  if (id < 0 || id >= SW_PUBLIC) return -1;
  const int bit = sw(id);
  const int cur = forms();
  if (value >= 0) g_forms.store(value ? (cur | bit) : (cur & ~bit), std::memory_order_relaxed);
  return (cur & bit) ? 1 : 0;
}

int catre_screen_run_len(int value) {
  const int prev = g_run_len.load(std::memory_order_relaxed);
  if (value >= 0) g_run_len.store(value > 16 ? 16 : value, std::memory_order_relaxed);
  return prev;
}

int catre_screen_run_rule(int B, int N, int M, int cus) {
  if (B <= 0 || N <= 0 || M < 0 || cus <= 0) return -1;
  return screen_run_rule(B, N, M, cus);
}

int catre_form_decision(int stage, int mode, int save, int rows, int probe, int B, int N, int M, int switches, int cus,
                        int run_len, int bf_pair_min, int* out) {
  FormDecision d;
  if (!out || !form_decision(stage, mode, save != 0, rows != 0, probe != 0, B, N, M, switches < 0 ? -1 : effective_forms(switches), cus,
                             run_len, bf_pair_min, &d))
    return -1;
  out[0] = d.form, out[1] = d.row_split, out[2] = d.S, out[3] = d.grid;
  return 0;
}

int catre_debug_knob(int id, int value) {
#ifdef CATRE_DEBUG_TRACE
  if (id == 0) return hipMemcpyToSymbol(HIP_SYMBOL(g_dephase_cycles), &value, sizeof(int)) == hipSuccess ? CATRE_OK : CATRE_ERR_LAUNCH;
  if (id == 1) return hipMemcpyToSymbol(HIP_SYMBOL(g_ablate), &value, sizeof(int)) == hipSuccess ? CATRE_OK : CATRE_ERR_LAUNCH;
  if (id == 2) return hipMemcpyToSymbol(HIP_SYMBOL(g_screen_count_on), &value, sizeof(int)) == hipSuccess ? CATRE_OK : CATRE_ERR_LAUNCH;
  if (id == 3) {  // SCREEN_STAMP of catre_screen.h into the buffer of catre_debug_trunk_trace (>= 1 << 24 entries)
    unsigned long long* t = value ? g_trunk_trace : nullptr;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_screen_trace), &t, sizeof(t)) == hipSuccess ? CATRE_OK : CATRE_ERR_LAUNCH;
  }
  return CATRE_ERR_BAD_ARG;
#else
  (void)id;
  (void)value;
  return CATRE_ERR_UNSUPPORTED;
#endif
}

// Identity of the capture `stream` is recording into (0: not capturing).  HipRuntime keys "this capture already holds a
// weight-pack node" on it: two captures on one stream are two graphs, each needs its own pack node.
int catre_stream_capture_id(void* stream, unsigned long long* id_out) {
  REQUIRE(id_out);
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo((hipStream_t)stream, &status, &id) != hipSuccess) return CATRE_ERR_LAUNCH;
  *id_out = status == hipStreamCaptureStatusActive ? id : 0ull;
  return CATRE_OK;
}

int catre_debug_screen_counts(unsigned long long* out192, int reset) {
#ifdef CATRE_DEBUG_TRACE
  REQUIRE(out192);
  if (hipMemcpyFromSymbol(out192, HIP_SYMBOL(g_screen_cnt), 3 * 64 * sizeof(unsigned long long)) != hipSuccess) return CATRE_ERR_LAUNCH;
  if (reset) {
    const unsigned long long z[3 * 64] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_screen_cnt), z, sizeof(z)) != hipSuccess) return CATRE_ERR_LAUNCH;
  }
  return CATRE_OK;
#else
  (void)out192;
  (void)reset;
  return CATRE_ERR_UNSUPPORTED;
#endif
}

int catre_debug_trunk_trace(void* device_buffer) {
#ifdef CATRE_DEBUG_TRACE
  g_trunk_trace = (unsigned long long*)device_buffer;
  // (the screened epilogues' sub-phase stamps need a larger buffer: off until catre_debug_knob 3 asks for them)
  unsigned long long* none = nullptr;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_screen_trace), &none, sizeof(none)) == hipSuccess ? CATRE_OK : CATRE_ERR_LAUNCH;
#else
  (void)device_buffer;
  return CATRE_ERR_UNSUPPORTED;  // product build: no stamps in the kernels (make TRACE=1 builds the instrumented library)
#endif
}

#ifdef CATRE_NO_PROFILING
int catre_profile_enable(int, int) { return CATRE_ERR_UNSUPPORTED; }
int catre_profile_collect(float*, int, int*) { return CATRE_ERR_UNSUPPORTED; }
#else
int catre_profile_enable(int kernel_id, int max_records) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
  delete[] g_prof.ev;
  g_prof = ProfState();
  if (kernel_id < 0 || max_records <= 0) return CATRE_OK;
  if (kernel_id >= CATRE_K_COUNT) return CATRE_ERR_BAD_ARG;
  g_prof.ev = new hipEvent_t[2 * max_records];
  for (int i = 0; i < 2 * max_records; ++i)
    if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) return CATRE_ERR_LAUNCH;
  g_prof.kernel = kernel_id;
  g_prof.cap = max_records;
  return CATRE_OK;
}

int catre_profile_collect(float* ms_out, int max_out, int* n_out) {
  REQUIRE(n_out && (ms_out || max_out == 0));
  std::lock_guard<std::mutex> lk(g_prof_mu);
  int n = g_prof.n < max_out ? g_prof.n : max_out;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return CATRE_ERR_LAUNCH;
    if (hipEventElapsedTime(&ms_out[i], g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) return CATRE_ERR_LAUNCH;
  }
  *n_out = n;
  g_prof.n = 0;
  return CATRE_OK;
}
#endif

int catre_colmax(const float* x, float* out, int B, int C, int N, void* stream) {
  REQUIRE(x && out && B > 0 && C > 0 && N > 0);
  const int rows = B * C;
  const int grid = rows / 4 < 8192 ? (rows + 3) / 4 : 8192;
  {
    ProfScope ps(CATRE_K_COLMAX, (hipStream_t)stream);
    hipLaunchKernelGGL(k_colmax, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, rows, N);
  }
  return check_launch();
}

#include "catre_trainfwd_api.inc"

}  // extern "C"
