// Host side of the encoder launches, free of HIP: the kernel-form switch table, the pure decision which kernel form a
// stage runs (catre_form_decision of the C ABI), the packed-weight layout and one weight bundle per encoder stage.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdlib>

#include "../../include/catre_hip.h"
#include "catre_host.h"  // align_up (the plain C++ part)

namespace catre_host {

constexpr int TILE = 64;  // points per tile (TP of catre_device.h)
inline int tiles_of(int n) { return (n + TILE - 1) / TILE; }

// ---- the switch table --------------------------------------------------------------------------
// Which kernel FORM a full grid takes where more than one exists.  All forms of a stage give the same bits; the switches
// exist for A/B measurements and for tests that compare the forms in one process.  The environment sets the process
// default once, catre_form_switch changes ids 0 - 9 at run time; the three STN arms follow the environment only.
enum {
  SW_TRUNK4, SW_STN4, SW_STN_PAIR, SW_ROTW, SW_FC_TAIL, SW_SCREEN, SW_SCREEN_STN, SW_SCREEN_POOL, SW_SCREEN_RUN, SW_SCREEN_F16,
  SW_PUBLIC,  // ids below: catre_form_switch
  SW_POOL_STN = SW_PUBLIC, SW_RUN_STN, SW_F16_STN, SW_COUNT
};
constexpr int sw(int id) { return 1 << id; }

#ifndef CATRE_SCREEN_DEFAULT
#define CATRE_SCREEN_DEFAULT true
#endif
#ifndef CATRE_SCREEN_STN_DEFAULT
#define CATRE_SCREEN_STN_DEFAULT true
#endif
#ifndef CATRE_SCREEN_POOL_DEFAULT
#define CATRE_SCREEN_POOL_DEFAULT true
#endif
#ifndef CATRE_SCREEN_RUN_DEFAULT
#define CATRE_SCREEN_RUN_DEFAULT true
#endif
#ifndef CATRE_SCREEN_F16_DEFAULT
#define CATRE_SCREEN_F16_DEFAULT true
#endif
#ifndef CATRE_SCREEN_POOL_STN_DEFAULT
#define CATRE_SCREEN_POOL_STN_DEFAULT true
#endif
#ifndef CATRE_SCREEN_RUN_STN_DEFAULT
#define CATRE_SCREEN_RUN_STN_DEFAULT true
#endif
#ifndef CATRE_SCREEN_F16_STN_DEFAULT
#define CATRE_SCREEN_F16_STN_DEFAULT true
#endif

struct Switch {
  const char* env;
  bool dflt;
  int needs;  // the switches this one refines: it has no effect unless all of them are on
};
constexpr int POOL = sw(SW_SCREEN_POOL), POOLED_STN = POOL | sw(SW_POOL_STN), SCREENED_STN = sw(SW_SCREEN) | sw(SW_SCREEN_STN);
// one row per switch: form, default, the A/B file under profiles/ that decided it
constexpr Switch SWITCHES[SW_COUNT] = {
    {"CATRE_TRUNK4", true, 0},                                // k_trunk4, one wave per SIMD; on (r05_ab_trunk4.jsonl)
    {"CATRE_STN4", true, 0},                                  // k_stn*<1, false, true>, one wave per SIMD; on (r05_ab_stn4.txt)
    {"CATRE_STN_PAIR", true, 0},                              // k_stn*_pair, two tiles per workgroup; on (r05_ab_stn_pair.txt)
    {"CATRE_ROTW", false, 0},                                 // k_rot_l1w; off, 8 % slower than k_rot_l1<1> (r06_rotw_phases.txt)
    {"CATRE_FC_TAIL", false, 0},                              // k_fc_tail, B <= 8; off, 0.643 vs 0.620 ms (r06_fc_tail_ab.jsonl)
    {"CATRE_SCREEN", CATRE_SCREEN_DEFAULT, 0},                // k_trunk4s, screened conv4 max-pool; on, 30.7 vs 34.0 ms (screen_ab.jsonl)
    {"CATRE_SCREEN_STN", CATRE_SCREEN_STN_DEFAULT, sw(SW_SCREEN)},  // k_stn*_pair_s, conv3 screened; on, 28.97 vs 30.82 ms (screen_stn_ab.jsonl)
    {"CATRE_SCREEN_POOL", CATRE_SCREEN_POOL_DEFAULT, 0},      // k_trunk4sp, a list per wave; on, 24.55 vs 28.70 ms (screen_pool_ab.jsonl); a probe reads it with `screen` off
    {"CATRE_SCREEN_RUN", CATRE_SCREEN_RUN_DEFAULT, POOL},     // k_trunk4sr, runs of tiles; on, 21.59 vs 24.25 ms (screen_run_ab.jsonl)
    {"CATRE_SCREEN_F16", CATRE_SCREEN_F16_DEFAULT, POOL},     // k_trunk4sp16 / sr16, one fp16 screen product; on, 19.40 vs 21.67 ms (screen_f16_ab.jsonl)
    {"CATRE_SCREEN_POOL_STN", CATRE_SCREEN_POOL_STN_DEFAULT, POOL},  // the STN kernels' own arm of each: k_stn*_pair_sp (screen_pool_ab.jsonl)
    {"CATRE_SCREEN_RUN_STN", CATRE_SCREEN_RUN_STN_DEFAULT, SCREENED_STN | sw(SW_SCREEN_RUN) | POOLED_STN},  // k_stn*_pair_sr (screen_run_ab.jsonl)
    {"CATRE_SCREEN_F16_STN", CATRE_SCREEN_F16_STN_DEFAULT, sw(SW_SCREEN_F16) | POOLED_STN},  // k_stn*_pair_sp16 / _sr16 (screen_f16_ab.jsonl)
};

// `screen_epi` (catre_form_switch id SW_EPI, CATRE_SCREEN_EPI): the lean selection, list build and scan behind the fp16
// screen's sweep (k_*_sr16e / k_*_sp16e; on, profiles/screen_epi_ab.jsonl).  It picks no other FORM - grid, run length and
// screen arithmetic are those of `run_f16` / `screen_f16` - so it is no bit of the 13-bit form word the decision reads: ids
// 10 - 12 stay the raw bits of the env-only STN arms, and this switch takes the first id behind the word.
#ifndef CATRE_SCREEN_EPI_DEFAULT
#define CATRE_SCREEN_EPI_DEFAULT true
#endif
constexpr int SW_EPI = SW_COUNT;
inline std::atomic<int> g_screen_epi{-1};
inline bool screen_epi() {
  int v = g_screen_epi.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("CATRE_SCREEN_EPI");
    v = e ? atoi(e) != 0 : CATRE_SCREEN_EPI_DEFAULT;
    g_screen_epi.store(v, std::memory_order_relaxed);
  }
  return v != 0;
}

// `screen_da` (SW_DA, CATRE_SCREEN_DA) and its STN arm (SW_DA_STN, CATRE_SCREEN_DA_STN; counts while `screen_da` is on):
// the fp16 screen's eps with the activations' rounding MEASURED per tile and the weights' error sign-split
// (catre_screen.h) - a runtime flag of the same fp16-screen kernels, no form and no kernel of its own; off is the
// shipped eps bit for bit.  Fewer candidates reach the replay; the outputs keep their bits either way.
#ifndef CATRE_SCREEN_DA_DEFAULT
#define CATRE_SCREEN_DA_DEFAULT true
#endif
#ifndef CATRE_SCREEN_DA_STN_DEFAULT
#define CATRE_SCREEN_DA_STN_DEFAULT false
#endif
constexpr int SW_DA = SW_COUNT + 1, SW_DA_STN = SW_COUNT + 2;
inline std::atomic<int> g_screen_da{-1}, g_screen_da_stn{-1};
inline int env_switch(std::atomic<int>& g, const char* env, bool dflt) {
  int v = g.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv(env);
    v = e ? atoi(e) != 0 : dflt;
    g.store(v, std::memory_order_relaxed);
  }
  return v;
}
inline int screen_da() { return env_switch(g_screen_da, "CATRE_SCREEN_DA", CATRE_SCREEN_DA_DEFAULT); }
inline int screen_da_stn() {
  return screen_da() && env_switch(g_screen_da_stn, "CATRE_SCREEN_DA_STN", CATRE_SCREEN_DA_STN_DEFAULT);
}

// the raw switch word: read from the environment once, ids 0 - 9 then follow catre_form_switch
inline std::atomic<int> g_forms{-1};
inline int forms() {
  int v = g_forms.load(std::memory_order_relaxed);
  if (v < 0) {
    v = 0;
    for (int id = 0; id < SW_COUNT; ++id) {
      const char* e = getenv(SWITCHES[id].env);
      if (e ? atoi(e) != 0 : SWITCHES[id].dflt) v |= sw(id);
    }
    g_forms.store(v, std::memory_order_relaxed);
  }
  return v;
}
// what the launches read: a switch counts as off while a switch it refines is off
inline int effective_forms(int raw) {
  int v = raw;
  for (int id = 0; id < SW_COUNT; ++id)
    if ((raw & SWITCHES[id].needs) != SWITCHES[id].needs) v &= ~sw(id);
  return v;
}

// Smallest grid (in PAIRS of tiles) that takes the 128-point bf16 trunk; read once (CATRE_BF_PAIR_MIN overrides it for A/B
// measurements: 0 = always, a huge value = never).  512 pairs = two workgroups for each of the 256 CUs.
inline int bf_pair_min() {
  static const int v = [] {
    const char* e = getenv("CATRE_BF_PAIR_MIN");
    return e ? atoi(e) : 512;
  }();
  return v;
}
inline std::atomic<int> g_run_len{0};  // catre_screen_run_len: > 0 forces the length

// ---- the decision ------------------------------------------------------------------------------
// workgroups per 64-point tile of the encoder kernels: small grids split a tile's output channels over 2 or 4
// workgroups as long as that still fits one wave of workgroups on the 256 CUs
inline int row_split(int tiles) { return tiles * 4 <= 256 ? 4 : tiles * 2 <= 256 ? 2 : 1; }
// the fp32 encoder kernels also come with eight workgroups per tile (a single object: 32 tiles on 256 CUs)
inline int row_split8(int tiles) { return tiles * 8 <= 256 ? 8 : row_split(tiles); }

// Run length of k_trunk4sr.  One workgroup fits a CU, so a grid of R workgroups that each walk up to S tiles takes
// ceil(R / cus) * S tile slots.  The rule: the largest S <= 16 that takes no more slots than the one-tile grid's
// ceil(tiles / cus) - its last round is then as full as the one-tile grid's - else 1, the one-tile kernel k_trunk4sp.
// (B = 256, N = M = 1024 on 256 CUs: 16; B = 128: 16; B = 64: 8; B = 200: 1.)
inline int screen_run_rule(int B, int N, int M, int cus) {
  const int TN = tiles_of(N), TM = tiles_of(M);
  const long long slots1 = ((long long)B * (TN + TM) + cus - 1) / cus;
  for (int S = 16; S > 1; --S) {
    const long long R = (long long)B * ((TN + S - 1) / S + (TM + S - 1) / S);
    if ((R + cus - 1) / cus * S <= slots1) return S;
  }
  return 1;
}

enum { STAGE_STN3D, STAGE_STNKD, STAGE_TRUNK };
enum { MODE_F32, MODE_SPLIT, MODE_BF16 };  // (the fp16-operand mode takes the bf16 forms)
struct FormDecision {
  int form;       // catre_kernel_form
  int row_split;  // workgroups per tile
  int S;          // tiles per run of the trunk's run form, PAIRS per run (SP) of the STNs'; else 1
  int grid;       // workgroups
};

// Which kernel form one launch of `stage` takes.  Pure: everything it depends on is an argument.  `eff`: effective_forms;
// `run_len`: the forced run length, 0 = the rule on `cus` compute units.  The order is the point: run before one tile,
// fp16 screen before pooled before plain screen, those before the dense wide form; a probe forces the screened form
// on, and the STN probe keeps the one-pair kernels.  False for arguments no caller can produce.
inline bool form_decision(int stage, int mode, bool save, bool rows, bool probe, int B, int N, int M, int eff, int cus, int run_len,
                          int bf_min, FormDecision* out) {
  if (stage < STAGE_STN3D || stage > STAGE_TRUNK || mode < MODE_F32 || mode > MODE_BF16 || B <= 0 || N <= 0 || M < 0 || cus <= 0 ||
      N > (1 << 30) || M > (1 << 30) || run_len < 0 || run_len > 16 || eff < 0 || eff >= sw(SW_COUNT) || (long long)B * (tiles_of(N) + tiles_of(M)) > (1 << 27))
    return false;
  // rows come with saves only; a backward that recomputes its rows is fp32 STN; the probes are fp32 inference
  if ((rows && !save) || (save && !rows && (mode != MODE_F32 || stage == STAGE_TRUNK)) || (probe && (save || mode != MODE_F32)))
    return false;
  auto on = [eff](int id) { return (eff >> id & 1) != 0; };
  const bool trunk = stage == STAGE_TRUNK;
  const int TN = tiles_of(N), TM = tiles_of(M), tiles = B * (TN + TM), pairs = B * ((TN + 1) / 2 + (TM + 1) / 2);
  FormDecision d{CATRE_FORM_UNSUPPORTED, 1, 1, tiles};
  // full fp32 grids: the trunk's one wave per SIMD; the STN kernels on pairs of tiles (fewer pairs than CUs: one tile per
  // workgroup keeps the whole chip busy)
  const bool stn_wide = on(SW_STN4) && on(SW_STN_PAIR) && pairs >= 256;
  if (mode == MODE_BF16) {
    // grids that fill the chip twice over take PAIRS of tiles per workgroup (same bits, fewer prologues and weight fetches
    // per MFMA); below that the 64-point kernels spread better.  The trunk with saves has the pair kernel only.
    const bool pair = (save && trunk) || pairs >= bf_min;
    d.form = save ? (pair ? CATRE_FORM_TRAIN_BF_PAIR : CATRE_FORM_TRAIN_BF) : pair ? CATRE_FORM_BF_PAIR : CATRE_FORM_BF;
    if (pair) d.grid = pairs;
  } else if (save) {
    // the one-wave-per-SIMD STN does not pay WITH saves (470 MB of activation saves per launch want a second resident
    // workgroup); with no rows asked for, the inference pair kernel with the arg-max epilogue
    if (mode == MODE_SPLIT)
      d.form = CATRE_FORM_TRAIN_SPLIT;
    else if (trunk)
      d.form = on(SW_TRUNK4) && row_split8(tiles) == 1 ? CATRE_FORM_TRAIN_WAVE4 : CATRE_FORM_TRAIN_RS1;
    else if (!rows && stn_wide)
      d.form = CATRE_FORM_TRAIN_PAIR, d.grid = pairs;
    else
      d.form = CATRE_FORM_TRAIN_RS1;
  } else if (mode == MODE_SPLIT) {
    d.form = CATRE_FORM_SPLIT_RS, d.row_split = row_split(tiles), d.grid = tiles * d.row_split;
  } else {
    const bool full = row_split8(tiles) == 1, wide = full && (trunk ? on(SW_TRUNK4) : stn_wide);
    const bool screen = on(trunk ? SW_SCREEN : SW_SCREEN_STN), f16 = on(trunk ? SW_SCREEN_F16 : SW_F16_STN);
    const bool runs = trunk ? on(SW_SCREEN) && on(SW_SCREEN_RUN) : on(SW_RUN_STN) && !probe;
    const int S = wide && runs ? (run_len > 0 ? run_len : screen_run_rule(B, N, M, cus)) : 1;
    if (probe && !wide) {  // the screened forms exist for the wide kernels only
    } else if (S > 1) {
      d.form = f16 ? CATRE_FORM_RUN_F16 : CATRE_FORM_RUN;
      d.S = trunk ? S : S / 2;
      d.grid = trunk ? B * ((TN + S - 1) / S + (TM + S - 1) / S) : B * (((TN + 1) / 2 + d.S - 1) / d.S + ((TM + 1) / 2 + d.S - 1) / d.S);
    } else if (wide && (screen || probe)) {
      d.form = f16 ? CATRE_FORM_SCREEN_F16 : on(trunk ? SW_SCREEN_POOL : SW_POOL_STN) ? CATRE_FORM_SCREEN_POOL : CATRE_FORM_SCREEN;
      d.grid = trunk ? tiles : pairs;
    } else if (wide) {
      d.form = trunk ? CATRE_FORM_WAVE4 : CATRE_FORM_PAIR, d.grid = trunk ? tiles : pairs;
    } else if (!trunk && full && on(SW_STN4)) {
      d.form = CATRE_FORM_WAVE4;
    } else {
      d.form = CATRE_FORM_RS8, d.row_split = row_split8(tiles), d.grid = tiles * d.row_split;
    }
  }
  *out = d;
  return true;
}

// ---- packed weights ----------------------------------------------------------------------------

struct PackLayout {
  size_t stn_c2, stn_c3, fstn_c1, fstn_c2, fstn_c3, c2, c3, c4, rot_l0[2], rot_l1[2], ts_w0t, ts_w1t, sumwp, total;
  // bf16 fragment packs of the same matrices (catre_bf16.h), offsets in floats
  size_t bf_stn_c2, bf_stn_c3, bf_fstn_c1, bf_fstn_c2, bf_fstn_c3, bf_c2, bf_c3, bf_c4, bf_rot_l0[2], bf_rot_l1[2];
  // hi + lo bf16 fragment packs of the three split-mode layers (catre_split.h), offsets in floats
  size_t sp_stn_c2, sp_stn_c3, sp_fstn_c1, sp_fstn_c2, sp_fstn_c3, sp_c3, sp_c4, sp_rot_l0[2], sp_rot_l1[2];
  // fp16 fragment packs of the bf16 packs' matrices, same layout (CATRE_PACK_F16, CATRE_DTYPE_F16), offsets in floats
  size_t f16_stn_c2, f16_stn_c3, f16_fstn_c1, f16_fstn_c2, f16_fstn_c3, f16_c2, f16_c3, f16_c4, f16_rot_l0[2], f16_rot_l1[2];
  // screened max-pool of the fp32 path (catre_screen.h), part of the fp32 encoder pack: hi + lo bf16 fragments of conv4 and
  // its weight-row norms; the same of stn.conv3 and fstn.conv3 (k_stn3d_pair_s / k_stnkd_pair_s)
  size_t scr_c4, scr_nw4, scr_stn_c3, scr_fstn_c3, scr_nw_stn, scr_nw_fstn;
  // the fp16 screen of the same three layers (`screen_f16`): row-scaled fp16 fragments and the rows' 2^-scale (k_pack_screen_f16)
  size_t s16_c4, s16_stn_c3, s16_fstn_c3, s16_uw4, s16_uw_stn, s16_uw_fstn;
};

inline PackLayout pack_layout(int ts_in) {
  PackLayout L;
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += align_up(n, 64);
    return r;
  };
  L.stn_c2 = take(128 * 64);
  L.stn_c3 = take(1024 * 128);
  L.fstn_c1 = take(64 * 64);
  L.fstn_c2 = take(128 * 64);
  L.fstn_c3 = take(1024 * 128);
  L.c2 = take(128 * 64);
  L.c3 = take(512 * 128);
  L.c4 = take(1024 * 512);
  for (int h = 0; h < 2; ++h) {
    L.rot_l0[h] = take(256 * 64);
    L.rot_l1[h] = take(256 * 256);
  }
  L.sumwp = take(64);
  L.bf_stn_c2 = take(128 * 64 / 2);
  L.bf_stn_c3 = take(1024 * 128 / 2);
  L.bf_fstn_c1 = take(64 * 64 / 2);
  L.bf_fstn_c2 = take(128 * 64 / 2);
  L.bf_fstn_c3 = take(1024 * 128 / 2);
  L.bf_c2 = take(128 * 64 / 2);
  L.bf_c3 = take(512 * 128 / 2);
  L.bf_c4 = take(1024 * 512 / 2);
  for (int h = 0; h < 2; ++h) {
    L.bf_rot_l0[h] = take(256 * 64 / 2);
    L.bf_rot_l1[h] = take(256 * 256 / 2);
  }
  L.sp_stn_c2 = take(128 * 64);
  L.sp_stn_c3 = take(1024 * 128);
  L.sp_fstn_c1 = take(64 * 64);
  L.sp_fstn_c2 = take(128 * 64);
  L.sp_fstn_c3 = take(1024 * 128);
  L.sp_c3 = take(512 * 128);
  L.sp_c4 = take(1024 * 512);
  for (int h = 0; h < 2; ++h) {
    L.sp_rot_l0[h] = take(256 * 64);
    L.sp_rot_l1[h] = take(256 * 256);
  }
  L.f16_stn_c2 = take(128 * 64 / 2);
  L.f16_stn_c3 = take(1024 * 128 / 2);
  L.f16_fstn_c1 = take(64 * 64 / 2);
  L.f16_fstn_c2 = take(128 * 64 / 2);
  L.f16_fstn_c3 = take(1024 * 128 / 2);
  L.f16_c2 = take(128 * 64 / 2);
  L.f16_c3 = take(512 * 128 / 2);
  L.f16_c4 = take(1024 * 512 / 2);
  for (int h = 0; h < 2; ++h) {
    L.f16_rot_l0[h] = take(256 * 64 / 2);
    L.f16_rot_l1[h] = take(256 * 256 / 2);
  }
  L.scr_c4 = take(1024 * 512);
  L.scr_nw4 = take(1024);
  L.scr_stn_c3 = take(1024 * 128);
  L.scr_fstn_c3 = take(1024 * 128);
  L.scr_nw_stn = take(1024);
  L.scr_nw_fstn = take(1024);
  L.s16_c4 = take(1024 * 512 / 2);
  L.s16_stn_c3 = take(1024 * 128 / 2);
  L.s16_fstn_c3 = take(1024 * 128 / 2);
  L.s16_uw4 = take(3 * 1024);  // 2^-scale, then the rows' rounding errors and their sign-split form (k_screen_f16_dw)
  L.s16_uw_stn = take(3 * 1024);
  L.s16_uw_fstn = take(3 * 1024);
  // everything above is independent of ts_in (the stage entry points rely on that)
  L.ts_w0t = take((size_t)ts_in * 256);
  L.ts_w1t = take(256 * 256);
  L.total = o;
  return L;
}

// ---- one weight bundle per encoder stage -------------------------------------------------------
// a packed image; the kernel that takes it says how it reads it: fp32 (f32x4) or bf16 / fp16 fragments (u32x4)
struct Pack {
  const float* p;
  template <class T>
  operator const T*() const { return reinterpret_cast<const T*>(p); }
};
enum PackKind { PK_F32, PK_SPLIT, PK_BF16, PK_F16 };  // which image of a layer a compute mode reads
// what the screened forms read of a stage's last layer: fragments (row-scaled fp16, or hi + lo bf16), weight-row norms,
// the fp16 rows' 2^-scale and rounding errors
struct ScreenW {
  Pack wps;
  const float *nw, *uw;
};
struct Stn3dW {  // stn.conv1 .. conv3
  const float *w1, *b1, *b2, *b3;
  Pack w2, w3;
  ScreenW sc;
};
struct StnkdW {  // the encoder's conv1, then fstn.conv1 .. conv3
  const float *wc1, *bc1, *b1, *b2, *b3;
  Pack w1, w2, w3;
  ScreenW sc;
};
struct TrunkW {  // conv1 .. conv4
  const float *w1, *b1, *b2, *b3, *b4;
  Pack w2, w3, w4;
  ScreenW sc;
};

inline Stn3dW stn3d_weights(const float* const* prm, const float* packed, const PackLayout& L, PackKind k, bool f16_screen = false) {
  const size_t c2[] = {L.stn_c2, L.sp_stn_c2, L.bf_stn_c2, L.f16_stn_c2}, c3[] = {L.stn_c3, L.sp_stn_c3, L.bf_stn_c3, L.f16_stn_c3};
  return {prm[CATRE_P_STN_CONV1_W], prm[CATRE_P_STN_CONV1_B], prm[CATRE_P_STN_CONV2_B], prm[CATRE_P_STN_CONV3_B], {packed + c2[k]},
          {packed + c3[k]}, {{packed + (f16_screen ? L.s16_stn_c3 : L.scr_stn_c3)}, packed + L.scr_nw_stn, packed + L.s16_uw_stn}};
}
inline StnkdW stnkd_weights(const float* const* prm, const float* packed, const PackLayout& L, PackKind k, bool f16_screen = false) {
  const size_t c1[] = {L.fstn_c1, L.sp_fstn_c1, L.bf_fstn_c1, L.f16_fstn_c1}, c2[] = {L.fstn_c2, L.sp_fstn_c2, L.bf_fstn_c2, L.f16_fstn_c2},
               c3[] = {L.fstn_c3, L.sp_fstn_c3, L.bf_fstn_c3, L.f16_fstn_c3};
  return {prm[CATRE_P_CONV1_W], prm[CATRE_P_CONV1_B], prm[CATRE_P_FSTN_CONV1_B], prm[CATRE_P_FSTN_CONV2_B], prm[CATRE_P_FSTN_CONV3_B],
          {packed + c1[k]}, {packed + c2[k]}, {packed + c3[k]},
          {{packed + (f16_screen ? L.s16_fstn_c3 : L.scr_fstn_c3)}, packed + L.scr_nw_fstn, packed + L.s16_uw_fstn}};
}
inline TrunkW trunk_weights(const float* const* prm, const float* packed, const PackLayout& L, PackKind k, bool f16_screen = false) {
  // (conv2 has no split image: K = 64 stays on the fp32 pack)
  const size_t c2[] = {L.c2, L.c2, L.bf_c2, L.f16_c2}, c3[] = {L.c3, L.sp_c3, L.bf_c3, L.f16_c3}, c4[] = {L.c4, L.sp_c4, L.bf_c4, L.f16_c4};
  return {prm[CATRE_P_CONV1_W], prm[CATRE_P_CONV1_B], prm[CATRE_P_CONV2_B], prm[CATRE_P_CONV3_B], prm[CATRE_P_CONV4_B], {packed + c2[k]},
          {packed + c3[k]}, {packed + c4[k]}, {{packed + (f16_screen ? L.s16_c4 : L.scr_c4)}, packed + L.scr_nw4, packed + L.s16_uw4}};
}

}  // namespace catre_host
