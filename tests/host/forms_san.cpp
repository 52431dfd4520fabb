// Stand-alone driver of the HIP-free host code of csrc/catre_forms.h for a sanitizer build
// (-fsanitize=address,undefined): the switch table, the form decision over every switch state and the weight-bundle
// builders on real buffers.  tests/test_form_decision_host.py compiles and runs it.
#include <cstdio>
#include <vector>

#include "../../catre_amd/csrc/catre_forms.h"

using namespace catre_host;

int main() {
  long long sum = 0;
  // the table: environment read, raw word, refinement
  const int raw0 = forms();
  if (raw0 < 0 || raw0 >= sw(SW_COUNT)) return 1;
  for (int raw = 0; raw < sw(SW_COUNT); ++raw) {
    const int eff = effective_forms(raw);
    if ((eff & ~raw) != 0 || effective_forms(eff) != eff) return 2;  // only clears bits; idempotent
    sum += eff;
  }
  // the decision: every switch state, stage, mode and caller kind at shapes on both sides of the thresholds
  const int shapes[][3] = {{1, 1024, 1024}, {5, 1024, 1024}, {64, 64, 64}, {65, 64, 64}, {128, 64, 64}, {255, 64, 0},
                           {256, 1024, 1024}, {200, 960, 448}, {33, 100, 70}, {1 << 20, 1 << 20, 1 << 20}, {2147483647, 2147483647, 2147483647}};
  for (const auto& s : shapes)
    for (int raw = 0; raw < sw(SW_COUNT); ++raw)
      for (int stage = -1; stage <= 3; ++stage)
        for (int mode = 0; mode <= 2; ++mode)
          for (int kind = 0; kind < 4; ++kind) {  // inference, probe, training with rows, training without
            FormDecision d{-1, -1, -1, -1};
            const bool ok = form_decision(stage, mode, kind >= 2, kind == 2, kind == 1, s[0], s[1], s[2], effective_forms(raw),
                                          raw & 1 ? 256 : 64, raw % 17, bf_pair_min(), &d);
            if (ok && (d.form < CATRE_FORM_UNSUPPORTED || d.form > CATRE_FORM_TRAIN_BF || d.row_split < 1 || d.S < 1 || d.grid < 1))
              return 3;
            sum += ok ? d.form + d.grid : 0;
          }
  // the bundles: every pack kind, with and without the fp16 screen, each pointer read at its first element
  const PackLayout L = pack_layout(1);
  std::vector<float> packed(L.total, 1.f), param(4, 2.f);
  std::vector<const float*> prm(CATRE_P_COUNT, param.data());
  for (int k = PK_F32; k <= PK_F16; ++k)
    for (int f16 = 0; f16 < 2; ++f16) {
      const Stn3dW a = stn3d_weights(prm.data(), packed.data(), L, (PackKind)k, f16);
      const StnkdW b = stnkd_weights(prm.data(), packed.data(), L, (PackKind)k, f16);
      const TrunkW c = trunk_weights(prm.data(), packed.data(), L, (PackKind)k, f16);
      const float* ps[] = {a.w1, a.b1, a.w2, a.b2, a.w3, a.b3, a.sc.wps, a.sc.nw, a.sc.uw, b.wc1, b.bc1, b.w1, b.b1, b.w2, b.b2,
                           b.w3, b.b3, b.sc.wps, b.sc.nw, b.sc.uw, c.w1, c.b1, c.w2, c.b2, c.w3, c.b3, c.w4, c.b4, c.sc.wps,
                           c.sc.nw, c.sc.uw};
      for (const float* p : ps) sum += (long long)*p;
      sum += (long long)a.sc.uw[2 * 1024 - 1] + (long long)c.sc.uw[2 * 1024 - 1] + (long long)((const float*)c.w4)[1024 * 512 / 2 - 1];
    }
  std::printf("forms_san ok %lld\n", sum);
  return 0;
}
