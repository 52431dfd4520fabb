"""Where the time goes with kernel-form switch `screen_da` off and on (and its STN arm), in one process of the instrumented
library: the phases of the pooled fp16-screen kernels per (wave, tile) - row norms (+ the measuring pass) and sweep,
selection, list build, replay, scan, store - for trunk conv4, stn.conv3 and fstn.conv3.

Needs the instrumented library (`make -C catre_amd/csrc TRACE=1`), whose kernels stamp the shader clock (TRUNK_STAMP of
csrc/catre_enc.h, SCREEN_STAMP of csrc/catre_screen.h, turned on by catre_debug_knob 3):
    CATRE_HIP_LIB=catre_amd/csrc/libcatre_hip_trace.so python profiles/trace_screen_da.py [out.txt]
One refine iteration of the headline batch (B = 256, N = M = 1024, recipe weights) per arm, candidate counters off,
steady-state tiles (the first and the last quarter of the grid dropped), cycles per (wave, tile).
Trunk: "norms+sweep" is TRUNK_STAMP 5 -> 6 (the deferred pointfeat stores, screen_row_norms, the barrier and the fp16 sweep).
STN kernels: "norms" is SCREEN_STAMP 6 -> 7 (screen_row_norms of both tiles of the pair and the barrier), stamped at the
pair's first tile; the sweep is not stamped there."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catre_amd import hip, synth  # noqa: E402
from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes  # noqa: E402
from catre_amd.config import default_cfg  # noqa: E402

B, N, M = 256, 1024, 1024
cfg = default_cfg(device="cuda:0")
model, _ = build_model_optimizer(cfg, is_test=True)
sd = synth.recipe_state_dict(expected_state_shapes(cfg))
model.load_state_dict({k: v.cuda() for k, v in sd.items()})
model.eval()
batch = {k: v.cuda() for k, v in synth.make_inputs(B, N, M, seed=1).items()}
model.refine(batch, n_iter=1)
tiles = B * 32
lib = hip.load()
buf = torch.zeros((1 << 24) + tiles * 8 * 16, dtype=torch.int64, device="cuda")
hip.check(lib.catre_debug_knob(2, 0), "catre_debug_knob (needs the TRACE=1 library)")  # the counters' atomics off
names = ("selection", "list build", "replay", "scan", "store")
lines = []
prev = [hip.form_switch(n) for n in ("screen_da", "screen_da_stn")]
for da, stn in ((False, False), (True, False), (True, True)):
    hip.form_switch("screen_da", da)
    hip.form_switch("screen_da_stn", stn)
    buf.zero_()
    hip.check(lib.catre_debug_trunk_trace(ctypes.c_void_p(buf.data_ptr())), "catre_debug_trunk_trace")
    hip.check(lib.catre_debug_knob(3, 1), "catre_debug_knob 3")
    model.refine(batch, n_iter=1)
    torch.cuda.synchronize()
    hip.check(lib.catre_debug_trunk_trace(None), "catre_debug_trunk_trace")
    lines.append(f"== screen_da {'on' if da else 'off'}, screen_da_stn {'on' if stn else 'off'}: cycles per (wave, tile), mean over "
                 "waves and steady-state tiles")
    for layer, kname in enumerate(("k_trunk4sr16e", "k_stn3d_pair_sr16e", "k_stnkd_pair_sr16e")):
        full = buf[layer << 22:(layer << 22) + tiles * 64].view(tiles, 8, 8)[tiles // 4:3 * tiles // 4].cpu().double()
        t = full[:, 4:, :6]
        ok = (t != 0).all(2).all(1)
        t = t[ok]
        d = t[:, :, 1:] - t[:, :, :-1]
        tot = t[:, :, 5] - t[:, :, 0]
        if layer == 0:
            w = full[:, :4, :]
            okw = (w[:, :, 5:8] != 0).all(2).all(1)
            head = f"norms+sweep {(w[okw][:, :, 6] - w[okw][:, :, 5]).mean():7.0f}  whole tile {(w[okw][:, :, 7] - w[okw][:, :, 0]).mean():7.0f}"
        else:
            n = full[:, 4:, 6:8]
            okn = (n != 0).all(2).all(1)      # stamped at the first tile of a pair
            head = f"norms (pair) {(n[okn][:, :, 1] - n[okn][:, :, 0]).mean():7.0f}"
        lines.append(f"  {kname:20s} {head}  " + "  ".join(f"{n} {d[:, :, i].mean():7.0f}" for i, n in enumerate(names))
                     + f"  | whole epilogue {tot.mean():7.0f}  ({int(ok.sum())} tiles)")
for n, p in zip(("screen_da", "screen_da_stn"), prev):
    hip.form_switch(n, p)
text = "\n".join(lines) + "\n"
print(text, end="")
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(text)
