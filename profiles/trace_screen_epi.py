"""Sub-phase split of the screened max-pool epilogue (selection, list build, replay, scan, store) of the pooled fp16-screen
kernels: trunk conv4, stn.conv3 and fstn.conv3, with kernel-form switch `screen_epi` off and on in one process.

Needs the instrumented library (`make -C catre_amd/csrc TRACE=1`), whose kernels stamp the shader clock (SCREEN_STAMP of
csrc/catre_screen.h, turned on by catre_debug_knob 3):
    CATRE_HIP_LIB=catre_amd/csrc/libcatre_hip_trace.so python profiles/trace_screen_epi.py [out.txt]
One refine iteration of the headline batch (B = 256, N = M = 1024, recipe weights) per arm, candidate counters off,
steady-state tiles (the first and the last quarter of the grid dropped), cycles per (wave, tile)."""
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
prev = hip.form_switch("screen_epi")
for epi in (False, True):
    hip.form_switch("screen_epi", epi)
    buf.zero_()
    hip.check(lib.catre_debug_trunk_trace(ctypes.c_void_p(buf.data_ptr())), "catre_debug_trunk_trace")
    hip.check(lib.catre_debug_knob(3, 1), "catre_debug_knob 3")
    model.refine(batch, n_iter=1)
    torch.cuda.synchronize()
    hip.check(lib.catre_debug_trunk_trace(None), "catre_debug_trunk_trace")
    lines.append(f"== screen_epi {'on' if epi else 'off'}: cycles per (wave, tile), mean over waves and steady-state tiles")
    for layer, kname in enumerate(("k_trunk4sr16", "k_stn3d_pair_sr16", "k_stnkd_pair_sr16")):
        t = buf[layer << 22:(layer << 22) + tiles * 64].view(tiles, 8, 8)[tiles // 4:3 * tiles // 4, 4:, :6].cpu().double()
        ok = (t != 0).all(2).all(1)
        t = t[ok]
        d = t[:, :, 1:] - t[:, :, :-1]
        tot = t[:, :, 5] - t[:, :, 0]
        lines.append(f"  {kname + ('e' if epi else ''):20s} " + "  ".join(f"{n} {d[:, :, i].mean():7.0f}" for i, n in enumerate(names))
                     + f"  | whole epilogue {tot.mean():7.0f}  ({int(ok.sum())} tiles)")
hip.form_switch("screen_epi", prev)
text = "\n".join(lines) + "\n"
print(text, end="")
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(text)
