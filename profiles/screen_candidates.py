"""Candidate-count histograms and further-rounds shares of the three screened layers (kernel-form switches `screen` and
`screen_stn`: trunk conv4, stn.conv3, fstn.conv3) on the bench inputs.  With `screen_pool` on (the default; CATRE_SCREEN_POOL=0
for the per-channel replay) the kernels that replay from one list per wave report list entries and rounds of 64 per
(wave, tile) instead of trips per 32-channel block.  With `screen_run` on (the default; CATRE_SCREEN_RUN=0 for one tile per
workgroup, CATRE_SCREEN_RUN_STN=0 for the trunk alone) a workgroup carries the running maximum over a run of tiles: fewer
entries, channels without a candidate (bin 0) and (wave, tile) units whose list is empty.  With `screen_f16` on (the default;
CATRE_SCREEN_F16=0 for the split-bf16 screen, CATRE_SCREEN_F16_STN=0 for the trunk alone) the pooled and run kernels screen
with one fp16 product: a wider eps, more entries.

Needs the instrumented library (`make -C catre_amd/csrc TRACE=1`), whose screened kernels count while they run:
    CATRE_HIP_LIB=catre_amd/csrc/libcatre_hip_trace.so python profiles/screen_candidates.py [out.txt]
One K = 4 refine of the headline batch (B = 256, N = M = 1024, `synth.make_inputs(seed=1000)`, recipe weights)."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catre_amd import hip, synth  # noqa: E402
from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes  # noqa: E402
from catre_amd.config import default_cfg  # noqa: E402

B, N, M, K = 256, 1024, 1024, 4
cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=K, device="cuda:0")
model, _ = build_model_optimizer(cfg, is_test=True)
sd = synth.recipe_state_dict(expected_state_shapes(cfg))
model.load_state_dict({k: v.cuda() for k, v in sd.items()}, strict=True)
model.eval()
batch = {k: v.cuda() for k, v in synth.make_inputs(B, N, M, seed=1000).items()}
lib = hip.load()
hip.form_switch("screen", True)
hip.form_switch("screen_stn", True)
model.refine(batch, n_iter=K)   # warm-up (packs the weights)
torch.cuda.synchronize()
cnt = (ctypes.c_ulonglong * (3 * 64))()
hip.check(lib.catre_debug_screen_counts(cnt, 1), "catre_debug_screen_counts (needs the TRACE=1 library)")
model.refine(batch, n_iter=K)
torch.cuda.synchronize()
hip.check(lib.catre_debug_screen_counts(cnt, 1), "catre_debug_screen_counts")
pool = hip.form_switch("screen_pool")
run = pool and hip.form_switch("screen_run")
run_stn = run and os.environ.get("CATRE_SCREEN_RUN_STN", "1") != "0"
f16 = pool and hip.form_switch("screen_f16")
f16_stn = f16 and os.environ.get("CATRE_SCREEN_F16_STN", "1") != "0"
S = (hip.screen_run_len() or hip.screen_run_rule(B, N, M, torch.cuda.get_device_properties(0).multi_processor_count)) if run else 1
lines = [f"B={B} N=M={N} K={K} refine, make_inputs(seed=1000), recipe weights; screen_pool {'on' if pool else 'off'}; "
         f"screen_run {'on, run length ' + str(S) + (' (STN kernels: ' + ('on' if run_stn else 'off') + ')') if run and S > 1 else 'off'}; "
         f"screen_f16 {'on (STN kernels: ' + ('on' if f16_stn else 'off') + ')' if f16 else 'off'}; "
         "per-channel replay: chains a lane carries at once: 4"]
for row, name in enumerate(("trunk conv4 (k_trunk4s)", "stn.conv3 (k_stn3d_pair_s)", "fstn.conv3 (k_stnkd_pair_s)")):
    c = list(cnt)[64 * row:64 * row + 64]
    pooled = c[51] > 0   # only the pooled replay counts rounds
    if pooled:
        name = name.replace("_s)", "_sp)").replace("k_trunk4s", "k_trunk4sp")
        if run and S > 1 and (row == 0 or run_stn):
            name = name.replace("sp)", "sr)")
        if f16 and (row == 0 or f16_stn):
            name = name.replace(")", "16)")
    lines.append(f"screened {name}")
    tot = sum(c[:32])
    mean = sum(i * v for i, v in enumerate(c[:32])) / max(tot, 1)
    lines.append(f"candidates per (tile, channel): {tot} pairs, mean {mean:.4f} (bin 31 = 31 and more)")
    for i, v in enumerate(c[:32]):
        if v:
            lines.append(f"  {i:2d}: {v:10d}  {v / tot:.6f}")
    if pooled:
        lines.append(f"list entries per (wave, tile): mean {c[50] / max(c[49], 1):.2f}; rounds of 64 entries: mean "
                     f"{c[51] / max(c[49], 1):.4f} over {c[49]} units (bin 15 = 15 and more)")
        for i, v in enumerate(c[32:48]):
            if v:
                lines.append(f"  {i:2d}: {v:10d}  {v / max(c[49], 1):.6f}")
        lines.append(f"(wave, tile) units whose list filled up (replayed in more than one batch): {c[48]} of {c[49]}")
        lines.append(f"(wave, tile) units with an empty list: {c[52]} of {c[49]}")
        continue
    tt = sum(c[32:48])
    tmean = sum(i * v for i, v in enumerate(c[32:48])) / max(tt, 1)
    lines.append(f"replay trips per (wave, tile, 32-channel block): {tt} blocks, mean {tmean:.4f} (bin 15 = 15 and more)")
    for i, v in enumerate(c[32:48]):
        if v:
            lines.append(f"  {i:2d}: {v:10d}  {v / tt:.6f}")
    lines.append(f"(wave, tile) units with a block of more than 4 trips (a further replay round): {c[48]} of {c[49]} = "
                 f"{c[48] / max(c[49], 1):.5f}")
text = "\n".join(lines) + "\n"
print(text, end="")
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(text)
