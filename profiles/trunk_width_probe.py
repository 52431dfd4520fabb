"""Kernel time of the dense trunk at conv4 width D (``catre_trunk_w``, csrc/catre_trunkw.h) next to the shipped trunk:

    python profiles/trunk_width_probe.py [--out profiles/trunk_width_kernel_times.json]

B = 256, N = M = 1024 (the headline shape: 8192 tiles of 64 points).  Per entry: device events around `reps` back-to-back
calls after `warmup` calls, the mean per call in microseconds (a call = the trunk kernel + the tile-maxima reduction, a few
microseconds), and the conv4 FLOP the call issues - 2 x 512 x D per point - per second against the 157.3 TFLOP/s fp32 matrix
peak.  conv1..conv3 and the pointfeat GEMM (0.16 GFLOP per cloud pair, the same at every D) are not counted, so the figure
is a lower bound of the matrix rate at small D, where they are most of the kernel.  Entries: ``catre_trunk_w`` at D = 64 ..
1024; the shipped ``catre_trunk`` in its default (screened, one wave per SIMD) form - its issued FLOP are not 2 x 512 x 1024
per point, the screen runs on the bf16 pipe, so only its time is comparable; and the dense 8-wave ``k_trunk<1>`` (form
switch ``trunk4`` off), the kernel ``catre_trunk_w`` at D = 1024 restates."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from catre_amd import hip, synth  # noqa: E402
from catre_amd import runtime as RT  # noqa: E402
from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes  # noqa: E402
from catre_amd.config import default_cfg  # noqa: E402

PEAK_TFLOPS = 157.3
DEV = "cuda:0"


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trunk_width_kernel_times.json"))
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    B, N, M = args.B, args.N, args.M
    lib, dev = hip.load(), torch.device(DEV)
    cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=2, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=True)
    model.load_state_dict({k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()}, strict=True)
    rt = model.eval()._runtime()
    batch = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=5).items()}
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)
    st = rt.stage_pointnet(x, tfd, True)
    trans, t64 = st["trans"].contiguous(), st["trans_feat"].contiguous()
    pts = hip.points_desc(x, tfd)
    prm, packed = rt.params(dev, hip.PACK_ALL)
    ws = rt.workspace(B, N, M, dev)
    sp = hip.stream_ptr(dev)
    points = B * (N + M)
    pointfeat = torch.empty(points, 64, dtype=torch.float32, device=DEV)
    entries = []

    def entry(name, D, us, counted=True):
        flop = 2.0 * 512 * D * points
        e = dict(kernel=name, out_dim=D, us=round(us, 1))
        if counted:
            e["conv4_tflops"] = round(flop / us * 1e-6, 2)
            e["conv4_frac_of_fp32_matrix_peak"] = round(flop / us * 1e-6 / PEAK_TFLOPS, 4)
        entries.append(e)
        print(e)

    gfeat = torch.empty(2 * B, 1088, dtype=torch.float32, device=DEV)

    def shipped():
        hip.check(lib.catre_trunk(ctypes.byref(pts), hip.ptr(trans), hip.ptr(t64), prm, hip.ptr(packed), hip.ptr(gfeat),
                                  hip.ptr(pointfeat), hip.ptr(ws), ws.numel(), B, N, M, sp), "catre_trunk")

    entry("catre_trunk, default form (screened max-pool, one wave per SIMD)", 1024, timed(shipped, args.warmup, args.reps),
          counted=False)
    want = gfeat.clone()
    prev = hip.form_switch("trunk4", False)
    try:
        entry("catre_trunk, dense 8-wave k_trunk<1> (form switch trunk4 off)", 1024, timed(shipped, args.warmup, args.reps))
    finally:
        hip.form_switch("trunk4", prev)
    assert torch.equal(gfeat, want)
    iw, ib = hip.PARAM_KEYS.index("pcl_net.conv4.weight"), hip.PARAM_KEYS.index("pcl_net.conv4.bias")
    for D in hip.OUT_DIMS:
        tensors = list(rt._param_keep)
        tensors[iw], tensors[ib] = tensors[iw][:D].contiguous(), tensors[ib][:D].contiguous()
        prm_w = hip.param_array(tensors)
        packed_w = torch.empty(lib.catre_packed_floats_w(D), dtype=torch.float32, device=DEV)
        hip.check(lib.catre_pack_encoder_w(prm_w, D, hip.ptr(packed_w), packed_w.numel(), sp), "catre_pack_encoder_w")
        g = torch.empty(2 * B, D + 64, dtype=torch.float32, device=DEV)

        def wide():
            hip.check(lib.catre_trunk_w(ctypes.byref(pts), hip.ptr(trans), hip.ptr(t64), prm_w, hip.ptr(packed_w), D, hip.ptr(g),
                                        hip.ptr(pointfeat), hip.ptr(ws), ws.numel(), B, N, M, sp), "catre_trunk_w")

        entry("catre_trunk_w (k_trunkw)", D, timed(wide, args.warmup, args.reps))
        assert torch.equal(g[:, :D], want[:, :D]) and torch.equal(g[:, D:], want[:, 1024:])   # the timed calls computed the shipped bits
    out = dict(what="device events around back-to-back calls, mean per call; conv4 FLOP = 2 x 512 x out_dim per point",
               shape=dict(B=B, N=N, M=M, tiles=points // 64), warmup=args.warmup, reps=args.reps,
               device=torch.cuda.get_device_name(0), fp32_matrix_peak_tflops=PEAK_TFLOPS, entries=entries)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
