"""Time and parity of the tracking kernels (``catre_amd/tracking.py``, ``csrc/catre_track.h``) on the GPU:

    python profiles/track_probe.py --out DIR     # DIR/track_time.json, DIR/track_parity.json

Kernel time: ``catre_nn_stats`` through the C ABI on preallocated buffers (posed dst, tau, no per-point outputs), I = 256
and I = 1 at N = M = 1024, HIP events around ``--reps`` back-to-back calls after a warm-up, five windows.  A call is two
launches (the pair sweep and the per-instance finish).

Step time: ``Tracker.step`` on a 480x640 synthetic frame (``synth.make_depth_scene``), default model (N = M = 1024, K = 4),
I = 1 and I = 8: events around whole steps, and around the three phases of the same composition written out (crop +
sample, refine, score + gate; it is bit-identical to ``step``, ``tests/test_track.py``).  The phases are launched from
Python, so at I = 1 they are host-bound: the numbers are what a caller sees, not kernel sums.  Untrained seeded weights:
the track drifts, which does not change what is launched.

Parity: the worst deviations over the cases ``tests/test_track.py`` asserts on (``tests/track_cases.py`` yields them to
both), with the bounds they are held to."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 1024


def windows(fn, reps, n_windows=5):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(n_windows):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def kernel_time(I, reps):
    import torch

    from catre_amd import hip

    lib = hip.load()
    g = torch.Generator().manual_seed(I)
    src = (torch.rand(I, N, 3, generator=g) * 0.3 - 0.15).cuda()
    dst = (torch.rand(I, N, 3, generator=g) * 0.3 - 0.15).cuda()
    pose = torch.eye(3, 4).repeat(I, 1, 1).cuda()
    scale, tau = torch.ones(I, 3).cuda(), torch.full((I,), 0.02).cuda()
    mean_d, inlier = torch.empty(I).cuda(), torch.empty(I).cuda()
    nbytes = lib.catre_nn_stats_workspace_bytes(I, N, N)
    ws = torch.empty(nbytes // 8, dtype=torch.float64).cuda()
    st = hip.stream_ptr(src.device)
    nul = ctypes.c_void_p(0)

    def call():
        hip.check(lib.catre_nn_stats(hip.ptr(src), N, hip.ptr(dst), N, nul, nul, hip.ptr(pose), hip.ptr(scale), 0, hip.ptr(tau), I,
                                     hip.ptr(mean_d), hip.ptr(inlier), nul, nul, hip.ptr(ws), nbytes, st), "catre_nn_stats")

    for _ in range(20):
        call()
    torch.cuda.synchronize()
    w = windows(call, reps)
    pairs = I * N * N
    ms = float(np.median(w))
    return dict(instances=I, n_src=N, n_dst=N, ms_per_call=round(ms, 5), ms_windows=[round(x, 5) for x in w], calls_per_window=reps,
                pairs_per_call=pairs, gpairs_per_s=round(pairs / ms / 1e6, 2), gflop_per_s_at_8_flop_per_pair=round(8 * pairs / ms / 1e6, 1))


def step_time(I, model, reps):
    import torch

    from catre_amd import pcl_prep, synth, tracking

    scene = synth.make_depth_scene(H=480, W=640, n_inst=I, seed=1)
    inputs = synth.make_inputs(I, N, N, seed=2)
    depth, K = scene["depth"].cuda(), scene["K"]
    kps, mean_scales = inputs["obj_kps"].cuda(), inputs["obj_mean_scales"].cuda()
    pose0, scale0 = scene["poses"].cuda(), scene["scales"].cuda()
    tr = tracking.Tracker(model, kps, K, mean_scales=mean_scales, min_inlier=0.0).reset(pose0, scale0)
    for _ in range(10):
        tr.step(depth)
    torch.cuda.synchronize()
    tr.reset(pose0, scale0)
    w = windows(lambda: tr.step(depth), reps)

    # the same composition with events between the phases
    Kd = K.cuda().expand(I, 3, 3).contiguous()
    zero = torch.zeros(1, 480, 640, dtype=torch.uint8, device="cuda")
    pose, scale, age = pose0.clone(), scale0.clone(), torch.zeros(I, dtype=torch.int32, device="cuda")
    n_iter = tr.n_iter
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    for t in range(reps):
        ev[t][0].record()
        pcl, _, counts = pcl_prep.sample_frames(depth[None], K, [0] * I, pose, scale, labels=zero, label_of=[0] * I, ratio=tr.ratio,
                                                num_points=N, use_ball=True, sample="device", seed=t, return_pixels=True)
        ev[t][1].record()
        out = model.refine({"pcl": pcl, "obj_kps": kps, "obj_pose_est": pose, "obj_scale_est": scale, "K": Kd,
                            "obj_mean_scales": mean_scales}, n_iter=n_iter)
        ev[t][2].record()
        sc = tracking.fit_score(pcl, kps, out[f"pose_{n_iter}"], out[f"scale_{n_iter}"], 0.1)
        pose, scale, _, age = tracking.track_gate(out[f"pose_{n_iter}"], out[f"scale_{n_iter}"], pose, scale, counts,
                                                  sc.inlier_obs, sc.d_obs, age, 0.0, True)
        ev[t][3].record()
    torch.cuda.synchronize()
    ph = [float(np.median([ev[t][k].elapsed_time(ev[t][k + 1]) for t in range(reps)])) for k in range(3)]
    return dict(instances=I, frame="480x640", points=N, n_iter=n_iter, step_ms=round(float(np.median(w)), 4),
                step_ms_windows=[round(x, 4) for x in w], steps_per_window=reps,
                phase_ms_median=dict(crop_sample=round(ph[0], 4), refine=round(ph[1], 4), score_gate=round(ph[2], 4)),
                score_gate_share_of_refine=round(ph[2] / ph[1], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--step-reps", type=int, default=300)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    import torch

    from catre_amd import synth
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    assert torch.cuda.is_available(), "track_probe.py measures on a HIP device"
    devinfo = dict(device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName)
    cfg = default_cfg(device="cuda:0")
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.cuda() for k, v in sd.items()}, strict=True)
    model.eval()

    res = dict(what="catre_nn_stats and Tracker.step", **devinfo,
               kernel=[kernel_time(256, a.reps), kernel_time(1, a.reps)],
               kernel_note="HIP events around back-to-back C-ABI calls on preallocated buffers after 20 warm-up calls; a call "
                           "is two launches; at I = 1 (four workgroups, each wave alone on its SIMD) the time holds those two "
                           "launches and the latency of one 1024-point sweep, not a throughput",
               step=[step_time(1, model, a.step_reps), step_time(8, model, a.step_reps)],
               step_note="step_ms: HIP events around back-to-back Tracker.step calls after 10 warm-up steps, Python wrapper "
                         "and allocations included; phase_ms_median: per-step events between the phases of the same "
                         "composition written out; refine at I = 1 is the one-object K = 4 refine the README quotes")
    json.dump(res, open(os.path.join(a.out, "track_time.json"), "w"), indent=1)
    print(json.dumps(res))

    from tests import track_cases as C

    par = {}
    for name, transforms in (("edges_plain", False), ("edges_posed", True)):
        rows = list(C.edge_rows(transforms))
        par[name] = C.worst(C.worst_point(r) for r in rows)
        par[name + "_mean"] = C.worst((r["mean_dev"], r["mean_bound"]) for r in rows)
    rows = list(C.add_rows())
    for key in ("add", "adi"):
        par[key] = C.worst((r["dev"], r["bound"]) for r in rows if r["key"] == key)
    par = dict(what="worst deviation over the cases of tests/track_cases.py (largest deviation / bound), with the bound at that "
                    "point; edges: catre_nn_stats vs the fp64 restatement tests/track_ref.py, plain = without transforms (bound "
                    "8 * 2^-24 * d), posed = with (bound 16 * 2^-24 * (max |p| + max |q|)); add / adi: "
                    "evaluation.add_errors vs tests/golden/pose_error_add.npz, written by the unmodified reference",
               **devinfo, **par)
    json.dump(par, open(os.path.join(a.out, "track_parity.json"), "w"), indent=1)
    print(json.dumps(par))


if __name__ == "__main__":
    main()
