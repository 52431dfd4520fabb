"""Time of trimmed ICP (``catre_amd/icp.py``, ``csrc/catre_icp.h``) on the GPU:

    python profiles/icp_time.py --out profiles     # profiles/icp_time.json

``catre_icp`` (n_iter = 20), ``catre_icp_step`` and ``catre_nn_stats`` through the C ABI on preallocated buffers, at I = 256
and I = 1 instances of N = M = 1024 points (``synth.make_inputs``: a posed prior with 2 mm noise seen from 10 degrees / 1 cm
off).  HIP events around ``--reps`` back-to-back calls after a warm-up of one second of the same calls, five windows; the
median window is quoted, all five are stored (the method of ``profiles/bop_time.py``).

``step_share`` = one step / (one step + one neighbour search): what the new kernel adds to an iteration.

Alongside, in the same process and for scale: the one-object K = 4 refine, ``tracking.fit_score`` and ``icp.icp`` through their
Python wrappers with per-call events (median, wrappers and allocations included), and ``Tracker.step`` on a synthetic depth
frame with and without ``recover="icp"``."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from profiles.bop_time import per_call_ms, windows  # noqa: E402

N, N_ITER = 1024, 20


def icp_time(I, reps, step_reps):
    import torch

    from catre_amd import hip, synth

    lib = hip.load()
    d = synth.make_inputs(I, N, N, seed=4)
    pcl, kps, pose, scale = (d[k].cuda().contiguous() for k in ("pcl", "obj_kps", "obj_pose_est", "gt_scale"))
    dev, nul = pcl.device, ctypes.c_void_p(0)
    st = hip.stream_ptr(dev)
    nbytes = lib.catre_icp_workspace_bytes(I, N, N, N_ITER)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    pose_out, scale_out = torch.empty_like(pose), torch.empty_like(scale)
    rmse = torch.empty(N_ITER + 1, I, device=dev)
    kept = torch.empty(N_ITER + 1, I, dtype=torch.int32, device=dev)
    status = torch.zeros(I, dtype=torch.int32, device=dev)

    def loop():
        hip.check(lib.catre_icp(hip.ptr(pcl), N, nul, hip.ptr(kps), N, hip.ptr(pose), hip.ptr(scale), nul, 0.7, 0, N_ITER, I,
                                hip.ptr(pose_out), hip.ptr(scale_out), hip.ptr(rmse), hip.ptr(kept), hip.ptr(status), hip.ptr(ws),
                                nbytes, st), "catre_icp")

    nn_bytes = lib.catre_nn_stats_workspace_bytes(I, N, N)
    nn_ws = torch.empty(nn_bytes // 8, dtype=torch.float64, device=dev)
    mean_d = torch.empty(I, device=dev)
    nn_d2 = torch.empty(I, N, device=dev)
    nn_j = torch.empty(I, N, dtype=torch.int32, device=dev)

    def nn():
        hip.check(lib.catre_nn_stats(hip.ptr(pcl), N, hip.ptr(kps), N, nul, nul, hip.ptr(pose), hip.ptr(scale), 0, nul, I,
                                     hip.ptr(mean_d), nul, hip.ptr(nn_d2), hip.ptr(nn_j), hip.ptr(nn_ws), nn_bytes, st), "catre_nn_stats")

    step_status = torch.zeros(I, dtype=torch.int32, device=dev)

    def step():
        hip.check(lib.catre_icp_step(hip.ptr(pcl), N, nul, hip.ptr(kps), N, hip.ptr(pose), hip.ptr(scale), hip.ptr(nn_d2), hip.ptr(nn_j),
                                     nul, 0.7, 0, 1, I, hip.ptr(pose_out), hip.ptr(scale_out), hip.ptr(rmse), hip.ptr(kept), nul,
                                     hip.ptr(step_status), st), "catre_icp_step")

    nn()
    torch.cuda.synchronize()
    out = {}
    for name, fn, r in (("icp", loop, reps), ("nn_stats", nn, step_reps), ("icp_step", step, step_reps)):
        w = windows(fn, r)
        out[name] = dict(ms_per_call=round(float(np.median(w)), 5), ms_windows=[round(x, 5) for x in w],
                         first_over_last=round(w[0] / w[-1], 3), calls_per_window=r)
    assert status.sum().item() == 0 and step_status.sum().item() == 0 and torch.isfinite(rmse).all()
    s, n = out["icp_step"]["ms_per_call"], out["nn_stats"]["ms_per_call"]
    return dict(instances=I, points=N, prior_points=N, n_iter=N_ITER, trim=0.7, **out, step_share=round(s / (s + n), 3),
                ms_per_iteration=round(out["icp"]["ms_per_call"] / (N_ITER + 1), 5),
                rmse_first_last_mm=[round(1e3 * float(rmse[0].mean()), 4), round(1e3 * float(rmse[-1].mean()), 4)])


def wrapper_side(reps):
    """the one-object K = 4 refine, fit_score and icp through their Python wrappers, and Tracker.step with and without recovery"""
    import torch

    from catre_amd import icp, synth, tracking
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    cfg = default_cfg(device="cuda:0")
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.cuda() for k, v in sd.items()}, strict=True)
    model.eval()
    n_iter = int(cfg.MODEL.CATRE.N_ITER_TEST)
    batch = {k: v.cuda() for k, v in synth.make_inputs(1, N, N, seed=2).items()}
    pcl, kps, pose, scale = batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"]
    res = dict(n_iter_refine=n_iter, points=N,
               refine_ms=per_call_ms(lambda: model.refine(batch, n_iter=n_iter), reps),
               fit_score_ms=per_call_ms(lambda: tracking.fit_score(pcl, kps, pose, scale), reps),
               icp_ms=per_call_ms(lambda: icp.icp(pcl, kps, pose, scale, n_iter=N_ITER), reps))
    scene = synth.make_depth_scene(H=240, W=320, n_inst=1, seed=3)
    depth = scene["depth"].cuda()

    def tracker(**kw):
        tr = tracking.Tracker(model, kps, scene["K"], mean_scales=batch["obj_mean_scales"], num_points=N, **kw)
        return tr.reset(scene["poses"].cuda(), scene["scales"].cuda())

    plain, rec = tracker(), tracker(recover="icp")
    res["tracker_step_ms"] = per_call_ms(lambda: plain.step(depth), reps)
    res["tracker_step_recover_ms"] = per_call_ms(lambda: rec.step(depth), reps)
    res["recover_share_of_step"] = round(1.0 - res["tracker_step_ms"] / res["tracker_step_recover_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--step-reps", type=int, default=1000)
    ap.add_argument("--wrapper-reps", type=int, default=200)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    import torch

    assert torch.cuda.is_available(), "icp_time.py measures on a HIP device"
    res = dict(what="catre_icp, catre_icp_step", device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
               icp=[icp_time(256, a.reps, a.step_reps), icp_time(1, a.reps, a.step_reps)],
               kernel_note="HIP events around back-to-back C-ABI calls on preallocated buffers after one second of the same calls; the "
                           "median of five windows.  catre_icp: 3 (n_iter + 1) launches; catre_nn_stats: two; catre_icp_step: one.  "
                           "step_share = icp_step / (icp_step + nn_stats)",
               wrappers=wrapper_side(a.wrapper_reps),
               wrapper_note="per-call HIP events, median, Python wrappers and allocations included; refine_ms is the one-object "
                            "K = n_iter_refine refine; tracker_step_* is Tracker.step on a 240x320 frame at 1024 points, "
                            "recover_share_of_step = 1 - tracker_step_ms / tracker_step_recover_ms")
    json.dump(res, open(os.path.join(a.out, "icp_time.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
