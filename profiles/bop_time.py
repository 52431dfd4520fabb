"""Time of the BOP pose errors (``catre_amd/pose_errors.py``, ``csrc/catre_bop.h``) on the GPU:

    python profiles/bop_time.py --out profiles     # profiles/bop_time.json

``catre_sym_err`` and ``catre_vsd`` through the C ABI on preallocated buffers.  HIP events around ``--reps`` back-to-back calls
after a warm-up of one second of the same calls (ten calls were not enough: the windows kept falling), five windows; the median
window is quoted, all five are stored, and ``first_over_last`` says what drift is left.

* ``sym_errors`` at I = 256 instances of n = 1024 points with S = 1 and with S = 314 symmetries per instance, and at I = 1:
  two launches per call.  ``point_sym_pairs`` = I * n * S is the work of the sweep; ``g_pairs_per_s`` divides it by the call
  time (the finish launch and the staging of the estimate's points are inside).
* ``vsd`` at 256 windows of 160x160 in 16 frames of 480x640, and at 16 full frames, T = 10 taus: a memset and two launches.
  ``bytes_per_call`` = the three fp32 depth reads per pixel (the least the comparison must move), ``gb_per_s`` over the call time.

Alongside, in the same process and for scale: the one-object K = 4 refine and ``evaluation.add_errors`` (ADD and ADD-S, n = 1024)
with per-call events (median, Python wrappers and allocations included), and ``sym_errors`` / ``vsd`` through their wrappers at I = 1."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, H, W = 1024, 480, 640
WARM_S = 1.0     # seconds of back-to-back calls before the first window: ten calls left the clocks still rising


def windows(fn, reps, n_windows=5):
    import time

    import torch

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_S:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
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


def poses(rng, I):
    pose = np.zeros((I, 3, 4))
    for i in range(I):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        z = rng.uniform(0.5, 1.2)
        pose[i, :, :3] = q
        pose[i, :, 3] = [rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.2, 0.2) * z, z]
    return pose.astype(np.float32)


def sym_time(I, S, reps):
    import torch

    from catre_amd import hip, pose_errors, synth

    lib = hip.load()
    rng = np.random.default_rng(I + S)
    pts = torch.as_tensor((rng.uniform(-0.5, 0.5, (I, N, 3)) * 0.2).astype(np.float32)).cuda()
    pose_gt = poses(rng, I)
    pose_est = pose_gt.copy()
    pose_est[:, :, 3] += rng.normal(0, 0.01, (I, 3)).astype(np.float32)
    pose_gt, pose_est = torch.as_tensor(pose_gt).cuda(), torch.as_tensor(pose_est).cuda()
    K = torch.tensor([[0.9 * W, 0, W / 2 - 0.5], [0, 0.9 * W, H / 2 - 0.5], [0, 0, 1]]).expand(I, 3, 3).contiguous().cuda()
    syms = pose_errors.SymSets.from_list([None if S == 1 else synth.y_axis_symmetries(S)] * I, "cuda")
    assert syms.s_max == S
    nbytes = lib.catre_sym_err_workspace_bytes(I, S)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    err = torch.empty(3, I, device="cuda")
    best = torch.empty(3, I, dtype=torch.int32, device="cuda")
    st, nul = hip.stream_ptr(pts.device), ctypes.c_void_p(0)

    def call():
        hip.check(lib.catre_sym_err(hip.ptr(pts), 0, N, hip.ptr(pose_est), hip.ptr(pose_gt), nul, nul, hip.ptr(K), hip.ptr(syms.syms),
                                    hip.ptr(syms.sym_off), hip.ptr(syms.sym_of), syms.n_sets, syms.s_tot, S, I, hip.ptr(ws), nbytes,
                                    hip.ptr(err), hip.ptr(best), nul, st), "catre_sym_err")

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    w = windows(call, reps)
    ms = float(np.median(w))
    assert torch.isfinite(err).all()
    pairs = I * N * S
    return dict(instances=I, points=N, symmetries=S, ms_per_call=round(ms, 5), ms_windows=[round(x, 5) for x in w],
                first_over_last=round(w[0] / w[-1], 3),
                calls_per_window=reps, point_sym_pairs=pairs, g_pairs_per_s=round(pairs / ms / 1e6, 3))


def vsd_time(I, h, w, F, reps, T=10):
    import torch

    from catre_amd import hip

    lib = hip.load()
    rng = np.random.default_rng(I + h)
    gt = rng.uniform(0.6, 1.4, (I, h, w)).astype(np.float32)
    est = (gt + rng.normal(0, 0.05, gt.shape)).astype(np.float32)
    gt[rng.random(gt.shape) < 0.4], est[rng.random(est.shape) < 0.4] = 0, 0
    test = (1.0 + 0.3 * rng.random((F, H, W))).astype(np.float32)
    test[rng.random(test.shape) < 0.03] = 0
    est, gt, test = (torch.as_tensor(a).cuda() for a in (est, gt, test))
    K = torch.tensor([[0.9 * W, 0, W / 2 - 0.5], [0, 0.9 * W, H / 2 - 0.5], [0, 0, 1]]).expand(I, 3, 3).contiguous().cuda()
    fo = torch.tensor([i % F for i in range(I)], dtype=torch.int32).cuda()
    org = torch.tensor([[int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))] for _ in range(I)], dtype=torch.int32).cuda()
    diam = torch.full((I,), 0.25, dtype=torch.float64, device="cuda")
    taus = (ctypes.c_double * T)(*[0.05 * (k + 1) for k in range(T)])
    counts = torch.empty(I, 2 + T, dtype=torch.int32, device="cuda")
    errors = torch.empty(I, T, dtype=torch.float64, device="cuda")
    st = hip.stream_ptr(est.device)

    def call():
        hip.check(lib.catre_vsd(hip.ptr(est), hip.ptr(gt), hip.ptr(test), hip.ptr(K), hip.ptr(fo), hip.ptr(org), hip.ptr(diam), taus,
                                0.015, 0, I, h, w, F, H, W, T, hip.ptr(counts), hip.ptr(errors), st), "catre_vsd")

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    ws = windows(call, reps)
    ms = float(np.median(ws))
    nbytes = 3 * 4 * I * h * w
    return dict(windows=I, window=f"{h}x{w}", frames=F, frame=f"{H}x{W}", taus=T, ms_per_call=round(ms, 5),
                ms_windows=[round(x, 5) for x in ws], first_over_last=round(ws[0] / ws[-1], 3), calls_per_window=reps,
                pixels_per_call=I * h * w, bytes_per_call=nbytes,
                gb_per_s=round(nbytes / ms / 1e6, 2), union_pixels=int(counts[:, 0].sum().item()),
                mean_error=round(float(errors.mean().item()), 4))


def per_call_ms(fn, reps):
    import torch

    for _ in range(10):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return round(float(np.median([a.elapsed_time(b) for a, b in ev])), 4)


def refine_side(reps):
    """the one-object K = 4 refine, add_errors, sym_errors and vsd (Python wrappers) in this process"""
    import torch

    from catre_amd import evaluation, pose_errors, synth
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    cfg = default_cfg(device="cuda:0")
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.cuda() for k, v in sd.items()}, strict=True)
    model.eval()
    rng = np.random.default_rng(3)
    kps = torch.as_tensor(rng.uniform(-0.5, 0.5, (1, N, 3)).astype(np.float32)).cuda()
    scale = torch.tensor([[0.2, 0.25, 0.2]]).cuda()
    pose = torch.as_tensor(poses(rng, 1)).cuda()
    pose_est = pose.clone()
    pose_est[:, :, 3] += 0.01
    inputs = synth.make_inputs(1, N, N, seed=2)
    pcl = ((kps * scale[:, None, :]) @ pose[:, :, :3].transpose(1, 2) + pose[:, None, :, 3]).contiguous()
    K = torch.tensor([[0.9 * W, 0, W / 2 - 0.5], [0, 0.9 * W, H / 2 - 0.5], [0, 0, 1]])
    n_iter = int(cfg.MODEL.CATRE.N_ITER_TEST)
    batch = {"pcl": pcl, "obj_kps": kps, "obj_pose_est": pose, "obj_scale_est": scale, "K": K.cuda()[None].contiguous(),
             "obj_mean_scales": inputs["obj_mean_scales"].cuda()}
    Kd = K.cuda()
    one, y314 = pose_errors.SymSets.from_list([None], "cuda"), pose_errors.SymSets.from_list([synth.y_axis_symmetries(314)], "cuda")
    win = torch.as_tensor(rng.uniform(0.6, 1.4, (1, 160, 160)).astype(np.float32)).cuda()
    frame = torch.as_tensor(rng.uniform(0.6, 1.4, (1, H, W)).astype(np.float32)).cuda()
    org = torch.tensor([[200, 100]], dtype=torch.int32).cuda()
    return dict(n_iter=n_iter, points=N,
                refine_ms=per_call_ms(lambda: model.refine(batch, n_iter=n_iter), reps),
                add_ms=per_call_ms(lambda: evaluation.add_errors(pose_est, pose, kps, scale, scale), reps),
                add_s_ms=per_call_ms(lambda: evaluation.add_errors(pose_est, pose, kps, scale, scale, symmetric=True), reps),
                sym_errors_s1_ms=per_call_ms(lambda: pose_errors.sym_errors(pose_est, pose, kps, Kd, one, scale_est=scale, scale_gt=scale), reps),
                sym_errors_s314_ms=per_call_ms(lambda: pose_errors.sym_errors(pose_est, pose, kps, Kd, y314, scale_est=scale, scale_gt=scale), reps),
                vsd_window_ms=per_call_ms(lambda: pose_errors.vsd(win, win, frame, Kd, origin=org, diameter=0.25), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--small-reps", type=int, default=1000)
    ap.add_argument("--step-reps", type=int, default=200)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    import torch

    assert torch.cuda.is_available(), "bop_time.py measures on a HIP device"
    res = dict(what="catre_sym_err, catre_vsd", device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
               sym_errors=[sym_time(256, 1, a.small_reps), sym_time(256, 314, a.reps), sym_time(1, 1, a.small_reps),
                           sym_time(1, 314, a.small_reps)],
               vsd=[vsd_time(256, 160, 160, 16, a.reps), vsd_time(16, H, W, 16, a.reps)],
               kernel_note="HIP events around back-to-back C-ABI calls on preallocated buffers after one second of the same calls; the "
                           "median of five windows, first_over_last = first window / last window.  catre_sym_err: two launches; catre_vsd: a memset and two launches.  g_pairs_per_s and "
                           "gb_per_s divide the counted work by the whole call time, the small launches included",
               refine=refine_side(a.step_reps),
               refine_note="per-call HIP events, median, Python wrappers and allocations included; refine_ms is the one-object "
                           "K = n_iter refine; add_ms / add_s_ms are evaluation.add_errors, the other three this module at I = 1")
    json.dump(res, open(os.path.join(a.out, "bop_time.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
