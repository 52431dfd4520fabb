"""Time of the splat render (``catre_amd/render.py``, ``csrc/catre_render.h``) on the GPU:

    python profiles/splat_time.py --out profiles     # profiles/splat_time.json

``catre_splat_render`` through the C ABI on preallocated buffers - all outputs, ``vis`` included, so a call is the table
copy and four launches (clear, splat, resolve, visible) - at I = 256 box priors of M = 1024 points spread over F = 16 frames
of 480x640 (16 per frame, 0.5 - 1.2 m, rho_rel 0.06, r_max 24), with and without an observed depth, and at I = 1, F = 1.
HIP events around ``--reps`` back-to-back calls after a warm-up, five windows, the median window is quoted.

What the splat does per call is counted next to the time: ``disc_pixels`` = the (point, pixel) pairs that pass the distance
test (counted with torch from the same fp32 centres and radii, row by row) and ``rendered_pixels`` = the pixels that end up
covered.  The kernel issues an atomic only where a plain load does not already show a smaller key, so the number of
atomics per call lies between the two and is NOT counted; ``disc_pixels / time`` is the rate of resolved pixel updates,
``rendered_pixels / time`` a lower bound of the atomic rate.  Both rates hold the other three launches as well.

Alongside, in the same process: the one-object K = 4 refine and ``fit_score`` (N = M = 1024, per-call events, median), and
``splat_prior`` through the Python wrapper at I = 1 (allocations included) - what ``Tracker(crop="render")`` adds to a step."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M, H, W = 1024, 480, 640
RHO_REL, R_MAX, DELTA = 0.06, 24.0, 0.015


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


def scene(I, F, seed):
    """I box priors of M surface points, I / F per frame, turned at random, 0.5 - 1.2 m in front of a 576-pixel camera"""
    rng = np.random.default_rng(seed)
    kps = rng.uniform(-0.5, 0.5, (I, M, 3))
    face = rng.integers(0, 3, (I, M))
    np.put_along_axis(kps, face[..., None], np.where(rng.random((I, M, 1)) < 0.5, -0.5, 0.5), axis=2)
    scale = rng.uniform(0.1, 0.25, (I, 3))
    pose = np.zeros((I, 3, 4))
    for i in range(I):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        z = rng.uniform(0.5, 1.2)
        pose[i, :, :3] = q
        pose[i, :, 3] = [rng.uniform(-0.45, 0.45) * z, rng.uniform(-0.32, 0.32) * z, z]
    K = np.array([[0.9 * W, 0, W / 2 - 0.5], [0, 0.9 * W, H / 2 - 0.5], [0, 0, 1]], np.float32)
    frame_of = [i % F for i in range(I)]
    depth = (1.0 + 0.3 * rng.random((F, H, W))).astype(np.float32)
    depth[rng.random((F, H, W)) < 0.03] = 0
    return kps.astype(np.float32), pose.astype(np.float32), scale.astype(np.float32), K, frame_of, depth


def disc_pixels(kps, pose, scale, rho, K):
    """(point, pixel) pairs inside a disc and the image, from fp32 centres and radii (torch, on the device)"""
    import torch

    p = torch.einsum("irc,imc->imr", pose[:, :, :3], kps * scale[:, None, :]) + pose[:, None, :, 3]
    z = p[..., 2]
    u0, v0 = K[0, 0] * p[..., 0] / z + K[0, 2], K[1, 1] * p[..., 1] / z + K[1, 2]
    r = torch.clamp(K[0, 0] * rho[:, None] / z, max=R_MAX)
    total = 0
    for dv in range(-int(R_MAX) - 1, int(R_MAX) + 2):
        v = torch.floor(v0) + dv
        h2 = r * r - (v - v0) ** 2
        half = torch.sqrt(torch.clamp(h2, min=0))
        lo, hi = torch.clamp(torch.ceil(u0 - half), min=0), torch.clamp(torch.floor(u0 + half), max=W - 1)
        n = torch.where((h2 >= 0) & (v >= 0) & (v <= H - 1) & (z > 0), torch.clamp(hi - lo + 1, min=0), torch.zeros_like(hi))
        total += int(n.sum().item())
    return total


def splat_time(I, F, with_depth, reps):
    import torch

    from catre_amd import hip

    lib = hip.load()
    kps, pose, scale, K, frame_of, depth = scene(I, F, seed=I)
    kps, pose, scale, depth = (torch.as_tensor(a).cuda() for a in (kps, pose, scale, depth))
    rho = (RHO_REL * torch.linalg.vector_norm(scale, dim=1)).contiguous()
    nbytes = lib.catre_splat_workspace_bytes(F, H, W)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")
    labels, point, fit, counts = i32(F, H, W), i32(F, H, W), i32(F, H, W), i32(I, 5)
    zbuf = torch.empty(F, H, W, device="cuda")
    cls = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    vis = torch.empty(I, M, dtype=torch.uint8, device="cuda")
    k9 = (ctypes.c_float * (9 * F))(*[float(v) for v in np.tile(K.reshape(-1), F)])
    fo = (ctypes.c_int32 * I)(*frame_of)
    st = hip.stream_ptr(kps.device)
    dptr = hip.ptr(depth) if with_depth else ctypes.c_void_p(0)

    def call():
        hip.check(lib.catre_splat_render(hip.ptr(kps), hip.ptr(pose), hip.ptr(scale), hip.ptr(rho), dptr, k9, fo, R_MAX, DELTA, F, I, M,
                                         H, W, hip.ptr(ws), nbytes, hip.ptr(labels), hip.ptr(zbuf), hip.ptr(point), hip.ptr(cls),
                                         hip.ptr(fit), hip.ptr(counts), hip.ptr(vis), st), "catre_splat_render")

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    w = windows(call, reps)
    ms = float(np.median(w))
    discs = disc_pixels(kps, pose, scale, rho, torch.as_tensor(K).cuda())
    rendered = int((labels > 0).sum().item())
    cnt = counts.sum(0).tolist()
    assert cnt[0] == rendered == sum(cnt[1:])
    return dict(instances=I, points=M, frames=F, frame=f"{H}x{W}", observed_depth=bool(with_depth), ms_per_call=round(ms, 5),
                ms_windows=[round(x, 5) for x in w], calls_per_window=reps, disc_pixels_per_call=discs, rendered_pixels_per_call=rendered,
                class_pixels=dict(agree=cnt[1], occluded=cnt[2], free=cnt[3], hole=cnt[4]), visible_points=int(vis.sum().item()),
                g_disc_pixels_per_s=round(discs / ms / 1e6, 3), g_rendered_pixels_per_s=round(rendered / ms / 1e6, 4))


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


def tracker_side(reps):
    """the one-object K = 4 refine, fit_score and splat_prior (Python wrappers) in this process"""
    import torch

    from catre_amd import render, synth, tracking
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    cfg = default_cfg(device="cuda:0")
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.cuda() for k, v in sd.items()}, strict=True)
    model.eval()
    kps, pose, scale, K, _, depth = scene(1, 1, seed=1)
    kps, pose, scale, depth = (torch.as_tensor(a).cuda() for a in (kps, pose, scale, depth))
    inputs = synth.make_inputs(1, M, M, seed=2)
    pcl = (kps * scale[:, None, :]) @ pose[:, :, :3].transpose(1, 2) + pose[:, None, :, 3]
    n_iter = int(cfg.MODEL.CATRE.N_ITER_TEST)
    batch = {"pcl": pcl.contiguous(), "obj_kps": kps, "obj_pose_est": pose, "obj_scale_est": scale,
             "K": torch.as_tensor(K).cuda()[None].contiguous(), "obj_mean_scales": inputs["obj_mean_scales"].cuda()}
    return dict(n_iter=n_iter, points=M,
                refine_ms=per_call_ms(lambda: model.refine(batch, n_iter=n_iter), reps),
                fit_score_ms=per_call_ms(lambda: tracking.fit_score(batch["pcl"], kps, pose, scale, 0.1), reps),
                splat_prior_ms=per_call_ms(lambda: render.splat_prior(kps, pose, scale, K, (H, W), depth=depth, delta=0.05), reps),
                splat_prior_visible_ms=per_call_ms(lambda: render.splat_prior(kps, pose, scale, K, (H, W), depth=depth,
                                                                              return_visible=True), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--small-reps", type=int, default=1000)
    ap.add_argument("--step-reps", type=int, default=200)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    import torch

    assert torch.cuda.is_available(), "splat_time.py measures on a HIP device"
    res = dict(what="catre_splat_render", device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
               rho_rel=RHO_REL, r_max=R_MAX, delta=DELTA,
               kernel=[splat_time(256, 16, True, a.reps), splat_time(256, 16, False, a.reps), splat_time(1, 1, True, a.small_reps),
                       splat_time(1, 1, False, a.small_reps)],
               kernel_note="HIP events around back-to-back C-ABI calls on preallocated buffers after 10 warm-up calls, all outputs "
                           "written (vis included): one table copy and four launches per call; the median of five windows.  The "
                           "atomics issued per call lie between rendered_pixels and disc_pixels (an atomic is skipped where a plain "
                           "load already shows a smaller key) and are not counted: g_rendered_pixels_per_s is a lower bound of the "
                           "64-bit atomicMin rate the call sustained, g_disc_pixels_per_s the rate of resolved pixel updates",
               tracker=tracker_side(a.step_reps),
               tracker_note="per-call HIP events, median, Python wrappers and allocations included; refine_ms is the one-object "
                            "K = n_iter refine, splat_prior_ms what Tracker(crop='render') adds to a step at I = 1")
    json.dump(res, open(os.path.join(a.out, "splat_time.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
