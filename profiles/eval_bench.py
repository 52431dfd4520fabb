"""Time the device evaluator (catre_amd/evaluation.py) on a REAL275-sized synthetic set: 2 754 images, 5 evaluated
iterations (pose_0 .. pose_4), seeded.

    python profiles/eval_bench.py [--images 2754] [--iters 5] [--repeat 5] [--out profiles/eval_device_times.json]

Timed, synchronised, after one warm-up call: ``NocsEvaluator.evaluate()`` (all iterations at once) split into host
flattening, device (uploads + the three kernels + the download of the match arrays) and host AP integration; the three
kernels alone between HIP events; ``compute_independent_mAP`` on one iteration's ``final_results``.  The only reference
time available is the one the fixture generator recorded on ITS machine's CPU for a 300-image set
(tests/golden/eval_nocs.npz, ``meta``): it is printed next to the device time, scaled per image and iteration, and comes
from a different machine - no ratio is claimed.  Per-kernel times: run this script under
``rocprofv3 --kernel-trace --stats -- python profiles/eval_bench.py --out ''``."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from catre_amd import evaluation as E  # noqa: E402

OBJ_NAMES = ["bottle", "bowl", "camera", "can", "laptop", "mug"]


def _rotations(rng, n, max_rad):
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    a = rng.uniform(0, max_rad, n)[:, None, None]
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = (-axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0],
                                                                          -axis[:, 1], axis[:, 0])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def make_set(n_img, n_iter, seed):
    """About 5 GTs per image (REAL275: 2 754 images, ~14 k objects), a detection for 9 in 10, pose error shrinking with the
    iteration.  -> gt_dict, per-object image index / class id, pose [T, N, 3, 4], scale [T, N, 3] (float32)."""
    rng = np.random.default_rng(seed)
    n_gt = rng.integers(3, 8, n_img)
    img = np.repeat(np.arange(n_img), n_gt)
    n = len(img)
    cls = rng.integers(1, len(OBJ_NAMES) + 1, n)
    R = _rotations(rng, n, np.pi)
    t = np.stack([rng.uniform(-.3, .3, n), rng.uniform(-.3, .3, n), rng.uniform(.5, 1.5, n)], 1)
    s = rng.uniform(.05, .3, (n, 3))
    gt_RT = np.zeros((n, 4, 4), np.float32)
    gt_RT[:, :3, :3], gt_RT[:, :3, 3], gt_RT[:, 3, 3] = R, t, 1
    hv = np.where(cls == len(OBJ_NAMES), rng.integers(0, 2, n), 1)
    off = np.concatenate([[0], np.cumsum(n_gt)])
    gt_dict = OrderedDict((f"scene/{i}", dict(gt_class_ids=cls[a:b], gt_RTs=gt_RT[a:b], gt_scales=s[a:b].astype(np.float32),
                                               gt_handle_visibility=hv[a:b])) for i, (a, b) in enumerate(zip(off[:-1], off[1:])))
    det = np.flatnonzero(rng.random(n) < 0.9)
    pose, scale = [], []
    for k in range(n_iter):
        err = 0.35 / (1 + k)
        Rp = R[det] @ _rotations(rng, len(det), err)
        tp = t[det] + rng.normal(0, 0.05 / (1 + k), (len(det), 3))
        pose.append(np.concatenate([Rp, tp[:, :, None]], 2).astype(np.float32))
        scale.append((s[det] * (1 + rng.normal(0, 0.2 / (1 + k), (len(det), 3)))).astype(np.float32))
    return gt_dict, img[det], cls[det], np.stack(pose), np.stack(scale)


def final_results(gt_dict, img, cls, pose, scale, it):
    last = np.array([[0, 0, 0, 1]], np.float32)
    res = []
    for i, gt in enumerate(gt_dict.values()):
        rows = np.flatnonzero(img == i)
        res.append(dict(gt, pred_class_ids=cls[rows], pred_scores=np.ones(len(rows)), pred_scales=scale[it, rows],
                        pred_RTs=np.stack([np.concatenate([m, last]) for m in pose[it, rows]]) if len(rows) else np.zeros((0, 4, 4), np.float32)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2754)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_device_times.json"))
    a = ap.parse_args()

    gt_dict, img, cls, pose, scale = make_set(a.images, a.iters, a.seed)
    ev = E.NocsEvaluator(OBJ_NAMES, n_iter_test=a.iters - 1)
    ev.set_gts(gt_dict)
    keys = list(gt_dict)
    for lo in range(0, len(img), a.batch):                       # objects arrive image by image, `batch` at a time
        rows = np.arange(lo, min(lo + a.batch, len(img)))
        ims = sorted(set(img[rows].tolist()))
        batch = dict(im_id=torch.from_numpy(np.searchsorted(ims, img[rows])).cuda(), obj_cls=torch.from_numpy(cls[rows] - 1).cuda())
        out = {f"pose_{k}": torch.from_numpy(pose[k, rows]).cuda() for k in range(a.iters)}
        out.update({f"scale_{k}": torch.from_numpy(scale[k, rows]).cuda() for k in range(a.iters)})
        ev.process([keys[i] for i in ims], batch, out)

    def timed(fn):
        fn()                                                      # warm-up
        ts = []
        for _ in range(a.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return r, float(np.median(ts)), float(np.min(ts))

    parts = []

    def run_eval():
        r = ev.evaluate()
        parts.append(dict(ev.timings))
        return r

    res, ev_med, ev_min = timed(run_eval)
    split = {k: float(np.median([p[k] for p in parts[1:]])) for k in parts[0]}

    # the three kernels alone, between events
    gts = list(gt_dict.values())
    synset = ["BG"] + OBJ_NAMES
    deg, cm, iou, sel = E.threshold_lists(E.DEGREE_THRESHOLDS, E.SHIFT_THRESHOLDS, E.IOU_3D_THRESHOLDS, 0.1, True)
    groups = E.flatten_groups(img, cls, np.ones(len(img)), np.repeat(np.arange(len(gts)), [len(g["gt_class_ids"]) for g in gts]),
                              np.concatenate([g["gt_class_ids"] for g in gts]), len(gts), len(synset))
    gt_pose = np.ascontiguousarray(np.concatenate([g["gt_RTs"] for g in gts])[:, :3, :])
    gt_scale, gt_hv = np.concatenate([g["gt_scales"] for g in gts]), np.concatenate([g["gt_handle_visibility"] for g in gts])
    dpose, dscale = torch.from_numpy(pose).cuda(), torch.from_numpy(scale).cuda()
    E.run_kernels(groups, dpose, dscale, gt_pose, gt_scale, gt_hv, synset, deg, cm, iou, sel, dpose.device)
    kern = []
    for _ in range(a.repeat):
        # run_kernels uploads its index arrays first; the events bracket uploads + kernels, the uploads being a few 100 KB
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        E.run_kernels(groups, dpose, dscale, gt_pose, gt_scale, gt_hv, synset, deg, cm, iou, sel, dpose.device)
        e1.record()
        torch.cuda.synchronize()
        kern.append(e0.elapsed_time(e1) / 1e3)

    fr = final_results(gt_dict, img, cls, pose, scale, a.iters - 1)
    one, one_med, one_min = timed(lambda: E.compute_independent_mAP(fr, synset, E.DEGREE_THRESHOLDS, E.SHIFT_THRESHOLDS, E.IOU_3D_THRESHOLDS))
    last = res[f"iter{a.iters - 1}"]
    assert np.array_equal(one[0], last["iou_3d_aps"]) and np.array_equal(one[1], last["pose_aps"])

    meta = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "eval_nocs.npz"))["meta"]))["sets"]["as_called"]
    ref_per = meta["reference_wall_s"] / meta["images"]
    result = dict(
        images=a.images, iterations=a.iters, predictions_per_iteration=int(len(img)), gts=int(len(groups.gt_idx)),
        groups=int(groups.G), pairs=int(len(groups.pair_group)), device=torch.cuda.get_device_name(0),
        evaluate_all_iterations_s=dict(median=ev_med, min=ev_min, **{f"{k}_median": v for k, v in split.items()}),
        uploads_plus_three_kernels_event_s=dict(median=float(np.median(kern)), min=float(np.min(kern))),
        compute_independent_mAP_one_iteration_s=dict(median=one_med, min=one_min),
        reference_other_machine=dict(
            wall_s=meta["reference_wall_s"], images=meta["images"], predictions=meta["predictions"],
            s_per_image_and_iteration=ref_per, projected_s_for_this_set=ref_per * a.images * a.iters,
            note="the reference's compute_independent_mAP on the CPU of the machine that wrote tests/golden/eval_nocs.npz, "
                 "a 300-image set, scaled by images x iterations; a DIFFERENT machine from the device times above"),
        mean_ap=dict(IoU50=float(last["iou_3d_aps"][-1, 2]), re10te5=float(last["pose_aps"][-1, 1, 1])))
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
