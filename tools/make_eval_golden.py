"""Fixture for the device evaluator (``catre_amd/evaluation.py``), written by the UNMODIFIED reference (needs the
reference tree, see ``oracle/ref_shim.py``; never needed to build, test or run the product):

    python tools/make_eval_golden.py            # tests/golden/eval_nocs.npz

``core/catre/engine/test_utils.py`` is loaded as it is (it needs numpy and tqdm only).  Its ``compute_3d_matches``,
``compute_RT_overlaps`` and ``compute_match_from_degree_cm`` are wrapped with recorders and its own
``compute_independent_mAP`` (:760-924) is run - the per-class loop is not restated here.  Two seeded sets of synthetic
images, float32 inputs:

* ``exact``: the reference is called on the inputs widened to float64, so its own arithmetic is double throughout.
  Stored: IoU overlaps, (degree, cm), every match array, both AP arrays.  ``synset_names`` holds ``phone``; distinct scores.
* ``as_called``: the reference is called as its evaluator calls it (catre_custom_evaluator.py:237-260): float32
  ``pred_RTs`` / ``pred_scales`` - mixed fp32 / fp64 arithmetic - and all scores 1.0.  Stored: match and AP arrays.

Every call of the three functions that sees an object is stored, in call order (image, then class id), with arrays of one
kind concatenated along their last axis; ``*/call_*`` give image, class and sizes of each call.

Cases a set must hold (asserted): missing and wrong-class detections, images with predictions but no GT and the reverse,
empty images, a group of >= 8 objects, mugs with both handle flags.  Discrete choices must not depend on rounding, so a
seed is skipped (the next one taken) unless: nothing is NaN; every arccos argument is <= 1 - 1e-12 in magnitude (checked
on the angle: >= acos(1 - 1e-12)); no two positive IoUs and no two degree + cm sums of one prediction are equal; every
IoU, degree and cm is >= 1e-4 (in its own unit) away from every threshold in use.
"""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_nocs.npz")
DEGREE_THRESHOLDS, SHIFT_THRESHOLDS, IOU_3D_THRESHOLDS = [5, 10], [2, 5, 10], [0.1, 0.25, 0.50, 0.75]
SETS = (  # name, first seed, images, synset_names, distinct scores, float32 call
    ("exact", 11, 300, ["BG", "bottle", "bowl", "phone", "can", "laptop", "mug"], True, False),
    ("as_called", 23, 300, ["BG", "bottle", "bowl", "camera", "can", "laptop", "mug"], False, True),
)
MARGIN = 1e-4
MIN_ANGLE_DEG = float(np.degrees(np.arccos(1 - 1e-12)))


def load_reference():
    path = os.path.join(ref_shim.REFERENCE_ROOT, "core", "catre", "engine", "test_utils.py")
    if not os.path.exists(path):
        raise RuntimeError(f"reference tree not found at {ref_shim.REFERENCE_ROOT}")
    spec = importlib.util.spec_from_file_location("ref_test_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rot(rng, max_deg=180.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.radians(rng.uniform(0, max_deg))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _roty(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def make_images(seed, n_img, synset_names, distinct_scores):
    """-> list of dicts of float32 / int arrays (gt_cls, gt_RT [n,3,4], gt_scale, gt_hv, pred_cls, pred_RT, pred_scale,
    pred_scores)."""
    rng = np.random.default_rng(seed)
    n_cls = len(synset_names) - 1
    mug = synset_names.index("mug")
    images = []
    for im in range(n_img):
        kind = "big" if im == 7 else rng.choice(["plain", "empty", "no_gt", "no_pred"], p=[0.88, 0.04, 0.04, 0.04])
        n_gt = 8 if kind == "big" else 0 if kind in ("empty", "no_gt") else int(rng.choice(7, p=[.05, .2, .3, .2, .12, .08, .05]))
        gt_cls = np.full(n_gt, 1 + im % n_cls) if kind == "big" else rng.integers(1, n_cls + 1, n_gt)
        gt_RT, gt_scale, gt_hv, pred = [], [], [], []
        for k in range(n_gt):
            R, t = _rot(rng), np.array([rng.uniform(-.3, .3), rng.uniform(-.3, .3), rng.uniform(.5, 1.5)])
            s = rng.uniform(.05, .3, 3)
            gt_RT.append(np.concatenate([R, t[:, None]], 1))
            gt_scale.append(s)
            gt_hv.append(int(rng.integers(0, 2)) if gt_cls[k] == mug else 1)
            if kind == "no_pred" or rng.random() < 0.12:      # missing detection
                continue
            cls = int(gt_cls[k]) if rng.random() < 0.92 else int(1 + (gt_cls[k] + rng.integers(0, n_cls - 1)) % n_cls)
            err = rng.choice([3.0, 12.0, 60.0], p=[.5, .35, .15])
            Rp = (R @ _roty(rng.uniform(0, 2 * np.pi)) if rng.random() < 0.5 else R) @ _rot(rng, err)
            Rp = Rp * (1 + rng.normal(0, 0.01))               # a network's rotation block is not exactly orthonormal
            tp = t + rng.normal(0, rng.choice([0.01, 0.04, 0.15], p=[.5, .35, .15]), 3)
            pred.append((cls, np.concatenate([Rp, tp[:, None]], 1), s * (1 + rng.normal(0, 0.12, 3))))
        n_fp = int(rng.integers(1, 4)) if kind == "no_gt" else int(rng.random() < 0.15) if kind == "plain" else 0
        for _ in range(n_fp):                                  # detections of nothing
            t = np.array([rng.uniform(-.3, .3), rng.uniform(-.3, .3), rng.uniform(.5, 1.5)])
            pred.append((int(rng.integers(1, n_cls + 1)), np.concatenate([_rot(rng), t[:, None]], 1), rng.uniform(.05, .3, 3)))
        pred = [pred[i] for i in rng.permutation(len(pred))]
        n_pred = len(pred)
        images.append(dict(
            gt_cls=np.asarray(gt_cls, np.int32).reshape(-1), gt_RT=np.asarray(gt_RT, np.float32).reshape(-1, 3, 4),
            gt_scale=np.asarray(gt_scale, np.float32).reshape(-1, 3), gt_hv=np.asarray(gt_hv, np.int32).reshape(-1),
            pred_cls=np.asarray([p[0] for p in pred], np.int32).reshape(-1),
            pred_RT=np.asarray([p[1] for p in pred], np.float32).reshape(-1, 3, 4),
            pred_scale=np.asarray([p[2] for p in pred], np.float32).reshape(-1, 3),
            pred_scores=np.ones(n_pred)))
    if distinct_scores:                                        # distinct over the whole set, not only inside an image
        total = sum(len(im["pred_cls"]) for im in images)
        vals, at = (rng.permutation(4 * total)[:total] + 1) / (4 * total + 1.0), 0
        for im in images:
            im["pred_scores"] = vals[at:at + len(im["pred_cls"])]
            at += len(im["pred_cls"])
    return images


def final_results(images, float32_call):
    """The list the reference's evaluator hands to compute_independent_mAP (catre_custom_evaluator.py:239-245)."""
    last = np.array([[0, 0, 0, 1]], np.float32)

    def rt44(a, dtype):
        return np.stack([np.concatenate([m, last], 0) for m in a]).astype(dtype) if len(a) else np.zeros((0, 4, 4), dtype)

    ptype = np.float32 if float32_call else np.float64
    return [dict(gt_class_ids=im["gt_cls"], gt_RTs=rt44(im["gt_RT"], np.float64), gt_scales=im["gt_scale"].astype(np.float64),
                 gt_handle_visibility=im["gt_hv"], pred_class_ids=im["pred_cls"], pred_scores=im["pred_scores"],
                 pred_bboxes=np.tile(np.array([[1, 1, 9, 9]], np.int32), (len(im["pred_cls"]), 1)),
                 pred_RTs=rt44(im["pred_RT"], ptype), pred_scales=im["pred_scale"].astype(ptype)) for im in images]


def run_recorded(mod, results, synset_names):
    """The reference's compute_independent_mAP with recorders around its three helpers -> (aps, records)."""
    rec = {"m3d": [], "rt": [], "pose": []}
    orig = (mod.compute_3d_matches, mod.compute_RT_overlaps, mod.compute_match_from_degree_cm)

    def m3d(*a, **k):
        out = orig[0](*a, **k)
        rec["m3d"].append(out)
        return out

    def rt(*a, **k):
        out = orig[1](*a, **k)
        rec["rt"].append(out)
        return out

    def pose(*a, **k):
        out = orig[2](*a, **k)
        rec["pose"].append(out)
        return out

    mod.compute_3d_matches, mod.compute_RT_overlaps, mod.compute_match_from_degree_cm = m3d, rt, pose
    try:
        aps = mod.compute_independent_mAP(results, synset_names, degree_thresholds=DEGREE_THRESHOLDS,
                                          shift_thresholds=SHIFT_THRESHOLDS, iou_3d_thresholds=IOU_3D_THRESHOLDS)
    finally:
        mod.compute_3d_matches, mod.compute_RT_overlaps, mod.compute_match_from_degree_cm = orig
    return aps, rec


def pack(images, results, synset_names, aps, rec, with_overlaps):
    """Flat arrays of one set + the smallest distances to a discrete decision."""
    calls = [(i, c) for i, r in enumerate(results) if len(r["gt_class_ids"]) or len(r["pred_class_ids"])
             for c in range(1, len(synset_names))]
    assert len(calls) == len(rec["m3d"]) == len(rec["rt"]) == len(rec["pose"])
    keep = [k for k, (gm, pm, _, _) in enumerate(rec["m3d"]) if gm.shape[1] or pm.shape[1]]
    cat = lambda xs, dtype, axis=-1: np.concatenate([np.asarray(x) for x in xs], axis=axis).astype(dtype)  # noqa: E731
    out = dict(
        n_gt=np.array([len(im["gt_cls"]) for im in images], np.uint8), n_pred=np.array([len(im["pred_cls"]) for im in images], np.uint8),
        **{k: np.concatenate([im[k] for im in images]) for k in ("gt_RT", "gt_scale", "pred_RT", "pred_scale", "pred_scores")},
        **{k: np.concatenate([im[k] for im in images]).astype(np.int8) for k in ("gt_cls", "gt_hv", "pred_cls")},
        call_img=np.array([calls[k][0] for k in keep], np.int16), call_cls=np.array([calls[k][1] for k in keep], np.int8),
        call_np=np.array([rec["m3d"][k][1].shape[1] for k in keep], np.uint8),
        call_ng=np.array([rec["m3d"][k][0].shape[1] for k in keep], np.uint8),
        call_mp=np.array([rec["pose"][k][1].shape[2] for k in keep], np.uint8),
        call_mg=np.array([rec["pose"][k][0].shape[2] for k in keep], np.uint8),
        iou_gt_match=cat([rec["m3d"][k][0] for k in keep], np.int8), iou_pred_match=cat([rec["m3d"][k][1] for k in keep], np.int8),
        order=cat([rec["m3d"][k][3] for k in keep], np.int8),
        pose_gt_match=cat([rec["pose"][k][0] for k in keep], np.int8), pose_pred_match=cat([rec["pose"][k][1] for k in keep], np.int8),
        iou_3d_aps=aps[0], pose_aps=aps[1])
    iou = cat([rec["m3d"][k][2].ravel() for k in keep], np.float32)
    degcm = cat([rec["rt"][k].reshape(-1, 2) for k in keep], np.float64, axis=0)
    if with_overlaps:
        out.update(iou=iou, degcm=degcm)
    for k in ("iou_gt_match", "iou_pred_match", "order", "pose_gt_match", "pose_pred_match"):
        assert out[k].max(initial=-1) < 127

    deg_list, cm_list = DEGREE_THRESHOLDS + [360], SHIFT_THRESHOLDS + [100]
    dist = dict(
        nan=bool(np.isnan(iou).any() or np.isnan(degcm).any() or np.isnan(aps[0]).any() or np.isnan(aps[1]).any()),
        iou=float(min(np.abs(iou.astype(np.float64) - t).min() for t in IOU_3D_THRESHOLDS)),
        deg=float(min(np.abs(degcm[:, 0] - t).min() for t in deg_list)), cm=float(min(np.abs(degcm[:, 1] - t).min() for t in cm_list)),
        angle=float(min(degcm[:, 0].min(), (180 - degcm[:, 0]).min())), iou_tie=np.inf, sum_tie=np.inf)
    for k in keep:
        for row in rec["m3d"][k][2].astype(np.float64):
            pos = np.sort(row[row > 0])
            if len(pos) > 1:
                dist["iou_tie"] = float(min(dist["iou_tie"], np.diff(pos).min()))
        for row in rec["rt"][k].sum(-1):
            if len(row) > 1:
                dist["sum_tie"] = float(min(dist["sum_tie"], np.diff(np.sort(row)).min()))
    return out, dist


def has_cases(images, synset_names):
    mug = synset_names.index("mug")
    hv = np.concatenate([im["gt_hv"][im["gt_cls"] == mug] for im in images])
    flags = dict(
        empty=any(len(im["gt_cls"]) == 0 and len(im["pred_cls"]) == 0 for im in images),
        pred_no_gt=any(len(im["gt_cls"]) == 0 and len(im["pred_cls"]) > 0 for im in images),
        gt_no_pred=any(len(im["gt_cls"]) > 0 and len(im["pred_cls"]) == 0 for im in images),
        missing=any(0 < len(im["pred_cls"]) < len(im["gt_cls"]) for im in images),
        wrong_class=any(len(set(im["pred_cls"]) - set(im["gt_cls"])) and len(im["gt_cls"]) for im in images),
        big_group=any(np.bincount(im["gt_cls"]).max(initial=0) >= 8 and np.bincount(im["pred_cls"]).max(initial=0) >= 6 for im in images),
        mug_flags=set(hv.tolist()) == {0, 1})
    return flags


def main():
    mod = load_reference()
    arrays, meta = {}, dict(degree_thresholds=DEGREE_THRESHOLDS, shift_thresholds=SHIFT_THRESHOLDS,
                            iou_3d_thresholds=IOU_3D_THRESHOLDS, margin=MARGIN, sets={})
    for name, seed, n_img, synset_names, distinct, f32 in SETS:
        while True:
            images = make_images(seed, n_img, synset_names, distinct)
            flags = has_cases(images, synset_names)
            results = final_results(images, f32)
            t0 = time.perf_counter()
            mod.compute_independent_mAP(results, synset_names, degree_thresholds=DEGREE_THRESHOLDS,
                                        shift_thresholds=SHIFT_THRESHOLDS, iou_3d_thresholds=IOU_3D_THRESHOLDS)
            wall = time.perf_counter() - t0
            aps, rec = run_recorded(mod, results, synset_names)
            out, dist = pack(images, results, synset_names, aps, rec, with_overlaps=not f32)
            ok = (all(flags.values()) and not dist["nan"] and dist["angle"] >= MIN_ANGLE_DEG and dist["iou_tie"] > 0 and
                  dist["sum_tie"] > 0 and min(dist["iou"], dist["deg"], dist["cm"]) >= MARGIN)
            print(name, "seed", seed, "ok" if ok else "SKIPPED", flags, dist, f"reference {wall:.2f} s")
            if ok:
                break
            seed += 1
        arrays.update({f"{name}/{k}": v for k, v in out.items()})
        meta["sets"][name] = dict(seed=seed, images=n_img, synset_names=synset_names, predictions=int(out["n_pred"].sum()),
                                  gts=int(out["n_gt"].sum()), float32_call=f32, reference_wall_s=round(wall, 3),
                                  min_distance={k: v for k, v in dist.items() if k != "nan"})
    meta["reference_wall_note"] = ("seconds of the reference's compute_independent_mAP for the set on the CPU that wrote "
                                   "this file (one run, no recorders)")
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(GOLDEN, **arrays)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
