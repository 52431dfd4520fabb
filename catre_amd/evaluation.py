"""NOCS-style evaluation of refined poses on the device: 3D IoU, degree / cm matching, mAP.

What the reference does in nested Python / numpy loops on the host (``compute_independent_mAP``,
core/catre/engine/test_utils.py:760-924, driven by core/catre/engine/catre_custom_evaluator.py:121-311) runs here as
three HIP launches whatever the number of images (``csrc/catre_eval.h``):

* ``compute_independent_mAP`` takes the reference's arguments and ``final_results`` list and returns its two AP arrays;
* ``overlaps_and_matches`` returns the intermediate arrays per (image, class) group, for tests and debugging;
* ``NocsEvaluator`` collects a model's ``out_dict`` without leaving the device and evaluates all K + 1 iterations at once.

On the host stay (a) every ordering by score - with tied scores (CATRE's default is all 1.0) the order is whatever
numpy's sort makes of it, so it is made with the reference's own call, ``np.argsort(scores)[::-1]``, and the device
receives permutations - and (b) the AP integration of a few thousand matches per class
(``ap_from_matches_scores``, test_utils.py:112-137).  There is no CPU fallback for the rest.

Deviation from the reference: the arccos argument is clamped to [-1, 1] in every degree branch (the reference clamps
the generic branch only and returns NaN elsewhere when rounding pushes the argument past 1).  Tie rules among GTs are
numpy's for the group sizes that occur: equal IoUs - the later GT wins; equal degree + cm sums - the earlier one.
"""
import math
import time
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch

from . import hip

MODE_GENERIC, MODE_YSYM, MODE_MUG, MODE_FLIP = 0, 1, 2, 3     # CATRE_EVAL_* of include/catre_hip.h
N_ROT = 20                                                     # CATRE_EVAL_NROT
_YSYM_NAMES = ("bottle", "bowl", "can")                        # test_utils.py:178, :665
_FLIP_NAMES = ("phone", "eggbox", "glue")                      # test_utils.py:676

# the evaluator's thresholds and table rows (catre_custom_evaluator.py:247-311)
DEGREE_THRESHOLDS = [5, 10]
SHIFT_THRESHOLDS = [2, 5, 10]
DEGREE_SHIFT_THRESHOLDS = [(5, 2), (5, 5), (10, 2), (10, 5), (10, 10)]
IOU_3D_THRESHOLDS = [0.1, 0.25, 0.50, 0.75]

ABI_CALLS = {"catre_eval_overlaps": 0, "catre_eval_match_iou": 0, "catre_eval_match_pose": 0}


def abi_call_count():
    """C-ABI calls made by this module so far (constant per evaluation, whatever the number of images)."""
    return sum(ABI_CALLS.values())


def _call(name, *args):
    ABI_CALLS[name] += 1
    hip.check(getattr(hip.load(), name)(*args), name)


def class_modes(synset_names):
    """CATRE_EVAL_* per class id of ``synset_names`` (test_utils.py:178-180, 665-683)."""
    return np.array([MODE_YSYM if n in _YSYM_NAMES else MODE_MUG if n == "mug" else MODE_FLIP if n in _FLIP_NAMES
                     else MODE_GENERIC for n in synset_names], dtype=np.int32)


def rotation_table():
    """[20, 2] (cos, sin) of 2 pi i / 20 with the reference's own calls (test_utils.py:187-200): its bits."""
    n = N_ROT
    return np.array([[np.cos(2 * math.pi * i / float(n)), np.sin(2 * math.pi * i / float(n))] for i in range(n)],
                    dtype=np.float64)


def ap_from_matches_scores(pred_match, pred_scores, gt_match, order=None):
    """``compute_ap_from_matches_scores`` (test_utils.py:112-137) with the same float operations, vectorised: the
    Python loop over the precisions is a reversed running maximum.  ``gt_match``: the array, or its length.
    ``order``: ``np.argsort(pred_scores)[::-1]`` if the caller already has it (it is the same for every threshold)."""
    pred_match = np.asarray(pred_match)
    pred_scores = np.asarray(pred_scores)
    assert pred_match.shape[0] == pred_scores.shape[0]
    n_gt = int(gt_match) if np.isscalar(gt_match) else len(gt_match)
    if order is None:
        order = np.argsort(pred_scores)[::-1]
    hits = np.cumsum(pred_match[order] > -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        precisions = hits / (np.arange(len(pred_match)) + 1)
        recalls = hits.astype(np.float32) / n_gt          # float32, as :122 has it
    precisions = np.concatenate([[0], precisions, [0]])
    recalls = np.concatenate([[0], recalls, [1]])
    precisions = np.maximum.accumulate(precisions[::-1])[::-1]
    indices = np.where(recalls[:-1] != recalls[1:])[0] + 1
    return np.sum((recalls[indices] - recalls[indices - 1]) * precisions[indices])


@dataclass
class Groups:
    """CSR view of an evaluation set.  Group = one (image, class) pair holding a prediction or a GT; groups are ordered
    by class, then by image, so a class's predictions / GTs are one contiguous range in the reference's concatenation
    order (image order first, the score order inside each image)."""
    n_img: int
    num_classes: int
    group_cls: np.ndarray     # [G]
    group_img: np.ndarray     # [G]
    pred_off: np.ndarray      # [G + 1] int32
    gt_off: np.ndarray        # [G + 1] int32
    pair_off: np.ndarray      # [G + 1] int32
    pair_group: np.ndarray    # [Q] int32
    pred_idx: np.ndarray      # [P] int32: row of the caller's prediction arrays, in matching order
    pred_local: np.ndarray    # [P]: the same as an index into the group's predictions in their image order (`indices`, :557)
    pred_scores: np.ndarray   # [P] scores in matching order
    gt_idx: np.ndarray        # [NG] int32: row of the caller's GT arrays
    cls_pred: np.ndarray      # [num_classes + 1]: prediction range of each class
    cls_gt: np.ndarray        # [num_classes + 1]

    @property
    def G(self):
        return len(self.group_cls)


def flatten_groups(pred_img, pred_cls, pred_scores, gt_img, gt_cls, n_img, num_classes):
    """Group flat per-object arrays (image index, class id [, score]) into ``Groups``.  Objects of a class outside
    1 .. num_classes - 1 are dropped, as the reference's class loop never sees them (:810)."""
    pred_img, pred_cls = np.asarray(pred_img, np.int64), np.asarray(pred_cls, np.int64)
    gt_img, gt_cls = np.asarray(gt_img, np.int64), np.asarray(gt_cls, np.int64)
    pred_scores = np.asarray(pred_scores)

    def by_group(img, cls):
        keep = np.flatnonzero((cls >= 1) & (cls < num_classes) & (img >= 0) & (img < n_img))
        key = cls[keep] * n_img + img[keep]
        o = np.argsort(key, kind="stable")          # class, image, then the order inside the image
        return keep[o], key[o]

    rows_p, key_p = by_group(pred_img, pred_cls)
    rows_g, key_g = by_group(gt_img, gt_cls)
    keys = np.union1d(key_p, key_g)
    G = len(keys)
    grp_p, grp_g = np.searchsorted(keys, key_p), np.searchsorted(keys, key_g)
    n_p, n_g = np.bincount(grp_p, minlength=G), np.bincount(grp_g, minlength=G)
    pred_off = np.concatenate([[0], np.cumsum(n_p)])
    gt_off = np.concatenate([[0], np.cumsum(n_g)])
    pair_off = np.concatenate([[0], np.cumsum(n_p * n_g)])
    if max(pred_off[-1], gt_off[-1], pair_off[-1]) >= 2 ** 31:
        raise ValueError("evaluation set too large for int32 offsets")

    # matching order inside each group: np.argsort(scores)[::-1] of the group's scores (test_utils.py:557).  Without
    # ties that is THE descending order, made for all groups at once; a group with ties gets the reference's own call.
    sc = pred_scores[rows_p]
    order = np.lexsort((-sc.astype(np.float64), grp_p))
    s2, g2 = sc[order], grp_p[order]
    tied = np.unique(g2[1:][(s2[1:] == s2[:-1]) & (g2[1:] == g2[:-1])])
    for g in tied:
        a, b = pred_off[g], pred_off[g + 1]
        order[a:b] = a + np.argsort(sc[a:b])[::-1]
    pred_local = order - pred_off[:-1][grp_p]      # grp_p is sorted, so group g's positions are pred_off[g] ..

    group_cls, group_img = keys // max(n_img, 1), keys % max(n_img, 1)
    cls_edges = np.searchsorted(group_cls, np.arange(num_classes + 1))
    return Groups(
        n_img=n_img, num_classes=num_classes, group_cls=group_cls, group_img=group_img,
        pred_off=pred_off.astype(np.int32), gt_off=gt_off.astype(np.int32), pair_off=pair_off.astype(np.int32),
        pair_group=np.repeat(np.arange(G, dtype=np.int32), n_p * n_g),
        pred_idx=rows_p[order].astype(np.int32), pred_local=pred_local, pred_scores=sc[order],
        gt_idx=rows_g.astype(np.int32), cls_pred=pred_off[cls_edges], cls_gt=gt_off[cls_edges])


def _stack(results, key, tail, dtype):
    parts = [np.asarray(r[key], dtype=dtype).reshape((-1,) + tail) for r in results]
    return np.concatenate(parts, axis=0) if parts else np.zeros((0,) + tail, dtype)


def flatten_results(final_results, num_classes):
    """``final_results`` (one dict per image: gt_class_ids, gt_RTs, gt_scales, gt_handle_visibility, pred_class_ids,
    pred_scores, pred_RTs, pred_scales - what catre_custom_evaluator.py:239-245 merges) -> ``Groups`` and the flat
    float32 arrays the kernels read: pred_pose [N, 3, 4], pred_scale [N, 3], gt_pose, gt_scale, gt_hv."""
    n_img = len(final_results)
    n_pred = [len(r["pred_class_ids"]) for r in final_results]
    n_gt = [len(r["gt_class_ids"]) for r in final_results]
    pred_img = np.repeat(np.arange(n_img), n_pred)
    gt_img = np.repeat(np.arange(n_img), n_gt)
    pred_cls = _stack(final_results, "pred_class_ids", (), np.int64)
    gt_cls = _stack(final_results, "gt_class_ids", (), np.int64)
    scores = [np.asarray(r["pred_scores"]).reshape(-1) for r in final_results]
    pred_scores = np.concatenate(scores) if scores else np.zeros(0)
    groups = flatten_groups(pred_img, pred_cls, pred_scores, gt_img, gt_cls, n_img, num_classes)
    arrays = dict(
        pred_pose=np.ascontiguousarray(_stack(final_results, "pred_RTs", (4, 4), np.float32)[:, :3, :]),
        pred_scale=_stack(final_results, "pred_scales", (3,), np.float32),
        gt_pose=np.ascontiguousarray(_stack(final_results, "gt_RTs", (4, 4), np.float32)[:, :3, :]),
        gt_scale=_stack(final_results, "gt_scales", (3,), np.float32),
        gt_hv=_stack(final_results, "gt_handle_visibility", (), np.int32))
    return groups, arrays


def _device(device):
    if not torch.cuda.is_available():
        raise hip.CatreHipError("catre_amd.evaluation runs on HIP devices only (no CPU fallback); no device is present")
    device = torch.device(device)
    if device.type != "cuda":
        raise hip.CatreHipError(f"catre_amd.evaluation runs on HIP devices only (no CPU fallback), got {device}")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def threshold_lists(degree_thresholds, shift_thresholds, iou_3d_thresholds, iou_pose_thres, use_matches_for_pose):
    """The reference's lists (:771-781): 360 degrees / 100 cm appended; the index of ``iou_pose_thres`` (-1: unused)."""
    deg, cm, iou = list(degree_thresholds) + [360], list(shift_thresholds) + [100], list(iou_3d_thresholds)
    sel = -1
    if use_matches_for_pose:
        assert iou_pose_thres in iou
        sel = iou.index(iou_pose_thres)
    return deg, cm, iou, sel


def run_kernels(groups, pred_pose, pred_scale, gt_pose, gt_scale, gt_hv, synset_names, deg, cm, iou, sel, device):
    """The three launches.  pred_pose [T, N, 3, 4] / pred_scale [T, N, 3]: float32 DEVICE tensors; the GT arrays: host
    arrays in the caller's row order.  -> dict of device tensors: iou [T, Q] f32, degcm [T, Q, 2] f64, iou_pred_match
    [T, S, P], iou_gt_match [T, S, NG], pose_pred_match [T, D, C, P], pose_gt_match [T, D, C, NG] (int32; pose
    matches index the IoU-selected subset of the group, -2 = not in it)."""
    hip.require_dev_f32(pred_pose, "pred_pose", (None, None, 3, 4))
    T, N = int(pred_pose.shape[0]), int(pred_pose.shape[1])
    hip.require_dev_f32(pred_scale, "pred_scale", (T, N, 3))
    device = pred_pose.device
    G, P, NG, Q = groups.G, len(groups.pred_idx), len(groups.gt_idx), len(groups.pair_group)
    S, D, C = len(iou), len(deg), len(cm)
    if groups.pred_idx.size and int(groups.pred_idx.max()) >= N:
        raise ValueError("prediction index beyond the pose array")

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)

    i32 = torch.int32
    out = dict(iou=torch.empty((T, Q), dtype=torch.float32, device=device),
               degcm=torch.empty((T, Q, 2), dtype=torch.float64, device=device),
               iou_pred_match=torch.empty((T, S, P), dtype=i32, device=device),
               iou_gt_match=torch.empty((T, S, NG), dtype=i32, device=device),
               pose_pred_match=torch.empty((T, D, C, P), dtype=i32, device=device),
               pose_gt_match=torch.empty((T, D, C, NG), dtype=i32, device=device))
    if G == 0 or T == 0:
        return out
    with torch.cuda.device(device):
        st = hip.stream_ptr(device)
        pred_off, gt_off, pair_off = dev(groups.pred_off, np.int32), dev(groups.gt_off, np.int32), dev(groups.pair_off, np.int32)
        keep = [dev(groups.pred_idx, np.int32), dev(np.asarray(gt_pose, np.float32)[groups.gt_idx], np.float32),
                dev(np.asarray(gt_scale, np.float32)[groups.gt_idx], np.float32),
                dev(np.asarray(gt_hv)[groups.gt_idx], np.int32), dev(groups.pair_group, np.int32),
                dev(class_modes(synset_names)[groups.group_cls], np.int32), dev(rotation_table(), np.float64),
                dev(iou, np.float64), dev(deg, np.float64), dev(cm, np.float64)]
        pred_idx, gtp, gts, gthv, pair_group, modes, cs, th_iou, th_deg, th_cm = keep
        p = hip.ptr
        _call("catre_eval_overlaps", p(pred_pose), p(pred_scale), p(pred_idx), p(gtp), p(gts), p(gthv), p(pred_off),
              p(gt_off), p(pair_off), p(pair_group), p(modes), p(cs), p(out["iou"]), p(out["degcm"]), T, N, P, NG, G, Q, st)
        _call("catre_eval_match_iou", p(out["iou"]), p(pred_off), p(gt_off), p(pair_off), p(th_iou),
              p(out["iou_pred_match"]), p(out["iou_gt_match"]), T, S, P, NG, G, Q, st)
        _call("catre_eval_match_pose", p(out["degcm"]), p(pred_off), p(gt_off), p(pair_off), p(out["iou_pred_match"]),
              p(out["iou_gt_match"]), S, sel, p(th_deg), p(th_cm), p(out["pose_pred_match"]), p(out["pose_gt_match"]),
              T, D, C, P, NG, G, Q, st)
    return out


def aps_from_matches(groups, iou_pred_match, iou_gt_match, pose_pred_match, pose_gt_match, sel):
    """Host part of one iteration (test_utils.py:900-924): matches (numpy, [S, P], [S, NG], [D, C, P], [D, C, NG]) ->
    (iou_3d_aps [num_classes + 1, S], pose_aps [num_classes + 1, D, C])."""
    nc = groups.num_classes
    S, (D, C) = iou_pred_match.shape[0], pose_pred_match.shape[:2]
    iou_3d_aps, pose_aps = np.zeros((nc + 1, S)), np.zeros((nc + 1, D, C))
    for cls_id in range(1, nc):
        p0, p1, g0, g1 = groups.cls_pred[cls_id], groups.cls_pred[cls_id + 1], groups.cls_gt[cls_id], groups.cls_gt[cls_id + 1]
        scores = groups.pred_scores[p0:p1]
        order = np.argsort(scores)[::-1]
        for s in range(S):
            iou_3d_aps[cls_id, s] = ap_from_matches_scores(iou_pred_match[s, p0:p1], scores, g1 - g0, order)
        if sel >= 0:
            pm, gm = iou_pred_match[sel, p0:p1] > -1, iou_gt_match[sel, g0:g1] > -1
            scores = scores[pm]
            order = np.argsort(scores)[::-1]
        else:
            pm, gm = slice(None), np.ones(g1 - g0, dtype=bool)
        n_gt = int(np.count_nonzero(gm))
        for d in range(D):
            for c in range(C):
                pose_aps[cls_id, d, c] = ap_from_matches_scores(pose_pred_match[d, c, p0:p1][pm], scores, n_gt, order)
    iou_3d_aps[-1, :] = np.mean(iou_3d_aps[1:-1, :], axis=0)
    pose_aps[-1] = np.mean(pose_aps[1:-1], axis=0)
    return iou_3d_aps, pose_aps


def compute_independent_mAP(final_results, synset_names=("BG", "bottle", "bowl", "camera", "can", "laptop", "mug"),
                            degree_thresholds=(360,), shift_thresholds=(100,), iou_3d_thresholds=(0.1,),
                            iou_pose_thres=0.1, use_matches_for_pose=True, device="cuda"):
    """The reference's ``compute_independent_mAP`` (test_utils.py:760-924): same arguments, same ``final_results``,
    same ``(iou_3d_aps, pose_aps)``; overlaps and matching on ``device``.  Raises without a HIP device."""
    device = _device(device)
    deg, cm, iou, sel = threshold_lists(degree_thresholds, shift_thresholds, iou_3d_thresholds, iou_pose_thres,
                                        use_matches_for_pose)
    groups, a = flatten_results(final_results, len(synset_names))
    out = run_kernels(groups, torch.from_numpy(a["pred_pose"]).to(device)[None], torch.from_numpy(a["pred_scale"]).to(device)[None],
                      a["gt_pose"], a["gt_scale"], a["gt_hv"], synset_names, deg, cm, iou, sel, device)
    m = {k: out[k][0].cpu().numpy() for k in ("iou_pred_match", "iou_gt_match", "pose_pred_match", "pose_gt_match")}
    return aps_from_matches(groups, m["iou_pred_match"], m["iou_gt_match"], m["pose_pred_match"], m["pose_gt_match"], sel)


def split_groups(groups, out, sel, t=0):
    """Per-group views of ``run_kernels``' arrays for iteration ``t``: {(image, class id): dict} with, in the
    reference's shapes, ``order`` (the `indices` of :557), ``iou`` [np, ng] float32, ``degcm`` [np, ng, 2] for every pair
    (rows in matching order), ``iou_pred_match`` [S, np], ``iou_gt_match`` [S, ng], the subset masks ``pose_pred_sel`` /
    ``pose_gt_sel`` and the compacted ``pose_pred_match`` [D, C, m_p] / ``pose_gt_match`` [D, C, m_g]."""
    h = {k: v[t].cpu().numpy() for k, v in out.items()}
    res = OrderedDict()
    for g in range(groups.G):
        p0, p1, g0, g1, q0 = groups.pred_off[g], groups.pred_off[g + 1], groups.gt_off[g], groups.gt_off[g + 1], groups.pair_off[g]
        n_p, n_g = p1 - p0, g1 - g0
        if sel >= 0:
            ps, gs = h["iou_pred_match"][sel, p0:p1] > -1, h["iou_gt_match"][sel, g0:g1] > -1
        else:
            ps, gs = np.ones(n_p, dtype=bool), np.ones(n_g, dtype=bool)
        res[(int(groups.group_img[g]), int(groups.group_cls[g]))] = dict(
            order=groups.pred_local[p0:p1], scores=groups.pred_scores[p0:p1],
            iou=h["iou"][q0:q0 + n_p * n_g].reshape(n_p, n_g), degcm=h["degcm"][q0:q0 + n_p * n_g].reshape(n_p, n_g, 2),
            iou_pred_match=h["iou_pred_match"][:, p0:p1], iou_gt_match=h["iou_gt_match"][:, g0:g1],
            pose_pred_sel=ps, pose_gt_sel=gs,
            pose_pred_match=h["pose_pred_match"][:, :, p0:p1][:, :, ps], pose_gt_match=h["pose_gt_match"][:, :, g0:g1][:, :, gs])
    return res


def overlaps_and_matches(final_results, synset_names, degree_thresholds, shift_thresholds, iou_3d_thresholds,
                         iou_pose_thres=0.1, use_matches_for_pose=True, device="cuda"):
    """The intermediate arrays of ``compute_independent_mAP`` per (image index, class id) group - see ``split_groups``."""
    device = _device(device)
    deg, cm, iou, sel = threshold_lists(degree_thresholds, shift_thresholds, iou_3d_thresholds, iou_pose_thres,
                                        use_matches_for_pose)
    groups, a = flatten_results(final_results, len(synset_names))
    out = run_kernels(groups, torch.from_numpy(a["pred_pose"]).to(device)[None], torch.from_numpy(a["pred_scale"]).to(device)[None],
                      a["gt_pose"], a["gt_scale"], a["gt_hv"], synset_names, deg, cm, iou, sel, device)
    return split_groups(groups, out, sel)


def format_table(rows):
    """``tabulate(rows, tablefmt="plain")`` for rows of strings with a text column in each: left-aligned cells padded to
    the column width, two spaces between columns, no trailing blanks."""
    width = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    return "\n".join("  ".join(c.ljust(w) for c, w in zip(r, width)).rstrip() for r in rows)


def table_rows(iou_3d_aps, pose_aps, obj_names):
    """The rows of catre_custom_evaluator.py:262-311 for the evaluator's thresholds: header, IoU25/50/75,
    re5te2 .. re10te10, re5, re10, te2, te5 (the reference zips te2 / te5 against the first two shift thresholds)."""
    synset_names = ["BG"] + list(obj_names)
    cols = [i for i, n in enumerate(synset_names) if n in obj_names] + [-1]
    rows = [["objects"] + list(obj_names) + [f"Avg({len(obj_names)})"]]
    for metric, thres in zip(["IoU25", "IoU50", "IoU75"], IOU_3D_THRESHOLDS[1:]):
        rows.append([metric] + [f"{100 * iou_3d_aps[i, IOU_3D_THRESHOLDS.index(thres)]:.2f}" for i in cols])
    for metric, (d, s) in zip(["re5te2", "re5te5", "re10te2", "re10te5", "re10te10"], DEGREE_SHIFT_THRESHOLDS):
        rows.append([metric] + [f"{100 * pose_aps[i, DEGREE_THRESHOLDS.index(d), SHIFT_THRESHOLDS.index(s)]:.2f}" for i in cols])
    for metric, d in zip(["re5", "re10"], DEGREE_THRESHOLDS):
        rows.append([metric] + [f"{100 * pose_aps[i, DEGREE_THRESHOLDS.index(d), -1]:.2f}" for i in cols])
    for metric, s in zip(["te2", "te5"], SHIFT_THRESHOLDS):
        rows.append([metric] + [f"{100 * pose_aps[i, -1, SHIFT_THRESHOLDS.index(s)]:.2f}" for i in cols])
    return rows


class NocsEvaluator:
    """Device-side stand-in for the reference's ``CATRE_Evaluator`` of catre_custom_evaluator.py (the mAP one).

    ``set_gts`` takes the mapping its ``get_gts()`` builds (:81-102; reading the dataset catalogs is the caller's
    business), ``process`` keeps a batch's predictions as device tensors - no synchronisation, no per-object Python -
    and ``evaluate`` runs all ``n_iter_test + 1`` iterations through the three kernels at once.  ``train_objs`` is kept
    for the caller as the reference keeps it: its ``process`` does not map labels through it either (:156-157)."""

    def __init__(self, obj_names, n_iter_test, train_objs=None):
        self.obj_names = list(obj_names)
        self.n_iter_test = int(n_iter_test)
        self.train_objs = train_objs
        self.gt_dict = OrderedDict()
        self._image_index = {}
        self.timings = {}
        self.reset()

    def set_gts(self, gt_dict):
        """``{scene_im_id: dict(gt_class_ids, gt_RTs [n, 4, 4], gt_scales, gt_handle_visibility, ...)}``; its order is
        the image order of the evaluation (:240)."""
        self.gt_dict = gt_dict
        self._image_index = {k: i for i, k in enumerate(gt_dict)}

    def reset(self):
        self._batches = []

    def process(self, scene_im_ids, batch, out_dict, scores=None):
        """``scene_im_ids``: the scene_im_id of each image of the batch (``inputs[i]["scene_im_id"]``); ``batch["im_id"]``
        indexes it per object, ``batch["obj_cls"] + 1`` is the class id (:157).  ``out_dict``: ``pose_i`` [B, 3, 4] /
        ``scale_i`` [B, 3] for i = 0 .. n_iter_test.  ``scores``: [B] (tensor or array-like), default 1.0 (:151-154)."""
        T = self.n_iter_test + 1
        pose = torch.stack([out_dict[f"pose_{i}"].detach() for i in range(T)])
        scale = torch.stack([out_dict[f"scale_{i}"].detach() for i in range(T)])
        hip.require_dev_f32(pose, "pose", (T, None, 3, 4))
        hip.require_dev_f32(scale, "scale", (T, pose.shape[1], 3))
        device = pose.device
        lut = torch.tensor([self._image_index.get(s, -1) for s in scene_im_ids], dtype=torch.int64).pin_memory()
        img = lut.to(device, non_blocking=True)[batch["im_id"].detach().to(device).long()]
        cls = batch["obj_cls"].detach().to(device).long() + 1
        if scores is not None:
            if not isinstance(scores, torch.Tensor):
                scores = torch.as_tensor(np.asarray(scores, dtype=np.float64)).pin_memory()
            scores = scores.detach().to(device, non_blocking=True).double()
        self._batches.append((img, cls, pose, scale, scores))

    def evaluate(self):
        """-> ``{"iter{i}": dict(iou_3d_aps, pose_aps, rows, table)}`` for i = 0 .. n_iter_test, the arrays being what
        ``compute_independent_mAP`` returns on the reference's merged list for that iteration (:237-260) and ``table``
        the text of its ``_tab_iter{i}.txt`` without the final newline."""
        if not self.gt_dict:
            raise RuntimeError("NocsEvaluator.evaluate(): no ground truths - call set_gts() first")
        if not self._batches:
            raise RuntimeError("Please run inference first")            # catre_custom_evaluator.py:234
        t0 = time.perf_counter()
        device = _device(self._batches[0][2].device)
        synset_names = ["BG"] + self.obj_names
        deg, cm, iou, sel = threshold_lists(DEGREE_THRESHOLDS, SHIFT_THRESHOLDS, IOU_3D_THRESHOLDS, 0.1, True)
        pose = torch.cat([b[2] for b in self._batches], dim=1).contiguous()
        scale = torch.cat([b[3] for b in self._batches], dim=1).contiguous()
        img = torch.cat([b[0] for b in self._batches]).cpu().numpy()
        cls = torch.cat([b[1] for b in self._batches]).cpu().numpy()
        scores = torch.cat([torch.ones(len(b[0]), dtype=torch.float64, device=device) if b[4] is None else b[4]
                            for b in self._batches]).cpu().numpy()
        gts = list(self.gt_dict.values())
        n_gt = [len(g["gt_class_ids"]) for g in gts]
        groups = flatten_groups(img, cls, scores, np.repeat(np.arange(len(gts)), n_gt),
                                _stack(gts, "gt_class_ids", (), np.int64), len(gts), len(synset_names))
        gt_pose = np.ascontiguousarray(_stack(gts, "gt_RTs", (4, 4), np.float32)[:, :3, :])
        t1 = time.perf_counter()
        out = run_kernels(groups, pose, scale, gt_pose, _stack(gts, "gt_scales", (3,), np.float32),
                          _stack(gts, "gt_handle_visibility", (), np.int32), synset_names, deg, cm, iou, sel, device)
        m = {k: out[k].cpu().numpy() for k in ("iou_pred_match", "iou_gt_match", "pose_pred_match", "pose_gt_match")}
        t2 = time.perf_counter()
        res = OrderedDict()
        for t in range(self.n_iter_test + 1):
            iou_3d_aps, pose_aps = aps_from_matches(groups, m["iou_pred_match"][t], m["iou_gt_match"][t],
                                                    m["pose_pred_match"][t], m["pose_gt_match"][t], sel)
            rows = table_rows(iou_3d_aps, pose_aps, self.obj_names)
            res[f"iter{t}"] = dict(iou_3d_aps=iou_3d_aps, pose_aps=pose_aps, rows=rows, table=format_table(rows))
        t3 = time.perf_counter()
        # host flattening / upload + kernels + download / host AP, seconds, of the last call
        self.timings = dict(flatten_s=t1 - t0, device_s=t2 - t1, ap_s=t3 - t2)
        return res


def add_errors(pose_est, pose_gt, pts, scale_est=None, scale_gt=None, symmetric=False):
    """ADD (``symmetric=False``) or ADD-S per instance on the device (``lib/pysixd/pose_error.py``: ``add`` :256-271,
    ``adi`` :274-296): pose_est, pose_gt [I,3,4], pts [I,n,3] or [n,3] (model points, shared) fp32 on the device, optional
    scale_est / scale_gt [I,3] applied to the points first -> [I] fp32, the mean distance from every model point under the
    ground truth to the same point (ADD) or to the nearest point (ADD-S) of the model under the estimate - the set the
    reference builds its KD-tree on.  One ``catre_nn_stats`` call (``tracking.nn_stats``), nothing read back."""
    from .tracking import nn_stats

    if not isinstance(pose_est, torch.Tensor) or pose_est.ndim != 3 or tuple(pose_est.shape[1:]) != (3, 4):
        raise ValueError("pose_est: expected a [I,3,4] tensor")
    I = pose_est.shape[0]
    if isinstance(pts, torch.Tensor) and pts.ndim == 2:
        pts = pts[None].expand(I, *pts.shape)
    return nn_stats(pts, pts, src_pose=pose_gt, src_scale=scale_gt, dst_pose=pose_est, dst_scale=scale_est,
                    paired=not symmetric).mean_d
