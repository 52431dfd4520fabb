"""Device evaluator (catre_amd/evaluation.py, csrc/catre_eval.h) against tests/golden/eval_nocs.npz, which the unmodified
reference wrote (tools/make_eval_golden.py): two sets of 300 synthetic images, `exact` (reference run in float64 on the
float32 inputs) and `as_called` (reference run as its evaluator calls it, float32 predictions, all scores 1.0).

Tolerances on `exact`: IoU 1.2e-7 abs (one float32 ulp below 1: the reference stores IoU in a float32 array), degree and
cm 1e-7 abs (double arithmetic; the generator keeps every arccos argument <= 1 - 1e-12, which bounds acos' conditioning),
every match array equal, AP arrays 1e-12 (same float64 operations on equal matches).  On `as_called`: match arrays equal,
AP arrays 1e-12 - the generator keeps every IoU / degree / cm >= 1e-4 from every threshold, fp32-vs-fp64 differences of
these quantities being <= 1e-5."""
import ctypes
import functools
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from catre_amd import evaluation as E
from catre_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_nocs.npz")
SETS = ("exact", "as_called")


@functools.lru_cache(maxsize=None)
def _load(name):
    """-> dict: the set's arrays, `meta`, `thr` (the three threshold lists) and `results` = the final_results list
    with float32 poses and scales, as a model returns them."""
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    s = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
    s["meta"], s["names"] = meta["sets"][name], meta["sets"][name]["synset_names"]
    s["thr"] = (meta["degree_thresholds"], meta["shift_thresholds"], meta["iou_3d_thresholds"])
    g_off = np.concatenate([[0], np.cumsum(s["n_gt"].astype(np.int64))])
    p_off = np.concatenate([[0], np.cumsum(s["n_pred"].astype(np.int64))])
    last = np.tile(np.array([[[0, 0, 0, 1]]], np.float32), (max(g_off[-1], p_off[-1]), 1, 1))
    gt44 = np.concatenate([s["gt_RT"], last[:g_off[-1]]], 1)
    pr44 = np.concatenate([s["pred_RT"], last[:p_off[-1]]], 1)
    s["g_off"], s["p_off"] = g_off, p_off
    s["results"] = [dict(gt_class_ids=s["gt_cls"][a:b].astype(np.int32), gt_RTs=gt44[a:b], gt_scales=s["gt_scale"][a:b],
                         gt_handle_visibility=s["gt_hv"][a:b].astype(np.int32), pred_class_ids=s["pred_cls"][c:d].astype(np.int32),
                         pred_scores=s["pred_scores"][c:d], pred_RTs=pr44[c:d], pred_scales=s["pred_scale"][c:d])
                    for a, b, c, d in zip(g_off[:-1], g_off[1:], p_off[:-1], p_off[1:])]
    # offsets of every recorded call into the concatenated arrays
    for k, n in (("c_p", s["call_np"]), ("c_g", s["call_ng"]), ("c_mp", s["call_mp"]), ("c_mg", s["call_mg"]),
                 ("c_q", s["call_np"].astype(np.int64) * s["call_ng"]), ("c_mq", s["call_mp"].astype(np.int64) * s["call_mg"])):
        s[k] = np.concatenate([[0], np.cumsum(n.astype(np.int64))])
    s["sel"] = s["thr"][2].index(0.1)
    return s


def _groups(s):
    groups, arrays = E.flatten_results(s["results"], len(s["names"]))
    index = {(int(i), int(c)): g for g, (i, c) in enumerate(zip(groups.group_img, groups.group_cls))}
    return groups, arrays, index


# ---------------------------------------------------------------------------------------------- CPU


def test_fixture_holds_the_required_cases():
    assert os.path.getsize(GOLDEN) < 270 * 1024
    for name in SETS:
        s = _load(name)
        assert s["meta"]["images"] == len(s["results"]) == 300
        assert s["call_np"].max() >= 8 or s["call_ng"].max() >= 8
        d = s["meta"]["min_distance"]
        assert min(d["iou"], d["deg"], d["cm"]) >= 1e-4 and d["iou_tie"] > 0 and d["sum_tie"] > 0
    assert "phone" in _load("exact")["names"] and "phone" not in _load("as_called")["names"]
    assert len(set(_load("exact")["pred_scores"])) == len(_load("exact")["pred_scores"])
    assert (_load("as_called")["pred_scores"] == 1.0).all()


@pytest.mark.parametrize("name", SETS)
def test_flattening_reproduces_the_recorded_in_image_order(name):
    """CSR flattening + score permutations: every recorded call of compute_3d_matches is one group with the recorded
    sizes, the recorded `indices` (np.argsort(scores)[::-1] of the group) and the right rows of the flat arrays."""
    s = _load(name)
    groups, arrays, index = _groups(s)
    assert groups.G == len(s["call_img"])
    assert (np.diff(groups.group_cls) >= 0).all()                  # class-major: a class is one contiguous range
    for k, (im, c) in enumerate(zip(s["call_img"], s["call_cls"])):
        g = index[(int(im), int(c))]
        p0, p1, g0, g1 = groups.pred_off[g], groups.pred_off[g + 1], groups.gt_off[g], groups.gt_off[g + 1]
        assert (p1 - p0, g1 - g0) == (s["call_np"][k], s["call_ng"][k])
        assert groups.pair_off[g + 1] - groups.pair_off[g] == (p1 - p0) * (g1 - g0)
        want = s["order"][s["c_p"][k]:s["c_p"][k + 1]]
        assert np.array_equal(groups.pred_local[p0:p1], want), (im, c)
        rows = s["p_off"][im] + np.flatnonzero(s["results"][im]["pred_class_ids"] == c)
        assert np.array_equal(groups.pred_idx[p0:p1], rows[want])
        assert np.array_equal(groups.gt_idx[g0:g1], s["g_off"][im] + np.flatnonzero(s["results"][im]["gt_class_ids"] == c))
    assert (groups.pair_group == np.repeat(np.arange(groups.G), np.diff(groups.pair_off))).all()
    assert arrays["pred_pose"].dtype == np.float32 and arrays["pred_pose"].shape[1:] == (3, 4)


def _recorded_flat_matches(s, groups, index):
    """The recorded match arrays laid out as run_kernels lays its results out."""
    D, C, S = len(s["thr"][0]) + 1, len(s["thr"][1]) + 1, len(s["thr"][2])
    P, NG = len(groups.pred_idx), len(groups.gt_idx)
    ipm, igm = np.full((S, P), -9, np.int32), np.full((S, NG), -9, np.int32)
    ppm, pgm = np.full((D, C, P), -2, np.int32), np.full((D, C, NG), -2, np.int32)
    for k, (im, c) in enumerate(zip(s["call_img"], s["call_cls"])):
        g = index[(int(im), int(c))]
        p0, p1, g0, g1 = groups.pred_off[g], groups.pred_off[g + 1], groups.gt_off[g], groups.gt_off[g + 1]
        ipm[:, p0:p1] = s["iou_pred_match"][:, s["c_p"][k]:s["c_p"][k + 1]]
        igm[:, g0:g1] = s["iou_gt_match"][:, s["c_g"][k]:s["c_g"][k + 1]]
        ps, gs = ipm[s["sel"], p0:p1] > -1, igm[s["sel"], g0:g1] > -1
        ppm[:, :, p0 + np.flatnonzero(ps)] = s["pose_pred_match"][:, :, s["c_mp"][k]:s["c_mp"][k + 1]]
        pgm[:, :, g0 + np.flatnonzero(gs)] = s["pose_gt_match"][:, :, s["c_mg"][k]:s["c_mg"][k + 1]]
    assert (ipm > -9).all() and (igm > -9).all()
    return ipm, igm, ppm, pgm


@pytest.mark.parametrize("name", SETS)
def test_host_ap_reproduces_the_reference_aps_from_its_recorded_matches(name):
    s = _load(name)
    groups, _, index = _groups(s)
    iou_aps, pose_aps = E.aps_from_matches(groups, *_recorded_flat_matches(s, groups, index), s["sel"])
    assert iou_aps.shape == s["iou_3d_aps"].shape and pose_aps.shape == s["pose_aps"].shape
    assert np.abs(iou_aps - s["iou_3d_aps"]).max() <= 1e-12
    assert np.abs(pose_aps - s["pose_aps"]).max() <= 1e-12
    assert s["iou_3d_aps"][1:-1].min() > 0 and 0 < s["pose_aps"][-1, 0, 0] < s["pose_aps"][-1, -1, -1]   # not a trivial set


def test_ap_function_follows_the_reference_formula_on_a_written_out_case():
    # 4 predictions (scores descending as given), hits at ranks 1 and 3, 3 GTs: precisions 1, 1/2, 2/3, 1/2 ->
    # running max 1, 2/3, 2/3, 1/2; recall steps of 1/3 (float32) at ranks 1 and 3, then the padded step to 1 at precision 0
    third = float(np.float32(1) / np.float32(3))
    two_thirds = float(np.float32(2) / np.float32(3))
    want = third * 1.0 + (two_thirds - third) * (2 / 3)
    got = E.ap_from_matches_scores(np.array([0, -1, 2, -1]), np.array([.9, .8, .7, .6]), np.zeros(3))
    assert abs(got - want) <= 1e-15
    assert E.ap_from_matches_scores(np.zeros(0), np.zeros(0), np.zeros(0)) == 0      # a class without any instance


def test_new_symbols_are_exported():
    lib = hip.load()
    for n in ("catre_eval_overlaps", "catre_eval_match_iou", "catre_eval_match_pose"):
        assert n in hip.EXPORTED_SYMBOLS and hasattr(lib, n)


def test_bad_arguments_return_bad_arg_without_a_device():
    lib, nul = hip.load(), ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    ok = ctypes.cast(buf, ctypes.c_void_p)      # host memory: never dereferenced, the checks come first
    assert lib.catre_eval_overlaps(*[nul] * 14, 1, 4, 4, 4, 1, 16, nul) == -1                 # null arrays
    assert lib.catre_eval_overlaps(*[ok] * 14, 0, 4, 4, 4, 1, 16, nul) == -1                  # T < 1
    assert lib.catre_eval_overlaps(*[ok] * 14, 1, 4, 4, 4, 1, 17, nul) == -1                  # more pairs than P x NG
    assert lib.catre_eval_overlaps(*[ok] * 14, 1, 2, 4, 4, 1, 16, nul) == -1                  # more predictions than rows
    assert lib.catre_eval_match_iou(*[nul] * 7, 1, 4, 4, 4, 1, 16, nul) == -1
    assert lib.catre_eval_match_iou(*[ok] * 7, 1, 0, 4, 4, 1, 16, nul) == -1                  # no threshold
    assert lib.catre_eval_match_iou(*[ok] * 7, 1, 4, -1, 4, 1, 16, nul) == -1
    assert lib.catre_eval_match_pose(*[nul] * 6, 4, 0, *[nul] * 4, 1, 3, 4, 4, 4, 1, 16, nul) == -1
    assert lib.catre_eval_match_pose(*[ok] * 6, 4, 4, *[ok] * 4, 1, 3, 4, 4, 4, 1, 16, nul) == -1      # sel >= S
    assert lib.catre_eval_match_pose(*[ok] * 4, nul, nul, 4, 0, *[ok] * 4, 1, 3, 4, 4, 4, 1, 16, nul) == -1  # sel without matches


def test_there_is_no_cpu_fallback():
    s = _load("exact")
    with pytest.raises(hip.CatreHipError):
        E.compute_independent_mAP(s["results"][:3], s["names"], *s["thr"], device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(hip.CatreHipError):
            E.compute_independent_mAP(s["results"][:3], s["names"], *s["thr"])


def test_table_rows_carry_the_reference_names_and_formatting():
    obj = ["bottle", "bowl", "camera", "can", "laptop", "mug"]
    rng = np.random.default_rng(0)
    iou, pose = rng.random((8, 4)), rng.random((8, 3, 4))
    rows = E.table_rows(iou, pose, obj)
    assert [r[0] for r in rows] == ["objects", "IoU25", "IoU50", "IoU75", "re5te2", "re5te5", "re10te2", "re10te5", "re10te10",
                                    "re5", "re10", "te2", "te5"]
    assert rows[0] == ["objects"] + obj + ["Avg(6)"] and all(len(r) == 8 for r in rows)
    assert rows[2][1:] == [f"{100 * iou[i, 2]:.2f}" for i in (1, 2, 3, 4, 5, 6, -1)]                       # IoU50
    assert rows[6][1:] == [f"{100 * pose[i, 1, 0]:.2f}" for i in (1, 2, 3, 4, 5, 6, -1)]                   # re10te2
    assert rows[9][1:] == [f"{100 * pose[i, 0, -1]:.2f}" for i in (1, 2, 3, 4, 5, 6, -1)]                  # re5
    assert rows[12][1:] == [f"{100 * pose[i, -1, 1]:.2f}" for i in (1, 2, 3, 4, 5, 6, -1)]                 # te5
    text = E.format_table(rows).splitlines()
    assert text[0] == "objects   bottle  bowl   camera  can    laptop  mug    Avg(6)"     # tabulate's "plain" layout
    assert all(ln == ln.rstrip() and ln.split() == r for ln, r in zip(text, rows))


# ---------------------------------------------------------------------------------------------- GPU


@functools.lru_cache(maxsize=None)
def _device_run(name):
    s = _load(name)
    per_group = E.overlaps_and_matches(s["results"], s["names"], *s["thr"])
    aps = E.compute_independent_mAP(s["results"], s["names"], *s["thr"])
    return per_group, aps


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_device_matches_and_aps_equal_the_reference(name):
    s = _load(name)
    per_group, (iou_aps, pose_aps) = _device_run(name)
    assert len(per_group) == len(s["call_img"])
    for k, (im, c) in enumerate(zip(s["call_img"], s["call_cls"])):
        r = per_group[(int(im), int(c))]
        where = f"{name} image {im} class {c}"
        assert np.array_equal(r["order"], s["order"][s["c_p"][k]:s["c_p"][k + 1]]), where
        assert np.array_equal(r["iou_pred_match"], s["iou_pred_match"][:, s["c_p"][k]:s["c_p"][k + 1]]), where
        assert np.array_equal(r["iou_gt_match"], s["iou_gt_match"][:, s["c_g"][k]:s["c_g"][k + 1]]), where
        assert np.array_equal(r["pose_pred_match"], s["pose_pred_match"][:, :, s["c_mp"][k]:s["c_mp"][k + 1]]), where
        assert np.array_equal(r["pose_gt_match"], s["pose_gt_match"][:, :, s["c_mg"][k]:s["c_mg"][k + 1]]), where
    d_iou, d_pose = np.abs(iou_aps - s["iou_3d_aps"]).max(), np.abs(pose_aps - s["pose_aps"]).max()
    print(f"{name}: max |AP - reference| IoU {d_iou:.3e} pose {d_pose:.3e}")
    assert d_iou <= 1e-12 and d_pose <= 1e-12


@pytest.mark.gpu
def test_device_overlaps_equal_the_reference_in_double():
    s = _load("exact")
    per_group, _ = _device_run("exact")
    e_iou = e_deg = e_cm = 0.0
    n_pairs = 0
    for k, (im, c) in enumerate(zip(s["call_img"], s["call_cls"])):
        r = per_group[(int(im), int(c))]
        want = s["iou"][s["c_q"][k]:s["c_q"][k + 1]].reshape(r["iou"].shape)
        assert r["iou"].dtype == np.float32
        e_iou = max(e_iou, np.abs(r["iou"].astype(np.float64) - want).max(initial=0))
        got = r["degcm"][r["pose_pred_sel"]][:, r["pose_gt_sel"]]        # the reference computes the IoU-matched subset only
        want = s["degcm"][s["c_mq"][k]:s["c_mq"][k + 1]].reshape(got.shape)
        e_deg = max(e_deg, np.abs(got[..., 0] - want[..., 0]).max(initial=0))
        e_cm = max(e_cm, np.abs(got[..., 1] - want[..., 1]).max(initial=0))
        n_pairs += want.shape[0] * want.shape[1]
        assert not np.isnan(r["degcm"]).any() and not np.isnan(r["iou"]).any()
    print(f"max abs err: IoU {e_iou:.3e} degree {e_deg:.3e} cm {e_cm:.3e} over {len(s['iou'])} / {n_pairs} pairs")
    assert len(s["iou"]) > 500 and n_pairs > 300
    assert e_iou <= 1.2e-7 and e_deg <= 1e-7 and e_cm <= 1e-7


def _evaluator_inputs(s, n_img, T, seed):
    """The first n_img images of a set as a model would deliver them: objects in shuffled order, T iterations (the last one
    the fixture's predictions, the others perturbed), and the final_results list equivalent to each iteration."""
    rng = np.random.default_rng(seed)
    n = int(s["p_off"][n_img])
    img_of = np.repeat(np.arange(n_img), s["n_pred"][:n_img])
    perm = rng.permutation(n)
    pose = np.stack([s["pred_RT"][:n] + np.float32(0.01 * (T - 1 - t)) * rng.standard_normal((n, 3, 4)).astype(np.float32)
                     for t in range(T)])
    scale = np.stack([s["pred_scale"][:n] * np.float32(1 + 0.02 * (T - 1 - t)) for t in range(T)])
    assert np.array_equal(pose[-1], s["pred_RT"][:n])
    gt_dict = OrderedDict((f"scene/{i}", {k: s["results"][i][k] for k in ("gt_class_ids", "gt_RTs", "gt_scales", "gt_handle_visibility")})
                          for i in range(n_img))
    last = np.array([[0, 0, 0, 1]], np.float32)
    finals = []
    for t in range(T):
        res = []
        for i in range(n_img):
            rows = perm[img_of[perm] == i]                           # the image's objects in the order they are processed
            res.append(dict(gt_dict[f"scene/{i}"], pred_class_ids=s["pred_cls"][rows].astype(np.int32), pred_scores=np.ones(len(rows)),
                            pred_RTs=np.stack([np.concatenate([m, last]) for m in pose[t, rows]]) if len(rows) else np.zeros((0, 4, 4), np.float32),
                            pred_scales=scale[t, rows]))
        finals.append(res)
    return perm, img_of, pose, scale, gt_dict, finals


def _feed(ev, s, perm, img_of, pose, scale, n_batches):
    T = pose.shape[0]
    for rows in np.array_split(perm, n_batches):
        ims = sorted(set(img_of[rows].tolist()))
        batch = dict(im_id=torch.tensor([ims.index(i) for i in img_of[rows]]).cuda(),
                     obj_cls=torch.tensor(s["pred_cls"][rows].astype(np.int64) - 1).cuda())
        out = {f"pose_{t}": torch.from_numpy(pose[t, rows]).cuda() for t in range(T)}
        out.update({f"scale_{t}": torch.from_numpy(scale[t, rows]).cuda() for t in range(T)})
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                      # process() must not synchronise
        try:
            ev.process([f"scene/{i}" for i in ims], batch, out)
        finally:
            torch.cuda.set_sync_debug_mode("default")


@pytest.mark.gpu
def test_nocs_evaluator_equals_compute_independent_map_per_iteration():
    s = _load("as_called")
    T, n_img = 5, 120
    perm, img_of, pose, scale, gt_dict, finals = _evaluator_inputs(s, n_img, T, seed=3)
    ev = E.NocsEvaluator(s["names"][1:], n_iter_test=T - 1)
    ev.set_gts(gt_dict)
    _feed(ev, s, perm, img_of, pose, scale, n_batches=4)
    res = ev.evaluate()
    assert list(res) == [f"iter{t}" for t in range(T)]
    thr = (E.DEGREE_THRESHOLDS, E.SHIFT_THRESHOLDS, E.IOU_3D_THRESHOLDS)
    for t in range(T):
        iou_aps, pose_aps = E.compute_independent_mAP(finals[t], s["names"], *thr)
        assert np.array_equal(res[f"iter{t}"]["iou_3d_aps"], iou_aps) and np.array_equal(res[f"iter{t}"]["pose_aps"], pose_aps)
        rows = res[f"iter{t}"]["rows"]
        assert rows == E.table_rows(iou_aps, pose_aps, s["names"][1:]) and rows[1][0] == "IoU25" and rows[-1][0] == "te5"
        assert rows[2][-1] == f"{100 * iou_aps[-1, 2]:.2f}" and res[f"iter{t}"]["table"] == E.format_table(rows)
    assert not np.array_equal(res["iter0"]["pose_aps"], res[f"iter{T - 1}"]["pose_aps"])     # the iterations are told apart
    # reset() clears the collected predictions
    ev.reset()
    with pytest.raises(RuntimeError):
        ev.evaluate()
    keep = perm[img_of[perm] < 40]
    _feed(ev, s, keep, img_of, pose, scale, n_batches=2)
    again = ev.evaluate()
    first40 = [[dict(r) for r in f[:40]] + [dict(r, pred_class_ids=r["pred_class_ids"][:0], pred_scores=r["pred_scores"][:0],
                                                 pred_RTs=r["pred_RTs"][:0], pred_scales=r["pred_scales"][:0]) for r in f[40:]]
               for f in finals]
    want = E.compute_independent_mAP(first40[T - 1], s["names"], *thr)
    assert np.array_equal(again[f"iter{T - 1}"]["iou_3d_aps"], want[0]) and np.array_equal(again[f"iter{T - 1}"]["pose_aps"], want[1])


@pytest.mark.gpu
def test_number_of_abi_calls_does_not_depend_on_the_number_of_images():
    s = _load("as_called")
    counts = []
    for n_img in (30, 300):
        perm, img_of, pose, scale, gt_dict, _ = _evaluator_inputs(s, n_img, 2, seed=5)
        ev = E.NocsEvaluator(s["names"][1:], n_iter_test=1)
        ev.set_gts(gt_dict)
        _feed(ev, s, perm, img_of, pose, scale, n_batches=3)
        before = E.abi_call_count()
        ev.evaluate()
        counts.append(E.abi_call_count() - before)
    assert counts == [3, 3]


def _rt(R, t):
    return np.concatenate([np.concatenate([np.asarray(R, np.float32), np.asarray(t, np.float32)[:, None]], 1),
                           np.array([[0, 0, 0, 1]], np.float32)], 0)


def _image(cls, gts, preds, scores=None):
    return dict(gt_class_ids=np.full(len(gts), cls, np.int32), gt_RTs=np.stack([_rt(R, t) for R, t, _ in gts]),
                gt_scales=np.array([sc for _, _, sc in gts], np.float32), gt_handle_visibility=np.ones(len(gts), np.int32),
                pred_class_ids=np.full(len(preds), cls, np.int32), pred_scores=np.ones(len(preds)) if scores is None else np.asarray(scores),
                pred_RTs=np.stack([_rt(R, t) for R, t, _ in preds]), pred_scales=np.array([sc for _, _, sc in preds], np.float32))


@pytest.mark.gpu
def test_documented_behaviours_outside_the_fixtures():
    names = ["BG", "bottle", "bowl", "phone", "can", "laptop", "mug"]
    eye, laptop = np.eye(3), 5
    rng = np.random.default_rng(1)
    # image 0 - an IoU EQUAL to the threshold: unit GT cube, prediction = its lower half -> IoU = 0.5 / (1 + 0.5 - 0.5) =
    # 0.5 exactly; a second GT (IoU 0.25 / 1.25 = 0.2 with the prediction) stays free as well at threshold 0.5
    im0 = _image(laptop, [(eye, [0, 0, 0], [1, 1, 1]), (eye, [0, 0, -0.75], [1, 1, 1])], [(eye, [0, 0, -0.25], [1, 1, 0.5])])
    # image 1 - ties: two identical GTs, two identical predictions.  Equal IoUs: the LATER GT wins, so prediction 1
    # (np.argsort([1, 1])[::-1] puts it first) takes GT 1, prediction 0 takes GT 0.  Equal degree + cm sums: the EARLIER GT
    # wins, so the first prediction in matching order takes GT 0 and the second GT 1.
    g = (eye, [0.5, 0, 1], [0.2, 0.3, 0.2])
    p = (eye, [0.51, 0, 1], [0.2, 0.3, 0.2])
    im1 = _image(laptop, [g, g], [p, p])
    # images 2..7 - the clamp: prediction == GT for a y-symmetric class, the flip class and a generic class; rounding may
    # push the arccos argument past 1, where the reference's unclamped branches return NaN: here the angle is 0 within
    # arccos' resolution at 1 (acos(1 - 2.2e-16) = 2.1e-8 rad = 1.2e-6 degree; a few ulps of the argument -> 1e-5 degree)
    clamp = []
    for cls in (1, 1, 3, 3, laptop, laptop):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.linalg.det(q))
        o = (q, rng.uniform(-0.2, 0.2, 3) + [0, 0, 1], rng.uniform(0.1, 0.3, 3))
        clamp.append(_image(cls, [o], [o]))
    res = E.overlaps_and_matches([im0, im1] + clamp, names, [5, 10], [2, 5, 10], [0.1, 0.25, 0.5, 0.75])

    r = res[(0, laptop)]
    assert r["iou"][0, 0] == 0.5 and abs(float(r["iou"][0, 1]) - 0.2) < 1e-7
    assert r["iou_pred_match"].tolist() == [[0], [0], [-1], [-1]]
    assert r["iou_gt_match"].tolist() == [[0, -1], [0, -1], [-1, -1], [-1, -1]]

    r = res[(1, laptop)]
    assert r["order"].tolist() == [1, 0] and r["iou"][0, 0] == r["iou"][0, 1] > 0.75
    assert (r["iou_pred_match"] == [1, 0]).all() and (r["iou_gt_match"] == [1, 0]).all()
    assert r["degcm"][0, 0, 0] <= 1e-5 and abs(r["degcm"][0, 0, 1] - 1.0) < 1e-5          # 0 degree, 1 cm
    assert r["degcm"][0, 0, 0] + r["degcm"][0, 0, 1] == r["degcm"][0, 1, 0] + r["degcm"][0, 1, 1]
    assert (r["pose_pred_match"] == [0, 1]).all() and (r["pose_gt_match"] == [0, 1]).all()

    # a y-axis angle is normalised by both norms: its argument is 1 within a few ulps.  The trace branches see the float32
    # rounding of the rotation (|R R^T - I| ~ 1e-7 after the cbrt(det) division): acos(1 - 3e-7) = 0.044 degree at most.
    for k, (cls, bound) in enumerate(((1, 1e-5), (1, 1e-5), (3, 0.05), (3, 0.05), (laptop, 0.05), (laptop, 0.05))):
        r = res[(2 + k, cls)]
        assert np.isfinite(r["degcm"]).all() and 0 <= r["degcm"][0, 0, 0] <= bound and r["degcm"][0, 0, 1] == 0, (cls, r["degcm"])
        assert abs(float(r["iou"][0, 0]) - 1) <= 1.2e-7
        assert (r["iou_pred_match"] == 0).all() and (r["pose_pred_match"] == 0).all() and (r["pose_gt_match"] == 0).all()
