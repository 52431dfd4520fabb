"""Tracking on the device (``catre_amd/tracking.py``, ``csrc/catre_track.h``): the nearest-neighbour kernel against the
fp64 restatement ``tests/track_ref.py`` (itself pinned to the reference's ``pose_error.add`` / ``adi`` by
``tests/test_track_host.py``), the gate, and ``Tracker.step`` against the composition written out by hand.

Distance bounds, derived from the arithmetic (u = 2^-24, the fp32 unit round-off):
* without transforms the inputs are exact; a coordinate difference carries one rounding, the two fmas and the product three
  more, the square root halves the relative error of d^2 and adds one: under 4 u d.  Bound 8 u d.
* with transforms a point R (s x) + t carries one rounding per product / fma / sum and coordinate - under 4 sqrt(3) u |s x|
  + u |p| <= 8 u |p| for the objects here - on both ends of a distance.  Bound 16 u (max |p| + max |q|).
* mean_d is accumulated in double from the fp32 square roots and rounded once: the same bounds.
A neighbour index is compared where the restatement's runner-up is further than twice the bound behind (otherwise both are
right answers); ``tests/test_track_host.py`` checks on the CPU that this skips at most 1 % of the points of any case.
"""
import os

import numpy as np
import pytest
import torch

from tests import track_ref as REF
from tests.track_cases import (CHUNK, TILE, U, add_rows, dev as _dev, distance_bound, edge_cases, edge_data,  # noqa: F401
                               edge_reference, edge_rows, run_nn as _run, worst, worst_point)
from tests.util import GOLDEN_DIR


# ---- 1. edges against the restatement ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("transforms", [False, True], ids=["plain", "posed"])
def test_edges_against_the_restatement(transforms):
    points, means = [], []
    for row in edge_rows(transforms):
        case, i, r, d, bound = row["case"], row["i"], row["ref"], row["data"], row["bound"]
        points.append(worst_point(row))
        means.append((row["mean_dev"], row["mean_bound"]))
        assert (row["dev"] <= bound).all(), (case, i, row["dev"].max(), np.max(bound))
        assert row["mean_dev"] <= row["mean_bound"], (case, i, row["mean_dev"], r.mean_d)
        if d["paired"]:
            assert np.array_equal(row["nn_j"], np.arange(case[0])), (case, i)
        else:
            sure = r.gap > 2 * bound
            assert (~sure).sum() <= 0.01 * len(sure), (case, i)
            assert np.array_equal(row["nn_j"][sure], r.nn_j[sure]), (case, i)
        # the share moves by 1 / n_src for every point whose distance lies within the bound of tau
        near = int((np.abs(np.sqrt(r.nn_d2) - float(d["tau"][i])) <= bound).sum())
        assert abs(round(row["inlier"] * case[0]) - r.count) <= near, (case, i, row["inlier"], r.inlier)
    print("posed" if transforms else "plain", "points", worst(points), "mean_d", worst(means))


# ---- 2. exact lattice ---------------------------------------------------------------------------------------------------
def lattice_data(transforms):
    rng = np.random.default_rng(77)
    I, n_src, n_dst = 2, TILE + 44, CHUNK + 76
    d = {"src": (rng.integers(-24, 25, (I, n_src, 3)) / 64).astype(np.float32),
         "dst": (rng.integers(-24, 25, (I, n_dst, 3)) / 64).astype(np.float32), "paired": False,
         "tau": np.array([3 / 64, 2 / 64], np.float32)}
    d["dst"][:, 500:600] = d["dst"][:, 0:100]                    # duplicates inside a chunk ...
    d["dst"][:, CHUNK + 10:CHUNK + 60] = d["dst"][:, 100:150]    # ... and across two
    d["src"][:, :30] = d["dst"][:, 510:540]                      # some src points on duplicated dst points: d = 0
    for k in ("src_pose", "src_scale", "dst_pose", "dst_scale"):
        d[k] = None
    if transforms:   # signed permutations, lattice translations and power-of-two scales: still exact
        P = np.array([[[0, -1, 0, 1.5], [0, 0, 1, -0.25], [-1, 0, 0, 0.75]], [[0, 0, 1, -2], [1, 0, 0, 0.5], [0, 1, 0, 1]]], np.float32)
        d["src_pose"] = d["dst_pose"] = P
        d["src_scale"] = d["dst_scale"] = np.array([[2, 1, 0.5], [0.5, 2, 1]], np.float32)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("transforms", [False, True], ids=["plain", "posed"])
def test_exact_lattice(transforms):
    d = lattice_data(transforms)
    refs = edge_reference(d)
    got = _run(d)
    for i, r in enumerate(refs):
        m = r.nn_d2 * 4096 * 4                                               # a scale of 1/2 gives quarters of 1/64^2
        assert np.array_equal(m, np.round(m)) and m.max() < 2 ** 24          # exact in fp32 as claimed
        t2 = float(d["tau"][i]) ** 2
        assert (r.nn_d2 == t2).any() and (r.nn_d2 == 0).any(), "the seed must put a pair on the threshold"
        assert np.array_equal(got.nn_d2[i].cpu().numpy().astype(np.float64), r.nn_d2), i
        assert np.array_equal(got.nn_j[i].cpu().numpy(), r.nn_j), i
        assert got.inlier[i].item() == float(np.float32(r.count / len(r.nn_d2))), (i, got.inlier[i].item(), r.count)
        # duplicated dst points: the lowest index won
        assert (r.nn_d2[:30] == 0).all() and (r.nn_j[:30] < 100).all()
    # one rounding in mean_d: sqrt is correctly rounded per point, the sum is double
    want = np.array([np.sqrt(r.nn_d2).astype(np.float32).astype(np.float64).mean() for r in refs])
    assert np.array_equal(got.mean_d.cpu().numpy(), want.astype(np.float32))


# ---- 3. batch independence ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["nearest", "paired"])
def test_batch_independence(paired):
    n_src = TILE + 44
    d = edge_data((n_src, n_src if paired else CHUNK + 76, 3, paired), True)
    whole = _run(d)
    for i in range(3):
        one = {k: (v[i:i + 1] if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        alone = _run(one)
        for f in ("mean_d", "inlier", "nn_d2", "nn_j"):
            assert torch.equal(getattr(whole, f)[i:i + 1], getattr(alone, f)), (i, f)
    # one tau for all as a float, and no tau at all: the same distances
    same = dict(d, tau=np.full(3, 0.03, np.float32))
    from catre_amd import tracking

    args = [_dev(d[k]) for k in ("src", "dst", "src_pose", "src_scale", "dst_pose", "dst_scale")]
    flt = tracking.nn_stats(*args, paired=paired, tau=0.03)
    none = tracking.nn_stats(*args, paired=paired)
    assert torch.equal(flt.inlier, _run(same).inlier) and torch.equal(flt.mean_d, whole.mean_d)
    assert none.inlier is None and none.nn_d2 is None and torch.equal(none.mean_d, whole.mean_d)


# ---- 4. ADD and ADD-S against the reference's recorded values -------------------------------------------------------------
@pytest.mark.gpu
def test_add_and_adds_against_the_reference():
    from catre_amd import evaluation

    rows = list(add_rows())
    assert len(rows) >= 20 and {r["key"] for r in rows} == {"add", "adi"}
    for r in rows:
        assert r["dev"] <= r["bound"], r
    for key in ("add", "adi"):
        print(key, worst((r["dev"], r["bound"]) for r in rows if r["key"] == key))
    z = np.load(os.path.join(GOLDEN_DIR, "pose_error_add.npz"))
    # a batch, shared points, with scales: against the restatement
    g = {k: z[f"c7/{k}"] for k in ("R_est", "t_est", "R_gt", "t_gt", "pts")}
    est = np.concatenate((g["R_est"], g["t_est"].reshape(3, 1)), 1)
    gt = np.concatenate((g["R_gt"], g["t_gt"].reshape(3, 1)), 1)
    ests, gts = np.stack((est, gt, est)), np.stack((gt, gt, est))
    s_est, s_gt = np.array([[1, 1.25, 0.75]] * 3, np.float32), np.array([[1.5, 1, 1]] * 3, np.float32)
    got = evaluation.add_errors(_dev(ests), _dev(gts), _dev(g["pts"]), _dev(s_est), _dev(s_gt), symmetric=True).cpu().numpy()
    for i in range(3):
        r = REF.nn_stats_one(g["pts"], g["pts"], gts[i], s_gt[i], ests[i], s_est[i])
        assert abs(float(got[i]) - r.mean_d) <= 16 * U * 2 * 2.0, i


# ---- 5. gate -------------------------------------------------------------------------------------------------------------
def gate_inputs():
    I = 12
    rng = np.random.default_rng(5)
    pose_new, scale_new = rng.normal(size=(I, 3, 4)).astype(np.float32), rng.uniform(0.1, 0.3, (I, 3)).astype(np.float32)
    pose_prev, scale_prev = rng.normal(size=(I, 3, 4)).astype(np.float32), rng.uniform(0.1, 0.3, (I, 3)).astype(np.float32)
    below = np.nextafter(np.float32(0.25), np.float32(0))
    above = np.nextafter(np.float32(0.25), np.float32(1))
    #                  ok    empty low   at    above e+l   nanP  infS  nanI  all   e+nan l+nan
    counts = np.array([9,    0,    9,    9,    9,    0,    9,    9,    9,    0,    0,    9], np.int32)
    inlier = np.array([0.9,  0.9,  below, 0.25, above, 0.1, 0.9,  0.9,  np.nan, 0.1, 0.9,  0.1], np.float32)
    mean_d = np.array([0.01] * 9 + [np.inf, 0.01, np.nan], np.float32)
    pose_new[6, 1, 2] = np.nan
    scale_new[7, 0] = np.inf
    scale_new[10, 2] = np.nan           # EMPTY | NONFINITE: a fine inlier share, an empty crop, a NaN scale
    pose_new[11, 0, 3] = -np.inf        # LOW_FIT | NONFINITE: an infinite translation and a NaN mean_d
    want = [0, 1, 2, 0, 0, 3, 4, 4, 4, 7, 5, 6]   # every value a status can take
    return pose_new, scale_new, pose_prev, scale_prev, counts, inlier, mean_d, want


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [True, False], ids=["hold", "follow"])
def test_gate_equals_the_restatement(hold):
    from catre_amd import tracking

    pose_new, scale_new, pose_prev, scale_prev, counts, inlier, mean_d, want = gate_inputs()
    age = np.array([0, 2, 0, 5, 1, 0, 0, 3, 0, 0, 4, 1], np.int32)
    args = [_dev(a) for a in (pose_new, scale_new, pose_prev, scale_prev, counts, inlier, mean_d)]
    age_d = _dev(age)
    for call in range(3):                                            # the age over three calls
        p, s, st, age_d_new = tracking.track_gate(*args, age_d, min_inlier=0.25, hold=hold)
        rp, rs, rst, age = REF.gate(pose_new, scale_new, pose_prev, scale_prev, counts, inlier, mean_d, 0.25, hold, age)
        assert st.cpu().tolist() == rst.tolist() == want, call
        assert age_d_new.cpu().tolist() == age.tolist(), call
        assert age_d_new.data_ptr() != age_d.data_ptr()              # the input is not modified
        age_d = age_d_new
        # bit-equal, NaN included
        assert np.array_equal(p.cpu().numpy().view(np.int32), rp.view(np.int32)), call
        assert np.array_equal(s.cpu().numpy().view(np.int32), rs.view(np.int32)), call
    assert sorted(set(want)) == list(range(8))
    assert age.tolist() == [0, 5, 3, 0, 0, 3, 3, 6, 3, 3, 7, 4]
    for i in (6, 7, 8, 9, 10, 11):                                           # NONFINITE holds whatever `hold` says
        assert np.array_equal(p[i].cpu().numpy(), pose_prev[i]) and np.array_equal(s[i].cpu().numpy(), scale_prev[i])
    if not hold:                                                     # EMPTY / LOW_FIT alone follow the new estimate
        for i in (1, 2, 5):
            assert np.array_equal(p[i].cpu().numpy(), pose_new[i])


# ---- 6-8. the tracker ----------------------------------------------------------------------------------------------------
N_PTS, N_ITER, H, W, T = 64, 2, 48, 64, 3


@pytest.fixture(scope="module")
def rig():
    from catre_amd import synth
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    cfg = default_cfg(num_pcl=N_PTS, num_kps=N_PTS, n_iter=N_ITER, device="cuda:0")
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.cuda() for k, v in sd.items()}, strict=True)
    model.eval()
    scene = synth.make_depth_scene(H=H, W=W, n_inst=2, seed=3)
    inputs = synth.make_inputs(2, N_PTS, N_PTS, seed=9)
    depth = torch.stack([torch.where(scene["depth"] > 0, scene["depth"] + 0.003 * t, scene["depth"]) for t in range(T)])
    # every other column of the blobs only: the masked crops and the mask-free ball crop see different pixels
    masks = scene["masks"] & (torch.arange(W) % 2 == 0)[None, None, :]
    labels = torch.zeros(H, W, dtype=torch.uint8)
    for i in range(2):
        labels[masks[i]] = i + 1
    return dict(model=model, kps=inputs["obj_kps"].cuda(), mean_scales=inputs["obj_mean_scales"].cuda(), K=scene["K"],
                depth=depth.cuda(), masks=masks.cuda(), labels=labels.cuda(), label_of=[1, 2],
                pose0=scene["poses"].cuda(), scale0=scene["scales"].cuda())


def _tracker(rig, **kw):
    from catre_amd import tracking

    tr = tracking.Tracker(rig["model"], rig["kps"], rig["K"], mean_scales=rig["mean_scales"], seed=11, **kw)
    return tr.reset(rig["pose0"], rig["scale0"])


def _eager(rig, pix_kw, seed=11, tau_rel=0.1, min_inlier=0.0, hold=True):
    """The composition written out: sample_frames -> model.refine -> fit_score -> gate, state carried by hand."""
    from catre_amd import pcl_prep, tracking

    pose, scale = rig["pose0"].clone(), rig["scale0"].clone()
    age = torch.zeros(2, dtype=torch.int32, device="cuda")
    Kd = rig["K"].cuda().expand(2, 3, 3).contiguous()
    steps = []
    for t in range(T):
        pcl, _, counts = pcl_prep.sample_frames(rig["depth"][t:t + 1], rig["K"], [0, 0], pose, scale, ratio=0.5,
                                                num_points=N_PTS, use_ball=True, sample="device", seed=seed + t,
                                                return_pixels=True, **pix_kw)
        out = rig["model"].refine({"pcl": pcl, "obj_kps": rig["kps"], "obj_pose_est": pose, "obj_scale_est": scale, "K": Kd,
                                   "obj_mean_scales": rig["mean_scales"]}, n_iter=N_ITER)
        score = tracking.fit_score(pcl, rig["kps"], out[f"pose_{N_ITER}"], out[f"scale_{N_ITER}"], tau_rel)
        pose, scale, status, age = tracking.track_gate(out[f"pose_{N_ITER}"], out[f"scale_{N_ITER}"], pose, scale, counts,
                                                       score.inlier_obs, score.d_obs, age, min_inlier, hold)
        steps.append(dict(pose=pose, scale=scale, pose_iters=torch.stack([out[f"pose_{i}"] for i in range(N_ITER + 1)]),
                          score=score, status=status, age=age, pcl=pcl))
    return steps


def _same_step(a, b):
    for k in ("pose", "scale", "pose_iters", "status", "age", "pcl"):
        assert torch.equal(a[k], b[k]), k
    for f in ("d_obs", "inlier_obs", "d_prior"):
        assert torch.equal(getattr(a["score"], f), getattr(b["score"], f)), f


@pytest.mark.gpu
@pytest.mark.parametrize("pixels", ["labels", "masks", "ball"])
def test_tracker_equals_the_eager_composition(rig, pixels):
    zero = torch.zeros(1, H, W, dtype=torch.uint8, device="cuda")
    step_kw = {"labels": dict(labels=rig["labels"], label_of=rig["label_of"]), "masks": dict(masks=rig["masks"]), "ball": {}}[pixels]
    eager_kw = {"labels": dict(labels=rig["labels"][None], label_of=rig["label_of"]), "masks": dict(masks=rig["masks"]),
                "ball": dict(labels=zero, label_of=[0, 0])}[pixels]
    want = _eager(rig, eager_kw)
    tr = _tracker(rig)
    got = [tr.step(rig["depth"][t], **step_kw) for t in range(T)]
    for t in range(T):
        _same_step(got[t], want[t])
        print(pixels, t, "status", got[t]["status"].tolist(), "d_obs", got[t]["score"].d_obs.tolist(),
              "inlier", got[t]["score"].inlier_obs.tolist())
    assert torch.isfinite(got[0]["pose"]).all() and (got[0]["pcl"] != 0).any()
    # track() is the same loop, stacked
    seq = _tracker(rig).track(rig["depth"], **({"masks": rig["masks"][None].expand(T, 2, H, W)} if pixels == "masks" else
                                               {"labels": rig["labels"][None].expand(T, H, W), "label_of": rig["label_of"]}
                                               if pixels == "labels" else {}))
    assert tuple(seq["pose"].shape) == (T, 2, 3, 4) and tuple(seq["score"].d_obs.shape) == (T, 2)
    for t in range(T):
        assert torch.equal(seq["pose"][t], got[t]["pose"]) and torch.equal(seq["pcl"][t], got[t]["pcl"])
    if pixels == "ball":   # the mask-free run is the run given an all-zero label image
        tr = _tracker(rig)
        for t in range(T):
            _same_step(tr.step(rig["depth"][t], labels=zero[0], label_of=[0, 0]), got[t])
        masked = _tracker(rig).step(rig["depth"][0], masks=rig["masks"])
        assert not torch.equal(masked["pcl"], got[0]["pcl"])          # and not the masked one


@pytest.mark.gpu
def test_step_reads_nothing_back(rig):
    from catre_amd import pcl_prep, tracking

    tr = _tracker(rig)
    tr.step(rig["depth"][0])                                         # packs the model's weights once
    torch.cuda.synchronize()
    grown = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in (1, 2, 0):
            before = (pcl_prep.abi_call_count(), tracking.abi_call_count())
            tr.step(rig["depth"][t])
            grown.append((pcl_prep.abi_call_count() - before[0], tracking.abi_call_count() - before[1]))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert grown[0] == grown[1] == grown[2] and grown[0][0] > 0 and grown[0][1] == 5, grown


@pytest.mark.gpu
def test_lost_and_recovered(rig):
    from catre_amd import pcl_prep, tracking

    tr = _tracker(rig)
    first = tr.step(rig["depth"][0])
    assert first["status"].tolist() == [0, 0] and first["age"].tolist() == [0, 0]
    lost = tr.step(torch.zeros(H, W, device="cuda"))
    assert all(s & tracking.EMPTY for s in lost["status"].tolist()), lost["status"].tolist()
    assert lost["age"].tolist() == [1, 1]
    assert torch.equal(lost["pose"], first["pose"]) and torch.equal(lost["scale"], first["scale"])   # held bit for bit
    back = tr.step(rig["depth"][2])
    assert back["status"].tolist() == [0, 0] and back["age"].tolist() == [0, 0]
    # its crop was centred on the held pose (frame counter 2: seed 11 + 2)
    zero = torch.zeros(1, H, W, dtype=torch.uint8, device="cuda")
    pcl = pcl_prep.sample_frames(rig["depth"][2:3], rig["K"], [0, 0], first["pose"], first["scale"], labels=zero,
                                 label_of=[0, 0], ratio=0.5, num_points=N_PTS, use_ball=True, sample="device", seed=13)
    assert torch.equal(back["pcl"], pcl)
    # without hold a lost frame follows the refined pose, unless it is not finite
    tr = _tracker(rig, hold_on_lost=False)
    first = tr.step(rig["depth"][0])
    lost = tr.step(torch.zeros(H, W, device="cuda"))
    for i, st in enumerate(lost["status"].tolist()):
        assert st & tracking.EMPTY
        assert torch.equal(lost["pose"][i], first["pose"][i] if st & tracking.NONFINITE else lost["pose_iters"][-1][i])


@pytest.mark.gpu
def test_low_fit_holds_the_track_end_to_end(rig):
    """min_inlier > 0 through ``Tracker`` itself: an object whose score falls short is flagged LOW_FIT, ages, and keeps the
    pose it had; one that passes is carried on.  The untrained weights give both kinds on this scene; the threshold sits
    between their inlier shares, taken from a first run."""
    from catre_amd import tracking

    probe = _tracker(rig).step(rig["depth"][0])
    inl = probe["score"].inlier_obs.tolist()
    assert probe["status"].tolist() == [0, 0] and abs(inl[0] - inl[1]) > 0.1, inl
    thr = 0.5 * (inl[0] + inl[1])
    low, high = (0, 1) if inl[0] < inl[1] else (1, 0)
    tr = _tracker(rig, min_inlier=thr)
    a = tr.step(rig["depth"][0])
    assert a["status"].tolist()[low] == tracking.LOW_FIT and a["status"].tolist()[high] == 0
    assert a["age"].tolist()[low] == 1 and a["age"].tolist()[high] == 0
    assert torch.equal(a["pose"][low], rig["pose0"][low]) and torch.equal(a["scale"][low], rig["scale0"][low])      # held
    assert torch.equal(a["pose"][high], a["pose_iters"][-1][high]) and torch.equal(a["pose"][high], probe["pose"][high])
    b = tr.step(rig["depth"][1])
    st = b["status"].tolist()
    assert b["age"].tolist()[low] == (2 if st[low] else 0)
    if st[low]:   # still lost: cropped around the held pose again, which is still carried
        assert torch.equal(b["pose"][low], rig["pose0"][low])
    # without hold the same frame follows the refined pose and still reports the low fit
    f = _tracker(rig, min_inlier=thr, hold_on_lost=False).step(rig["depth"][0])
    assert f["status"].tolist() == a["status"].tolist() and f["age"].tolist() == a["age"].tolist()
    assert torch.equal(f["pose"], probe["pose"]) and torch.equal(f["scale"], probe["scale"])
