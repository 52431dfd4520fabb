"""Inputs, bounds and measured deviations of the nearest-neighbour kernel's parity tests, shared by ``tests/test_track.py``
(which asserts on them), ``tests/test_track_host.py`` (the CPU-side precondition) and ``profiles/track_probe.py`` (which
records the worst of them).  The bounds are derived in the docstring of ``tests/test_track.py``."""
import json
import os

import numpy as np

from tests import track_ref as REF
from tests.util import GOLDEN_DIR

U = 2.0 ** -24
CHUNK, TILE = 1024, 256          # NN_CHUNK, NN_THREADS of csrc/catre_track.h
EDGE_SEED = 20260


def edge_cases():
    """(n_src, n_dst, I, paired)"""
    pairs = [(1, 1), (1, 257), (63, 65), (64, 64), (255, 256), (257, 1), (TILE + 1, CHUNK - 1), (TILE + 1, CHUNK), (TILE + 1, CHUNK + 1)]
    cases = [(a, b, I, False) for a, b in pairs for I in (1, 3)]
    cases += [(n, n, I, True) for n in (1, 64, TILE + 1) for I in (1, 3)]
    return cases


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _pose(rng, I, t=None):
    t = np.stack([rng.uniform(-0.3, 0.3, I), rng.uniform(-0.3, 0.3, I), rng.uniform(0.6, 1.4, I)], 1) if t is None else t
    R = np.stack([_rot(rng) for _ in range(I)])
    return np.concatenate((R, t[:, :, None]), 2).astype(np.float32)


def edge_data(case, transforms):
    n_src, n_dst, I, paired = case
    rng = np.random.default_rng([EDGE_SEED, n_src, n_dst, I, int(paired), int(transforms)])
    d = {"src": rng.uniform(-0.15, 0.15, (I, n_src, 3)).astype(np.float32),
         "dst": rng.uniform(-0.15, 0.15, (I, n_dst, 3)).astype(np.float32), "paired": paired,
         "tau": rng.uniform(0.01, 0.05, I).astype(np.float32)}
    for k in ("src_pose", "src_scale", "dst_pose", "dst_scale"):
        d[k] = None
    if transforms:   # two poses of one object, a few centimetres apart
        d["src_pose"] = _pose(rng, I)
        d["dst_pose"] = _pose(rng, I, d["src_pose"][:, :, 3].astype(np.float64) + rng.normal(0, 0.02, (I, 3)))
        d["src_scale"] = rng.uniform(0.5, 1.5, (I, 3)).astype(np.float32)
        d["dst_scale"] = rng.uniform(0.5, 1.5, (I, 3)).astype(np.float32)
    return d


def edge_reference(d):
    return REF.nn_stats(d["src"], d["dst"], d["src_pose"], d["src_scale"], d["dst_pose"], d["dst_scale"], d["paired"], d["tau"])


def distance_bound(d, i, r):
    """the bound on |d - d64| of instance i: per point without transforms, one number with"""
    if d["src_pose"] is None:
        return 8 * U * np.sqrt(r.nn_d2)
    p = REF.apply_pose(d["src"][i], d["src_pose"][i], d["src_scale"][i])
    q = REF.apply_pose(d["dst"][i], d["dst_pose"][i], d["dst_scale"][i])
    return 16 * U * (np.linalg.norm(p, axis=1).max() + np.linalg.norm(q, axis=1).max())


def dev(a, dtype=None):
    import torch

    return None if a is None else torch.as_tensor(a, dtype=dtype).cuda()


def run_nn(d, **kw):
    """``tracking.nn_stats`` on the device for a data dict of :func:`edge_data`'s form, with the per-point outputs"""
    from catre_amd import tracking

    return tracking.nn_stats(dev(d["src"]), dev(d["dst"]), dev(d["src_pose"]), dev(d["src_scale"]), dev(d["dst_pose"]),
                             dev(d["dst_scale"]), paired=d["paired"], tau=dev(d.get("tau")), return_nn=True, **kw)


def edge_rows(transforms):
    """Runs every edge case on the device; yields one dict per (case, instance): the restatement's result ``ref``, the
    distance bound, |d - d64| per point, the deviation and bound of mean_d, and the device's nn_j and inlier share."""
    for case in edge_cases():
        d = edge_data(case, transforms)
        got = run_nn(d)
        mean_d, inlier = got.mean_d.cpu().numpy().astype(np.float64), got.inlier.cpu().numpy()
        nn_d = np.sqrt(got.nn_d2.cpu().numpy().astype(np.float64))
        nn_j = got.nn_j.cpu().numpy()
        for i, r in enumerate(edge_reference(d)):
            bound = distance_bound(d, i, r)
            yield dict(case=case, i=i, data=d, ref=r, bound=bound, dev=np.abs(nn_d[i] - np.sqrt(r.nn_d2)),
                       mean_dev=abs(mean_d[i] - r.mean_d), mean_bound=bound if transforms else 8 * U * r.mean_d,
                       nn_j=nn_j[i], inlier=float(inlier[i]))


def add_rows():
    """``evaluation.add_errors`` on every case of ``tests/golden/pose_error_add.npz``; yields dict(j, key, got, want, dev,
    bound) for ADD (``key == "add"``) and ADD-S (``"adi"``)."""
    from catre_amd import evaluation

    z = np.load(os.path.join(GOLDEN_DIR, "pose_error_add.npz"))
    for j in range(len(json.loads(str(z["meta"]))["cases"])):
        g = {k: z[f"c{j}/{k}"] for k in ("R_est", "t_est", "R_gt", "t_gt", "pts")}
        est = np.concatenate((g["R_est"], g["t_est"].reshape(3, 1)), 1)[None]
        gt = np.concatenate((g["R_gt"], g["t_gt"].reshape(3, 1)), 1)[None]
        p, q = REF.apply_pose(g["pts"], gt[0]), REF.apply_pose(g["pts"], est[0])
        bound = 16 * U * (np.linalg.norm(p, axis=1).max() + np.linalg.norm(q, axis=1).max())
        for sym, key in ((False, "add"), (True, "adi")):
            got = evaluation.add_errors(dev(est), dev(gt), dev(g["pts"]), symmetric=sym)
            assert tuple(got.shape) == (1,)
            want = float(z[f"c{j}/{key}"])
            yield dict(j=j, key=key, got=float(got.item()), want=want, dev=abs(float(got.item()) - want), bound=bound)


def worst(pairs):
    """(deviation, bound) pairs -> the one with the largest deviation / bound"""
    out = {"worst_abs_dev": 0.0, "bound_there": None, "worst_ratio": 0.0}
    for d, b in pairs:
        ratio = d / b if b > 0 else (0.0 if d == 0 else float("inf"))
        if ratio >= out["worst_ratio"]:
            out = {"worst_abs_dev": float(d), "bound_there": float(b), "worst_ratio": float(ratio)}
    return out


def worst_point(row):
    """the (deviation, bound) of the point of an :func:`edge_rows` row that comes closest to its bound"""
    b = np.broadcast_to(row["bound"], row["dev"].shape)
    k = int(np.argmax(np.where(b > 0, row["dev"] / np.where(b > 0, b, 1), np.where(row["dev"] == 0, 0.0, np.inf))))
    return float(row["dev"][k]), float(b[k])
