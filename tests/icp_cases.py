"""Inputs of the trimmed-ICP tests (``tests/test_icp_host.py``, ``tests/test_icp.py``): seeded, built here, nothing read
from outside the repository.  The convergence reference is computed once per process and shared."""
import functools

import numpy as np

from tests import icp_ref as REF

N_DST = 1024 + 76                      # one whole NN_CHUNK of csrc/catre_track.h and a part of the next
STEP_N_SRC = (3, 4, 255, 256, 257, 1024 + 44)
CONV_SEEDS, CONV_BOXES, CONV_ITERS, PATCH = (0, 1, 2), (1, 3, 5, 7), 30, 256


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def box_prior(M, rng):
    """points on the surface of a 1.0 x 0.6 x 0.9 box: no rotational symmetry a 10 degree start could fall into"""
    p = rng.uniform(-0.5, 0.5, (M, 3))
    p[np.arange(M), rng.integers(0, 3, M)] = rng.choice([-0.5, 0.5], M)
    return p * np.array([1.0, 0.6, 0.9])


# ---- one step -------------------------------------------------------------------------------------------------------------
def step_data(n_src, I=4, seed=0):
    """I instances: an observed cloud sampled from the posed prior with 2 mm noise, every fifth point clutter up to 6 cm
    away, seen from a pose 4 degrees / 4 mm off.  counts: ragged, with 0, 1, 2 and n_src among them when I == 4."""
    rng = np.random.default_rng([411, n_src, I, seed])
    kps = np.stack([box_prior(N_DST, rng) for _ in range(I)]).astype(np.float32)
    scale = rng.uniform(0.1, 0.25, (I, 3)).astype(np.float32)
    pose_gt, pose, pcl = np.zeros((I, 3, 4)), np.zeros((I, 3, 4), np.float32), np.zeros((I, n_src, 3), np.float32)
    for i in range(I):
        R = rot(rng.normal(size=3), rng.uniform(0, 180))
        t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.6, 1.4)])
        pose_gt[i] = np.concatenate((R, t[:, None]), 1)
        x = kps[i][rng.integers(0, N_DST, n_src)].astype(np.float64) * scale[i]
        p = x @ R.T + t + rng.normal(0, 0.002, (n_src, 3))
        clutter = np.arange(n_src) % 5 == 4
        p[clutter] += rng.uniform(-0.06, 0.06, (int(clutter.sum()), 3))
        pcl[i] = p
        pose[i] = np.concatenate((rot(rng.normal(size=3), 4.0) @ R, (t + rng.normal(0, 0.004 / np.sqrt(3), 3))[:, None]), 1)
    counts = np.array([n_src, 0, 1, 2][:I], np.int32)
    tau = np.full(I, 0.02, np.float32)
    return dict(pcl=pcl, kps=kps, pose=pose, scale=scale, counts=counts, tau=tau, pose_gt=pose_gt)


def full_counts(n_src, I=4):
    """a second ragged set: every instance with enough rows for a fit (where n_src allows)"""
    return np.array([n_src, max(n_src - 1, 0), (n_src + 1) // 2, min(n_src, 3)][:I], np.int32)


# ---- ties -------------------------------------------------------------------------------------------------------------------
def lattice_data():
    """Dyadic coordinates (multiples of 1/64, identity pose, unit scale): every d2 is exact in fp32 and many are equal."""
    rng = np.random.default_rng(78)
    I, n_src = 2, 256 + 44
    pcl = (rng.integers(-24, 25, (I, n_src, 3)) / 64).astype(np.float32)
    kps = (rng.integers(-24, 25, (I, N_DST, 3)) / 64 + np.array([1 / 128, 0, 0])).astype(np.float32)
    pose = np.tile(np.eye(3, 4, dtype=np.float32), (I, 1, 1))
    scale = np.ones((I, 3), np.float32)
    return dict(pcl=pcl, kps=kps, pose=pose, scale=scale, counts=np.array([n_src, n_src - 7], np.int32))


# ---- convergence ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def convergence_inputs():
    """``synth.make_inputs(8, 1024, 1024, seed)``, seeds 0-2, the box instances 1, 3, 5, 7 (the cylinders are symmetric about
    y: no unique rotation).  Scale held at the ground truth; the first 256 observed points replaced by a plane patch 12 cm
    beside the object: ``gt_trans + (U(-0.15, 0.15), 0.12, U(-0.15, 0.15))`` from ``default_rng(seed)``, instance after
    instance.  -> list of dicts (fp32 arrays of one instance + the ground truth)."""
    from catre_amd import synth

    out = []
    for seed in CONV_SEEDS:
        d = {k: v.numpy() for k, v in synth.make_inputs(8, 1024, 1024, seed).items()}
        rng = np.random.default_rng(seed)
        for b in CONV_BOXES:
            pcl = d["pcl"][b].copy()
            xz = rng.uniform(-0.15, 0.15, (PATCH, 2))
            pcl[:PATCH] = (d["gt_trans"][b].astype(np.float64) + np.stack((xz[:, 0], np.full(PATCH, 0.12), xz[:, 1]), 1)).astype(np.float32)
            out.append(dict(seed=seed, b=b, pcl=pcl, kps=d["obj_kps"][b], pose=d["obj_pose_est"][b], scale=d["gt_scale"][b],
                            gt_rot=d["gt_rot"][b], gt_trans=d["gt_trans"][b]))
    return out


def pose_errors(pose, case):
    """-> (rotation error in degrees, translation error in metres) against the case's ground truth"""
    pose = np.asarray(pose, np.float64)
    return REF.rot_err_deg(pose[:, :3], case["gt_rot"]), float(np.linalg.norm(pose[:, 3] - case["gt_trans"].astype(np.float64)))


@functools.lru_cache(maxsize=None)
def convergence_reference():
    """The restatement on every convergence case, ``CONV_ITERS`` rigid iterations without tau, pose rounded to fp32 every
    iteration as on the device: -> list of dict(trim07 = Result, trim10 = Result, err07, err10)."""
    rows = []
    for c in convergence_inputs():
        r07 = REF.icp(c["pcl"], c["kps"], c["pose"], c["scale"], CONV_ITERS, trim=0.7, fast=True)
        r10 = REF.icp(c["pcl"], c["kps"], c["pose"], c["scale"], CONV_ITERS, trim=1.0, fast=True)
        rows.append(dict(trim07=r07, trim10=r10, err07=pose_errors(r07.pose, c), err10=pose_errors(r10.pose, c)))
    return rows


def dev(a, dtype=None):
    import torch

    return None if a is None else torch.as_tensor(a, dtype=dtype).cuda()


# ---- one step on the device against the restatement ---------------------------------------------------------------------------
STEP_TRIMS = (0.5, 0.7, 1.0)


def bound(ref):
    """|device - restatement| allowed on a value the device rounds once to fp32: the fp64 quantities agree to the 1e-12
    the alignment tests use (measured there: 1.2e-15), and one rounding to fp32 can then fall on either side."""
    return 2.0 ** -23 * np.abs(np.asarray(ref, np.float64)) + 1e-11


def device_nn(d):
    from catre_amd import tracking

    return tracking.nn_stats(dev(d["pcl"]), dev(d["kps"]), dst_pose=dev(d["pose"]), dst_scale=dev(d["scale"]), return_nn=True)


def step_rows(n_src):
    """Every configuration of one step at ``n_src`` on the device, fed the device's own neighbours, beside the restatement
    fed the same: yields dict(cfg, i, got = ICPStep on the host as numpy, ref = icp_ref.Step)."""
    from catre_amd import icp

    d = step_data(n_src)
    nn = device_nn(d)
    d2, nj = nn.nn_d2.cpu().numpy(), nn.nn_j.cpu().numpy()
    args = [dev(d[k]) for k in ("pcl", "kps", "pose", "scale")]
    for cname, counts in (("ragged", d["counts"]), ("full", full_counts(n_src)), ("none", None)):
        for tau in (None, d["tau"]):
            for trim in STEP_TRIMS:
                for with_scale in (False, True):
                    got = icp.icp_step(*args, nn, counts=dev(counts), tau=dev(tau), trim=trim, estimate_scale=with_scale,
                                       return_mask=True)
                    got = [t.cpu().numpy() for t in got]
                    for i in range(len(d["pcl"])):
                        ref = REF.step(d["pcl"][i], d["kps"][i], d["pose"][i], d["scale"][i], d2[i], nj[i],
                                       None if counts is None else int(counts[i]), None if tau is None else tau[i], trim, with_scale)
                        yield dict(cfg=(n_src, cname, tau is not None, trim, with_scale), i=i, got=[g[i] for g in got], ref=ref,
                                   pose_in=d["pose"][i], scale_in=d["scale"][i])


def step_ratio(row):
    """the largest |device - restatement| / bound over pose, scale and rmse of one row (0 where both are NaN alike)"""
    pose, scale, rmse = row["got"][0], row["got"][1], row["got"][2]
    ref = row["ref"]
    worst = 0.0
    for g, r in ((pose, ref.pose), (scale, ref.scale), (rmse, np.float64(ref.rmse))):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        with np.errstate(invalid="ignore"):
            q = np.where(np.isnan(g) & np.isnan(r), 0.0, np.abs(g - r) / bound(r))
        worst = float("inf") if np.isnan(q).any() else max(worst, float(q.max()))
    return worst
