"""fp64 numpy restatement of trimmed ICP (``csrc/catre_icp.h``, contract in ``include/catre_hip.h``), written from the
rules, not from the kernel: what ``tests/test_icp.py`` compares the device with.  The reference project has no ICP to record
values from; ``tests/test_icp_host.py`` pins the selection rule to a plain sort and the loop to exact recovery.

One step, given every observed point's squared distance ``d2`` to and index ``nn_j`` of its nearest posed prior point:
  candidates  rows k < n with 0 <= d2 <= tau^2 (tau^2: ONE fp32 product; no tau: every finite d2) and 0 <= nn_j < n_dst;
  kept        the m = ceil(float32(trim) * c) candidates smallest under (d2, k);
  fit         Umeyama in float64 of source = R (s * kps[nn_j]) + t onto target = pcl over the kept rows;
  update      R' = dR R, t' = sigma dR t + dt, s' = sigma s, rounded once to ``dtype``;
  status      FEW (m < 3) | DEGENERATE (sigma_2 <= 1e-12 sigma_1) | NONFINITE, sticky; any bit: pose and scale pass through."""
from collections import namedtuple

import numpy as np

from tests import track_ref

FEW, DEGENERATE, NONFINITE = 1, 2, 4

Step = namedtuple("Step", "pose scale rmse kept mask status sv_ratio")
Result = namedtuple("Result", "pose scale rmse kept status sv_ratio")


def select(d2, nn_j=None, n=None, n_dst=None, tau=None, trim=1.0):
    """-> (mask [len(d2)] bool, c, m).  d2 is taken as it is (any float dtype)."""
    d2 = np.asarray(d2)
    N = len(d2)
    k = np.arange(N)
    with np.errstate(invalid="ignore"):
        cand = (k < (N if n is None else n)) & np.isfinite(d2) & (d2 >= 0)
        if tau is not None:
            cand &= d2 <= np.float32(tau) * np.float32(tau)            # one fp32 product, equality inside
    if nn_j is not None and n_dst is not None:
        cand &= (np.asarray(nn_j) >= 0) & (np.asarray(nn_j) < n_dst)
    rows = k[cand]
    c = len(rows)
    m = min(c, int(np.ceil(float(np.float32(trim)) * c)))
    order = np.argsort(d2[rows] + 0.0, kind="stable")                   # stable: equal values stay in index order
    mask = np.zeros(N, bool)
    mask[rows[order[:m]]] = True
    return mask, c, m


def umeyama(S, T):
    """S, T [m,3] float64 -> (sigma, R, mean of S, mean of T, singular values of the covariance): T ~ sigma R S + t with
    t = mu_T - sigma R mu_S, left to the caller, who may hold sigma at 1 (``preprocess/pose_data.py:56-87``)."""
    ms, mt = S.mean(0), T.mean(0)
    Sc, Tc = S - ms, T - mt
    C = Tc.T @ Sc / len(S)
    U, D, Vt = np.linalg.svd(C)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D = D.copy()
        D[2] = -D[2]
        U = U.copy()
        U[:, 2] = -U[:, 2]
    R = U @ Vt
    var = (Sc ** 2).sum() / len(S)
    sigma = D.sum() / var
    return sigma, R, ms, mt, np.abs(D)


def step(pcl, kps, pose, scale, d2, nn_j, n=None, tau=None, trim=0.7, with_scale=False, status=0, dtype=np.float32):
    """One instance.  pcl [N,3], kps [M,3], pose [3,4], scale [3]; -> ``Step`` (pose / scale in ``dtype``; rmse float64
    before its rounding; sv_ratio = sigma_2 / sigma_1 of the kept covariance, NaN when nothing was fitted)."""
    pose_in, scale_in = np.asarray(pose), np.asarray(scale)
    pose64, scale64 = pose_in.astype(np.float64), scale_in.astype(np.float64)
    mask, c, m = select(d2, nn_j, n, len(kps), tau, trim)
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = float(np.sqrt(np.asarray(d2, np.float64)[mask].sum() / m)) if m else float("nan")
    st = int(status)
    if m < 3:
        st |= FEW
    if not (np.isfinite(pose64).all() and np.isfinite(scale64).all()):
        st |= NONFINITE
    ratio = float("nan")
    new_pose, new_scale = pose_in, scale_in
    if m >= 3:
        S = track_ref.apply_pose(np.asarray(kps)[np.asarray(nn_j)[mask]], pose64, scale64)
        T = np.asarray(pcl, np.float64)[mask]
        with np.errstate(all="ignore"):
            try:
                sigma, dR, ms, mt, D = umeyama(S, T)
            except np.linalg.LinAlgError:                               # a NaN covariance
                sigma, dR, ms, mt, D = np.nan, np.full((3, 3), np.nan), S.mean(0), T.mean(0), np.full(3, np.nan)
            if D[1] <= 1e-12 * D[0]:
                st |= DEGENERATE
            ratio = float(D[1] / D[0]) if D[0] > 0 else float("nan")
            if not with_scale:
                sigma = 1.0
            dt = mt - sigma * dR @ ms
            if not (np.isfinite(sigma) and np.isfinite(dR).all() and np.isfinite(dt).all()):
                st |= NONFINITE
            R2 = dR @ pose64[:, :3]
            t2 = sigma * dR @ pose64[:, 3] + dt
            new_pose = np.concatenate((R2, t2[:, None]), 1).astype(dtype)
            new_scale = (sigma * scale64).astype(dtype)
    if st:
        new_pose, new_scale = pose_in, scale_in                         # bit for bit
    return Step(new_pose, new_scale, rmse, m, mask, st, ratio)


def nearest(pcl, kps, pose, scale, dtype=np.float32, fast=False):
    """-> (d2 [N] in ``dtype``, nn_j [N]): float64 distances of coordinate differences, the lowest index on a tie.
    ``fast``: the index from the centred matrix form (|p|^2 + |q|^2 - 2 p.q through BLAS), the distance of that pair by
    differences - for long loops where a near-tie may go either way."""
    q = track_ref.apply_pose(kps, pose, scale)
    p = np.asarray(pcl, np.float64)
    if not fast:
        r = track_ref.nn_stats_one(p, q)
        return r.nn_d2.astype(dtype), r.nn_j
    with np.errstate(all="ignore"):
        mid = np.nanmean(q, 0)
        pc, qc = p - mid, q - mid
        j = np.argmin((qc ** 2).sum(1)[None, :] - 2.0 * pc @ qc.T, axis=1)
        diff = p - q[j]
        return ((diff[:, 0] ** 2 + diff[:, 1] ** 2) + diff[:, 2] ** 2).astype(dtype), j.astype(np.int32)


def icp(pcl, kps, pose, scale, n_iter, n=None, tau=None, trim=0.7, with_scale=False, dtype=np.float32, fast=False):
    """One instance: ``n_iter`` rounds of ``nearest`` + ``step`` and a final measurement -> ``Result`` (rmse, kept, sv_ratio:
    [n_iter + 1]).  ``dtype``: what pose, scale and d2 are rounded to every iteration (float32: as the device; float64: no
    rounding at all)."""
    pose, scale = np.asarray(pose, dtype), np.asarray(scale, dtype)
    rmse, kept, ratio, st = [], [], [], 0
    for it in range(n_iter + 1):
        d2, j = nearest(pcl, kps, pose, scale, dtype, fast)
        if it < n_iter:
            s = step(pcl, kps, pose, scale, d2, j, n, tau, trim, with_scale, st, dtype)
            pose, scale, st = s.pose, s.scale, s.status
            rmse.append(s.rmse), kept.append(s.kept), ratio.append(s.sv_ratio)
        else:
            mask, _, m = select(d2, j, n, len(kps), tau, trim)
            with np.errstate(invalid="ignore", divide="ignore"):
                rmse.append(float(np.sqrt(d2.astype(np.float64)[mask].sum() / m)) if m else float("nan"))
            kept.append(m), ratio.append(float("nan"))
    return Result(pose, scale, np.array(rmse), np.array(kept), st, np.array(ratio))


def rot_err_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
