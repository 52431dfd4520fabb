"""fp64 numpy restatement of ``catre_nn_stats`` and ``catre_track_gate`` (``csrc/catre_track.h``): what the GPU tests of
``tests/test_track.py`` compare with.  ``tests/test_track_host.py`` checks it against what the unmodified reference's
``lib/pysixd/pose_error.py`` (``add`` :256-271, ``adi`` :274-296) wrote into ``tests/golden/pose_error_add.npz``.

Inputs are taken as they are (fp32 values widened to float64); every operation is float64 except ``tau ** 2``, which is
the one fp32 product the kernel forms."""
from collections import namedtuple

import numpy as np

EMPTY, LOW_FIT, NONFINITE = 1, 2, 4

NNStats = namedtuple("NNStats", "mean_d inlier count nn_d2 nn_j gap")


def apply_pose(x, pose=None, scale=None):
    """x [n,3] -> R (s * x) + t (``lib/pysixd/misc.py:1014-1026``); None = identity."""
    x = np.asarray(x, np.float64)
    if scale is not None:
        x = x * np.asarray(scale, np.float64)[None, :]
    if pose is not None:
        pose = np.asarray(pose, np.float64)
        x = x @ pose[:3, :3].T + pose[:3, 3][None, :]
    return x


def nn_stats_one(src, dst, src_pose=None, src_scale=None, dst_pose=None, dst_scale=None, paired=False, tau=None):
    """One instance -> NNStats(mean_d, inlier share, inlier count, nn_d2 [n_src], nn_j [n_src], gap [n_src]); ``gap`` is the
    distance of the second-best neighbour minus the best one (inf with a single dst point or ``paired``)."""
    p = apply_pose(src, src_pose, src_scale)
    q = apply_pose(dst, dst_pose, dst_scale)
    if paired:
        if len(p) != len(q):
            raise ValueError("paired needs n_src == n_dst")
        d2 = ((p - q) ** 2).sum(1)
        j = np.arange(len(p))
        gap = np.full(len(p), np.inf)
    else:
        diff = p[:, None, :] - q[None, :, :]
        all_d2 = (diff[:, :, 0] ** 2 + diff[:, :, 1] ** 2) + diff[:, :, 2] ** 2
        j = np.argmin(all_d2, axis=1)                       # the first index of the minimum
        d2 = all_d2[np.arange(len(p)), j]
        if q.shape[0] > 1:
            rest = all_d2.copy()
            rest[np.arange(len(p)), j] = np.inf
            gap = np.sqrt(rest.min(axis=1)) - np.sqrt(d2)
        else:
            gap = np.full(len(p), np.inf)
    mean_d = float(np.sqrt(d2).mean())
    if tau is None:
        count, inlier = None, None
    else:
        t2 = float(np.float32(tau) * np.float32(tau))
        count = int((d2 <= t2).sum())
        inlier = count / len(p)
    return NNStats(mean_d, inlier, count, d2, j.astype(np.int32), gap)


def nn_stats(src, dst, src_pose=None, src_scale=None, dst_pose=None, dst_scale=None, paired=False, tau=None):
    """A batch [I,n,3] -> list of :func:`nn_stats_one` results."""
    pick = lambda a, i: None if a is None else a[i]
    return [nn_stats_one(src[i], dst[i], pick(src_pose, i), pick(src_scale, i), pick(dst_pose, i), pick(dst_scale, i), paired,
                         pick(tau, i)) for i in range(len(src))]


def add_error(R_est, t_est, R_gt, t_gt, pts, symmetric=False):
    """``pose_error.add`` / ``pose_error.adi``: src = pts under the ground truth, dst = pts under the estimate."""
    est = np.concatenate((np.asarray(R_est, np.float64), np.asarray(t_est, np.float64).reshape(3, 1)), 1)
    gt = np.concatenate((np.asarray(R_gt, np.float64), np.asarray(t_gt, np.float64).reshape(3, 1)), 1)
    return nn_stats_one(pts, pts, src_pose=gt, dst_pose=est, paired=not symmetric).mean_d


def gate(pose_new, scale_new, pose_prev, scale_prev, counts, inlier, mean_d, min_inlier, hold, age):
    """-> (pose_out, scale_out, status, age_out); the arrays keep their dtype (values are copied, never computed)."""
    I = len(counts)
    pose_out, scale_out = np.array(pose_prev, copy=True), np.array(scale_prev, copy=True)
    status, age_out = np.zeros(I, np.int32), np.array(age, dtype=np.int32, copy=True)
    min_inlier = np.float32(min_inlier)
    for i in range(I):
        st = 0
        if counts[i] == 0:
            st |= EMPTY
        if np.float32(inlier[i]) < min_inlier:
            st |= LOW_FIT
        if not (np.isfinite(pose_new[i]).all() and np.isfinite(scale_new[i]).all() and np.isfinite(inlier[i])
                and np.isfinite(mean_d[i])):
            st |= NONFINITE
        keep_prev = st != 0 and (hold or (st & NONFINITE))
        if not keep_prev:
            pose_out[i], scale_out[i] = pose_new[i], scale_new[i]
        status[i] = st
        age_out[i] = age_out[i] + 1 if st else 0
    return pose_out, scale_out, status, age_out
