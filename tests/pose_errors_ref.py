"""fp64 numpy restatement of the BOP pose errors (``catre_amd/pose_errors.py``, ``csrc/catre_bop.h``): the symmetry sets of
``lib/pysixd/misc.py:220-282``, ``mssd`` / ``mspd`` / ``proj_sym`` of ``lib/pysixd/pose_error.py:131-217`` per symmetry, and
``vsd`` (:22-128) after its renders in the reference's mixed precisions.  ``tests/test_pose_errors_host.py`` pins it to the
reference's own numbers (``tests/golden/pose_error_bop.npz``); the GPU tests compare the device against it.

The bounds of the point errors are computed here per (point, symmetry) from the arithmetic ``catre_bop.h`` spells out
(u = 2^-24; the derivation stands in ``tests/test_pose_errors.py``)."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
SAFE = 1.001          # second-order terms of the first-order bounds (relative size e / z, u: below 1e-5)

SymRef = namedtuple("SymRef", "err best e3 e2 p2 b3 b2 bp gap bound")   # err, best, gap, bound: [3] = mssd, mspd, proj
VsdRef = namedtuple("VsdRef", "errors counts vis_gt vis_est inside dist_test dist_gt dist_est")


# ---- symmetry sets ------------------------------------------------------------------------------------------------------
def rotation(angle, axis):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _turns(axis, offset, step):
    count = int(np.ceil(np.pi / step))
    off = np.asarray(offset, np.float64).reshape(3)
    out = []
    for k in range(1, count):
        R = rotation(k * 2.0 * np.pi / count, axis)
        out.append(np.hstack([R, (off - R @ off).reshape(3, 1)]))
    return out


def axis_symmetry_transforms(axis, step):
    return np.stack(_turns(axis, np.zeros(3), step))


def symmetry_transforms(model_info, step):
    disc = [np.hstack([np.eye(3), np.zeros((3, 1))])]
    for sym in model_info.get("symmetries_discrete", ()):
        disc.append(np.reshape(np.asarray(sym, np.float64), (4, 4))[:3])
    cont = [t for sym in model_info.get("symmetries_continuous", ()) for t in _turns(sym["axis"], sym["offset"], step)]
    if not cont:
        return np.stack(disc)
    return np.stack([np.hstack([c[:, :3] @ d[:, :3], (c[:, :3] @ d[:, 3] + c[:, 3]).reshape(3, 1)]) for d in disc for c in cont])


# ---- MSSD, MSPD, proj_sym -----------------------------------------------------------------------------------------------------
def compose(pose, scale=None, sym=None):
    """[R | t], scale, [R_s | t_s] -> A [3,4] with A p~ = R (s * (R_s p + t_s)) + t"""
    pose = np.asarray(pose, np.float64)
    L = pose[:, :3] * (np.ones(3) if scale is None else np.asarray(scale, np.float64))[None, :]
    if sym is None:
        return np.hstack([L, pose[:, 3:]])
    sym = np.asarray(sym, np.float64)
    return np.hstack([L @ sym[:, :3], (L @ sym[:, 3] + pose[:, 3]).reshape(3, 1)])


def _posed(A, pts):
    """-> x [n,3], e_x [n,3]: the posed points and the bound on each fp32 coordinate"""
    x = pts @ A[:, :3].T + A[:, 3]
    a = np.abs(pts) @ np.abs(A[:, :3]).T
    return x, U * (4 * a + 4 * np.abs(A[:, 3]))


def _projected(x, e, K):
    """-> uv [n,2], e_uv [n,2]"""
    f, c = np.array([K[0, 0], K[1, 1]], np.float64), np.array([K[0, 2], K[1, 2]], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = f * x[:, :2] / x[:, 2:3]
        uv = a + c
        e_uv = (f * e[:, :2] + np.abs(a) * e[:, 2:3]) / np.abs(x[:, 2:3]) + 2 * U * np.abs(a) + U * np.abs(uv)
    return uv, e_uv


def sym_errors(pose_est, pose_gt, pts, K, syms, scale_est=None, scale_gt=None, f32_roots=False):
    """One instance: pose_est, pose_gt [3,4], pts [n,3], K [3,3], syms [S,3,4] (fp32 values) -> ``SymRef``.
    e3, e2, p2 [S]: the per-symmetry errors; b3, b2, bp [S]: the bounds on the device's deviation from them; err / best [3]: the
    minima and the lowest index that reaches each; gap [3]: runner-up minus winner (inf for one symmetry); bound [3]: the
    largest bound of a symmetry (what a minimum over the set may move by).  ``f32_roots``: p2 as the mean of the fp32-rounded roots (the device's value where every squared
    distance is exact)."""
    pts, K = np.asarray(pts, np.float64), np.asarray(K, np.float64)
    xe, ee = _posed(compose(pose_est, scale_est), pts)
    ue, eue = _projected(xe, ee, K)
    S = len(syms)
    e3, e2, p2, b3, b2, bp = (np.zeros(S) for _ in range(6))
    for s in range(S):
        xg, eg = _posed(compose(pose_gt, scale_gt, syms[s]), pts)
        ug, eug = _projected(xg, eg, K)
        d3 = np.sqrt(((xe - xg) ** 2).sum(1))
        d2sq = ((ue - ug) ** 2).sum(1)
        d2 = np.sqrt(d2sq)
        roots = np.sqrt(d2sq.astype(np.float32)).astype(np.float64) if f32_roots else d2
        e3[s], e2[s], p2[s] = d3.max(), d2.max(), roots.mean()
        n3 = SAFE * (np.sqrt(((ee + eg) ** 2).sum(1)) + 4 * U * d3)
        n2 = SAFE * (np.sqrt(((eue + eug) ** 2).sum(1)) + 3 * U * d2)
        b3[s], b2[s], bp[s] = n3.max(), n2.max(), n2.mean() + U * p2[s]
    tabs, bnds = (e3, e2, p2), (b3, b2, bp)
    best = np.array([int(np.argmin(t)) for t in tabs])
    err = np.array([t[b] for t, b in zip(tabs, best)])
    gap = np.array([np.partition(t, 1)[1] - t.min() if S > 1 else np.inf for t in tabs])
    bound = np.array([np.max(b) for b in bnds])                             # any symmetry may be the device's winner
    return SymRef(err, best, e3, e2, p2, b3, b2, bp, gap, bound)


# ---- VSD ------------------------------------------------------------------------------------------------------------------------
def dist_image(depth, K, u0=0, v0=0):
    """``misc.depth_im_to_dist_im_fast`` for a window whose top-left pixel is (u0, v0) of the image K belongs to"""
    K = np.asarray(K, np.float64)
    h, w = depth.shape
    xs, ys = np.meshgrid(u0 + np.arange(w), v0 + np.arange(h))
    pre_x = (xs - K[0, 2]) / np.float64(K[0, 0])
    pre_y = (ys - K[1, 2]) / np.float64(K[1, 1])
    return np.sqrt(np.multiply(pre_x, depth) ** 2 + np.multiply(pre_y, depth) ** 2 + depth.astype(np.float64) ** 2)


def visib_mask(d_test, d_model, delta, mode):
    diff = d_model.astype(np.float32) - d_test.astype(np.float32)
    near = diff <= np.float32(delta)
    if mode == "bop18":
        return (d_test > 0) & (d_model > 0) & near
    assert mode == "bop19", mode
    return (near | (d_test == 0)) & (d_model > 0)


def vsd(depth_est, depth_gt, depth_test, K, delta, taus, diameter=None, origin=(0, 0), visib_mode="bop19"):
    """depth_est, depth_gt [h,w], depth_test [H,W] fp32 -> ``VsdRef``; the window's top-left pixel is ``origin`` = (u0, v0) of
    the frame, window pixels outside the frame are ignored."""
    h, w = depth_est.shape
    H, W = depth_test.shape
    u0, v0 = int(origin[0]), int(origin[1])
    xs, ys = np.meshgrid(u0 + np.arange(w), v0 + np.arange(h))
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    test = np.zeros((h, w), np.float32)
    test[inside] = depth_test[ys[inside], xs[inside]]
    dt, dg, de = (dist_image(np.asarray(d, np.float32), K, u0, v0) for d in (test, depth_gt, depth_est))
    vis_gt = visib_mask(dt, dg, delta, visib_mode) & inside
    vis_est = (visib_mask(dt, de, delta, visib_mode) | (vis_gt & (de > 0))) & inside
    inter, union = vis_gt & vis_est, vis_gt | vis_est
    dists = np.abs(dg[inter] - de[inter])
    if diameter is not None:
        dists = dists / np.float64(diameter)
    counts = np.array([union.sum(), inter.sum()] + [(dists >= np.float64(t)).sum() for t in taus], np.int64)
    if counts[0] == 0:
        errors = np.ones(len(taus))
    else:
        errors = np.array([(c + counts[0] - counts[1]) / float(counts[0]) for c in counts[2:]], np.float64)
    return VsdRef(errors, counts, vis_gt, vis_est, inside, dt, dg, de)
