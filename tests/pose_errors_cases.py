"""Inputs shared by ``tests/test_pose_errors_host.py`` (preconditions, on the CPU) and ``tests/test_pose_errors.py`` (the device):
seeded cases at the tiling edges of ``k_sym_err``, their restatement results (computed once), and the golden file."""
import functools
import json
import os

import numpy as np

from tests import pose_errors_ref as REF
from tests.util import GOLDEN_DIR

CHUNK, SYM_TILE = 512, 8                  # BOP_CHUNK, BOP_SYM_TILE of csrc/catre_bop.h
SET_SIZES = (1, 2, SYM_TILE - 1, SYM_TILE, SYM_TILE + 1, 314)
# name -> (points, scales, shared [n,3] points, K per instance); every case is a ragged batch of the six set sizes
EDGE_CASES = {"n1": (1, True, False, True), "n63": (63, False, True, False), "n64": (64, True, True, True),
              "n65": (65, False, False, True), "below_chunk": (CHUNK - 1, True, False, False),
              "chunk": (CHUNK, False, False, True), "above_chunk": (CHUNK + 1, True, True, True)}


def golden():
    return np.load(os.path.join(GOLDEN_DIR, "pose_error_bop.npz"), allow_pickle=False)


def golden_meta(g):
    return json.loads(str(g["meta"]))


@functools.lru_cache(maxsize=None)
def sym_set(S):
    """identity + the S - 1 turns by 2 pi / S about the y axis through (0.01, 0, -0.02) -> [S,3,4] fp32 values (float64)"""
    from catre_amd import pose_errors

    eye = np.hstack([np.eye(3), np.zeros((3, 1))])[None]
    if S == 1:
        return eye
    turns = pose_errors.symmetry_transforms({"symmetries_continuous": [{"axis": [0, 1, 0], "offset": [0.01, 0, -0.02]}]},
                                            np.pi / (S - 0.5))
    assert len(turns) == S - 1
    return np.concatenate([eye, turns]).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def edge_data(name):
    """a box-shaped object of about 0.2 m per instance in view of a ~600 px camera; the estimate is a few degrees and some
    millimetres off a non-identity member of the instance's set"""
    n, scales, shared, k_per = EDGE_CASES[name]
    rng = np.random.default_rng(sorted(EDGE_CASES).index(name) + 300)
    I = len(SET_SIZES)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    pts = rng.uniform(-1, 1, ((1 if shared else I), n, 3)) * rng.uniform(0.05, 0.12, 3)
    if n == 1:
        pts = pts * 0 + np.array([0.09, 0.03, -0.07]) * rng.uniform(0.8, 1.2, (pts.shape[0], 1, 3))     # off the axis
    d = dict(pts=f32(pts[0] if shared else pts), pose_est=np.zeros((I, 3, 4), np.float32), pose_gt=np.zeros((I, 3, 4), np.float32),
             scale_est=None, scale_gt=None, sets=[sym_set(S) for S in SET_SIZES], pick=[])
    if scales:
        s = rng.uniform(0.8, 1.25, (I, 3))
        s[:, 2] = s[:, 0]                                       # a turn about y then keeps the scaled object on itself
        d["scale_gt"], d["scale_est"] = f32(s), f32(s * rng.uniform(0.98, 1.02, (I, 3)))
    K = np.array([[[600 + 3 * i, 0, 320.5 - i], [0, 598 - 2 * i, 239.25 + i], [0, 0, 1]] for i in range(I)], np.float32)
    d["K"] = K if k_per else K[0]
    for i, S in enumerate(SET_SIZES):
        R_gt = REF.rotation(rng.uniform(0, np.pi), rng.normal(size=3))
        t_gt = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15), rng.uniform(0.6, 1.4)])
        pick = 0 if S == 1 else int(rng.integers(1, S))
        sym = d["sets"][i][pick]
        dR = REF.rotation(np.deg2rad(rng.uniform(2, 5)), rng.normal(size=3))
        sg = np.ones(3) if not scales else d["scale_gt"][i].astype(np.float64)
        d["pose_gt"][i] = f32(np.hstack([R_gt, t_gt.reshape(3, 1)]))
        d["pose_est"][i] = f32(np.hstack([R_gt @ sym[:, :3] @ dR, (R_gt @ (sg * sym[:, 3]) + t_gt + rng.normal(0, 0.004, 3)).reshape(3, 1)]))
        d["pick"].append(pick)
    return d


def instance(d, i):
    """the arguments of ``REF.sym_errors`` for instance i of a case"""
    pts = d["pts"] if d["pts"].ndim == 2 else d["pts"][i]
    K = d["K"] if d["K"].ndim == 2 else d["K"][i]
    return dict(pose_est=d["pose_est"][i], pose_gt=d["pose_gt"][i], pts=pts, K=K, syms=d["sets"][i],
                scale_est=None if d["scale_est"] is None else d["scale_est"][i],
                scale_gt=None if d["scale_gt"] is None else d["scale_gt"][i])


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    d = edge_data(name)
    return [REF.sym_errors(**instance(d, i)) for i in range(len(SET_SIZES))]


def lattice_data():
    """Every operation of the kernel is exact: model coordinates on a 1/16 grid with y in {-1, 0, 2}, poses that turn the
    model's y axis into the camera's z axis (z = y + 2 in {1, 2, 4}), power-of-two scales on x and z, symmetries that are
    quarter turns about y with dyadic offsets, fx = fy = 64.  Instance 0's set holds the turn its estimate stands on TWICE
    (indices 1 and 3): an exact tie, the lower index wins.  Instance 1 has unit scales and a set of two."""
    rng = np.random.default_rng(91)
    n = 300
    pts = np.stack([rng.integers(-16, 17, (2, n)) / 16, rng.choice([-1.0, 0.0, 2.0], (2, n)), rng.integers(-16, 17, (2, n)) / 16], -1)
    q = lambda k: np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [[-1, 0, 0], [0, 1, 0], [0, 0, -1]],
                            [[0, 0, -1], [0, 1, 0], [1, 0, 0]]], np.float64)[k]
    sym = lambda k, t=(0, 0, 0): np.hstack([q(k), np.reshape(np.asarray(t, np.float64), (3, 1))])
    sets = [np.stack([sym(0), sym(1, (0.25, 0, -0.125)), sym(2), sym(1, (0.25, 0, -0.125)), sym(3, (0, 0, 0.5))]),
            np.stack([sym(0), sym(2, (0.125, 0, 0))])]
    P = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)          # camera x = x, y = -z, z = y
    t_gt = np.array([[0.25, -0.5, 2.0], [-0.5, 0.25, 2.0]])
    scale = np.array([[2.0, 1.0, 0.5], [1.0, 1.0, 1.0]])
    pose_gt = np.stack([np.hstack([P, t_gt[i].reshape(3, 1)]) for i in range(2)])
    # the estimate: the ground truth composed with the picked member, pushed off by a lattice step
    pose_est = np.zeros((2, 3, 4))
    for i, (pick, push) in enumerate(((1, (0.125, -0.25, 0.0)), (1, (-0.25, 0.125, 0.0)))):
        s = sets[i][pick]
        pose_est[i, :, :3] = P @ s[:, :3]
        pose_est[i, :, 3] = P @ (scale[i] * s[:, 3]) + t_gt[i] + np.asarray(push)
    # diag(s_gt) R_s = R_s diag(s_est): the quarter turn of instance 0 swaps the scales of x and z
    scale_est = np.array([[0.5, 1.0, 2.0], [1.0, 1.0, 1.0]])
    K = np.array([[64, 0, 28], [0, 64, 20], [0, 0, 1]], np.float32)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    return dict(pts=f32(pts), pose_est=f32(pose_est), pose_gt=f32(pose_gt), scale_est=f32(scale_est), scale_gt=f32(scale),
                sets=sets, K=K, pick=[1, 1])


# ---- the device ---------------------------------------------------------------------------------------------------------------
def dev(a, dtype=None):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def run_sym(d, per_sym=True, rows=None):
    """``pose_errors.sym_errors`` on a case (``rows``: these instances only)"""
    import torch

    from catre_amd import pose_errors

    I = len(d["sets"])
    rows = list(range(I)) if rows is None else list(rows)
    pick = lambda a, per: None if a is None else dev(a[rows] if per else a, torch.float32)
    syms = pose_errors.SymSets.from_list([d["sets"][i] for i in rows], "cuda")
    return pose_errors.sym_errors(pick(d["pose_est"], True), pick(d["pose_gt"], True), pick(d["pts"], d["pts"].ndim == 3),
                                  pick(d["K"], d["K"].ndim == 3), syms, scale_est=pick(d["scale_est"], True),
                                  scale_gt=pick(d["scale_gt"], True), per_sym=per_sym)


# ---- the envelope the bounds are stated for -----------------------------------------------------------------------------------
ENVELOPE_SETS = (1, 2, SYM_TILE + 1)


@functools.lru_cache(maxsize=None)
def envelope_data():
    """The conditions the caps on the bounds are stated for, at their edge: model points up to |p| = 2 m in every direction (a
    tenth of them on that sphere, one straight towards the camera) around a centre 2.3 m in front of a 600 px camera, so that
    the nearest point stands at z = 0.3 m and points project many hundreds of pixels off the principal point."""
    rng = np.random.default_rng(7)
    I, n = len(ENVELOPE_SETS), 200
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    d = dict(pts=np.zeros((I, n, 3), np.float32), pose_est=np.zeros((I, 3, 4), np.float32), pose_gt=np.zeros((I, 3, 4), np.float32),
             scale_est=None, scale_gt=None, sets=[sym_set(S) for S in ENVELOPE_SETS], pick=[0] * I,
             K=np.array([[600, 0, 320], [0, 600, 240], [0, 0, 1]], np.float32))
    for i in range(I):
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        pts = 2 * v * rng.uniform(0.2, 1, (n, 1)) ** (1 / 3)
        pts[:20] = 2 * v[:20] * 0.999999
        R = REF.rotation(rng.uniform(0, np.pi), rng.normal(size=3))
        pts[0] = R.T @ np.array([0, 0, -2.0]) * 0.999999
        t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), 2.3 + 1e-4])
        dR = REF.rotation(np.deg2rad(rng.uniform(0.5, 2)), rng.normal(size=3))
        d["pts"][i], d["pose_gt"][i] = f32(pts), f32(np.hstack([R, t.reshape(3, 1)]))
        d["pose_est"][i] = f32(np.hstack([R @ dR, (t + np.array([0.002, -0.003, 0.02])).reshape(3, 1)]))
    return d


@functools.lru_cache(maxsize=None)
def envelope_reference():
    d = envelope_data()
    return [REF.sym_errors(**instance(d, i)) for i in range(len(ENVELOPE_SETS))]


# ---- VSD: pixels that tell a fused distance from the reference's ---------------------------------------------------------------
K_LM = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], np.float32)


def _dist_pair(x, y, d):
    """the reference's distance at pixel (x, y) for the fp32 depth d (every product and sum rounded, ``misc.py:643-645``), and
    what a compiler that contracts makes of it: fl(a a), then two fused multiply-adds - each exact product and sum rounded once"""
    from fractions import Fraction as Fr

    K = K_LM.astype(np.float64)
    px, py, dd = (x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], np.float64(d)
    a, b = px * dd, py * dd
    plain = np.sqrt(a * a + b * b + dd * dd)
    acc = float(Fr(float(a * a)) + Fr(float(b)) * Fr(float(b)))
    acc = float(Fr(acc) + Fr(float(dd)) * Fr(float(dd)))
    return float(plain), float(np.sqrt(np.float64(acc)))


@functools.lru_cache(maxsize=None)
def contraction_data(count=16, h=24, w=32):
    """``count`` windows of h x w with ONE rendered pixel each, in front of a hole (visible in ``bop19``), chosen by search so that
    |dist_gt - dist_est| differs between the reference's arithmetic and the contracted one.  Tau t sits on instance t's plain
    value where the contracted one is smaller (cost 1, contracted: 0), one double step above it where the contracted one is larger
    (cost 0, contracted: 1) -> dict with depth_est, depth_gt [count,h,w], taus, want [count] (the cost of instance t at tau t)
    and fused [count] (what contraction would count)."""
    rng = np.random.default_rng(17)
    est, gt = np.zeros((count, h, w), np.float32), np.zeros((count, h, w), np.float32)
    taus, want, fused = [], [], []
    while len(taus) < count:
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        dg, de = np.float32(rng.uniform(0.6, 1.4)), np.float32(rng.uniform(0.6, 1.4))
        (gp, gf), (ep, ef) = _dist_pair(x, y, dg), _dist_pair(x, y, de)
        plain, contracted = abs(gp - ep), abs(gf - ef)
        if plain == contracted or len(taus) % 2 != int(contracted > plain):      # both directions, in turn
            continue
        i = len(taus)
        gt[i, y, x], est[i, y, x] = dg, de
        tau = plain if contracted < plain else float(np.nextafter(plain, np.inf))
        taus.append(tau)
        want.append(int(plain >= tau))
        fused.append(int(contracted >= tau))
    return dict(depth_est=est, depth_gt=gt, depth_test=np.zeros((1, h, w), np.float32), K=K_LM, taus=taus, want=np.array(want),
                fused=np.array(fused))
