"""Seeded inputs shared by ``tests/test_render_host.py`` (CPU) and ``tests/test_render.py`` (device): the two edge cases of
the splat render, their restatement (computed once), and small helpers."""
import functools

import numpy as np

from tests import render_ref as REF

EDGE_SEED = 20261
RHO_REL = 0.06
EDGE_CASES = ("near_I3_M65_48x64", "deep_I2_M257_96x128_F2")


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def box_points(rng, n, ext):
    """n points on the surface of a box of extents ``ext``, centred on the origin"""
    p = rng.uniform(-0.5, 0.5, (n, 3))
    face = rng.integers(0, 3, n)
    p[np.arange(n), face] = np.where(rng.random(n) < 0.5, -0.5, 0.5)
    return p * np.asarray(ext)


def rho_of(scale, rho_rel=RHO_REL):
    """float64 of what ``render.splat_prior`` computes in fp32 (the restatement's radius bound allows for that rounding)"""
    return rho_rel * np.linalg.norm(np.asarray(scale, np.float64), axis=1)


def pose_of(R, t):
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def camera(H, W, f):
    return np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]], np.float32)


@functools.lru_cache(maxsize=None)
def edge_data(name):
    """name -> dict of fp32 arrays.  Between them the two cases hold: discs clipped at the left / top (near) and right / bottom
    (deep) borders, an instance behind the camera and one with a NaN pose (near), one wholly outside the image (deep), a NaN
    point and a single point behind the camera (near), radii at the ``r_max`` cap (both) and below half a pixel (deep: a
    box 3.5 m deep, whose far end has discs smaller than a pixel)."""
    rng = np.random.default_rng(EDGE_SEED + EDGE_CASES.index(name))
    if name == EDGE_CASES[0]:
        I, M, (H, W), F, frame_of, f, r_max = 3, 65, (48, 64), 1, [0, 0, 0], 60.0, 6.0
        kps = np.stack([box_points(rng, M, (0.5, 0.4, 0.6)) for _ in range(I)])
        scale = np.array([[0.8, 1.0, 1.2], [1.0, 1.0, 1.0], [1.1, 0.9, 1.0]])
        pose = np.stack([pose_of(rotation(rng), t) for t in ((-0.35, -0.25, 0.9), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0))])
        pose[2, 1, 1] = np.nan
        kps[0, 7] = np.nan
        kps[0, 11] = pose[0, :, :3].T @ np.array([0.0, 0.0, -2.0]) / scale[0]     # a single point behind the camera
        depth = 0.9 + rng.normal(0, 0.15, (F, H, W))
    else:
        I, M, (H, W), F, frame_of, f, r_max = 2, 257, (96, 128), 2, [1, 0], 120.0, 2.0
        kps = np.stack([box_points(rng, M, (0.5, 0.4, 3.5)), box_points(rng, M, (0.3, 0.3, 0.3))])
        scale = np.array([[0.12, 0.1, 0.11], [1.0, 1.0, 1.0]])
        kps[0] /= scale[0]                                        # a 0.5 x 0.4 x 3.5 m box with a small |scale|: rho = 0.0115 m
        tilt = np.array([[1, 0, 0], [0, np.cos(0.05), -np.sin(0.05)], [0, np.sin(0.05), np.cos(0.05)]])
        pose = np.stack([pose_of(tilt, (0.15, 0.1, 2.25)), pose_of(rotation(rng), (5.0, 0.0, 1.0))])
        depth = 2.0 + rng.normal(0, 1.0, (F, H, W))
    depth[rng.random((F, H, W)) < 0.1] = 0
    d = dict(kps=kps, pose=pose, scale=scale, depth=np.maximum(depth, 0))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    d.update(K=camera(H, W, f)[None].repeat(F, 0), frame_of=frame_of, F=F, size=(H, W), r_max=r_max, delta=0.015, name=name)
    return d


@functools.lru_cache(maxsize=None)
def edge_reference(name, with_depth=True):
    d = edge_data(name)
    return REF.render(d["kps"], d["pose"], d["scale"], rho_of(d["scale"]), d["K"], d["frame_of"], d["F"], d["size"], d["r_max"],
                      depth=d["depth"] if with_depth else None, delta=d["delta"])


def dev(a, dtype=None):
    import torch

    return None if a is None else torch.as_tensor(a, dtype=dtype).cuda()


def run_splat(d, frame_of="all", with_depth=True, return_visible=True, rho_rel=RHO_REL, **kw):
    """``render.splat_prior`` on the device for a dict of :func:`edge_data`'s form (``rho``, if the dict has one, sets the radii)"""
    import torch

    from catre_amd import render

    if d.get("rho") is not None:
        kw["rho"] = dev(d["rho"], torch.float32)

    return render.splat_prior(dev(d["kps"]), dev(d["pose"]), dev(d["scale"]), d["K"], d["size"],
                              frame_of=d["frame_of"] if frame_of == "all" else frame_of, n_frames=d["F"], rho_rel=rho_rel,
                              r_max=d["r_max"], depth=dev(d["depth"]) if with_depth else None, delta=d["delta"],
                              return_visible=return_visible, **kw)
