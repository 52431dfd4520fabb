"""fp64 numpy restatement of the splat render (``catre_amd/render.py``, ``csrc/catre_render.h``): projection, disc
footprints, the z-buffer with its tie order, the pixel classes and the point visibility - and, for every pixel and point,
whether the answer is SURE, i.e. cannot be moved by the fp32 roundings of the device.  The bounds are derived in the
docstring of ``tests/test_render.py``; the helpers below compute them per point."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
BACKGROUND, AGREE, OCCLUDED, FREE, HOLE = 0, 1, 2, 3, 4
FMAX = float(np.finfo(np.float32).max)

Ref = namedtuple("Ref", "labels zbuf point cls labels_fit counts visible sure unsure_of zb_bound vis_sure drawn")


def classes(zbuf, d_test, delta):
    """cls of rendered depth ``zbuf`` (0 = background) against observed depth ``d_test``; the difference is ONE fp32
    subtraction, as in the reference (``d_model.astype(np.float32) - d_test.astype(np.float32)``) and on the device."""
    zb, d = np.asarray(zbuf, np.float32), np.asarray(d_test, np.float32)
    diff = zb - d
    dl = np.float32(delta)
    c = np.full(zb.shape, AGREE, np.uint8)
    c[diff < -dl] = FREE
    c[diff > dl] = OCCLUDED
    c[~(d > 0)] = HOLE
    c[~(zb > 0)] = BACKGROUND
    return c


def posed(kps, pose, scale):
    """[I,M,3] float64: R (s * x) + t"""
    k, p, s = (np.asarray(a, np.float64) for a in (kps, pose, scale))
    return np.einsum("irc,imc->imr", p[:, :, :3], k * s[:, None, :]) + p[:, None, :, 3]


def project(kps, pose, scale, rho, K, frame_of, r_max):
    """Per point, float64 [I,M]: z, u0, v0, r, drawn, and the error bounds ez, eu, ev, er (see tests/test_render.py)."""
    with np.errstate(all="ignore"):
        P = posed(kps, pose, scale)
        Kf = np.asarray(K, np.float64)[np.asarray(frame_of)]
        fx, fy, cx, cy = (Kf[:, a, b][:, None] for a, b in ((0, 0), (1, 1), (0, 2), (1, 2)))
        x, y, z = P[..., 0], P[..., 1], P[..., 2]
        ax, ay = fx * x / z, fy * y / z
        u0, v0 = ax + cx, ay + cy
        rr = fx * np.asarray(rho, np.float64)[:, None] / z
        r = np.where(rr > r_max, float(r_max), rr)
        drawn = (z > 0) & (np.abs(u0) <= FMAX) & (np.abs(v0) <= FMAX) & (np.abs(r) <= FMAX)
        ep = 8 * U * np.linalg.norm(P, axis=-1)
        ez = ep
        eu = (fx + np.abs(ax)) * ep / z + 2 * U * np.abs(ax) + U * np.abs(u0)
        ev = (fy + np.abs(ay)) * ep / z + 2 * U * np.abs(ay) + U * np.abs(v0)
        er = np.abs(r) * (8 * U + ep / z)
    return z, u0, v0, r, drawn, ez, eu, ev, er


def render(kps, pose, scale, rho, K, frame_of, n_frames, size, r_max, depth=None, delta=0.015):
    """-> ``Ref``.  kps [I,M,3], pose [I,3,4], scale [I,3], rho [I], K [F,3,3]; every value fp32-representable (taken to
    float64 here).  ``sure`` [F,H,W]: no candidate disc has |d2 - r2| within its bound, the two nearest covering points
    differ in z by more than twice the z bound, and an observed depth is further than the class bound from both class
    boundaries.  ``unsure_of`` [I]: non-sure pixels an instance covers (it could win or lose each).  ``zb_bound`` [F,H,W]:
    the z bound of the winner.  ``vis_sure`` [I,M]: the visibility of the point cannot flip."""
    kps = np.asarray(kps, np.float64)
    I, M = kps.shape[:2]
    F, (H, W) = int(n_frames), size
    dl = float(np.float32(delta))
    z, u0, v0, r, drawn, ez, eu, ev, er = project(kps, pose, scale, rho, K, frame_of, r_max)
    z1 = np.full((F, H, W), np.inf)
    z2 = np.full((F, H, W), np.inf)
    e1 = np.zeros((F, H, W))
    e2 = np.zeros((F, H, W))
    lab = np.zeros((F, H, W), np.int32)
    pt = np.full((F, H, W), -1, np.int32)
    edge = np.zeros((F, H, W), bool)
    cover = np.zeros((I, F, H, W), bool)        # pixels an instance covers or may cover
    for i in range(I):
        f = int(frame_of[i])
        for m in range(M):
            if not drawn[i, m]:
                continue
            a, b, rad = u0[i, m], v0[i, m], r[i, m]
            xs = np.arange(int(np.clip(np.floor(a - rad) - 1, 0, W)), int(np.clip(np.ceil(a + rad) + 2, 0, W)))
            ys = np.arange(int(np.clip(np.floor(b - rad) - 1, 0, H)), int(np.clip(np.ceil(b + rad) + 2, 0, H)))
            if not len(xs) or not len(ys):
                continue
            du, dv = xs[None, :] - a, ys[:, None] - b
            d2, r2 = du * du + dv * dv, rad * rad
            bound = 2 * (2 * np.abs(du) * eu[i, m] + 2 * np.abs(dv) * ev[i, m] + 4 * U * d2 + 2 * abs(rad) * er[i, m] + U * r2)
            near = np.abs(d2 - r2) <= bound
            inside = d2 <= r2
            sl = (f, slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
            edge[sl] |= near
            cover[(i,) + sl] |= inside | near
            zz = z[i, m]
            first = inside & (zz < z1[sl])          # ascending (i, m): a strict < keeps the lower instance / point on a tie
            second = inside & ~first & (zz < z2[sl])
            z2[sl] = np.where(first, z1[sl], np.where(second, zz, z2[sl]))
            e2[sl] = np.where(first, e1[sl], np.where(second, ez[i, m], e2[sl]))
            z1[sl] = np.where(first, zz, z1[sl])
            e1[sl] = np.where(first, ez[i, m], e1[sl])
            lab[sl] = np.where(first, i + 1, lab[sl])
            pt[sl] = np.where(first, m, pt[sl])
    rendered = lab > 0
    zbuf = np.where(rendered, z1, 0.0)
    with np.errstate(invalid="ignore"):     # inf - inf on background pixels
        sure = ~edge & ~(rendered & (z2 - z1 <= 2 * np.maximum(e1, e2)))
    if depth is not None:
        d = np.asarray(depth, np.float64).reshape(F, H, W)
        diff = zbuf - d
        cls = np.full((F, H, W), AGREE, np.uint8)
        cls[diff < -dl] = FREE
        cls[diff > dl] = OCCLUDED
        cls[~(d > 0)] = HOLE
        cb = e1 + 2 * U * np.maximum(np.abs(zbuf), np.abs(d))
        sure &= ~(rendered & (d > 0) & (np.minimum(np.abs(diff - dl), np.abs(diff + dl)) <= cb))
    else:
        d = None
        cls = np.full((F, H, W), AGREE, np.uint8)
    cls[~rendered] = BACKGROUND
    counts = np.zeros((I, 5), np.int64)
    for i in range(I):
        won = lab == i + 1
        counts[i, 0] = won.sum()
        for c in (AGREE, OCCLUDED, FREE, HOLE):
            counts[i, c] = (won & (cls == c)).sum()
    unsure_of = np.array([(cover[i] & ~sure).sum() for i in range(I)])
    # point visibility
    vis = np.zeros((I, M), bool)
    vsure = np.ones((I, M), bool)
    for i in range(I):
        f = int(frame_of[i])
        for m in range(M):
            if not drawn[i, m]:
                continue
            a, b = u0[i, m], v0[i, m]
            uc, vc = np.rint(a), np.rint(b)          # half to even, like rintf
            if abs(a - np.floor(a) - 0.5) <= eu[i, m] or abs(b - np.floor(b) - 0.5) <= ev[i, m]:
                vsure[i, m] = False
            if not (0 <= uc <= W - 1 and 0 <= vc <= H - 1):
                continue
            px = (f, int(vc), int(uc))
            if not sure[px]:
                vsure[i, m] = False
            behind = z[i, m] - zbuf[px]
            if abs(behind - dl) <= ez[i, m] + e1[px] + 2 * U * abs(z[i, m]):
                vsure[i, m] = False
            vis[i, m] = lab[px] == i + 1 and behind <= dl and cls[px] != OCCLUDED
    return Ref(lab, zbuf, pt, cls, np.where(cls == AGREE, lab, 0).astype(np.int32), counts, vis, sure, unsure_of,
               np.where(rendered, e1, 0.0), vsure, drawn)
