"""numpy restatement of the mesh rasteriser (``render.render_mesh``, ``csrc/catre_mesh.h``) in two stages.

Stage 1 (:func:`project`): the posed, projected and snapped vertices in fp64, with the per-vertex error bounds ``eu, ev, ez``
of ``tests/render_ref.project`` - the device computes them in fp32, so it is compared within those bounds.

Stage 2 (:func:`raster`): a function of the vertex RECORDS (xi, yi, bits of z, ok) alone - int64 coverage with the top-left
fill rule, fp64 depth and model coordinates in the device's operation order, the key minimum, the classes
(``render_ref.classes``), counts, culled counts and a per-pixel cover count.  Given the device's own records, every output of
the device equals this stage bit for bit: integer arithmetic is exact and every fp64 operation is IEEE on both sides."""
from collections import namedtuple

import numpy as np

from tests import render_ref as REF

SNAP = 256
LIMIT = 2 ** 23
BG = np.uint64(0xFFFFFFFFFFFFFFFF)

Projected = namedtuple("Projected", "u v z eu ev ez inst local")
Raster = namedtuple("Raster", "labels zbuf face cls labels_fit counts culled coord cover zd")


def instance_offsets(meshes, mesh_of):
    nv = np.array([len(meshes[g][0]) for g in mesh_of], np.int64)
    nf = np.array([len(meshes[g][1]) for g in mesh_of], np.int64)
    return np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(nf)])


# ---- stage 1 -----------------------------------------------------------------------------------------------------------------
def project(meshes, mesh_of, pose, scale, K, frame_of):
    """meshes: list of (verts, faces); pose [I,3,4], scale [I,3], K [F,3,3] -> ``Projected`` of [NV] float64 arrays,
    instance-major: u, v (pixels), z and their bounds."""
    out = [[] for _ in range(8)]
    for i, g in enumerate(mesh_of):
        v = np.asarray(meshes[g][0], np.float64)[None]
        z, u0, v0, _, _, ez, eu, ev, _ = REF.project(v, np.asarray(pose)[i:i + 1], np.asarray(scale)[i:i + 1], np.zeros(1), K,
                                                     [int(frame_of[i])], 1.0)
        for o, a in zip(out, (u0[0], v0[0], z[0], eu[0], ev[0], ez[0], np.full(v.shape[1], i), np.arange(v.shape[1]))):
            o.append(a)
    return Projected(*(np.concatenate(o) for o in out))


def snapped(p):
    """fp64 reference of the records -> (256 u, 256 v, ok_sure_true, ok_sure_false): where neither mask holds the fp32
    roundings of the device may decide ``ok`` either way."""
    with np.errstate(all="ignore"):
        x, y = SNAP * p.u, SNAP * p.v
        ex, ey = 0.5 + SNAP * p.eu, 0.5 + SNAP * p.ev
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(p.z)
        yes = fin & (p.z - p.ez > 0) & (np.abs(x) + ex < LIMIT) & (np.abs(y) + ey < LIMIT) & (np.abs(p.u) + p.eu < REF.FMAX) & \
            (np.abs(p.v) + p.ev < REF.FMAX)
        no = ~fin | (p.z + p.ez <= 0) | (np.abs(x) - ex >= LIMIT) | (np.abs(y) - ey >= LIMIT)
    return x, y, yes, no


def records(p):
    """Records as an exact renderer would write them: (xi, yi, bits of fl32(z), ok) [NV,4] int32 - for the host tests, whose
    scenes are chosen so that snapping is exact."""
    x, y, yes, _ = snapped(p)
    rec = np.zeros((len(x), 4), np.int32)
    rec[:, 0] = np.where(yes, np.rint(np.where(yes, x, 0)), 0).astype(np.int32)
    rec[:, 1] = np.where(yes, np.rint(np.where(yes, y, 0)), 0).astype(np.int32)
    rec[:, 2] = p.z.astype(np.float32).view(np.int32)
    rec[:, 3] = yes
    return rec


# ---- stage 2 -----------------------------------------------------------------------------------------------------------------
def _top_left(dx, dy):
    return dy < 0 or (dy == 0 and dx > 0)


def _edge(ax, ay, bx, by, sx, sy):
    return np.int64(bx - ax) * (sy - ay) - np.int64(by - ay) * (sx - ax)


def raster(rec, meshes, mesh_of, frame_of, n_frames, size, pixel_center=0.0, depth=None, delta=0.015):
    """rec [NV,4] int32 -> ``Raster``.  ``cover`` [F,H,W] counts the faces that cover each sample (all of them, not the winner
    alone); ``zd`` [F,H,W] float64 is the winner's depth BEFORE its one rounding to fp32."""
    rec = np.asarray(rec, np.int64)
    F, (H, W), I = int(n_frames), size, len(mesh_of)
    c = {0.0: 0, 0.5: SNAP // 2}[pixel_center]
    ivo, ifo = instance_offsets(meshes, mesh_of)
    keys = np.full((F, H, W), BG, np.uint64)
    zd = np.zeros((F, H, W))
    coord = np.zeros((F, H, W, 3), np.float32)
    cover = np.zeros((F, H, W), np.int32)
    culled = np.zeros(I, np.int32)
    for i, g in enumerate(mesh_of):
        verts, faces = meshes[g]
        verts64, vn, fr = np.asarray(verts, np.float32).astype(np.float64), len(verts), int(frame_of[i])
        for local, tri in enumerate(np.asarray(faces, np.int64)):
            if (tri < 0).any() or (tri >= vn).any():
                culled[i] += 1
                continue
            p = rec[ivo[i] + tri]
            if not p[:, 3].all():
                culled[i] += 1
                continue
            area2 = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0])
            if area2 == 0:
                continue
            order = [0, 2, 1] if area2 < 0 else [0, 1, 2]
            p, a, area2 = p[order], verts64[tri[order]], abs(int(area2))
            (x0, y0), (x1, y1), (x2, y2) = ((int(q[0]), int(q[1])) for q in p)
            z3 = p[:, 2].astype(np.int32).view(np.float32).astype(np.float64)
            ulo, uhi = max((min(x0, x1, x2) - c + SNAP - 1) >> 8, 0), min((max(x0, x1, x2) - c) >> 8, W - 1)
            vlo, vhi = max((min(y0, y1, y2) - c + SNAP - 1) >> 8, 0), min((max(y0, y1, y2) - c) >> 8, H - 1)
            if ulo > uhi or vlo > vhi:
                continue
            sx = (np.arange(ulo, uhi + 1, dtype=np.int64) * SNAP + c)[None, :]
            sy = (np.arange(vlo, vhi + 1, dtype=np.int64) * SNAP + c)[:, None]
            e = [_edge(x1, y1, x2, y2, sx, sy), _edge(x2, y2, x0, y0, sx, sy), _edge(x0, y0, x1, y1, sx, sy)]
            tl = [_top_left(x2 - x1, y2 - y1), _top_left(x0 - x2, y0 - y2), _top_left(x1 - x0, y1 - y0)]
            cov = np.ones(e[0].shape, bool)
            for ek, tk in zip(e, tl):
                cov &= (ek > 0) | ((ek == 0) & tk)
            if not cov.any():
                continue
            with np.errstate(all="ignore"):
                w = [ek.astype(np.float64) * (1.0 / z3[k]) for k, ek in enumerate(e)]
                Wn = (w[0] + w[1]) + w[2]
                zf64 = np.float64(area2) / Wn
                zf = zf64.astype(np.float32)
                key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(ifo[i] + local)
                cd = np.stack([(((w[0] * a[0, k] + w[1] * a[1, k]) + w[2] * a[2, k]) / Wn).astype(np.float32) for k in range(3)], -1)
            sl = (fr, slice(vlo, vhi + 1), slice(ulo, uhi + 1))
            cover[sl] += cov
            win = cov & (key < keys[sl])
            keys[sl] = np.where(win, key, keys[sl])
            zd[sl] = np.where(win, zf64, zd[sl])
            coord[sl] = np.where(win[..., None], cd, coord[sl])
    rendered = keys != BG
    gidx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    inst = np.where(rendered, np.searchsorted(ifo, gidx, side="right") - 1, 0)
    labels = np.where(rendered, inst + 1, 0).astype(np.int32)
    face = np.where(rendered, gidx - ifo[inst], -1).astype(np.int32)
    zbuf = np.where(rendered, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    if depth is None:
        cls = np.where(rendered, REF.AGREE, REF.BACKGROUND).astype(np.uint8)
    else:
        cls = REF.classes(zbuf, np.asarray(depth, np.float32).reshape(F, H, W), delta)
        cls[~rendered] = REF.BACKGROUND
    counts = np.zeros((I, 5), np.int32)
    for i in range(I):
        won = labels == i + 1
        counts[i, 0] = won.sum()
        for k in (REF.AGREE, REF.OCCLUDED, REF.FREE, REF.HOLE):
            counts[i, k] = (won & (cls == k)).sum()
    return Raster(labels, zbuf, face, cls, np.where(cls == REF.AGREE, labels, 0).astype(np.int32), counts, culled, coord, cover,
                  np.where(rendered, zd, 0.0))


def render(meshes, mesh_of, pose, scale, K, frame_of, n_frames, size, pixel_center=0.0, depth=None, delta=0.015):
    """Both stages with exact records (:func:`records`) -> (``Raster``, records, ``Projected``)."""
    p = project(meshes, mesh_of, pose, scale, K, frame_of)
    rec = records(p)
    return raster(rec, meshes, mesh_of, frame_of, n_frames, size, pixel_center, depth, delta), rec, p
