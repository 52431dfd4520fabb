"""The splat render on the device (``catre_amd/render.py``, ``csrc/catre_render.h``) against the fp64 restatement
``tests/render_ref.py`` (itself pinned to the reference's ``lib/pysixd/visibility.py`` by ``tests/test_render_host.py``),
bit for bit where the arithmetic is exact, and ``Tracker(crop="render")`` against the composition written out by hand.

Bounds, derived from the arithmetic (u = 2^-24, the fp32 unit round-off; ``render_ref.project`` computes them per point):
* a point p = R (s x) + t carries one rounding per product / fma / sum and coordinate - under 4 sqrt(3) u |s x| + u |p|
  <= 8 u |p| for the objects here (``tests/test_track.py``).  e_p = 8 u |p| bounds every coordinate, so e_z = e_p: the bound
  on ``zbuf`` where the winner is the restatement's.
* u0 = fl(fl(fl(fx x) / z) + cx).  With a = fx x / z: the error of x moves a by fx e_p / z, the error of z by |a| e_p / z,
  the product and the quotient add 2 u |a|, the sum u |u0|:  e_u = (fx + |a|) e_p / z + 2 u |a| + u |u0|; e_v alike.
* r = fl(fl(fx rho) / z), capped: rho = rho_rel |scale| is computed in fp32 on the device (a cast, three squares, two sums, a
  root, a product: under 6 u relative), the product and the quotient add 2 u, z adds e_p / z:  e_r = r (8 u + e_p / z).
  min(., r_max) does not enlarge it.
* d2 = fma(du, du, fl(dv dv)) with du = fl(u - u0): du carries e_u + u |du|, so d2 moves by 2 |du| e_u + 2 |dv| e_v +
  2 u (du^2 + dv^2) from its inputs and 2 u d2 from its own two roundings; r2 = fl(r r) moves by 2 r e_r + u r2.  A pixel
  is NOT SURE for a disc if |d2 - r2| <= 2 (2 |du| e_u + 2 |dv| e_v + 4 u d2 + 2 r e_r + u r2) - twice the sum.
* the z-buffer: two covering points whose z differ by at most twice the larger e_z may swap: not sure.
* the class: diff = fl(zbuf - d) carries e_z + u |diff| <= e_z + 2 u max(|zbuf|, |d|); a pixel within that of +-delta is not
  sure.  A point's visibility is not sure if u0 or v0 lies within e_u / e_v of a half-integer, if its centre pixel is not
  sure, or if p.z - zbuf lies within e_z(point) + e_z(winner) + 2 u |p.z| of delta.
``labels``, ``point`` and ``cls`` are compared at sure pixels, ``visible`` at sure points; ``tests/test_render_host.py`` checks
on the CPU that at most 1 % of the rendered pixels of a case are not sure."""
import os

import numpy as np
import pytest
import torch

from tests import render_cases as C
from tests import render_ref as REF
from tests.util import GOLDEN_DIR

U = REF.U


def _np(t):
    return t.cpu().numpy()


def _same_splat(a, b, what=""):
    for f in ("labels", "zbuf", "point", "cls", "labels_fit", "counts", "visible"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (what, f)
        if x is not None:
            assert torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y), (what, f)


def _equals_ref(got, r, what=""):
    """every output of a device ``Splat`` equals the restatement's, bit for bit"""
    for f in ("labels", "point", "cls", "labels_fit", "counts"):
        assert np.array_equal(_np(getattr(got, f)).astype(np.int64), np.asarray(getattr(r, f)).astype(np.int64)), (what, f)
    assert np.array_equal(_np(got.zbuf).view(np.uint32), r.zbuf.astype(np.float32).view(np.uint32)), (what, "zbuf")
    if got.visible is not None:
        assert np.array_equal(_np(got.visible), r.visible), (what, "visible")


# ---- 1. edges against the restatement ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.EDGE_CASES)
def test_edges_against_the_restatement(name):
    d, r = C.edge_data(name), C.edge_reference(name)
    got = C.run_splat(d)
    sure = r.sure
    lab, pt, cls, zb = _np(got.labels), _np(got.point), _np(got.cls), _np(got.zbuf).astype(np.float64)
    print(name, "rendered", int((r.labels > 0).sum()), "non-sure", int((~sure).sum()), "labels differ at", int((lab != r.labels).sum()),
          "zbuf dev", float(np.abs(zb - r.zbuf)[sure].max()), "bound", float(r.zb_bound.max()), "counts", _np(got.counts).tolist())
    assert np.array_equal(lab[sure], r.labels[sure]) and np.array_equal(pt[sure], r.point[sure])
    assert np.array_equal(cls[sure], r.cls[sure])
    assert np.array_equal(_np(got.labels_fit), np.where(cls == REF.AGREE, lab, 0))
    assert (np.abs(zb - r.zbuf)[sure] <= r.zb_bound[sure]).all()
    counts = _np(got.counts)
    assert (np.abs(counts - r.counts) <= r.unsure_of[:, None]).all(), (counts.tolist(), r.counts.tolist(), r.unsure_of.tolist())
    assert (counts[:, 0] == counts[:, 1:].sum(1)).all()
    for i in range(counts.shape[0]):
        if r.counts[i, 0] == 0 and r.unsure_of[i] == 0:                  # behind the camera, NaN pose, wholly outside
            assert (counts[i] == 0).all() and not (lab == i + 1).any(), i
    assert (counts[:, 0] == 0).any()
    vs = r.vis_sure
    assert np.array_equal(_np(got.visible)[vs], r.visible[vs])
    # without an observed depth every rendered pixel is AGREE and labels_fit is labels
    r0 = C.edge_reference(name, False)
    g0 = C.run_splat(d, with_depth=False)
    assert torch.equal(g0.labels, got.labels) and torch.equal(g0.zbuf, got.zbuf) and torch.equal(g0.labels_fit, g0.labels)
    assert np.array_equal(_np(g0.cls), (lab > 0).astype(np.uint8)) and np.array_equal(_np(g0.visible)[r0.vis_sure], r0.visible[r0.vis_sure])


# ---- 2. exact lattice ---------------------------------------------------------------------------------------------------
def lattice_data():
    """fx = fy = 64, z in {1, 2, 4}, x and y multiples of 1/64: u0, v0 are multiples of 1/4, r of 1/4 (rho = 4/64 and 5/64:
    r in {4, 2, 1} and {5, 2.5, 1.25}), d2 and r2 multiples of 1/16 below 2^24: every quantity is exact in fp32."""
    rng = np.random.default_rng(78)
    I, M, H, W = 2, 300, 40, 56
    z = rng.choice([1.0, 2.0, 4.0], (I, M), p=[0.1, 0.3, 0.6])
    cam = np.stack([rng.integers(-2, W + 2, (I, M)) - 28, rng.integers(-2, H + 2, (I, M)) - 20], -1)   # whole pixels at z = 1 ...
    frac = rng.integers(0, 4, (I, M, 2)) / 4 * (z[..., None] == 4) + rng.integers(0, 2, (I, M, 2)) / 2 * (z[..., None] == 2)
    xy = (cam + frac) * z[..., None] / 64                                                     # ... halves at 2, quarters at 4
    p = np.concatenate([xy, z[..., None]], -1)
    p[0, 10], p[0, 11] = [-10 / 64, 5 / 64, 1.0], [10 / 64, -8 / 64, 1.0]
    p[0, 20] = p[0, 11]                          # a duplicated point inside a tile ...
    p[0, 280] = p[0, 10]                         # ... and across two: the lower m wins
    p[1, 5] = p[0, 10]                           # the same point in two instances: the lower i wins
    # both instances stand at the same signed permutation, lattice translation and power-of-two scale: kps = inverse
    P = np.array([[0, -1, 0, 0.5], [0, 0, 1, -0.25], [-1, 0, 0, 3.0]])
    s = np.array([2.0, 1.0, 0.5])
    kps = np.einsum("rc,imr->imc", P[:, :3], p - P[:, 3]) / s
    K = np.array([[64, 0, 28], [0, 64, 20], [0, 0, 1]], np.float32)[None]
    d = dict(kps=kps.astype(np.float32), pose=np.stack([P, P]).astype(np.float32), scale=np.stack([s, s]).astype(np.float32),
             rho=np.array([4 / 64, 5 / 64], np.float32), K=K, frame_of=[0, 0], F=1, size=(H, W), r_max=64.0, delta=2.0 ** -6,
             depth=None)
    assert np.array_equal(REF.posed(d["kps"], d["pose"], d["scale"]), p)
    return d


@pytest.mark.gpu
def test_exact_lattice():
    d = lattice_data()
    ref = lambda depth: REF.render(d["kps"], d["pose"], d["scale"], d["rho"], d["K"], d["frame_of"], 1, d["size"], d["r_max"],
                                   depth=depth, delta=d["delta"])
    r0 = ref(None)
    # an observed depth on diff == +-delta, one ulp beyond either, holes and equal depths, in turn over the rendered pixels
    zb = r0.zbuf.astype(np.float32)
    dl = np.float32(d["delta"])
    k = np.arange(zb.size).reshape(zb.shape) % 6
    lo, hi = zb - dl, zb + dl
    depth = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(9)),
                                                                  np.zeros_like(zb)], zb).astype(np.float32)
    depth[zb == 0] = 1.0
    d["depth"] = depth
    r = ref(depth)
    # exact in fp32, as claimed
    z, u0, v0, rad, drawn, *_ = REF.project(d["kps"], d["pose"], d["scale"], d["rho"], d["K"], d["frame_of"], d["r_max"])
    assert drawn.all() and set(np.unique(z)) == {1.0, 2.0, 4.0} and set(np.unique(rad)) == {5.0, 4.0, 2.5, 2.0, 1.25, 1.0}
    for a in (u0, v0, rad):
        assert np.array_equal(a * 4, np.round(a * 4)) and np.abs(a).max() < 2 ** 12
    rendered = r.labels > 0
    iw, mw = r.labels[rendered] - 1, r.point[rendered]
    vv, uu = np.nonzero(rendered[0])
    d2w = (uu - u0[iw, mw]) ** 2 + (vv - v0[iw, mw]) ** 2
    assert (d2w == rad[iw, mw] ** 2).any() and (d2w <= rad[iw, mw] ** 2).all(), "the seed must put pixels on d2 == r2"
    # ties: the duplicates (m = 20 of 11, m = 280 of 10) never win, instance 1's copy of (0, 10) loses that point's centre pixel
    won = lambda i, m: ((r.labels == i + 1) & (r.point == m)).sum()
    assert won(0, 10) > 0 and won(0, 11) > 0 and won(0, 20) == 0 and won(0, 280) == 0
    c10 = (0, int(v0[0, 10]), int(u0[0, 10]))
    assert r.labels[c10] == 1 and r.point[c10] <= 10 and z[1, 5] == z[0, 10] == 1 and (u0[1, 5], v0[1, 5]) == (u0[0, 10], v0[0, 10])
    diff = zb - depth
    on = rendered & (depth > 0)
    assert (diff[on] == dl).any() and (diff[on] == -dl).any() and (r.cls == REF.OCCLUDED).any() and (r.cls == REF.FREE).any()
    assert np.array_equal(r.cls, REF.classes(zb, depth, dl)) and not r.visible.all() and r.visible.any()
    got = C.run_splat(d)
    _equals_ref(got, r, "lattice")
    _equals_ref(C.run_splat(d, with_depth=False), r0, "lattice without depth")


# ---- 3. round trip with the back-projection -------------------------------------------------------------------------------
def backproject(depth, K):
    """pcl_point's formula in fp32, for the pixels with depth > 0 -> [n,3] fp32 in row-major pixel order"""
    v, u = np.nonzero(depth > 0)
    z = depth[v, u].astype(np.float32)
    fx, fy, cx, cy = (np.float32(K[a, b]) for a, b in ((0, 0), (1, 1), (0, 2), (1, 2)))
    x = (u.astype(np.float32) - cx) * z / fx
    y = (v.astype(np.float32) - cy) * z / fy
    return np.stack([x, y, z], -1).astype(np.float32)


def splat_depth_image(d_model, d_test, delta):
    from catre_amd import render

    K = C.camera(*d_model.shape, 50.0)
    pts = backproject(d_model, K)
    eye = torch.eye(3, 4)[None].cuda()
    return render.splat_prior(C.dev(pts)[None], eye, torch.ones(1, 3).cuda(), K, d_model.shape, rho=torch.full((1,), 0.3 / 50.0).cuda(),
                              r_max=1.0, depth=C.dev(d_test)[None], delta=float(delta), return_visible=True)


@pytest.mark.gpu
def test_round_trip_with_the_back_projection():
    rng = np.random.default_rng(79)
    H, W = 24, 32
    patch = np.zeros((H, W), np.float32)
    patch[5:17, 7:25] = rng.uniform(0.7, 1.3, (12, 18)).astype(np.float32)      # r = 15 / z / 50: 0.23 .. 0.43 px
    got = splat_depth_image(patch, patch, 0.0)
    assert np.array_equal(_np(got.labels)[0] != 0, patch > 0)
    assert np.array_equal(_np(got.zbuf)[0].view(np.uint32), patch.view(np.uint32))
    assert np.array_equal(_np(got.cls)[0], (patch > 0).astype(np.uint8)) and got.visible.all()
    assert np.array_equal(_np(got.point)[0][patch > 0], np.arange(216)) and _np(got.counts).tolist() == [[216, 216, 0, 0, 0]]
    # the fixture's rendered and observed depth: the device's classes are the reference's two masks
    g = np.load(os.path.join(GOLDEN_DIR, "visib_mask.npz"))
    got = splat_depth_image(g["d_model"], g["d_test"], g["delta"])
    cls = _np(got.cls)[0]
    assert np.array_equal(_np(got.zbuf)[0].view(np.uint32), g["d_model"].view(np.uint32))
    assert np.array_equal((cls == REF.AGREE) | (cls == REF.FREE), g["bop18"])
    assert np.array_equal((cls == REF.AGREE) | (cls == REF.FREE) | (cls == REF.HOLE), g["bop19"])
    assert np.array_equal(cls, REF.classes(g["d_model"], g["d_test"], g["delta"]))
    assert np.array_equal(_np(got.visible)[0], (cls != REF.OCCLUDED)[g["d_model"] > 0])


# ---- 4. corners -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_corners():
    from catre_amd import render

    H, W = 13, 19                                                       # 247 pixels: not a multiple of 256
    K = np.array([[8, 0, 9], [0, 8, 6], [0, 0, 1]], np.float32)
    eye, one = torch.eye(3, 4)[None].cuda(), torch.ones(1, 3).cuda()
    for (u, v) in ((0, 0), (W - 1, H - 1)):
        kps = torch.tensor([[[(u - 9) / 8, (v - 6) / 8, 1.0]]]).cuda()
        got = render.splat_prior(kps, eye, one, K, (H, W), rho=torch.full((1,), 0.3 / 8).cuda(), return_visible=True)
        want = np.zeros((H, W), np.int32)
        want[v, u] = 1
        assert np.array_equal(_np(got.labels)[0], want) and got.visible.all() and _np(got.counts).tolist() == [[1, 1, 0, 0, 0]]
        assert np.array_equal(_np(got.point)[0], want - 1) and np.array_equal(_np(got.zbuf)[0], want.astype(np.float32))
        for big in (1e9, 3e38):                                         # r * r overflows to +inf for the second: still every pixel
            got = render.splat_prior(kps, eye, one, K, (H, W), rho=torch.full((1,), big).cuda(), r_max=big)
            assert (got.labels == 1).all() and (got.zbuf == 1).all() and (got.point == 0).all() and (got.cls == 1).all()
            assert _np(got.counts).tolist() == [[H * W, H * W, 0, 0, 0]]
    # a hair in front of the camera: centres beyond any int, nothing drawn, nothing out of bounds
    kps = torch.tensor([[[0.3, -0.2, 1e-36]]]).cuda()
    got = render.splat_prior(kps, eye, one, K, (H, W), rho=torch.full((1,), 0.01).cuda(), return_visible=True)
    assert not got.labels.any() and not got.visible.any() and not got.counts.any() and (got.point == -1).all()


# ---- 5. independence and determinism ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frames_are_independent_and_calls_repeat():
    d = C.edge_data(C.EDGE_CASES[1])
    both = C.run_splat(d)
    _same_splat(C.run_splat(d), both, "second call")
    for f in range(d["F"]):
        mine = [i for i, g in enumerate(d["frame_of"]) if g == f]
        one = dict(d, kps=d["kps"][mine], pose=d["pose"][mine], scale=d["scale"][mine], depth=d["depth"][f:f + 1], K=d["K"][f:f + 1],
                   frame_of=[0] * len(mine), F=1)
        got = C.run_splat(one)
        orig = torch.tensor([0] + [i + 1 for i in mine], dtype=torch.int32).cuda()
        assert torch.equal(orig[got.labels.long()][0], both.labels[f]) and torch.equal(orig[got.labels_fit.long()][0], both.labels_fit[f])
        for k in ("zbuf", "point", "cls"):
            assert torch.equal(getattr(got, k)[0], getattr(both, k)[f]), (f, k)
        assert torch.equal(got.counts, both.counts[mine]) and torch.equal(got.visible, both.visible[mine])
    assert both.labels[1].any() and not both.labels[0].any()


# ---- 6. visibility and fit_score_visible ----------------------------------------------------------------------------------------
def occluded_scene():
    """Two boxes in front of a wall; the observed depth is their own render, with a plane in front of the left half of box 0."""
    rng = np.random.default_rng(80)
    I, M, N, (H, W) = 2, 256, 128, (64, 96)
    kps = np.stack([C.box_points(rng, M, (1.0, 1.0, 1.0)) for _ in range(I)]).astype(np.float32)
    scale = np.array([[0.25, 0.2, 0.22], [0.2, 0.25, 0.2]], np.float32)
    pose = np.stack([C.pose_of(C.rotation(rng), t) for t in ((-0.18, 0.0, 1.0), (0.2, 0.02, 1.2))]).astype(np.float32)
    K = C.camera(H, W, 90.0)[None]
    d = dict(kps=kps, pose=pose, scale=scale, K=K, frame_of=[0, 0], F=1, size=(H, W), r_max=24.0, delta=0.015, depth=None)
    clear = REF.render(kps, pose, scale, C.rho_of(scale), K, [0, 0], 1, (H, W), 24.0)
    depth = np.where(clear.labels > 0, clear.zbuf, 2.0).astype(np.float32)
    pcl = np.stack([backproject(np.where(clear.labels[0] == i + 1, depth[0], 0), K[0])[rng.permutation((clear.labels == i + 1).sum())[:N]]
                    for i in range(I)])
    u_mid = int(round(float(90.0 * pose[0, 0, 3] / pose[0, 2, 3] + K[0, 0, 2])))
    depth[0, :, :u_mid] = np.where(clear.labels[0, :, :u_mid] == 1, 0.6, depth[0, :, :u_mid])
    d["depth"] = depth
    return d, pcl.astype(np.float32)


@pytest.mark.gpu
def test_visibility_and_fit_score_visible():
    from catre_amd import render, tracking

    d, pcl = occluded_scene()
    r = REF.render(d["kps"], d["pose"], d["scale"], C.rho_of(d["scale"]), d["K"], [0, 0], 1, d["size"], d["r_max"], depth=d["depth"],
                   delta=d["delta"])
    assert (r.cls == REF.OCCLUDED).sum() > 100 and 0.05 < r.visible[0].mean() < r.visible[1].mean()
    got = C.run_splat(d)
    vs = r.vis_sure
    assert (~vs).sum() <= 0.02 * vs.size and np.array_equal(_np(got.visible)[vs], r.visible[vs])
    args = [C.dev(a) for a in (pcl, d["kps"], d["pose"], d["scale"])]
    score, d_vis, share = render.fit_score_visible(*args, d["K"][0], C.dev(d["depth"]))
    plain = tracking.fit_score(*args)
    for f in plain._fields:
        assert torch.equal(getattr(score, f), getattr(plain, f)), f
    P = REF.posed(d["kps"], d["pose"], d["scale"])
    nn = np.sqrt(((P[:, :, None, :] - pcl.astype(np.float64)[:, None, :, :]) ** 2).sum(-1)).min(-1)          # [I,M]
    dvis, vis = _np(d_vis).astype(np.float64), _np(got.visible)
    for i in range(2):
        bound = 16 * U * (np.linalg.norm(P[i], axis=-1).max() + np.linalg.norm(pcl[i], axis=-1).max())
        want = nn[i][r.visible[i]].mean()
        slack = (~vs[i]).sum() * nn[i].max() / max(1, min(r.visible[i].sum(), vis[i].sum()))                 # points that may flip
        print(i, "d_prior_visible", dvis[i], "restatement", want, "bound", bound + slack, "d_prior", plain.d_prior[i].item(),
              "share", share[i].item())
        assert abs(dvis[i] - want) <= bound + slack + U * want
        assert share[i].item() == float(np.float32(vis[i].sum()) / np.float32(vis.shape[1]))
    assert d_vis[0].item() < plain.d_prior[0].item()                     # the occluded half no longer counts against the fit
    # an instance without a visible point: NaN
    hidden = np.where(r.labels > 0, np.float32(0.3), d["depth"]).astype(np.float32)
    _, d_none, share0 = render.fit_score_visible(*args, d["K"][0], C.dev(hidden))
    assert torch.isnan(d_none).all() and not share0.any()


# ---- 7. Tracker(crop="render") ---------------------------------------------------------------------------------------------------
N_PTS, N_ITER, TH, TW = 64, 2, 48, 64
CROP = dict(crop_delta=0.05, rho_rel=0.1, r_max=24.0)


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
    inputs = synth.make_inputs(2, N_PTS, N_PTS, seed=9)
    kps = inputs["obj_kps"].numpy().astype(np.float32)
    scale = np.array([[0.3, 0.2, 0.06], [0.2, 0.3, 0.06]], np.float32)                     # flat towards the camera
    rotz = lambda a: np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    pose = np.stack([C.pose_of(rotz(a), t) for a, t in ((0.3, (-0.2, 0.0, 0.9)), (-0.5, (0.22, 0.03, 1.0)))]).astype(np.float32)
    K = C.camera(TH, TW, 0.9 * TW)
    # the objects at their carried pose (their own render, sure pixels only), one in either half of the image, and behind
    # each a plane 6 cm beyond its farthest pixel: further than crop_delta behind every pixel of it, and inside its ball
    r = REF.render(kps, pose, scale, C.rho_of(scale, CROP["rho_rel"]), K[None], [0, 0], 1, (TH, TW), CROP["r_max"])
    obj = (r.labels[0] > 0) & r.sure[0]
    left = np.arange(TW)[None, :] < TW // 2
    assert not (obj & (r.labels[0] == 1) & ~left).any() and not (obj & (r.labels[0] == 2) & left).any()
    planes = [np.float32(r.zbuf[0][obj & (r.labels[0] == i + 1)].max() + 0.06) for i in range(2)]
    plane = np.broadcast_to(np.where(left, planes[0], planes[1]), (TH, TW))
    depth = np.where(obj, r.zbuf[0], plane).astype(np.float32)
    return dict(model=model, kps=C.dev(kps), mean_scales=inputs["obj_mean_scales"].cuda(), K=torch.as_tensor(K), depth=C.dev(depth),
                pose0=C.dev(pose), scale0=C.dev(scale), obj_labels=np.where(obj, r.labels[0], 0), plane=plane, depth_np=depth,
                pose_np=pose, scale_np=scale, K_np=K)


def _tracker(rig, **kw):
    from catre_amd import tracking

    tr = tracking.Tracker(rig["model"], rig["kps"], rig["K"], mean_scales=rig["mean_scales"], seed=11, **kw)
    return tr.reset(rig["pose0"], rig["scale0"])


def _same_step(a, b):
    for k in ("pose", "scale", "pose_iters", "status", "age", "pcl"):
        assert torch.equal(a[k], b[k]), k
    for f in ("d_obs", "inlier_obs", "d_prior"):
        assert torch.equal(getattr(a["score"], f), getattr(b["score"], f)), f


@pytest.mark.gpu
def test_tracker_render_crop(rig):
    from catre_amd import pcl_prep, render, tracking

    # on the CPU first: the ball around either object holds plane pixels, all of them more than crop_delta behind the object
    pts = backproject(np.where(rig["obj_labels"] == 0, rig["depth_np"], 0), rig["K_np"])
    for i in range(2):
        radius = max(0.5 * np.linalg.norm(rig["scale_np"][i]), 0.05) * 1.1       # cat_data_utils.py: ratio * |R s|, floor, growth
        assert (np.linalg.norm(pts - rig["pose_np"][i][:, 3], axis=1) <= 0.9 * radius).sum() > 20, i
    obj_z = rig["depth_np"][rig["obj_labels"] > 0]
    assert (rig["plane"][rig["obj_labels"] > 0] - obj_z > CROP["crop_delta"]).all() and (rig["obj_labels"] == 1).sum() > 50 < (rig["obj_labels"] == 2).sum()

    # the composition written out by hand
    pose, scale = rig["pose0"].clone(), rig["scale0"].clone()
    age = torch.zeros(2, dtype=torch.int32, device="cuda")
    Kd = rig["K"].cuda().expand(2, 3, 3).contiguous()
    depth = rig["depth"][None]
    want, pixs = [], []
    for t in range(2):
        sp = render.splat_prior(rig["kps"], pose, scale, rig["K"], (TH, TW), rho_rel=CROP["rho_rel"], r_max=CROP["r_max"], depth=depth,
                                delta=CROP["crop_delta"])
        pcl, pix, counts = pcl_prep.sample_frames(depth, rig["K"], [0, 0], pose, scale, labels=sp.labels_fit, label_of=[1, 2], ratio=0.5,
                                                  num_points=N_PTS, use_ball=True, sample="device", seed=11 + t, return_pixels=True)
        out = rig["model"].refine({"pcl": pcl, "obj_kps": rig["kps"], "obj_pose_est": pose, "obj_scale_est": scale, "K": Kd,
                                   "obj_mean_scales": rig["mean_scales"]}, n_iter=N_ITER)
        score = tracking.fit_score(pcl, rig["kps"], out[f"pose_{N_ITER}"], out[f"scale_{N_ITER}"], 0.1)
        pose, scale, status, age = tracking.track_gate(out[f"pose_{N_ITER}"], out[f"scale_{N_ITER}"], pose, scale, counts,
                                                       score.inlier_obs, score.d_obs, age, 0.0, True)
        want.append(dict(pose=pose, scale=scale, pose_iters=torch.stack([out[f"pose_{i}"] for i in range(N_ITER + 1)]), score=score,
                         status=status, age=age, pcl=pcl, splat_counts=sp.counts))
        pixs.append(pix)
    # frame 0 starts at the carried pose: every sampled pixel is one of the object's own
    pix0 = _np(pixs[0])
    assert (pix0 >= 0).all()
    for i in range(2):
        assert (rig["obj_labels"].reshape(-1)[pix0[i]] == i + 1).all(), i
    tr = _tracker(rig, crop="render", **CROP)
    torch.cuda.synchronize()
    grown = []
    for t in range(2):
        before = (render.abi_call_count(), pcl_prep.abi_call_count(), tracking.abi_call_count())
        got = tr.step(rig["depth"])
        grown.append((render.abi_call_count() - before[0], pcl_prep.abi_call_count() - before[1], tracking.abi_call_count() - before[2]))
        _same_step(got, want[t])
        assert torch.equal(got["splat_counts"], want[t]["splat_counts"]) and tuple(got["splat_counts"].shape) == (2, 5)
    assert grown[0] == grown[1] and grown[0][0] == 2 and grown[0][2] == 5, grown
    # the ball alone samples the plane as well, and is what a Tracker built without the keyword does
    ball, plain = _tracker(rig, crop="ball"), _tracker(rig)
    _, pixb, _ = pcl_prep.sample_frames(depth, rig["K"], [0, 0], rig["pose0"], rig["scale0"],
                                        labels=torch.zeros(1, TH, TW, dtype=torch.uint8, device="cuda"), label_of=[0, 0], ratio=0.5,
                                        num_points=N_PTS, use_ball=True, sample="device", seed=11, return_pixels=True)
    assert (rig["obj_labels"].reshape(-1)[_np(pixb)] == 0).any(1).all()
    for t in range(2):
        a, b = ball.step(rig["depth"]), plain.step(rig["depth"])
        _same_step(a, b)
        assert "splat_counts" not in a and "splat_counts" not in b
    assert not torch.equal(a["pcl"], got["pcl"])
