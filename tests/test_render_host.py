"""The splat render without a GPU: the classes of ``tests/render_ref.py`` (the fp64 numpy restatement the GPU tests compare
with) against what the unmodified reference's ``lib/pysixd/visibility.py`` wrote into ``tests/golden/visib_mask.npz``
(``tools/make_render_golden.py``), its tie order and ``<=`` boundaries on a hand-made case, the parts of the C ABI that
need no device, the argument checks of ``catre_amd.render`` and ``Tracker(crop=...)``, and the CPU-side preconditions of the
GPU edge test: the cases hold the edges they claim, and at most 1 % of their rendered pixels are too close to call."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from catre_amd import hip
from tests import render_cases as C
from tests import render_ref as REF
from tests.util import GOLDEN_DIR

NEW_SYMBOLS = ("catre_splat_workspace_bytes", "catre_splat_render")
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "visib_mask.npz"))


def test_fixture_holds_the_threshold_pixels(gold):
    d_test, d_model, dl = gold["d_test"], gold["d_model"], gold["delta"]
    assert d_test.dtype == d_model.dtype == dl.dtype == np.float32 and d_test.shape == d_model.shape == (24, 32)
    assert (d_test == 0).any() and (d_model == 0).any() and ((d_test == 0) & (d_model > 0)).any()
    both = (d_test > 0) & (d_model > 0)
    diff = (d_model - d_test)[both]
    ulp = np.spacing(d_model[both])
    for t in (dl, -dl):
        assert (diff == t).sum() >= 32 and (diff == t + ulp).sum() >= 32 and (diff == t - ulp).sum() >= 32, t
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "visib_mask.npz")) < 16384


def test_restatement_classes_equal_the_reference_masks(gold):
    cls = REF.classes(gold["d_model"], gold["d_test"], gold["delta"])
    assert set(np.unique(cls)) == {REF.BACKGROUND, REF.AGREE, REF.OCCLUDED, REF.FREE, REF.HOLE}
    assert np.array_equal((cls == REF.AGREE) | (cls == REF.FREE), gold["bop18"])
    assert np.array_equal((cls == REF.AGREE) | (cls == REF.FREE) | (cls == REF.HOLE), gold["bop19"])
    assert np.array_equal(cls == REF.BACKGROUND, gold["d_model"] == 0)


def hand_case():
    """fx = fy = 1, cx = cy = 0: a point (x, y, z) lands on pixel (x / z, y / z).  Instance 0: points 0 and 1 coincide on pixel
    (3,3) at z = 1 (r = 2.5), point 2 sits on pixel (9,6) at z = 0.5 (r = 5) and covers part of their disc.  Instance 1
    repeats instance 0's point 0; its other points are outside the image."""
    kps = np.zeros((2, 3, 3), np.float32)
    kps[0] = [[3, 3, 1], [3, 3, 1], [4.5, 3, 0.5]]
    kps[1] = [[3, 3, 1], [40, 40, 1], [40, 40, 1]]
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None].repeat(2, 0).astype(np.float32)
    depth = np.full((1, 12, 16), 1.0, np.float32)
    # row 3, u = 1..5 (zbuf 1, 1, 1, 1, 0.5): just behind +delta, on -delta, on +delta, a hole, just beyond -delta
    depth[0, 3, 1:6] = [0.75 - 2.0 ** -20, 1.25, 0.75, 0.0, 0.75 + 2.0 ** -20]
    return dict(kps=kps, pose=eye, scale=np.ones((2, 3), np.float32), rho=np.array([2.5, 2.5]), K=np.eye(3, dtype=np.float32)[None],
                depth=depth, delta=0.25, r_max=100.0, size=(12, 16))


def test_restatement_ties_and_boundaries():
    h = hand_case()
    r = REF.render(h["kps"], h["pose"], h["scale"], h["rho"], h["K"], [0, 0], 1, h["size"], h["r_max"], depth=h["depth"],
                   delta=h["delta"])
    # the near disc, r = 5 about (9,6): (4,6) and (6,2) [3-4-5] are ON the circle and inside, (14,10) is outside
    assert r.labels[0, 6, 4] == 1 and r.labels[0, 2, 6] == 1 and r.point[0, 2, 6] == 2 and r.labels[0, 10, 14] == 0
    assert r.point[0, 3, 3] == 0 and r.zbuf[0, 3, 3] == 1.0                # lower m on a tie
    assert r.point[0, 3, 5] == 2 and r.zbuf[0, 3, 5] == 0.5                # (5,3) is on the near circle: the nearer point wins
    assert (r.labels <= 1).all() and r.counts[1].tolist() == [0] * 5       # lower i on a tie: instance 1 wins nothing
    assert r.cls[0, 3, 1:6].tolist() == [REF.OCCLUDED, REF.AGREE, REF.AGREE, REF.HOLE, REF.FREE]
    assert r.labels_fit[0, 3, 1:6].tolist() == [0, 1, 1, 0, 0] and r.counts[0, 0] == r.counts[0, 1:].sum() == (r.labels == 1).sum()
    zb, d = np.float32([1, 1, 1, 1, 1, 1]), np.float32([0.75, 1.25, 0.75 - 2.0 ** -20, 1.25 + 2.0 ** -20, 0, -1])
    assert REF.classes(zb, d, 0.25).tolist() == [REF.AGREE, REF.AGREE, REF.OCCLUDED, REF.FREE, REF.HOLE, REF.HOLE]
    assert REF.classes(np.float32([0]), np.float32([1]), 0.25).tolist() == [REF.BACKGROUND]
    # the coinciding points are both the surface of their pixel; instance 1's copy is not: the pixel is instance 0's
    assert r.visible[0].tolist() == [True, True, True] and not r.visible[1].any()
    moved = dict(h, depth=np.where(np.arange(16) == 3, np.float32(0.5), h["depth"]))     # something in front of pixel (3,3)
    r2 = REF.render(moved["kps"], h["pose"], h["scale"], h["rho"], h["K"], [0, 0], 1, h["size"], h["r_max"], depth=moved["depth"],
                    delta=h["delta"])
    assert r2.visible[0].tolist() == [False, False, True] and r2.cls[0, 3, 3] == REF.OCCLUDED
    assert not r.sure[0, 6, 4] and not r.sure[0, 3, 5] and not r.sure[0, 3, 3]     # on a circle; two points at one depth
    assert r.sure[0, 6, 9] and r.sure[0, 10, 14]                                   # interior, background


def test_new_symbols_are_declared_and_exported():
    lib = hip.load()
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "catre_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert n in hip.EXPORTED_SYMBOLS and hasattr(lib, n) and f"{n}(" in header, n
    for k, v in dict(BACKGROUND=0, AGREE=1, OCCLUDED=2, FREE=3, HOLE=4).items():
        assert f"CATRE_SPLAT_{k} = {v}" in header, k
    from catre_amd import render
    assert (render.BACKGROUND, render.AGREE, render.OCCLUDED, render.FREE, render.HOLE) == (0, 1, 2, 3, 4)
    assert (REF.BACKGROUND, REF.AGREE, REF.OCCLUDED, REF.FREE, REF.HOLE) == (0, 1, 2, 3, 4)


def test_bad_arguments_are_refused_without_a_device():
    lib = hip.load()
    buf = (ctypes.c_double * 64)()
    ok, nul = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    size = lib.catre_splat_workspace_bytes
    assert size(0, 4, 4) == 0 and size(1, 0, 4) == 0 and size(1, 4, -1) == 0 and size(-1, 4, 4) == 0
    assert size(1, 1 << 15, 1 << 15) == 0 and size(4, 1 << 14, 1 << 14) == 0 and size(1 << 10, 1 << 10, 1 << 10) == 0
    assert size(1, 1, 1) > 0 and size(2, 48, 64) >= size(1, 48, 64) + 48 * 64 * 8 and size(3, 1 << 14, 1 << 14) > 0
    K = (ctypes.c_float * 18)(*([100, 0, 32, 0, 100, 24, 0, 0, 1] * 2))
    fo = (ctypes.c_int32 * 4)(0, 1, 1, 0)
    big = (ctypes.c_int32 * 70000)()

    def splat(inp=(ok,) * 4, depth=ok, K=K, fo=fo, r_max=8.0, delta=0.015, F=2, I=4, M=8, H=48, W=64, ws=ok, nbytes=1 << 30,
              req=(ok,) * 2, counts=ok, opt=(nul,) * 3, vis=nul):
        return lib.catre_splat_render(*inp, depth, K, fo, r_max, delta, F, I, M, H, W, ws, nbytes, req[0], req[1], opt[0], opt[1],
                                      opt[2], counts, vis, nul)

    for k in range(4):                                                   # kps, pose, scale, rho
        assert splat(inp=tuple(nul if i == k else ok for i in range(4))) == BAD_ARG, k
    for kw in (dict(K=nul), dict(fo=nul), dict(req=(nul, ok)), dict(req=(ok, nul)), dict(counts=nul), dict(F=0), dict(I=0),
               dict(M=0), dict(H=0), dict(W=-3), dict(I=-1), dict(H=1 << 15, W=1 << 15), dict(F=1 << 10, H=1 << 10, W=1 << 10),
               dict(r_max=-1.0), dict(r_max=float("nan")), dict(delta=float("nan")),
               dict(fo=(ctypes.c_int32 * 4)(0, 2, 0, 0)), dict(fo=(ctypes.c_int32 * 4)(0, 0, -1, 0)), dict(F=1),
               dict(K=(ctypes.c_float * 18)(*([0.0] * 18))), dict(K=(ctypes.c_float * 18)(*([float("nan")] * 18)))):
        assert splat(**kw) == BAD_ARG, kw
    assert splat(I=65536, fo=big) == UNSUPPORTED and splat(M=65537) == UNSUPPORTED
    assert splat(nbytes=size(2, 48, 64) - 1) == WORKSPACE and splat(nbytes=0) == WORKSPACE and splat(ws=nul) == WORKSPACE
    assert splat(depth=nul, nbytes=0) == WORKSPACE                        # depth is optional: the next check is reached


def test_splat_prior_argument_checks():
    from catre_amd import render

    kps, pose, scale, K = torch.zeros(2, 8, 3), torch.zeros(2, 3, 4), torch.ones(2, 3), torch.eye(3)
    before = render.abi_call_count()
    ok = dict(kps=kps, poses=pose, scales=scale, K=K, size=(48, 64))
    for kw in (dict(kps=torch.zeros(8, 3)), dict(kps=torch.zeros(2, 8, 4)), dict(kps=torch.zeros(0, 8, 3)), dict(kps="no tensor"),
               dict(poses=torch.zeros(2, 4, 4)), dict(poses=None), dict(scales=torch.ones(3, 3)), dict(scales=None),
               dict(K=torch.eye(4)), dict(K=torch.zeros(2, 3, 3)), dict(size=(48,)), dict(size=(0, 64)), dict(size=48),
               dict(n_frames=0), dict(frame_of=[0]), dict(frame_of=[0, 1]), dict(frame_of=[0, -1]),
               dict(depth=torch.zeros(48, 65)), dict(depth=torch.zeros(2, 48, 64)), dict(depth="no tensor"),
               dict(kps=torch.zeros(1, 65537, 3), poses=pose[:1], scales=scale[:1])):
        with pytest.raises(ValueError):
            render.splat_prior(**{**ok, **kw})
    with pytest.raises(ValueError):
        render.splat_prior(**ok, n_frames=2, frame_of=[0, 1], depth=torch.zeros(48, 64))
    with pytest.raises(ValueError):
        render.fit_score_visible(kps, kps, pose, scale, K, torch.zeros(2, 48, 64))
    with pytest.raises(hip.CatreHipError):                               # well-formed, but not on a device: no CPU fallback
        render.splat_prior(**ok)
    assert render.abi_call_count() == before                             # refused before any entry point is called


def test_tracker_crop_argument_checks():
    from catre_amd import tracking
    from catre_amd.config import default_cfg

    model = types.SimpleNamespace(cfg=default_cfg(num_pcl=64, num_kps=64, n_iter=2, device="cpu"))
    kps, K = torch.zeros(2, 64, 3), torch.eye(3)
    with pytest.raises(ValueError, match="crop"):
        tracking.Tracker(model, kps, K, crop="mesh")
    assert tracking.Tracker(model, kps, K).crop == "ball"
    tr = tracking.Tracker(model, kps, K, crop="render")
    assert (tr.crop, tr.crop_delta) == ("render", 0.05)
    tr.reset(torch.zeros(2, 3, 4), torch.ones(2, 3))
    depth = torch.ones(48, 64)
    masks, labels = torch.ones(2, 48, 64, dtype=torch.bool), torch.zeros(48, 64, dtype=torch.uint8)
    for kw in (dict(masks=masks), dict(labels=labels, label_of=[0, 0]), dict(labels=labels), dict(label_of=[1, 2])):
        with pytest.raises(ValueError, match="render"):
            tr.step(depth, **kw)
    with pytest.raises(hip.CatreHipError):                               # reaches the render, which needs the device
        tr.step(depth)


@pytest.mark.parametrize("name", C.EDGE_CASES)
def test_edge_cases_hold_their_edges_and_are_sure(name):
    d, r = C.edge_data(name), C.edge_reference(name)
    rendered = r.labels > 0
    unsure = int((~r.sure & rendered).sum())
    print(name, "rendered", int(rendered.sum()), "non-sure", unsure, "non-sure points", int((~r.vis_sure).sum()))
    assert rendered.sum() > 400 and unsure <= 0.01 * rendered.sum()
    assert (~r.vis_sure).sum() <= 0.02 * r.vis_sure.size
    _, _, _, rad, drawn, *_ = REF.project(d["kps"], d["pose"], d["scale"], C.rho_of(d["scale"]), d["K"], d["frame_of"], d["r_max"])
    assert (rad[drawn] == d["r_max"]).any() and (rad[drawn] < d["r_max"]).any()
    assert set(np.unique(r.cls)) == {0, 1, 2, 3, 4} and r.visible.any()
    if name == C.EDGE_CASES[0]:
        assert rendered[:, :, 0].any() and rendered[:, 0, :].any()       # clipped left and top
        assert drawn.sum(1).tolist() == [63, 0, 0]                       # a NaN point and one behind; behind the camera; NaN pose
        assert r.counts[1:].sum() == 0
    else:
        assert rendered[:, :, -1].any() and rendered[:, -1, :].any()     # clipped right and bottom
        assert (rad[0] < 0.5).sum() > 20 and drawn[1].all() and r.counts[1].sum() == 0    # wholly outside the image
        assert not rendered[0].any() and rendered[1].any()               # frame_of = [1, 0]
