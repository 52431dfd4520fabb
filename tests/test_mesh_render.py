"""The mesh rasteriser on the GPU (``render.render_mesh``, ``csrc/catre_mesh.h``) against ``tests/mesh_render_ref.py``.

Stage 1 - the vertex records - is fp32 on the device: compared with the fp64 restatement within the per-vertex bounds of
``tests/render_ref.project`` (derived in ``tests/test_render.py``), every vertex.  Stage 2 - everything after the records - is
integer and IEEE fp64 arithmetic in a fixed order: given the device's own records, every output equals the restatement's bit
for bit, on every pixel."""
import numpy as np
import pytest
import torch

from catre_amd import meshes as MS
from catre_amd import pose_errors, render
from tests import mesh_render_cases as C
from tests import mesh_render_ref as MREF

pytestmark = pytest.mark.gpu
DELTA = 0.015


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _run(d, pc=0.0, depth=None, meshes=None, **kw):
    ms = MS.MeshSet.from_list(d["meshes"] if meshes is None else meshes, "cuda", mesh_of=d["mesh_of"])
    out = render.render_mesh(ms, _cuda(d["pose"]), _cuda(d["scale"]), d["K"], d["size"], frame_of=d["frame_of"], n_frames=d["F"],
                             depth=None if depth is None else _cuda(depth), delta=DELTA, pixel_center=pc, return_coords=True,
                             return_projected=True, **kw)
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _assert_stage2(out, d, pc, depth=None, meshes=None):
    ref = MREF.raster(out.projected.cpu().numpy(), d["meshes"] if meshes is None else meshes, d["mesh_of"], d["frame_of"], d["F"],
                      d["size"], pc, depth, DELTA)
    for name in ("labels", "face", "cls", "labels_fit", "counts", "culled"):
        got = getattr(out, name).cpu().numpy()
        assert got.shape == getattr(ref, name).shape and np.array_equal(got, getattr(ref, name)), name
    assert np.array_equal(_bits(out.zbuf), ref.zbuf.view(np.int32))
    assert np.array_equal(_bits(out.coord), ref.coord.view(np.int32))
    return ref


@pytest.mark.parametrize("name", C.SCENES)
def test_stage1_records_against_fp64(name):
    d = C.scene(name)
    rec = _run(d).projected.cpu().numpy()
    p = MREF.project(d["meshes"], d["mesh_of"], d["pose"], d["scale"], d["K"], d["frame_of"])
    x, y, yes, no = MREF.snapped(p)
    assert rec.shape == (len(x), 4) and set(np.unique(rec[:, 3])) <= {0, 1}
    ok = rec[:, 3] == 1
    assert ok[yes].all() and not ok[no].any()
    assert yes.sum() >= 3 and (name != "edges" or no.sum() == 4)
    with np.errstate(all="ignore"):
        assert (np.abs(rec[ok, 0] - x[ok]) <= 0.5 + 256 * p.eu[ok]).all() and (np.abs(rec[ok, 1] - y[ok]) <= 0.5 + 256 * p.ev[ok]).all()
    assert (rec[~ok, :2] == 0).all()
    z = rec[:, 2].copy().view(np.float32).astype(np.float64)
    assert (np.abs(z - p.z) <= p.ez).all()
    print(name, "vertices", len(x), "ok", int(ok.sum()), "worst |xi - 256 u| / bound",
          float((np.abs(rec[ok, 0] - x[ok]) / (0.5 + 256 * p.eu[ok])).max()))


@pytest.mark.parametrize("pc", (0.0, 0.5))
@pytest.mark.parametrize("name", C.SCENES)
def test_stage2_is_bit_exact(name, pc):
    d = C.scene(name)
    plain = _run(d, pc)
    ref = _assert_stage2(plain, d, pc)
    assert (ref.labels > 0).any()
    depth = C.observed(ref.zbuf, DELTA, np.random.default_rng(3))
    seen = _run(d, pc, depth=depth)
    ref2 = _assert_stage2(seen, d, pc, depth=depth)
    if name != "tiny":
        assert set(np.unique(ref2.cls)) == {0, 1, 2, 3, 4}
    assert np.array_equal(_bits(seen.zbuf), _bits(plain.zbuf)) and torch.equal(seen.labels, plain.labels)
    # either winding draws the same image
    flipped = [(v, f[:, ::-1].copy()) for v, f in d["meshes"]]
    rev = _run(d, pc, meshes=flipped)
    _assert_stage2(rev, d, pc, meshes=flipped)
    for a in ("labels", "face", "counts", "culled"):
        assert torch.equal(getattr(rev, a), getattr(plain, a)), a
    assert np.array_equal(_bits(rev.zbuf), _bits(plain.zbuf))


def test_scenes_hold_what_they_claim_on_the_device():
    e = _run(C.scene("edges"))
    assert e.culled.tolist() == [4, 4] and set(e.labels.unique().tolist()) == {0, 1} and set(e.face.unique().tolist()) == {-1, 0}
    t = _run(C.scene("tiny"))
    assert (t.labels > 0).all() and t.counts[:, 0].tolist()[2] == 0 and set(t.labels.unique().tolist()) == {1, 2}
    c = _run(C.scene("counts"))
    assert (c.counts[:, 0] > 0).all() and c.culled.tolist() == [0] * 5


@pytest.mark.parametrize("pc", (0.0, 0.5))
def test_lattice_quad_on_the_device(pc):
    K = C.lattice_K(3.0, -2.0)
    want = np.zeros((48, 64), np.int32)
    want[8:16, 8:24] = 1
    for diagonal in (0, 1):
        for reverse in (False, True):
            for swap in (False, True):
                d = dict(meshes=[C.quad(diagonal, reverse, swap, K)], mesh_of=[0], pose=C.EYE[None], scale=np.ones((1, 3), np.float32),
                         K=K[None], frame_of=[0], F=1, size=(48, 64))
                out = _run(d, pc)
                assert np.array_equal(out.labels[0].cpu().numpy(), want), (diagonal, reverse, swap)
                assert (out.zbuf[0].cpu().numpy() == want.astype(np.float32)).all() and out.counts.tolist() == [[128, 128, 0, 0, 0]]
                assert out.projected[:, 3].all() and (out.projected[:, :2] % 256 == 0).all()


def test_frames_together_equal_frames_one_by_one_and_calls_repeat():
    d = C.scene("shared")
    both = _run(d, 0.5)
    again = _run(d, 0.5)
    for a in ("labels", "face", "cls", "labels_fit", "counts", "culled", "projected"):
        assert torch.equal(getattr(both, a), getattr(again, a)), a
    assert np.array_equal(_bits(both.zbuf), _bits(again.zbuf)) and np.array_equal(_bits(both.coord), _bits(again.coord))
    for f in range(d["F"]):
        mine = [i for i, g in enumerate(d["frame_of"]) if g == f]
        one = dict(d, mesh_of=[d["mesh_of"][i] for i in mine], pose=d["pose"][mine], scale=d["scale"][mine], K=d["K"][f:f + 1],
                   frame_of=[0] * len(mine), F=1)
        alone = _run(one, 0.5)
        lab = torch.tensor([0] + [i + 1 for i in mine], dtype=torch.int32).cuda()[alone.labels[0].long()]
        assert torch.equal(lab, both.labels[f]) and torch.equal(alone.face[0], both.face[f])
        assert np.array_equal(_bits(alone.zbuf[0]), _bits(both.zbuf[f])) and np.array_equal(_bits(alone.coord[0]), _bits(both.coord[f]))
        assert torch.equal(alone.counts, both.counts[mine]) and (lab > 0).any()


def test_permuting_faces_changes_neither_labels_nor_depth():
    d = C.scene("shared")
    base = _run(d)
    rng = np.random.default_rng(5)
    perm = [(v, f[rng.permutation(len(f))]) for v, f in d["meshes"]]
    out = _run(d, meshes=perm)
    assert torch.equal(out.labels, base.labels) and np.array_equal(_bits(out.zbuf), _bits(base.zbuf))
    assert not torch.equal(out.face, base.face) and torch.equal(out.counts, base.counts)


def test_vsd_mesh_is_its_composition_and_zero_at_the_ground_truth():
    rng = np.random.default_rng(9)
    I, size = 3, (48, 64)
    K = np.array([[70, 0, 31.5], [0, 70, 23.5], [0, 0, 1]], np.float32)
    ms = MS.MeshSet.from_list([MS.box_mesh((1.0, 0.7, 0.5)), MS.icosphere(2, 0.5)], "cuda", mesh_of=[0, 1, 0])
    pose_gt = np.stack([C.random_pose(rng) for _ in range(I)])
    pose_est = pose_gt.copy()
    pose_est[:, :, 3] += rng.normal(0, 0.01, (I, 3)).astype(np.float32)
    scale = rng.uniform(0.2, 0.3, (I, 3)).astype(np.float32)
    pe, pg, s = _cuda(pose_est), _cuda(pose_gt), _cuda(scale)
    own = list(range(I))
    # the scene every instance is seen in: all three rendered into one frame
    scene = render.render_mesh(ms, pg, s, K, size)
    depth_test = scene.zbuf[0].contiguous()
    errors, counts = pose_errors.vsd_mesh(ms, pe, s, pg, s, K, depth_test, delta=DELTA)
    est = render.render_mesh(ms, pe, s, K, size, frame_of=own, n_frames=I)
    gt = render.render_mesh(ms, pg, s, K, size, frame_of=own, n_frames=I)
    e2, c2 = pose_errors.vsd(est.zbuf, gt.zbuf, depth_test, torch.as_tensor(K), delta=DELTA)
    assert torch.equal(counts, c2) and np.array_equal(errors.cpu().numpy().view(np.int64), e2.cpu().numpy().view(np.int64))
    assert (errors > 0).any() and (counts[:, 0] > 0).all()
    # a box at its ground-truth pose against its own rendered depth: every error is 0
    box = ms.with_mesh_of([0])
    mine = render.render_mesh(box, pg[:1], s[:1], K, size)
    e0, c0 = pose_errors.vsd_mesh(box, pg[:1], s[:1], pg[:1], s[:1], K, mine.zbuf[0].contiguous(), delta=DELTA)
    assert (e0 == 0).all() and c0[0, 0] == c0[0, 1] == mine.counts[0, 0] > 100 and (c0[0, 2:] == 0).all()
    # a window of the frame
    o = [[8, 4]]
    ew, cw = pose_errors.vsd_mesh(box, pg[:1], s[:1], pg[:1], s[:1], K, mine.zbuf[0].contiguous(), origin=o, size=(40, 48), delta=DELTA)
    assert (ew == 0).all() and 0 < cw[0, 0] <= c0[0, 0]
