"""The mesh rasteriser without a GPU: the numpy restatement the GPU tests compare with (``tests/mesh_render_ref.py``) is
pinned on scenes whose answer is known analytically - the fill rule, watertightness, perspective-correct depth, the model
coordinates - and the host layer (``catre_amd.meshes``, the argument checks of ``render.render_mesh`` and
``pose_errors.vsd_mesh``, the parts of the C ABI that need no device) is checked."""
import ctypes
import os

import numpy as np
import pytest
import torch

from catre_amd import hip, meshes as MS, pose_errors, render
from tests import mesh_render_cases as C
from tests import mesh_render_ref as MREF
from tests.util import GOLDEN_DIR

NEW_SYMBOLS = ("catre_mesh_workspace_bytes", "catre_mesh_render")
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def _render(verts, faces, K, size=(48, 64), pc=0.0, pose=None, scale=None):
    pose = C.EYE[None] if pose is None else pose
    scale = np.ones((1, 3), np.float32) if scale is None else scale
    return MREF.render([(verts, faces)], [0], pose, scale, K[None], [0], 1, size, pixel_center=pc)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", (0.0, 0.5))
@pytest.mark.parametrize("diagonal", (0, 1))
@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("swap", (False, True))
def test_lattice_quad_covers_its_half_open_pixel_set(pc, diagonal, reverse, swap):
    """[8,24] x [8,16] px: exactly the 128 pixels [8,24) x [8,16), each once - top and left borders in, bottom and right out;
    at pixel_center 0.5 the same set, every sample strictly inside or on the diagonal"""
    K = C.lattice_K(3.0, -2.0)
    r, rec, _ = _render(*C.quad(diagonal, reverse, swap, K), K, pc=pc)
    assert rec[:, 3].all() and sorted(map(tuple, rec[:, :2].tolist())) == [(2048, 2048), (2048, 4096), (6144, 2048), (6144, 4096)]
    want = np.zeros((48, 64), np.int32)
    want[8:16, 8:24] = 1
    assert np.array_equal(r.cover[0], want) and np.array_equal(r.labels[0], want) and want.sum() == 128
    assert (r.zbuf[0][want == 1] == 1.0).all() and (r.zbuf[0][want == 0] == 0.0).all()
    assert r.counts.tolist() == [[128, 128, 0, 0, 0]] and r.culled.tolist() == [0]
    assert set(np.unique(r.face[0][want == 1])) == {0, 1} and (r.face[0][want == 0] == -1).all()


@pytest.mark.parametrize("pc", (0.0, 0.5))
def test_fan_vertex_on_a_sample_is_covered_once(pc):
    K = C.lattice_K()
    r, _, _ = _render(*C.fan((20 + pc, 14 + pc), K), K, pc=pc)
    assert r.cover[0, 14, 20] == 1 and r.cover.max() == 1 and r.cover.sum() > 100


@pytest.mark.parametrize("mesh", ("icosphere", "box"))
@pytest.mark.parametrize("pc", (0.0, 0.5))
def test_closed_meshes_cover_every_sample_an_even_number_of_times(mesh, pc):
    rng = np.random.default_rng(7)
    verts, faces = MS.icosphere(2, 0.5) if mesh == "icosphere" else MS.box_mesh((1.0, 0.7, 0.5))
    K = np.array([[70, 0, 31.5], [0, 70, 23.5], [0, 0, 1]], np.float32)
    r, rec, _ = _render(verts, faces, K, pc=pc, pose=C.random_pose(rng)[None], scale=np.float32([[0.3, 0.25, 0.35]]))
    assert rec[:, 3].all() and (r.cover % 2 == 0).all() and (r.cover == 2).sum() > 300 and r.culled.tolist() == [0]
    assert np.array_equal(r.labels > 0, r.cover > 0) and r.counts[0, 0] == (r.cover > 0).sum()


def _plane_depth(rec, tri, K, px, py, c):
    """fp64 ray-plane intersection: the plane through the three record points, the ray of the sample (px + c, py + c)"""
    P = []
    for k in tri:
        z = float(np.int32(rec[k, 2]).view(np.float32))
        P.append(z * np.array([(rec[k, 0] / 256 - K[0, 2]) / K[0, 0], (rec[k, 1] / 256 - K[1, 2]) / K[1, 1], 1.0]))
    n = np.cross(P[1] - P[0], P[2] - P[0])
    ray = np.array([(px + c - K[0, 2]) / K[0, 0], (py + c - K[1, 2]) / K[1, 1], 1.0])
    return float(n @ P[0]) / float(n @ ray)


@pytest.mark.parametrize("pc", (0.0, 0.5))
def test_depth_is_the_ray_plane_intersection(pc):
    K = C.lattice_K(2.0, 1.0).astype(np.float64)
    verts, faces = C.tilted_plane(K)
    r, rec, _ = _render(verts, faces, K.astype(np.float32), pc=pc)
    assert (rec[:, :2] % 256 == 0).all() and rec[:, 3].all()             # lattice vertices: snapping is exact
    ys, xs = np.nonzero(r.labels[0])
    assert len(ys) == 36 * 24 and (r.cover[0][ys, xs] == 1).all()
    worst = 0.0
    for py, px in zip(ys, xs):
        want = _plane_depth(rec, faces[r.face[0, py, px]], K, px, py, pc)
        worst = max(worst, abs(r.zd[0, py, px] - want) / want)
        assert r.zbuf[0, py, px] == np.float32(r.zd[0, py, px])          # one rounding to fp32
    print("depth vs ray-plane, worst relative", worst)
    assert worst <= 1e-12
    assert r.zbuf[0][ys, xs].min() < 0.8 * r.zbuf[0][ys, xs].max()       # it is tilted


def test_coords_round_trip():
    """With Y = R (s * coord) + t and X the back-projection of (px + c, py + c, zbuf): both are the same perspective-correct
    barycentric combination, b_k = w_k / W, of corner points - Y of the posed vertices P_k, X of the record points
    P'_k = z_k ray(xi_k / 256, yi_k / 256) - so |X - Y| <= max_k |P'_k - P_k|.  P'_k has the depth of P_k and its pixel position
    moved by the snap, at most 2^-9 px in u and in v: |P'_k - P_k| <= sqrt(2) 2^-9 z_k / f.  The facing angle does not enter,
    because both points are taken at the same barycentric coordinates; it would - as a factor tan(theta), at most sqrt(3) at the
    60 degrees kept here - were X compared with the true surface along the ray, so the scene keeps every drawn face within
    60 degrees of facing the camera and the test checks that it does.  On top: the record depth, zbuf and the three coord
    components are each one rounding to fp32, 4 * 2^-24 |P| in all.
    bound = sqrt(2) 2^-9 z_max / f + 2^-22 |P|_max."""
    rng = np.random.default_rng(11)
    K = np.array([[70, 0, 31.5], [0, 70, 23.5], [0, 0, 1]], np.float32)
    verts, faces = MS.grid_mesh(7, 5, (1.0, 0.8))
    verts[:, 2] = 0.1 * np.sin(3 * verts[:, 0]) * np.cos(2 * verts[:, 1])       # a curved sheet that faces the camera
    a = 0.35
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.diag([1.0, -1.0, -1.0])
    pose = np.concatenate([R, [[0.02], [-0.01], [0.7]]], 1).astype(np.float32)[None]
    scale = np.float32([[0.5, 0.45, 0.6]])
    for pc in (0.0, 0.5):
        r, rec, p = _render(verts, faces, K, pc=pc, pose=pose, scale=scale)
        P = MREF.REF.posed(verts[None], pose, scale)[0]
        tri = P[faces]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        cen = tri.mean(1)
        cosang = np.abs((n * cen).sum(1)) / np.linalg.norm(n, axis=1) / np.linalg.norm(cen, axis=1)
        assert np.degrees(np.arccos(cosang)).max() <= 60.0
        ys, xs = np.nonzero(r.labels[0])
        assert len(ys) > 500
        z = r.zbuf[0][ys, xs].astype(np.float64)
        X = np.stack([(xs + pc - K[0, 2]) / K[0, 0] * z, (ys + pc - K[1, 2]) / K[1, 1] * z, z], 1)
        co = r.coord[0][ys, xs].astype(np.float64)
        Y = (co * scale[0].astype(np.float64)) @ pose[0, :, :3].astype(np.float64).T + pose[0, :, 3].astype(np.float64)
        bound = np.sqrt(2) * 2.0 ** -9 * P[:, 2].max() / 70 + 2.0 ** -22 * np.linalg.norm(P, axis=1).max()
        err = np.linalg.norm(X - Y, axis=1).max()
        print("pixel_center", pc, "coords round trip: worst", err, "bound", bound)
        assert err <= bound
        assert (r.coord[0][r.labels[0] == 0] == 0).all()


def test_edge_scene_holds_its_edges():
    d = C.scene("edges")
    r, rec, _ = MREF.render(d["meshes"], d["mesh_of"], d["pose"], d["scale"], d["K"], d["frame_of"], d["F"], d["size"])
    assert rec[:, 3].tolist() == [1] * 6 + [0, 0] + [1] * 6 + [0, 0]                  # behind and ON the camera plane: not ok
    assert r.culled.tolist() == [4, 4]                       # two faces with a vertex that is not ok, two with a bad index
    assert set(np.unique(r.labels)) == {0, 1}                # the same coplanar faces: the lower instance wins all
    assert set(np.unique(r.face)) == {-1, 0}                 # duplicates (1: same winding, 9: reversed): the lower face wins
    assert r.cover.max() == 6 and r.counts[1].tolist() == [0] * 5        # three copies per instance; the sliver covers no sample
    t = C.scene("tiny")
    r, rec, _ = MREF.render(t["meshes"], t["mesh_of"], t["pose"], t["scale"], t["K"], t["frame_of"], t["F"], t["size"])
    assert (r.labels > 0).all() and (r.labels == 2).any() and (r.labels == 1).any() and r.counts[2, 0] == 0
    assert (r.cover >= 1).all() and r.counts[:, 0].sum() == 63


# ---- meshes --------------------------------------------------------------------------------------------------------------------
def test_load_obj(tmp_path):
    path = tmp_path / "m.obj"
    path.write_text("# a comment\no thing\nv 0 0 0\nv 1 0 0 0.5 0.5 0.5\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0 0\n"
                    "f 1 2 3 4\nv 0.5 0.5 1  # apex\nf -1/1/1 1/2/1 2//1\nf 2/7 3/8 5/9\ns off\nf 5 4 3 1 2\n")
    v, f = MS.load_obj(str(path))
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == (5, 3) and v[4].tolist() == [0.5, 0.5, 1.0]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [1, 2, 4], [4, 3, 2], [4, 2, 0], [4, 0, 1]]
    for bad in ("v 0 0 0\nf 1 2 3\n", "v 0 0\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n",
                "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 1 2\n", "vn 0 0 1\n"):
        path.write_text(bad)
        with pytest.raises(ValueError):
            MS.load_obj(str(path))


def test_makers_are_closed_and_wound_outwards():
    for (v, f), nv, nf in ((MS.box_mesh((1, 2, 3)), 8, 12), (MS.icosphere(0), 12, 20), (MS.icosphere(2), 162, 320),
                           (MS.icosphere(3, 0.5), 642, 1280)):
        assert v.shape == (nv, 3) and f.shape == (nf, 3) and v.dtype == np.float32 and f.dtype == np.int32
        tri = v[f].astype(np.float64)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert ((n * tri.mean(1)).sum(1) > 0).all()                                    # outwards
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert len(set(map(tuple, e.tolist()))) == len(e)                              # every directed edge once ...
        assert set(map(tuple, e.tolist())) == set(map(tuple, e[:, ::-1].tolist()))     # ... and its reverse once: closed
    assert np.allclose(np.linalg.norm(MS.icosphere(3, 0.5)[0], axis=1), 0.5, atol=1e-6)
    assert np.abs(MS.box_mesh((1, 2, 3))[0]).max(0).tolist() == [0.5, 1.0, 1.5]
    v, f = MS.grid_mesh(2, 2, (2.0, 2.0))
    assert v.shape == (9, 3) and f.shape == (8, 3) and v[4].tolist() == [0.0, 0.0, 0.0] and v[8].tolist() == [1.0, 1.0, 0.0]
    tri = v[f]
    assert (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])[:, 2] > 0).all()
    for bad in (lambda: MS.grid_mesh(0, 2), lambda: MS.icosphere(-1), lambda: MS.icosphere(8)):
        with pytest.raises(ValueError):
            bad()


def test_mesh_set_tables():
    a, b = MS.box_mesh(), MS.icosphere(1)
    ms = MS.MeshSet.from_list([a, b], "cpu", mesh_of=[1, 0, 1])
    assert (ms.n_meshes, ms.n_inst, ms.v_tot, ms.t_tot) == (2, 3, 8 + 42, 12 + 80)
    assert ms.vert_off.tolist() == [0, 8, 50] and ms.face_off.tolist() == [0, 12, 92] and ms.mesh_of.tolist() == [1, 0, 1]
    assert ms.verts.dtype == torch.float32 and ms.faces.dtype == ms.vert_off.dtype == ms.mesh_of.dtype == torch.int32
    assert np.array_equal(ms.verts[8:].numpy(), b[0]) and np.array_equal(ms.faces[12:].numpy(), b[1])    # local indices
    ivo, ifo = ms.instance_offsets()
    assert ivo.tolist() == [0, 42, 50, 92] and ifo.tolist() == [0, 80, 92, 172]
    assert np.array_equal(ivo, MREF.instance_offsets([a, b], [1, 0, 1])[0])
    assert MS.MeshSet.from_list([a, b], "cpu").mesh_of.tolist() == [0, 1]
    again = ms.with_mesh_of([0])
    assert again.verts is ms.verts and again.n_inst == 1 and again.instance_offsets()[1].tolist() == [0, 12]
    ok = MS.MeshSet.from_list([(torch.zeros(3, 3), torch.tensor([[0, 1, 7]]))], "cpu")      # indices are not checked here
    assert ok.t_tot == 1
    for bad in (dict(meshes=[]), dict(meshes=[a], mesh_of=[1]), dict(meshes=[a], mesh_of=[-1]), dict(meshes=[a], mesh_of=[]),
                dict(meshes=[(a[0][:, :2], a[1])]), dict(meshes=[(a[0], a[1][:, :2])]), dict(meshes=[(a[0], a[1].astype(np.float32))]),
                dict(meshes=[(a[0][:0], a[1])]), dict(meshes=[(a[0], a[1][:0])]), dict(meshes=[a[0]]), dict(meshes=[a], mesh_of="x")):
        with pytest.raises(ValueError):
            MS.MeshSet.from_list(bad["meshes"], "cpu", mesh_of=bad.get("mesh_of"))


# ---- host layer ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    lib = hip.load()
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "catre_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert n in hip.EXPORTED_SYMBOLS and hasattr(lib, n) and f"{n}(" in header, n


def test_bad_arguments_are_refused_without_a_device():
    lib = hip.load()
    buf = (ctypes.c_double * 64)()
    ok, nul = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    size = lib.catre_mesh_workspace_bytes
    assert size(0, 4, 4, 8) == 0 and size(1, 0, 4, 8) == 0 and size(1, 4, -1, 8) == 0 and size(1, 4, 4, 0) == 0
    assert size(1, 1 << 15, 1 << 15, 8) == 0
    assert size(1, 9, 7, 3) >= 63 * 8 + 3 * 16 + 4 * 4 + 3 * 4 and size(2, 48, 64, 100) >= size(1, 48, 64, 100) + 48 * 64 * 8
    assert size(1, 48, 64, 200) >= size(1, 48, 64, 100) + 100 * 16
    K = (ctypes.c_float * 18)(*([100, 0, 32, 0, 100, 24, 0, 0, 1] * 2))
    fo = (ctypes.c_int32 * 4)(0, 1, 1, 0)

    def call(tab=(ok,) * 9, depth=ok, K=K, fo=fo, delta=0.015, half=0, G=2, V=20, T=30, F=2, I=4, NV=40, NF=60, H=48, W=64,
             ws=ok, nbytes=1 << 30, req=(ok,) * 2, counts=ok, culled=ok, opt=(nul,) * 3, coord=nul, proj=nul):
        return lib.catre_mesh_render(*tab, depth, K, fo, delta, half, G, V, T, F, I, NV, NF, H, W, ws, nbytes, req[0], req[1],
                                     opt[0], opt[1], opt[2], counts, culled, coord, proj, nul)

    for k in range(9):               # verts, faces, vert_off, face_off, mesh_of, inst_vert_off, inst_face_off, pose, scale
        assert call(tab=tuple(nul if i == k else ok for i in range(9))) == BAD_ARG, k
    for kw in (dict(K=nul), dict(fo=nul), dict(req=(nul, ok)), dict(req=(ok, nul)), dict(counts=nul), dict(culled=nul), dict(G=0),
               dict(V=0), dict(T=0), dict(F=0), dict(I=0), dict(NV=3), dict(NF=3), dict(H=0), dict(W=-3), dict(H=1 << 15, W=1 << 15),
               dict(delta=float("nan")), dict(half=2), dict(half=-1), dict(fo=(ctypes.c_int32 * 4)(0, 2, 0, 0)), dict(F=1),
               dict(K=(ctypes.c_float * 18)(*([0.0] * 18)))):
        assert call(**kw) == BAD_ARG, kw
    assert call(nbytes=size(2, 48, 64, 40) - 1) == WORKSPACE and call(ws=nul) == WORKSPACE
    assert call(depth=nul, nbytes=0) == WORKSPACE                         # depth is optional: the next check is reached


def test_render_mesh_and_vsd_mesh_argument_checks():
    ms = MS.MeshSet.from_list([MS.box_mesh(), MS.icosphere(0)], "cpu")
    pose, scale, K = torch.zeros(2, 3, 4), torch.ones(2, 3), torch.eye(3)
    before = render.abi_call_count(), pose_errors.abi_call_count()
    ok = dict(meshes=ms, poses=pose, scales=scale, K=K, size=(48, 64))
    for kw in (dict(meshes=[MS.box_mesh()]), dict(meshes=None), dict(poses=torch.zeros(3, 3, 4)), dict(poses=torch.zeros(2, 4, 4)),
               dict(poses=None), dict(scales=torch.ones(2, 4)), dict(scales=None), dict(K=torch.eye(4)), dict(K=torch.zeros(2, 3, 3)),
               dict(size=(48,)), dict(size=(0, 64)), dict(size=48), dict(size=(1 << 15, 1 << 15)), dict(n_frames=0),
               dict(frame_of=[0]), dict(frame_of=[0, 1]), dict(frame_of=[0, -1]), dict(depth=torch.zeros(48, 65)),
               dict(depth=torch.zeros(2, 48, 64)), dict(depth="no tensor"), dict(pixel_center=0.25), dict(pixel_center=1),
               dict(pixel_center=None), dict(delta=float("nan"))):
        with pytest.raises(ValueError):
            render.render_mesh(**{**ok, **kw})
    with pytest.raises(hip.CatreHipError):                               # well-formed, but not on a device: no CPU fallback
        render.render_mesh(**ok)
    with pytest.raises(hip.CatreHipError):
        render.render_mesh(**ok, pixel_center=0.5, n_frames=2, frame_of=[1, 0], return_coords=True, return_projected=True)
    depth = torch.ones(48, 64)
    vok = dict(meshes=ms, pose_est=pose, scale_est=scale, pose_gt=pose, scale_gt=scale, K=K, depth_test=depth)
    for kw in (dict(meshes="x"), dict(pose_est=torch.zeros(3, 4)), dict(pose_gt=torch.zeros(3, 3, 4)), dict(scale_gt=torch.ones(2, 2)),
               dict(scale_est=None), dict(K=torch.eye(2)), dict(depth_test=torch.ones(48)), dict(origin=[[0, 0], [1, 1]]),
               dict(size=(0, 4)), dict(origin=[[0, 0]], size=(8, 8)), dict(frame_of=[0, 1]), dict(pixel_center=0.3),
               dict(taus=[]), dict(visib_mode="bop20"), dict(delta=float("nan"))):
        with pytest.raises(ValueError):
            pose_errors.vsd_mesh(**{**vok, **kw})
    with pytest.raises(hip.CatreHipError):
        pose_errors.vsd_mesh(**vok)
    assert (render.abi_call_count(), pose_errors.abi_call_count()) == before         # refused before any entry point is called
