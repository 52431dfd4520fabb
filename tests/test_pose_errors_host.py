"""Host side of the BOP pose errors (``catre_amd/pose_errors.py``): the restatement ``tests/pose_errors_ref.py`` against the
reference's own numbers (``tests/golden/pose_error_bop.npz``, written by ``tools/make_pose_error_golden.py`` from the unmodified
``lib/pysixd``), the host functions of the module, the argument checks, and - on the CPU - the preconditions of the GPU tests
(``tests/test_pose_errors.py``)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from catre_amd import hip, pose_errors
from tests import pose_errors_cases as C
from tests import pose_errors_ref as REF
from tests.util import GOLDEN_DIR

BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
NEW_SYMBOLS = ("catre_sym_err_workspace_bytes", "catre_sym_err", "catre_vsd")


@pytest.fixture(scope="module")
def gold():
    return C.golden()


# ---- the restatement and the module's host functions against the reference ---------------------------------------------------
def test_symmetry_sets_equal_the_reference(gold):
    infos = json.loads(str(gold["model_infos"]))
    step = C.golden_meta(gold)["step"]
    sizes = []
    for k, info in enumerate(infos):
        want = gold[f"info{k}/syms"]
        for got in (REF.symmetry_transforms(info, step), pose_errors.symmetry_transforms(info, step)):
            assert got.shape == want.shape and got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12, k
        sizes.append(len(want))
    assert sizes == [1, 3, 314, 628]
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    for k, has in enumerate((True, True, False, False)):       # with a continuous symmetry the identity is NOT in the list
        assert any(np.array_equal(t, eye) for t in pose_errors.symmetry_transforms(infos[k], step)) == has, k
        assert any(np.abs(t - eye).max() < 1e-9 for t in gold[f"info{k}/syms"]) == has, k
    assert np.abs(gold["info2/syms"][:, :, 3]).max() > 0.01                           # the offset axis moves the origin
    want = gold["axis_y/syms"]
    for got in (REF.axis_symmetry_transforms([0, 1, 0], step), pose_errors.axis_symmetry_transforms([0, 1, 0], step)):
        assert got.shape == want.shape == (314, 3, 4) and np.abs(got - want).max() <= 1e-12
    assert pose_errors.symmetry_transforms(infos[2]).shape == (314, 3, 4)              # the default step is the config's 0.01
    # the loader-shaped set of the benchmark: 313 turns by 2 pi / 314
    from catre_amd import synth

    assert np.abs(gold["sets/y314"][1:, :, :3] - synth.y_axis_symmetries(314)).max() <= 1e-6 and len(gold["sets/y314"]) == 314


def test_restatement_point_errors_equal_the_reference(gold):
    cases = C.golden_meta(gold)["sym_cases"]
    assert sorted({c["n"] for c in cases}) == [1, 63, 64, 65, 257] and {c["set"] for c in cases} == {"one", "two", "y314"}
    for j, c in enumerate(cases):
        g = lambda k: gold[f"s{j}/{k}"]
        syms = gold[f"sets/{c['set']}"]
        r = REF.sym_errors(np.hstack([g("R_est"), g("t_est").reshape(3, 1)]), np.hstack([g("R_gt"), g("t_gt").reshape(3, 1)]),
                           g("pts"), g("K"), syms)
        for k, name in enumerate(("mssd", "mspd", "proj")):
            assert abs(r.err[k] - float(g(name))) <= 1e-12, (j, name, r.err[k], float(g(name)))
        if len(syms) > 1:                                        # the estimate stands off a non-identity member
            assert (r.best > 0).all(), (j, r.best)
        for a in ("pts", "R_est", "t_est", "R_gt", "t_gt", "K"):
            assert g(a).dtype == np.float32, (j, a)


def _vsd_case(gold, j, c):
    return REF.vsd(gold[f"v{j}/d_est"], gold[f"v{j}/d_gt"], gold[f"v{j}/d_test"], gold["vsd/K"], float(gold["vsd/delta"]),
                   gold["vsd/taus"], float(gold["vsd/diameter"]) if c["normalized"] else None, visib_mode=c["mode"])


def test_restatement_vsd_equals_the_reference_exactly(gold):
    cases = C.golden_meta(gold)["vsd_cases"]
    assert {(c["mode"], c["normalized"]) for c in cases} == {(m, n) for m in ("bop19", "bop18") for n in (False, True)}
    for j, c in enumerate(cases):
        r = _vsd_case(gold, j, c)
        assert np.array_equal(r.counts, gold[f"v{j}/counts"]), (j, r.counts, gold[f"v{j}/counts"])
        assert np.array_equal(r.errors, gold[f"v{j}/errors"]), (j, r.errors, gold[f"v{j}/errors"])
        if c["empty"]:
            assert r.counts[0] == 0 and (r.errors == 1.0).all()
    assert any(c["empty"] for c in cases)


def test_vsd_fixture_holds_its_threshold_pixels(gold):
    """the edges the fixture claims: pixels on delta and one fp32 step to either side, for either render; pixels on a tau"""
    cases = C.golden_meta(gold)["vsd_cases"]
    dl, taus, diam = np.float32(gold["vsd/delta"]), gold["vsd/taus"], float(gold["vsd/diameter"])
    for j, c in enumerate(cases):
        if c["empty"]:
            continue
        r = _vsd_case(gold, j, c)
        t32 = r.dist_test.astype(np.float32)
        for row, dist, mask in ((5, r.dist_gt, r.vis_gt), (15, r.dist_est, r.vis_est)):
            diff = dist.astype(np.float32)[row:row + 3] - t32[row:row + 3]
            assert (diff[0] == dl).all() and (diff[1] > dl).all() and (diff[2] < dl).all(), (j, row)
            step = np.spacing(dist.astype(np.float32)[row])
            assert (diff[1] - dl <= 2 * step).all() and (dl - diff[2] <= 2 * step).all(), (j, row)   # the neighbouring values
            assert mask[row].all() and not mask[row + 1].any() and mask[row + 2].all(), (j, row)
        inter = r.vis_gt & r.vis_est
        d = np.abs(r.dist_gt - r.dist_est) / (diam if c["normalized"] else 1.0)
        on = [int(((d == t) & inter).sum()) for t in taus]
        assert sum(n > 0 for n in on) >= 3 and sum(on) >= 6, (j, on)
        assert ((r.dist_test == 0) & (r.dist_gt > 0)).any() and r.counts[0] > r.counts[1] > 0


# ---- SymSets --------------------------------------------------------------------------------------------------------------------
def test_symsets_identity_and_padding():
    from catre_amd import losses, synth

    rot = synth.y_axis_symmetries(6)                                       # [5,3,3], no identity
    eye34 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    full = pose_errors.symmetry_transforms({"symmetries_discrete": [[-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]]})  # leads with I
    s = pose_errors.SymSets.from_list([None, rot, full, torch.as_tensor(rot)], "cpu")
    assert s.sizes == (1, 6, 2, 6) and s.s_max == 6 and s.s_tot == 15 and s.n_sets == 4 and s.n_inst == 4
    assert s.sym_off.tolist() == [0, 1, 7, 9, 15] and s.sym_of.tolist() == [0, 1, 2, 3]
    assert s.syms.dtype == torch.float32 and tuple(s.syms.shape) == (15, 3, 4) and s.sym_off.dtype == s.sym_of.dtype == torch.int32
    for g in range(4):
        assert np.array_equal(s.host[g][0], eye34), g                       # the identity first ...
    assert np.array_equal(s.host[2], full.astype(np.float32))               # ... and not twice where the list leads with it
    assert np.array_equal(s.host[1][1:, :, :3], rot) and not s.host[1][:, :, 3].any()
    cands, valid = s.padded()
    assert cands.shape == (4, 6, 3, 4) and valid.sum(1).tolist() == [1, 6, 2, 6]
    assert np.array_equal(cands[0, 3], eye34) and np.array_equal(cands[2, 5], eye34)
    # the same candidates, in the same order, as the loss's table of the same list
    lc, lv, _ = losses._sym_tensor([None, rot], "cpu", torch.float32)
    assert np.array_equal(lc.numpy(), cands[:2, :, :, :3]) and np.array_equal(lv.numpy().astype(bool), valid[:2])
    shared = pose_errors.SymSets.from_list([None, rot], "cpu", sym_of=[1, 0, 1, 1, 0])
    assert shared.n_inst == 5 and shared.sym_of.tolist() == [1, 0, 1, 1, 0] and shared.n_sets == 2
    for bad in (dict(sym_infos=[]), dict(sym_infos=[np.zeros((2, 4, 4))]), dict(sym_infos=[np.zeros((3, 3))]),
                dict(sym_infos=[None], sym_of=[1]), dict(sym_infos=[None], sym_of=[-1]), dict(sym_infos=[None], sym_of=["a"])):
        with pytest.raises(ValueError):
            pose_errors.SymSets.from_list(bad["sym_infos"], "cpu", sym_of=bad.get("sym_of"))


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    lib = hip.load()
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "catre_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert n in hip.EXPORTED_SYMBOLS and hasattr(lib, n) and f"{n}(" in header, n
    assert "CATRE_VSD_BOP19 = 0, CATRE_VSD_BOP18 = 1, CATRE_VSD_MAX_TAUS = 16" in header
    assert (pose_errors.BOP19, pose_errors.BOP18, pose_errors.MAX_TAUS) == (0, 1, 16)
    assert set(pose_errors.ABI_CALLS) == set(NEW_SYMBOLS)
    assert len(pose_errors.DEFAULT_TAUS) == 10 and pose_errors.DEFAULT_TAUS[0] == 0.05 and pose_errors.DEFAULT_TAUS[-1] == 0.5


def test_bad_arguments_are_refused_without_a_device():
    lib = hip.load()
    buf = (ctypes.c_double * 64)()
    ok, nul = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    size = lib.catre_sym_err_workspace_bytes
    assert size(0, 4) == 0 and size(4, 0) == 0 and size(-1, 4) == 0 and size(1 << 30, 1 << 30) == 0
    assert size(1, 1) > 0 and size(256, 314) >= 3 * 256 * 314 * 4

    def sym(ptrs=(ok,) * 3, scales=(nul, nul), tabs=(ok,) * 4, n=8, G=2, S_tot=9, S_max=8, I=4, ws=ok, nbytes=1 << 30,
            out=(ok, ok), tables=nul, shared=0):
        return lib.catre_sym_err(ptrs[0], shared, n, ptrs[1], ptrs[2], scales[0], scales[1], *tabs, G, S_tot, S_max, I, ws, nbytes,
                                 out[0], out[1], tables, nul)

    for k in range(3):                                                   # pts, pose_est, pose_gt
        assert sym(ptrs=tuple(nul if i == k else ok for i in range(3))) == BAD_ARG, k
    for k in range(4):                                                   # K, syms, sym_off, sym_of
        assert sym(tabs=tuple(nul if i == k else ok for i in range(4))) == BAD_ARG, k
    for kw in (dict(out=(nul, ok)), dict(out=(ok, nul)), dict(n=0), dict(n=1 << 30), dict(G=0), dict(S_tot=0), dict(S_max=0),
               dict(S_max=10), dict(I=0), dict(I=-2)):
        assert sym(**kw) == BAD_ARG, kw
    assert sym(nbytes=size(4, 8) - 1) == WORKSPACE and sym(ws=nul) == WORKSPACE and sym(nbytes=0) == WORKSPACE
    assert sym(scales=(ok, ok), shared=1, nbytes=0) == WORKSPACE           # the optional arrays: the next check is reached

    taus = (ctypes.c_double * 17)(*([0.1] * 17))

    def vsd(imgs=(ok,) * 3, K=ok, opt=(nul,) * 3, taus=taus, delta=0.015, mode=0, I=2, h=24, w=32, F=1, H=24, W=32, T=6,
            out=(ok, ok)):
        return lib.catre_vsd(*imgs, K, *opt, taus, delta, mode, I, h, w, F, H, W, T, out[0], out[1], nul)

    for k in range(3):                                                   # depth_est, depth_gt, depth_test
        assert vsd(imgs=tuple(nul if i == k else ok for i in range(3))) == BAD_ARG, k
    nan = (ctypes.c_double * 17)(*([0.1] * 3 + [float("nan")] + [0.1] * 13))
    for kw in (dict(K=nul), dict(taus=nul), dict(out=(nul, ok)), dict(out=(ok, nul)), dict(I=0), dict(h=0), dict(w=-1), dict(F=0),
               dict(H=0), dict(W=0), dict(T=0), dict(delta=float("nan")), dict(mode=2), dict(mode=-1), dict(taus=nan),
               dict(h=1 << 15, w=1 << 15), dict(H=1 << 15, W=1 << 15)):
        assert vsd(**kw) == BAD_ARG, kw
    assert vsd(T=17) == UNSUPPORTED


# ---- the Python layer's argument checks -----------------------------------------------------------------------------------------
def test_sym_errors_argument_checks():
    I, n = 3, 8
    syms = pose_errors.SymSets.from_list([None] * I, "cpu")
    ok = dict(pose_est=torch.zeros(I, 3, 4), pose_gt=torch.zeros(I, 3, 4), pts=torch.zeros(I, n, 3), K=torch.eye(3), syms=syms)
    before = pose_errors.abi_call_count()
    for kw in (dict(pose_est=torch.zeros(I, 4, 4)), dict(pose_est=torch.zeros(0, 3, 4)), dict(pose_est="no tensor"),
               dict(pose_gt=torch.zeros(I + 1, 3, 4)), dict(pose_gt=None), dict(pts=torch.zeros(I, n, 4)), dict(pts=torch.zeros(I + 1, n, 3)),
               dict(pts=torch.zeros(I, 0, 3)), dict(pts=torch.zeros(3)), dict(pts=None), dict(K=torch.eye(4)), dict(K=torch.zeros(I + 1, 3, 3)),
               dict(syms=[None] * I), dict(syms=pose_errors.SymSets.from_list([None] * (I + 1), "cpu")), dict(sym_of=[0, 1]),
               dict(sym_of=[0, 1, 3]), dict(sym_of=[0, -1, 0]), dict(sym_of="abc"), dict(scale_est=torch.ones(I, 4)),
               dict(scale_gt=torch.ones(I + 1, 3)), dict(scale_gt="no tensor"),
               dict(pts=torch.zeros(I, n, 3, device="meta")), dict(pose_gt=torch.zeros(I, 3, 4, device="meta")),
               dict(scale_est=torch.ones(I, 3, device="meta"))):
        with pytest.raises(ValueError):
            pose_errors.sym_errors(**{**ok, **kw})
    with pytest.raises(hip.CatreHipError):                               # well-formed, but not on a device: no CPU fallback
        pose_errors.sym_errors(**ok)
    assert pose_errors.abi_call_count() == before                        # refused before any entry point is called


def test_vsd_argument_checks():
    I, h, w = 2, 24, 32
    img = torch.zeros(I, h, w)
    ok = dict(depth_est=img, depth_gt=img, depth_test=torch.zeros(1, h, w), K=torch.eye(3))
    before = pose_errors.abi_call_count()
    for kw in (dict(depth_est=torch.zeros(h, w)), dict(depth_est=torch.zeros(0, h, w)), dict(depth_est="no tensor"),
               dict(depth_gt=torch.zeros(I, h, w + 1)), dict(depth_gt=None), dict(depth_test=torch.zeros(1, 1, h, w)),
               dict(depth_test=torch.zeros(0, h, w)), dict(depth_test=None), dict(K=torch.eye(4)), dict(K=torch.zeros(3, 3, 3)),
               dict(taus=()), dict(taus=[0.1] * 17), dict(taus=[0.1, float("nan")]), dict(taus="abc"), dict(taus=None),
               dict(visib_mode="bop20"), dict(cost_type="linear"), dict(delta=float("nan")),
               dict(frame_of=[0]), dict(frame_of=[0, 1]), dict(frame_of=[0, -1]), dict(frame_of=["a", "b"]),
               dict(origin=[0, 0]), dict(origin=[[0, 0]]), dict(origin=[[0, 0, 0], [0, 0, 0]]), dict(origin=[[0, 1 << 31], [0, 0]]),
               dict(diameter=[0.1, 0.2, 0.3]), dict(diameter=torch.ones(I + 1)),
               dict(depth_gt=torch.zeros(I, h, w, device="meta")), dict(depth_test=torch.zeros(1, h, w, device="meta"))):
        with pytest.raises(ValueError):
            pose_errors.vsd(**{**ok, **kw})
    with pytest.raises(NotImplementedError):
        pose_errors.vsd(**ok, cost_type="tlinear")
    with pytest.raises(hip.CatreHipError):
        pose_errors.vsd(**ok, frame_of=[0, 0], origin=[[0, 0], [3, -2]], diameter=0.2)
    kps, pose, scale = torch.zeros(I, 8, 3), torch.zeros(I, 3, 4), torch.ones(I, 3)
    okp = dict(kps=kps, pose_est=pose, scale_est=scale, pose_gt=pose, scale_gt=scale, K=torch.eye(3), depth_test=torch.zeros(h, w))
    for kw in (dict(pose_est=torch.zeros(3, 4)), dict(depth_test="no tensor"), dict(origin=[[0, 0], [1, 1]]), dict(K=torch.eye(4)),
               dict(size=(h, w), origin=[[0, 0]]), dict(kps=torch.zeros(I, 8, 4)), dict(scale_gt=None), dict(size=(0, w))):
        with pytest.raises(ValueError):
            pose_errors.vsd_prior(**{**okp, **kw})
    with pytest.raises(hip.CatreHipError):
        pose_errors.vsd_prior(**okp, size=(12, 16), origin=[[0, 0], [5, 5]])
    assert pose_errors.abi_call_count() == before
    assert "splatted point prior".upper() in pose_errors.vsd_prior.__doc__.upper() and "mesh render" in pose_errors.vsd_prior.__doc__
    assert "any renderer" in pose_errors.vsd_prior.__doc__


# ---- preconditions of the GPU tests ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.EDGE_CASES))
def test_edge_cases_hold_their_edges_and_can_be_called(name):
    """Each case holds the sizes it claims, stays inside the conditions the bounds are stated for, keeps the bounds below what
    would hide a failure, and its winners are never too close to call: the cap on such instances is zero."""
    n, scales, shared, k_per = C.EDGE_CASES[name]
    d, refs = C.edge_data(name), C.edge_reference(name)
    assert d["pts"].shape == ((n, 3) if shared else (6, n, 3)) and (d["scale_gt"] is not None) == scales
    assert d["K"].shape == ((6, 3, 3) if k_per else (3, 3)) and [len(s) for s in d["sets"]] == list(C.SET_SIZES)
    assert C.SET_SIZES == (1, 2, C.SYM_TILE - 1, C.SYM_TILE, C.SYM_TILE + 1, 314)
    for i, r in enumerate(refs):
        a = C.instance(d, i)
        s = np.ones(3) if a["scale_gt"] is None else a["scale_gt"].astype(np.float64)
        assert np.linalg.norm(a["pts"].astype(np.float64) * s, axis=1).max() <= 2.0 and 590 <= a["K"][0, 0] <= 620
        for pose, sc in ((a["pose_est"], a["scale_est"]), (a["pose_gt"], a["scale_gt"])):
            z = (a["pts"].astype(np.float64) * (1 if sc is None else sc)) @ pose[2, :3].astype(np.float64) + pose[2, 3]
            assert z.min() >= 0.3, (i, z.min())
        assert r.b3.max() < 1e-5 and r.b2.max() < 1e-2 and r.bp.max() < 1e-2, (i, r.b3.max(), r.b2.max(), r.bp.max())
        assert (r.gap > 2 * r.bound).all(), (name, i, r.gap, r.bound)
        if C.SET_SIZES[i] > 1:
            assert (r.best > 0).all(), (i, r.best, d["pick"][i])             # at or next to the member the estimate stands off
    assert {c[0] for c in C.EDGE_CASES.values()} == {1, 63, 64, 65, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1}


def test_lattice_case_is_exact_and_ties():
    d = C.lattice_data()
    for i in range(2):
        a = C.instance(d, i)
        r = REF.sym_errors(**a)
        for pose, sc, sets in ((a["pose_est"], a["scale_est"], [None]), (a["pose_gt"], a["scale_gt"], list(a["syms"]))):
            for sym in sets:
                x = a["pts"].astype(np.float64) @ REF.compose(pose, sc, sym)[:, :3].T + REF.compose(pose, sc, sym)[:, 3]
                assert set(np.unique(x[:, 2])) <= {1.0, 2.0, 4.0} and np.array_equal(x * 32, np.round(x * 32)) and np.abs(x).max() < 8
                uv = 64 * x[:, :2] / x[:, 2:3] + np.array([28.0, 20.0])
                assert np.array_equal(uv * 2, np.round(uv * 2)) and np.abs(uv).max() < 512
        assert (r.best == d["pick"][i]).all()
    r0 = REF.sym_errors(**C.instance(d, 0))
    for t in (r0.e3, r0.e2, r0.p2):
        assert t[1] == t[3] == t.min() and t[1] < t[[0, 2, 4]].min()               # an exact tie of two symmetries: the lower wins


def test_envelope_case_stands_at_the_stated_conditions():
    """|p| <= 2 m reached, z >= 0.3 m reached, a 600 px camera - and at that edge the bounds keep under their caps and no winner is
    too close to call"""
    d, refs = C.envelope_data(), C.envelope_reference()
    assert d["K"][0, 0] == d["K"][1, 1] == 600
    for i, r in enumerate(refs):
        a = C.instance(d, i)
        norm = np.linalg.norm(a["pts"].astype(np.float64), axis=1)
        assert norm.max() <= 2.0 and (norm > 1.9999).sum() >= 20, (i, norm.max())
        zs = [a["pts"].astype(np.float64) @ pose[2, :3].astype(np.float64) + pose[2, 3] for pose in (a["pose_est"], a["pose_gt"])]
        assert min(z.min() for z in zs) >= 0.3 and zs[1].min() < 0.301, (i, [z.min() for z in zs])
        x = a["pts"].astype(np.float64) @ a["pose_gt"][:, :3].astype(np.float64).T + a["pose_gt"][:, 3]
        assert np.hypot(600 * x[:, 0] / x[:, 2], 600 * x[:, 1] / x[:, 2]).max() > 800   # far outside the image: |q| is what the bound grows with
        assert r.b3.max() < 1e-5 and r.b2.max() < 1e-2 and r.bp.max() < 1e-2, (i, r.b3.max(), r.b2.max(), r.bp.max())
        assert (r.gap > 2 * r.bound).all(), (i, r.gap, r.bound)


def test_contraction_pixels_tell_the_two_arithmetics_apart():
    d = C.contraction_data()
    assert len(d["taus"]) == 16 and (d["want"] != d["fused"]).all() and d["want"].sum() == 8
    for i in range(16):
        v, u = np.argwhere(d["depth_gt"][i] > 0)[0]
        assert (d["depth_gt"][i] > 0).sum() == 1 == (d["depth_est"][i] > 0).sum() and d["depth_est"][i, v, u] > 0
        (gp, gf), (ep, ef) = C._dist_pair(u, v, d["depth_gt"][i, v, u]), C._dist_pair(u, v, d["depth_est"][i, v, u])
        assert abs(gp - ep) != abs(gf - ef) and abs(float(np.nextafter(gp, 9)) - gp) >= abs(gp - gf)   # one double step, if any
        r = REF.vsd(d["depth_est"][i], d["depth_gt"][i], d["depth_test"][0], d["K"], 0.015, d["taus"])
        assert r.dist_gt[v, u] == gp and r.dist_est[v, u] == ep                 # the restatement is the uncontracted one
        assert r.counts[0] == r.counts[1] == 1 and r.counts[2 + i] == d["want"][i], (i, r.counts)
