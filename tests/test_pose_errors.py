"""The BOP pose errors on the device (``catre_amd/pose_errors.py``, ``csrc/catre_bop.h``) against the fp64 restatement
``tests/pose_errors_ref.py`` (itself pinned to the reference's ``lib/pysixd`` by ``tests/test_pose_errors_host.py``), bit for bit
where the arithmetic is exact, and against the reference's own VSD numbers (``tests/golden/pose_error_bop.npz``).

Bounds of the point errors, derived from the arithmetic the kernel spells out (u = 2^-24; ``pose_errors_ref._posed`` /
``_projected`` / ``sym_errors`` compute them per point and symmetry; first order, times 1.001 for what is of second order):
* the composite A = R diag(s) [R_s | t_s] + [0 | t] is formed in double (2^-53: nothing) and rounded once per entry: u |A|.  A
  posed coordinate is three fmas, t + A0 p.x first, each rounding a partial sum of at most a + |t| with a = sum_c |A_c| |p_c|:
  e_x = u a + u |t| + 3 u (a + |t|) = u (4 a + 4 |t|), for the estimate and for the ground truth under a symmetry alike.
* u = fl(fl(fl(fx x) / z) + cx).  With q = fx x / z: the error of x moves q by fx e_x / z, the error of z by |q| e_z / z, the
  product and the quotient add 2 u |q|, the sum u |u|: e_u = (fx e_x + |q| e_z) / z + 2 u |q| + u |u|; e_v alike.
* a 3D distance d = sqrt(fma(dx, dx, fma(dy, dy, dz dz))) with dx = fl(x_est - x_gt): the inputs move it by at most the norm of
  (e_x,est + e_x,gt) over the coordinates; the three subtractions add u d, the three roundings of d^2 1.5 u d, the root u d:
  under |e| + 4 u d.  A pixel distance alike with two terms: |e_uv| + 3 u d.
* a maximum over the points moves by at most the largest bound of a point; the mean (added in double: nothing) by the mean
  bound plus u for its one rounding to fp32; a minimum over the symmetries by the largest bound of a symmetry.
Two conditions keep the bounds from hiding a failure, asserted here and on the CPU in ``tests/test_pose_errors_host.py``: with
|p| <= 2 m and z >= 0.3 m in front of a 600 px camera the MSSD bound stays below 1e-5 m, the MSPD / proj bound below 1e-2 px.
The edge cases lie well inside those conditions (objects of 0.2 m at 0.6 - 1.4 m); ``pose_errors_cases.envelope_data`` stands AT
them - points on the |p| = 2 m sphere in every direction, the nearest at z = 0.3 m, projections many hundreds of pixels off
the principal point - and the same caps are asserted on its bounds (the largest: 3.2e-6 m, 7.0e-3 px).
The winning index is compared in every case: the host test shows the runner-up more than twice the bound behind in all of them.

VSD is compared exactly: integer counts, and errors that are one double division of them.  ``profiles/bop_parity.py`` records the
worst deviation / bound ratios of the edge cases in ``profiles/bop_parity.json``."""
import numpy as np
import pytest
import torch

from tests import pose_errors_cases as C
from tests import pose_errors_ref as REF


def _np(t):
    return t.cpu().numpy()


# ---- 1. edges against the restatement ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.EDGE_CASES))
def test_edges_against_the_restatement(name):
    d, refs = C.edge_data(name), C.edge_reference(name)
    got = C.run_sym(d)
    err = np.stack([_np(got.mssd), _np(got.mspd), _np(got.proj)], 1).astype(np.float64)
    best = np.stack([_np(got.best_mssd), _np(got.best_mspd), _np(got.best_proj)], 1)
    tabs = [_np(t).astype(np.float64) for t in (got.e3, got.e2, got.p2)]
    for i, r in enumerate(refs):
        S = C.SET_SIZES[i]
        assert r.b3.max() < 1e-5 and r.b2.max() < 1e-2 and r.bp.max() < 1e-2, (name, i)
        for q, (want, bound, what) in enumerate(((r.e3, r.b3, "e3"), (r.e2, r.b2, "e2"), (r.p2, r.bp, "p2"))):
            dev_ = np.abs(tabs[q][i, :S] - want)
            print(name, "S", S, what, "worst dev", dev_.max(), "bound there", bound[np.argmax(dev_ / bound)], "ratio", (dev_ / bound).max())
            assert (dev_ <= bound).all(), (name, i, what, dev_.max(), bound.max())
            assert np.isposinf(tabs[q][i, S:]).all(), (name, i, what)                     # the padding behind the set
            assert abs(err[i, q] - r.err[q]) <= r.bound[q], (name, i, what)
            assert err[i, q] == tabs[q][i, :S].min().astype(np.float32), (name, i, what)   # the minima are the tables'
        assert (r.gap > 2 * r.bound).all() and np.array_equal(best[i], r.best), (name, i, best[i], r.best)


@pytest.mark.gpu
def test_envelope_of_the_bounds():
    d, refs = C.envelope_data(), C.envelope_reference()
    got = C.run_sym(d)
    tabs = [_np(t).astype(np.float64) for t in (got.e3, got.e2, got.p2)]
    best = np.stack([_np(got.best_mssd), _np(got.best_mspd), _np(got.best_proj)], 1)
    for i, r in enumerate(refs):
        S = C.ENVELOPE_SETS[i]
        assert r.b3.max() < 1e-5 and r.b2.max() < 1e-2 and r.bp.max() < 1e-2, i
        for q, (want, bound, what) in enumerate(((r.e3, r.b3, "e3"), (r.e2, r.b2, "e2"), (r.p2, r.bp, "p2"))):
            dev_ = np.abs(tabs[q][i, :S] - want)
            print("envelope S", S, what, "worst dev", dev_.max(), "largest bound", bound.max(), "ratio", (dev_ / bound).max())
            assert (dev_ <= bound).all(), (i, what, dev_.max(), bound.max())
        assert (r.gap > 2 * r.bound).all() and np.array_equal(best[i], r.best), (i, best[i], r.best)


# ---- 2. exact lattice ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_lattice_and_tie():
    d = C.lattice_data()
    got = C.run_sym(d)
    for i in range(2):
        r = REF.sym_errors(**C.instance(d, i), f32_roots=True)
        S = len(d["sets"][i])
        for t, want, what in ((got.e3, r.e3, "e3"), (got.e2, r.e2, "e2"), (got.p2, r.p2, "p2")):
            # squared distances are exact; the root is correctly rounded (fp64 root, then one rounding: innocuous for 53 >= 2 * 24 + 2)
            assert np.array_equal(_np(t)[i, :S].view(np.uint32), want.astype(np.float32).view(np.uint32)), (i, what)
        for t, k in ((got.mssd, 0), (got.mspd, 1), (got.proj, 2)):
            assert _np(t)[i] == np.float32(r.err[k]), (i, k)
        assert (_np(got.best_mssd)[i], _np(got.best_mspd)[i], _np(got.best_proj)[i]) == (1, 1, 1), i
    e3 = _np(got.e3)[0]
    assert e3[1] == e3[3] == e3[:5].min()                                 # the tie of symmetries 1 and 3: index 1 was reported


# ---- 3. independence, NaN, per_sym ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_instance_alone_equals_instance_in_batch():
    d = C.edge_data("above_chunk")
    whole = C.run_sym(d)
    for i in (0, 2, 5):
        alone = C.run_sym(d, rows=[i])
        S = C.SET_SIZES[i]
        for f in ("mssd", "mspd", "proj", "best_mssd", "best_mspd", "best_proj"):
            assert torch.equal(getattr(whole, f)[i:i + 1], getattr(alone, f)), (i, f)
        for f in ("e3", "e2", "p2"):
            assert torch.equal(getattr(whole, f)[i, :S], getattr(alone, f)[0, :S]), (i, f)
    # a different batch order and shared sets: still the same bits per instance
    from catre_amd import pose_errors

    perm = [5, 0, 3, 3, 1]
    syms = pose_errors.SymSets.from_list(d["sets"], "cuda", sym_of=perm)
    pick = lambda a: C.dev(a[perm], torch.float32)
    got = pose_errors.sym_errors(pick(d["pose_est"]), pick(d["pose_gt"]), C.dev(d["pts"], torch.float32), pick(d["K"]), syms,
                                 scale_est=pick(d["scale_est"]), scale_gt=pick(d["scale_gt"]))
    assert got.e3 is None and got.p2 is None
    for f in ("mssd", "mspd", "proj", "best_mssd", "best_mspd", "best_proj"):
        assert torch.equal(getattr(got, f), getattr(whole, f)[perm]), f
    # sym_of given at the call, as a list and as a device tensor
    syms2 = pose_errors.SymSets.from_list(d["sets"], "cuda")
    args = (pick(d["pose_est"]), pick(d["pose_gt"]), C.dev(d["pts"], torch.float32), pick(d["K"]), syms2)
    kw = dict(scale_est=pick(d["scale_est"]), scale_gt=pick(d["scale_gt"]))
    for so in (perm, torch.tensor(perm, dtype=torch.int32).cuda()):
        assert torch.equal(pose_errors.sym_errors(*args, sym_of=so, **kw).mssd, got.mssd)


@pytest.mark.gpu
def test_nan_pose_leaves_the_others_untouched():
    d = C.edge_data("n65")
    whole = C.run_sym(d)
    for field, idx in (("pose_est", (2, 0, 3)), ("pose_gt", (4, 1, 1)), ("pts", (5, 17, 2))):
        bad = dict(d)
        bad[field] = d[field].copy()
        bad[field][idx] = np.nan
        got = C.run_sym(bad)
        i = idx[0]
        others = [j for j in range(6) if j != i]
        for f in ("mssd", "mspd", "proj"):
            assert torch.isnan(getattr(got, f)[i]), (field, f)
            assert torch.equal(getattr(got, f)[others], getattr(whole, f)[others]), (field, f)
        for f in ("best_mssd", "best_mspd", "best_proj"):
            assert torch.equal(getattr(got, f)[others], getattr(whole, f)[others]), (field, f)
    d = C.edge_data("n64")                                                # a case with scales
    whole = C.run_sym(d)
    for field, idx in (("scale_est", (1, 2)), ("scale_gt", (3, 0))):
        bad = dict(d)
        bad[field] = d[field].copy()
        bad[field][idx] = np.nan
        got = C.run_sym(bad)
        others = [j for j in range(6) if j != idx[0]]
        for f in ("mssd", "mspd", "proj"):
            assert torch.isnan(getattr(got, f)[idx[0]]), (field, f)
            assert torch.equal(getattr(got, f)[others], getattr(whole, f)[others]), (field, f)


@pytest.mark.gpu
def test_per_sym_tables_agree_with_the_minima_and_nothing_is_read_back():
    from catre_amd import pose_errors

    d = C.edge_data("n64")
    with_t, without = C.run_sym(d, per_sym=True), C.run_sym(d, per_sym=False)
    for f, t in (("mssd", "e3"), ("mspd", "e2"), ("proj", "p2")):
        tab = getattr(with_t, t)
        assert tuple(tab.shape) == (6, 314) and torch.equal(getattr(with_t, f), tab.min(1).values), f
        assert torch.equal(getattr(with_t, "best_" + f), tab.argmin(1).int()), f          # no ties here: argmin is the index
        assert torch.equal(getattr(with_t, f), getattr(without, f)), f
    # the ABI-call count does not depend on I, S or n, and nothing synchronises with the host
    args = {}
    for name, rows in (("n64", [0, 1]), ("n65", list(range(6)))):
        dd = C.edge_data(name)
        pick = lambda a, per=True: None if a is None else C.dev(a[rows] if per else a, torch.float32)
        args[name] = ((pick(dd["pose_est"]), pick(dd["pose_gt"]), pick(dd["pts"], dd["pts"].ndim == 3), pick(dd["K"], dd["K"].ndim == 3),
                       pose_errors.SymSets.from_list([dd["sets"][i] for i in rows], "cuda")),
                      dict(scale_est=pick(dd["scale_est"]), scale_gt=pick(dd["scale_gt"])))
    torch.cuda.synchronize()
    grown = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for name in ("n64", "n65"):
            before = pose_errors.abi_call_count()
            pose_errors.sym_errors(*args[name][0], **args[name][1])
            grown.append(pose_errors.abi_call_count() - before)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert grown == [2, 2], grown


# ---- 4. VSD ---------------------------------------------------------------------------------------------------------------------
def _golden_vsd(g, j, c, **kw):
    from catre_amd import pose_errors

    diam = float(g["vsd/diameter"]) if c["normalized"] else None
    return pose_errors.vsd(C.dev(g[f"v{j}/d_est"])[None], C.dev(g[f"v{j}/d_gt"])[None], C.dev(g[f"v{j}/d_test"])[None], g["vsd/K"],
                           delta=float(g["vsd/delta"]), taus=g["vsd/taus"].tolist(), diameter=diam, visib_mode=c["mode"], **kw)


@pytest.mark.gpu
def test_vsd_equals_the_reference_exactly():
    """both modes, with and without the diameter, the pixels on delta and one fp32 step beside it, the pixels on a tau, an empty union;
    24 x 32 windows: 768 pixels, three rows of 256 in one workgroup, a width that is no multiple of 64 (more than one workgroup
    per window: ``test_vsd_windows``)"""
    g = C.golden()
    cases = C.golden_meta(g)["vsd_cases"]
    for j, c in enumerate(cases):
        errors, counts = _golden_vsd(g, j, c)
        assert errors.dtype == torch.float64 and counts.dtype == torch.int32 and tuple(errors.shape) == (1, 6) and tuple(counts.shape) == (1, 8)
        assert np.array_equal(_np(counts)[0], g[f"v{j}/counts"]), (j, c, _np(counts)[0], g[f"v{j}/counts"])
        assert np.array_equal(_np(errors)[0], g[f"v{j}/errors"]), (j, c)
        if c["empty"]:
            assert (_np(errors) == 1.0).all() and _np(counts)[0, 0] == 0


@pytest.mark.gpu
def test_vsd_batches_frames_and_tau_counts():
    from catre_amd import pose_errors

    g = C.golden()
    cases = C.golden_meta(g)["vsd_cases"]
    K, delta = g["vsd/K"], float(g["vsd/delta"])
    # four instances in two frames, a diameter per instance, K per instance
    inst = [(0, 0), (2, 1), (3, 0), (0, 1)]                               # (case whose renders are used, observed frame)
    frames = np.stack([g["v0/d_test"], g["v2/d_test"]])
    est, gt = (np.stack([g[f"v{j}/{k}"] for j, _ in inst]) for k in ("d_est", "d_gt"))
    diam = np.array([0.25, 0.2, 0.5, 0.125])
    Ks = np.stack([K + np.float32([[0, 0, i], [0, 0, -i], [0, 0, 0]]) for i in range(4)])
    for mode in ("bop19", "bop18"):
        for taus in ([0.07], [0.01 * k for k in range(1, 17)]):            # T = 1 and T = 16
            errors, counts = pose_errors.vsd(C.dev(est), C.dev(gt), C.dev(frames), Ks, delta=delta, taus=taus, diameter=diam,
                                             frame_of=[f for _, f in inst], visib_mode=mode)
            for i, (_, f) in enumerate(inst):
                r = REF.vsd(est[i], gt[i], frames[f], Ks[i], delta, taus, diam[i], visib_mode=mode)
                assert np.array_equal(_np(counts)[i], r.counts) and np.array_equal(_np(errors)[i], r.errors), (mode, len(taus), i)
            assert tuple(counts.shape) == (4, 2 + len(taus)) and (_np(counts)[:, 0] > 0).all()
    # frame_of and origin as device tensors, a diameter as a device tensor: the same
    e2, c2 = pose_errors.vsd(C.dev(est), C.dev(gt), C.dev(frames), C.dev(Ks), delta=delta, taus=taus, diameter=C.dev(diam),
                             frame_of=torch.tensor([f for _, f in inst], dtype=torch.int32).cuda(),
                             origin=torch.zeros(4, 2, dtype=torch.int32).cuda(), visib_mode=mode)
    assert torch.equal(e2, errors) and torch.equal(c2, counts)


@pytest.mark.gpu
def test_vsd_windows():
    from catre_amd import pose_errors

    g = C.golden()
    K, delta, taus = g["vsd/K"], float(g["vsd/delta"]), g["vsd/taus"].tolist()
    test, est, gt = g["v0/d_test"], g["v0/d_est"].copy(), g["v0/d_gt"].copy()
    u0, v0, h, w = 9, 3, 17, 19                                            # 323 pixels: not a multiple of 64 or 256
    inside = np.zeros_like(est, bool)
    inside[v0:v0 + h, u0:u0 + w] = True
    est[~inside], gt[~inside] = 0, 0                                      # nothing rendered outside the window
    full_e, full_c = pose_errors.vsd(C.dev(est)[None], C.dev(gt)[None], C.dev(test)[None], K, delta=delta, taus=taus)
    crop = lambda a: np.ascontiguousarray(a[v0:v0 + h, u0:u0 + w])
    win_e, win_c = pose_errors.vsd(C.dev(crop(est))[None], C.dev(crop(gt))[None], C.dev(test)[None], K, delta=delta, taus=taus,
                                   origin=[[u0, v0]])
    assert torch.equal(win_c, full_c) and torch.equal(win_e, full_e) and _np(full_c)[0, 1] > 0
    r = REF.vsd(crop(est), crop(gt), test, K, delta, taus, origin=(u0, v0))
    assert np.array_equal(_np(win_c)[0], r.counts) and np.array_equal(_np(win_e)[0], r.errors)
    # a window of 50 x 70 = 3500 pixels: a workgroup walks 2048, so two per instance add into the same counts; three instances
    rng = np.random.default_rng(6)
    frame = rng.uniform(0.7, 1.3, (60, 90)).astype(np.float32)
    frame[rng.random(frame.shape) < 0.1] = 0
    big_o = [[11, 7], [0, 0], [20, 10]]
    e_b = np.stack([frame[v:v + 50, u:u + 70] for u, v in big_o]) + rng.normal(0, 0.03, (3, 50, 70)).astype(np.float32)
    g_b = (e_b + rng.normal(0, 0.05, e_b.shape)).astype(np.float32)
    e_b[rng.random(e_b.shape) < 0.3], g_b[rng.random(g_b.shape) < 0.3] = 0, 0
    errors, counts = pose_errors.vsd(C.dev(e_b), C.dev(g_b), C.dev(frame), K, delta=delta, taus=taus, origin=big_o, visib_mode="bop18")
    for i, o in enumerate(big_o):
        r = REF.vsd(e_b[i], g_b[i], frame, K, delta, taus, origin=o, visib_mode="bop18")
        assert np.array_equal(_np(counts)[i], r.counts) and np.array_equal(_np(errors)[i], r.errors), (i, o)
        assert r.counts[1] > 500 and (r.vis_gt | r.vis_est).reshape(-1)[2048:].sum() > 100 < (r.vis_gt | r.vis_est).reshape(-1)[:2048].sum()
    # windows hanging over every edge of the frame: the pixels outside are ignored
    rng = np.random.default_rng(5)
    hh, ww = 20, 27
    origins = [[-5, -3], [32 - 9, 24 - 6], [-30, 2], [40, 40]]           # the last two: a sliver, and wholly outside
    e_w = rng.uniform(0.7, 1.3, (4, hh, ww)).astype(np.float32)
    g_w = (e_w + rng.normal(0, 0.05, e_w.shape)).astype(np.float32)
    errors, counts = pose_errors.vsd(C.dev(e_w), C.dev(g_w), C.dev(test), K, delta=delta, taus=taus, origin=origins, diameter=0.25)
    for i, o in enumerate(origins):
        r = REF.vsd(e_w[i], g_w[i], test, K, delta, taus, 0.25, origin=o)
        assert np.array_equal(_np(counts)[i], r.counts) and np.array_equal(_np(errors)[i], r.errors), (i, o)
        assert r.counts[0] <= r.inside.sum() < hh * ww
    assert _np(counts)[0, 0] > 0 and _np(counts)[3, 0] == 0 and (_np(errors)[3] == 1.0).all()   # an empty union gives 1.0


@pytest.mark.gpu
def test_vsd_distance_is_not_contracted():
    """``misc.py:643-645`` rounds every square and every sum of the distance; a compiler that contracts them into fused
    multiply-adds moves the value under the root by a double step now and then.  Sixteen pixels found by search where that
    step shows in |dist_gt - dist_est|, each with a tau on (or one double step above) the reference's value: the cost of
    instance t at tau t is the reference's, and what contraction would count is the opposite in all sixteen."""
    from catre_amd import pose_errors

    d = C.contraction_data()
    errors, counts = pose_errors.vsd(C.dev(d["depth_est"]), C.dev(d["depth_gt"]), C.dev(d["depth_test"]), d["K"], taus=d["taus"])
    counts = _np(counts)
    assert (counts[:, :2] == 1).all()
    assert (d["want"] != d["fused"]).all()
    assert np.array_equal(counts[np.arange(16), 2 + np.arange(16)], d["want"]), (counts[np.arange(16), 2 + np.arange(16)], d["want"])
    for i in range(16):
        r = REF.vsd(d["depth_est"][i], d["depth_gt"][i], d["depth_test"][0], d["K"], 0.015, d["taus"])
        assert np.array_equal(counts[i], r.counts) and np.array_equal(_np(errors)[i], r.errors), i


# ---- 5. vsd_prior --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_vsd_prior_is_its_composition():
    from catre_amd import pose_errors, render
    from tests import render_cases as RC

    rng = np.random.default_rng(93)
    H, W, M = 48, 64, 256

    def scene(I):
        kps = np.stack([RC.box_points(rng, M, (1.0, 1.0, 1.0)) for _ in range(I)]).astype(np.float32)
        scale = rng.uniform(0.18, 0.25, (I, 3)).astype(np.float32)
        pose_gt = np.stack([RC.pose_of(RC.rotation(rng), (rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.2)))
                            for _ in range(I)]).astype(np.float32)
        pose_est = pose_gt.copy()
        pose_est[:, :, 3] += rng.normal(0, 0.01, (I, 3)).astype(np.float32)
        depth = rng.uniform(0.8, 1.4, (2, H, W)).astype(np.float32)
        return [C.dev(a) for a in (kps, pose_est, scale * np.float32(1.02), pose_gt, scale)], C.dev(depth)

    K = torch.as_tensor(RC.camera(H, W, 70.0))                            # on the host, where splat_prior reads it
    grown = {}
    for I in (1, 3):
        (kps, pe, se, pg, sg), depth = scene(I)
        fo = [i % 2 for i in range(I)]
        own = list(range(I))
        est = render.splat_prior(kps, pe, se, K, (H, W), frame_of=own, n_frames=I)
        gt = render.splat_prior(kps, pg, sg, K, (H, W), frame_of=own, n_frames=I)
        want = pose_errors.vsd(est.zbuf, gt.zbuf, depth, K, diameter=0.3, frame_of=fo)
        torch.cuda.synchronize()
        before = render.abi_call_count() + pose_errors.abi_call_count()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = pose_errors.vsd_prior(kps, pe, se, pg, sg, K, depth, frame_of=fo, diameter=0.3)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        grown[I] = render.abi_call_count() + pose_errors.abi_call_count() - before
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and (got[1][:, 1] > 0).all(), I
        # a window: the render's camera is shifted, the comparison reads the full-image K
        u0, v0, h, w = 6, 4, 40, 52
        Kw = K.clone()
        Kw[0, 2] -= u0
        Kw[1, 2] -= v0
        est = render.splat_prior(kps, pe, se, Kw, (h, w), frame_of=own, n_frames=I)
        gt = render.splat_prior(kps, pg, sg, Kw, (h, w), frame_of=own, n_frames=I)
        want = pose_errors.vsd(est.zbuf, gt.zbuf, depth, K, frame_of=fo, origin=[[u0, v0]] * I, visib_mode="bop18", taus=[0.1, 0.3])
        got = pose_errors.vsd_prior(kps, pe, se, pg, sg, K, depth, frame_of=fo, origin=[[u0, v0]] * I, size=(h, w), visib_mode="bop18",
                                    taus=[0.1, 0.3])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), I
    assert grown[1] == grown[3] == 5, grown                               # 2 x (workspace size, render) + the comparison
