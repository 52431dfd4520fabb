"""Initial poses from NOCS maps on the device: ``catre_amd.nocs_align`` over ``catre_umeyama`` / ``catre_nocs_align``
(``csrc/catre_align.h``) against the values the unmodified reference wrote into ``tests/golden/nocs_align.npz`` and
against ``tests/nocs_align_ref.py``, the numpy restatement ``tests/test_nocs_align_host.py`` holds to the same fixture.

Bounds.  Discrete outputs (validity, iterations, winning iteration, inlier count and mask) are exact: the fixture's
cases keep every residual >= 1e-9 (relative) from its threshold, every 5-point covariance at sigma_2 / sigma_1 >= 1e-3
and the stop expression >= 1e-9 from 0.99, and the device seed below was chosen on the CPU so that the evaluated draws
meet the same conditions (asserted here through the restatement's trace).  s, R, t: 1e-12 absolute (float64 results of
magnitude <= 1.5; the restatement itself sits <= 2e-15 from the reference).  fp32 outputs of ``init_pose_from_nocs``:
1e-6 absolute on R, 1e-6 relative on t and scale - about 8 fp32 ulps at magnitude 1, the output format.

Shapes: the fixture's n = 0, 5, 37, 63, 64, 65 (one wave and its edges), 1000, 1024 (four waves, whole tiles) and 5000
(several tiles per wave, a partial last one) as ONE ragged batch of Nmax = 5000 whose unused rows are NaN."""
import json
import os

import numpy as np
import pytest
import torch

from catre_amd import hip, nocs_align, pcl_prep, synth
from tests import nocs_align_ref as REF
from tests.util import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
SEED = 1                      # device draws: with keys 100 + case every case meets the preconditions (checked on the CPU)
MAX_ITER = 128


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN_DIR, "nocs_align.npz"))
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def batch(gold):
    """every stored case as one ragged batch; rows beyond counts[i] are NaN"""
    z, meta = gold
    J = len(meta["cases"])
    counts = [c["n"] for c in meta["cases"]]
    Nmax = max(counts)
    assert Nmax == 5000 and 0 in counts and 5 in counts
    src = np.full((J, Nmax, 3), np.nan, np.float32)
    dst = np.full((J, Nmax, 3), np.nan, np.float32)
    draws = np.zeros((J, MAX_ITER, 5), np.int32)
    for j, n in enumerate(counts):
        src[j, :n], dst[j, :n], draws[j] = z[f"c{j}/src"], z[f"c{j}/dst"], z[f"c{j}/draws"]
    t = lambda a: torch.from_numpy(a).to(DEV)
    return dict(J=J, counts=counts, Nmax=Nmax, src=t(src), dst=t(dst), draws=t(draws), counts_t=t(np.asarray(counts, np.int32)),
                keys=torch.arange(100, 100 + J, dtype=torch.int64))


def _cpu(sim):
    return nocs_align.Similarity(*[None if v is None else v.cpu().numpy() for v in sim])


def _same(a, b, rows_a, rows_b, n=None):
    """bit equality of two results at the given rows (masks over the first n columns)"""
    for name in ("scale", "R", "t", "valid", "n_inliers", "iters", "best_it"):
        x, y = getattr(a, name)[rows_a], getattr(b, name)[rows_b]
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    if a.inliers is not None and b.inliers is not None:
        assert np.array_equal(a.inliers[rows_a][..., :n], b.inliers[rows_b][..., :n])


def _check_against(got, j, want_valid, iters, best_it, inliers, s, R, t, n, label):
    """row j of a device result against expected values: discrete exact, s / R / t within TOL"""
    assert got.valid[j] == want_valid and got.iters[j] == iters and got.best_it[j] == best_it, (label, j, got.valid[j], got.iters[j], got.best_it[j])
    assert got.n_inliers[j] == len(inliers), (label, j)
    mask = np.zeros(got.inliers.shape[1], np.uint8)
    mask[inliers] = 1
    assert np.array_equal(got.inliers[j], mask), (label, j)
    err = max(abs(got.scale[j] - s), np.abs(got.R[j] - R).max(), np.abs(got.t[j] - t).max())
    print(f"{label} case {j} n={n}: iters {iters} best_it {best_it} inliers {len(inliers)} max |err| {err:.2e}")
    assert err <= TOL, (label, j, err)
    if not want_valid:
        assert got.scale[j] == 1.0 and np.array_equal(got.R[j], np.eye(3)) and np.array_equal(got.t[j], np.zeros(3))
    return err


@pytest.fixture(scope="module")
def ref_run(batch):
    """the reference-draw route on the ragged batch, once"""
    before = nocs_align.abi_call_count()
    out = nocs_align.estimate_similarity(batch["src"], batch["dst"], batch["counts_t"], draws=batch["draws"], return_inliers=True)
    assert nocs_align.abi_call_count() - before == 2           # the workspace size and the alignment itself
    return _cpu(out)


@pytest.fixture(scope="module")
def dev_run(batch):
    """the device-draw route on the ragged batch, once"""
    out = nocs_align.estimate_similarity(batch["src"], batch["dst"], batch["counts_t"], seed=SEED, keys=batch["keys"],
                                         return_inliers=True)
    return _cpu(out)


def test_reference_draws_reproduce_the_reference_on_a_ragged_batch(gold, batch, ref_run):
    z, meta = gold
    worst = 0.0
    for j, c in enumerate(meta["cases"]):
        worst = max(worst, _check_against(ref_run, j, 0 if c["none"] else 1, c["iters"], c["best_it"], z[f"c{j}/inliers"],
                                          float(z[f"c{j}/s"]), z[f"c{j}/R"], z[f"c{j}/t"], c["n"], "reference draws"))
    print(f"worst |err| vs the reference {worst:.2e}")
    assert ref_run.valid.tolist() == [0 if c["none"] else 1 for c in meta["cases"]]
    for n, arr in ((0, ref_run.iters), (0, ref_run.n_inliers)):
        assert arr[batch["counts"].index(0)] == n


def test_every_case_alone_is_bit_equal_to_its_row(batch, ref_run, dev_run):
    for j, n in enumerate(batch["counts"]):
        N1 = max(n, 1)
        src, dst = batch["src"][j:j + 1, :N1].contiguous(), batch["dst"][j:j + 1, :N1].contiguous()
        cnt = batch["counts_t"][j:j + 1]
        alone = _cpu(nocs_align.estimate_similarity(src, dst, cnt if n == 0 else None, draws=batch["draws"][j:j + 1],
                                                    return_inliers=True))
        _same(alone, ref_run, slice(0, 1), slice(j, j + 1), n)
        alone = _cpu(nocs_align.estimate_similarity(src, dst, cnt, seed=SEED, keys=batch["keys"][j:j + 1], return_inliers=True))
        _same(alone, dev_run, slice(0, 1), slice(j, j + 1), n)
    # a reversed batch: the slot does not matter either
    rev = list(range(batch["J"]))[::-1]
    out = _cpu(nocs_align.estimate_similarity(batch["src"][rev], batch["dst"][rev], batch["counts_t"][rev], seed=SEED,
                                              keys=batch["keys"][rev], return_inliers=True))
    _same(out, dev_run, slice(None), rev)


def test_device_draws(gold, batch, dev_run):
    z, meta = gold
    draws = nocs_align.draw_indices(batch["counts_t"], seed=SEED, keys=batch["keys"])
    want = REF.draw_indices(batch["counts"], seed=SEED, keys=batch["keys"].numpy())
    assert draws.dtype == torch.int32 and np.array_equal(draws.cpu().numpy(), want)
    # default keys are 0 .. I-1; another seed is another stream
    assert np.array_equal(nocs_align.draw_indices(batch["counts_t"], seed=7).cpu().numpy(), REF.draw_indices(batch["counts"], seed=7))
    assert np.array_equal(nocs_align.draw_indices(batch["counts_t"], seed=2 ** 40 + 3, keys=[-1, 2 ** 40] * 5 + [9], max_iter=17).cpu().numpy(),
                          REF.draw_indices(batch["counts"], seed=2 ** 40 + 3, keys=[-1, 2 ** 40] * 5 + [9], max_iter=17))
    replay = _cpu(nocs_align.estimate_similarity(batch["src"], batch["dst"], batch["counts_t"], draws=draws, return_inliers=True))
    _same(replay, dev_run, slice(None), slice(None))
    for j, c in enumerate(meta["cases"]):                      # no case is skipped
        out, tr = REF.estimate_similarity(z[f"c{j}/src"], z[f"c{j}/dst"], want[j], trace=True)
        if c["n"]:
            assert tr.margin >= 1e-9 and tr.sv_ratio >= 1e-3 and tr.stop_margin >= 1e-9, (j, tr)
        _check_against(dev_run, j, out.valid, out.iters, out.best_it, out.inliers, out.scale, out.R, out.t, c["n"], "device draws")
    # default keys: instance i is keyed by its slot
    a = _cpu(nocs_align.estimate_similarity(batch["src"][:3], batch["dst"][:3], batch["counts_t"][:3], seed=5))
    b = _cpu(nocs_align.estimate_similarity(batch["src"][:3], batch["dst"][:3], batch["counts_t"][:3], seed=5, keys=[0, 1, 2]))
    _same(a, b, slice(None), slice(None))
    assert a.inliers is None


def test_fewer_iterations_non_finite_rows_and_bad_draws(gold, batch):
    z, meta = gold
    j = batch["counts"].index(1000)
    src, dst, cnt = batch["src"][j:j + 1], batch["dst"][j:j + 1], batch["counts_t"][j:j + 1]
    for max_iter in (1, 31, 33):                                  # one partial block, a block edge on either side
        got = _cpu(nocs_align.estimate_similarity(src, dst, cnt, draws=batch["draws"][j:j + 1, :max_iter].contiguous(),
                                                  max_iter=max_iter, return_inliers=True))
        out = REF.estimate_similarity(z[f"c{j}/src"], z[f"c{j}/dst"], z[f"c{j}/draws"], max_iter=max_iter)
        _check_against(got, 0, out.valid, out.iters, out.best_it, out.inliers, out.scale, out.R, out.t, 1000, f"max_iter {max_iter}")
    with pytest.raises(ValueError):
        nocs_align.estimate_similarity(src, dst, cnt, max_iter=129)
    # a non-finite value inside the first n rows, too few rows, a count the arrays cannot hold: invalid, identity
    bad = dst.clone()
    bad[0, 999, 2] = float("inf")
    for s_, d_, c_ in ((src, bad, cnt), (src, dst, torch.tensor([4], dtype=torch.int32, device=DEV)),
                       (src, dst, torch.tensor([5001], dtype=torch.int32, device=DEV)),
                       (src, dst, torch.tensor([-3], dtype=torch.int32, device=DEV))):
        got = _cpu(nocs_align.estimate_similarity(s_, d_, c_, draws=batch["draws"][j:j + 1], return_inliers=True))
        assert got.valid[0] == 0 and got.iters[0] == 0 and got.best_it[0] == -1 and got.n_inliers[0] == 0
        assert got.scale[0] == 1.0 and np.array_equal(got.R[0], np.eye(3)) and not got.inliers.any()
    # draws outside [0, n) select nothing: every hypothesis is empty, the instance invalid after all iterations
    wild = torch.full((1, MAX_ITER, 5), 1000, dtype=torch.int32, device=DEV)
    wild[0, ::2] = -1
    got = _cpu(nocs_align.estimate_similarity(src, dst, cnt, draws=wild, return_inliers=True))
    assert got.valid[0] == 0 and got.iters[0] == MAX_ITER and got.best_it[0] == -1 and got.n_inliers[0] == 0 and not got.inliers.any()


def test_umeyama_alone(gold):
    z, meta = gold
    names = meta["umeyama"]
    g = {n: {k: z[f"u/{n}/{k}"] for k in ("src", "dst", "count", "mask", "s", "R", "t")} for n in names}
    Nmax = max(len(v["src"]) for v in g.values())
    assert Nmax == 1000
    src = np.full((len(names), Nmax, 3), np.nan, np.float32)
    dst = np.full((len(names), Nmax, 3), np.nan, np.float32)
    mask = np.ones((len(names), Nmax), np.uint8)
    counts = np.zeros(len(names), np.int32)
    for i, n in enumerate(names):
        m = len(g[n]["src"])
        src[i, :m], dst[i, :m], mask[i, :m], counts[i] = g[n]["src"], g[n]["dst"], g[n]["mask"], g[n]["count"]
    t = lambda a: torch.from_numpy(a).to(DEV)
    s, R, tr = [v.cpu().numpy() for v in nocs_align.umeyama(t(src), t(dst), t(counts), t(mask))]
    assert s.dtype == R.dtype == tr.dtype == np.float64 and R.shape == (len(names), 3, 3)
    for i, n in enumerate(names):
        err = max(abs(s[i] - float(g[n]["s"])), np.abs(R[i] - g[n]["R"]).max(), np.abs(tr[i] - g[n]["t"]).max())
        print(f"umeyama {n}: max |err| {err:.2e}")
        assert err <= TOL, (n, err)
    # the same instances alone, without counts / mask where the case has none, and with a bool mask: the same bits
    for i, n in enumerate(names):
        m = len(g[n]["src"])
        plain = n in ("m5", "m64", "m65", "m1000", "mirrored", "planar")
        a = nocs_align.umeyama(t(src[i:i + 1, :m]), t(dst[i:i + 1, :m]), None if plain else t(counts[i:i + 1]),
                               None if plain else t(mask[i:i + 1, :m]).bool())
        for x, y in zip(a, (s, R, tr)):
            assert np.array_equal(x.cpu().numpy()[0], y[i]), n
    # nothing kept: the identity
    s0, R0, t0 = nocs_align.umeyama(t(src[:1]), t(dst[:1]), t(np.zeros(1, np.int32)))
    assert s0.item() == 1.0 and torch.equal(R0[0].cpu(), torch.eye(3, dtype=torch.float64)) and not t0.any()


def test_init_pose_from_nocs(gold, batch, ref_run):
    z, meta = gold
    J = batch["J"]
    g = torch.Generator().manual_seed(3)
    extents = (0.2 + 0.6 * torch.rand(J, 3, generator=g)).to(DEV)
    pose, scale, valid = nocs_align.init_pose_from_nocs(batch["dst"], batch["src"], extents, counts=batch["counts_t"], draws=batch["draws"])
    assert pose.dtype == scale.dtype == torch.float32 and valid.dtype == torch.bool
    assert tuple(pose.shape) == (J, 3, 4) and tuple(scale.shape) == (J, 3) and tuple(valid.shape) == (J,)
    pose, scale, valid, ext = pose.cpu().numpy(), scale.cpu().numpy(), valid.cpu().numpy(), extents.cpu().numpy().astype(np.float64)
    assert valid.tolist() == [not c["none"] for c in meta["cases"]]
    for j, c in enumerate(meta["cases"]):
        s, R, t = float(z[f"c{j}/s"]), z[f"c{j}/R"], z[f"c{j}/t"]
        if c["none"]:
            assert np.array_equal(pose[j], np.eye(3, 4, dtype=np.float32)) and np.array_equal(scale[j], ext[j].astype(np.float32))
            continue
        eR = np.abs(pose[j, :, :3] - R).max()
        et = (np.abs(pose[j, :, 3] - t) / np.abs(t)).max()
        es = (np.abs(scale[j] - s * ext[j]) / (s * ext[j])).max()
        print(f"init pose case {j}: |dR| {eR:.2e} rel dt {et:.2e} rel ds {es:.2e}")
        assert eR <= 1e-6 and et <= 1e-6 and es <= 1e-6, (j, eR, et, es)


def _frames(H, W):
    """two frames, labels 1..3 per frame; coord holds the NOCS coordinates of every labelled pixel under a similarity of
    its instance; label 3 of frame 1 has no valid depth -> (depth, K, labels, coord, frame_of, label_of, truth)"""
    g = torch.Generator().manual_seed(H * 1000 + W)
    K = torch.tensor([[1.1 * W, 0.0, W / 2 - 0.5], [0.0, 1.1 * W, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = torch.stack([0.9 + 0.1 * f + 0.05 * torch.rand(H, W, generator=g) for f in range(2)])
    labels = torch.zeros(2, H, W, dtype=torch.int32)
    for f in range(2):
        for lab in (1, 2, 3):
            labels[f, :, (lab - 1) * W // 3:lab * W // 3] = lab
        labels[f, 0, :] = 0
    depth[0, 1, 1] = 0.0                                           # a hole inside label 1 of frame 0
    depth[1][labels[1] == 3] = 0.0
    frame_of, label_of = [0, 0, 0, 1, 1, 1], [1, 2, 3, 1, 2, 3]
    coord = torch.zeros(2, H, W, 3)
    truth = []
    for f, lab in zip(frame_of, label_of):
        q = torch.randn(4, generator=g)
        w, x, y, z = (q / q.norm()).tolist()
        R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        pts = pcl_prep.backproject_th(depth[f], K)
        sel = labels[f] == lab
        p = pts[sel]
        t = p.mean(0) if len(p) and depth[f][sel].max() > 0 else torch.zeros(3)
        s = 2.5 * (p - t).norm(dim=1).max().clamp(min=1e-3)          # coordinates end up inside [-0.5, 0.5]
        coord[f][sel] = ((p - t) @ R) / s
        truth.append((s.item(), R, t))
    return depth, K, labels, coord, frame_of, label_of, truth


@pytest.mark.parametrize("H,W", [(7, 9), (64, 64)])
def test_init_from_frames(H, W):
    depth, K, labels, coord, frame_of, label_of, truth = _frames(H, W)
    N = 64
    I = len(frame_of)
    g = torch.Generator().manual_seed(11)
    extents = (0.3 + 0.5 * torch.rand(I, 3, generator=g)).to(DEV)
    d, lab, co = depth.to(DEV), labels.to(DEV), coord.to(DEV)
    before = nocs_align.abi_call_count(), pcl_prep.abi_call_count()
    pose, scale, valid, pcl = nocs_align.init_from_frames(d, K, frame_of, co, labels=lab, label_of=label_of, extents=extents,
                                                          num_points=N, seed=4)
    assert nocs_align.abi_call_count() - before[0] == 2 and pcl_prep.abi_call_count() - before[1] == 3
    assert pose.dtype == scale.dtype == torch.float32 and tuple(pose.shape) == (I, 3, 4) and tuple(scale.shape) == (I, 3)
    assert tuple(pcl.shape) == (I, N, 3) and valid.dtype == torch.bool
    # by hand: the same clouds and pixels from sample_frames, the coordinate map gathered at them
    pcl2, pix, cnt = pcl_prep.sample_frames(d, K, frame_of, torch.zeros(I, 3, 4, device=DEV), torch.ones(I, 3, device=DEV), labels=lab,
                                            label_of=label_of, num_points=N, use_ball=False, sample="device", seed=4, return_pixels=True)
    assert torch.equal(pcl, pcl2)
    assert cnt.tolist()[5] == 0 and min(cnt.tolist()[:5]) > 0
    nocs = torch.stack([co[f].reshape(-1, 3)[pix[i].clamp(min=0).long()] for i, f in enumerate(frame_of)])
    counts = torch.where(cnt > 0, N, 0).to(torch.int32)
    pose2, scale2, valid2 = nocs_align.init_pose_from_nocs(pcl2, nocs, extents, counts=counts, seed=4)
    assert torch.equal(pose, pose2) and torch.equal(scale, scale2) and torch.equal(valid, valid2)
    assert valid.tolist() == [True] * 5 + [False]                  # the label without valid depth is invalid
    assert torch.equal(pose[5].cpu(), torch.eye(3, 4)) and torch.equal(scale[5], extents[5])
    for i in range(5):                                             # exact correspondences: the similarity comes back (fp32 inputs)
        s, R, t = truth[i]
        assert (pose[i, :, :3].cpu() - R).abs().max() < 1e-3 and (pose[i, :, 3].cpu() - t).abs().max() < 1e-3
        assert ((scale[i] / extents[i]).cpu() - s).abs().max() < 1e-3 * s
    # poses and scales feed the ball crop and the refine loop as they are
    keep = [0, 1, 2, 3, 4]
    ball = pcl_prep.sample_frames(d, K, [frame_of[i] for i in keep], pose[keep], scale[keep], labels=lab,
                                  label_of=[label_of[i] for i in keep], num_points=N, use_ball=True, sample="device", seed=4)
    assert tuple(ball.shape) == (5, N, 3) and torch.isfinite(ball).all() and (ball[..., 2] > 0).all()
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    M = 32
    cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=1, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=True)
    inputs = {k: v.to(DEV) for k, v in synth.make_inputs(5, N, M, seed=2).items()}
    inputs.update(pcl=ball, obj_pose_est=pose[keep], obj_scale_est=scale[keep])
    out = model.eval().refine(inputs, n_iter=1)
    assert tuple(out["pose_1"].shape) == (5, 3, 4) and torch.isfinite(out["pose_1"]).all() and torch.isfinite(out["scale_1"]).all()


def test_cpu_tensors_raise():
    x = torch.zeros(1, 8, 3)
    with pytest.raises(hip.CatreHipError):
        nocs_align.estimate_similarity(x, x)
    with pytest.raises(hip.CatreHipError):
        nocs_align.estimate_similarity(x.to(DEV), x.to(DEV), torch.tensor([8], dtype=torch.int32))
