"""Trimmed ICP on the device (``catre_amd/icp.py``, ``csrc/catre_icp.h``) against the fp64 restatement ``tests/icp_ref.py``
(pinned to a plain sort and to exact recovery by ``tests/test_icp_host.py``), and ``Tracker(recover="icp")`` against the
composition written out by hand.

Bound on pose, scale and rmse of one step: ``2^-23 |ref| + 1e-11`` - the fp64 quantities of both sides agree to the 1e-12 the
alignment tests use (1.2e-15 measured there), then the device rounds once to fp32 and the restatement does too: two
roundings of nearly the same number differ by at most one fp32 ulp.  The kept set and its size are integer and fp32-compare
arithmetic on the same inputs: they are compared for equality."""
import numpy as np
import pytest
import torch

from tests import icp_cases as C
from tests import icp_ref as REF


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(a, b):
    """torch.equal, on the bit patterns where the tensors are fp32 (an rmse over no row is NaN on both sides)"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


# ---- 1. one step against the restatement -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_src", C.STEP_N_SRC)
def test_one_step_against_the_restatement(n_src):
    worst, fits, statuses = 0.0, 0, set()
    for row in C.step_rows(n_src):
        pose, scale, rmse, kept, status, mask = row["got"]
        ref, tag = row["ref"], (row["cfg"], row["i"])
        assert np.array_equal(mask.astype(bool), ref.mask), tag
        assert int(kept) == ref.kept == int(mask.sum()), tag
        assert int(status) == ref.status, (tag, int(status), ref.status)
        statuses.add(int(status))
        if ref.status:                                                  # passes through bit for bit
            assert np.array_equal(_bits(pose), _bits(row["pose_in"])) and np.array_equal(_bits(scale), _bits(row["scale_in"])), tag
        else:
            fits += 1
            assert ref.sv_ratio >= 1e-3, (tag, ref.sv_ratio)            # where Jacobi and LAPACK agree (tools/make_align_golden.py)
            assert not np.array_equal(_bits(pose), _bits(row["pose_in"])), tag
            if not row["cfg"][4]:
                assert np.array_equal(_bits(scale), _bits(row["scale_in"])), tag   # rigid: sigma = 1 exactly
        ratio = C.step_ratio(row)
        assert ratio <= 1.0, (tag, ratio)
        worst = max(worst, ratio)
    assert fits >= 8 and statuses >= {0, REF.FEW}, (fits, statuses)
    print(f"n_src {n_src}: worst |device - restatement| / bound {worst:.3f} over {fits} fits")


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_on_a_lattice():
    from catre_amd import icp

    d = C.lattice_data()
    nn = C.device_nn(d)
    d2, nj = nn.nn_d2.cpu().numpy(), nn.nn_j.cpu().numpy()
    args = [C.dev(d[k]) for k in ("pcl", "kps", "pose", "scale")]
    tau = np.full(2, 7 / 128, np.float32)                               # tau^2 = 49 / 2^14: exact, and a value d2 takes
    inside_a_run = 0
    for trim in (0.3, 0.5, 0.7, 0.9, 1.0):
        for t in (None, tau):
            got = icp.icp_step(*args, nn, counts=C.dev(d["counts"]), tau=C.dev(t), trim=trim, return_mask=True)
            for i in range(2):
                m64 = d2[i].astype(np.float64) * 2 ** 14
                assert np.array_equal(m64, np.round(m64)) and m64.max() < 2 ** 24      # exact in fp32 as claimed
                n = int(d["counts"][i])
                assert (d2[i][:n] == tau[i] * tau[i]).sum() >= 2, "the seed must put pairs on the threshold"
                ref = REF.step(d["pcl"][i], d["kps"][i], d["pose"][i], d["scale"][i], d2[i], nj[i], n, None if t is None else t[i], trim)
                mask = got.mask[i].cpu().numpy().astype(bool)
                assert np.array_equal(mask, ref.mask) and int(got.kept[i]) == ref.kept, (trim, t is not None, i)
                assert not mask[n:].any()
                if t is not None:
                    assert mask[:n][d2[i][:n] == tau[i] * tau[i]].any() or trim < 1.0
                    assert not mask[d2[i] > tau[i] * tau[i]].any()
                # the boundary value: of the candidates that have it, the lowest indices are kept
                edge = d2[i][mask].max()
                cand = np.flatnonzero((np.arange(len(mask)) < n) & (d2[i] == edge) & ((d2[i] <= tau[i] * tau[i]) if t is not None else True))
                k_in = int(mask[cand].sum())
                assert mask[cand[:k_in]].all() and not mask[cand[k_in:]].any()
                inside_a_run += 0 < k_in < len(cand)
    assert inside_a_run >= 4, inside_a_run                               # the trim boundary fell inside a run of equal values


# ---- 3. status ---------------------------------------------------------------------------------------------------------------
def _status_data():
    d = C.step_data(257, I=4, seed=5)
    d["counts"] = np.array([257, 2, 257, 257], np.int32)                 # instance 1: FEW
    line = np.zeros((C.N_DST, 3), np.float32)                            # instance 2: prior and points on one line
    line[:, 0] = np.linspace(-0.5, 0.5, C.N_DST, dtype=np.float32)
    d["kps"][2] = line
    d["pose"][2] = np.eye(3, 4, dtype=np.float32)
    d["scale"][2] = 1.0
    d["pcl"][2] = 0
    d["pcl"][2][:, 0] = np.linspace(-0.4, 0.4, 257, dtype=np.float32) + np.float32(0.01)
    d["pose"][3][1, 2] = np.nan                                          # instance 3: NONFINITE
    d["pcl"][0][11] = np.nan                                             # a NaN observed point in a normal instance
    return d


@pytest.mark.gpu
def test_status_bits_pass_the_pose_through_and_stick():
    from catre_amd import icp

    d = _status_data()
    nn = C.device_nn(d)
    args = [C.dev(d[k]) for k in ("pcl", "kps", "pose", "scale")]
    s = icp.icp_step(*args, nn, counts=C.dev(d["counts"]), return_mask=True)
    st = s.status.cpu().tolist()
    assert st[0] == 0 and st[1] == REF.FEW, st
    assert st[2] & REF.DEGENERATE and not st[2] & REF.FEW, st
    assert st[3] & REF.NONFINITE, st
    assert s.kept.cpu().tolist()[1] == 2 and s.kept.cpu().tolist()[3] == 0
    assert not bool(s.mask[0, 11]) and int(s.kept[0]) == int(np.ceil(float(np.float32(0.7)) * 256))   # the NaN row is no candidate
    assert torch.isfinite(s.pose[0]).all() and not torch.equal(s.pose[0], args[2][0])
    for i in (1, 2, 3):                                                  # bit for bit, the NaN included
        assert np.array_equal(_bits(s.pose[i].cpu().numpy()), _bits(d["pose"][i])), i
        assert np.array_equal(_bits(s.scale[i].cpu().numpy()), _bits(d["scale"][i])), i
    assert np.isfinite(s.rmse.cpu().numpy()[:3]).all()                   # rmse and kept are still reported
    # the loop: the bits stay, the poses still pass through after further iterations
    for with_scale in (False, True):
        r = icp.icp(*args, n_iter=4, counts=C.dev(d["counts"]), estimate_scale=with_scale)
        rs = r.status.cpu().tolist()
        assert rs[0] == 0 and rs[1] == REF.FEW and rs[2] & REF.DEGENERATE and rs[3] & REF.NONFINITE, rs
        for i in (1, 2, 3):
            assert np.array_equal(_bits(r.pose[i].cpu().numpy()), _bits(d["pose"][i])), i
            assert np.array_equal(_bits(r.scale[i].cpu().numpy()), _bits(d["scale"][i])), i
        assert torch.equal(r.kept[:, 1], torch.full((5,), 2, dtype=torch.int32, device="cuda"))
    # an earlier bit alone holds a pose that would otherwise move; the caller's status tensor is not modified
    earlier = torch.tensor([REF.DEGENERATE, 0, 0, 0], dtype=torch.int32, device="cuda")
    h = icp.icp_step(*args, nn, counts=C.dev(d["counts"]), status=earlier)
    assert h.status.cpu().tolist()[0] == REF.DEGENERATE and torch.equal(h.pose[0], args[2][0]) and torch.equal(h.scale[0], args[3][0])
    assert earlier.cpu().tolist() == [REF.DEGENERATE, 0, 0, 0]
    assert _same(h.rmse, s.rmse) and torch.equal(h.kept, s.kept)
    # update=False measures only
    e = icp.icp_step(*args, nn, counts=C.dev(d["counts"]), update=False, return_mask=True)
    assert _same(e.rmse, s.rmse) and torch.equal(e.kept, s.kept) and torch.equal(e.mask, s.mask)
    assert e.pose.data_ptr() == args[2].data_ptr() and e.status.cpu().tolist() == [0, 0, 0, 0]


# ---- 4. composition ------------------------------------------------------------------------------------------------------------
def _by_hand(args, n_iter, counts, tau, trim, with_scale):
    from catre_amd import icp, tracking

    pcl, kps, pose, scale = args
    status, rmse, kept = None, [], []
    for it in range(n_iter + 1):
        nn = tracking.nn_stats(pcl, kps, dst_pose=pose, dst_scale=scale, return_nn=True)
        s = icp.icp_step(pcl, kps, pose, scale, nn, counts=counts, tau=tau, trim=trim, estimate_scale=with_scale,
                         update=it < n_iter, status=status)
        pose, scale, status = s.pose, s.scale, s.status
        rmse.append(s.rmse), kept.append(s.kept)
    return pose, scale, torch.stack(rmse), torch.stack(kept), status


@pytest.mark.gpu
@pytest.mark.parametrize("with_scale", [False, True], ids=["rigid", "similarity"])
def test_loop_equals_the_steps_issued_one_by_one(with_scale):
    from catre_amd import icp

    n_src = 1024 + 44
    d = C.step_data(n_src)
    args = [C.dev(d[k]) for k in ("pcl", "kps", "pose", "scale")]
    counts = C.dev(np.array([n_src, 0, n_src // 2, 700], np.int32))
    for tau in (None, C.dev(d["tau"])):
        before = icp.abi_call_count()
        got = icp.icp(*args, n_iter=3, counts=counts, tau=tau, trim=0.7, estimate_scale=with_scale)
        assert icp.abi_call_count() - before == 2                        # the workspace query and ONE call, whatever n_iter
        want = _by_hand(args, 3, counts, tau, 0.7, with_scale)
        for g, w, name in zip(got, want, got._fields):
            assert _same(g, w), name
        assert got.status.cpu().tolist() == [0, REF.FEW, 0, 0]
        assert not torch.equal(got.pose[0], args[2][0]) and torch.equal(got.pose[1], args[2][1])
        assert (got.scale[0] != args[3][0]).any() == with_scale
    # tau_rel is tau = tau_rel * |scale| of the incoming scale, formed on the device; a float tau is that value for all
    rel = icp.icp(*args, n_iter=2, tau_rel=0.1)
    same = icp.icp(*args, n_iter=2, tau=0.1 * torch.linalg.vector_norm(args[3], dim=1))
    assert all(_same(a, b) for a, b in zip(rel, same))
    flt = icp.icp(*args, n_iter=2, tau=0.02)
    assert all(_same(a, b) for a, b in zip(flt, icp.icp(*args, n_iter=2, tau=C.dev(d["tau"]))))
    # no iteration at all: the pose as it came and its fit
    zero = icp.icp(*args, n_iter=0, counts=counts)
    assert torch.equal(zero.pose, args[2]) and torch.equal(zero.scale, args[3]) and tuple(zero.rmse.shape) == (1, 4)
    one = icp.icp(*args, n_iter=1, counts=counts)
    assert _same(zero.rmse[0], one.rmse[0]) and torch.equal(zero.kept[0], one.kept[0]) and zero.status.cpu().tolist() == [0] * 4


# ---- 5. batch independence -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_independence():
    from catre_amd import icp

    d = C.step_data(1024 + 44)
    counts = C.full_counts(1024 + 44)
    args = [C.dev(d[k]) for k in ("pcl", "kps", "pose", "scale")]
    whole = icp.icp(*args, n_iter=3, counts=C.dev(counts), tau=C.dev(d["tau"]), estimate_scale=True)
    step = icp.icp_step(*args, C.device_nn(d), counts=C.dev(counts), return_mask=True)
    for i in range(4):
        one = [a[i:i + 1].contiguous() for a in args]
        alone = icp.icp(*one, n_iter=3, counts=C.dev(counts[i:i + 1]), tau=C.dev(d["tau"][i:i + 1]), estimate_scale=True)
        for f in ("pose", "scale", "status"):
            assert torch.equal(getattr(whole, f)[i:i + 1], getattr(alone, f)), (i, f)
        assert torch.equal(whole.rmse[:, i:i + 1], alone.rmse) and torch.equal(whole.kept[:, i:i + 1], alone.kept), i
        d1 = {k: d[k][i:i + 1] for k in ("pcl", "kps", "pose", "scale")}
        s1 = icp.icp_step(*one, C.device_nn(d1), counts=C.dev(counts[i:i + 1]), return_mask=True)
        for f in ("pose", "scale", "rmse", "kept", "status", "mask"):
            assert torch.equal(getattr(step, f)[i:i + 1], getattr(s1, f)), (i, f)


# ---- 6. convergence --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_convergence_with_and_without_the_trim():
    """The device against the restatement on the cluttered cases of the host test: the same basin, not the same path.

    rmse may not rise from one iteration to the next beyond 1e-5 relative.  In exact arithmetic it cannot rise at all:
    re-matching, re-selecting and re-fitting each lower the trimmed sum or leave it.  The device rounds the pose to fp32
    every iteration - at the optimum a second-order effect, (6e-8 m)^2 / rmse, about 1e-9 relative as the restatement shows
    (``test_icp_host.py``) - and forms every distance in fp32 from fp32 posed points: about 2e-8 m on a 2 mm distance per
    point, 1e-5, which averages over the ~540 kept points to under 1e-6.  Measured: 8.6e-8 at worst."""
    from catre_amd import icp

    cases, rows = C.convergence_inputs(), C.convergence_reference()
    worst_rise = 0.0
    for s0 in range(0, len(cases), 4):
        batch = cases[s0:s0 + 4]
        args = [C.dev(np.stack([c[k] for c in batch])) for k in ("pcl", "kps", "pose", "scale")]
        r07 = icp.icp(*args, n_iter=C.CONV_ITERS, trim=0.7)
        r10 = icp.icp(*args, n_iter=C.CONV_ITERS, trim=1.0)
        assert r07.status.cpu().tolist() == [0] * 4 and r10.status.cpu().tolist() == [0] * 4
        assert torch.equal(r07.scale, args[3])                           # rigid: the scale is held
        rm = r07.rmse.cpu().numpy().astype(np.float64)
        worst_rise = max(worst_rise, float(np.max(rm[1:] / rm[:-1])) - 1.0)
        assert (rm[1:] <= rm[:-1] * (1 + 1e-5)).all(), np.max(rm[1:] / rm[:-1]) - 1
        for i, c in enumerate(batch):
            ref = rows[s0 + i]
            rot07, tr07 = C.pose_errors(r07.pose[i].cpu().numpy(), c)
            rot10, _ = C.pose_errors(r10.pose[i].cpu().numpy(), c)
            print(f"seed {c['seed']} b {c['b']}: device {rot07:.3f} deg {1e3 * tr07:.3f} mm, restatement {ref['err07'][0]:.3f} deg "
                  f"{1e3 * ref['err07'][1]:.3f} mm; untrimmed {rot10:.1f} deg")
            assert rot07 <= 2 * ref["err07"][0] + 0.1 and tr07 <= 2 * ref["err07"][1] + 1e-4, (c["seed"], c["b"])
            assert rot10 >= 10.0, (c["seed"], c["b"])
    print(f"worst rise of rmse between iterations: {worst_rise:.2e} relative")


# ---- 7. the tracker ----------------------------------------------------------------------------------------------------------------
N_PTS, N_ITER, H, W, T = 64, 2, 48, 64, 3


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
    scene = synth.make_depth_scene(H=H, W=W, n_inst=2, seed=3)
    inputs = synth.make_inputs(2, N_PTS, N_PTS, seed=9)
    depth = torch.stack([torch.where(scene["depth"] > 0, scene["depth"] + 0.003 * t, scene["depth"]) for t in range(T)])
    return dict(model=model, kps=inputs["obj_kps"].cuda(), mean_scales=inputs["obj_mean_scales"].cuda(), K=scene["K"],
                depth=depth.cuda(), pose0=scene["poses"].cuda(), scale0=scene["scales"].cuda())


def _tracker(rig, **kw):
    from catre_amd import tracking

    tr = tracking.Tracker(rig["model"], rig["kps"], rig["K"], mean_scales=rig["mean_scales"], seed=11, **kw)
    return tr.reset(rig["pose0"], rig["scale0"])


def _by_hand_track(rig, recover, tau_rel=0.1, iters=20, trim=0.7):
    """sample_frames -> refine -> fit_score (-> icp from the carried pose -> fit_score -> rule -> where) -> gate"""
    from catre_amd import icp, pcl_prep, tracking

    pose, scale = rig["pose0"].clone(), rig["scale0"].clone()
    age = torch.zeros(2, dtype=torch.int32, device="cuda")
    Kd = rig["K"].cuda().expand(2, 3, 3).contiguous()
    zero = torch.zeros(1, H, W, dtype=torch.uint8, device="cuda")
    steps = []
    for t in range(T):
        pcl, _, counts = pcl_prep.sample_frames(rig["depth"][t:t + 1], rig["K"], [0, 0], pose, scale, ratio=0.5, num_points=N_PTS,
                                                use_ball=True, sample="device", seed=11 + t, return_pixels=True, labels=zero,
                                                label_of=[0, 0])
        out = rig["model"].refine({"pcl": pcl, "obj_kps": rig["kps"], "obj_pose_est": pose, "obj_scale_est": scale, "K": Kd,
                                   "obj_mean_scales": rig["mean_scales"]}, n_iter=N_ITER)
        pose_n, scale_n = out[f"pose_{N_ITER}"], out[f"scale_{N_ITER}"]
        score = tracking.fit_score(pcl, rig["kps"], pose_n, scale_n, tau_rel)
        step = {}
        if recover:
            cand = icp.icp(pcl, rig["kps"], pose, scale, n_iter=iters, trim=trim)
            score_c = tracking.fit_score(pcl, rig["kps"], cand.pose, cand.scale, tau_rel)
            take = (cand.status == 0) & ~(score.inlier_obs >= score_c.inlier_obs)
            pose_n = torch.where(take[:, None, None], cand.pose, pose_n)
            scale_n = torch.where(take[:, None], cand.scale, scale_n)
            step = dict(score_refine=score, score_icp=score_c)
            score = tracking.FitScore(*(torch.where(take, c, r) for c, r in zip(score_c, score)))
            step.update(recovered=take, icp=cand)
        pose, scale, status, age = tracking.track_gate(pose_n, scale_n, pose, scale, counts, score.inlier_obs, score.d_obs, age,
                                                       0.0, True)
        step.update(pose=pose, scale=scale, pose_iters=torch.stack([out[f"pose_{i}"] for i in range(N_ITER + 1)]), score=score,
                    status=status, age=age, pcl=pcl)
        steps.append(step)
    return steps


def _same_step(a, b):
    for k in ("pose", "scale", "pose_iters", "status", "age", "pcl"):
        assert torch.equal(a[k], b[k]), k
    for f in ("d_obs", "inlier_obs", "d_prior"):
        assert torch.equal(getattr(a["score"], f), getattr(b["score"], f)), f


@pytest.mark.gpu
def test_tracker_recovery_equals_the_composition(rig):
    from catre_amd import icp, pcl_prep, tracking

    # tau_rel 0.1: the scores decide; tau_rel 1e-9: nothing lies within tau, both inlier shares are 0 and `>=` keeps the refine
    wants = {}
    for tau_rel in (0.1, 1e-9):
        want = wants[tau_rel] = _by_hand_track(rig, True, tau_rel)
        tr = _tracker(rig, recover="icp", tau_rel=tau_rel)
        for t in range(T):
            got = tr.step(rig["depth"][t])
            _same_step(got, want[t])
            assert got["recovered"].dtype == torch.bool and torch.equal(got["recovered"], want[t]["recovered"])
            for g, w in zip(got["icp"], want[t]["icp"]):
                assert torch.equal(g, w)
            # the rule, on the scores of the two candidates
            ref, cand = want[t]["score_refine"], want[t]["score_icp"]
            rule = (got["icp"].status == 0) & ~(ref.inlier_obs >= cand.inlier_obs)
            assert torch.equal(got["recovered"], rule)
            sel = torch.where(got["recovered"], cand.inlier_obs, ref.inlier_obs)
            assert torch.equal(got["score"].inlier_obs, sel)
            print("tau_rel", tau_rel, "frame", t, "recovered", got["recovered"].tolist(), "refine", ref.inlier_obs.tolist(), "icp",
                  cand.inlier_obs.tolist(), "status", got["status"].tolist())
            if tau_rel == 1e-9:
                assert got["recovered"].tolist() == [False, False]
    # a Tracker() beside it: the bits and the ABI calls it had before
    plain_want = _by_hand_track(rig, False)
    plain, rec = _tracker(rig), _tracker(rig, recover="icp")
    plain.step(rig["depth"][0]), rec.step(rig["depth"][0])
    _same_step(_tracker(rig).step(rig["depth"][0]), plain_want[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                              # no device -> host copy in either
    try:
        grown = []
        for tr in (plain, rec, plain, rec):
            before = (pcl_prep.abi_call_count(), tracking.abi_call_count(), icp.abi_call_count())
            res = tr.step(rig["depth"][1 if len(grown) < 2 else 2])
            grown.append((pcl_prep.abi_call_count() - before[0], tracking.abi_call_count() - before[1], icp.abi_call_count() - before[2]))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert grown[0] == grown[2] and grown[1] == grown[3], grown
    assert grown[0][1:] == (5, 0) and grown[1][1:] == (9, 2) and grown[0][0] == grown[1][0], grown
    assert "recovered" in res and "icp" in res
    seq = _tracker(rig, recover="icp").track(rig["depth"])
    assert tuple(seq["recovered"].shape) == (T, 2) and tuple(seq["icp"].rmse.shape) == (T, 21, 2)
    for t in range(T):
        assert torch.equal(seq["pose"][t], wants[0.1][t]["pose"]) and torch.equal(seq["recovered"][t], wants[0.1][t]["recovered"])
