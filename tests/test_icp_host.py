"""Trimmed ICP without a GPU: the selection rule of ``tests/icp_ref.py`` (the fp64 restatement the GPU tests compare with)
against a plain sort, exact recovery of a known offset, the CPU-side precondition of the GPU convergence test, the parts of
the C ABI that need no device and the argument checks of ``catre_amd.icp``."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from catre_amd import hip
from tests import icp_cases as C
from tests import icp_ref as REF
from tests.util import GOLDEN_DIR

NEW_SYMBOLS = ("catre_icp_workspace_bytes", "catre_icp_step", "catre_icp")
BAD_ARG, WORKSPACE = -1, -2


# ---- 1. the selection rule ------------------------------------------------------------------------------------------------
def _plain(d2, trim, tau=None):
    """the rule spelled with sorted(): candidates, then the first m of sorted((d2, k))"""
    t2 = None if tau is None else np.float32(tau) * np.float32(tau)
    cand = [(float(v), k) for k, v in enumerate(d2) if math.isfinite(v) and (t2 is None or v <= t2)]
    m = math.ceil(float(np.float32(trim)) * len(cand))
    return sorted(k for _, k in sorted(cand)[:m]), len(cand), m


def _selection_cases():
    rng = np.random.default_rng(3)
    rand = rng.uniform(0, 1, 300).astype(np.float32)
    yield "random", rand, 0.7, None
    yield "random, tau", rand, 0.5, 0.6
    yield "all equal", np.full(37, 0.25, np.float32), 0.7, None
    yield "trim 1", rand, 1.0, None
    yield "m 1", rand, 1e-6, None
    zeros = rand.copy()
    zeros[::3] = 0
    yield "zeros", zeros, 0.4, None
    yield "zeros only", np.zeros(10, np.float32), 0.3, None
    bad = rand.copy()
    bad[5], bad[17], bad[100] = np.inf, np.nan, np.inf
    yield "inf and nan", bad, 1.0, None
    yield "inf and nan, trimmed", bad, 0.7, None
    on = rand.copy()
    on[[7, 70, 200]] = np.float32(0.5) * np.float32(0.5)
    yield "tau on a value", on, 1.0, 0.5
    yield "tau on a value, boundary inside the run", np.where(on <= 0.25, np.float32(0.25), on), 0.9, 0.5
    yield "nothing inside tau", rand + 1, 0.7, 0.5


@pytest.mark.parametrize("case", list(_selection_cases()), ids=lambda c: c[0])
def test_selection_rule_against_a_plain_sort(case):
    _, d2, trim, tau = case
    want, c, m = _plain(d2, trim, tau)
    mask, c_got, m_got = REF.select(d2, tau=tau, trim=trim)
    assert (c_got, m_got) == (c, m) and np.flatnonzero(mask).tolist() == want
    assert not mask[~np.isfinite(d2)].any()
    if tau is not None and c:
        assert (d2[mask] <= np.float32(tau) * np.float32(tau)).all()


def test_selection_details():
    d2 = np.full(37, 0.25, np.float32)
    mask, c, m = REF.select(d2, trim=0.7)
    assert (c, m) == (37, 26) and np.flatnonzero(mask).tolist() == list(range(26))        # every row a tie: the lowest indices
    assert REF.select(d2, trim=1e-6)[2] == 1 and REF.select(d2, trim=1.0)[2] == 37
    on = np.array([0.3, 0.25, 0.2, 0.25, 0.26], np.float32)
    assert np.flatnonzero(REF.select(on, tau=0.5, trim=1.0)[0]).tolist() == [1, 2, 3]       # equality is inside
    assert REF.select(on, n=2, trim=1.0)[0].tolist() == [True, True, False, False, False]  # rows >= n are no candidates
    assert REF.select(on, nn_j=[0, 9, 0, -1, 0], n_dst=9, trim=1.0)[0].tolist() == [True, False, True, False, True]
    assert REF.select(on, tau=np.nan, trim=1.0)[1:] == (0, 0)
    assert REF.select(np.zeros(0, np.float32), trim=0.7)[1:] == (0, 0)
    # m = ceil((double)(float)trim * c): 0.7f is below 0.7, 0.5f is exact
    assert REF.select(np.arange(10, dtype=np.float32), trim=0.7)[2] == 7 and REF.select(np.arange(11, dtype=np.float32), trim=0.5)[2] == 6


# ---- 2. exact recovery ------------------------------------------------------------------------------------------------------
def test_exact_recovery_of_a_known_offset():
    rng = np.random.default_rng(12)
    kps = C.box_prior(1024, rng)
    scale = np.array([0.12, 0.2, 0.15])
    R, t = C.rot([1, 2, 3], 40.0), np.array([0.05, -0.1, 0.9])
    pcl = (kps[::3] * scale) @ R.T + t                                   # a subset of the posed prior, no noise
    pose0 = np.concatenate((C.rot([3, -1, 2], 5.0) @ R, (t + 0.005 * np.array([2, -1, 2]) / 3)[:, None]), 1)
    for trim in (1.0, 0.7):
        r = REF.icp(pcl, kps, pose0, scale, 60, trim=trim, dtype=np.float64)
        print("trim", trim, "rmse", r.rmse[[0, 5, 10, 20, 40, 60]], "kept", r.kept[-1])
        assert r.status == 0 and r.rmse[0] > 1e-3 and r.rmse[-1] < 1e-9
        assert np.abs(r.pose[:, :3] - R).max() < 1e-9 and np.abs(r.pose[:, 3] - t).max() < 1e-9
        assert np.array_equal(r.scale, scale)                            # rigid: the scale is carried


# ---- 3. precondition of the GPU convergence test ----------------------------------------------------------------------------
def test_trimming_is_what_makes_the_cluttered_cases_converge():
    """With the plane patch beside the object, 30 rigid iterations reach the pose only when the patch is trimmed away.
    The restatement rounds pose and distances to fp32 every iteration, as the device does."""
    cases, rows = C.convergence_inputs(), C.convergence_reference()
    assert len(cases) == 12
    for c, r in zip(cases, rows):
        (rot07, tr07), (rot10, tr10) = r["err07"], r["err10"]
        ratio = r["trim07"].sv_ratio[:-1]
        rm = r["trim07"].rmse
        print(f"seed {c['seed']} b {c['b']}: trim 0.7 {rot07:.3f} deg {1e3 * tr07:.3f} mm | trim 1.0 {rot10:.1f} deg {1e3 * tr10:.1f} mm"
              f" | min sv ratio {ratio.min():.3f} | worst rmse rise {np.max(rm[1:] / rm[:-1]) - 1:.2e}")
        assert r["trim07"].status == 0 and r["trim10"].status == 0
        assert rot07 <= 1.0 and tr07 <= 1e-3, (c["seed"], c["b"])
        assert rot10 >= 10.0, (c["seed"], c["b"])
        assert (ratio >= 1e-3).all() and (r["trim10"].sv_ratio[:-1] >= 1e-3).all()   # Jacobi and LAPACK agree there


# ---- 4. symbols and argument checks -----------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    lib = hip.load()
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "catre_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert n in hip.EXPORTED_SYMBOLS and hasattr(lib, n) and f"{n}(" in header, n
    for bit in ("CATRE_ICP_FEW = 1", "CATRE_ICP_DEGENERATE = 2", "CATRE_ICP_NONFINITE = 4", "CATRE_ICP_MAX_ITER 256"):
        assert bit in header, bit


def test_bad_arguments_are_refused_without_a_device():
    lib = hip.load()
    buf = (ctypes.c_double * 64)()
    ok, nul = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    size = lib.catre_icp_workspace_bytes
    for bad in ((0, 8, 8, 1), (-1, 8, 8, 1), (2, 0, 8, 1), (2, 8, 0, 1), (2, 8, 8, -1), (2, 8, 8, 257), (2, 1 << 30, 8, 1),
                (2, 8, 1 << 30, 1), (1 << 24, 256, 8, 1)):
        assert size(*bad) == 0, bad
    assert size(2, 8, 8, 0) > 0 and size(2, 8, 8, 256) == size(2, 8, 8, 0)          # nothing is kept per iteration
    assert size(3, 257, 8, 1) > size(3, 256, 8, 1) > lib.catre_nn_stats_workspace_bytes(3, 256, 8)
    assert size(2, 8, 1 << 20, 1) == size(2, 8, 1, 1)

    def step(pcl=ok, n_src=8, kps=ok, n_dst=8, pose=ok, scale=ok, d2=ok, j=ok, trim=0.7, update=1, I=2, pose_out=ok, scale_out=ok,
             rmse=ok, kept=ok, status=ok):
        return lib.catre_icp_step(pcl, n_src, nul, kps, n_dst, pose, scale, d2, j, nul, trim, 0, update, I, pose_out, scale_out,
                                  rmse, kept, nul, status, nul)

    def run(pcl=ok, n_src=8, kps=ok, n_dst=8, pose=ok, scale=ok, trim=0.7, n_iter=2, I=2, pose_out=ok, scale_out=ok, rmse=ok,
            kept=ok, status=ok, ws=ok, nbytes=1 << 20):
        return lib.catre_icp(pcl, n_src, nul, kps, n_dst, pose, scale, nul, trim, 0, n_iter, I, pose_out, scale_out, rmse, kept,
                             status, ws, nbytes, nul)

    shared = [dict(pcl=nul), dict(kps=nul), dict(pose=nul), dict(scale=nul), dict(rmse=nul), dict(kept=nul), dict(pose_out=nul),
              dict(scale_out=nul), dict(status=nul), dict(I=0), dict(I=-3), dict(n_src=0), dict(n_dst=0), dict(n_src=-1),
              dict(n_dst=1 << 30), dict(I=1 << 24), dict(trim=0.0), dict(trim=-0.5), dict(trim=1.0001), dict(trim=float("nan"))]
    for kw in shared + [dict(d2=nul), dict(j=nul)]:
        assert step(**kw) == BAD_ARG, kw
    for kw in shared + [dict(n_iter=-1), dict(n_iter=257)]:
        assert run(**kw) == BAD_ARG, kw
    need = size(2, 8, 8, 2)
    assert run(nbytes=need - 1) == WORKSPACE and run(nbytes=0) == WORKSPACE and run(ws=nul) == WORKSPACE


def test_python_argument_checks_come_before_any_abi_call():
    from catre_amd import icp, tracking

    pcl, kps, pose, scale = torch.zeros(2, 8, 3), torch.zeros(2, 9, 3), torch.zeros(2, 3, 4), torch.ones(2, 3)
    nn = (torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int32))
    before = (icp.abi_call_count(), tracking.abi_call_count())
    bad_common = [dict(pcl=torch.zeros(8, 3)), dict(pcl=torch.zeros(2, 8, 4)), dict(pcl=torch.zeros(0, 8, 3)), dict(pcl="no tensor"),
                  dict(kps=torch.zeros(3, 9, 3)), dict(kps=torch.zeros(2, 0, 3)), dict(pose=torch.zeros(2, 4, 4)), dict(pose=None),
                  dict(scale=torch.zeros(2)), dict(scale=None), dict(counts=torch.zeros(3, dtype=torch.int32)),
                  dict(counts=torch.zeros(2)), dict(tau=torch.zeros(3)), dict(trim=0.0), dict(trim=1.5), dict(trim=float("nan"))]
    for kw in bad_common:
        a = dict(pcl=pcl, kps=kps, pose=pose, scale=scale)
        a.update(kw)
        with pytest.raises(ValueError):
            icp.icp(**a)
        with pytest.raises(ValueError):
            icp.icp_step(nn=nn, **a)
    for kw in (dict(n_iter=-1), dict(n_iter=257), dict(tau=0.02, tau_rel=0.1)):
        with pytest.raises(ValueError):
            icp.icp(pcl, kps, pose, scale, **kw)
    for bad_nn in ((torch.zeros(2, 7), nn[1]), (nn[0], torch.zeros(2, 8)), (nn[0], torch.zeros(2, 9, dtype=torch.int32)), (None, None)):
        with pytest.raises(ValueError):
            icp.icp_step(pcl, kps, pose, scale, bad_nn)
    with pytest.raises(ValueError):
        icp.icp_step(pcl, kps, pose, scale, nn, status=torch.zeros(2))
    for call in (lambda: icp.icp(pcl, kps, pose, scale), lambda: icp.icp(pcl, kps, pose, scale, tau_rel=0.1),
                 lambda: icp.icp_step(pcl, kps, pose, scale, nn)):
        with pytest.raises(hip.CatreHipError):                           # well-formed, but not on a device: no CPU fallback
            call()
    assert (icp.abi_call_count(), tracking.abi_call_count()) == before
    assert (icp.FEW, icp.DEGENERATE, icp.NONFINITE) == (REF.FEW, REF.DEGENERATE, REF.NONFINITE)


def test_tracker_recover_arguments():
    import types

    from catre_amd import tracking
    from catre_amd.config import default_cfg

    model = types.SimpleNamespace(cfg=default_cfg(num_pcl=64, num_kps=64, n_iter=2, device="cpu"))
    kps, K = torch.zeros(2, 64, 3), torch.eye(3)
    assert tracking.Tracker(model, kps, K).recover is None
    tr = tracking.Tracker(model, kps, K, recover="icp")
    assert (tr.recover, tr.recover_iters, tr.recover_trim) == ("icp", 20, 0.7)
    for kw in (dict(recover="kalman"), dict(recover="icp", recover_iters=-1), dict(recover="icp", recover_trim=0.0),
               dict(recover="icp", recover_trim=1.2)):
        with pytest.raises(ValueError):
            tracking.Tracker(model, kps, K, **kw)
