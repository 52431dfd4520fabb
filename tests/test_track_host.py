"""Tracking without a GPU: ``tests/track_ref.py`` (the fp64 numpy restatement the GPU tests compare with) against what the
unmodified reference's ``lib/pysixd/pose_error.py`` wrote into ``tests/golden/pose_error_add.npz``
(``tools/make_track_golden.py``), the gate's restatement on constructed inputs, the parts of the C ABI that need no device,
the argument checks of ``catre_amd.tracking`` and the CPU-side precondition of the GPU edge test (how many neighbours it
may skip as too close to call).

Bound on ADD / ADD-S: 1e-12 absolute - the restatement repeats the reference's float64 formula; a brute-force minimum and
cKDTree's differ only in how the squared distance of a pair is summed (values are about 1e-2)."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from catre_amd import hip
from tests import track_ref as REF
from tests.util import GOLDEN_DIR

TOL = 1e-12
NEW_SYMBOLS = ("catre_nn_stats_workspace_bytes", "catre_nn_stats", "catre_track_gate")
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN_DIR, "pose_error_add.npz"))
    return z, json.loads(str(z["meta"]))


def test_fixture_holds_1_to_257_points(gold):
    z, meta = gold
    ns = [c["n"] for c in meta["cases"]]
    assert min(ns) == 1 and max(ns) == 257 and {63, 64, 65, 256} <= set(ns)
    assert any(c["sym"] for c in meta["cases"])
    for j, c in enumerate(meta["cases"]):
        assert z[f"c{j}/pts"].dtype == np.float32 and z[f"c{j}/pts"].shape == (c["n"], 3)
        for k in ("R_est", "t_est", "R_gt", "t_gt"):
            assert z[f"c{j}/{k}"].dtype == np.float32
        if c["sym"]:   # the turned estimate: ADD sees the turn, ADD-S does not
            assert float(z[f"c{j}/add"]) > 5 * float(z[f"c{j}/adi"])


def test_restatement_agrees_with_the_reference(gold):
    z, meta = gold
    worst = 0.0
    for j, c in enumerate(meta["cases"]):
        g = {k: z[f"c{j}/{k}"] for k in ("R_est", "t_est", "R_gt", "t_gt", "pts")}
        add = REF.add_error(g["R_est"], g["t_est"], g["R_gt"], g["t_gt"], g["pts"], symmetric=False)
        adi = REF.add_error(g["R_est"], g["t_est"], g["R_gt"], g["t_gt"], g["pts"], symmetric=True)
        e = max(abs(add - float(z[f"c{j}/add"])), abs(adi - float(z[f"c{j}/adi"])))
        print(f"case {j} n={c['n']}: add {add:.9f} adi {adi:.9f} max |err| {e:.2e}")
        worst = max(worst, e)
    assert worst <= TOL, worst


def test_restatement_ties_and_threshold():
    src = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    dst = np.array([[0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0]])
    r = REF.nn_stats_one(src, dst, tau=0.5)
    assert r.nn_j.tolist() == [2, 0] and r.nn_d2.tolist() == [0.0, 0.25]      # duplicates: the lowest index
    assert r.count == 2 and r.inlier == 1.0 and r.mean_d == 0.25                # d^2 == tau^2 is inside
    assert REF.nn_stats_one(src, dst, tau=0.49).count == 1
    p = REF.nn_stats_one(src, dst[:2], paired=True)
    assert p.nn_j.tolist() == [0, 1] and p.nn_d2.tolist() == [0.25, 0.25]
    pose = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]])
    assert np.array_equal(REF.apply_pose(np.array([[1.0, 2.0, 3.0]]), pose, np.array([2.0, 0.5, 1.0])), [[0.0, 4.0, 6.0]])


def test_gate_restatement():
    I = 9
    pose_new = np.tile(np.arange(12, dtype=np.float32).reshape(1, 3, 4), (I, 1, 1)) + 100
    scale_new = np.full((I, 3), 2, np.float32)
    pose_prev, scale_prev = np.zeros((I, 3, 4), np.float32), np.ones((I, 3), np.float32)
    counts = np.array([5, 0, 5, 5, 0, 5, 0, 5, 0], np.int32)
    inlier = np.array([0.5, 0.5, 0.2, 0.25, 0.1, 0.5, 0.5, 0.1, 0.1], np.float32)
    mean_d = np.array([0.01, 0.01, 0.01, 0.01, 0.01, np.inf, 0.01, 0.01, np.nan], np.float32)
    pose_new[6, 2, 1] = np.nan                                         # with an empty crop
    scale_new[7, 1] = np.inf                                           # with a low fit
    age = np.array([3, 3, 0, 7, 1, 0, 2, 0, 5], np.int32)
    E, L, N = REF.EMPTY, REF.LOW_FIT, REF.NONFINITE
    for hold in (True, False):
        p, s, st, a = REF.gate(pose_new, scale_new, pose_prev, scale_prev, counts, inlier, mean_d, 0.25, hold, age)
        assert st.tolist() == [0, E, L, 0, E | L, N, E | N, L | N, E | L | N]
        assert sorted(set(st.tolist())) == list(range(8))             # every value a status can take
        assert a.tolist() == [0, 4, 1, 0, 2, 1, 3, 1, 6]
        kept_prev = [False, hold, hold, False, hold, True, True, True, True]   # NONFINITE always holds
        for i in range(I):
            assert np.array_equal(p[i], pose_prev[i] if kept_prev[i] else pose_new[i]), (hold, i)
            assert np.array_equal(s[i], scale_prev[i] if kept_prev[i] else scale_new[i]), (hold, i)
    assert age.tolist() == [3, 3, 0, 7, 1, 0, 2, 0, 5]                 # the input is not modified


def test_edge_cases_skip_at_most_one_percent_of_neighbours():
    """The precondition of test_track.py's edge test, on the CPU: with its seed, the share of src points whose best and
    second-best neighbours are closer than twice the distance bound stays under 1 % in every case."""
    from tests import track_cases as T

    for case in T.edge_cases():
        for xf in (False, True):
            data = T.edge_data(case, xf)
            for i, r in enumerate(T.edge_reference(data)):
                bound = T.distance_bound(data, i, r)
                skipped = int((r.gap <= 2 * bound).sum()) if not data["paired"] else 0
                assert skipped <= 0.01 * len(r.gap), (case, xf, i, skipped)


def test_new_symbols_are_declared_and_exported():
    lib = hip.load()
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "catre_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert n in hip.EXPORTED_SYMBOLS and hasattr(lib, n) and f"{n}(" in header, n


def test_bad_arguments_are_refused_without_a_device():
    lib = hip.load()
    buf = (ctypes.c_double * 64)()
    ok, nul = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    size = lib.catre_nn_stats_workspace_bytes
    assert size(0, 8, 8) == 0 and size(-1, 8, 8) == 0 and size(2, 0, 8) == 0 and size(2, 8, 0) == 0 and size(2, 8, -4) == 0
    assert size(2, 1 << 30, 8) == 0 and size(2, 8, 1 << 30) == 0
    # one launch of 256-thread workgroups, one per instance and 256 src points: below 2^32 threads
    assert size((1 << 24) - 1, 256, 8) > 0 and size(1 << 24, 256, 8) == 0 and size(1 << 23, 257, 8) == 0
    assert size(1, 1, 1) > 0 and size(3, 257, 8) > size(3, 256, 8) and size(3, 8, 8) >= size(2, 8, 8)
    assert size(2, 8, 1 << 20) == size(2, 8, 1)                      # partials are per src tile

    def nn(src=ok, n_src=8, dst=ok, n_dst=8, paired=0, tau=ok, I=2, mean=ok, inlier=ok, ws=ok, nbytes=1 << 20):
        return lib.catre_nn_stats(src, n_src, dst, n_dst, nul, nul, nul, nul, paired, tau, I, mean, inlier, nul, nul, ws, nbytes, nul)

    for kw in (dict(src=nul), dict(dst=nul), dict(mean=nul), dict(I=0), dict(I=-2), dict(n_src=0), dict(n_dst=0), dict(n_src=-1),
               dict(n_dst=1 << 30), dict(I=1 << 24), dict(tau=nul)):   # ..., more workgroups than a launch takes, inlier without tau
        assert nn(**kw) == BAD_ARG, kw
    assert nn(paired=1, n_dst=9) == UNSUPPORTED and nn(paired=1, n_src=7) == UNSUPPORTED
    assert nn(nbytes=size(2, 8, 8) - 1) == WORKSPACE and nn(nbytes=0) == WORKSPACE and nn(ws=nul) == WORKSPACE

    def gate(ptrs=(ok,) * 7, outs=(ok,) * 4, I=2):
        return lib.catre_track_gate(*ptrs, 0.0, 1, I, *outs, nul)

    for k in range(7):
        assert gate(ptrs=tuple(nul if i == k else ok for i in range(7))) == BAD_ARG, k
    for k in range(4):
        assert gate(outs=tuple(nul if i == k else ok for i in range(4))) == BAD_ARG, k
    assert gate(I=0) == BAD_ARG and gate(I=-1) == BAD_ARG


def test_nn_stats_argument_checks():
    from catre_amd import tracking

    x, before = torch.zeros(2, 8, 3), tracking.abi_call_count()
    for bad in (torch.zeros(8, 3), torch.zeros(2, 8, 4), torch.zeros(2, 0, 3), torch.zeros(0, 8, 3), "no tensor"):
        with pytest.raises(ValueError):
            tracking.nn_stats(bad, x)
        with pytest.raises(ValueError):
            tracking.nn_stats(x, bad)
    with pytest.raises(ValueError):
        tracking.nn_stats(x, torch.zeros(3, 8, 3))                   # another batch
    with pytest.raises(ValueError):
        tracking.nn_stats(x, torch.zeros(2, 9, 3), paired=True)
    for kw in (dict(src_pose=torch.zeros(2, 4, 4)), dict(dst_pose=torch.zeros(3, 3, 4)), dict(src_scale=torch.zeros(2)),
               dict(dst_scale=torch.zeros(2, 4)), dict(tau=torch.zeros(3))):
        with pytest.raises(ValueError):
            tracking.nn_stats(x, x, **kw)
    with pytest.raises(ValueError):
        tracking.fit_score(x, x, torch.zeros(2, 3, 3), torch.zeros(2, 3))
    with pytest.raises(hip.CatreHipError):                           # well-formed, but not on a device: no CPU fallback
        tracking.nn_stats(x, x)
    assert tracking.abi_call_count() == before                       # refused before any entry point is called


def test_tracker_argument_checks():
    from catre_amd import tracking
    from catre_amd.config import default_cfg

    model = types.SimpleNamespace(cfg=default_cfg(num_pcl=64, num_kps=64, n_iter=2, device="cpu"))
    kps, K = torch.zeros(2, 64, 3), torch.eye(3)
    for bad in (torch.zeros(64, 3), torch.zeros(2, 64, 2)):
        with pytest.raises(ValueError):
            tracking.Tracker(model, bad, K)
    with pytest.raises(ValueError):
        tracking.Tracker(model, kps, torch.eye(4))
    with pytest.raises(ValueError):
        tracking.Tracker(model, kps, K, mean_scales=torch.zeros(3, 3))
    tr = tracking.Tracker(model, kps, K)
    assert (tr.num_points, tr.n_iter, tr.ratio) == (64, 2, 0.5)
    depth = torch.ones(48, 64)
    with pytest.raises(ValueError, match="before reset"):
        tr.step(depth)
    with pytest.raises(ValueError):
        tr.reset(torch.zeros(2, 3, 3), torch.ones(2, 3))
    with pytest.raises(ValueError):
        tr.reset(torch.zeros(2, 3, 4), torch.ones(3, 3))
    tr.reset(torch.zeros(2, 3, 4), torch.ones(2, 3))
    masks, labels = torch.ones(2, 48, 64, dtype=torch.bool), torch.zeros(48, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="not both"):
        tr.step(depth, masks=masks, labels=labels, label_of=[0, 0])
    with pytest.raises(ValueError, match="label_of"):
        tr.step(depth, labels=labels)
    with pytest.raises(ValueError):
        tr.step(depth, masks=masks, label_of=[0, 0])
    with pytest.raises(ValueError):
        tr.step(depth, masks=masks[:1])
    with pytest.raises(ValueError):
        tr.step(depth, labels=torch.zeros(2, 48, 64, dtype=torch.uint8), label_of=[0, 0])
    with pytest.raises(ValueError):
        tr.step(torch.ones(2, 48, 64))
    with pytest.raises(ValueError):
        tr.track(torch.ones(48, 64))
    with pytest.raises(hip.CatreHipError):                           # a well-formed call on CPU tensors: no CPU fallback
        tr.step(depth)
