"""The NOCS-map alignment without a GPU: ``tests/nocs_align_ref.py`` (the repository's numpy restatement of
``preprocess/pose_data.py:56-165``, the GPU tests' comparison target) against what the unmodified reference wrote into
``tests/golden/nocs_align.npz`` (``tools/make_align_golden.py``), the preconditions of that fixture, the evaluated draw
function, and the parts of the C ABI that need no device.

Bound on s, R, t: 1e-12 absolute.  A Jacobi-SVD restatement with another summation order differs from the reference's
(LAPACK, pairwise sums) final fit by a few 1e-16 at n = 37 ... 5000; the bound leaves three orders for FMA contraction.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from catre_amd import hip
from tests import nocs_align_ref as REF
from tests.util import GOLDEN_DIR

TOL = 1e-12
NEW_SYMBOLS = ("catre_umeyama", "catre_nocs_align", "catre_nocs_align_draws", "catre_nocs_align_workspace_bytes")
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN_DIR, "nocs_align.npz"))
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def runs(gold):
    z, meta = gold
    return [REF.estimate_similarity(z[f"c{j}/src"], z[f"c{j}/dst"], z[f"c{j}/draws"], trace=True) for j in range(len(meta["cases"]))]


def test_fixture_holds_the_cases_the_contract_names(gold):
    z, meta = gold
    got = [(c["n"], c["outliers"]) for c in meta["cases"]]
    for want in ((37, 0.2), (63, 0.3), (64, 0.3), (65, 0.3), (1000, 0.3), (1024, 0.5), (5000, 0.3), (1024, 0.95), (5, 0.0), (0, 0.0)):
        assert want in got, want
    assert [c["none"] for c in meta["cases"] if c["outliers"] == 0.95] == [True]
    assert {"m5", "m64", "m65", "m1000", "mirrored", "planar", "mask", "counts"} <= set(meta["umeyama"])
    for j, c in enumerate(meta["cases"]):
        assert z[f"c{j}/src"].dtype == np.float32 and z[f"c{j}/src"].shape == (c["n"], 3)
        if c["n"]:
            assert np.abs(z[f"c{j}/src"]).max() <= 0.5
            d = z[f"c{j}/draws"][:c["iters"]]
            assert d.min() >= 0 and d.max() < c["n"]
        if c["n"] and not c["none"] and not (c["n"] == 1024 and c["best_ratio"] < 0.2):
            # every case but the all-outlier one (and the seed that never draws five inliers) recovers the true inlier set
            assert np.array_equal(np.where(z[f"c{j}/true_inlier"])[0], z[f"c{j}/inliers"]), j


def test_restatement_reproduces_the_reference_on_its_draws(gold, runs):
    z, meta = gold
    worst = 0.0
    for j, c in enumerate(meta["cases"]):
        out, _ = runs[j]
        assert out.valid == (0 if c["none"] else 1), j
        assert out.iters == c["iters"] and out.best_it == c["best_it"], (j, out.iters, out.best_it)
        if c["n"]:
            assert np.array_equal(out.inliers, z[f"c{j}/inliers"]), j
            assert out.n_inliers == len(z[f"c{j}/inliers"])
        err = max(abs(out.scale - float(z[f"c{j}/s"])), np.abs(out.R - z[f"c{j}/R"]).max(), np.abs(out.t - z[f"c{j}/t"]).max())
        print(f"case {j} n={c['n']}: iters {out.iters} best_it {out.best_it} inliers {out.n_inliers} max |err| {err:.2e}")
        worst = max(worst, err)
        if c["none"]:
            assert out.scale == 1.0 and np.array_equal(out.R, np.eye(3)) and np.array_equal(out.t, np.zeros(3))
    assert worst <= TOL, worst


def test_preconditions_hold_on_the_stored_cases(gold, runs):
    _, meta = gold
    for j, c in enumerate(meta["cases"]):
        if not c["n"]:
            continue
        _, tr = runs[j]
        print(f"case {j}: margin {tr.margin:.2e} sigma2/sigma1 {tr.sv_ratio:.3f} stop margin {tr.stop_margin:.2e}")
        assert tr.margin >= 1e-9 and tr.sv_ratio >= 1e-3 and tr.stop_margin >= 1e-9, (j, tr)
        assert c["margin"] >= 1e-9 and c["sv_ratio"] >= 1e-3 and c["stop_margin"] >= 1e-9      # as the reference saw them


def test_umeyama_restatement_matches_the_reference(gold):
    z, meta = gold
    for name in meta["umeyama"]:
        g = {k: z[f"u/{name}/{k}"] for k in ("src", "dst", "count", "mask", "s", "R", "t")}
        keep = np.where(g["mask"][:int(g["count"])] != 0)[0]
        s, R, t, _ = REF.umeyama(g["src"][keep], g["dst"][keep])
        err = max(abs(s - float(g["s"])), np.abs(R - g["R"]).max(), np.abs(t - g["t"]).max())
        print(f"{name}: m {len(keep)} max |err| {err:.2e} det {np.linalg.det(g['R']):+.3f}")
        assert err <= TOL, (name, err)
        assert abs(np.linalg.det(g["R"]) - 1) < 1e-9
    # the mirrored pair takes the det < 0 branch: the third singular value enters the scale with a minus sign
    g = {k: z[f"u/mirrored/{k}"] for k in ("src", "dst")}
    S, T = g["src"].astype(np.float64), g["dst"].astype(np.float64)
    C = (T - T.mean(0)).T @ (S - S.mean(0)) / len(S)
    U, D, Vh = np.linalg.svd(C)
    assert np.linalg.det(U) * np.linalg.det(Vh) < 0 and D[2] > 1e-3 * D[0]


def test_degenerate_inputs_are_invalid(gold):
    z, _ = gold
    src, dst, draws = z["c0/src"], z["c0/dst"], z["c0/draws"]
    for n in (0, 1, 4):
        out = REF.estimate_similarity(src[:n], dst[:n], draws)
        assert out.valid == 0 and out.iters == 0 and out.best_it == -1 and out.scale == 1.0
    bad = dst.copy()
    bad[3, 1] = np.nan
    assert REF.estimate_similarity(src, bad, draws).valid == 0
    bad[3, 1] = np.inf
    assert REF.estimate_similarity(bad, dst, draws).valid == 0


def test_numpy_draws_are_in_range_and_uniform():
    for n, iters in ((7, 128), (1000, 128)):
        I = 400
        d = REF.draw_indices(np.full(I, n), seed=12345, max_iter=iters)
        assert d.shape == (I, iters, 5) and d.dtype == np.int32 and d.min() >= 0 and d.max() < n
        total = d.size
        cnt = np.bincount(d.ravel(), minlength=n)
        p = 1.0 / n
        sigma = np.sqrt(total * p * (1 - p))
        dev = np.abs(cnt - total * p).max() / sigma
        print(f"n={n}: {total} draws, largest bucket deviation {dev:.2f} sigma")
        assert dev <= 5.0
    a = REF.draw_indices([10, 10, 10], seed=3, keys=[5, 6, 5])
    assert np.array_equal(a[0], a[2]) and not np.array_equal(a[0], a[1])          # the key, not the slot
    assert np.array_equal(a[1], REF.draw_indices([10], seed=3, keys=[6])[0])
    assert not np.array_equal(a, REF.draw_indices([10, 10, 10], seed=4, keys=[5, 6, 5]))
    assert np.array_equal(REF.draw_indices([0, 3], seed=1)[0], np.zeros((128, 5), np.int32))
    # a known answer of Philox4x32-10 (Random123 kat_vectors: counter 0, key 0)
    w = REF.philox4x32(np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1), 0, 0)
    assert [int(x[0]) for x in w] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def test_new_symbols_are_declared_and_exported():
    lib = hip.load()
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "catre_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert n in hip.EXPORTED_SYMBOLS and hasattr(lib, n) and f"{n}(" in header, n


def test_bad_arguments_are_refused_without_a_device():
    lib = hip.load()
    buf = (ctypes.c_double * 64)()
    ok, nul = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    size = lib.catre_nocs_align_workspace_bytes
    assert size(0, 8, 128) == 0 and size(2, 0, 128) == 0 and size(-1, 8, 128) == 0 and size(2, 8, 0) == 0 and size(2, 8, 129) == 0
    assert size(2, 1 << 30, 128) == 0
    assert size(3, 8, 128) > size(2, 8, 128) > size(2, 8, 64) > 0

    def umeyama(src=ok, dst=ok, s=ok, R=ok, t=ok, I=2, N=8):
        return lib.catre_umeyama(src, dst, nul, nul, I, N, s, R, t, nul, nul)

    for kw in (dict(src=nul), dict(dst=nul), dict(s=nul), dict(R=nul), dict(t=nul), dict(I=0), dict(I=-3), dict(N=0), dict(N=-1)):
        assert umeyama(**kw) == BAD_ARG, kw

    def align(src=ok, dst=ok, ws=ok, nbytes=1 << 30, outs=(ok,) * 7, I=2, N=8, max_iter=128):
        return lib.catre_nocs_align(src, dst, nul, nul, 0, nul, I, N, max_iter, 0.99, 0.1, ws, nbytes, *outs, nul, nul)

    for kw in (dict(src=nul), dict(dst=nul), dict(ws=nul), dict(I=0), dict(N=0), dict(I=-1), dict(N=-8)):
        assert align(**kw) == BAD_ARG, kw
    for k in range(7):
        assert align(outs=tuple(nul if i == k else ok for i in range(7))) == BAD_ARG, k
    assert align(max_iter=0) == UNSUPPORTED and align(max_iter=129) == UNSUPPORTED and align(max_iter=-1) == UNSUPPORTED
    assert align(nbytes=size(2, 8, 128) - 1) == WORKSPACE and align(nbytes=0) == WORKSPACE

    draws = lib.catre_nocs_align_draws
    assert draws(nul, 0, nul, 2, 128, ok, nul) == BAD_ARG and draws(ok, 0, nul, 2, 128, nul, nul) == BAD_ARG
    assert draws(ok, 0, nul, 0, 128, ok, nul) == BAD_ARG
    assert draws(ok, 0, nul, 2, 0, ok, nul) == UNSUPPORTED and draws(ok, 0, nul, 2, 129, ok, nul) == UNSUPPORTED


def test_cpu_tensors_are_refused():
    import torch

    from catre_amd import nocs_align

    x, before = torch.zeros(2, 8, 3), nocs_align.abi_call_count()
    with pytest.raises(hip.CatreHipError):
        nocs_align.umeyama(x, x)
    with pytest.raises(hip.CatreHipError):
        nocs_align.estimate_similarity(x, x)
    with pytest.raises(hip.CatreHipError):
        nocs_align.draw_indices(torch.tensor([5, 6], dtype=torch.int32))
    with pytest.raises(hip.CatreHipError):
        nocs_align.init_pose_from_nocs(x, x, torch.ones(2, 3))
    assert nocs_align.abi_call_count() == before          # refused before any entry point is called
