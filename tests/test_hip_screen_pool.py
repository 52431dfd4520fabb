"""The pooled replay of the screened max-pool (kernel-form switch `screen_pool`: k_trunk4sp, k_stn3d_pair_sp, k_stnkd_pair_sp
in csrc/catre_screen.h): one candidate list per wave instead of per-channel replay trips.  It must return the bits of the
per-channel replay (`screen_pool` off) and of the dense kernels (`screen` off).

Shapes: the smallest full grids.  (33, 128, 128): more than 128 tiles, the trunk's full-grid form.  (33, 100, 70): ragged
tiles of 36 and 6 valid points.  (64, 256, 256): 256 STN pairs.  (64, 200, 150): ragged second tiles and a one-tile pair of
22 points (M = 150).
Clouds: synthetic; every point identical (64 ties per channel: 16384 entries per wave, the list of 512 is replayed and
emptied 32 times); r copies of 64 / r distinct points, r = 2 .. 16: at least r entries per channel, r x 256 and more per
wave - below (r = 2 gives 512 if nothing else ties), around and above the list's capacity."""
import ctypes
import functools

import pytest
import torch

from tests.test_hip_screen import _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(33, 128, 128), (33, 100, 70), (64, 256, 256), (64, 200, 150)]
KINDS = ["synthetic", "identical", "copies2", "copies4", "copies8", "copies16"]


@functools.lru_cache(maxsize=None)
def _cached_model(N, M):
    return _model(N, M)


def _cloud_batch(B, N, M, kind):
    if not kind.startswith("copies"):
        return _batch(B, N, M, kind)
    r = int(kind[6:])
    d = 64 // r                  # distinct points; every tile of 64 holds each of them r times
    b = _batch(B, N, M, "synthetic")
    b["pcl"] = b["pcl"][:, :d].repeat(1, (N + d - 1) // d, 1)[:, :N].contiguous()
    b["obj_kps"] = b["obj_kps"][:, :d].repeat(1, (M + d - 1) // d, 1)[:, :M].contiguous()
    return b


def _three_arms(fn):
    """fn() dense (`screen` off), per-channel replay (`screen`, `screen_stn` on, `screen_pool` off), pooled (all on)."""
    from catre_amd import hip

    names = ("screen", "screen_stn", "screen_pool")
    prev = [hip.form_switch(n) for n in names]
    try:
        hip.form_switch("screen", False)
        dense = fn()
        hip.form_switch("screen", True)
        hip.form_switch("screen_stn", True)
        hip.form_switch("screen_pool", False)
        chan = fn()
        assert hip.form_switch("screen_pool", True) is False
        pool = fn()
        assert hip.form_switch("screen_pool") is True
    finally:
        for n, p in zip(names, prev):
            hip.form_switch(n, p)
    torch.cuda.synchronize()
    return dense, chan, pool


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_pooled_replay_returns_the_bits_of_both_other_forms(B, N, M, kind):
    from catre_amd import runtime as RT

    model = _cached_model(N, M)
    batch = _cloud_batch(B, N, M, kind)
    rt = model._runtime()
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)

    def run():
        st = rt.stage_pointnet(x, tfd, True)
        st = {k: st[k].clone() for k in ("gfeat", "pointfeat", "stn_pool", "fstn_pool")}
        out = model.refine(batch, n_iter=2)
        return st, {k: v.clone() for k, v in out.items() if k.startswith(("pose_", "scale_"))}

    (st_d, out_d), (st_c, out_c), (st_p, out_p) = _three_arms(run)
    for arm, st, out in (("dense", st_d, out_d), ("per-channel", st_c, out_c)):
        for key in ("gfeat", "pointfeat", "stn_pool", "fstn_pool"):
            assert torch.isfinite(st_p[key]).all(), (B, N, M, kind, key)
            assert torch.equal(st[key], st_p[key]), (B, N, M, kind, arm, key, (st[key] != st_p[key]).sum().item())
        for i in range(3):
            for key in (f"pose_{i}", f"scale_{i}"):
                assert torch.equal(out[key], out_p[key]), (B, N, M, kind, arm, key)


def _pool_on(fn):
    from catre_amd import hip

    names = ("screen", "screen_stn", "screen_pool")
    prev = [hip.form_switch(n) for n in names]
    try:
        for n in names:
            hip.form_switch(n, True)
        return fn()
    finally:
        for n, p in zip(names, prev):
            hip.form_switch(n, p)


def test_trunk_probe_follows_the_switch_and_returns_the_bits_of_the_plain_call():
    from catre_amd import hip
    from catre_amd import runtime as RT

    B, N, M = 33, 128, 128
    model = _cached_model(N, M)
    batch = _batch(B, N, M, "synthetic")
    rt = model._runtime()
    lib = hip.load()
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)
    R, C, tiles = B * (N + M), 2 * B, B * (N + M) // 64

    def run():
        st = rt.stage_pointnet(x, tfd, True)
        pts = hip.points_desc(x, tfd)
        prm, packed = rt.params(torch.device(DEV), hip.PACK_ALL)
        ws = rt.workspace(B, N, M, torch.device(DEV))
        sp = hip.stream_ptr(torch.device(DEV))
        trans, t64 = st["trans"].contiguous(), st["trans_feat"].contiguous()
        scr, eps = (torch.full((tiles, 1024, 64), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
        gfeat = torch.empty(C, 1088, dtype=torch.float32, device=DEV)
        pointfeat = torch.empty(R, 64, dtype=torch.float32, device=DEV)
        hip.check(lib.catre_trunk_screen_probe(ctypes.byref(pts), hip.ptr(trans), hip.ptr(t64), prm, hip.ptr(packed),
                                               hip.ptr(scr), hip.ptr(eps), hip.ptr(gfeat), hip.ptr(pointfeat), hip.ptr(ws),
                                               ws.numel(), B, N, M, sp), "catre_trunk_screen_probe")
        torch.cuda.synchronize()
        return st, scr, eps, gfeat, pointfeat

    st, scr, eps, gfeat, pointfeat = _pool_on(run)
    assert torch.equal(gfeat, st["gfeat"]) and torch.equal(pointfeat, st["pointfeat"])
    assert torch.isfinite(scr).all() and torch.isfinite(eps).all() and (eps > 0).all()


@pytest.mark.parametrize("which,name", [(0, "stn"), (1, "fstn")])
def test_stn_probe_follows_the_switch_and_returns_the_bits_of_the_plain_call(which, name):
    from catre_amd import hip
    from catre_amd import runtime as RT

    B, N, M = 64, 256, 256
    model = _cached_model(N, M)
    batch = _batch(B, N, M, "synthetic")
    rt = model._runtime()
    lib = hip.load()
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)
    C, tiles = 2 * B, B * (N + M) // 64

    def run():
        st = rt.stage_pointnet(x, tfd, True)
        pts = hip.points_desc(x, tfd)
        prm, packed = rt.params(torch.device(DEV), hip.PACK_ALL)
        ws = rt.workspace(B, N, M, torch.device(DEV))
        sp = hip.stream_ptr(torch.device(DEV))
        trans = st["trans"].contiguous()
        scr, eps = (torch.full((tiles, 1024, 64), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
        rows = torch.full((tiles, 64, 128), float("nan"), dtype=torch.float32, device=DEV)
        pooled = torch.empty(C, 1024, dtype=torch.float32, device=DEV)
        hip.check(lib.catre_stn_screen_probe(which, ctypes.byref(pts), hip.ptr(trans), prm, hip.ptr(packed), hip.ptr(scr),
                                             hip.ptr(eps), hip.ptr(rows), hip.ptr(pooled), hip.ptr(ws), ws.numel(), B, N, M,
                                             sp), "catre_stn_screen_probe")
        torch.cuda.synchronize()
        return st, scr, eps, rows, pooled

    st, scr, eps, rows, pooled = _pool_on(run)
    assert torch.equal(pooled, st[f"{name}_pool"])
    assert torch.isfinite(scr).all() and torch.isfinite(eps).all() and torch.isfinite(rows).all()
