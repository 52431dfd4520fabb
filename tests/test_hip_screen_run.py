"""The run form of the screened max-pool (kernel-form switch `screen_run`: k_trunk4sr, k_stn3d_pair_sr, k_stnkd_pair_sr in
csrc/catre_screen.h): a workgroup walks up to S consecutive tiles (S / 2 pairs) of one cloud and carries the exact running
maximum, so that a tile replays only the points that can still beat it.  It must return the bits of the pooled form with
`screen_run` off and of the dense kernels (`screen` off), for every run length.

Shapes, the smallest full grids where a run can go wrong:
  (33, 128, 128)   runs of 2; S = 16 longer than the cloud        (33, 100, 70)    a run that ends in a ragged tile (36 / 6)
  (9, 1024, 1024)  whole-cloud runs                                (9, 960, 448)    15 and 7 tiles: short last runs
  (9, 1000, 500)   ragged last tile of a long run                  (64, 256, 256)   runs of pairs
  (64, 200, 150)   runs of pairs, ragged                           (22, 960, 448)   264 pairs, a last pair of one tile
Clouds: synthetic; identical (every point ties with the running maximum: the list overflows with a finite running
maximum); copies4; first_then_one (tile 0 distinct, every later tile 64 copies of one of its points: most channels of the
later tiles have no candidate, a few carry 64 ties, some waves get an empty list); one_then_distinct (the reverse: the
running maximum comes from an all-ties tile, then most channels are beaten)."""
import ctypes
import functools

import pytest
import torch

from tests.test_hip_screen import _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(33, 128, 128), (33, 100, 70), (9, 1024, 1024), (9, 960, 448), (9, 1000, 500), (64, 256, 256), (64, 200, 150),
          (22, 960, 448)]
KINDS = ["synthetic", "identical", "copies4", "first_then_one", "one_then_distinct"]
RUN_LENGTHS = (2, 3, 4, 16)
SWITCHES = ("screen", "screen_stn", "screen_pool", "screen_run")


@functools.lru_cache(maxsize=None)
def _cached_model(N, M):
    return _model(N, M)


def _first_then_one(c):
    """[B, P, 3]: tile 0 as it is, tile t >= 1 = 64 copies of point t % 64 of tile 0."""
    P = c.shape[1]
    idx = torch.arange(P)
    src = torch.where(idx < 64, idx, (idx // 64) % 64).clamp_(max=min(P, 64) - 1)
    return c[:, src].contiguous()


def _one_then_distinct(c):
    """[B, P, 3]: tile 0 = 64 copies of point 0, the later tiles as they are."""
    c = c.clone()
    c[:, :64] = c[:, :1]
    return c


def _cloud_batch(B, N, M, kind):
    if kind in ("synthetic", "identical"):
        return _batch(B, N, M, kind)
    b = _batch(B, N, M, "synthetic")
    if kind == "copies4":
        b["pcl"] = b["pcl"][:, :16].repeat(1, (N + 15) // 16, 1)[:, :N].contiguous()
        b["obj_kps"] = b["obj_kps"][:, :16].repeat(1, (M + 15) // 16, 1)[:, :M].contiguous()
    else:
        f = _first_then_one if kind == "first_then_one" else _one_then_distinct
        b["pcl"], b["obj_kps"] = f(b["pcl"]), f(b["obj_kps"])
    return b


class _Forms:
    """Set the four switches and the run length, restore all of them on exit."""

    def __enter__(self):
        from catre_amd import hip

        self.prev = [hip.form_switch(n) for n in SWITCHES]
        self.prev_len = hip.screen_run_len()
        return self

    def set(self, screen, run, length=0):
        from catre_amd import hip

        hip.form_switch("screen", screen)
        hip.form_switch("screen_stn", True)
        hip.form_switch("screen_pool", True)
        hip.form_switch("screen_run", run)
        hip.screen_run_len(length)

    def __exit__(self, *exc):
        from catre_amd import hip

        for n, p in zip(SWITCHES, self.prev):
            hip.form_switch(n, p)
        hip.screen_run_len(self.prev_len)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_run_form_returns_the_bits_of_both_other_forms(B, N, M, kind):
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

    with _Forms() as forms:
        forms.set(False, False)
        arms = [("dense", run())]
        forms.set(True, False)
        arms.append(("pooled", run()))
        runs = []
        for S in RUN_LENGTHS:
            forms.set(True, True, S)
            runs.append((S, run()))
        torch.cuda.synchronize()
    for S, (st_r, out_r) in runs:
        for arm, (st, out) in arms:
            for key in ("gfeat", "pointfeat", "stn_pool", "fstn_pool"):
                assert torch.isfinite(st_r[key]).all(), (B, N, M, kind, S, key)
                assert torch.equal(st[key], st_r[key]), (B, N, M, kind, S, arm, key, (st[key] != st_r[key]).sum().item())
            for i in range(3):
                for key in (f"pose_{i}", f"scale_{i}"):
                    assert torch.equal(out[key], out_r[key]), (B, N, M, kind, S, arm, key)


def test_run_len_round_trips_and_zero_restores_the_rule():
    from catre_amd import hip

    prev = hip.screen_run_len()
    try:
        hip.screen_run_len(0)
        assert hip.screen_run_len() == 0
        for S in (1, 2, 3, 7, 16):
            hip.screen_run_len(S)
            assert hip.screen_run_len() == S          # a query changes nothing
            assert hip.screen_run_len() == S
        assert hip.screen_run_len(40) == 16 and hip.screen_run_len() == 16   # clamped to the longest run
        assert hip.screen_run_len(0) == 16 and hip.screen_run_len() == 0
    finally:
        hip.screen_run_len(prev)
    assert hip.form_switch("screen_run") in (True, False)
    assert hip.FORM_IDS["screen_run"] == 8


def _run_on(fn, length):
    with _Forms() as forms:
        forms.set(True, True, length)
        return fn()


@pytest.mark.parametrize("length", [2, 16])
def test_trunk_probe_follows_the_switch_and_returns_the_bits_of_the_plain_call(length):
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

    st, scr, eps, gfeat, pointfeat = _run_on(run, length)
    assert torch.equal(gfeat, st["gfeat"]) and torch.equal(pointfeat, st["pointfeat"])
    # S and eps do not depend on the running maximum: every tile of a run reports them
    assert torch.isfinite(scr).all() and torch.isfinite(eps).all() and (eps > 0).all()


@pytest.mark.parametrize("which,name", [(0, "stn"), (1, "fstn")])
def test_stn_probe_returns_the_bits_of_the_plain_call_with_the_switch_on(which, name):
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

    st, scr, eps, rows, pooled = _run_on(run, 4)
    assert torch.equal(pooled, st[f"{name}_pool"])
    assert torch.isfinite(scr).all() and torch.isfinite(eps).all() and torch.isfinite(rows).all()
