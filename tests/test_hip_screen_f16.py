"""The fp16 screen of the pooled and run forms (kernel-form switch `screen_f16`: k_trunk4sp16 / k_trunk4sr16,
k_stn3d_pair_sp16 / _sr16, k_stnkd_pair_sp16 / _sr16 in csrc/catre_screen.h).  The screen only decides which points are
replayed in fp32, so the dense kernels (`screen` off), the split-bf16 pooled / run kernels (`screen_f16` off) and the fp16
ones must return the same bits.

Shapes - the smallest that take the full-grid forms (more than 128 tiles for the trunk, 256 pairs for the STN kernels;
smaller batches never reach a screened kernel):
  (33, 128, 128)  two tiles per cloud         (33, 100, 70)  ragged last tiles (36 and 6 valid points)
  (64, 256, 192)  256 STN pairs, the prior clouds end in a pair of one tile
Run lengths 1 (the one-tile `_sp16` kernels), 2, 3 and 16 (the `_sr16` kernels; 16 is longer than every cloud here).
Clouds: synthetic; a tile of 64 identical points in front of distinct ones and behind them (the list at, below and above
its capacity); coordinates x 1e3 and x 1e-4 (activations outside the unscaled fp16 range both ways); all-zero; one huge
point among small ones (one scale per tile: the small points sit far below the tile's largest).
The unscalable regime (row norms >= 2^75: every point a candidate, the replay alone decides) has its own test."""
import ctypes
import functools

import pytest
import torch

from tests.test_hip_screen import _batch, _model
from tests.test_hip_screen_run import _first_then_one, _one_then_distinct

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(33, 128, 128), (33, 100, 70), (64, 256, 192)]
KINDS = ["synthetic", "one_then_distinct", "first_then_one", "x1e3", "x1e-4", "zero", "huge_point"]
RUN_LENGTHS = (1, 2, 3, 16)
SWITCHES = ("screen", "screen_stn", "screen_pool", "screen_run", "screen_f16")
KEYS = ("gfeat", "pointfeat", "stn_pool", "fstn_pool")


@functools.lru_cache(maxsize=None)
def _cached_model(N, M):
    return _model(N, M)


class _Forms:
    """Set the screen switches and the run length, restore all of them on exit."""

    def __enter__(self):
        from catre_amd import hip

        self.prev = [hip.form_switch(n) for n in SWITCHES]
        self.prev_len = hip.screen_run_len()
        return self

    def set(self, screen, f16, length=0):
        from catre_amd import hip

        hip.form_switch("screen", screen)
        hip.form_switch("screen_stn", True)
        hip.form_switch("screen_pool", True)
        hip.form_switch("screen_run", True)
        hip.form_switch("screen_f16", f16)
        hip.screen_run_len(length)

    def __exit__(self, *exc):
        from catre_amd import hip

        for n, p in zip(SWITCHES, self.prev):
            hip.form_switch(n, p)
        hip.screen_run_len(self.prev_len)


def _clouds(B, N, M, kind):
    """x [B, 3, N], tfd [B, 3, M] as `pose_apply` returns them, changed per `kind`."""
    from catre_amd import runtime as RT

    batch = _batch(B, N, M, "synthetic")
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)
    x, tfd = x.permute(0, 2, 1).contiguous(), tfd.permute(0, 2, 1).contiguous()   # [B, P, 3]
    if kind == "one_then_distinct":
        x, tfd = _one_then_distinct(x), _one_then_distinct(tfd)
    elif kind == "first_then_one":
        x, tfd = _first_then_one(x), _first_then_one(tfd)
    elif kind == "x1e3":
        x, tfd = x * 1e3, tfd * 1e3
    elif kind == "x1e-4":
        x, tfd = x * 1e-4, tfd * 1e-4
    elif kind == "zero":
        x, tfd = torch.zeros_like(x), torch.zeros_like(tfd)
    elif kind == "huge_point":
        x, tfd = x.clone(), tfd.clone()
        x[:, 5] *= 1e4
        tfd[:, 37 % M] *= 1e4
    both = torch.cat([x.reshape(-1, 3), tfd.reshape(-1, 3)]).contiguous()         # one cloud-major buffer, as pose_apply's
    return both[: B * N].view(B, N, 3).permute(0, 2, 1), both[B * N:].view(B, M, 3).permute(0, 2, 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_fp16_screen_returns_the_bits_of_the_dense_and_the_split_bf16_forms(B, N, M, kind):
    model = _cached_model(N, M)
    rt = model._runtime()
    x, tfd = _clouds(B, N, M, kind)

    def run():
        st = rt.stage_pointnet(x, tfd, True)
        return {k: st[k].clone() for k in KEYS}

    with _Forms() as forms:
        forms.set(False, False)
        dense = run()
        arms = []
        for S in RUN_LENGTHS:
            forms.set(True, False, S)
            arms.append((f"bf16 S={S}", run()))
            forms.set(True, True, S)
            arms.append((f"fp16 S={S}", run()))
        torch.cuda.synchronize()
    for key in KEYS:
        assert torch.isfinite(dense[key]).all(), (B, N, M, kind, key)
        for arm, st in arms:
            assert torch.equal(dense[key], st[key]), (B, N, M, kind, arm, key, (dense[key] != st[key]).sum().item())


def _probe_trunk(rt, x, tfd, trans, t64, B, N, M):
    from catre_amd import hip

    lib = hip.load()
    pts = hip.points_desc(x, tfd)
    prm, packed = rt.params(torch.device(DEV), hip.PACK_ALL)
    ws = rt.workspace(B, N, M, torch.device(DEV))
    sp = hip.stream_ptr(torch.device(DEV))
    R, C, tiles = B * (N + M), 2 * B, B * (N + M) // 64
    scr, eps = (torch.full((tiles, 1024, 64), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
    gfeat = torch.empty(C, 1088, dtype=torch.float32, device=DEV)
    pointfeat = torch.empty(R, 64, dtype=torch.float32, device=DEV)
    hip.check(lib.catre_trunk_screen_probe(ctypes.byref(pts), hip.ptr(trans), hip.ptr(t64), prm, hip.ptr(packed),
                                           hip.ptr(scr), hip.ptr(eps), hip.ptr(gfeat), hip.ptr(pointfeat), hip.ptr(ws),
                                           ws.numel(), B, N, M, sp), "catre_trunk_screen_probe")
    torch.cuda.synchronize()
    return scr, eps, gfeat, pointfeat


def test_fp16_device_bound_holds_for_every_output_of_conv4(record_property):
    """The probe with the form on returns the fp16 S (unscaled) and its eps: |y64 - S| <= eps against the exact (float64)
    product of the saved conv3 rows with conv4's weights, and |dense fp32 - S| <= eps against the float32 matmul of the
    same rows, for all 132 x 1024 x 64 outputs.  The worst ratio is printed and recorded; measured on MI355X: 0.085 for
    both (the CPU emulation of tests/test_screen_f16_host.py saw 0.09 at K = 512)."""
    from catre_amd import hip

    B, N, M = 33, 128, 128
    model = _cached_model(N, M)
    rt = model._runtime()
    lib = hip.load()
    x, tfd = _clouds(B, N, M, "synthetic")
    st = rt.stage_pointnet(x, tfd, True)
    trans, t64 = st["trans"].contiguous(), st["trans_feat"].contiguous()
    pts = hip.points_desc(x, tfd)
    prm, packed = rt.params(torch.device(DEV), hip.PACK_ALL)
    ws = rt.workspace(B, N, M, torch.device(DEV))
    sp = hip.stream_ptr(torch.device(DEV))
    R, C, tiles = B * (N + M), 2 * B, B * (N + M) // 64

    def e(*s, dt=torch.float32):
        return torch.empty(*s, dtype=dt, device=DEV)

    x1, h1, pf, c2, c3, g, idx = e(R, 8), e(R, 64), e(R, 64), e(R, 128), e(R, 512), e(C, 1024), e(C, 1024, dt=torch.int32)
    hip.check(lib.catre_train_trunk_fwd(ctypes.byref(pts), hip.ptr(trans), hip.ptr(t64), prm, hip.ptr(packed), hip.ptr(x1),
                                        hip.ptr(h1), hip.ptr(pf), hip.ptr(c2), hip.ptr(c3), hip.ptr(g), hip.ptr(idx),
                                        hip.ptr(ws), ws.numel(), B, N, M, 0, sp), "catre_train_trunk_fwd")
    with _Forms() as forms:
        forms.set(True, False, 2)
        scr_b, eps_b, _, _ = _probe_trunk(rt, x, tfd, trans, t64, B, N, M)
        forms.set(True, True, 2)
        scr, eps, gfeat, pointfeat = _probe_trunk(rt, x, tfd, trans, t64, B, N, M)
    assert torch.equal(gfeat, st["gfeat"]) and torch.equal(pointfeat, st["pointfeat"])
    assert not torch.equal(scr, scr_b) and (eps > eps_b).all()      # it is the other screen: the probe followed the switch
    W4 = dict(model.named_parameters())["pcl_net.conv4.weight"].detach().reshape(1024, 512)
    y64 = (c3.double() @ W4.double().t()).view(tiles, 64, 1024).transpose(1, 2)
    y32 = (c3 @ W4.t()).view(tiles, 64, 1024).transpose(1, 2)
    r64 = ((y64 - scr.double()).abs() / eps.double()).max().item()
    r32 = ((y32.double() - scr.double()).abs() / eps.double()).max().item()
    record_property("largest_abs_err_over_eps_f16", r64)
    print(f"fp16 screen: largest |y64 - S| / eps = {r64:.5f}, |y32 - S| / eps = {r32:.5f} over {scr.numel()} outputs")
    assert torch.isfinite(scr).all() and torch.isfinite(eps).all() and (eps > 0).all()
    assert r64 <= 1.0 and r32 <= 1.0, (r64, r32)


def test_unscalable_tiles_take_every_point_and_keep_the_bits():
    """Row norms >= 2^75 cannot be scaled into fp16 (catre_screen.h): such a tile takes all its valid points as candidates.
    Clouds x 1e24 give conv3 / conv2 rows with norms of 1e24 and more; the trunk (identity transforms, so that nothing
    overflows fp32) and stn.conv3 must still return the dense bits.  The probe shows the regime was reached: the fp16
    accumulators of these tiles overflowed (and are ignored)."""
    from catre_amd import hip

    B, N, M = 64, 128, 128
    model = _cached_model(N, M)
    rt = model._runtime()
    lib = hip.load()
    x0, tfd0 = _clouds(B, N, M, "synthetic")
    both = torch.cat([x0.permute(0, 2, 1).reshape(-1, 3), tfd0.permute(0, 2, 1).reshape(-1, 3)]).contiguous() * 1e24
    x, tfd = both[: B * N].view(B, N, 3).permute(0, 2, 1), both[B * N:].view(B, M, 3).permute(0, 2, 1)
    C, R = 2 * B, B * (N + M)
    trans = torch.eye(3, device=DEV).repeat(C, 1, 1).contiguous()
    t64 = torch.eye(64, device=DEV).repeat(C, 1, 1).contiguous()
    pts = hip.points_desc(x, tfd)
    prm, packed = rt.params(torch.device(DEV), hip.PACK_ALL)
    ws = rt.workspace(B, N, M, torch.device(DEV))
    sp = hip.stream_ptr(torch.device(DEV))

    def run():
        gfeat = torch.empty(C, 1088, dtype=torch.float32, device=DEV)
        pointfeat = torch.empty(R, 64, dtype=torch.float32, device=DEV)
        pool = torch.empty(C, 1024, dtype=torch.float32, device=DEV)
        hip.check(lib.catre_trunk(ctypes.byref(pts), hip.ptr(trans), hip.ptr(t64), prm, hip.ptr(packed), hip.ptr(gfeat),
                                  hip.ptr(pointfeat), hip.ptr(ws), ws.numel(), B, N, M, sp), "catre_trunk")
        hip.check(lib.catre_stn3d_pool(ctypes.byref(pts), prm, hip.ptr(packed), hip.ptr(pool), hip.ptr(ws), ws.numel(),
                                       B, N, M, sp), "catre_stn3d_pool")
        return gfeat, pool

    with _Forms() as forms:
        forms.set(False, False)
        dense = run()
        got = []
        for S in (1, 2):
            forms.set(True, True, S)
            got.append(run())
        scr, eps, _, _ = _probe_trunk(rt, x, tfd, trans, t64, B, N, M)
        torch.cuda.synchronize()
    assert not torch.isfinite(scr).all()
    for d in dense:
        assert torch.isfinite(d).all() and d.abs().max().item() > 1e22
    for g in got:
        for d, v in zip(dense, g):
            assert torch.equal(d, v), (d != v).sum().item()


def test_short_refine_is_identical_with_the_switch_on_and_off():
    """K = 2, 49 objects, N = 1000, M = 360: every pose_* / scale_* slot, `screen_f16` on and off."""
    from catre_amd import hip

    B, N, M = 49, 1000, 360
    model = _cached_model(N, M)
    batch = _batch(B, N, M, "synthetic")
    prev = hip.form_switch("screen_f16")
    outs = []
    try:
        for on in (False, True):
            hip.form_switch("screen_f16", on)
            out = model.refine(batch, n_iter=2)
            outs.append({k: v.clone() for k, v in out.items() if k.startswith(("pose_", "scale_"))})
    finally:
        hip.form_switch("screen_f16", prev)
    torch.cuda.synchronize()
    assert outs[0].keys() == outs[1].keys() and len(outs[0]) == 6
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
