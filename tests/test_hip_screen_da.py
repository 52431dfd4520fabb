"""`screen_da` / `screen_da_stn` on the device (csrc/catre_screen.h): the fp16-screen kernels select with an eps that takes
the activations' rounding as measured per tile and the weights' error split by sign.  The bound only decides which points
are replayed in fp32, so switch off, switch on and the dense form (`screen` off) must return the same bits, and the probes
must show |y64 - S| < eps with the new eps for every output.

Shapes (B, N, M): (2, 64, 64), (3, 100, 64) with ragged last tiles and (2, 192, 128) - grids of a few tiles, which take the
dense eight-workgroups-per-tile kernels under every switch (the screened forms exist for grids of more than 128 tiles): they
pin that the switches change nothing there.  (33, 128, 128) and (33, 100, 70) - ragged: 36 and 6 valid points - are the
smallest that reach the screened trunk, (64, 256, 192) the smallest that reaches the screened STN pair kernels (256 pairs;
the prior clouds end in a pair of one tile), as in tests/test_hip_screen_f16.py, whose cloud kinds and run lengths are
used: 1 (the one-tile kernels), 2, 3, 16."""
import ctypes

import pytest
import torch

from tests.test_hip_screen import _batch
from tests.test_hip_screen_f16 import (DEV, KEYS, RUN_LENGTHS, _cached_model, _clouds, _Forms, _probe_trunk)

pytestmark = pytest.mark.gpu

SMALL = [(2, 64, 64), (3, 100, 64), (2, 192, 128)]
SCREENED = [(33, 128, 128), (33, 100, 70), (64, 256, 192)]
KINDS = ["synthetic", "one_then_distinct", "first_then_one", "x1e3", "x1e-4", "zero", "huge_point"]
ARMS = ((False, False), (True, False), (True, True))      # (screen_da, screen_da_stn)


class _Da:
    """Set `screen_da` and its STN arm, restore both on exit."""

    def __enter__(self):
        from catre_amd import hip

        self.prev = [hip.form_switch(n) for n in ("screen_da", "screen_da_stn")]
        return self

    def set(self, da, stn):
        from catre_amd import hip

        hip.form_switch("screen_da", da)
        hip.form_switch("screen_da_stn", stn)

    def __exit__(self, *exc):
        from catre_amd import hip

        for n, p in zip(("screen_da", "screen_da_stn"), self.prev):
            hip.form_switch(n, p)


def test_the_switches_read_back_and_are_no_bits_of_the_form_word():
    from catre_amd import hip

    with _Da() as da:
        da.set(True, True)
        assert hip.form_switch("screen_da", False) is True and hip.form_switch("screen_da") is False
        assert hip.form_switch("screen_da_stn", False) is True and hip.form_switch("screen_da_stn") is False
        word = sum(1 << b for b in range(13) if b not in (3, 4))
        a = hip.form_decision("trunk", "fp32", 256, 1024, 1024, word)
        da.set(True, True)
        assert hip.form_decision("trunk", "fp32", 256, 1024, 1024, word) == a and a[0] == "run_f16"


def _compare(B, N, M, kind, lengths):
    model = _cached_model(N, M)
    rt = model._runtime()
    x, tfd = _clouds(B, N, M, kind)

    def run():
        st = rt.stage_pointnet(x, tfd, True)
        return {k: st[k].clone() for k in KEYS}

    with _Forms() as forms, _Da() as da:
        forms.set(False, True)
        dense = run()
        arms = []
        for S in lengths:
            forms.set(True, True, S)
            for on, stn in ARMS:
                da.set(on, stn)
                arms.append((f"da={int(on)} stn={int(stn)} S={S}", run()))
        torch.cuda.synchronize()
    for key in KEYS:
        assert torch.isfinite(dense[key]).all(), (B, N, M, kind, key)
        for arm, st in arms:
            assert torch.equal(dense[key], st[key]), (B, N, M, kind, arm, key, (dense[key] != st[key]).sum().item())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,M", SCREENED)
def test_pooled_features_keep_the_bits_of_the_dense_form_off_and_on(B, N, M, kind):
    _compare(B, N, M, kind, RUN_LENGTHS)


@pytest.mark.parametrize("B,N,M", SMALL)
def test_small_grids_are_untouched_by_the_switches(B, N, M):
    for kind in ("synthetic", "huge_point"):
        _compare(B, N, M, kind, (1, 2))


def test_unscalable_tiles_keep_the_bits():
    """Clouds x 1e24 (row norms past 2^75: every point a candidate; the measured rho is inf / inf there and must not matter)."""
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

    with _Forms() as forms, _Da() as da:
        forms.set(False, True)
        dense = run()
        got = []
        for S in (1, 2):
            forms.set(True, True, S)
            da.set(True, True)
            got.append(run())
        torch.cuda.synchronize()
    for d in dense:
        assert torch.isfinite(d).all() and d.abs().max().item() > 1e22
    for g in got:
        for d, v in zip(dense, g):
            assert torch.equal(d, v), (d != v).sum().item()


def test_every_slot_of_a_short_refine_is_identical_off_and_on():
    """K = 2 at (33, 128, 128) and (64, 256, 192): every pose_* / scale_* slot under the three arms."""
    for B, N, M in ((33, 128, 128), (64, 256, 192)):
        model = _cached_model(N, M)
        batch = _batch(B, N, M, "synthetic")
        outs = []
        with _Da() as da:
            for on, stn in ARMS:
                da.set(on, stn)
                out = model.refine(batch, n_iter=2)
                outs.append({k: v.clone() for k, v in out.items() if k.startswith(("pose_", "scale_"))})
        torch.cuda.synchronize()
        assert len(outs[0]) == 6
        for o in outs[1:]:
            assert o.keys() == outs[0].keys()
            for k in o:
                assert torch.isfinite(o[k]).all() and torch.equal(outs[0][k], o[k]), (B, N, M, k)


def test_trunk_probe_reports_the_new_bound_and_it_holds_for_every_output(record_property):
    """catre_trunk_screen_probe at (33, 128, 128): the same S with the switch off and on, a smaller eps everywhere with it
    on, and max |y64 - S| / eps < 1 over all 132 x 1024 x 64 outputs, y64 the float64 product of the dense conv3 rows with
    conv4's weights.  Measured on MI355X: 0.132 with `screen_da` (0.085 with the shipped bound); eps is 0.63 of the shipped one
    on average."""
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
    with _Forms() as forms, _Da() as da:
        forms.set(True, True, 2)
        da.set(False, False)
        scr0, eps0, _, _ = _probe_trunk(rt, x, tfd, trans, t64, B, N, M)
        da.set(True, False)
        scr, eps, gfeat, pointfeat = _probe_trunk(rt, x, tfd, trans, t64, B, N, M)
    assert torch.equal(gfeat, st["gfeat"]) and torch.equal(pointfeat, st["pointfeat"])
    assert torch.equal(scr, scr0) and (eps < eps0).all()
    W4 = dict(model.named_parameters())["pcl_net.conv4.weight"].detach().reshape(1024, 512)
    y64 = (c3.double() @ W4.double().t()).view(tiles, 64, 1024).transpose(1, 2)
    r0 = ((y64 - scr.double()).abs() / eps0.double()).max().item()
    r64 = ((y64 - scr.double()).abs() / eps.double()).max().item()
    record_property("largest_abs_err_over_eps_da", r64)
    print(f"trunk: largest |y64 - S| / eps = {r64:.5f} with screen_da, {r0:.5f} without; mean eps / shipped eps "
          f"{(eps / eps0).mean().item():.4f} over {scr.numel()} outputs")
    assert torch.isfinite(scr).all() and torch.isfinite(eps).all() and (eps > 0).all()
    assert r64 < 1.0, r64


@pytest.mark.parametrize("which,name", [(0, "stn"), (1, "fstn")])
def test_stn_probe_reports_the_new_bound_and_it_holds_for_every_output(record_property, which, name):
    """catre_stn_screen_probe at (64, 256, 256), the smallest grid of its existing test (the probe needs 256 pairs): the
    same for conv3 of either STN, y64 from the image rows the probe returns.  Measured on MI355X: 0.344 (stn) and 0.309
    (fstn) with the arm on, 0.222 and 0.203 with it off."""
    from catre_amd import hip
    from catre_amd import runtime as RT

    B, N, M = 64, 256, 256
    model = _cached_model(N, M)
    batch = _batch(B, N, M, "synthetic")
    rt = model._runtime()
    lib = hip.load()
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)
    st = rt.stage_pointnet(x, tfd, True)
    pts = hip.points_desc(x, tfd)
    prm, packed = rt.params(torch.device(DEV), hip.PACK_ALL)
    ws = rt.workspace(B, N, M, torch.device(DEV))
    sp = hip.stream_ptr(torch.device(DEV))
    C, tiles = 2 * B, B * (N + M) // 64
    trans = st["trans"].contiguous()

    def probe():
        scr, eps = (torch.full((tiles, 1024, 64), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
        rows = torch.full((tiles, 64, 128), float("nan"), dtype=torch.float32, device=DEV)
        pooled = torch.empty(C, 1024, dtype=torch.float32, device=DEV)
        hip.check(lib.catre_stn_screen_probe(which, ctypes.byref(pts), hip.ptr(trans), prm, hip.ptr(packed), hip.ptr(scr),
                                             hip.ptr(eps), hip.ptr(rows), hip.ptr(pooled), hip.ptr(ws), ws.numel(), B, N, M, sp),
                  "catre_stn_screen_probe")
        torch.cuda.synchronize()
        return scr, eps, rows, pooled

    with _Forms() as forms, _Da() as da:
        forms.set(True, True, 0)
        da.set(True, False)                     # the STN arm off: the shipped eps
        scr0, eps0, _, _ = probe()
        da.set(True, True)
        scr, eps, rows, pooled = probe()
    assert torch.equal(pooled, st[f"{name}_pool"]) and torch.isfinite(rows).all() and (rows >= 0).all()
    assert torch.equal(scr, scr0) and (eps < eps0).all()
    W3 = dict(model.named_parameters())[f"pcl_net.{name}.conv3.weight"].detach().reshape(1024, 128).double()
    y = (rows.double().view(tiles * 64, 128) @ W3.t()).view(tiles, 64, 1024).transpose(1, 2)
    r0 = ((y - scr.double()).abs() / eps0.double()).max().item()
    r = ((y - scr.double()).abs() / eps.double()).max().item()
    record_property(f"largest_abs_err_over_eps_da_{name}", r)
    print(f"{name}: largest |y64 - S| / eps = {r:.5f} with screen_da_stn, {r0:.5f} without; mean eps / shipped eps "
          f"{(eps / eps0).mean().item():.4f}")
    assert torch.isfinite(scr).all() and torch.isfinite(eps).all() and (eps > 0).all()
    assert r < 1.0, r
