"""The screened conv3 max-pool of the two STN pair kernels (kernel-form switch `screen_stn`, k_stn3d_pair_s / k_stnkd_pair_s
in csrc/catre_screen.h) against the dense pair kernels it must reproduce bit for bit, and the device's error bound against
the exact product.

Shapes: the smallest that take the pair form (256 pairs).  (64, 256, 256): full pairs only.  (64, 200, 150): a ragged second
tile of 8 valid points (N = 200: pairs of 128 + 72) and a cloud of three tiles whose last pair is a single tile of 22 points
(M = 150).  (128, 65, 64): a second tile with one valid point (N = 65) and one-tile pairs throughout (M = 64)."""
import ctypes

import pytest
import torch

from tests.test_hip_screen import _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(64, 256, 256), (64, 200, 150), (128, 65, 64)]
KINDS = ["synthetic", "identical", "alternating"]


def _stn_forms(fn):
    """fn() with `screen` on and `screen_stn` off, then on."""
    from catre_amd import hip

    prev, prev_stn = hip.form_switch("screen"), hip.form_switch("screen_stn")
    try:
        hip.form_switch("screen", True)
        hip.form_switch("screen_stn", False)
        off = fn()
        assert hip.form_switch("screen_stn", True) is False
        on = fn()
        assert hip.form_switch("screen_stn") is True
    finally:
        hip.form_switch("screen", prev)
        hip.form_switch("screen_stn", prev_stn)
    torch.cuda.synchronize()
    return off, on


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_screened_stn_returns_the_bits_of_the_dense_pair_kernels(B, N, M, kind):
    """`stn_pool` and `fstn_pool` of `stage_pointnet` and every slot of a K = 2 refine: `torch.equal` with `screen_stn` off and
    on (`screen` on).  Identical points make every point of a tile a candidate (all eight replay rounds), two alternating
    points 32 exact ties per channel."""
    from catre_amd import runtime as RT

    model = _model(N, M)
    batch = _batch(B, N, M, kind)
    rt = model._runtime()
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)

    def run():
        st = rt.stage_pointnet(x, tfd, True)
        out = model.refine(batch, n_iter=2)
        return st, out

    (st0, out0), (st1, out1) = _stn_forms(run)
    for key in ("stn_pool", "fstn_pool", "gfeat", "pointfeat"):
        assert torch.equal(st0[key], st1[key]), (B, N, M, kind, key, (st0[key] != st1[key]).sum().item())
    for i in range(3):
        for key in (f"pose_{i}", f"scale_{i}"):
            assert torch.equal(out0[key], out1[key]), (B, N, M, kind, key)


@pytest.mark.parametrize("which,name", [(0, "stn"), (1, "fstn")])
def test_device_bound_holds_for_every_output_of_conv3(record_property, which, name):
    """`catre_stn_screen_probe`: |y - screen| <= eps for all 512 x 1024 x 64 outputs of conv3, y = the exact (float64) product
    of the image rows the probe returns (the fp32 conv2 image the screen read) with conv3's weights; eps finite and positive;
    the probe's pooled output equals the normal path's.  The bound is worst-case: the CPU emulation (tests/test_screen_bound.py)
    sits far below 1 and the trunk measured 0.0049 of eps at K = 512; measured on MI355X here: 0.043 (stn), 0.040 (fstn).  The ratio goes into the report (`record_property`)
    whether the test passes or not."""
    from catre_amd import hip
    from catre_amd import runtime as RT

    B, N, M = 64, 256, 256
    model = _model(N, M)
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
    scr, eps = (torch.empty(tiles, 1024, 64, dtype=torch.float32, device=DEV) for _ in range(2))
    rows = torch.full((tiles, 64, 128), float("nan"), dtype=torch.float32, device=DEV)
    pooled = torch.empty(C, 1024, dtype=torch.float32, device=DEV)
    hip.check(lib.catre_stn_screen_probe(which, ctypes.byref(pts), hip.ptr(trans), prm, hip.ptr(packed), hip.ptr(scr),
                                         hip.ptr(eps), hip.ptr(rows), hip.ptr(pooled), hip.ptr(ws), ws.numel(), B, N, M, sp),
              "catre_stn_screen_probe")
    torch.cuda.synchronize()
    assert torch.equal(pooled, st[f"{name}_pool"])
    assert torch.isfinite(rows).all()
    W3 = dict(model.named_parameters())[f"pcl_net.{name}.conv3.weight"].detach().reshape(1024, 128).double()
    y = (rows.double().view(tiles * 64, 128) @ W3.t()).view(tiles, 64, 1024).transpose(1, 2)
    ratio = ((y - scr.double()).abs() / eps.double()).max().item()
    record_property("largest_abs_err_over_eps", ratio)
    print(f"{name}.conv3: largest |y - screen| / eps over {scr.numel()} outputs: {ratio:.5f}")
    assert torch.isfinite(eps).all() and (eps > 0).all()
    assert ratio <= 1.0, f"|y - screen| exceeds the device bound: largest |y - screen| / eps = {ratio:.4f}"


def test_probe_is_unsupported_off_the_pair_form():
    """Fewer than 256 pairs: no full-grid pair form, the probe says so."""
    from catre_amd import hip
    from catre_amd import runtime as RT

    B, N, M = 4, 128, 128
    model = _model(N, M)
    batch = _batch(B, N, M, "synthetic")
    rt = model._runtime()
    lib = hip.load()
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)
    pts = hip.points_desc(x, tfd)
    prm, packed = rt.params(torch.device(DEV), hip.PACK_ALL)
    ws = rt.workspace(B, N, M, torch.device(DEV))
    tiles = B * (N + M) // 64
    scr, eps = (torch.empty(tiles, 1024, 64, dtype=torch.float32, device=DEV) for _ in range(2))
    rows = torch.empty(tiles, 64, 128, dtype=torch.float32, device=DEV)
    pooled = torch.empty(2 * B, 1024, dtype=torch.float32, device=DEV)
    r = lib.catre_stn_screen_probe(0, ctypes.byref(pts), None, prm, hip.ptr(packed), hip.ptr(scr), hip.ptr(eps),
                                   hip.ptr(rows), hip.ptr(pooled), hip.ptr(ws), ws.numel(), B, N, M,
                                   hip.stream_ptr(torch.device(DEV)))
    assert r == -4, r   # CATRE_ERR_UNSUPPORTED
