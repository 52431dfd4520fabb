"""The lean epilogue of the fp16-screen kernels (kernel-form switch `screen_epi`: k_trunk4sr16e / k_trunk4sp16e,
k_stn3d_pair_sr16e / _sp16e, k_stnkd_pair_sr16e / _sp16e in csrc/catre_screen.h).  The candidate predicate is unchanged -
only how the mask, the list and the scan are computed - so the switch off, the switch on and the dense kernels (`screen`
off) must return the same bits.

Shapes, clouds and run lengths are those of tests/test_hip_screen_f16.py: the smallest grids that take the full-grid forms,
ragged last tiles, a pair of one tile; lists below, at and above their capacity (more than one batch), all-zero clouds
(every point a tie) and one huge point per tile; run lengths 1 (the one-tile `_sp16e` kernels), 2, 3 and 16 (`_sr16e`)."""
import pytest
import torch

from tests.test_hip_screen import _batch
from tests.test_hip_screen_f16 import KEYS, RUN_LENGTHS, SHAPES, _cached_model, _clouds, _Forms, _probe_trunk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KINDS = ["synthetic", "one_then_distinct", "first_then_one", "zero", "huge_point"]


class _Epi:
    """Set `screen_epi`, restore it on exit."""

    def __enter__(self):
        from catre_amd import hip

        self.prev = hip.form_switch("screen_epi")
        return self

    def set(self, on):
        from catre_amd import hip

        hip.form_switch("screen_epi", on)

    def __exit__(self, *exc):
        from catre_amd import hip

        hip.form_switch("screen_epi", self.prev)


def test_the_switch_reads_back_and_is_no_bit_of_the_form_word():
    from catre_amd import hip

    assert hip.FORM_IDS["screen_epi"] == 13 and "screen_epi" not in hip.SWITCH_BITS
    with _Epi() as epi:
        epi.set(True)
        assert hip.form_switch("screen_epi", False) is True
        assert hip.form_switch("screen_epi") is False
        # the decision does not read it: the same form, run length and grid either way
        a = hip.form_decision("trunk", "fp32", 256, 1024, 1024, sum(1 << b for b in range(13) if b not in (3, 4)))
        epi.set(True)
        assert hip.form_decision("trunk", "fp32", 256, 1024, 1024, sum(1 << b for b in range(13) if b not in (3, 4))) == a
        assert a[0] == "run_f16"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_lean_epilogue_returns_the_bits_of_the_parent_epilogue_and_of_the_dense_form(B, N, M, kind):
    model = _cached_model(N, M)
    rt = model._runtime()
    x, tfd = _clouds(B, N, M, kind)

    def run():
        st = rt.stage_pointnet(x, tfd, True)
        return {k: st[k].clone() for k in KEYS}

    with _Forms() as forms, _Epi() as epi:
        forms.set(False, False)
        dense = run()
        arms = []
        for S in RUN_LENGTHS:
            forms.set(True, True, S)
            for on in (False, True):
                epi.set(on)
                arms.append((f"epi {'on' if on else 'off'} S={S}", run()))
        torch.cuda.synchronize()
    for key in KEYS:
        assert torch.isfinite(dense[key]).all(), (B, N, M, kind, key)
        for arm, st in arms:
            assert torch.equal(dense[key], st[key]), (B, N, M, kind, arm, key, (dense[key] != st[key]).sum().item())


def test_short_refine_is_identical_in_every_slot_under_both_arms():
    """K = 2 at (33, 128, 128): every pose_* / scale_* slot, `screen_epi` off and on."""
    B, N, M = 33, 128, 128
    model = _cached_model(N, M)
    batch = _batch(B, N, M, "synthetic")
    outs = []
    with _Epi() as epi:
        for on in (False, True):
            epi.set(on)
            out = model.refine(batch, n_iter=2)
            outs.append({k: v.clone() for k, v in out.items() if k.startswith(("pose_", "scale_"))})
    torch.cuda.synchronize()
    assert outs[0].keys() == outs[1].keys() and len(outs[0]) == 6
    for k in outs[0]:
        assert torch.isfinite(outs[0][k]).all() and torch.equal(outs[0][k], outs[1][k]), k


def test_probe_with_the_switch_on_still_returns_the_screen_value_and_its_bound():
    """The lean kernels carry no probe code: with the switch on a probe call takes the kernels that do.  It must return S and
    eps of the fp16 screen with |y64 - S| <= eps against the exact (float64) product of the dense conv3 rows with conv4's
    weights, the same S and eps as with the switch off, and the features of the unprobed stage."""
    import ctypes

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
    with _Forms() as forms, _Epi() as epi:
        forms.set(True, True, 2)
        epi.set(False)
        scr0, eps0, _, _ = _probe_trunk(rt, x, tfd, trans, t64, B, N, M)
        epi.set(True)
        scr, eps, gfeat, pointfeat = _probe_trunk(rt, x, tfd, trans, t64, B, N, M)
    assert torch.equal(gfeat, st["gfeat"]) and torch.equal(pointfeat, st["pointfeat"])
    assert torch.equal(scr, scr0) and torch.equal(eps, eps0)
    W4 = dict(model.named_parameters())["pcl_net.conv4.weight"].detach().reshape(1024, 512)
    y64 = (c3.double() @ W4.double().t()).view(tiles, 64, 1024).transpose(1, 2)
    r64 = ((y64 - scr.double()).abs() / eps.double()).max().item()
    print(f"probe with screen_epi on: largest |y64 - S| / eps = {r64:.5f} over {scr.numel()} outputs")
    assert torch.isfinite(scr).all() and torch.isfinite(eps).all() and (eps > 0).all()
    assert r64 <= 1.0, r64
