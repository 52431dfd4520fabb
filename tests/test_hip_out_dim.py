"""The PointNet encoder at ``PCLNET.INIT_CFG.out_dim`` 64, 128, 256 and 512 on the device.

1. ``catre_trunk_w`` against the shipped ``catre_trunk``, bit for bit: the new kernel accumulates every conv4 output from the
   same operands in the same K order, so at conv4 rows ``[:D']`` of a 1024-wide model it must return the shipped kernel's
   ``gfeat[:, :D']``, its 64 ``max_n pointfeat`` columns and ``pointfeat`` exactly.  Shapes: a single point (1,1,1); tiles
   one short of / one past 64 (5,63,65); ragged tiles of 36 and 6 points, several tiles per cloud (3,100,70); a third tile of
   one point next to a one-point cloud (2,129,1); and (33,128,128), 132 tiles, where the shipped side is its full-grid
   (screened one-wave) form instead of the small-grid ones.  ``catre_trunk_w`` itself has one grid form.
2. Whole models of ``tests/golden/out_dim.npz`` (records of the unmodified reference, ``tools/make_outdim_golden.py``)
   and 12 edge shapes at D = 128 against the fp32 oracle: 2e-5, the project's stage bar.
3. One training iteration per fixture case: losses 1e-4 relative, every gradient tensor within ``max(2e-4 of the tensor's
   maximum, 2 x the fp32 reference's own deviation from its fp64 run)`` (tests/test_head_forms.py's rule); W256 under
   autocast by tests/test_hip_amp_pin.py's criterion.
4. W256 in the reduced-precision modes; 5. invariants.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from catre_amd import hip, synth
from tests.test_out_dim_host import _json, case_cfg, cases, fixture, width_cfg
from tests.util import recipe_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIGHT, GRAD_REL = 2e-5, 2e-4
WIDTHS = (64, 128, 256, 512, 1024)


def _to_dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def sample_index(numel, n=512):
    if numel <= n:
        return np.arange(numel, dtype=np.int64)
    return np.unique(np.linspace(0, numel - 1, n).astype(np.int64))


def _split(flat, counts):
    return np.split(np.asarray(flat), np.cumsum(counts)[:-1])


# ------------------------------------------------------------------------------------------------- 1. the kernel, exactly
def _shipped_model(N, M):
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from catre_amd.config import default_cfg

    cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=2, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=True)
    model.load_state_dict({k: v.to(DEV) for k, v in recipe_sd(cfg, 3).items()}, strict=True)
    return model.eval()


def _trunk_w(rt, pts, trans, t64, D, B, N, M, pad=0, ws=None):
    """catre_pack_encoder_w + catre_trunk_w at conv4 rows [:D] of the runtime's (1024-wide) parameters; `pad` floats of
    sentinel behind gfeat / pointfeat."""
    lib, dev = hip.load(), torch.device(DEV)
    tensors = list(rt._param_keep)
    iw, ib = hip.PARAM_KEYS.index("pcl_net.conv4.weight"), hip.PARAM_KEYS.index("pcl_net.conv4.bias")
    tensors[iw], tensors[ib] = tensors[iw][:D].contiguous(), tensors[ib][:D].contiguous()
    prm = hip.param_array(tensors)
    packed = torch.empty(lib.catre_packed_floats_w(D), dtype=torch.float32, device=DEV)
    sp = hip.stream_ptr(dev)
    hip.check(lib.catre_pack_encoder_w(prm, D, hip.ptr(packed), packed.numel(), sp), "catre_pack_encoder_w")
    C = 2 * B
    gfeat = torch.full((C * (D + 64) + pad,), -7.0, dtype=torch.float32, device=DEV)
    pointfeat = torch.full((B * (N + M) * 64 + pad,), -7.0, dtype=torch.float32, device=DEV)
    ws = rt.workspace(B, N, M, dev) if ws is None else ws
    hip.check(lib.catre_trunk_w(ctypes.byref(pts), hip.ptr(trans), hip.ptr(t64), prm, hip.ptr(packed), D, hip.ptr(gfeat),
                                hip.ptr(pointfeat), hip.ptr(ws), lib.catre_workspace_bytes(B, N, M), B, N, M, sp),
              "catre_trunk_w")
    torch.cuda.synchronize()
    del tensors
    return gfeat, pointfeat


@pytest.mark.parametrize("B,N,M", [(1, 1, 1), (5, 63, 65), (3, 100, 70), (2, 129, 1), (33, 128, 128)])
def test_trunk_w_returns_the_bits_of_the_shipped_trunk(B, N, M):
    from catre_amd import runtime as RT

    lib, dev = hip.load(), torch.device(DEV)
    model = _shipped_model(N, M)
    rt = model._runtime()
    batch = _to_dev(synth.make_inputs(B, N, M, seed=70 + B))
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)
    st = rt.stage_pointnet(x, tfd, True)   # the STNs' outputs: any fixed transforms do, both kernels read the same
    trans, t64 = st["trans"].contiguous(), st["trans_feat"].contiguous()
    prm, packed = rt.params(dev, hip.PACK_ALL)
    ws = rt.workspace(B, N, M, dev)
    sp = hip.stream_ptr(dev)
    pose, scale = batch["obj_pose_est"].contiguous(), batch["obj_scale_est"].contiguous()
    for apply_pose in (False, True):
        if apply_pose:   # the raw clouds, posed on load
            pts = hip.points_desc(batch["pcl"].permute(0, 2, 1), batch["obj_kps"].permute(0, 2, 1))
            pts.pose, pts.scale, pts.apply_pose, pts.zero_center = pose.data_ptr(), scale.data_ptr(), 1, 1
        else:
            pts = hip.points_desc(x, tfd)
        for ft in (t64, None):
            gfeat = torch.empty(2 * B, 1088, dtype=torch.float32, device=DEV)
            pointfeat = torch.empty(B * (N + M), 64, dtype=torch.float32, device=DEV)
            hip.check(lib.catre_trunk(ctypes.byref(pts), hip.ptr(trans), hip.ptr(ft), prm, hip.ptr(packed), hip.ptr(gfeat),
                                      hip.ptr(pointfeat), hip.ptr(ws), ws.numel(), B, N, M, sp), "catre_trunk")
            torch.cuda.synchronize()
            if not apply_pose and ft is not None:
                assert torch.equal(gfeat, st["gfeat"]) and torch.equal(pointfeat, st["pointfeat"])
            for D in WIDTHS:
                g, pf = _trunk_w(rt, pts, trans, ft, D, B, N, M)
                g = g.view(2 * B, D + 64)
                what = (B, N, M, apply_pose, ft is not None, D)
                assert torch.equal(g[:, :D], gfeat[:, :D]), what + ("conv4 max", int((g[:, :D] != gfeat[:, :D]).sum()))
                assert torch.equal(g[:, D:], gfeat[:, 1024:]), what + ("pointfeat max",)
                assert torch.equal(pf.view(-1, 64), pointfeat), what + ("pointfeat",)


@pytest.mark.parametrize("D", [64, 256])
def test_trunk_w_writes_nothing_behind_its_outputs(D):
    from catre_amd import runtime as RT

    B, N, M, PAD = 3, 100, 70, 4096
    lib = hip.load()
    model = _shipped_model(N, M)
    rt = model._runtime()
    batch = _to_dev(synth.make_inputs(B, N, M, seed=73))
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"], True)
    st = rt.stage_pointnet(x, tfd, True)
    need = lib.catre_workspace_bytes(B, N, M)
    ws = torch.full((need + 4 * PAD,), 0x5A, dtype=torch.uint8, device=DEV)
    g, pf = _trunk_w(rt, hip.points_desc(x, tfd), st["trans"].contiguous(), st["trans_feat"].contiguous(), D, B, N, M, pad=PAD,
                     ws=ws)
    assert bool((g[-PAD:] == -7.0).all()) and bool((pf[-PAD:] == -7.0).all()) and bool((ws[need:] == 0x5A).all())
    assert not bool((g[:-PAD] == -7.0).any()) and not bool((pf[:-PAD] == -7.0).any())   # and every output was written
    assert torch.equal(g[:-PAD].view(2 * B, D + 64)[:, :D], st["gfeat"][:, :D])


def test_trunk_w_status_codes_on_the_device():
    lib = hip.load()
    t = torch.zeros(64, device=DEV)
    prm = hip.param_array([t] * hip.CATRE_P_COUNT)
    assert lib.catre_pack_encoder_w(prm, 256, hip.ptr(t), t.numel(), hip.stream_ptr(torch.device(DEV))) == -2   # short image
    assert lib.catre_pack_encoder_w(prm, 96, hip.ptr(t), 1 << 30, hip.stream_ptr(torch.device(DEV))) == -4


# ------------------------------------------------------------------------------------------------- 2. whole models
def _model(name, freeze=False):
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    D, B, N, M, seed, salt, amp, over = cases()[name]
    cfg = case_cfg(name, DEV)
    if freeze:
        cfg.MODEL.CATRE.PCLNET.FREEZE = True
    model, _ = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in recipe_sd(cfg, salt).items()}, strict=True)
    return cfg, model, _to_dev(synth.make_inputs(B, N, M, seed=seed))


@pytest.mark.parametrize("name", sorted(cases()))
def test_refine_matches_the_reference_record(name):
    from catre_amd import runtime as RT

    z = fixture()
    K = int(z["meta_k_iter"][0])
    D = cases()[name][0]
    cfg, model, batch = _model(name)
    model.eval()
    out = model.refine(batch, n_iter=K)
    for i in range(1, K + 1):
        for what, ref in (("pose", z[f"{name}__poses"][i]), ("scale", z[f"{name}__scales"][i])):
            err = float(np.abs(out[f"{what}_{i}"].cpu().numpy() - ref).max())
            print(f"{name} {what}_{i}: {err:.2e}")
            assert err <= TIGHT, (name, what, i, err)
    # the encoder's pooled feature of iteration 1
    x, tfd = RT.pose_apply(batch["pcl"], batch["obj_kps"], batch["obj_pose_est"], batch["obj_scale_est"],
                           bool(cfg.INPUT.ZERO_CENTER_INPUT))
    st = model._runtime().stage_pointnet(x, tfd, bool(cfg.MODEL.CATRE.PCLNET.INIT_CFG.feature_transform))
    assert tuple(st["gfeat"].shape) == (2 * batch["pcl"].shape[0], D + 64)
    err = float(np.abs(st["gfeat"][:, :D].cpu().numpy() - z[f"{name}__g1"]).max())
    print(f"{name} g: {err:.2e} (max |g| {np.abs(z[f'{name}__g1']).max():.2e})")
    assert err <= TIGHT, (name, err)


@pytest.mark.parametrize("B,N,M", [(1, 1, 1), (5, 63, 65), (3, 64, 64), (2, 129, 1), (7, 130, 257), (4, 2, 300),
                                   (1, 4096, 32), (2, 32, 33), (1, 31, 97), (4, 96, 160), (8, 33, 31), (9, 33, 95)])
def test_ragged_shapes_match_oracle_at_128(B, N, M):
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from oracle import catre_oracle as O

    K = 2
    cfg = width_cfg(128, DEV, N, M)
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = recipe_sd(cfg, 3)
    model.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=True)
    batch = synth.make_inputs(B, N, M, seed=40 + B)
    out = model.eval().refine(_to_dev(batch), n_iter=K)
    with torch.no_grad():
        want = O.refine_k(batch, sd, width_cfg(128, "cpu", N, M), n_iter=K)
    for i in range(1, K + 1):
        assert (out[f"pose_{i}"].cpu() - want[f"pose_{i}"]).abs().max() <= TIGHT, (B, N, M, i)
        assert (out[f"scale_{i}"].cpu() - want[f"scale_{i}"]).abs().max() <= TIGHT, (B, N, M, i)


# ------------------------------------------------------------------------------------------------- 3. training
def _train_iteration(cfg, model, batch, autocast=False):
    from catre_amd.batching import batch_updater_test

    model.train()
    model.zero_grad(set_to_none=True)
    b = dict(batch)
    batch_updater_test(cfg, b)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out, ld = model(b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
                        obj_class=b["obj_cls"], gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"],
                        obj_kps=b["obj_kps"], mean_scales=b["obj_mean_scales"], sym_info=[None] * b["pcl"].shape[0],
                        do_loss=True, cur_iter=1)
    sum(ld.values()).backward()
    return (out, {k: float(v) for k, v in ld.items()},
            {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None})


def _check_gradients(name, grads, tensors):
    """Every tensor of `tensors` within max(2e-4 of its maximum, 2 x the fp32 reference's own deviation from fp64)."""
    z = fixture()
    meta = _json(z, f"{name}__meta")
    bad = []
    for t, r64, dev32 in zip(meta["tensors"], _split(z[f"{name}__g64"], meta["counts"]), z[f"{name}__dev32"]):
        if t not in tensors:
            continue
        got = grads[t].reshape(-1)[torch.from_numpy(sample_index(grads[t].numel()))].double().numpy()
        err, bar = float(np.abs(got - r64).max()), max(GRAD_REL * float(np.abs(r64).max()), 2.0 * float(dev32))
        if not err <= bar:
            bad.append((t, err, bar))
    print(f"{name}: {len(tensors)} gradient tensors, outside their bar: {bad}")
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(cases()))
def test_training_iteration_matches_the_fp64_record(name):
    z = fixture()
    meta = _json(z, f"{name}__meta")
    cfg, model, batch = _model(name)
    out, losses, grads = _train_iteration(cfg, model, batch)
    assert list(losses) == meta["loss_keys"]
    for k, want in zip(meta["loss_keys"], z[f"{name}__loss64"]):
        print(f"{name} {k}: {losses[k]:.8f} vs {want:.8f}")
        assert abs(losses[k] - want) <= 1e-4 * abs(want), (k, losses[k], want)
    assert sorted(grads) == sorted(meta["tensors"])
    none = [k for k, _ in meta["keys"] if k not in grads]
    assert sorted(none) == sorted(meta["gradnone"]) and len(none) == 6 and all(".norm." in k for k in none)
    _check_gradients(name, grads, meta["tensors"])
    for what in ("pose_1", "scale_1"):
        assert float(np.abs(out[what].detach().cpu().numpy() - z[f"{name}__train_{what}"]).max()) <= TIGHT, what


def test_w256_autocast_training_is_no_further_from_fp32_than_the_references_own():
    """The criterion of tests/test_hip_amp_pin.py: per tensor, the distance to the reference's fp32 gradient is at most
    1.2 x the reference's own autocast distance + 5e-3 (relative to the fp32 gradient's norm, on the sampled entries).

    At out_dim != 1024 the encoder is fp32 in every compute mode (its no-grad trunk is an fp32 kernel, and the training
    forward takes the same precision); the heads run on bf16 operands.  Measured on MI355X: the rotation heads' tensors at
    about half the reference's own distance; the closest to its bar is the one-element ``rot_head.rot_head_x.conv_p.bias``,
    0.0143 against 1.2 x 0.00851 + 0.005 = 0.0152 (the reference's autocast value of that element, 0.140625, is a bf16 number
    that lies 0.85 % from the fp32 one while its other gradients of the head are 1.9-2.9 % off).  With the encoder's pooled
    layers on bf16 operands as well, as the layer-wise ops do under autocast, that element was at 0.01537 and missed."""
    z = fixture()
    meta = _json(z, "W256__meta")
    cfg, model, batch = _model("W256")
    _, losses, grads = _train_iteration(cfg, model, batch, autocast=True)
    assert all(np.isfinite(v) for v in losses.values()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    for k, l32 in zip(meta["loss_keys"], z["W256__loss32"]):
        assert abs(losses[k] - l32) <= 3e-2 * abs(l32) + 1e-3, (k, losses[k], l32)
    worse = []
    for t, r32, ramp in zip(meta["tensors"], _split(z["W256__g32"], meta["counts"]), _split(z["W256__gamp"], meta["counts"])):
        got = grads[t].reshape(-1)[torch.from_numpy(sample_index(grads[t].numel()))].double().numpy()
        n = float(np.linalg.norm(r32)) + 1e-30
        d_hip, d_ref = float(np.linalg.norm(got - r32)) / n, float(np.linalg.norm(ramp - r32)) / n
        if d_hip > 1.2 * d_ref + 5e-3:
            worse.append((t, d_hip, d_ref))
    assert not worse, worse


@pytest.mark.parametrize("autocast", [False, True])
def test_frozen_encoder_trains_the_heads_on_the_no_grad_route(autocast):
    """PCLNET.FREEZE: the encoder runs once, on the inference kernels (catre_trunk_w), in fp32 also under autocast; the heads
    follow the mode - fp32: the fp64 record's bar, autocast: the criterion of the autocast test above on the heads' tensors."""
    z = fixture()
    meta = _json(z, "W256__meta")
    cfg, model, batch = _model("W256", freeze=True)
    rt = model._runtime()
    calls = []
    stage = rt.stage_pointnet
    rt.stage_pointnet = lambda *a, **k: calls.append(1) or stage(*a, **k)
    try:
        _, losses, grads = _train_iteration(cfg, model, batch, autocast=autocast)
    finally:
        del rt.stage_pointnet
    assert calls == [1]
    heads = [t for t in meta["tensors"] if not t.startswith("pcl_net.")]
    assert sorted(grads) == sorted(heads)
    if not autocast:
        for k, want in zip(meta["loss_keys"], z["W256__loss64"]):
            assert abs(losses[k] - want) <= 1e-4 * abs(want), (k, losses[k], want)
        _check_gradients("W256", grads, heads)
        return
    for k, l32 in zip(meta["loss_keys"], z["W256__loss32"]):
        assert abs(losses[k] - l32) <= 3e-2 * abs(l32) + 1e-3, (k, losses[k], l32)
    worse = []
    for t, r32, ramp in zip(meta["tensors"], _split(z["W256__g32"], meta["counts"]), _split(z["W256__gamp"], meta["counts"])):
        if t not in grads:
            continue
        got = grads[t].reshape(-1)[torch.from_numpy(sample_index(grads[t].numel()))].double().numpy()
        n = float(np.linalg.norm(r32)) + 1e-30
        d_hip, d_ref = float(np.linalg.norm(got - r32)) / n, float(np.linalg.norm(ramp - r32)) / n
        if d_hip > 1.2 * d_ref + 5e-3:
            worse.append((t, d_hip, d_ref))
    assert not worse, worse


# ------------------------------------------------------------------------------------------------- 4. modes
def test_w256_refine_in_the_reduced_precision_modes():
    z = fixture()
    K = int(z["meta_k_iter"][0])
    cfg, model, batch = _model("W256")
    model.eval()

    def err(out):
        return max(float(np.abs(out[f"{w}_{i}"].cpu().numpy() - z[f"W256__{w}s"][i]).max()) for i in range(1, K + 1)
                   for w in ("pose", "scale"))

    with torch.autocast("cuda", dtype=torch.bfloat16):
        e_amp = err(model.refine(batch, n_iter=K))
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = "bf16"
    e_bf16 = err(model.refine(batch, n_iter=K))
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = "split"
    e_split = err(model.refine(batch, n_iter=K))
    print(f"W256 refine vs the fp32 record: autocast {e_amp:.2e}, bf16 {e_bf16:.2e}, split {e_split:.2e}")
    assert e_amp <= 1e-2 and e_bf16 <= 1e-2, (e_amp, e_bf16)
    assert e_split <= TIGHT, e_split
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = "fp16"
    with pytest.raises(NotImplementedError, match="out_dim"):
        model.refine(batch, n_iter=1)


# ------------------------------------------------------------------------------------------------- 5. invariants
def test_an_object_does_not_depend_on_the_batch_around_it():
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    N, M = 100, 70
    cfg = width_cfg(256, DEV, N, M)
    model, _ = build_model_optimizer(cfg, is_test=True)
    model.load_state_dict({k: v.to(DEV) for k, v in recipe_sd(cfg, 2).items()}, strict=True)
    model.eval()
    batch = _to_dev(synth.make_inputs(3, N, M, seed=51))
    out3 = model.refine(batch, n_iter=2)
    out1 = model.refine({k: (v[:1].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}, n_iter=2)
    for k in ("pose_1", "scale_1", "pose_2", "scale_2"):
        assert torch.equal(out3[k][0], out1[k][0]), k


def test_state_dict_round_trip_with_the_reference_shaped_checkpoint():
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    cfg, model, batch = _model("W128")
    want = [(k, tuple(s)) for k, s in _json(fixture(), "W128__meta")["keys"]]
    sd = model.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    other, _ = build_model_optimizer(case_cfg("W128", DEV), is_test=True)
    other.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    a, b = model.eval().refine(batch, n_iter=2), other.eval().refine(batch, n_iter=2)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_pointnetfeat_on_its_own_at_the_width():
    """PointNetfeat.forward: global_feat [B,D] and the as-written [B,D+64,n] tensor, no-grad (catre_trunk_w) against the
    layer-wise training ops (same arithmetic, fp32 re-association only: the stage bar)."""
    from catre_amd.pointnet import PointNetfeat

    D, B, n = 256, 3, 100
    shapes = {f"pcl_net.{k}": tuple(v.shape) for k, v in PointNetfeat(n, out_dim=D, feature_transform=True).state_dict().items()}
    sd = {k[len("pcl_net."):]: v.to(DEV) for k, v in synth.recipe_state_dict(shapes, 4).items()}
    x = _to_dev(synth.make_inputs(B, n, 8, seed=9))["pcl"].permute(0, 2, 1)
    outs = []
    for gf in (True, False):
        net = PointNetfeat(n, global_feat=gf, out_dim=D, feature_transform=True).to(DEV)
        net.load_state_dict(sd, strict=True)
        with torch.no_grad():
            a = net(x)
        b = net(x)   # parameters require a gradient: the layer-wise ops
        assert tuple(a.shape) == ((B, D) if gf else (B, D + 64, n)) and a.shape == b.shape
        assert float((a - b.detach()).abs().max()) <= TIGHT
        with torch.autocast("cuda", dtype=torch.bfloat16):   # at this width the encoder is fp32 in every mode
            c = net(x)
            with torch.no_grad():
                e = net(x)
        assert torch.equal(c, b) and torch.equal(e, a)
        outs.append(a)
    assert torch.equal(outs[1][:, :D, 0], outs[0])
