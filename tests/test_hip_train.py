"""Training path: outputs and EVERY parameter gradient of one refine iteration (HIP forward + HIP backward
through torch.autograd) against torch autograd of the oracle in fp64."""
import numpy as np
import pytest
import torch

from tests.util import load_golden, recipe_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _oracle_grads(g, sd, Gp, Gs, dtype=torch.float64):
    from oracle import catre_oracle as O

    sdr = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g["batch"].items()}
    x, tfd = O.pose_apply(b["pcl"], b["obj_kps"], b["obj_pose_est"], b["obj_scale_est"], g["cfg"].INPUT.ZERO_CENTER_INPUT)
    pose, scale = O.model_forward(x, tfd, b["obj_pose_est"], b["obj_scale_est"], sdr, g["cfg"], K_zoom=b["K"],
                                  mean_scales=b["obj_mean_scales"])
    loss = (pose * Gp.to(dtype)).sum() + (scale * Gs.to(dtype)).sum()
    loss.backward()
    return pose.detach(), scale.detach(), {k: v.grad for k, v in sdr.items()}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["refine_b2_small", "refine_b3_ragged", "refine_b2_kpsfeat_trans", "refine_b2_noft",
                                  "refine_b2_deepim_noK", "refine_b2_allo", "refine_b2_n1024", "refine_b2_quat"])
def test_forward_train_and_all_param_grads(name, fused):
    """fused=True: the encoder forward on the fused kernels with extra stores (catre_train_*_fwd; N, M multiples of 64,
    feature transform on), the backward layer-wise as always; fused=False: every layer its own row GEMM."""
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from catre_amd.train_forward import forward_train

    g = load_golden(name)
    eligible = g["N"] % 64 == 0 and g["M"] % 64 == 0 and name != "refine_b2_noft"
    if fused and not eligible:
        pytest.skip("shape takes the layer-wise forward")
    if not fused and name == "refine_b2_n1024":
        pytest.skip("covered by the fused variant (the fp64 oracle backward at 2 x 2048 points takes a while)")
    cfg = g["cfg"].__deepcopy__({})
    cfg.MODEL.DEVICE = DEV
    model, _ = build_model_optimizer(cfg, is_test=False)
    sd = recipe_sd(cfg, g["salt"])
    model.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=True)
    model.train()
    batch = {k: v.to(DEV) for k, v in g["batch"].items()}
    batch_updater_test(cfg, batch)
    gen = torch.Generator().manual_seed(3)
    Gp, Gs = torch.randn(g["B"], 3, 4, generator=gen), torch.randn(g["B"], 3, generator=gen)
    p = dict(model.named_parameters())
    pose, scale, aux = forward_train(p, model._opts, batch["x"], batch["tfd_kps"], batch["obj_pose_est"],
                                     batch["obj_scale_est"], batch["K"], batch["obj_mean_scales"],
                                     rt=model._runtime() if fused else None)
    # forward agrees with the reference goldens (same bar as the fused path)
    assert np.abs(pose.detach().cpu().numpy() - g["ref"]["pose_1"]).max() <= 2e-5
    assert np.abs(scale.detach().cpu().numpy() - g["ref"]["scale_1"]).max() <= 2e-5
    ((pose * Gp.to(DEV)).sum() + (scale * Gs.to(DEV)).sum()).backward()
    rp, rs, rg = _oracle_grads(g, sd, Gp, Gs)
    unused = 0
    for k, prm in p.items():
        want = rg[k]
        if want is None:  # the never-used `norm` GroupNorms (find_unused_parameters is load-bearing)
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, k
            unused += 1
            continue
        assert prm.grad is not None, f"no gradient for {k}"
        got = prm.grad.cpu().double()
        scale_ref = float(want.abs().max()) + 1e-12
        err = float((got - want).abs().max()) / scale_ref
        assert err <= 2e-4, f"{name}: grad of {k}: rel-to-max error {err:.2e} (max |grad| {scale_ref:.3e})"
    assert unused == 6


def test_module_training_step_matches_reference_golden():
    """model(..., do_loss=True) -> (out_dict, loss_dict); sum(loss).backward(): the six loss terms and the parameter
    gradients against the reference's own training iteration (tests/golden/train_b4.npz)."""
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from tests.util import load_train_golden

    g = load_train_golden("train_b4")
    cfg = g["cfg"].__deepcopy__({})
    cfg.MODEL.DEVICE = DEV
    model, opt = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in recipe_sd(cfg, g["salt"]).items()}, strict=True)
    model.train()
    b = {k: v.to(DEV) for k, v in g["batch"].items()}
    batch_updater_test(cfg, b)
    out_dict, loss_dict = model(
        b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
        obj_class=b["obj_cls"], gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"],
        obj_kps=b["obj_kps"], mean_scales=b["obj_mean_scales"], sym_info=g["sym_info"], do_loss=True, cur_iter=1)
    ref = g["ref"]
    assert np.abs(out_dict["pose_1"].detach().cpu().numpy() - ref["pose_1"]).max() <= 2e-5
    assert set(loss_dict) == {k[6:] for k in ref if k.startswith("loss__")}
    for k, v in loss_dict.items():
        np.testing.assert_allclose(v.item(), ref[f"loss__{k}"][0], rtol=1e-4, atol=1e-7, err_msg=k)
    losses = sum(loss_dict.values())
    assert torch.isfinite(losses)
    losses.backward()
    for k, p in model.named_parameters():
        if f"gradnone__{k}" in ref:
            assert p.grad is None, k
            continue
        nrm = float(ref[f"gradnorm__{k}"][0])
        got = p.grad.cpu()
        np.testing.assert_allclose(float(got.norm()), nrm, rtol=1e-3, atol=1e-9, err_msg=k)
        np.testing.assert_allclose(got.reshape(-1)[:64].numpy(), ref[f"gradhead__{k}"], atol=1e-3 * nrm + 1e-9, rtol=0,
                                   err_msg=k)
    # the scalars the reference's forward logs (CATRE_disR_shared.py:127-164), written by the loss kernels into one
    # device tensor: same keys, same values
    vis = model.vis_scalars.as_dict()
    want = {k[5:].replace("__", "/"): float(v[0]) for k, v in ref.items() if k.startswith("vis__")}
    assert set(vis) == set(want) and len(vis) == 14
    for k in want:
        np.testing.assert_allclose(vis[k], want[k], rtol=2e-4, atol=2e-5, err_msg=k)
    # an optimizer step runs on the HIP-computed gradients and changes the next forward (weights are re-packed)
    before = model.refine(b, n_iter=1)["pose_1"].clone()
    opt.step()
    after = model.refine(b, n_iter=1)["pose_1"]
    assert torch.isfinite(after).all() and (after - before).abs().max() > 0


def test_amp_training_iteration_tracks_fp32():
    """torch.autocast around the forward (the reference's SOLVER.AMP.ENABLED, engine.py:304) switches the forward and
    dgrad row GEMMs to bf16 operands (fp32 accumulate / outputs).  Mixed-precision tolerances: every loss term within
    3e-2 relative (+1e-3 abs) of the fp32 iteration, every large gradient with cosine similarity >= 0.98 and norm within
    10 %; COMPUTE_DTYPE='fp32' forces full precision under autocast."""
    from catre_amd import synth
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg
    from oracle.catre_oracle import y_axis_symmetries

    B, N, M = 8, 256, 192
    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()})
    model.train()
    b = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=17).items()}
    batch_updater_test(cfg, b)
    sym = [y_axis_symmetries(12) if i % 3 == 0 else None for i in range(B)]

    def run(autocast, force=None):
        model.cfg.MODEL.CATRE.COMPUTE_DTYPE = force
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out, ld = model(b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
                            gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"], obj_kps=b["obj_kps"],
                            mean_scales=b["obj_mean_scales"], sym_info=sym, do_loss=True, cur_iter=1)
        sum(ld.values()).backward()
        return ({k: float(v) for k, v in ld.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                out["pose_1"].detach().clone())

    l32, g32, p32 = run(False)
    l16, g16, p16 = run(True)
    lf, gf, pf = run(True, force="fp32")
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = None
    assert torch.equal(pf, p32) and all(torch.equal(gf[k], g32[k]) for k in g32), "COMPUTE_DTYPE=fp32 must ignore autocast"
    assert p16.dtype == torch.float32 and not torch.equal(p16, p32), "autocast did not reach the bf16 GEMMs"
    assert (p16 - p32).abs().max() < 2e-2
    for k in l32:
        assert abs(l16[k] - l32[k]) <= 3e-2 * abs(l32[k]) + 1e-3, (k, l16[k], l32[k])
    checked = 0
    for k, g in g32.items():
        if g.numel() < 4096 or float(g.norm()) < 1e-8:
            continue
        cos = float(torch.nn.functional.cosine_similarity(g.reshape(-1), g16[k].reshape(-1), dim=0))
        ratio = float(g16[k].norm() / g.norm())
        assert cos >= 0.98 and 0.9 <= ratio <= 1.1, (k, cos, ratio)
        checked += 1
    assert checked >= 20


@pytest.mark.parametrize("mode", ["bf16", "split"])
def test_autocast_fused_encoder_forward_matches_the_layerwise_autocast_path(mode):
    """Under autocast the encoder forward of the training path runs on SAVE instances of the bf16-operand inference kernels
    (`catre_train_*_fwd`, compute_dtype = bf16: k_stn3d_bf / k_stnkd_bf / k_trunk_bf2 with fp32 row saves + arg-max) instead of
    one bf16 row GEMM per layer.  Same operand rounding (weights at pack time, activations when they are staged), so against the
    layer-wise autocast forward: refined pose within 2e-3, every saved activation within one bf16 ulp of the layer-wise one
    (the saved rows hold the ROUNDED activations; the feature transform is a bf16 MFMA here and an fp32 kernel there),
    gradients with cosine >= 0.97; pooled arg-max rows agree except where two candidates tie within rounding."""
    from catre_amd import synth, train_ops
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg
    from catre_amd.train_forward import forward_train

    B, N, M = 6, 192, 128   # N/64 = 3: the observed clouds end in a pair that holds ONE tile
    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()})
    model.train()
    b = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=23).items()}
    batch_updater_test(cfg, b)
    p = dict(model.named_parameters())
    gen = torch.Generator().manual_seed(5)
    Gp, Gs = torch.randn(B, 3, 4, generator=gen).to(DEV), torch.randn(B, 3, generator=gen).to(DEV)

    def run(rt):
        model.zero_grad(set_to_none=True)
        with train_ops.amp_mode(mode):
            pose, scale, _ = forward_train(p, model._opts, b["x"], b["tfd_kps"], b["obj_pose_est"], b["obj_scale_est"], b["K"],
                                           b["obj_mean_scales"], rt=rt)
            ((pose * Gp).sum() + (scale * Gs).sum()).backward()
        return pose.detach().clone(), {k: v.grad.clone() for k, v in p.items() if v.grad is not None}

    rt = model._runtime()
    pose_l, g_l = run(None)
    pose_f, g_f = run(rt)
    assert not torch.equal(pose_l, pose_f), "the fused reduced-precision forward was not taken"
    assert (pose_l - pose_f).abs().max() < (2e-3 if mode == "bf16" else 2e-5)
    assert set(g_l) == set(g_f) and len(g_f) == 68
    for k, g in g_l.items():
        if g.numel() < 1024 or float(g.norm()) < 1e-8:
            continue
        cos = float(torch.nn.functional.cosine_similarity(g.reshape(-1), g_f[k].reshape(-1), dim=0))
        # two bf16 pipelines flip single arg-max decisions in front of the pools: the fp32-vs-autocast test above holds 0.98
        if mode == "bf16":
            assert cos >= 0.97 and 0.9 <= float(g_f[k].norm() / g.norm()) <= 1.1, (k, cos)
        else:   # split: fp32-grade on both sides (the test against the fp32 iteration holds 5e-2 relative L2)
            assert cos >= 0.995 and 0.98 <= float(g_f[k].norm() / g.norm()) <= 1.02, (k, cos)
    # the saved rows themselves: fused (bf16-rounded) vs the fp32 kernels' saves rounded the same way
    desc = __import__("catre_amd.hip", fromlist=["points_desc"]).points_desc(b["x"], b["tfd_kps"])
    bufs = {}
    mi = {"bf16": 1, "split": 2}[mode]
    rel = 1e-2 if mode == "bf16" else 1e-4
    for m_ in (0, mi):
        buf = rt.train_encoder_buffers(B, N, M, torch.device(DEV), mode=m_)   # bf16: the rows behind each stack's first layer are bf16
        for v in buf.values():
            v.fill_(0) if v.dtype == torch.int32 else v.fill_(float("nan"))
        rt.train_stn3d(desc, buf, B, N, M, torch.device(DEV), m_)
        trans3 = torch.eye(3, device=DEV).reshape(1, 9).repeat(2 * B, 1).contiguous()
        rt.train_stnkd(desc, trans3, buf, B, N, M, torch.device(DEV), m_)
        trans64 = torch.eye(64, device=DEV).reshape(1, 4096).repeat(2 * B, 1).contiguous()
        rt.train_trunk(desc, trans3, trans64, buf, B, N, M, torch.device(DEV), m_)
        torch.cuda.synchronize()
        bufs[m_] = buf
    got, ref = bufs[mi], bufs[0]
    if mode == "bf16":
        assert all(got[k].dtype == torch.bfloat16 for k in ("a1", "a2", "f1", "f2", "c2", "c3"))
        got = {k: (v.float() if v.dtype == torch.bfloat16 else v) for k, v in got.items()}
    for k in ("a1", "x1", "h1", "pf"):   # inputs of the first reduced GEMMs: the fp32 values (bf16: rounded to bf16)
        want = ref[k].to(torch.bfloat16).float() if mode == "bf16" else ref[k]
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], want) or (got[k] - want).abs().max() <= rel * want.abs().max(), k
    for k in ("a2", "f1", "f2", "c2", "c3", "g_stn", "g_fstn", "g"):
        assert torch.isfinite(got[k]).all(), k
        err = (got[k] - ref[k]).abs().max() / ref[k].abs().max()
        assert err <= 2 * rel, (k, float(err))
    ar = torch.arange(B, device=DEV)
    lo = torch.cat([ar * N, B * N + ar * M])[:, None]                   # every cloud's own rows: [c N, (c+1) N), B N + [c M, (c+1) M)
    hi = lo + torch.cat([torch.full_like(ar, N), torch.full_like(ar, M)])[:, None]
    for k in ("i_stn", "i_fstn", "i"):
        assert (got[k] >= lo).all() and (got[k] < hi).all(), k
        assert float((got[k] == ref[k]).float().mean()) >= (0.9 if mode == "bf16" else 0.995), k


def test_split_training_iteration_matches_fp32():
    """COMPUTE_DTYPE='split' in training: the tiled forward / dgrad / wgrad GEMMs run hi + lo bf16 operands with three
    products (fp32-grade results on the bf16 pipe).  Losses within 1e-5 relative of the fp32 iteration, every gradient
    within 5e-2 relative L2, the refined pose within 2e-5."""
    from catre_amd import synth
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg
    from oracle.catre_oracle import y_axis_symmetries

    B, N, M = 8, 256, 192
    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()})
    model.train()
    b = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=19).items()}
    batch_updater_test(cfg, b)
    sym = [y_axis_symmetries(12) if i % 3 == 0 else None for i in range(B)]

    def run(force):
        model.cfg.MODEL.CATRE.COMPUTE_DTYPE = force
        model.zero_grad(set_to_none=True)
        out, ld = model(b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
                        gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"], obj_kps=b["obj_kps"],
                        mean_scales=b["obj_mean_scales"], sym_info=sym, do_loss=True, cur_iter=1)
        sum(ld.values()).backward()
        return ({k: float(v) for k, v in ld.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                out["pose_1"].detach().clone())

    l32, g32, p32 = run("fp32")
    ls, gs, ps = run("split")
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = None
    assert not torch.equal(ps, p32), "the split kernels did not run"
    assert (ps - p32).abs().max() < 2e-5
    for k in l32:
        assert abs(ls[k] - l32[k]) <= 1e-5 * abs(l32[k]) + 1e-7, (k, ls[k], l32[k])
    # a 1e-5 perturbation flips a few arg-max / ReLU decisions, which moves single gradient entries of the layers in
    # front of a max-pool discretely - so gradients are compared in norm: relative L2 error <= 5e-2 (measured ~1e-2 for
    # the STN's first layers, ~1e-5 behind the pools)
    worst = 0.0
    for k, g in g32.items():
        nrm = float(g.norm())
        if nrm < 1e-10:
            continue
        rel = float((gs[k] - g).norm()) / nrm
        worst = max(worst, rel)
        assert rel <= 5e-2, (k, rel)
        if rel > 1e-3:
            print(f"  {k}: {rel:.2e}")
    print(f"worst relative L2 gradient deviation: {worst:.2e}")


def test_modules_called_on_their_own_run_and_differentiate():
    """The registry modules keep the reference's module interface: PointNetfeat / STN3d / STNkd / ConvOutPerRotHead /
    FC_TransSizeHead called directly (materialised feature tensors, grad mode) run on the layer-wise HIP ops and agree
    with the oracle, values and gradients."""
    from oracle import catre_oracle as O
    from tests.test_hip_parity import build_model

    g = load_golden("refine_b2_small")
    cfg = g["cfg"].__deepcopy__({})
    cfg.MODEL.DEVICE = DEV
    model, sd = build_model(cfg, g["salt"])
    model.train()
    B, N, M = g["B"], g["N"], g["M"]
    x, k = O.pose_apply(g["batch"]["pcl"], g["batch"]["obj_kps"], g["batch"]["obj_pose_est"], g["batch"]["obj_scale_est"])
    sdd = {kk: v.double().requires_grad_(True) for kk, v in sd.items()}
    # PointNetfeat (grad mode) and the two STNs
    feat = model.pcl_net(x.to(DEV))
    want = O.pointnet_feat(x.double(), sdd)
    assert feat.requires_grad and np.abs(feat.detach().cpu().numpy() - want.detach().numpy()).max() <= 2e-5
    tr = model.pcl_net.stn(x.to(DEV))
    wtr, _ = O.stn(x.double(), sdd, "pcl_net.stn", 3)
    assert np.abs(tr.detach().cpu().numpy() - wtr.detach().numpy()).max() <= 2e-5
    h = torch.randn(B, 64, N, generator=torch.Generator().manual_seed(1))
    tf = model.pcl_net.fstn(h.to(DEV))
    wtf, _ = O.stn(h.double(), sdd, "pcl_net.fstn", 64)
    assert np.abs(tf.detach().cpu().numpy() - wtf.detach().numpy()).max() <= 2e-5
    # heads on a materialised [B,1088,N+M] / [B,1091] feature
    kf = O.pointnet_feat(k.double(), sdd)
    rot_feat = torch.cat([want, kf], dim=2).detach()
    r6 = model.rot_head(rot_feat.float().to(DEV))
    wr6 = O.rot_head(rot_feat, sdd)
    assert r6.shape == (B, 6) and np.abs(r6.detach().cpu().numpy() - wr6.detach().numpy()).max() <= 2e-5
    ts_in = torch.randn(B, model.ts_head.in_dim, generator=torch.Generator().manual_seed(2))
    dt, ds = model.ts_head(ts_in.to(DEV))
    wdt, wds = O.ts_head(ts_in.double(), sdd)
    assert np.abs(dt.detach().cpu().numpy() - wdt.detach().numpy()).max() <= 2e-5
    assert np.abs(ds.detach().cpu().numpy() - wds.detach().numpy()).max() <= 2e-5
    (r6.sum() + dt.sum() + ds.sum()).backward()
    (wr6.sum() + wdt.sum() + wds.sum()).backward()
    for name in ("rot_head.rot_head_x.layers.0.weight", "rot_head.rot_head_y.conv_p.weight", "ts_head.linears.0.weight",
                 "ts_head.fc_s.bias"):
        got = dict(model.named_parameters())[name].grad.cpu().double()
        ref = sdd[name].grad
        assert float((got - ref).abs().max()) <= 2e-4 * float(ref.abs().max()) + 1e-9, name


def test_ddp_world1_wraps_and_steps():
    """The reference wraps the model in DistributedDataParallel(find_unused_parameters=True)
    (core/catre/main_catre.py:154-160); world_size 1 over RCCL exercises the reducer hooks on the HIP gradients."""
    import os
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from tests.util import load_train_golden

    g = load_train_golden("train_b4")
    cfg = g["cfg"].__deepcopy__({})
    cfg.MODEL.DEVICE = DEV
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29631")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        model, opt = build_model_optimizer(cfg, is_test=False)
        model.load_state_dict({k: v.to(DEV) for k, v in recipe_sd(cfg, g["salt"]).items()}, strict=True)
        ddp = DistributedDataParallel(model, device_ids=[0], broadcast_buffers=False, find_unused_parameters=True)
        b = {k: v.to(DEV) for k, v in g["batch"].items()}
        batch_updater_test(cfg, b)
        _, loss_dict = ddp(b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
                           gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"], obj_kps=b["obj_kps"],
                           mean_scales=b["obj_mean_scales"], sym_info=g["sym_info"], do_loss=True, cur_iter=1)
        sum(loss_dict.values()).backward()
        nrm = float(g["ref"]["gradnorm__pcl_net.conv4.weight"][0])
        assert abs(float(model.pcl_net.conv4.weight.grad.norm()) - nrm) <= 1e-3 * nrm
        opt.step()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("variant", [
    {},                                                                    # the shipped configuration
    {"ROT_LOSS_TYPE": "L2", "ROT_YAXIS_LOSS_TYPE": "smoothL1"},
    {"TRANS_LOSS_TYPE": "MSE", "SCALE_LOSS_TYPE": "MSE"},
    {"TRANS_LOSS_DISENTANGLE": False, "PM_LOSS_SYM": False},
    {"PM_LW": 0.0, "ROT_LW": 2.0, "TRANS_LW": 0.5},
    # the reference's L2Loss (per-object norm, losses/l2_loss.py) and angular_distance_vec variants (:232-285)
    {"TRANS_LOSS_TYPE": "L2", "SCALE_LOSS_TYPE": "L2", "ROT_YAXIS_LOSS_TYPE": "L2"},
    {"TRANS_LOSS_TYPE": "L2", "TRANS_LOSS_DISENTANGLE": False, "ROT_YAXIS_LOSS_TYPE": "angular"},
])
def test_fused_loss_matches_oracle_values_and_gradients(variant):
    """catre_loss_fwd / catre_loss_bwd (row f1) vs fp64 autograd through the oracle's restatement of
    CATRE_disR_shared.catre_loss, including the symmetry-aware choice of the ground-truth rotation.
    Tolerances: losses 1e-5 rel; gradients 2e-5 of the tensor's max."""
    from catre_amd import synth
    from catre_amd.config import default_cfg
    from catre_amd.losses import catre_loss
    from oracle import catre_oracle as O

    B, M = 7, 150
    cfg = default_cfg(num_pcl=64, num_kps=M, device=DEV)
    for k, v in variant.items():
        cfg.MODEL.CATRE.LOSS_CFG[k] = v
    inp = synth.make_inputs(B, 64, M, seed=29)
    g = torch.Generator().manual_seed(3)
    sym = [O.y_axis_symmetries(12) if i in (1, 4, 5) else None for i in range(B)]
    # a perturbed estimate: gt rotated by a small random rotation, shifted, rescaled
    from oracle.aug_oracle import euler2mat
    dR = euler2mat(torch.randn(B, 3, generator=g) * 0.3)
    out_rot = (dR @ inp["gt_rot"]).contiguous()
    out_rot[1] = inp["gt_rot"][1] @ torch.from_numpy(sym[1][5]).float() @ dR[1]   # closest candidate is not the identity
    out_trans = inp["gt_trans"] + 0.05 * torch.randn(B, 3, generator=g)
    out_scale = inp["gt_scale"] + 0.02 * torch.randn(B, 3, generator=g)

    def leafs(dtype, dev):
        return [t.clone().to(dtype=dtype, device=dev).requires_grad_(True) for t in (out_rot, out_trans, out_scale)]

    r, t, s = leafs(torch.float32, DEV)
    dv = lambda x: x.to(DEV)
    ld = catre_loss(cfg, r, t, s, dv(inp["gt_rot"]), dv(inp["gt_trans"]), dv(inp["gt_scale"]), dv(inp["obj_kps"]), sym)
    w = {k: 1.0 + 0.25 * i for i, k in enumerate(sorted(ld))}   # distinct upstream gradients per term
    sum(w[k] * v for k, v in ld.items()).backward()

    rr, tr, sr = leafs(torch.float64, "cpu")
    dd = lambda x: x.double()
    ref = O.catre_loss(rr, tr, sr, dd(inp["gt_rot"]), dd(inp["gt_trans"]), dd(inp["gt_scale"]), dd(inp["obj_kps"]), sym,
                       cfg.MODEL.CATRE.LOSS_CFG)
    assert set(ref) == set(ld), (sorted(ref), sorted(ld))
    sum(w[k] * v for k, v in ref.items()).backward()
    for k in ref:
        np.testing.assert_allclose(float(ld[k]), float(ref[k]), rtol=1e-5, atol=1e-8, err_msg=k)
    for name, a, b in (("rot", r, rr), ("trans", t, tr), ("scale", s, sr)):
        if b.grad is None:
            assert a.grad is None or float(a.grad.abs().max()) == 0.0, name
            continue
        scale_ref = float(b.grad.abs().max()) + 1e-12
        err = float((a.grad.cpu().double() - b.grad).abs().max()) / scale_ref
        assert err <= 2e-5, (name, err)


@pytest.mark.parametrize("variant", [{}, {"TRANS_LOSS_DISENTANGLE": False}, {"PM_LW": 0.0}])
def test_summing_the_loss_dict_takes_the_precomputed_chain(variant):
    """`sum(loss_dict.values())` (engine.py:318) answers every step of its chain with the running sum the loss kernel wrote:
    the total and the gradients are BIT-equal to the same chain run as plain torch adds; anything off the chain (another
    order, a weighted sum, a sum of two of the terms) is plain torch on plain tensors."""
    from catre_amd import synth
    from catre_amd.config import default_cfg
    from catre_amd.losses import _LossTerm, catre_loss
    from oracle import catre_oracle as O

    B, M = 9, 96
    cfg = default_cfg(num_pcl=64, num_kps=M, device=DEV)
    for k, v in variant.items():
        cfg.MODEL.CATRE.LOSS_CFG[k] = v
    inp = synth.make_inputs(B, 64, M, seed=31)
    g = torch.Generator().manual_seed(5)
    sym = [O.y_axis_symmetries(12) if i in (0, 3) else None for i in range(B)]
    from oracle.aug_oracle import euler2mat
    out_rot = (euler2mat(torch.randn(B, 3, generator=g) * 0.2) @ inp["gt_rot"]).contiguous()
    out_trans = inp["gt_trans"] + 0.05 * torch.randn(B, 3, generator=g)
    out_scale = inp["gt_scale"] + 0.02 * torch.randn(B, 3, generator=g)
    dv = lambda x: x.to(DEV)

    def run(total_of):
        r, t, s = (x.clone().to(DEV).requires_grad_(True) for x in (out_rot, out_trans, out_scale))
        ld = catre_loss(cfg, r, t, s, dv(inp["gt_rot"]), dv(inp["gt_trans"]), dv(inp["gt_scale"]), dv(inp["obj_kps"]), sym)
        tot = total_of(ld)
        tot.backward()
        return ld, tot, [x.grad.clone() if x.grad is not None else None for x in (r, t, s)]

    def plain_chain(ld):
        acc = 0
        for v in ld.values():
            acc = acc + v.as_subclass(torch.Tensor)
        return acc

    def loop_form(ld):
        acc = 0
        for v in ld.values():
            acc += v              # (arrives as add_ on a view of the loss node's buffer: answered out of place)
        return acc

    ld, tot, grads = run(lambda ld: sum(ld.values()))
    ld2, tot2, grads2 = run(plain_chain)
    ld3, tot3, grads3 = run(loop_form)
    assert torch.equal(tot3.detach().as_subclass(torch.Tensor), tot2.detach())
    for a, b in zip(grads3, grads2):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    w = {k: 1.0 + 0.5 * i for i, k in enumerate(ld3)}
    off = 0
    for k, v in ld3.items():
        off += w[k] * v           # a weighted loop: plain torch
    assert type(off) is torch.Tensor
    assert isinstance(tot, _LossTerm) and type(tot2) is torch.Tensor
    assert tot.grad_fn is not None and "Add" not in type(tot.grad_fn).__name__      # no add kernel ran
    assert torch.equal(tot.detach().as_subclass(torch.Tensor), tot2.detach())
    for a, b in zip(grads, grads2):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    # off the chain: plain torch
    vals = list(ld.values())
    assert type(vals[0] + vals[-1]) is torch.Tensor and type(vals[0] * 2.0) is torch.Tensor
    assert type(sum(reversed(vals))) is torch.Tensor if len(vals) > 2 else True
    st = torch.stack(vals)
    assert type(st) is torch.Tensor and torch.equal(st.sum(), st.sum())
    np.testing.assert_allclose(float(st.double().sum()), float(tot), rtol=1e-6)
    # a partial chain is a real tensor too: the first two terms
    part = 0 + vals[0] + vals[1]
    assert torch.equal(part.detach().as_subclass(torch.Tensor), (vals[0].as_subclass(torch.Tensor) + vals[1].as_subclass(torch.Tensor)).detach())


def test_inference_after_a_training_forward_repacks_the_tail_images():
    """A training forward packs without the inference tails' images (CATRE_PACK_F32_TAILS: the ts head's transposed weights
    and the conv_p sums are read by the inference tail kernels only); an inference call on the same model right after - same
    weights, so the same fingerprint - must still get them: R, t, s equal, bit for bit, to a fresh model's."""
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    B, N, M = 5, 128, 128
    cfg, sd, kw, sym, ((model, opt),) = _train_setup(B, N, M, 41, 1)
    fresh, _ = build_model_optimizer(cfg, is_test=True)
    fresh.load_state_dict(sd)
    fresh.eval()
    args = (kw["x"], kw["tfd_kps"])
    ikw = dict(init_pose=kw["init_pose"], init_scale=kw["init_scale"], K_zoom=kw["K_zoom"], mean_scales=kw["mean_scales"])
    with torch.no_grad():
        want = fresh(*args, **ikw)
    _iteration(model, kw, sym)             # training forward + backward: packs the encoder / head images only
    model.eval()
    with torch.no_grad():
        got = model(*args, **ikw)          # no optimizer step in between: the weights are the ones just packed
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("amp", [False, True])
def test_graphed_train_step_replays_the_eager_iteration(amp):
    """GraphedTrainStep (forward + loss + backward + fused Ranger step in one HIP graph) against the eager loop on
    the same batches: same losses, same parameters after every step (the same kernels run in the same order), the
    caller's model / optimizer state untouched by the capture's warm-up, and a changing symmetric / non-symmetric mix.
    amp: the same under torch.autocast (fused bf16-operand encoder forward, bf16-operand dgrad / wgrad GEMMs)."""
    from catre_amd import synth
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg
    from catre_amd.graphed import GraphedTrainStep
    from oracle.catre_oracle import y_axis_symmetries

    B, N, M = 6, 128, 64
    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    sd = {k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()}
    sym12, sym7 = y_axis_symmetries(12), y_axis_symmetries(7)
    batches, syms = [], []
    for i in range(4):
        b = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=60 + i).items()}
        batch_updater_test(cfg, b)
        batches.append(b)
        syms.append([(sym12 if (j + i) % 3 == 0 else (sym7 if (j * i) % 4 == 1 else None)) for j in range(B)])

    def kwargs(b):
        return dict(x=b["x"].contiguous(), tfd_kps=b["tfd_kps"].contiguous(), init_pose=b["obj_pose_est"],
                    init_scale=b["obj_scale_est"], K_zoom=b["K"], gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"],
                    gt_scale=b["gt_scale"], obj_kps=b["obj_kps"], mean_scales=b["obj_mean_scales"])

    # eager reference run
    model_e, opt_e = build_model_optimizer(cfg, is_test=False)
    model_e.load_state_dict(sd)
    eager = []
    for b, s in zip(batches, syms):
        kw = kwargs(b)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out, ld = model_e(kw.pop("x"), kw.pop("tfd_kps"), sym_info=s, do_loss=True, cur_iter=1, **kw)
        sum(ld.values()).backward()
        opt_e.step()
        opt_e.zero_grad(set_to_none=True)
        eager.append(({k: float(v) for k, v in ld.items()}, out["pose_1"].detach().clone(),
                      {k: p.detach().clone() for k, p in model_e.named_parameters()}))

    model_g, opt_g = build_model_optimizer(cfg, is_test=False)
    model_g.load_state_dict(sd)
    step = GraphedTrainStep(model_g, opt_g, kwargs(batches[0]), syms[0], max_sym=12, amp=amp)
    for k, p in model_g.named_parameters():
        assert torch.equal(p, sd[k]), f"capture warm-up changed {k}"
    assert all(st["step"] == 0 for st in opt_g.state.values())
    for i, (b, s) in enumerate(zip(batches, syms)):
        out, ld = step(sym_info=s, **kwargs(b))
        torch.cuda.synchronize()
        want_l, want_pose, want_p = eager[i]
        for k, v in want_l.items():
            np.testing.assert_allclose(float(ld[k]), v, rtol=1e-6, atol=1e-9, err_msg=f"step {i} {k}")
        assert torch.equal(out["pose_1"], want_pose), f"step {i}: pose"
        for k, p in model_g.named_parameters():
            assert torch.equal(p, want_p[k]), f"step {i}: parameter {k}"
    assert all(st["step"] == 4 for st in opt_g.state.values() if "step" in st)
    with pytest.raises(ValueError):
        step(x=torch.zeros(B + 1, 3, N, device=DEV))


def test_vis_scalars_reach_an_active_event_storage(monkeypatch):
    """With detectron2's EventStorage active (engine.py:266) the forward writes the reference's 14 vis/ keys - one copy
    of one device tensor; without a storage nothing is copied."""
    import sys
    import types

    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from tests.util import load_train_golden

    g = load_train_golden("train_b4")
    cfg = g["cfg"].__deepcopy__({})
    cfg.MODEL.DEVICE = DEV
    model, _ = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in recipe_sd(cfg, g["salt"]).items()}, strict=True)
    b = {k: v.to(DEV) for k, v in g["batch"].items()}
    batch_updater_test(cfg, b)
    logged = {}

    class Storage:
        def put_scalars(self, **kw):
            logged.update(kw)

    events = types.ModuleType("detectron2.utils.events")
    events.get_event_storage = lambda: Storage()
    for name in ("detectron2", "detectron2.utils"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    monkeypatch.setitem(sys.modules, "detectron2.utils.events", events)
    call = lambda it: model(b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
                            gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"], obj_kps=b["obj_kps"],
                            mean_scales=b["obj_mean_scales"], sym_info=g["sym_info"], do_loss=True, cur_iter=it)
    call(3)
    assert len(logged) == 14 and all(k.endswith("_3") and k.startswith("vis/") for k in logged)
    np.testing.assert_allclose(logged["vis/error_R_3"], float(g["ref"]["vis__vis__error_R_1"][0]), rtol=2e-4)
    logged.clear()
    model.cfg.MODEL.CATRE.LOG_VIS_SCALARS = False
    call(1)
    assert not logged and model.vis_scalars._host is None  # nothing copied until asked for
    assert abs(model.vis_scalars.as_dict()["vis/error_t_1"] - float(g["ref"]["vis__vis__error_t_1"][0])) < 1e-3


def test_pose_update_backward_with_expanded_gradients():
    """`(pose.sum() + scale.sum()).backward()` hands stride-0 expanded gradients to the pose-update backward: the
    contiguous copies must stay alive until the kernel is enqueued (two temporaries shared one block)."""
    from catre_amd import hip
    from catre_amd import synth
    from catre_amd import train_ops as T
    from catre_amd.config import default_cfg
    from catre_amd.runtime import opts_from_cfg

    B = 9
    o = opts_from_cfg(default_cfg(device=DEV))
    inp = synth.make_inputs(B, 8, 8, seed=3)
    g = torch.Generator().manual_seed(1)
    mk = lambda *shape: (torch.randn(*shape, generator=g) * 0.3).to(DEV)
    rot, dt, ds = mk(B, 6) + 1.0, mk(B, 3) + torch.tensor([0, 0, 1.0], device=DEV), mk(B, 3) * 0.05
    pose0, scale0, K = inp["obj_pose_est"].to(DEV), inp["obj_scale_est"].to(DEV), inp["K"].to(DEV)

    def grads(expanded):
        leaves = [t.clone().requires_grad_(True) for t in (rot, dt, ds)]
        pose, scale = T.pose_update_autograd(*leaves, pose0, scale0, None, K, o)
        if expanded:
            (pose.sum() + scale.sum()).backward()              # both upstream gradients are expanded scalars
        else:
            torch.autograd.backward([pose, scale], [torch.ones_like(pose), torch.ones_like(scale)])
        return [t.grad.clone() for t in leaves]

    for a, b_ in zip(grads(True), grads(False)):
        assert torch.equal(a, b_)
    # forward with non-contiguous inputs (a strided mean_scales view next to a strided K)
    from catre_amd.runtime import pose_update

    o2 = hip.CatreOpts.from_buffer_copy(o)
    o2.scale_base_mean = 1
    ms_wide = torch.rand(B, 6, device=DEV) + 0.1
    K_wide = torch.zeros(B, 3, 6, device=DEV)
    K_wide[:, :, ::2] = K
    p1, s1 = pose_update(rot, dt, ds, pose0, scale0, ms_wide[:, ::2], K_wide[:, :, ::2], o2)
    p2, s2 = pose_update(rot, dt, ds, pose0, scale0, ms_wide[:, ::2].contiguous(), K, o2)
    assert torch.equal(p1, p2) and torch.equal(s1, s2)


# ------------------------------------------------------------------------------------------------- scratch ownership
def _train_setup(B, N, M, seed, n_models=1):
    from catre_amd import synth
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg
    from oracle.catre_oracle import y_axis_symmetries

    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    sd = {k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()}
    b = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=seed).items()}
    batch_updater_test(cfg, b)
    sym = [y_axis_symmetries(12) if j % 3 == 0 else None for j in range(B)]
    kw = dict(x=b["x"].contiguous(), tfd_kps=b["tfd_kps"].contiguous(), init_pose=b["obj_pose_est"],
              init_scale=b["obj_scale_est"], K_zoom=b["K"], gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"],
              gt_scale=b["gt_scale"], obj_kps=b["obj_kps"], mean_scales=b["obj_mean_scales"])
    pairs = []
    for _ in range(n_models):
        model, opt = build_model_optimizer(cfg, is_test=False)
        model.load_state_dict(sd)
        pairs.append((model, opt))
    return cfg, sd, kw, sym, pairs


def _iteration(model, kw, sym):
    kw = dict(kw)
    out, ld = model(kw.pop("x"), kw.pop("tfd_kps"), sym_info=sym, do_loss=True, cur_iter=1, **kw)
    sum(ld.values()).backward()
    return {k: v.detach().clone() for k, v in ld.items()}


@pytest.mark.parametrize("mode", ["fp32", "split"])
def test_two_models_training_on_two_streams_reproduce_their_solo_gradients(mode):
    """SURVEY 8(b) Threading: workspace per stream, re-entrant.  Two models run training iterations CONCURRENTLY on two
    streams (different batch sizes, so their split-K partials and reduction scratch differ in size and content); every
    gradient must equal, bit for bit, what the same model produced alone.  With one scratch buffer per device (round 2)
    the two streams raced on it."""
    from catre_amd import train_ops

    N, M = 256, 128
    setups = [_train_setup(B, N, M, seed, 1) for B, seed in ((12, 71), (7, 72))]
    solo = []
    with train_ops.amp_mode(mode):
        for cfg, sd, kw, sym, ((model, opt),) in setups:
            _iteration(model, kw, sym)
            torch.cuda.synchronize()
            solo.append({k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
            opt.zero_grad(set_to_none=True)
        streams = [torch.cuda.Stream(device=DEV) for _ in setups]
        bad = []
        for rnd in range(12):
            torch.cuda.synchronize()
            for (cfg, sd, kw, sym, ((model, opt),)), st in zip(setups, streams):
                with torch.cuda.stream(st):
                    for _ in range(2):   # back to back: keeps both streams busy at the same time
                        opt.zero_grad(set_to_none=True)
                        _iteration(model, kw, sym)
            torch.cuda.synchronize()
            for i, (cfg, sd, kw, sym, ((model, opt),)) in enumerate(setups):
                for k, p in model.named_parameters():
                    if p.grad is not None and not torch.equal(p.grad, solo[i][k]):
                        bad.append((rnd, i, k))
        assert not bad, f"{len(bad)} gradients differ from the solo run, first: {bad[:4]}"
        keys = {k for k in train_ops._scratch}
        assert len({s.cuda_stream for s in streams} & {k[1] for k in keys}) == 2   # one scratch per stream


def test_graphed_train_step_survives_a_scratch_grow_and_leaves_eager_weights_fresh():
    """(i) ADVICE r2 medium: the packs recorded during capture did not execute - an EAGER training forward issued after
    the capture and before the first replay must still run on the live weights.  (ii) VERDICT r2 weak #2: the graph owns
    the scratch it captured; an eager step at 4x the batch (which outgrows every per-stream cache entry) must not
    recycle it - replays stay bit-identical to the eager loop."""
    from catre_amd.graphed import GraphedTrainStep

    B, N, M = 4, 128, 64
    cfg, sd, kw, sym, ((m_e, o_e), (m_g, o_g)) = _train_setup(B, N, M, 81, n_models=2)
    _, _, kw_big, sym_big, ((m_big, o_big),) = _train_setup(4 * B, N, M, 82)
    want_first = _iteration(m_e, kw, sym)
    o_e.zero_grad(set_to_none=True)

    step = GraphedTrainStep(m_g, o_g, kw, sym, max_sym=12)
    # (i) eager forward on the graphed model right after capture: the warm-up's weights must not be what it sees
    got_first = _iteration(m_g, kw, sym)
    o_g.zero_grad(set_to_none=True)
    for k, v in want_first.items():
        assert torch.equal(v, got_first[k]), f"eager forward after capture ran on stale packed weights: {k}"

    eager = []
    for i in range(3):
        ld = _iteration(m_e, kw, sym)
        o_e.step()
        o_e.zero_grad(set_to_none=True)
        eager.append((ld, {k: p.detach().clone() for k, p in m_e.named_parameters()}))
    for i in range(3):
        if i == 1:  # (ii) a bigger eager step in between, on the SAME stream the replays are issued from and on the
            # capture's own stream key: every cache entry is outgrown and replaced
            from catre_amd import train_ops

            for st in (torch.cuda.current_stream(), step._keep[1]):
                with torch.cuda.stream(st):
                    _iteration(m_big, kw_big, sym_big)
                    o_big.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            assert train_ops.scratch_of(torch.device(DEV), step._keep[1]) is not step._keep[0]
            # churn the allocator so that a recycled block would actually be overwritten
            junk = [torch.randn(1 << 20, device=DEV) for _ in range(32)]
            del junk
        out, ld = step(sym_info=sym, **kw)
        torch.cuda.synchronize()
        for k, v in eager[i][0].items():
            assert torch.equal(ld[k], v), f"replay {i}: {k}"
        for k, p in m_g.named_parameters():
            assert torch.equal(p, eager[i][1][k]), f"replay {i}: parameter {k}"


def test_training_forward_sees_out_of_band_weight_writes():
    """`p.data.copy_()` (EMA, third-party optimizers) bumps neither _version nor the parameter epoch; the
    fused encoder forward must still read the live weights (the training forward re-packs unconditionally)."""
    cfg, sd, kw, sym, ((m_a, o_a), (m_b, o_b)) = _train_setup(3, 128, 64, 91, n_models=2)
    _iteration(m_a, kw, sym)
    o_a.zero_grad(set_to_none=True)
    new = {k: v * 1.01 for k, v in sd.items()}
    for k, p in m_a.named_parameters():
        p.data.copy_(new[k])
    m_b.load_state_dict(new)
    la, lb = _iteration(m_a, kw, sym), _iteration(m_b, kw, sym)
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    for (k, pa), (_, pb) in zip(m_a.named_parameters(), m_b.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad)), k


@pytest.mark.parametrize("B", [2, 16])
def test_stn_stacks_recompute_their_rows_in_the_backward_bit_for_bit(B):
    """fp32 training: the STN stacks store no activation rows (forward on the inference kernels with an arg-max epilogue - the
    one-wave pair kernels from 256 pairs on, B = 16); their row-sparse backward rebuilds y1 / y2 on its live rows with the
    forward kernels' own device code (`catre_op_stn_recompute`).  Against the form that saves the rows
    (`TRAIN_KERNELS.stn_recompute=False`): outputs and every one of the 68 gradients identical BIT FOR BIT - same operands, same
    K order, same summation order in every consumer."""
    from catre_amd import synth
    from catre_amd import train_ops as T
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg
    from catre_amd.train_forward import forward_train

    N = M = 1024
    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=False)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg), 2)
    model.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=True)
    model.train()
    batch = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=17).items()}
    batch_updater_test(cfg, batch)
    gen = torch.Generator().manual_seed(5)
    Gp, Gs = torch.randn(B, 3, 4, generator=gen).to(DEV), torch.randn(B, 3, generator=gen).to(DEV)
    p = dict(model.named_parameters())
    res = {}
    for rec in (False, True):
        model.zero_grad(set_to_none=True)
        with T.train_kernels(stn_recompute=rec):
            pose, scale, _ = forward_train(p, model._opts, batch["x"], batch["tfd_kps"], batch["obj_pose_est"],
                                           batch["obj_scale_est"], batch["K"], batch["obj_mean_scales"], rt=model._runtime())
            ((pose * Gp).sum() + (scale * Gs).sum()).backward()
        res[rec] = (pose.detach().clone(), scale.detach().clone(),
                    {k: v.grad.detach().clone() for k, v in p.items() if v.grad is not None})
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    assert len(res[True][2]) == 68 and sorted(res[True][2]) == sorted(res[False][2])
    for k, g in res[True][2].items():
        assert torch.equal(g, res[False][2][k]), k
