"""fp16-operand inference mode (``cfg.MODEL.CATRE.COMPUTE_DTYPE = "fp16"``): the bf16 mode's structure - GEMM operands
rounded (RNE) at the same points, fp32 accumulation / GroupNorm statistics / FC tails / SO(3) update - with fp16 operands,
the dtype the reference's autocast uses on "cuda" (engine.py:304, TEST.AMP_TEST).

The rounding oracle is the bf16 one (``oracle.catre_oracle.operand_rounding("bf16")``) with its rounding function
``_q`` replaced by an fp16 round trip for the duration of a call.  Tolerances:
  * vs that oracle, ONE ITERATION AT A TIME from the HIP path's own previous estimate: a quarter of the bf16 bars (fp16's
    ulp is 8x finer): 2e-4 abs on R, t, s for zero-centred inputs (measured 1.6e-5 .. 1.5e-4 over the refine goldens), 4e-4
    with ZERO_CENTER_INPUT=False (measured 8.8e-5);
  * free-running over K iterations vs the fp32 REFERENCE goldens: 1e-3 abs (measured 1.4e-4 .. 6.8e-4; the CPU emulation:
    <= 5.8e-4).
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests.util import golden_names, load_golden

EMU_TOL = 2e-4
EMU_TOL_UNCENTRED = 4e-4
FP32_TOL = 1e-3
DEV = "cuda:0"


def _q_fp16(t):
    return t.to(torch.float16).to(t.dtype)


@contextlib.contextmanager
def fp16_rounding(monkeypatch):
    """the oracle with the bf16 mode's rounding points, rounding to fp16"""
    from oracle import catre_oracle as O

    with monkeypatch.context() as mp, O.operand_rounding("bf16"):
        mp.setattr(O, "_q", _q_fp16)
        yield


def _max_dev(out, ref, K):
    return max(np.abs(out[f"{k}_{i}"].numpy() - ref[f"{k}_{i}"]).max() for i in range(1, K + 1) for k in ("pose", "scale"))


def test_fp16_emulation_is_within_1e3_of_the_fp32_reference_and_closer_than_bf16(monkeypatch):
    """CPU: the emulation the GPU tests rely on, against the fp32 reference goldens at every iteration of every refine
    golden, and closer to them than the bf16 emulation on the two goldens DESIGN 5c ranks (3.7e-3 / 7.9e-3 -> 2.3e-4 /
    3.3e-4).  The monkeypatch is undone on leaving the context."""
    from oracle import catre_oracle as O
    from tests.util import recipe_sd

    q0 = O._q
    for name in golden_names():
        g = load_golden(name)
        sd = recipe_sd(g["cfg"], g["salt"])
        with fp16_rounding(monkeypatch):
            assert O._q is _q_fp16
            out16 = O.refine_k(g["batch"], sd, g["cfg"], n_iter=g["K"])
        e16 = _max_dev(out16, g["ref"], g["K"])
        assert e16 <= FP32_TOL, f"{name}: fp16 emulation {e16:.3e} vs the fp32 reference"
        if name in ("refine_b2_n1024", "refine_b1_n2048_k8"):
            with O.operand_rounding("bf16"):
                outbf = O.refine_k(g["batch"], sd, g["cfg"], n_iter=g["K"])
            ebf = _max_dev(outbf, g["ref"], g["K"])
            assert e16 < ebf, f"{name}: fp16 {e16:.3e} not closer than bf16 {ebf:.3e}"
    assert O._q is q0 and O._ROUND["mode"] is None
    out32 = O.refine_k(g["batch"], sd, g["cfg"], n_iter=1)
    assert np.abs(out32["pose_1"].numpy() - g["ref"]["pose_1"]).max() < 2e-5


def _model(cfg, salt, dtype="fp16"):
    from tests.test_hip_parity import build_model

    model, sd = build_model(cfg, salt)
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = dtype
    return model, sd


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_names())
def test_fp16_refine_matches_rounding_oracle_and_fp32_reference(name, monkeypatch):
    from oracle import catre_oracle as O
    from tests.test_hip_parity import to_dev

    g = load_golden(name)
    model, sd = _model(g["cfg"], g["salt"])
    out = model.refine(to_dev(g["batch"]), n_iter=g["K"])
    torch.cuda.synchronize()
    for i in range(1, g["K"] + 1):
        step = dict(g["batch"])  # teacher-forced: the oracle starts iteration i from the HIP estimate i-1
        step["obj_pose_est"] = out[f"pose_{i - 1}"].cpu()
        if g["cfg"].MODEL.REFINE_SCLAE:
            step["obj_scale_est"] = out[f"scale_{i - 1}"].cpu()
        with fp16_rounding(monkeypatch):
            emu = O.refine_k(step, sd, g["cfg"], n_iter=1)
        for key in ("pose", "scale"):
            got = out[f"{key}_{i}"].cpu().numpy()
            e_emu = np.abs(got - emu[f"{key}_1"].numpy()).max()
            e_ref = np.abs(got - g["ref"][f"{key}_{i}"]).max()
            tol = EMU_TOL if g["cfg"].INPUT.ZERO_CENTER_INPUT else EMU_TOL_UNCENTRED
            assert e_emu <= tol, f"{name} {key}_{i}: {e_emu:.3e} vs the fp16 rounding oracle"
            assert e_ref <= FP32_TOL, f"{name} {key}_{i}: {e_ref:.3e} vs the fp32 reference"
    # the fp16 kernels ran: neither the fp32 nor the bf16 bits
    K = g["K"]
    for other in ("fp32", "bf16"):
        model.cfg.MODEL.CATRE.COMPUTE_DTYPE = other
        o = model.refine(to_dev(g["batch"]), n_iter=K)
        assert not torch.equal(o[f"pose_{K}"], out[f"pose_{K}"]), f"{name}: fp16 returned the {other} bits"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["refine_b2_n1024", "refine_b1_n2048_k8"])
def test_fp16_is_closer_to_the_fp32_reference_than_bf16(name):
    from tests.test_hip_parity import to_dev

    g = load_golden(name)
    K = g["K"]
    model, _ = _model(g["cfg"], g["salt"])
    o16 = model.refine(to_dev(g["batch"]), n_iter=K)
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = "bf16"
    obf = model.refine(to_dev(g["batch"]), n_iter=K)
    for key in (f"pose_{K}", f"scale_{K}"):
        e16 = np.abs(o16[key].cpu().numpy() - g["ref"][key]).max()
        ebf = np.abs(obf[key].cpu().numpy() - g["ref"][key]).max()
        assert e16 < ebf, f"{name} {key}: fp16 {e16:.3e} vs bf16 {ebf:.3e}"


@pytest.mark.gpu
def test_fp16_ragged_and_full_size_properties(monkeypatch):
    """Ragged tiles against the rounding oracle; at the full config-5 shape finite outputs, R in SO(3), determinism and
    batch-row independence."""
    from catre_amd import synth
    from oracle import catre_oracle as O
    from tests.test_hip_parity import to_dev

    cfg = load_golden("refine_b3_ragged")["cfg"].__deepcopy__({})
    for (B, N, M) in [(1, 1000, 500), (2, 65, 1), (3, 127, 130)]:
        cfg2 = cfg.__deepcopy__({})
        cfg2.INPUT.NUM_PCL, cfg2.INPUT.NUM_KPS = N, M
        cfg2.MODEL.CATRE.ROT_HEAD.INIT_CFG.num_points = N + M
        m2, sd2 = _model(cfg2, 3)
        b = synth.make_inputs(B, N, M, seed=40 + B)
        out = m2.refine(to_dev(b), n_iter=1)
        with fp16_rounding(monkeypatch):
            emu = O.refine_k(b, sd2, cfg2, n_iter=1)
        for key in ("pose_1", "scale_1"):
            assert np.abs(out[key].cpu().numpy() - emu[key].numpy()).max() <= EMU_TOL, (B, N, M, key)

    B, N, M, K = 256, 2048, 1024, 8  # BASELINE.json config 5 at its full per-GPU batch
    cfg5 = cfg.__deepcopy__({})
    cfg5.INPUT.NUM_PCL, cfg5.INPUT.NUM_KPS = N, M
    cfg5.MODEL.CATRE.ROT_HEAD.INIT_CFG.num_points = N + M
    m5, _ = _model(cfg5, 0)
    b = to_dev(synth.make_inputs(B, N, M, seed=5))
    o1 = m5.refine(b, n_iter=K)
    o2 = m5.refine(b, n_iter=K)
    R = o1[f"pose_{K}"][:, :3, :3]
    assert torch.isfinite(o1[f"pose_{K}"]).all() and torch.isfinite(o1[f"scale_{K}"]).all()
    assert (R @ R.transpose(1, 2) - torch.eye(3, device=R.device)).abs().max() < 1e-4
    assert (torch.linalg.det(R) - 1).abs().max() < 1e-4
    assert torch.equal(o1[f"pose_{K}"], o2[f"pose_{K}"]), "fp16 path must be deterministic"
    half = {k: (v[: B // 2] if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for k, v in b.items()}
    o3 = m5.refine(half, n_iter=K)
    assert torch.equal(o3[f"pose_{K}"], o1[f"pose_{K}"][: B // 2]), "objects must be independent of their batch"


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,M", [(40, 1024, 1024), (130, 300, 100), (48, 1000, 500)])
def test_fp16_pair_kernels_return_the_bits_of_the_tile_kernels(B, N, M):
    """Grids of >= 512 tile pairs take the 128-point forms (k_*_hf2), smaller ones the 64-point forms: same bits."""
    from catre_amd import synth
    from tests.test_hip_parity import to_dev

    TN, TM = -(-N // 64), -(-M // 64)
    assert B * ((TN + 1) // 2 + (TM + 1) // 2) >= 512 > 3 * ((TN + 1) // 2 + (TM + 1) // 2)
    cfg = load_golden("refine_b3_ragged")["cfg"].__deepcopy__({})
    cfg.INPUT.NUM_PCL, cfg.INPUT.NUM_KPS = N, M
    cfg.MODEL.CATRE.ROT_HEAD.INIT_CFG.num_points = N + M
    model, _ = _model(cfg, 2)
    b = to_dev(synth.make_inputs(B, N, M, seed=60 + B))
    big = model.refine(b, n_iter=2)
    for idx in ([0, 1, 2], [B - 3, B // 2, B - 1]):
        sub = {k: v[idx].contiguous() for k, v in b.items()}
        small = model.refine(sub, n_iter=2)
        for key in ("pose_1", "scale_1", "pose_2", "scale_2"):
            assert torch.equal(small[key], big[key][idx]), (key, idx)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [4.0, -8.0])
def test_fp16_rot_head_with_an_offset_second_layer_matches_the_rounding_oracle(offset, monkeypatch):
    """The GroupNorm-1 partials of k_rot_l1_hf with group means far from zero (layer-1 bias shifted by `offset`), full
    and ragged tiles, one iteration against the rounding oracle."""
    from catre_amd import synth
    from oracle import catre_oracle as O
    from tests.test_hip_parity import to_dev

    g = load_golden("refine_b3_ragged")
    for (B, N, M) in [(3, 128, 128), (2, 100, 70)]:
        cfg = g["cfg"].__deepcopy__({})
        cfg.INPUT.NUM_PCL, cfg.INPUT.NUM_KPS = N, M
        cfg.MODEL.CATRE.ROT_HEAD.INIT_CFG.num_points = N + M
        model, sd = _model(cfg, 2)
        sd = {k: v.clone() for k, v in sd.items()}
        for h in ("x", "y"):
            sd[f"rot_head.rot_head_{h}.layers.3.bias"] += offset
        model.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=True)
        b = synth.make_inputs(B, N, M, seed=60 + B)
        out = model.refine(to_dev(b), n_iter=1)
        with fp16_rounding(monkeypatch):
            emu = O.refine_k(b, sd, cfg, n_iter=1)
        for key in ("pose_1", "scale_1"):
            assert np.abs(out[key].cpu().numpy() - emu[key].numpy()).max() <= EMU_TOL, (offset, B, N, M, key)


@pytest.mark.gpu
def test_fp16_selection_module_loop_autocast_and_training_guard():
    """"fp16" and "float16" select the same bits; the module loop (batch_updater_test + forward) equals the fused refine at
    every iteration; autocast(float16) with COMPUTE_DTYPE unset keeps selecting the bf16 kernels; the training forward
    refuses the mode."""
    from catre_amd.batching import batch_updater_test
    from tests.test_hip_parity import to_dev

    g = load_golden("refine_b3_ragged")
    model, _ = _model(g["cfg"], g["salt"])
    batch = to_dev(g["batch"])
    fused = model.refine(batch, n_iter=g["K"])
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = "float16"
    alias = model.refine(batch, n_iter=g["K"])
    K = g["K"]
    assert torch.equal(alias[f"pose_{K}"], fused[f"pose_{K}"]) and torch.equal(alias[f"scale_{K}"], fused[f"scale_{K}"])
    b = dict(batch)
    poses_est = scales_est = None
    with torch.no_grad():
        for i in range(1, K + 1):
            batch_updater_test(model.cfg, b, poses_est=poses_est, scales_est=scales_est)
            o = model(b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
                      mean_scales=b["obj_mean_scales"], do_loss=False, cur_iter=i)
            poses_est, scales_est = o[f"pose_{i}"], o[f"scale_{i}"]
            assert torch.equal(poses_est, fused[f"pose_{i}"]) and torch.equal(scales_est, fused[f"scale_{i}"]), i

    b = dict(batch)
    batch_updater_test(model.cfg, b)
    args = (b["x"], b["tfd_kps"])
    kw = dict(init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"], mean_scales=b["obj_mean_scales"],
              do_loss=False, cur_iter=1)
    with torch.no_grad():
        p16 = model(*args, **kw)["pose_1"]
        model.cfg.MODEL.CATRE.COMPUTE_DTYPE = "bf16"
        pbf = model(*args, **kw)["pose_1"]
        model.cfg.MODEL.CATRE.COMPUTE_DTYPE = None
        with torch.autocast("cuda", dtype=torch.float16):
            p_amp = model(*args, **kw)["pose_1"]
    assert torch.equal(p_amp, pbf) and not torch.equal(p16, pbf)

    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = "fp16"
    zeros3 = torch.zeros(b["x"].shape[0], 3, device=DEV)
    eye = torch.eye(3, device=DEV).expand(b["x"].shape[0], 3, 3).contiguous()
    with pytest.raises(NotImplementedError, match="bf16"):
        model(*args, **dict(kw, do_loss=True), gt_ego_rot=eye, gt_trans=zeros3, gt_scale=zeros3 + 1,
              obj_kps=b["obj_kps"])


@pytest.mark.gpu
def test_switching_modes_never_reads_a_stale_or_missing_pack():
    """One model switched bf16 -> fp16 -> fp32 -> fp16 returns, each time, the bits a fresh model returns in that mode (the
    packed-weight cache repacks with the union when the fp16 packs are first wanted)."""
    from catre_amd import synth
    from catre_amd.config import default_cfg
    from tests.test_hip_parity import to_dev

    cfg = default_cfg(num_pcl=256, num_kps=128, n_iter=2, device=DEV)
    batch = to_dev(synth.make_inputs(3, 256, 128, seed=91))
    want = {}
    for mode in ("bf16", "fp16", "fp32"):
        fresh, _ = _model(cfg, 4, mode)
        want[mode] = fresh.refine(batch, n_iter=2)
    model, _ = _model(cfg, 4, "bf16")
    for mode in ("bf16", "fp16", "fp32", "fp16"):
        model.cfg.MODEL.CATRE.COMPUTE_DTYPE = mode
        got = model.refine(batch, n_iter=2)
        for k in ("pose_1", "pose_2", "scale_2"):
            assert torch.equal(got[k], want[mode][k]), (mode, k)


@pytest.mark.gpu
@pytest.mark.parametrize("B,K", [(2, 3), (12, 2)])
def test_fp16_refine_k_from_equals_refine_k_with_slot0_prefilled(B, K):
    from catre_amd import hip, synth
    from catre_amd.config import default_cfg
    from tests.test_hip_parity import to_dev

    N, M = 256, 128
    cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=K, device=DEV)
    model, _ = _model(cfg, 3)
    batch = to_dev(synth.make_inputs(B, N, M, seed=77))
    out = model.refine(batch, n_iter=K)  # catre_refine_k_from
    rt, lib = model._runtime(), hip.load()
    dev = batch["pcl"].device
    opts = model._inference_opts()
    assert opts.compute_dtype == hip.DTYPE_F16
    prm, packed = rt.params(dev, hip.PACK_ALL | hip.PACK_F16)
    ws = rt.workspace(B, N, M, dev)
    poses = torch.empty(K + 1, B, 3, 4, device=dev)
    scales = torch.empty(K + 1, B, 3, device=dev)
    poses[0].copy_(batch["obj_pose_est"])
    scales[0].copy_(batch["obj_scale_est"])
    hip.check(lib.catre_refine_k(hip.ptr(batch["pcl"]), hip.ptr(batch["obj_kps"]), hip.ptr(batch["obj_mean_scales"]),
                                 hip.ptr(batch["K"]), prm, hip.ptr(packed), ctypes.byref(opts), hip.ptr(poses),
                                 hip.ptr(scales), hip.ptr(ws), ws.numel(), B, N, M, K, hip.stream_ptr(dev)), "catre_refine_k")
    torch.cuda.synchronize()
    for i in range(K + 1):
        assert torch.equal(out[f"pose_{i}"], poses[i]) and torch.equal(out[f"scale_{i}"], scales[i]), i


@pytest.mark.gpu
def test_fp16_graphed_refine_replays_the_eager_loop():
    """GraphedRefine in fp16: the bits of the eager fp16 refine for new inputs, after in-place updates of an encoder conv
    weight and a rotation-head weight (the fp16 packs are outside PACK_ALL: the replay must re-pack them, and is called
    BEFORE any eager refine could do it), and with two instances replaying on two streams."""
    from catre_amd import synth
    from catre_amd.config import default_cfg
    from catre_amd.graphed import GraphedRefine
    from tests.test_hip_parity import to_dev

    model, _ = _model(default_cfg(), 0)
    b0, b1 = (to_dev(synth.make_inputs(2, 1024, 1024, seed=s)) for s in (81, 82))
    g = GraphedRefine(model, b0, n_iter=3)
    for b in (b0, b1, b0):
        want = model.refine(b, n_iter=3)
        got = g(b)
        for k in ("pose_0", "pose_1", "pose_3", "scale_3"):
            assert torch.equal(got[k], want[k]), k
    before = {k: v.clone() for k, v in g(b1).items()}
    with torch.no_grad():  # in-place updates: same storage, new values, read only through the fp16 packs
        model.pcl_net.conv4.weight.mul_(1.25)
        model.rot_head.rot_head_x.layers[3].weight.mul_(0.75)
    got = {k: v.clone() for k, v in g(b1).items()}  # no eager refine in between
    fresh, _ = _model(default_cfg(), 0)
    fresh.load_state_dict(model.state_dict(), strict=True)
    want = fresh.refine(b1, n_iter=3)
    assert not torch.equal(got["pose_3"], before["pose_3"]), "the weight update did not reach the replay"
    for k in ("pose_1", "pose_3", "scale_3"):
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(model.refine(b1, n_iter=3)[k], want[k]), k
    g2 = GraphedRefine(model, b0, n_iter=3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    w0, w1 = model.refine(b0, n_iter=3)["pose_3"].clone(), want["pose_3"].clone()
    torch.cuda.synchronize()
    for _ in range(5):
        with torch.cuda.stream(s1):
            o1 = g(b1)
        with torch.cuda.stream(s2):
            o2 = g2(b0)
    torch.cuda.synchronize()
    assert torch.equal(o1["pose_3"], w1) and torch.equal(o2["pose_3"], w0)


@pytest.mark.gpu
def test_four_modes_on_four_concurrent_streams_return_their_single_stream_bits():
    """One model, four streams, one compute mode each (fp16, bf16, split, fp32), 20 interleaved rounds: every call returns
    the bits it returns alone (each mode reads its own packs of one shared image, each stream its own workspace).  A
    correctness check of the pack / workspace sharing, not a stress test."""
    from catre_amd import synth
    from catre_amd.config import default_cfg
    from tests.test_hip_parity import build_model, to_dev

    model, _ = build_model(default_cfg(), 0)
    modes = ("fp16", "bf16", "split", "fp32")

    def refine(mode, b):  # the mode is read on the host when the call is issued
        model.cfg.MODEL.CATRE.COMPUTE_DTYPE = mode
        return model.refine(b, n_iter=3)

    batches = [to_dev(synth.make_inputs(b, 1024, 1024, seed=70 + i)) for i, b in enumerate((1, 2, 3, 1))]
    want = [refine(mode, b) for mode, b in zip(modes, batches)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in modes]
    outs = [None] * len(modes)
    for _ in range(20):
        for i, (mode, st) in enumerate(zip(modes, streams)):
            with torch.cuda.stream(st):
                outs[i] = refine(mode, batches[i])
        torch.cuda.synchronize()
        for mode, o, w in zip(modes, outs, want):
            assert torch.equal(o["pose_3"], w["pose_3"]) and torch.equal(o["scale_3"], w["scale_3"]), mode


@pytest.mark.gpu
def test_training_forward_entry_points_refuse_the_fp16_dtype():
    """compute_dtype = CATRE_DTYPE_F16 (3) outside the fused refine: CATRE_ERR_UNSUPPORTED (-4), not a launch."""
    from catre_amd import hip, synth
    from catre_amd.config import default_cfg

    B, N, M = 2, 128, 64
    model, _ = _model(default_cfg(num_pcl=N, num_kps=M, n_iter=1, device=DEV), 0)
    rt, lib = model._runtime(), hip.load()
    dev = torch.device(DEV)
    prm, packed = rt.params(dev)
    ws = rt.workspace(B, N, M, dev)
    b = synth.make_inputs(B, N, M, seed=3)
    x = b["pcl"].to(DEV).transpose(1, 2)
    k = b["obj_kps"].to(DEV).transpose(1, 2)
    pts = hip.points_desc(x, k)
    C = 2 * B
    a1, a2 = torch.empty(B * (N + M), 64, device=DEV), torch.empty(B * (N + M), 128, device=DEV)
    gbuf, ibuf = torch.empty(C, 1024, device=DEV), torch.empty(C, 1024, dtype=torch.int32, device=DEV)
    assert hip.DTYPE_F16 == 3
    rc = lib.catre_train_stn3d_fwd(ctypes.byref(pts), prm, hip.ptr(packed), hip.ptr(a1), hip.ptr(a2), hip.ptr(gbuf),
                                   hip.ptr(ibuf), hip.ptr(ws), ws.numel(), B, N, M, hip.DTYPE_F16, hip.stream_ptr(dev))
    assert rc == -4, rc
    rc = lib.catre_train_stn3d_fwd(ctypes.byref(pts), prm, hip.ptr(packed), hip.ptr(a1), hip.ptr(a2), hip.ptr(gbuf),
                                   hip.ptr(ibuf), hip.ptr(ws), ws.numel(), B, N, M, hip.DTYPE_F32, hip.stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    # the other training forwards, and the operator entry points that take a compute_dtype.  Every buffer is a real
    # allocation large enough for the shapes; for the operators a dtype outside the enum is a BAD_ARG (-1), so -4 is the
    # fp16 guard answering, not the generic validation.
    big = torch.zeros(1 << 22, device=DEV)
    nrows = torch.full((1,), B * (N + M), dtype=torch.int32, device=DEV)
    P, st = hip.ptr(big), hip.stream_ptr(dev)
    R, J, Kc = B * (N + M), 32, 32
    for dt in (hip.DTYPE_F16,):
        assert lib.catre_train_stnkd_fwd(ctypes.byref(pts), P, prm, hip.ptr(packed), P, P, P, P, hip.ptr(ws), ws.numel(), B,
                                         N, M, dt, st) == -4
        assert lib.catre_train_trunk_fwd(ctypes.byref(pts), P, P, prm, hip.ptr(packed), P, P, P, P, P, P, P, hip.ptr(ws),
                                         ws.numel(), B, N, M, dt, st) == -4
        assert lib.catre_train_rot_fwd(P, P, prm, hip.ptr(packed), P, P, P, P, P, hip.ptr(ws), ws.numel(), B, N, M, dt,
                                       st) == -4
    ops = {
        "catre_op_gemm_rows_gn": lambda dt: lib.catre_op_gemm_rows_gn(P, Kc, P, P, 0, P, J, J, Kc, B, N, M, None, dt, st),
        "catre_op_gemm_rows_cloudbias": lambda dt: lib.catre_op_gemm_rows_cloudbias(P, Kc, P, P, P, J, J, Kc, B, N, M, dt, st),
        "catre_op_gemm_rows_n": lambda dt: lib.catre_op_gemm_rows_n(P, Kc, None, 0, P, P, None, 0, P, J, R, J, Kc, 0,
                                                                  hip.ptr(nrows), dt, st),
        "catre_op_gemm_rows_nr": lambda dt: lib.catre_op_gemm_rows_nr(P, Kc, None, 0, P, P, None, 0, None, P, J, R, J, Kc, 0,
                                                                    hip.ptr(nrows), dt, st),
        "catre_op_gemm_tn_bias_lp": lambda dt: lib.catre_op_gemm_tn_bias_lp(P, J, None, 0, P, Kc, P, P, J, Kc, R, 0,
                                                                          hip.ptr(ws), ws.numel(), dt, st),
        "catre_op_gemm_tn_bias_n": lambda dt: lib.catre_op_gemm_tn_bias_n(P, J, None, 0, P, Kc, P, P, J, Kc, R, 0, hip.ptr(ws),
                                                                        ws.numel(), hip.ptr(nrows), dt, st),
        "catre_op_gemm_tn_bias_nr": lambda dt: lib.catre_op_gemm_tn_bias_nr(P, J, None, 0, P, Kc, None, P, P, J, Kc, R, 0,
                                                                          hip.ptr(ws), ws.numel(), hip.ptr(nrows), dt, st),
        "catre_op_fc_bwd": lambda dt: lib.catre_op_fc_bwd(P, J, None, P, Kc, P, Kc, P, P, P, 8, J, Kc, Kc, dt, st),
    }
    for name, call in ops.items():
        assert call(7) == -1, name
        assert call(hip.DTYPE_F16) == -4, name
    torch.cuda.synchronize()
