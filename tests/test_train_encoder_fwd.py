"""The fused training encoder forward (`catre_train_stn3d_fwd`, `catre_train_stnkd_fwd`, `catre_train_trunk_fwd`) in every
kernel form a training batch takes: the saved activation rows, the pooled features and the arg-max rows, against the
plain fp64 reference of tests/train_encoder_ref.py.

Inputs: `synth.make_inputs` posed like `batch_updater_test`, recipe weights, per-cloud transforms `I + 0.3 randn` (3 x 3)
and `I + 0.05 randn` (64 x 64) that are neither identities nor the STNs' own, every buffer prefilled with NaN / -1.  The
form each case takes is asserted through `hip.form_decision` with the live switch word.

a. Rows.  Every layer's saved output against fp64 `relu(W x + b)` of the kernel's OWN saved input row (teacher-forced; bf16:
   operands rounded where the kernels round them).  Bounds (train_encoder_ref.bound): fp32 atol = rtol = 2e-5; split atol
   1e-4, rtol 2e-5; bf16 2e-5 max|want|, plus 2^-8 |want| for a bf16 tensor; h1 / pf of bf16 - fp32 tensors holding bf16
   values - must be bf16-representable and lie between the roundings of want -+ 2e-5 max|want|.
b. Pools against the reference pool of the saved last input at the same bound; fp32: bit-equal to the inference kernels'.
c. Arg-max rows: inside their own cloud; the reference value at the reported row within the bound of the reference
   maximum; exactly the reference's row (the first row of the winning input point) wherever it beats every other input
   point by more than twice the bound; STN channels with a maximum <= 0 carry no gradient and need only be in range.  The
   share of pairs the margin leaves out is capped at 5 % (fp32, bf16) and 15 % (split).
d. First maximum, no margin: clouds of one repeated point, of one repeated tile, of tiles whose second half mirrors the first.
e. Batch independence: clouds of the large grids, run alone as a B = 3 batch in another kernel form, give the same bits.

Observed on an MI355X, worst |got - expected| (its bound) over the cases of a mode, and the share of pairs inside the margin:
  fp32   a1 3.4e-8 (2.9e-5)  a2 1.2e-7 (3.0e-5)  x1 2.0e-8 (2.5e-5)  h1 6.7e-8 (3.3e-5)  f1 2.3e-7 (3.3e-5)  f2 1.7e-7 (3.2e-5)
         pf 2.5e-7 (3.3e-5)  c2 2.1e-7 (3.4e-5)  c3 3.4e-7 (3.9e-5)  g_stn 2.0e-7 (3.1e-5)  g_fstn 2.9e-7 (3.6e-5)  g 5.4e-7 (4.1e-5)
         inside the margin: i_stn 2.27 %, i_fstn 2.31 %, i 2.17 % (cap 5 %)
  split  a1 1.9e-6 (1.1e-4)  a2 3.1e-6 (1.1e-4)  x1 2.0e-8 (1.0e-4)  h1 4.4e-8 (1.1e-4)  f1 3.7e-6 (1.1e-4)  f2 3.9e-6 (1.1e-4)
         pf 1.5e-7 (1.1e-4)  c2 3.5e-6 (1.1e-4)  c3 5.9e-6 (1.2e-4)  g_stn 2.4e-6 (1.1e-4)  g_fstn 3.1e-6 (1.1e-4)  g 3.3e-6 (1.2e-4)
         inside the margin: i_stn 8.68 %, i_fstn 7.91 %, i 7.89 % (cap 15 %)
  bf16   a1 9.8e-4 (1.8e-3)  a2 9.8e-4 (1.8e-3)  x1 2.1e-8 (4.4e-6)  f1 1.9e-3 (2.2e-3)  f2 2.0e-3 (2.7e-3)  c2 2.0e-3 (2.7e-3)
         c3 2.0e-3 (3.3e-3)  g_stn 7.0e-8 (1.2e-5)  g_fstn 1.1e-7 (1.7e-5)  g 2.6e-7 (2.0e-5)   (the bf16 tensors' error IS their
         one rounding: half a bf16 step of values in [0.25, 1))
         h1, pf: no element outside the rounded interval, want -+ 1.2e-5; at most one bf16 step (4.9e-4, 9.8e-4) from rne(want),
         where a rounding boundary lies inside it
         inside the margin: i_stn 1.19 %, i_fstn 1.61 %, i 1.85 % (cap 5 %)
Every arg-max row outside the margin was the reference's, in every case; the three crafted inputs and the batch-independence
cases passed with no exception in all modes.
"""
import functools

import pytest
import torch

from tests import train_encoder_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RT_MODE = {"fp32": 0, "bf16": 1, "split": 2}            # `mode` of HipRuntime.train_*; hip.MODES numbers the decision's
ROWS = ("a1", "a2", "x1", "h1", "f1", "f2", "pf", "c2", "c3")
POOLS = (("g_stn", "i_stn", "y_stn", True), ("g_fstn", "i_fstn", "y_fstn", True), ("g", "i", "y", False))
STAGES = ("stn3d", "stnkd", "trunk")
RS1 = dict(stn3d="train_rs1", stnkd="train_rs1", trunk="train_rs1")
WAVE4 = dict(RS1, trunk="train_wave4")
SPLIT = dict.fromkeys(STAGES, "train_split")
CASES = [
    ("fp32", (1, 64, 64), RS1),                         # the smallest grid: one tile per cloud
    ("fp32", (2, 192, 64), RS1),                        # 3 tiles and 1 tile per cloud
    ("fp32", (33, 128, 128), WAVE4),                    # 132 tiles: the trunk's one wave per SIMD
    ("fp32", (64, 192, 192), WAVE4),                    # the rows-saved side of the 256-pair grid
    ("split", (2, 192, 64), SPLIT),
    ("split", (33, 128, 128), SPLIT),
    ("bf16", (2, 192, 64), dict(stn3d="train_bf", stnkd="train_bf", trunk="train_bf_pair")),   # a one-tile pair (N), a half-empty cloud (M)
    ("bf16", (128, 192, 192), dict.fromkeys(STAGES, "train_bf_pair")),                           # 512 pairs, every cloud's last one half empty
]


def _switch_word():
    """the live switch word: ids 0 - 9 as catre_form_switch reads them back; the STN arms (10 - 12) follow the environment
    only and no training form reads them"""
    from catre_amd import hip

    return sum(1 << b for n, b in hip.SWITCH_BITS.items() if b >= 10 or hip.form_switch(n))


def _assert_forms(mode, B, N, M, want, stn_rows=True):
    from catre_amd import hip

    for stage in STAGES:
        d = hip.form_decision(stage, mode, B, N, M, _switch_word(), save=True, rows=stn_rows or stage == "trunk", bf_pair_min=512)
        assert d is not None and d[0] == want[stage], (stage, mode, B, N, M, d, want[stage])


@functools.lru_cache(maxsize=None)
def _model(N, M):
    from catre_amd import synth
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=False)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    model.train()
    return model, {k: v.to(DEV) for k, v in sd.items() if k.startswith("pcl_net.")}


@functools.lru_cache(maxsize=None)
def _inputs(B, N, M):
    """(points [B*(N+M),3], trans3 [2B,9], trans64 [2B,4096]) on the device"""
    return tuple(t.to(DEV) for t in (R.case_points(B, N, M, R.SEED),) + R.transforms(B, R.SEED))


def _run(pts, t3, t64, B, N, M, mode, stn_rows=True):
    """the three launches on NaN / -1 prefilled buffers -> the buffers"""
    from catre_amd import hip

    dev = torch.device(DEV)
    rt = _model(N, M)[0]._runtime()
    assert pts.is_contiguous() and pts.shape == (B * (N + M), 3) and t3.shape == (2 * B, 9) and t64.shape == (2 * B, 4096)
    x, k = pts[:B * N].view(B, N, 3).permute(0, 2, 1), pts[B * N:].view(B, M, 3).permute(0, 2, 1)
    desc = hip.points_desc(x, k)
    m = RT_MODE[mode]
    buf = rt.train_encoder_buffers(B, N, M, dev, stn_rows=stn_rows, mode=m)
    for v in buf.values():
        if v is not None:
            v.fill_(-1) if v.dtype == torch.int32 else v.fill_(float("nan"))
    packs = rt.train_stn3d(desc, buf, B, N, M, dev, m)
    rt.train_stnkd(desc, t3, buf, B, N, M, dev, m, packs=packs)
    rt.train_trunk(desc, t3, t64, buf, B, N, M, dev, m, packs=packs)
    torch.cuda.synchronize()
    return buf


def _inference_pools(pts, t3, t64, B, N, M):
    """the inference kernels' pools on the same inputs: catre_stn3d_pool, catre_stnkd_pool, catre_trunk gfeat[:, :1024]"""
    import ctypes

    from catre_amd import hip

    lib, dev = hip.load(), torch.device(DEV)
    rt = _model(N, M)[0]._runtime()
    x, k = pts[:B * N].view(B, N, 3).permute(0, 2, 1), pts[B * N:].view(B, M, 3).permute(0, 2, 1)
    desc = hip.points_desc(x, k)
    prm, packed = rt.params(dev, hip.PACK_ALL)
    ws, st = rt.workspace(B, N, M, dev), hip.stream_ptr(dev)
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    p3, p64, gfeat, pointfeat = e(2 * B, 1024), e(2 * B, 1024), e(2 * B, 1088), e(B * (N + M), 64)
    hip.check(lib.catre_stn3d_pool(ctypes.byref(desc), prm, hip.ptr(packed), hip.ptr(p3), hip.ptr(ws), ws.numel(), B, N, M, st),
              "catre_stn3d_pool")
    hip.check(lib.catre_stnkd_pool(ctypes.byref(desc), hip.ptr(t3), prm, hip.ptr(packed), hip.ptr(p64), hip.ptr(ws), ws.numel(),
                                   B, N, M, st), "catre_stnkd_pool")
    hip.check(lib.catre_trunk(ctypes.byref(desc), hip.ptr(t3), hip.ptr(t64), prm, hip.ptr(packed), hip.ptr(gfeat),
                              hip.ptr(pointfeat), hip.ptr(ws), ws.numel(), B, N, M, st), "catre_trunk")
    torch.cuda.synchronize()
    return {"g_stn": p3, "g_fstn": p64, "g": gfeat[:, :1024]}


def _in_own_cloud(idx, B, N, M):
    lo, hi = R.cloud_ranges(B, N, M, idx.device)
    return bool(((idx >= lo[:, None]) & (idx < hi[:, None])).all())


def check_outputs(buf, pts, t3, t64, sd, mode, B, N, M, say=print):
    """assertions a - c of the module docstring on the buffers of one rows-saved call -> (the teacher-forced reference,
    {name: figure})"""
    ref = R.encoder_rows(pts, t3, t64, sd, mode, B, N, M, saved=buf)
    first = R.first_identical_row(pts, B, N, M)
    seen = {}
    # a. the saved rows
    for k in ROWS:
        got = buf[k]
        assert got.dtype == (torch.bfloat16 if mode == "bf16" and k in R.BF16_TENSORS else torch.float32), k
        assert not bool(torch.isnan(got).any()), f"{k}: elements never written"
        if mode == "bf16" and k in R.HOLDS_BF16:
            assert torch.equal(got.float(), got.to(torch.bfloat16).float()), f"{k}: holds values that are no bf16"
        bad, err, tol = R.rows_error(got, ref[k], mode, k)
        say(f"{mode} {(B, N, M)} {k}: worst error {err:.2e} (bound {tol:.2e}), {bad} elements out of bound")
        seen[k] = (err, tol)
        assert bad == 0, (k, bad, err, tol)
    assert not bool(buf["x1"][:, 3:].any()), "x1: columns 3..7 are exact zeros"
    # b, c. the pools and their arg-max rows
    for g, i, y, stn in POOLS:
        assert not bool(torch.isnan(buf[g]).any()), f"{g}: elements never written"
        idx = buf[i].long()
        assert _in_own_cloud(idx, B, N, M), f"{i}: a row outside its own cloud"
        best, row, second = R.pool_reference(ref[y], first, B, N, M)
        want = best.clamp_min(0) if stn else best
        got = buf[g].double().clamp_min(0) if stn else buf[g].double()
        tol = R.pool_bound(ref[y], want, mode)
        err = (got - want).abs()
        say(f"{mode} {(B, N, M)} {g}: worst error {float(err.max()):.2e} (bound {float(tol.max()):.2e})")
        seen[g] = (float(err.max()), float(tol.max()))
        assert bool((err <= tol).all()), (g, float(err.max()))
        carries = best > 0 if stn else torch.ones_like(best, dtype=torch.bool)    # the pooled ReLU passes no gradient
        tol = R.pool_bound(ref[y], best, mode)
        at = torch.gather(ref[y], 0, idx)                                         # the reference's value at the reported row
        short = (best - at - tol).clamp_min(0) * carries
        assert not bool(short.any()), (i, "the reported row is no maximum", float(short.max()))
        decided = carries & (best - second > 2 * tol)
        wrong = decided & (idx != row)
        assert not bool(wrong.any()), (i, int(wrong.sum()), "rows differ from the reference's where the margin decides")
        share = 1.0 - float(decided.sum()) / max(int(carries.sum()), 1)
        say(f"{mode} {(B, N, M)} {i}: {100 * share:.2f} % of the pairs inside the margin (cap {100 * R.SKIP_CAP[mode]:.0f} %)")
        seen[i] = (share, R.SKIP_CAP[mode])
        assert share <= R.SKIP_CAP[mode], (i, share)
    return ref, seen


def _same_bits(a, b, what, keys=None):
    for k in keys or a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("mode,shape,forms", CASES, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s, _ in CASES])
def test_saved_rows_pools_and_argmax_rows_against_fp64(mode, shape, forms, record_property):
    B, N, M = shape
    _assert_forms(mode, B, N, M, forms)
    pts, t3, t64 = _inputs(B, N, M)
    sd = _model(N, M)[1]
    buf = _run(pts, t3, t64, B, N, M, mode)
    ref, seen = check_outputs(buf, pts, t3, t64, sd, mode, B, N, M)
    for k, (a, b) in seen.items():
        record_property(f"{k}", f"{a:.3e} ({b:.3e})")
    if mode == "fp32":                                   # argmax_tile_store: the pooled value keeps the inference kernels' bits
        inf = _inference_pools(pts, t3, t64, B, N, M)
        for g, _, _, stn in POOLS:
            assert torch.equal(buf[g].clamp_min(0) if stn else buf[g], inf[g]), f"{g}: not the inference kernel's pool"
    if shape == (2, 192, 64):                            # the device's fp64 reference against the same on the CPU
        cpu = R.encoder_rows(pts.cpu(), t3.cpu(), t64.cpu(), {k: v.cpu() for k, v in sd.items()}, mode, B, N, M,
                             saved={k: v.cpu() for k, v in buf.items()})
        for k, v in cpu.items():
            assert float((ref[k].cpu() - v).abs().max()) <= 1e-12, k


def test_fp32_trunk_one_wave_per_simd_and_eight_wave_forms_give_the_same_bits():
    from catre_amd import hip

    B, N, M = 33, 128, 128
    pts, t3, t64 = _inputs(B, N, M)
    was = hip.form_switch("trunk4")
    try:
        hip.form_switch("trunk4", True)
        _assert_forms("fp32", B, N, M, WAVE4)
        wave4 = _run(pts, t3, t64, B, N, M, "fp32")
        hip.form_switch("trunk4", False)
        _assert_forms("fp32", B, N, M, RS1)
        rs1 = _run(pts, t3, t64, B, N, M, "fp32")
    finally:
        hip.form_switch("trunk4", was)
    _same_bits(wave4, rs1, "train_wave4 against train_rs1")


def test_fp32_stn_without_saved_rows_small_grid():
    """stn_rows=False below the pair threshold: train_rs1 without rows - the pools and arg-max rows of the rows-saved call"""
    B, N, M = 2, 192, 64
    pts, t3, t64 = _inputs(B, N, M)
    _assert_forms("fp32", B, N, M, RS1, stn_rows=False)
    bare = _run(pts, t3, t64, B, N, M, "fp32", stn_rows=False)
    assert all(bare[k] is None for k in ("a1", "a2", "f1", "f2"))
    _same_bits(bare, _run(pts, t3, t64, B, N, M, "fp32"), "rows not saved against rows saved", [k for k in bare if bare[k] is not None])


def test_fp32_stn_pair_form_without_saved_rows():
    """256 pairs with an odd tile count per cloud: the STNs without rows take train_pair; with `stn_pair` off train_rs1 -
    the same bits, and those of the rows-saved call (checked against fp64 above)."""
    from catre_amd import hip

    B, N, M = 64, 192, 192
    pts, t3, t64 = _inputs(B, N, M)
    keys = ("g_stn", "i_stn", "g_fstn", "i_fstn", "x1", "h1", "pf", "c2", "c3", "g", "i")
    was = hip.form_switch("stn_pair")
    try:
        hip.form_switch("stn_pair", True)
        _assert_forms("fp32", B, N, M, dict(WAVE4, stn3d="train_pair", stnkd="train_pair"), stn_rows=False)
        pair = _run(pts, t3, t64, B, N, M, "fp32", stn_rows=False)
        hip.form_switch("stn_pair", False)
        _assert_forms("fp32", B, N, M, WAVE4, stn_rows=False)
        rs1 = _run(pts, t3, t64, B, N, M, "fp32", stn_rows=False)
    finally:
        hip.form_switch("stn_pair", was)
    for i in ("i_stn", "i_fstn", "i"):
        assert _in_own_cloud(pair[i].long(), B, N, M), i
    _same_bits(pair, rs1, "train_pair against train_rs1", keys)
    _same_bits(pair, _run(pts, t3, t64, B, N, M, "fp32"), "rows not saved against rows saved", keys)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("craft", ["one_point", "first_tile", "mirrored_halves"])
def test_first_maximum_wins(craft, mode):
    """Exact ties, no margin: bit-identical input points give bit-identical rows, and the first of them must be reported -
    inside a half-wave, across the two half-waves of a tile (rows 32..63 mirror rows 0..31), across the tiles of a pair and
    across the per-tile partials."""
    B, N, M = 2, 192, 64
    pts, t3, t64 = _inputs(B, N, M)
    pts = {"one_point": R.repeat_one_point, "first_tile": R.repeat_first_tile, "mirrored_halves": R.mirror_half_tiles}[craft](pts, B, N, M)
    buf = _run(pts, t3, t64, B, N, M, mode)
    lo, _ = R.cloud_ranges(B, N, M, pts.device)
    first = R.first_identical_row(pts, B, N, M)
    for k, v in buf.items():
        assert not bool(torch.isnan(v).any() if v.is_floating_point() else (v < 0).any()), f"{k}: elements never written"
    one = None
    if craft == "first_tile":                            # the one-tile clouds: the first tile of every cloud, same transforms
        (po, _), (pp, _) = R.cloud_groups(pts, B, N, M)
        one = _run(torch.cat([po[:, :64].reshape(-1, 3), pp[:, :64].reshape(-1, 3)], 0).contiguous(), t3, t64, B, 64, 64, mode)
        lo1, _ = R.cloud_ranges(B, 64, 64, pts.device)
    for g, i, _, _ in POOLS:
        idx = buf[i].long()
        assert _in_own_cloud(idx, B, N, M), i
        if craft == "one_point":
            assert torch.equal(idx, lo[:, None].expand_as(idx)), f"{i}: not the cloud's first row"
        elif craft == "first_tile":
            assert bool((idx - lo[:, None] < 64).all()), f"{i}: a row past the first tile"
            assert torch.equal(buf[g], one[g]), f"{g}: not the one-tile cloud's pool"
            assert torch.equal(idx - lo[:, None], one[i].long() - lo1[:, None]), f"{i}: not the one-tile cloud's row"
        assert torch.equal(first[idx], idx), f"{i}: a row with an earlier bit-identical input row"


@pytest.mark.parametrize("mode,shape,clouds,big,small", [
    ("bf16", (128, 192, 192), (0, 63, 127), dict.fromkeys(STAGES, "train_bf_pair"),
     dict(stn3d="train_bf", stnkd="train_bf", trunk="train_bf_pair")),
    ("fp32", (33, 128, 128), (0, 16, 32), WAVE4, RS1)], ids=["bf16", "fp32"])
def test_clouds_do_not_depend_on_their_batch(mode, shape, clouds, big, small):
    """Clouds of a large grid run alone as a B = 3 batch - another kernel form - give the same pools, saved rows and
    cloud-relative arg-max rows, bit for bit."""
    B, N, M = shape
    pts, t3, t64 = _inputs(B, N, M)
    _assert_forms(mode, B, N, M, big)
    _assert_forms(mode, 3, N, M, small)
    whole = _run(pts, t3, t64, B, N, M, mode)
    sel = torch.tensor(clouds, device=pts.device)
    both = torch.cat([sel, B + sel])
    (po, _), (pp, _) = R.cloud_groups(pts, B, N, M)
    alone = _run(torch.cat([po[sel].reshape(-1, 3), pp[sel].reshape(-1, 3)], 0).contiguous(), t3[both].contiguous(),
                 t64[both].contiguous(), 3, N, M, mode)
    lo, _ = R.cloud_ranges(B, N, M, pts.device)
    lo3, _ = R.cloud_ranges(3, N, M, pts.device)
    for k in ROWS:
        (wo, _), (wp, _) = R.cloud_groups(whole[k], B, N, M)
        want = torch.cat([wo[sel].reshape(-1, wo.shape[-1]), wp[sel].reshape(-1, wp.shape[-1])], 0)
        assert not bool(torch.isnan(want).any()) and torch.equal(alone[k], want), f"{k}: depends on the batch"
    for g, i, _, _ in POOLS:
        assert torch.equal(alone[g], whole[g][both]), f"{g}: depends on the batch"
        assert _in_own_cloud(whole[i].long(), B, N, M) and _in_own_cloud(alone[i].long(), 3, N, M), i
        assert torch.equal(alone[i].long() - lo3[:, None], whole[i][both].long() - lo[both][:, None]), f"{i}: depends on the batch"
