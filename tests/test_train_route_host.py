"""Host-side check of the training forward's route decision (catre_amd/train_route.py: train_route), in the style of
tests/test_form_decision_host.py.

The reference is `_mirror`: the predicates and ladders `forward_train` and its helpers carried BEFORE the decision became
one function (the fused_rot / lp_cm / enc_fp32 locals, the three-way encoder `if`, the five-way heads `if`, `_rot_head`'s
ladder, the knob reads of `_rot_heads_split` and `pointnet_rows_fused`, and the `*_ok` predicates of train_ops they called),
written out as plain `if`s over the same plain arguments.  `train_route == _mirror` over the full product of: 3 modes x 256
knob states x runtime {none, plain, layered} x rotation / ts head form x feature transform x D {64, 1024} x B {1, 16} x
encoder frozen x input grad x (N + M matches the runtime) x layers.3.bias x 7 (N, M) pairs on the predicates' edges.

Pruned - combinations no caller can produce:
  * no runtime with "N + M matches the runtime's" true (there is nothing to match): 1/6 of the product;
  * a frozen encoder with a differentiable 3-d input (frozen means nothing in front of the heads needs a gradient): 1/4.
Together 3/8 of the product is pruned (asserted below), under the one half allowed."""
import inspect
import itertools

import pytest
import torch

from catre_amd import train_forward as TF
from catre_amd import train_ops as T
from catre_amd import train_route as TR

NM = [(64, 64), (128, 64), (96, 64), (64, 96), (4096, 64), (4160, 64), (64, 0)]
KNOBS = [T.TrainKernels(*bits) for bits in itertools.product((False, True), repeat=len(T.TrainKernels._fields))]


def shapes(D, l3_bias=True, ft=True):
    """The shipped layer shapes at out_dim D."""
    rot = TR.RotShape(256, D + 64, 256, 256, l3_bias)
    return TR.Shapes(64, TR.Stack(64, 3, 128, 1024), TR.Stack(64, 64, 128, 1024) if ft else None, TR.Stack(128, 64, 512, D), (rot, rot))


# ---------------------------------------------------------------------------------------------- the parent's predicates
def _tiled(R, J, K, min_rows=2048):
    return (J % 32 == 0) and (J <= 256 or J in (512, 1024)) and (K in (8, 16, 32, 64, 128) or K % 256 == 0) and R >= min_rows


def _chain(x_grad, s, N, M):                                         # train_ops.pooled_chain_ok
    if N % 64 or M % 64 or max(N, M) > 4096:
        return False
    if x_grad and not _tiled(1, s.k1, s.j1, min_rows=0):
        return False
    return s.j1 in (64, 128) and s.j2 in (128, 512) and s.j3 <= 1024 and s.j3 % 32 == 0 and (s.k1 <= 8 or s.k1 in (64, 128))


def _mirror_head(mode, k, pfw, r, B, N, M):                          # train_forward._rot_head
    P = N + M
    if (k.fused_lp_rot and k.lp_rot_bf16_rows and mode == 1 and pfw == 64 and r.f0 == 256 and r.f3 == 256 and r.k3 == 256
            and r.l3_bias and N % 64 == 0 and M % 64 == 0 and N > 0 and M > 0):                       # rot_head_lp_ok
        return ("lp_node", "")
    if ((mode == 0 or (mode == 1 and k.fused_lp_rot)) and r.f0 == 256 and pfw == 64
            and N % 64 == 0 and M % 64 == 0 and N > 0):                                               # rot_l0_block_ok
        first = "l0_block"
    else:
        first = "layered"
    aw = r.f0
    if mode == 0 and aw == 256 and r.f3 == 256 and r.k3 == 256 and N % 64 == 0 and M % 64 == 0 and N > 0 and r.l3_bias:
        return (first, "l1_block")                                                                   # rot_l1_block_ok
    if (k.fused_lp_rot and mode == 1 and aw == 256 and r.f3 == 256 and r.k3 == 256 and r.l3_bias
            and N % 64 == 0 and M % 64 == 0 and N > 0 and M > 0):                                     # rot_l1_tail_lp_ok
        return (first, "l1_tail_lp")
    # linear_gn_partials gives partials from _RotLinear at J == 256 and _rot_linear_ok
    part = r.f3 == 256 and (N % 64 == 0 and M % 64 == 0 and _tiled(B * P, r.f3, r.k3, min_rows=64) and r.k3 % 8 == 0)
    if part and P % 64 == 0:
        return (first, "neck_tail")
    return (first, "layered")


def _mirror(mode, k, has_rt, layered, rot_shipped, ts_shipped, D, ft, B, N, M, nm_match, enc_frozen, pts_grad, sh):
    """forward_train before train_route, on plain arguments -> the same TrainRoute."""
    rot_packed = rot_shipped and not layered
    shapes_ok = (sh.conv1 == 64 and N % 64 == 0 and M % 64 == 0 and N > 0 and M > 0
                 and all(r.l3_bias and (r.f0, r.k0) == (256, D + 64) and (r.f3, r.k3) == (256, 256) for r in sh.rot))
    fused_rot = rot_packed and has_rt and mode == 0 and ft and nm_match and shapes_ok
    lp_cm = (rot_shipped and D == 1024 and has_rt and mode == 1 and k.fused_lp_rot and k.lp_rot_bf16_rows and ft and nm_match
             and shapes_ok)
    enc_fp32 = D != 1024
    stacks = ("", "", "", "")
    if has_rt and enc_frozen and (mode == 0 or enc_fp32) and nm_match:
        kind, enc_mode, hub = "frozen", 0, True
    elif has_rt and D == 1024 and mode in (0, 1, 2) and ft and N % 64 == 0 and M % 64 == 0 and nm_match:
        fused_lp_ok = _chain(pts_grad, sh.stn, N, M) and _chain(False, sh.fstn, N, M) and _chain(False, sh.trunk, N, M)
        if mode == 1 and not fused_lp_ok:
            kind, enc_mode, hub = "layered", mode, False
        else:
            kind, enc_mode = "fused", mode
            hub = _chain(False, sh.trunk, N, M)
            stacks = ("chain" if _chain(pts_grad, sh.stn, N, M) else "layered",
                      "chain" if _chain(False, sh.fstn, N, M) else "layered", "hub" if hub else "layered",
                      "saved" if not (mode == 0 and k.stn_recompute and not pts_grad) else "recomputed")
        fused_rot = fused_rot and hub
        lp_cm = lp_cm and hub
    else:
        kind, enc_mode, hub = "layered", (0 if enc_fp32 else mode), False
        fused_rot = lp_cm = False
    enc = TR.EncRoute(kind, enc_mode, *stacks)
    ts = "shipped" if ts_shipped else "form"
    if not rot_shipped:
        return TR.TrainRoute(enc, False, "form", None, None, ts)
    if fused_rot:
        return TR.TrainRoute(enc, True, "fused_f32", None, None, ts)
    if rot_packed and hub and mode == 2 and shapes_ok:
        return TR.TrainRoute(enc, False, "split", (k.split_l0_one_pass, k.split_l1_one_pass), None, ts)
    if lp_cm:
        return TR.TrainRoute(enc, True, "lp_pair", None, None, ts)
    return TR.TrainRoute(enc, False, "per_head", None, tuple(TR.PerHead(*_mirror_head(mode, k, sh.conv1, r, B, N, M)) for r in sh.rot),
                         ts)


def _cases(mode, rt, Ds=(64, 1024)):
    """(every argument behind the knobs) for one mode and runtime kind, and how many the pruning removed."""
    has_rt, layered = rt != "none", rt == "layered"
    kept, pruned = [], 0
    for rot, ts, ft, D, B, frozen, grad, nm, l3b, (N, M) in itertools.product(
            (True, False), (True, False), (True, False), Ds, (1, 16), (False, True), (False, True), (False, True),
            (True, False), NM):
        if (nm and not has_rt) or (frozen and grad):
            pruned += 1
            continue
        kept.append((has_rt, layered, rot, ts, D, ft, B, N, M, nm, frozen, grad, shapes(D, l3b, ft)))
    return kept, pruned


@pytest.mark.parametrize("D", [64, 1024])
@pytest.mark.parametrize("rt", ["none", "plain", "layered"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_train_route_is_the_parents_ladder(mode, rt, D):
    kept, _ = _cases(mode, rt, (D,))
    seen = set()
    for args in kept:
        for k in KNOBS:
            got = TR.train_route(mode, k, *args)
            if got != _mirror(mode, k, *args):
                raise AssertionError((mode, k, args, got, _mirror(mode, k, *args)))
            seen.add((got.enc.kind, got.heads))
    assert len(seen) >= (2 if rt == "none" else 4), seen            # the sweep does reach the different routes


def test_the_pruned_share():
    kept = pruned = 0
    for rt in ("none", "plain", "layered"):
        kc, p = _cases(0, rt)
        kept, pruned = kept + len(kc), pruned + p
    assert (kept + pruned) * 3 * len(KNOBS) == 3 * 256 * 3 * 2 ** 9 * 7
    assert pruned * 8 == (kept + pruned) * 3                          # 3/8, under one half


def test_the_default_routes():
    """What the shipped model takes at N = M = 1024 in the three modes (DESIGN: the routes the benchmarks measure)."""
    k, sh = T.TrainKernels(), shapes(1024)
    r = lambda mode, **kw: TR.train_route(mode, k, **dict(dict(
        has_rt=True, layered=False, rot_shipped=True, ts_shipped=True, D=1024, feature_transform=True, B=16, N=1024, M=1024,
        nm_match=True, enc_frozen=False, pts_grad=False, sh=sh), **kw))
    assert r(0) == TR.TrainRoute(TR.EncRoute("fused", 0, "chain", "chain", "hub", "recomputed" if k.stn_recompute else "saved"),
                                 True, "fused_f32", None, None, "shipped")
    want1 = "lp_pair" if k.fused_lp_rot and k.lp_rot_bf16_rows else "per_head"
    assert r(1).enc == TR.EncRoute("fused", 1, "chain", "chain", "hub", "saved") and r(1).heads == want1
    assert r(2).heads == "split" and r(2).split == (k.split_l0_one_pass, k.split_l1_one_pass) and not r(2).x_cm
    assert r(1, pts_grad=True).enc == TR.EncRoute("layered", 1, "", "", "", "")
    assert r(0, enc_frozen=True).enc.kind == "frozen" and r(0, enc_frozen=True).heads == "fused_f32"
    assert r(0, has_rt=False, nm_match=False).per_head == (TR.PerHead("l0_block", "l1_block"),) * 2


# ------------------------------------------------------------------------------------------------- the public wrappers
def _conv(j, k):
    return torch.zeros(j, k, 1)


@pytest.mark.parametrize("overrides", [{}, dict(fused_lp_rot=False), dict(lp_rot_bf16_rows=False)])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "split"])
def test_public_ok_wrappers_agree_with_the_pure_predicates(mode, overrides):
    """Each `*_ok` name the tests and callers use returns what the one pure predicate returns for the shapes of its tensors,
    the ambient compute mode and knobs."""
    m = {"fp32": 0, "bf16": 1, "split": 2}[mode]
    with T.amp_mode(mode), T.train_kernels(overrides):
        k = T.knobs()
        assert T._amp() == m and all(getattr(k, n) == v for n, v in overrides.items())
        for (N, M), D, bias, grad in itertools.product(NM, (64, 1024), (True, False), (False, True)):
            sh = shapes(D, bias)
            p = {}
            for pre, s in (("pcl_net.stn", sh.stn), ("pcl_net.fstn", sh.fstn)):
                p[f"{pre}.conv1.weight"], p[f"{pre}.conv2.weight"] = _conv(s.j1, s.k1), _conv(s.j2, s.j1)
                p[f"{pre}.conv3.weight"] = _conv(s.j3, s.j2)
            p["pcl_net.conv1.weight"] = _conv(64, 3)
            p["pcl_net.conv2.weight"], p["pcl_net.conv3.weight"] = _conv(128, 64), _conv(512, 128)
            p["pcl_net.conv4.weight"] = _conv(D, 512)
            for pre in TF._ROT_PREFIX:
                p[f"{pre}.layers.0.weight"], p[f"{pre}.layers.3.weight"] = _conv(256, D + 64), _conv(256, 256)
                if bias:
                    p[f"{pre}.layers.3.bias"] = torch.zeros(256)
            assert TF.route_shapes(p) == sh
            pts = torch.zeros(4, 3, requires_grad=grad)
            pf, a = torch.zeros(4, 64), torch.zeros(4, 256)
            w0, w3, b3 = torch.zeros(256, 64), p[f"{pre}.layers.3.weight"], p.get(f"{pre}.layers.3.bias")
            assert T.pooled_chain_ok(pts, *(p[f"pcl_net.stn.conv{i}.weight"] for i in (1, 2, 3)), N, M) \
                == TR.pooled_chain_ok(grad, sh.stn, N, M)
            assert T.pooled_chain_ok(pf, *(p[f"pcl_net.conv{i}.weight"] for i in (2, 3, 4)), N, M) \
                == TR.pooled_chain_ok(False, sh.trunk, N, M)
            assert TF.fused_lp_ok(pts, p, N, M) == TR.fused_lp_ok(grad, sh, N, M)
            assert T.rot_head_lp_ok(pf, w0, w3, b3, N, M) == TR.rot_head_lp_ok(m, k, 64, 256, 64, 256, 256, bias, N, M)
            assert T.rot_l1_tail_lp_ok(a, w3, b3, N, M) == TR.rot_l1_tail_lp_ok(m, k, 256, 256, 256, bias, N, M)
            assert T.rot_l0_block_ok(pf, w0, N, M) == TR.rot_l0_block_ok(m, k, 64, 256, 64, N, M)
            assert T.rot_l1_block_ok(a, w3, N, M) == TR.rot_l1_block_ok(m, 256, 256, 256, N, M)
            assert T.rot_heads_ok(pf, N, M) == TR.rot_heads_ok(m, 64, N, M)
            assert T._rot_linear_ok(16 * (N + M), 256, 256, N, M) == TR.rot_linear_ok(16 * (N + M), 256, 256, N, M)
            assert TF._rot_heads_shapes_ok(p, pf, N, M) == TR.rot_heads_shapes_ok(sh, D, N, M)
            assert TF._rot_heads_fused_ok(p, pf, N, M) == (TR.rot_heads_ok(m, 64, N, M) and TR.rot_heads_shapes_ok(sh, D, N, M))
            # and a predicate that is true somewhere, so the agreement is not all-False
    with T.amp_mode("bf16"):
        assert T.rot_head_lp_ok(torch.zeros(4, 64), torch.zeros(256, 64), _conv(256, 256), torch.zeros(256), 64, 64) \
            == (T.knobs().fused_lp_rot and T.knobs().lp_rot_bf16_rows)
    with T.amp_mode("fp32"):
        assert T.rot_l1_block_ok(torch.zeros(4, 256), _conv(256, 256), 64, 64) and T.rot_heads_ok(torch.zeros(4, 64), 64, 64)


def test_train_route_imports_neither_torch_nor_hip():
    src = inspect.getsource(TR)
    assert [ln for ln in src.splitlines() if ln.startswith(("import ", "from "))] == ["import typing"]


def test_train_forward_reads_mode_and_knobs_in_one_place():
    """Source scan: `T._amp` / `T.knobs` appear once each in train_forward.py, inside `_ambient` (the predicates' wrappers in
    train_ops read them for their stand-alone callers; forward_train passes its one reading down through the route)."""
    src = inspect.getsource(TF)
    assert src.count("T._amp(") == 1 and src.count("T.knobs(") == 1 and "_TLS" not in src
    assert "T._amp(), T.knobs()" in inspect.getsource(TF._ambient)
    assert inspect.getsource(TF.forward_train).count("_ambient()") == 1


def test_ambient_is_read_once_per_route(monkeypatch):
    """Counting the calls: the stand-alone helpers that need the mode or the knobs read them once."""
    calls = []
    amp, knobs = T._amp, T.knobs
    monkeypatch.setattr(T, "_amp", lambda: calls.append("amp") or amp())
    monkeypatch.setattr(T, "knobs", lambda: calls.append("knobs") or knobs())
    assert TF._ambient() == (0, T._DEFAULT_KNOBS) and calls == ["amp", "knobs"]


# ------------------------------------------------------------------------------------------------------------ RotHeadW
@pytest.mark.parametrize("conv_p_bias", [True, False])
@pytest.mark.parametrize("rot_dim", [3, 2])
def test_rot_head_weights_order_and_shapes(monkeypatch, rot_dim, conv_p_bias):
    B, D, P, pre = 2, 1024, 128, TF._ROT_PREFIX[0]
    p = {f"{pre}.layers.0.weight": torch.randn(256, D + 64, 1), f"{pre}.layers.0.bias": torch.randn(256),
         f"{pre}.layers.1.weight": torch.randn(256), f"{pre}.layers.1.bias": torch.randn(256),
         f"{pre}.layers.3.weight": torch.randn(256, 256, 1), f"{pre}.layers.3.bias": torch.randn(256),
         f"{pre}.layers.4.weight": torch.randn(256), f"{pre}.layers.4.bias": torch.randn(256),
         f"{pre}.neck.0.weight": torch.randn(rot_dim, 256, 1), f"{pre}.neck.0.bias": torch.randn(rot_dim),
         f"{pre}.conv_p.weight": torch.randn(1, P, 1)}
    if conv_p_bias:
        p[f"{pre}.conv_p.bias"] = torch.randn(1)
    # (the two ops the builder calls are HIP ops: their plain-torch meaning stands in on the host)
    monkeypatch.setattr(T, "split_cols", lambda w, k0: (w[:, :k0], w[:, k0:]))
    monkeypatch.setattr(T, "linear", lambda x, w, b=None: torch.nn.functional.linear(x, w, b))
    g = torch.randn(2 * B, D)
    hw = TF.rot_head_weights(p, pre, g)
    assert hw._fields == ("w0", "bias0", "g0", "be0", "w1", "b1", "g1", "be1", "wn", "bn", "wp", "bp")
    want = [(256, 64), (2 * B, 256), (256,), (256,), (256, 256, 1), (256,), (256,), (256,), (3, 256), (3,), (1, P, 1)]
    assert [tuple(t.shape) for t in hw[:11]] == want
    assert (hw.bp is None) == (not conv_p_bias) and (conv_p_bias is False or tuple(hw.bp.shape) == (1,))
    w0 = p[f"{pre}.layers.0.weight"].reshape(256, -1)
    assert torch.equal(hw.w0, w0[:, D:]) and torch.allclose(hw.bias0, g @ w0[:, :D].T + p[f"{pre}.layers.0.bias"], atol=1e-4)
    assert torch.equal(hw.wn[:rot_dim], p[f"{pre}.neck.0.weight"].reshape(rot_dim, 256)) and not hw.wn[rot_dim:].any()
    assert hw.g0 is p[f"{pre}.layers.1.weight"] and hw.be1 is p[f"{pre}.layers.4.bias"] and hw.b1 is p[f"{pre}.layers.3.bias"]
    assert TF.rot_dim(p, pre) == rot_dim
    raw = TF.rot_head_weights(p, pre, g, neck3=False)
    assert raw.wn is p[f"{pre}.neck.0.weight"] and raw.bn is p[f"{pre}.neck.0.bias"]
