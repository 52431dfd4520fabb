"""Autograd-connected forward of one refine iteration for TRAINING (``do_loss=True`` path of the reference's
``CATRE_disR_shared.forward``, ``core/catre/models/CATRE_disR_shared.py:57-124``).

Same arithmetic as the fused inference kernels, but laid out layer by layer on point-major activation
matrices so that ``torch.autograd`` can chain the hand-written HIP backward kernels of
``catre_amd/train_ops.py``.  The restructurings of the inference path are kept (the repeated global
feature becomes a per-cloud bias of rot-head layer 0; the ``[B,1088,N]`` tensors are never built), so the
gradients equal the reference's up to fp32 re-association.
"""
import typing

import torch

from . import hip
from . import train_ops as T
from . import train_route as TR


def _ambient():
    """(compute mode, knobs) of the forward in progress: thread-local state, read HERE and nowhere else in this module -
    ``forward_train`` once per forward, the stand-alone helpers when no route is handed to them."""
    return T._amp(), T.knobs()


def _stack(p, prefix, names):
    a, b, c = (p[f"{prefix}.{n}.weight"] for n in names)
    return TR.Stack(*T._jk(a), b.shape[0], c.shape[0])


_NO_ROT = TR.RotShape(0, 0, 0, 0, False)


def _rot_shape(p, prefix):
    w0, w3 = p.get(f"{prefix}.layers.0.weight"), p.get(f"{prefix}.layers.3.weight")
    if w0 is None or w3 is None:    # (a head of another depth: never asked about the shipped form's routes)
        return _NO_ROT
    return TR.RotShape(*T._jk(w0), *T._jk(w3), p.get(f"{prefix}.layers.3.bias") is not None)


def route_shapes(p, prefix="pcl_net"):
    """The layer shapes ``train_route`` reads, off the parameters."""
    convs = ("conv1", "conv2", "conv3")
    return TR.Shapes(p[f"{prefix}.conv1.weight"].shape[0], _stack(p, f"{prefix}.stn", convs),
                     _stack(p, f"{prefix}.fstn", convs) if f"{prefix}.fstn.conv1.weight" in p else None,
                     _stack(p, prefix, ("conv2", "conv3", "conv4")), tuple(_rot_shape(p, pre) for pre in _ROT_PREFIX))


def _points_rows(x):
    """[B,3,n] (any strides) -> [B*n, 3] contiguous rows (pure data movement)."""
    return x.permute(0, 2, 1).reshape(-1, 3).contiguous()


def _cloud_major_rows(x, tfd_kps):
    """x [B,3,N], tfd_kps [B,3,M] -> [B*N + B*M, 3] cloud-major point rows.  ``runtime.pose_apply`` (``batch_updater_test``)
    writes the two clouds back to back into one buffer: then the matrix is a view of it; anything else is concatenated."""
    xr, kr = _points_rows(x), _points_rows(tfd_kps)
    if (not xr.requires_grad and not kr.requires_grad and xr.dtype == kr.dtype == torch.float32 and xr.device == kr.device
            and xr.untyped_storage().data_ptr() == kr.untyped_storage().data_ptr()
            and kr.data_ptr() == xr.data_ptr() + xr.numel() * 4):
        return torch.as_strided(xr, (xr.shape[0] + kr.shape[0], 3), (3, 1))
    return torch.cat([xr, kr], 0)


def _stn(rows, p, prefix, k, B, N, M, pre=None, chain=False):
    """STN3d / STNkd on cloud-major rows [R, k] -> [C, k, k]  (pointnet.py:24-41 / 57-78).  ``pre``: (conv1 out, conv2
    out, pooled maxima, arg-max rows) already computed by the fused forward kernel - the nodes then only build the graph;
    ``chain``: the route's word on this stack (EncRoute.stn / .fstn == "chain")."""
    w = lambda n: p[f"{prefix}.{n}"]
    p1, p2, pg = (pre[0], pre[1], (pre[2], pre[3])) if pre is not None else (None, None, None)
    if chain:
        # the conv stack + pool as one node with a row-sparse backward (train_ops._PooledChain)
        g = T.pooled_chain(rows, w("conv1.weight"), w("conv1.bias"), w("conv2.weight"), w("conv2.bias"),
                           w("conv3.weight"), w("conv3.bias"), True, B, N, M, pre)
    else:
        h = T.linear(rows, w("conv1.weight"), w("conv1.bias"), relu=True, pre=p1)
        h = T.linear(h, w("conv2.weight"), w("conv2.bias"), relu=True, pre=p2)
        g = T.linear_maxpool(h, w("conv3.weight"), w("conv3.bias"), True, B, N, M, pre=pg)  # relu(conv3) then max
    h = T.linear(g, w("fc1.weight"), w("fc1.bias"), relu=True)
    h = T.linear(h, w("fc2.weight"), w("fc2.bias"), relu=True)
    t = T.linear(h, w("fc3.weight"), w("fc3.bias"), identity_k=k)
    return t.view(-1, k, k)


def pointnet_rows_fused(pts, desc, rt, p, B, N, M, prefix="pcl_net", mode=0, obj_copy=True, route=None):
    """The same graph as :func:`pointnet_rows` (feature_transform=True), but the three conv stacks run as the FUSED encoder
    kernels with extra stores (``catre_train_{stn3d,stnkd,trunk}_fwd``): one launch per block instead of a row GEMM per
    layer.  Every layer op becomes a graph node around an output that exists already (``pre=``); the backward is the
    layer-wise one, unchanged.  N, M multiples of 64.  mode 0: the fp32 kernels; mode 2: the split kernels (rows hold hi + lo);
    mode 1 (autocast): the bf16-operand kernels -
    the rows they save behind each stack's first layer are bf16 ROWS (half the bytes; the values the reduced-precision dgrad /
    wgrad kernels would round their operands to anyway), read in place by the row-sparse chains' backward - so mode 1
    wants all three stacks to be chains (`fused_lp_ok`).  ``route``: the EncRoute ``forward_train`` decided on; a stand-alone
    caller gets the same function's answer for its arguments."""
    w = lambda n: p[f"{prefix}.{n}"]
    dev = pts.device
    if route is None:
        route = TR.encoder_route(mode, _ambient()[1], True, w("conv4.weight").shape[0], True, N, M, True, False,
                                 pts.requires_grad, route_shapes(p, prefix))
        if route.kind != "fused":
            raise hip.CatreHipError(f"pointnet_rows_fused: no fused encoder forward for N={N}, M={M}, mode {mode}")
    buf = rt.train_encoder_buffers(B, N, M, dev, stn_rows=route.stn_rows == "saved", mode=mode)
    packs = rt.train_stn3d(desc, buf, B, N, M, dev, mode)   # (params, packed image): re-packed here, shared by the three kernels
    trans = _stn(pts, p, f"{prefix}.stn", 3, B, N, M, pre=(buf["a1"], buf["a2"], buf["g_stn"], buf["i_stn"]),
                 chain=route.stn == "chain")
    trans3 = trans.detach().reshape(-1, 9).contiguous()
    # x1 / h1 are written by the trunk kernel further down (same stream, before anything reads them)
    x1 = T.cloud_matmul(pts, trans, B, N, M, out_cols=8, pre=buf["x1"])
    h1, h1s = T.linear_fan2(x1, w("conv1.weight"), w("conv1.bias"), relu=True, pre=buf["h1"])  # two consumers, one backward pass
    rt.train_stnkd(desc, trans3, buf, B, N, M, dev, mode, packs=packs)
    trans_feat = _stn(h1s, p, f"{prefix}.fstn", 64, B, N, M, pre=(buf["f1"], buf["f2"], buf["g_fstn"], buf["i_fstn"]),
                      chain=route.fstn == "chain")
    trans64 = trans_feat.detach().reshape(-1, 4096).contiguous()
    rt.train_trunk(desc, trans3, trans64, buf, B, N, M, dev, mode, packs=packs)
    pf = T.cloud_matmul(h1, trans_feat, B, N, M, pre=buf["pf"])
    if route.trunk == "hub":
        # the conv stack with its row-sparse backward AND pointfeat's two other consumers (max over points, the rotation
        # heads' object-major copy) as one node: their three gradients meet in one pass (train_ops._PointfeatHub)
        g, pfmax, pf_obj = T.pointfeat_hub(pf, w("conv2.weight"), w("conv2.bias"), w("conv3.weight"), w("conv3.bias"),
                                           w("conv4.weight"), w("conv4.bias"), B, N, M,
                                           (buf["c2"], buf["c3"], buf["g"], buf["i"]), obj_copy=obj_copy)
        return g, pf, (pfmax, pf_obj)
    h = T.linear(pf, w("conv2.weight"), w("conv2.bias"), relu=True, pre=buf["c2"])
    h = T.linear(h, w("conv3.weight"), w("conv3.bias"), relu=True, pre=buf["c3"])
    g = T.linear_maxpool(h, w("conv4.weight"), w("conv4.bias"), False, B, N, M, pre=(buf["g"], buf["i"]))
    return g, pf, None


def fused_lp_ok(pts, p, N, M, prefix="pcl_net"):
    return TR.fused_lp_ok(pts.requires_grad, route_shapes(p, prefix), N, M)


def pointnet_rows(pts, p, B, N, M, feature_transform=True, prefix="pcl_net"):
    """PointNetfeat on cloud-major point rows [B*N + B*M, 3] -> (g [C,out_dim], pointfeat [R,64])  (pointnet.py:97-116)."""
    w = lambda n: p[f"{prefix}.{n}"]
    trans = _stn(pts, p, f"{prefix}.stn", 3, B, N, M)
    x1 = T.cloud_matmul(pts, trans, B, N, M, out_cols=8)                    # x^T @ trans, zero-padded to 8 columns
    if feature_transform:
        h1, h1s = T.linear_fan2(x1, w("conv1.weight"), w("conv1.bias"), relu=True)   # [R,64], two consumers
        trans_feat = _stn(h1s, p, f"{prefix}.fstn", 64, B, N, M)
        pf = T.cloud_matmul(h1, trans_feat, B, N, M)
    else:
        pf = T.linear(x1, w("conv1.weight"), w("conv1.bias"), relu=True)
    h = T.linear(pf, w("conv2.weight"), w("conv2.bias"), relu=True)
    h = T.linear(h, w("conv3.weight"), w("conv3.bias"), relu=True)
    g = T.linear_maxpool(h, w("conv4.weight"), w("conv4.bias"), False, B, N, M)   # conv4 has no ReLU (:114)
    return g, pf


def _split_w0(W0):
    """Rot-head layer 0's weight [F, D + 64(, 1)] -> (global half [F, D] (a view), point half [F, 64]): D, the encoder's
    out_dim, is read from the weight."""
    F, K = W0.shape[:2]
    return T.split_cols(W0.reshape(F, K), K - 64)


class RotHeadW(typing.NamedTuple):
    """One shipped-form rotation head's tensors, in the ONE order every op that takes a head takes them in
    (train_ops.rot_head_lp / rot_head_pair_lp / rot_heads; ``[4:]`` is what rot_l1_tail_lp takes behind its input)."""
    w0: torch.Tensor        # [256,64]: the point half of layers.0
    bias0: torch.Tensor     # [2B,256]: its global half applied to the pooled feature, + the conv bias - a bias per cloud
    g0: torch.Tensor        # GroupNorm 0 (layers.1) weight, bias
    be0: torch.Tensor
    w1: torch.Tensor        # layers.3 [256,256(,1)], bias
    b1: typing.Optional[torch.Tensor]
    g1: torch.Tensor        # GroupNorm 1 (layers.4) weight, bias
    be1: torch.Tensor
    wn: torch.Tensor        # neck [3,256], [3] or None (zero-padded from rot_dim rows: heads.neck_weight3)
    bn: typing.Optional[torch.Tensor]
    wp: torch.Tensor        # conv_p [1,P,1], bias or None
    bp: typing.Optional[torch.Tensor]


def rot_head_weights(p, prefix, g, neck3=True):
    """The :class:`RotHeadW` of head ``prefix`` for the pooled feature ``g`` [2B,out_dim].  neck3=False: the neck as the
    module holds it ([rot_dim,256(,1)], for heads.neck_rows)."""
    from .heads import neck_weight3

    w = lambda n: p[f"{prefix}.{n}"]
    W0g, W0l = _split_w0(w("layers.0.weight"))                                # global half (a view) | point half
    wn, bn = w("neck.0.weight"), w("neck.0.bias")
    if neck3:
        wn, bn = neck_weight3(wn, bn)
    return RotHeadW(W0l, T.linear(g, W0g, w("layers.0.bias")), w("layers.1.weight"), w("layers.1.bias"), w("layers.3.weight"),
                    p.get(f"{prefix}.layers.3.bias"), w("layers.4.weight"), w("layers.4.bias"), wn, bn, w("conv_p.weight"),
                    p.get(f"{prefix}.conv_p.bias"))


def rot_dim(p, prefix):
    return p[f"{prefix}.neck.0.weight"].shape[0]


def _first_cols(o, rd):
    """o[:, :rd] - the tensor itself when that is all of it (rot6d: rd = 3 of 3 columns; a slice node would cost a copy in
    the backward)."""
    return o if o.shape[1] == rd else o[:, :rd]


def _rot_head(g, pf_obj, p, prefix, B, N, M, route=None):
    """RotHead.forward (heads/conv_out_per_rot_head.py:126-140) on the never-materialised cat(pcl_feat,kps_feat), on the
    per-head ops ``route`` (a train_route.PerHead) names."""
    if route is None:
        route = TR.per_head_route(*_ambient(), pf_obj.shape[1], _rot_shape(p, prefix), B, N, M)
    P, rd = N + M, rot_dim(p, prefix)
    hw = rot_head_weights(p, prefix, g, neck3=route.second != "layered")
    if route.first == "lp_node":
        # autocast: the head as one node with bf16 [B*P,256] activations between its kernels
        return T.rot_head_lp(pf_obj, *hw, B, N, M)[:, :rd]
    # [B*P,256]; the per-cloud bias and the GroupNorm tile partials are epilogue work of the GEMMs
    if route.first == "l0_block":
        a = T.rot_l0_block(pf_obj, hw.w0, hw.bias0, hw.g0, hw.be0, B, N, M)
    else:
        y, part = T.linear_cloudbias(pf_obj, hw.w0, hw.bias0, B, N, M, with_gn_partials=True)
        a = T.gn_points_gelu(y, hw.g0, hw.be0, B, P, part)
    if route.second == "l1_tail_lp":
        # autocast: the whole second half of the head as one node whose backward is one pass on the bf16 matrix pipe
        return _first_cols(T.rot_l1_tail_lp(a, *hw[4:], B, N, M), rd)
    if route.second == "neck_tail":
        # GroupNorm + GELU + neck + conv_p as one node: the [B*P,256] activation in between is never stored and the backward
        # needs no reduction pass over y (train_ops._NeckTail)
        y, part = T.linear_gn_partials(a, hw.w1, hw.b1, B, N, M)
        return _first_cols(T.neck_tail(y, *hw[6:], B, P, part), rd)
    if route.second == "l1_block":
        y3 = T.rot_l1_block(a, *hw[4:10], B, N, M)
    else:
        from .heads import neck_rows

        y, part = T.linear_gn_partials(a, hw.w1, hw.b1, B, N, M)
        y3 = neck_rows(T.gn_points_gelu(y, hw.g1, hw.be1, B, P, part), hw.wn, hw.bn)   # [B*P,3] (columns >= rot_dim are zero)
    return _first_cols(T.weighted_point_sum(y3, hw.wp, hw.bp, B, P), rd)


def _rot_head_form(g, pf_obj, p, prefix, B, N, M, form, fused_tail=False):
    """RotHead.forward for a head of any configured form (``heads.HeadForm``: width, depth, GroupNorm on / off and groups,
    activation).  Layer 0 keeps the restructuring of the shipped route at any width: the global half ``W0[:, :D] g`` is a
    per-cloud bias, the point half runs on pointfeat - the ``[B,D+64,P]`` tensor is never built.  The matrix work is
    ``T.linear`` / ``T.linear_cloudbias`` (tiled MFMA kernel at widths 32..256 in steps of 32, 512 and 1024; the small
    GEMM - correct, slow - elsewhere), norm + activation the generic ops.  fused_tail (nothing needs a gradient): the last
    layer's norm + act, neck and conv_p are one op."""
    from .heads import neck_rows

    w = lambda n: p[f"{prefix}.{n}"]
    P, F, L = N + M, form.feat_dim, form.num_layers
    gn = lambda i: (w(f"layers.{3 * i + 1}.weight"), w(f"layers.{3 * i + 1}.bias")) if form.norm else (None, None)
    W0g, W0b = _split_w0(w("layers.0.weight"))                                # global half (a view) | point half
    bias0 = T.linear(g, W0g, w("layers.0.bias"))                              # [2B,F]: global half + conv bias
    y = T.linear_cloudbias(pf_obj, W0b, bias0, B, N, M)
    rd = w("neck.0.weight").shape[0]
    a = None
    for i in range(L):
        if i:
            y = T.linear(a, w(f"layers.{3 * i}.weight"), w(f"layers.{3 * i}.bias"))
        if fused_tail and i == L - 1:
            return T.gn_points_act_neck_wsum(y, *gn(i), w("neck.0.weight"), w("neck.0.bias"), w("conv_p.weight"),
                                             p.get(f"{prefix}.conv_p.bias"), B, P, form.groups, form.act, form.norm)
        a = T.gn_points_act(y, *gn(i), B, P, form.groups, form.act, form.norm)
    y3 = neck_rows(a, w("neck.0.weight"), w("neck.0.bias"))                  # [B*P,3] (columns >= rot_dim are zero)
    return _first_cols(T.weighted_point_sum(y3, w("conv_p.weight"), p.get(f"{prefix}.conv_p.bias"), B, P), rd)


def _ts_head(ts_feat, p, form):
    """FC_TransSizeHead.forward (fc_trans_size_head.py:61-70) on however many layers ``form`` describes -> (dt, ds)."""
    from .heads import SHIPPED_FORM

    h = ts_feat
    for i in range(form.num_layers):
        h = T.linear(h, p[f"ts_head.linears.{3 * i}.weight"], p[f"ts_head.linears.{3 * i}.bias"])
        if form == SHIPPED_FORM:
            h = T.gn_rows_gelu(h, p[f"ts_head.linears.{3 * i + 1}.weight"], p[f"ts_head.linears.{3 * i + 1}.bias"])
        else:
            h = T.gn_rows_act(h, p.get(f"ts_head.linears.{3 * i + 1}.weight"), p.get(f"ts_head.linears.{3 * i + 1}.bias"),
                              form.groups, form.act, form.norm)
    return (T.linear(h, p["ts_head.fc_t.weight"], p["ts_head.fc_t.bias"]),
            T.linear(h, p["ts_head.fc_s.weight"], p["ts_head.fc_s.bias"]))


def heads_rows(p, opts, forms, g, pfmax, pf_obj, init_pose, init_scale, B, N, M, fused_tail=False):
    """Both heads layer by layer from the encoder's outputs (g [2B,out_dim] pooled, pfmax [2B,64] max_n pointfeat, pf_obj
    [B*(N+M),64] object-major) -> (rot [B, 2 rot_dim], dt, ds): the route of heads that are not the shipped form - training,
    and with fused_tail the no-grad forward / refine."""
    rot_form, ts_form = forms
    feats = [g[:B], pfmax[:B]] + ([g[B:], pfmax[B:]] if opts.with_kps_feature else [])
    if opts.with_init_scale:
        feats.append(init_scale)
    if opts.with_init_trans:
        feats.append(init_pose[:, :3, 3])
    dt, ds = _ts_head(torch.cat(feats, 1), p, ts_form)
    rx, ry = (_rot_head_form(g, pf_obj, p, pre, B, N, M, rot_form, fused_tail) for pre in _ROT_PREFIX)
    return torch.cat([rx, ry], 1), dt, ds


_ROT_PREFIX = ("rot_head.rot_head_x", "rot_head.rot_head_y")


def _head_pair(g, p):
    """Both heads' :class:`RotHeadW`; g: the pooled feature, or one handle of it per head (train_ops.hub)."""
    g = g if isinstance(g, (tuple, list)) else (g, g)
    return [rot_head_weights(p, pre, g[h]) for h, pre in enumerate(_ROT_PREFIX)]


def _rot_dims(outs, p):
    return [_first_cols(o, rot_dim(p, pre)) for pre, o in zip(_ROT_PREFIX, outs)]


def _rot_heads_lp(g, pf, p, B, N, M, x_cm):
    """Both RotHeads under autocast as ONE node (train_ops._RotHeadPairLP): per head the kernels of `_RotHeadLP`, and the two
    data gradients pointfeat receives from them are summed by the second head's backward kernel instead of by autograd."""
    return _rot_dims(T.rot_head_pair_lp(pf, *_head_pair(g, p), B, N, M, x_cm), p)


def _rot_heads_shapes_ok(p, pf_obj, N, M):
    sh = route_shapes(p)
    return TR.rot_heads_shapes_ok(sh._replace(conv1=pf_obj.shape[1]), sh.trunk.j3, N, M)


def _rot_heads_fused_ok(p, pf_obj, N, M):
    return T.rot_heads_ok(pf_obj, N, M) and _rot_heads_shapes_ok(p, pf_obj, N, M)


def _rot_heads_split(g, pf, pf_obj, p, rt, B, N, M, one_pass=None):
    """Both RotHeads in split mode: ONE fused forward launch chain (`catre_train_rot_fwd`, k_rot_l1_split<true>) computes what
    the per-head ops would - y0, a0 = gelu(GN0(y0)), y1 and the GroupNorm partials - and the per-head ops become graph nodes
    around those buffers (`pre=`); their backward is unchanged (split dgrad / wgrad GEMMs, fp32 GroupNorm / GELU passes).
    one_pass: TrainRoute.split - (first block, second block + tail) as one node each (knobs split_l0 / l1_one_pass)."""
    if one_pass is None:
        k = _ambient()[1]
        one_pass = (k.split_l0_one_pass, k.split_l1_one_pass)
    P = N + M
    heads = _head_pair(g, p)
    prm, packed = rt._train_packs(pf.device, 2)
    buf = T.rot_heads_forward(pf.detach(), heads[0].bias0, heads[1].bias0, prm, packed, B, N, M, 2)
    out = []
    for h, hw in enumerate(heads):
        if one_pass[0]:
            # the first block as one node: its backward is the fp32 one-pass kernel (k_rot_l0_bwd: sums + one pass over
            # (da, y0)) instead of the GroupNorm apply pass, a per-cloud bias reduction and a split dgrad and wgrad
            a = T.rot_l0_block(pf_obj, hw.w0, hw.bias0, hw.g0, hw.be0, B, N, M,
                               pre=(buf["y0"][h], buf["a0"][h], buf["stat0"][h]))
        else:
            y, _ = T.linear_cloudbias(pf_obj, hw.w0, hw.bias0, B, N, M, with_gn_partials=True, pre=(buf["y0"][h], None))
            a = T.gn_points_gelu(y, hw.g0, hw.be0, B, P, None, pre=(buf["a0"][h], buf["stat0"][h]))
        if one_pass[1]:
            # the second block + tail as one node: backward = conv_p, then ONE pass with hi + lo operands (k_rot_l1_bwd_sp)
            out.append(T.rot_l1_tail_lp(a, *hw[4:], B, N, M, pre=(buf["y1"][h], buf["part1"][h])))
            continue
        y1, part1 = T.linear_gn_partials(a, hw.w1, hw.b1, B, N, M, pre=(buf["y1"][h], buf["part1"][h]))
        out.append(T.neck_tail(y1, *hw[6:], B, P, part1))
    return _rot_dims(out, p)


def _rot_heads_fused(g, pf, pf_obj, p, rt, B, N, M):
    """Both RotHeads (heads/conv_out_per_rot_head.py:126-140) with the fused forward (train_ops._RotHeads, fp32)."""
    prm, packed = rt._train_packs(pf.device, 0)
    return _rot_dims(T.rot_heads(pf.detach(), pf_obj, prm, packed, B, N, M, *_head_pair(g, p)), p)


def forward_train(p, opts, x, tfd_kps, init_pose, init_scale, K_zoom=None, mean_scales=None, rt=None, forms=None):
    """p: {state_dict key: live parameter}.  Returns (pose [B,3,4], scale [B,3], aux dict) - autograd-connected.
    ``rt``: the model's :class:`~catre_amd.runtime.HipRuntime`; with it the fp32 encoder forward takes the fused kernels.
    ``forms``: (rot head, ts head) ``heads.HeadForm`` - None or the shipped form keeps every route below as it is; a head of
    another form runs layer by layer on the generic norm + activation ops."""
    from .heads import SHIPPED_FORM

    rot_form, ts_form = forms if forms is not None else (SHIPPED_FORM, SHIPPED_FORM)
    B, N, M = x.shape[0], x.shape[2], tfd_kps.shape[2]
    D = p["pcl_net.conv4.weight"].shape[0]   # PCLNET.INIT_CFG.out_dim; the fused encoder / head forwards are built for 1024
    hip.require_dev_f32(x, "x", (B, 3, N), contiguous=False)
    hip.require_dev_f32(tfd_kps, "tfd_kps", (B, 3, M), contiguous=False)
    pts_grad = x.requires_grad or tfd_kps.requires_grad
    enc_frozen = not pts_grad and not any(v.requires_grad for k, v in p.items() if k.startswith("pcl_net."))
    ft = bool(opts.feature_transform)
    # one decision, taken once (train_route.train_route states the ladders): which encoder, which nodes per conv stack, in
    # which row order the rotation heads read pointfeat, which form the heads take
    mode, knobs = _ambient()
    route = TR.train_route(mode, knobs, rt is not None, bool(getattr(rt, "layered", False)), rot_form == SHIPPED_FORM,
                           ts_form == SHIPPED_FORM, D, ft, B, N, M, rt is not None and N + M == rt.N + rt.M, enc_frozen,
                           pts_grad, route_shapes(p))
    enc = route.enc
    if enc.kind == "frozen":
        # PCLNET.FREEZE (CATRE_disR_shared.py:301-304): nothing in front of the heads needs a gradient, so the encoder runs
        # on the INFERENCE kernels - no activation saves, no arg-max rows, no graph nodes (and no encoder backward)
        # like train_stn3d: the first kernel of a training forward re-packs what it reads - the fingerprint cannot see writes
        # through `p.data` (the reference's own Ranger, EMA), and the heads' backward reads the LIVE w0 / w1
        rt._fingerprint = None
        st = rt.stage_pointnet(x, tfd_kps, feature_transform=ft)
        g, pfmax, pf = st["gfeat"][:, :D], st["gfeat"][:, D:], st["pointfeat"]
        hub = (pfmax, pf if route.x_cm else T.object_major(pf, B, N, M))
    elif enc.kind == "fused":
        g, pf, hub = pointnet_rows_fused(_cloud_major_rows(x, tfd_kps), hip.points_desc(x, tfd_kps), rt, p, B, N, M,
                                         mode=mode, obj_copy=route.obj_copy, route=enc)
    else:
        # D != 1024: the encoder is fp32 in every compute mode, with and without grad - its no-grad trunk (catre_trunk_w) is
        # an fp32 kernel, and a model's training forward and its no-grad forward take the same encoder precision; the heads
        # follow the mode.  (Also where autocast meets a stack that is no chain, e.g. a differentiable 3-d input.)
        with T.amp_mode(None if enc.mode == mode else "fp32"):   # (the ops record the mode for their backward)
            (g, pf), hub = pointnet_rows(_cloud_major_rows(x, tfd_kps), p, B, N, M, ft), None
    # max_n pointfeat (flat_pcl_feat tail) and the rot heads' input in object-major order: [N observed | M prior] per object
    # (CATRE_disR_shared.py:69, :86)
    pfmax, pf_obj = hub if hub is not None else (T.maxpool_points(pf, B, N, M), T.object_major(pf, B, N, M))

    # g (pooled feature, [2B,out_dim]) has three consumers - its first B rows go to the ts head, all of it to each rotation
    # head - and pfmax one that reads its first B rows: their gradients are summed by one launch each (train_ops._Hub)
    if opts.with_kps_feature or g.shape[0] == B:
        feats = [g[:B], pfmax[:B]] + ([g[B:], pfmax[B:]] if opts.with_kps_feature else [])
        gs = (g, g)
    else:
        g_ts, gx, gy = T.hub(g, B)
        feats = [g_ts, T.hub(pfmax, B)[0]]
        gs = (gx, gy)
    if opts.with_init_scale:
        feats.append(init_scale)
    if opts.with_init_trans:
        feats.append(init_pose[:, :3, 3])
    ts_feat = torch.cat(feats, 1)                                             # [B, ts_in]
    dt, ds = _ts_head(ts_feat, p, ts_form)

    if route.heads == "form":
        rx, ry = (_rot_head_form(gs[h], pf_obj, p, pre, B, N, M, rot_form) for h, pre in enumerate(_ROT_PREFIX))
    elif route.heads == "fused_f32":
        rx, ry = _rot_heads_fused(gs, pf, pf_obj, p, rt, B, N, M)
    elif route.heads == "split":
        rx, ry = _rot_heads_split(gs, pf, pf_obj, p, rt, B, N, M, route.split)
    elif route.heads == "lp_pair":
        rx, ry = _rot_heads_lp(gs, pf_obj, p, B, N, M, route.x_cm)
    else:
        rx, ry = (_rot_head(gs[h], pf_obj, p, pre, B, N, M, route.per_head[h]) for h, pre in enumerate(_ROT_PREFIX))
    rot6d = torch.cat([rx, ry], 1)

    pose, scale = T.pose_update_autograd(rot6d, dt, ds, init_pose, init_scale, mean_scales, K_zoom, opts)
    return pose, scale, dict(rot6d=rot6d, trans_deltas=dt, scale_deltas=ds)
