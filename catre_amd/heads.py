"""Residual heads of the CATRE hot path.  Inside ``CATRE_disR_shared.forward`` they are evaluated by the fused
driver (the concatenated feature tensors are never built); called on their own - the reference's module interface,
``heads/conv_out_per_rot_head.py:62-71,126-140`` and ``fc_trans_size_head.py:61-70`` on a materialised feature tensor -
they run layer by layer on the HIP training ops (``catre_amd/train_ops.py``), autograd included.

Mirrors ``core/catre/models/heads/conv_out_per_rot_head.py`` and ``fc_trans_size_head.py``:
same class names, constructor kwargs, three ModuleList slots per layer (``layers.{3i}`` conv, ``{3i+1}`` GroupNorm or
Identity, ``{3i+2}`` the shared activation module; ``linears`` likewise), never-used ``norm`` attribute, and initialisation
(N(0, 0.001^2) conv/linear weights, zero bias, GN weight 1; ``fc_t``/``fc_s`` N(0, 0.01^2)), so reference checkpoints load
``strict=True``.

Width (``feat_dim``: multiples of 8 up to 1024), depth, ``norm`` GN / none with any dividing ``num_gn_groups`` and ``act``
relu / lrelu / silu / gelu / mish / none are all built (:class:`HeadForm`).  The shipped form keeps the kernels written for
it; any other runs its norm + activation on the generic ops (``train_ops.gn_points_act`` / ``gn_rows_act``).
"""
import typing

import torch.nn as nn

from . import hip

def _normal_init(m, std):
    nn.init.normal_(m.weight, 0.0, std)
    if m.bias is not None:
        nn.init.constant_(m.bias, 0.0)


class HeadForm(typing.NamedTuple):
    """What the norm + activation kernels need to know about a head: width, depth, GroupNorm on / off and its group count,
    activation (``hip.ACT_*``)."""
    feat_dim: int
    num_layers: int
    norm: bool
    groups: int
    act: int


SHIPPED_FORM = HeadForm(256, 2, True, 32, hip.ACT_GELU)   # every shipped config: the fused kernels are built for it

_BN_FAMILY = ("BN", "BN1d", "SyncBN", "FrozenBN", "nnSyncBN", "naiveSyncBN", "IN")
_ACTS = {"relu": hip.ACT_RELU, "lrelu": hip.ACT_LRELU, "leaky_relu": hip.ACT_LRELU, "leakyrelu": hip.ACT_LRELU,
         "silu": hip.ACT_SILU, "swish": hip.ACT_SILU, "gelu": hip.ACT_GELU, "mish": hip.ACT_MISH, "none": hip.ACT_NONE,
         "": hip.ACT_NONE}
_PARAM_ACTS = ("prelu", "aconc", "metaaconc", "smu")


def _norm_on(norm):
    """True: GroupNorm, False: none (layer_utils.get_norm:41-45); anything else is not built."""
    if norm is None or (isinstance(norm, str) and norm.lower() in ("", "none")):
        return False
    if norm == "GN":
        return True
    if norm in _BN_FAMILY:
        raise NotImplementedError(
            f"norm={norm!r}: the HIP heads implement 'GN' and 'none'.  'BN' is BatchNorm2d, which the reference itself cannot "
            "feed with the heads' 3-D tensors; 'BN1d' and the other batch / instance norms need batch statistics and running "
            "buffers")
    raise ValueError(f"Unknown norm: {norm!r} (the HIP heads implement 'GN' and 'none')")


def _get_norm(norm, channels, num_gn_groups):
    if not _norm_on(norm):
        return nn.Identity()
    return nn.GroupNorm(num_gn_groups, channels)   # ValueError when num_gn_groups does not divide channels


def act_id(act):
    """``hip.ACT_*`` of an activation name as ``layer_utils.get_nn_act_func:61-95`` spells them."""
    if act is None:
        return hip.ACT_NONE
    a = act.lower()
    if a in _ACTS:
        return _ACTS[a]
    if a in _PARAM_ACTS:
        raise NotImplementedError(f"act={act!r}: activations with learned parameters (prelu, aconc, metaaconc, smu) are not "
                                  "built; the HIP heads implement relu, lrelu, silu / swish, gelu, mish and none")
    if a == "sigmoid":
        raise NotImplementedError("act='sigmoid' is not built; the HIP heads implement relu, lrelu, silu / swish, gelu, mish "
                                  "and none")
    raise ValueError(f"Unknown activation function: {act}.")   # layer_utils.py:94


def _get_act(act):
    """The module ``get_nn_act_func`` returns (no parameters, so no state_dict key): slope 0.1 for the leaky ReLU, the
    exact-erf GELU."""
    i = act_id(act)
    return {hip.ACT_NONE: nn.Identity, hip.ACT_RELU: lambda: nn.ReLU(inplace=True),
            hip.ACT_LRELU: lambda: nn.LeakyReLU(negative_slope=0.1, inplace=True), hip.ACT_SILU: lambda: nn.SiLU(inplace=True),
            hip.ACT_GELU: nn.GELU, hip.ACT_MISH: lambda: nn.Mish(inplace=True)}[i]()


def _head_form(what, feat_dim, num_layers, norm, num_gn_groups, act, num_classes, norm_input, dropout):
    if int(feat_dim) != feat_dim or feat_dim % 8 or not 8 <= feat_dim <= 1024:
        raise NotImplementedError(f"{what}: feat_dim={feat_dim!r} - the HIP heads take any multiple of 8 in 8..1024")
    if int(num_layers) != num_layers or num_layers < 1:
        raise ValueError(f"{what}: num_layers={num_layers!r} must be an integer >= 1")
    if num_classes != 1:
        raise NotImplementedError(f"{what}: num_classes={num_classes} (class-aware heads) is not built: num_classes=1")
    if norm_input:
        raise NotImplementedError(f"{what}: norm_input=True (a BatchNorm1d on the input) is not built")
    if dropout:
        raise NotImplementedError(f"{what}: dropout=True is not built")
    on = _norm_on(norm)
    return HeadForm(int(feat_dim), int(num_layers), on, int(num_gn_groups) if on else 1, act_id(act))


class RotHead(nn.Module):
    """reference conv_out_per_rot_head.py:74-140."""

    def __init__(self, in_dim=1024, feat_dim=256, num_layers=2, rot_dim=4, norm="none", num_gn_groups=32,
                 act="leaky_relu", num_classes=1, kernel_size=1, num_points=1, norm_input=False, dropout=False,
                 point_bias=True):
        super().__init__()
        if kernel_size != 1:
            raise NotImplementedError(f"HIP rot head: kernel_size={kernel_size} is not built (the heads are 1x1 convolutions)")
        if in_dim not in [d + 64 for d in hip.OUT_DIMS]:
            raise NotImplementedError(f"HIP rot head: in_dim={in_dim} is not built - its input is cat(out_dim pooled, 64 "
                                      f"point-feature) channels: in_dim = out_dim + 64 for out_dim in {set(hip.OUT_DIMS)}")
        if not 1 <= int(rot_dim) <= 3:
            raise NotImplementedError(f"HIP rot head: rot_dim={rot_dim} is not built - rot_dim in {{1,2,3}} (3: rot6d, "
                                      "2: quat)")
        self.form = _head_form("HIP rot head", feat_dim, num_layers, norm, num_gn_groups, act, num_classes, norm_input,
                               dropout)
        self.norm = _get_norm(norm, feat_dim, num_gn_groups)  # never used in forward (reference :92)
        self.act_func = act_func = _get_act(act)
        self.num_classes = num_classes
        self.rot_dim = rot_dim
        self.layers = nn.ModuleList()
        for i in range(num_layers):
            self.layers.append(nn.Conv1d(in_dim if i == 0 else feat_dim, feat_dim, kernel_size))
            self.layers.append(_get_norm(norm, feat_dim, num_gn_groups))
            self.layers.append(act_func)
        self.neck = nn.ModuleList([nn.Conv1d(feat_dim, rot_dim * num_classes, 1)])
        self.conv_p = nn.Conv1d(num_points, 1, 1, bias=point_bias)
        self._init_weights()

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Linear)):
                _normal_init(m, 0.001)
            elif isinstance(m, nn.GroupNorm):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0.0)

    def forward(self, x):
        """x [B,in_dim,P] -> (r [B,rot_dim], feat [B,rot_dim,P]) like the reference (``:126-140``): per layer conv -> norm ->
        act, then neck = feat -> conv_p over the points."""
        from . import train_ops as T

        B, C, P = x.shape
        if P != self.conv_p.in_channels:
            raise ValueError(f"RotHead was built for {self.conv_p.in_channels} points, got {P}")
        f = self.form
        a = x.permute(0, 2, 1).reshape(B * P, C)
        for i in range(f.num_layers):
            y = T.linear(a, self.layers[3 * i].weight, self.layers[3 * i].bias)
            if f == SHIPPED_FORM:
                a = T.gn_points_gelu(y, self.layers[3 * i + 1].weight, self.layers[3 * i + 1].bias, B, P)
            else:
                gn = self.layers[3 * i + 1]
                a = T.gn_points_act(y, gn.weight if f.norm else None, gn.bias if f.norm else None, B, P, f.groups, f.act,
                                    f.norm)
        y3 = neck_rows(a, self.neck[0].weight, self.neck[0].bias)             # [B*P,3], columns >= rot_dim are zero
        r = T.weighted_point_sum(y3, self.conv_p.weight, self.conv_p.bias, B, P)
        rd = self.rot_dim
        feat = y3.view(B, P, 3)[:, :, :rd].permute(0, 2, 1)                      # the reference's `feat = x.clone()` (:132)
        return r[:, :rd], feat  # a padded column only carries conv_p.bias: sliced away


def neck_weight3(weight, bias):
    """neck Conv1d(feat_dim -> rot_dim) parameters as [3,feat_dim] / [3], zero-padded (differentiable) for the 3-column kernels."""
    import torch.nn.functional as F

    rd = weight.shape[0]
    w = weight.reshape(rd, -1)
    if rd < 3:
        w = F.pad(w, (0, 0, 0, 3 - rd))
        bias = F.pad(bias, (0, 3 - rd)) if bias is not None else None
    return w, bias


def neck_rows(a, weight, bias):
    """neck Conv1d(feat_dim -> rot_dim, k=1) on point rows, zero-padded to the 3 columns the point-sum kernels are built for
    (pure data movement on [rot_dim,feat_dim] / [rot_dim]; gradients of the padding rows are dropped by autograd)."""
    import torch.nn.functional as F

    from . import train_ops as T

    rd = weight.shape[0]
    w = weight.reshape(rd, -1)
    if rd < 3:
        w = F.pad(w, (0, 0, 0, 3 - rd))
        bias = F.pad(bias, (0, 3 - rd)) if bias is not None else None
    return T.linear(a, w, bias)


class ConvOutPerRotHead(nn.Module):
    """reference conv_out_per_rot_head.py:10-71: two independent RotHeads (x axis, y axis) -> rot6d."""

    def __init__(self, in_dim=1024, feat_dim=256, num_layers=2, rot_dim=3, norm="GN", num_gn_groups=32, act="gelu",
                 num_classes=1, kernel_size=1, num_points=1, per_rot_sup=False, norm_input=False, dropout=False,
                 point_bias=True, **args):
        super().__init__()
        self.per_rot_sup = per_rot_sup
        mk = lambda: RotHead(in_dim, feat_dim, num_layers, rot_dim, norm, num_gn_groups, act, num_classes, kernel_size,
                             num_points, norm_input, dropout, point_bias)
        self.rot_head_x = mk()
        self.rot_head_y = mk()
        self.form = self.rot_head_x.form
        self.num_points = num_points
        self.rot_dim = rot_dim

    def forward(self, x):
        import torch

        rx, feat_x = self.rot_head_x(x)
        ry, feat_y = self.rot_head_y(x)
        r_pred = torch.cat((rx, ry), dim=1)            # [B, 2*rot_dim] (:63-66)
        if self.per_rot_sup:
            return r_pred, torch.cat((feat_x, feat_y), dim=1)   # (:68-69)
        return r_pred


class FC_TransSizeHead(nn.Module):
    """reference fc_trans_size_head.py:9-70."""

    def __init__(self, in_dim=1024, feat_dim=256, num_layers=2, rot_dim=4, norm="none", num_gn_groups=32,
                 act="leaky_relu", num_classes=1, norm_input=False, dropout=False):
        super().__init__()
        self.form = _head_form("HIP ts head", feat_dim, num_layers, norm, num_gn_groups, act, num_classes, norm_input,
                               dropout)
        self.norm = _get_norm(norm, feat_dim, num_gn_groups)  # never used in forward (reference :28)
        self.act_func = act_func = _get_act(act)
        self.num_classes = num_classes
        self.rot_dim = rot_dim
        self.in_dim = in_dim
        self.linears = nn.ModuleList()
        for i in range(num_layers):
            self.linears.append(nn.Linear(in_dim if i == 0 else feat_dim, feat_dim))
            self.linears.append(_get_norm(norm, feat_dim, num_gn_groups))
            self.linears.append(act_func)
        self.fc_t = nn.Linear(feat_dim, 3 * num_classes)
        self.fc_s = nn.Linear(feat_dim, 3 * num_classes)
        self._init_weights()

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Linear)):
                _normal_init(m, 0.001)
            elif isinstance(m, nn.GroupNorm):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0.0)
        _normal_init(self.fc_t, 0.01)
        _normal_init(self.fc_s, 0.01)

    def forward(self, x):
        """x [B,in_dim] -> (trans deltas [B,3], scale deltas [B,3])."""
        from . import train_ops as T

        f = self.form
        h = x.flatten(1)
        for i in range(f.num_layers):
            h = T.linear(h, self.linears[3 * i].weight, self.linears[3 * i].bias)
            gn = self.linears[3 * i + 1]
            if f == SHIPPED_FORM:
                h = T.gn_rows_gelu(h, gn.weight, gn.bias)
            else:
                h = T.gn_rows_act(h, gn.weight if f.norm else None, gn.bias if f.norm else None, f.groups, f.act, f.norm)
        return T.linear(h, self.fc_t.weight, self.fc_t.bias), T.linear(h, self.fc_s.weight, self.fc_s.bias)
