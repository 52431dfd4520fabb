"""Heads of any configured width, depth, norm and activation - the part that needs no GPU: every case of
``tests/golden/head_forms.npz`` (written by the unmodified reference, ``tools/make_head_golden.py``) constructs with the
reference's ``state_dict`` keys and shapes, and what is still not built says so."""
import json
import os

import numpy as np
import pytest
import torch

from catre_amd import heads, hip
from catre_amd.config import default_cfg
from tests.util import GOLDEN_DIR


def fixture():
    return np.load(os.path.join(GOLDEN_DIR, "head_forms.npz"), allow_pickle=False)


def _json(z, key):
    return json.loads(bytes(z[key]).decode())


def head_cases():
    return _json(fixture(), "meta_head_cases")   # name -> [kind, B, P | in_dim, constructor kwargs]


def model_cases():
    return _json(fixture(), "meta_model_cases")  # name -> [B, N, M, seed, salt, autocast record, cfg overrides]


def build_head(kind, dim, kw):
    if kind == "rot":
        return heads.RotHead(**dict(kw, in_dim=1088, num_points=dim, rot_dim=kw.get("rot_dim", 3)))
    return heads.FC_TransSizeHead(**dict(kw, in_dim=dim))


def model_cfg(name, device="cpu"):
    B, N, M, seed, salt, amp, over = model_cases()[name]
    cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=2, device=device)
    for path, v in over.items():
        node = cfg
        keys = path.split(".")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = v
    return cfg


@pytest.mark.parametrize("name", sorted(head_cases()))
def test_head_case_has_the_reference_state_dict(name):
    kind, B, dim, kw = head_cases()[name]
    want = [(k, tuple(s)) for k, s in _json(fixture(), f"{name}__meta")["keys"]]
    mod = build_head(kind, dim, kw)
    got = [(k, tuple(v.shape)) for k, v in mod.state_dict().items()]
    assert got == want   # same keys, same order, same shapes
    # a checkpoint written by the reference loads strict=True
    mod.load_state_dict({k: torch.zeros(s) for k, s in want}, strict=True)
    slots = mod.layers if kind == "rot" else mod.linears
    assert len(slots) == 3 * kw["num_layers"]
    assert all(slots[3 * i + 2] is mod.act_func for i in range(kw["num_layers"]))   # the shared activation module
    gn = kw.get("norm") == "GN"
    assert all(isinstance(slots[3 * i + 1], torch.nn.GroupNorm if gn else torch.nn.Identity) for i in range(kw["num_layers"]))
    assert isinstance(mod.norm, torch.nn.GroupNorm if gn else torch.nn.Identity)     # the never-used attribute stays


@pytest.mark.parametrize("name", ["M1", "M2"])
def test_whole_model_case_has_the_reference_state_dict(name):
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes

    cfg = model_cfg(name)
    model, opt = build_model_optimizer(cfg, is_test=False)
    want = [(k, tuple(s)) for k, s in _json(fixture(), f"{name}__meta")["keys"]]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want
    assert expected_state_shapes(cfg) == dict(want)
    model.load_state_dict({k: torch.zeros(s) for k, s in want}, strict=True)
    assert sum(len(g["params"]) for g in opt.param_groups) == len(list(model.parameters()))


def test_initialisation_is_the_references():
    """N(0, 0.001^2) conv / linear weights, zero biases, GroupNorm weight 1 / bias 0; fc_t / fc_s N(0, 0.01^2)."""
    torch.manual_seed(3)
    r = heads.RotHead(in_dim=1088, feat_dim=512, num_layers=3, rot_dim=3, norm="GN", num_gn_groups=16, act="mish", num_points=40)
    t = heads.FC_TransSizeHead(in_dim=1094, feat_dim=512, num_layers=3, norm="GN", num_gn_groups=16, act="silu")
    for mod in (r, t):
        for m in mod.modules():
            if isinstance(m, torch.nn.GroupNorm):
                assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
            elif isinstance(m, (torch.nn.Conv1d, torch.nn.Linear)):
                assert bool((m.bias == 0).all())
    assert 0.9e-3 < float(r.layers[3].weight.detach().std()) < 1.1e-3 and 0.9e-3 < float(t.linears[6].weight.detach().std()) < 1.1e-3
    assert 0.8e-2 < float(t.fc_t.weight.detach().std()) < 1.2e-2 and 0.8e-2 < float(t.fc_s.weight.detach().std()) < 1.2e-2


def test_activation_names_and_modules():
    for names, ident, cls in ((("relu", "ReLU"), hip.ACT_RELU, torch.nn.ReLU),
                              (("lrelu", "leaky_relu", "LeakyReLU"), hip.ACT_LRELU, torch.nn.LeakyReLU),
                              (("silu", "swish"), hip.ACT_SILU, torch.nn.SiLU), (("gelu",), hip.ACT_GELU, torch.nn.GELU),
                              (("mish",), hip.ACT_MISH, torch.nn.Mish), (("none", "", None), hip.ACT_NONE, torch.nn.Identity)):
        for n in names:
            h = heads.FC_TransSizeHead(in_dim=16, feat_dim=8, num_layers=1, act=n)
            assert h.form.act == ident and isinstance(h.act_func, cls), n
    assert heads.FC_TransSizeHead(in_dim=16, feat_dim=8, act="lrelu").act_func.negative_slope == 0.1   # get_nn_act_func
    assert heads.FC_TransSizeHead(in_dim=16, feat_dim=8, act="gelu").act_func.approximate == "none"     # exact erf
    for n in ("GN", "none", "", None):
        h = heads.RotHead(in_dim=1088, feat_dim=64, rot_dim=3, norm=n, num_gn_groups=4)
        assert h.form.norm == (n == "GN") and h.form.groups == (4 if n == "GN" else 1)
    with pytest.raises(ValueError, match="Unknown activation"):
        heads.RotHead(in_dim=1088, rot_dim=3, act="tanhh")


@pytest.mark.parametrize("kw, msg", [
    (dict(norm="BN"), "BatchNorm2d"), (dict(norm="BN1d"), "batch statistics"), (dict(norm="SyncBN"), "GN"),
    (dict(norm="IN"), "GN"), (dict(act="prelu"), "learned parameters"), (dict(act="aconc"), "learned parameters"),
    (dict(act="metaaconc"), "learned parameters"), (dict(act="smu"), "learned parameters"), (dict(act="sigmoid"), "sigmoid"),
    (dict(dropout=True), "dropout"), (dict(norm_input=True), "norm_input"), (dict(num_classes=6), "num_classes"),
    (dict(feat_dim=36), "multiple of 8"), (dict(feat_dim=2048), "multiple of 8"),
])
def test_values_that_are_not_built_raise_and_say_so(kw, msg):
    for ctor, base in ((heads.RotHead, dict(in_dim=1088, rot_dim=3)), (heads.FC_TransSizeHead, dict(in_dim=1091)),
                       (heads.ConvOutPerRotHead, dict(in_dim=1088, rot_dim=3))):
        with pytest.raises(NotImplementedError, match=msg):
            ctor(**dict(base, **kw))


def test_rot_head_only_values_that_are_not_built():
    with pytest.raises(NotImplementedError, match="kernel_size"):
        heads.RotHead(in_dim=1088, rot_dim=3, kernel_size=3)
    with pytest.raises(NotImplementedError, match="in_dim"):
        heads.RotHead(in_dim=1024, rot_dim=3)
    for rd in (0, 4, 6):
        with pytest.raises(NotImplementedError, match="rot_dim"):
            heads.RotHead(in_dim=1088, rot_dim=rd)
    with pytest.raises(ValueError, match="num_layers"):
        heads.RotHead(in_dim=1088, rot_dim=3, num_layers=0)


def test_group_count_must_divide_the_width_like_nn_groupnorm():
    for ctor, base in ((heads.RotHead, dict(in_dim=1088, rot_dim=3)), (heads.FC_TransSizeHead, dict(in_dim=1091))):
        with pytest.raises(ValueError):
            ctor(**dict(base, feat_dim=40, norm="GN", num_gn_groups=32))
        ctor(**dict(base, feat_dim=40, norm="none", num_gn_groups=32))   # no GroupNorm is built: nothing to divide


def test_graphed_wrappers_refuse_heads_of_another_form():
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from catre_amd.graphed import GraphedRefine

    model, _ = build_model_optimizer(model_cfg("M2"), is_test=True)
    with pytest.raises(NotImplementedError, match="shipped head form"):
        GraphedRefine(model, {})
