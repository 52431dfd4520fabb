"""The PointNet encoder at ``PCLNET.INIT_CFG.out_dim`` 64, 128, 256 and 512 - the part that needs no GPU: every case of
``tests/golden/out_dim.npz`` (written by the unmodified reference, ``tools/make_outdim_golden.py``) constructs with the
reference's ``state_dict`` keys and shapes, widths that do not fit together are caught at construction, what is not built
for another width than 1024 says so, and the new C entry points decide their status codes before any HIP call."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from catre_amd import heads, hip
from catre_amd.config import default_cfg
from catre_amd.pointnet import PointNetfeat
from tests.util import GOLDEN_DIR

WIDTHS = (64, 128, 256, 512)
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4   # catre_status


def fixture():
    return np.load(os.path.join(GOLDEN_DIR, "out_dim.npz"), allow_pickle=False)


def _json(z, key):
    return json.loads(bytes(z[key]).decode())


def cases():
    return _json(fixture(), "meta_cases")   # name -> [D, B, N, M, seed, salt, autocast record, cfg overrides]


def case_cfg(name, device="cpu"):
    D, B, N, M, seed, salt, amp, over = cases()[name]
    cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=2, device=device)
    for path, v in over.items():
        node = cfg
        keys = path.split(".")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = v
    return cfg


def width_cfg(D, device="cpu", N=64, M=64):
    """The base config with the three widths that follow out_dim."""
    cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=2, device=device)
    cfg.MODEL.CATRE.PCLNET.INIT_CFG.out_dim = D
    cfg.MODEL.CATRE.ROT_HEAD.INIT_CFG.in_dim = D + 64
    cfg.MODEL.CATRE.TS_HEAD.INIT_CFG.in_dim = D + 64 + 3
    return cfg


@pytest.mark.parametrize("D", WIDTHS)
def test_pointnetfeat_constructs_at_the_width(D):
    net = PointNetfeat(num_points=64, out_dim=D)
    assert tuple(net.conv4.weight.shape) == (D, 512, 1) and tuple(net.conv4.bias.shape) == (D,)
    assert tuple(net.stn.conv3.weight.shape) == (1024, 128, 1)   # the STNs do not follow out_dim (pointnet.py:13-78)
    assert tuple(PointNetfeat(num_points=64, out_dim=D, feature_transform=True).fstn.conv3.weight.shape) == (1024, 128, 1)


@pytest.mark.parametrize("name", sorted(cases()))
def test_case_has_the_reference_state_dict(name):
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.runtime import opts_from_cfg

    D = cases()[name][0]
    cfg = case_cfg(name)
    model, opt = build_model_optimizer(cfg, is_test=False)
    want = [(k, tuple(s)) for k, s in _json(fixture(), f"{name}__meta")["keys"]]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want   # same keys, same order, same shapes
    assert expected_state_shapes(cfg) == dict(want)
    assert dict(want)["pcl_net.conv4.weight"] == (D, 512, 1)
    model.load_state_dict({k: torch.zeros(s) for k, s in want}, strict=True)
    n_enc = 32 if cfg.MODEL.CATRE.PCLNET.INIT_CFG.feature_transform else 20
    assert [len(g["params"]) for g in opt.param_groups] == [n_enc, 28, 14]
    assert opts_from_cfg(cfg).ts_in_dim == cfg.MODEL.CATRE.TS_HEAD.INIT_CFG.in_dim == dict(want)["ts_head.linears.0.weight"][1]
    assert model._runtime().out_dim == D and model._runtime().layered


def test_param_groups_of_the_base_config_at_256():
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    _, opt = build_model_optimizer(width_cfg(256), is_test=False)
    assert [len(g["params"]) for g in opt.param_groups] == [32, 28, 14]


@pytest.mark.parametrize("D", [100, 960, 2048])
def test_widths_outside_the_set_raise_and_name_it(D):
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    with pytest.raises(NotImplementedError, match="out_dim") as e:
        PointNetfeat(num_points=64, out_dim=D)
    assert all(str(d) in str(e.value) for d in (64, 128, 256, 512, 1024))
    with pytest.raises(NotImplementedError, match="out_dim"):
        build_model_optimizer(width_cfg(D), is_test=True)
    with pytest.raises(NotImplementedError, match="in_dim"):
        heads.RotHead(in_dim=D + 64, rot_dim=3)


def test_rot_head_width_1024_is_still_refused():
    with pytest.raises(NotImplementedError, match="in_dim"):
        heads.RotHead(in_dim=1024, rot_dim=3)
    with pytest.raises(NotImplementedError, match="in_dim"):
        heads.ConvOutPerRotHead(in_dim=1024, rot_dim=3)
    for D in WIDTHS + (1024,):
        assert tuple(heads.RotHead(in_dim=D + 64, rot_dim=3).layers[0].weight.shape) == (256, D + 64, 1)


def test_widths_that_do_not_fit_together_raise_value_error():
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    cfg = width_cfg(256)
    cfg.MODEL.CATRE.ROT_HEAD.INIT_CFG.in_dim = 1088
    with pytest.raises(ValueError, match="1088") as e:
        build_model_optimizer(cfg, is_test=True)
    assert "320" in str(e.value)
    cfg = width_cfg(256)
    cfg.MODEL.CATRE.TS_HEAD.INIT_CFG.in_dim = 1091
    with pytest.raises(ValueError, match="1091") as e:
        build_model_optimizer(cfg, is_test=True)
    assert "323" in str(e.value)
    cfg = width_cfg(128)
    cfg.MODEL.CATRE.TS_HEAD.WITH_KPS_FEATURE = True   # needs 2 x 192 + 3
    with pytest.raises(ValueError, match="195") as e:
        build_model_optimizer(cfg, is_test=True)
    assert "387" in str(e.value)
    cfg = default_cfg(device="cpu")    # the shipped width with a narrow rot head
    cfg.MODEL.CATRE.ROT_HEAD.INIT_CFG.in_dim = 320
    with pytest.raises(ValueError, match="320"):
        build_model_optimizer(cfg, is_test=True)


def test_graphed_wrappers_and_fp16_refuse_another_width():
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from catre_amd.graphed import GraphedRefine, GraphedTrainLoop, GraphedTrainStep
    from catre_amd.runtime import HipRuntime

    model, opt = build_model_optimizer(width_cfg(256), is_test=False)
    with pytest.raises(NotImplementedError, match="out_dim"):
        GraphedRefine(model, {})
    with pytest.raises(NotImplementedError, match="out_dim"):
        GraphedTrainStep(model, opt, {}, [])
    with pytest.raises(NotImplementedError, match="out_dim"):
        GraphedTrainLoop(model, opt, 64, 64, (2,))
    rt = model._runtime()
    o = model._opts_f16
    with pytest.raises(NotImplementedError, match="out_dim"):   # decided before anything touches a device
        rt._refine_iter_layered(None, None, None, None, None, None, o)
    model.cfg.MODEL.CATRE.COMPUTE_DTYPE = "fp16"
    assert model._inference_opts().compute_dtype == hip.DTYPE_F16
    # the entry points that read conv4 as [1024,512] / rot layer 0 as [256,1088] are never handed these weights
    for call in (lambda: rt._train_packs("cpu", 0), lambda: rt.stage_ts_head(torch.zeros(2, 320), None, torch.zeros(2, 3), o),
                 lambda: rt.stage_rot_head(torch.zeros(4, 320), None, 2, 64, 64)):
        with pytest.raises(NotImplementedError, match="out_dim"):
            call()
    with pytest.raises(NotImplementedError, match="out_dim"):
        HipRuntime(lambda: {}, 1, 1, 1, out_dim=96)


def test_new_entry_points_decide_their_status_without_a_gpu():
    lib = hip.load()
    floats = [lib.catre_packed_floats_w(d) for d in (64, 128, 256, 512, 1024)]
    assert all(a < b for a, b in zip(floats, floats[1:])) and floats[0] > 0
    assert [b - a for a, b in zip(floats, floats[1:])] == [64 * 512, 128 * 512, 256 * 512, 512 * 512]   # conv4's rows
    assert [lib.catre_packed_floats_w(d) for d in (0, -64, 96, 100, 960, 2048)] == [0] * 6
    buf = (ctypes.c_float * 16)()       # host memory: a call that got as far as a launch would be a bug of this test
    p = ctypes.cast(buf, ctypes.c_void_p)
    prm = (ctypes.c_void_p * hip.CATRE_P_COUNT)(*([p.value] * hip.CATRE_P_COUNT))
    pts = hip.CatrePoints()
    assert lib.catre_pack_encoder_w(None, 256, p, 1 << 30, None) == BAD_ARG
    assert lib.catre_pack_encoder_w(prm, 256, None, 1 << 30, None) == BAD_ARG
    assert lib.catre_pack_encoder_w(prm, 96, p, 1 << 30, None) == UNSUPPORTED
    assert lib.catre_pack_encoder_w(prm, 256, p, lib.catre_packed_floats_w(256) - 1, None) == WORKSPACE
    ok = [ctypes.byref(pts), p, p, prm, p, 256, p, p, p, 1 << 40, 2, 64, 64, None]
    for i in (0, 1, 3, 4, 6, 7, 8):     # every pointer but trans64 (NULL: no feature transform)
        args = list(ok)
        args[i] = None
        assert lib.catre_trunk_w(*args) == BAD_ARG, i
    for i, v in ((10, 0), (11, 0), (11, -1), (12, -1)):
        args = list(ok)
        args[i] = v
        assert lib.catre_trunk_w(*args) == BAD_ARG, (i, v)
    for d in (96, 0, 2048):
        args = list(ok)
        args[5] = d
        assert lib.catre_trunk_w(*args) == UNSUPPORTED, d
    args = list(ok)
    args[9] = lib.catre_workspace_bytes(2, 64, 64) - 1
    assert lib.catre_trunk_w(*args) == WORKSPACE


def test_fixture_is_small_and_holds_results_only():
    z = fixture()
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "out_dim.npz")) < 800 * 1024
    assert not any(k.split("__")[-1].startswith("in_") for k in z.files)
    assert sorted(cases()) == ["W128", "W256", "W512", "W64"] and [cases()[k][0] for k in sorted(cases())] == [128, 256, 512, 64]
