"""Host side of the fused optimizers (``catre_amd/optimizers.py``): everything that needs no GPU.

* ``tests/optim_oracle.py`` (the restatement the GPU tests measure against) reproduces, in fp32, every array that
  ``tests/golden/optim_steps.npz`` recorded from the reference classes.  The op sequence is the reference's, so the
  expectation is bit-equality; asserted is <= 4 fp32 ulps of each tensor's largest magnitude.
  Measured: 0 ulps - bit-equal - for every variant, parameter and state entry.  The projection ratios the restatement
  sees equal the recorded ones (asserted to 1e-6 relative).
* a ``state_dict`` recorded from the reference class loads into the fused class: ``load_state_dict``, key sets, the types
  of scalar state;
* ``build_model_optimizer`` dispatches the eight ``OPTIMIZER_CFG.type`` names to the fused classes; ``Ranger21``, ``Lamb`` and
  unknown names raise ``ValueError``;
* constructor validation raises what the reference raises.
"""
import ast

import numpy as np
import pytest
import torch

from catre_amd.config import default_cfg
from tests import optim_oracle as OO
from tests.optim_fixture import fixture, grads_for_step, reference_state, reference_state_dict, split_flat

ULPS = 4


@pytest.mark.parametrize("name", OO.variant_names())
def test_restatement_reproduces_the_reference_recording(name):
    cls, vname = name.split("/")
    z = fixture()
    params, draws = OO.make_problem(cls, int(z["meta_seed"]))
    shapes = [tuple(p.shape) for p in params]
    run = OO.Restated(cls, [p.clone() for p in params], OO.hypers_for(cls, OO.VARIANTS[cls][vname], len(params)))
    worst = 0.0

    def check(got, want, what):
        nonlocal worst
        ulp = OO.ulp_of(np.abs(want).max()) if want.size else 1.0
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) / ulp if want.size else 0.0
        worst = max(worst, err)
        assert err <= ULPS, f"{name} {what}: {err:.2f} ulps of the largest magnitude"

    for t in range(OO.STEPS):
        prev = split_flat(z[f"{name}/params"][t - 1], shapes) if t else params
        run.step(grads_for_step(cls, t, draws, params, prev), t)
        want = split_flat(z[f"{name}/params"][t], shapes)
        for i in range(len(params)):
            check(run.params[i].numpy(), want[i].numpy(), f"p{i} after step {t + 1}")
        if t + 1 in OO.STATE_STEPS:
            ref = reference_state(z, name, t + 1, shapes)
            for i, st in enumerate(ref):
                assert set(st) == set(run.state[i]), f"{name} state keys of tensor {i} at step {t + 1}"
                for key, val in st.items():
                    if torch.is_tensor(val):
                        check(run.state[i][key].numpy(), val.numpy(), f"{key}{i} at step {t + 1}")
                    else:
                        assert type(run.state[i][key]) is type(val), (key, type(run.state[i][key]), type(val))
                        assert run.state[i][key] == pytest.approx(val, rel=1e-15, abs=0), f"{name} {key}{i} at step {t + 1}"
            if cls == "MADGRAD":
                assert run.k == int(z[f"{name}/s{t + 1}/k"][0])
    if cls in OO.PROJECTION:
        rec = {(int(i), int(t)): [] for i, t, _, _ in z[f"{name}/ratios"]}
        for i, t, _, r in z[f"{name}/ratios"]:
            rec[(int(i), int(t))].append(r)
        assert set(rec) == set(run.ratios)
        for key, rs in rec.items():
            assert run.ratios[key] == pytest.approx(rs, rel=1e-6), f"{name} projection ratios of (tensor, step) {key}"
            assert all(r < 0.5 or r > 1.5 for r in rs)
    print(f"OPTIM_RESTATED {name}: worst {worst:.2f} ulps")


def _fused(cls):
    from catre_amd import optimizers

    return getattr(optimizers, cls)


def _groups(ps):
    return [dict({k: v for k, v in g.items() if k != "idx"}, params=[ps[i] for i in g["idx"] if i < len(ps)]) for g in OO.GROUPS]


@pytest.mark.parametrize("name", OO.variant_names())
def test_reference_state_dict_loads_into_the_fused_class(name):
    cls, vname = name.split("/")
    z = fixture()
    params, _ = OO.make_problem(cls, int(z["meta_seed"]))
    shapes = [tuple(p.shape) for p in params]
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = _fused(cls)(_groups(ps), **OO.VARIANTS[cls][vname])
    fresh = opt.state_dict()
    sd = reference_state_dict(z, name, shapes)
    # what the reference wrote has this class's param_groups keys (the two fused-only knobs are attributes, not group keys)
    assert [set(g) for g in sd["param_groups"]] == [set(g) for g in fresh["param_groups"]]
    for got, want in zip(fresh["param_groups"], sd["param_groups"]):
        assert got == want
    opt.load_state_dict(sd)
    ref = reference_state(z, name, 6, shapes)
    for i, p in enumerate(ps):
        st = opt.state[p] if p in opt.state else {}
        assert set(st) == set(ref[i]), f"{name}: state keys of tensor {i}"
        for key, val in ref[i].items():
            if torch.is_tensor(val):
                assert st[key].dtype == torch.float32 and torch.equal(st[key], val)
            else:
                assert type(st[key]) is type(val) and st[key] == val, (key, st[key], val)
    if cls == "MADGRAD":
        k = opt.state["k"]
        assert k.dtype == torch.long and tuple(k.shape) == (1,) and int(k) == 6 and not k.is_cuda
    # and the other way round: what the fused class writes has the same layout
    back = opt.state_dict()
    assert set(back) == set(sd) and set(back["state"]) == set(sd["state"])
    for idx, st in sd["state"].items():
        assert set(back["state"][idx]) == set(st) if isinstance(st, dict) else True


_CTOR = {
    "AdaBelief": dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-9, weight_decay=0.02, amsgrad=True, weight_decouple=True,
                      fixed_decay=True, rectify=True),
    "RangerAdaBelief": dict(lr=2e-4, alpha=0.6, k=5, N_sma_threshhold=4, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.02,
                            use_gc=False, gc_conv_only=True, gc_loc=False, adabelief=False, weight_decouple=False),
    "MADGRAD": dict(lr=2e-3, momentum=0.8, weight_decay=1e-4, eps=1e-7),
    "NAdamW": dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-9, weight_decay=0.02, momentum_decay=5e-3, amsgrad=True),
    "AdamP": dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-9, weight_decay=0.02, delta=0.2, wd_ratio=0.3, nesterov=True),
    "SGDP": dict(lr=2e-3, momentum=0.8, dampening=0.0, weight_decay=0.02, nesterov=True, eps=1e-9, delta=0.2, wd_ratio=0.3),
    "SGD_GC": dict(lr=2e-3, momentum=0.8, dampening=0.0, weight_decay=0.02, nesterov=True),
    "SGD_GCC": dict(lr=2e-3, momentum=0.8, dampening=0.1, weight_decay=0.02, nesterov=False),
}
_ATTRS = {"AdaBelief": ("weight_decouple", "fixed_decay", "rectify"),
          "RangerAdaBelief": ("use_gc", "gc_conv_only", "gc_loc", "adabelief", "weight_decouple", "alpha", "k", "N_sma_threshhold")}


@pytest.mark.parametrize("as_string", [False, True], ids=["dict", "string"])
@pytest.mark.parametrize("cls", OO.CLASSES)
def test_builder_dispatches_to_the_fused_class(cls, as_string):
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    cfg = default_cfg(device="cpu")
    kw = dict(_CTOR[cls], clean_grads=True, grad_limit=123.0)
    ocfg = dict(type=cls, **kw)
    cfg.SOLVER.OPTIMIZER_CFG = repr(ocfg) if as_string else ocfg
    if as_string:
        assert ast.literal_eval(cfg.SOLVER.OPTIMIZER_CFG) == ocfg
        cfg.SOLVER.OPTIMIZER_CFG = "dict(" + ", ".join(f"{k}={v!r}" for k, v in ocfg.items()) + ")"
    _, opt = build_model_optimizer(cfg, is_test=False)
    assert type(opt) is _fused(cls)
    lr, mult = float(cfg.SOLVER.BASE_LR), float(cfg.MODEL.CATRE.ROT_HEAD.get("LR_MULT", 1.0))
    assert len(opt.param_groups) == 3 and sum(len(g["params"]) for g in opt.param_groups) == 74
    assert opt.param_groups[0]["lr"] == pytest.approx(lr) and opt.param_groups[1]["lr"] == pytest.approx(lr * mult)
    assert opt.defaults["lr"] == kw["lr"]
    for g in opt.param_groups:
        for key, val in kw.items():
            if key in g and key != "lr":
                assert g[key] == val, (key, g[key], val)
    group_keys = set(opt.param_groups[0])
    for key in _ATTRS.get(cls, ()):
        assert getattr(opt, key) == kw[key], key
    assert all(key in group_keys or key in _ATTRS.get(cls, ()) or key in ("clean_grads", "grad_limit") for key in kw), cls
    assert opt.clean_grads is True and opt.grad_limit == 123.0
    cfg.SOLVER.CLIP_GRADIENTS = dict(ENABLED=True, CLIP_TYPE="full_model", CLIP_VALUE=0.5, NORM_TYPE=2.0)
    _, opt = build_model_optimizer(cfg, is_test=False)
    assert type(opt).__name__ == cls + "WithGradientClip" and isinstance(opt, _fused(cls))


@pytest.mark.parametrize("typ", ["Ranger21", "Lamb", "NoSuchOpt"])
def test_names_that_are_not_built_still_raise(typ):
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    cfg = default_cfg(device="cpu")
    cfg.SOLVER.OPTIMIZER_CFG = dict(type=typ, lr=1e-3)
    with pytest.raises(ValueError, match="Unknown optimizer name") as e:
        build_model_optimizer(cfg, is_test=False)
    for cls in OO.CLASSES:
        assert repr(cls) in str(e.value)   # the message lists what is available


_BAD = [
    ("AdaBelief", dict(lr=-1.0), "Invalid learning rate"), ("AdaBelief", dict(eps=-1.0), "Invalid epsilon value"),
    ("AdaBelief", dict(betas=(1.0, 0.9)), "Invalid beta parameter at index 0"),
    ("AdaBelief", dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1"),
    ("RangerAdaBelief", dict(alpha=1.5), "Invalid slow update rate"), ("RangerAdaBelief", dict(k=0), "Invalid lookahead steps"),
    ("RangerAdaBelief", dict(lr=0.0), "Invalid Learning Rate"), ("RangerAdaBelief", dict(eps=0.0), "Invalid eps"),
    ("MADGRAD", dict(momentum=1.0), "Momentum"), ("MADGRAD", dict(lr=0.0), "Learning rate"),
    ("MADGRAD", dict(weight_decay=-1.0), "Weight decay"), ("MADGRAD", dict(eps=-1.0), "Eps"),
    ("NAdamW", dict(lr=-1.0), "Invalid learning rate"), ("NAdamW", dict(eps=-1.0), "Invalid epsilon value"),
    ("NAdamW", dict(betas=(1.0, 0.9)), "index 0"), ("NAdamW", dict(betas=(0.9, 1.0)), "index 1"),
    ("NAdamW", dict(weight_decay=-1.0), "Invalid weight_decay value"), ("NAdamW", dict(momentum_decay=-1.0), "Invalid momentum_decay"),
    ("SGD_GC", dict(lr=-1.0), "Invalid learning rate"), ("SGD_GC", dict(lr=0.1, momentum=-1.0), "Invalid momentum value"),
    ("SGD_GC", dict(lr=0.1, weight_decay=-1.0), "Invalid weight_decay value"),
    ("SGD_GC", dict(lr=0.1, nesterov=True), "Nesterov momentum requires"),
    ("SGD_GCC", dict(lr=0.1, nesterov=True, momentum=0.9, dampening=0.1), "Nesterov momentum requires"),
    ("SGD_GCC", dict(lr=-1.0), "Invalid learning rate"),
]


@pytest.mark.parametrize("cls,kw,match", _BAD, ids=[f"{c}-{'-'.join(k)}" for c, k, _ in _BAD])
def test_constructor_validation_raises_what_the_reference_raises(cls, kw, match):
    with pytest.raises(ValueError, match=match):
        _fused(cls)([torch.nn.Parameter(torch.zeros(3))], **kw)


def test_constructor_signatures_and_defaults_are_the_reference_ones():
    import inspect

    for cls in OO.CLASSES:
        sig = inspect.signature(_fused(cls).__init__)
        names = [n for n in sig.parameters if n not in ("self", "params")]
        want = list(OO.DEFAULTS[cls])
        if cls in ("SGDP", "SGD_GC", "SGD_GCC"):
            want = ["lr"] + want   # lr=required
        assert names == want + ["clean_grads", "grad_limit"], cls
        for key, val in OO.DEFAULTS[cls].items():
            assert sig.parameters[key].default == val, (cls, key)
        assert sig.parameters["clean_grads"].default is False and sig.parameters["grad_limit"].default == 1e5


def test_cpu_or_non_fp32_tensors_are_an_error_not_a_fallback():
    from catre_amd import hip

    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(hip.CatreHipError, match="HIP devices only"):
        _fused("AdamP")([p]).step()
    q = torch.nn.Parameter(torch.zeros(4, 4))
    q.grad = torch.eye(4).to_sparse()
    with pytest.raises(RuntimeError, match="does not support sparse gradients"):
        _fused("NAdamW")([q]).step()
    with pytest.raises(RuntimeError, match="Ranger optimizer does not support sparse gradients"):
        _fused("RangerAdaBelief")([q]).step()
    with pytest.raises(RuntimeError, match="momentum != 0 is not compatible with sparse gradients"):
        _fused("MADGRAD")([q]).step()
