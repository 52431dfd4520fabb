"""The fused optimizer steps (``catre_op_optim_step``, ``catre_amd/optimizers.py``) on the device.

(a) every variant of ``tests/golden/optim_steps.npz`` (the reference classes' own recorded runs) through the fused class:
    parameters after each step, state after steps 6 and 13; then a fresh fused optimizer that loads the reference's step-6
    ``state_dict`` and continues to step 13;
(b) chunk / trip / row-length edges against the restatement (``tests/optim_oracle.py``) in fp64 with fp32 storage;
(c) properties that hold bit for bit;
(d) two training iterations through ``build_model_optimizer`` for each ``type``, and the packed-weight caches afterwards;
(e) steps after the first under ``torch.cuda.set_sync_debug_mode("error")``.

Bound of (a) and (b), the rule of ``tests/test_ranger_edges.py``: per case and per kind of tensor (parameter, each state
entry), ``max |fused - fp64| <= MULT x max(max |fp32 reference - fp64|, one fp32 ulp of the largest fp64 value)``.  The fp32
reference is the fixture (the reference class itself) in (a) and the restatement run in fp32 on the CPU in (b) - never
anything the fused step produced.  MULT = 2: the kernel is one more fp32 evaluation of the same formulas in another
rounding order (contracted multiply-adds, wave-tree row sums), so it may stray about as far from fp64 as the fp32
reference does and no further.

Measured on an MI355X, |fused - fp64| / bound:
(a) per variant, run from the start / resumed from the reference's step-6 state_dict (worst entry):
    AdaBelief: default 1.00/1.00  amsgrad 1.00/1.50  decouple 1.00/1.00  fixed_decay 1.00/1.00  rectify
        1.00/1.00
    RangerAdaBelief: default 1.00/1.00  no_gc 1.17/1.17  conv_only 1.00/1.00  gc_after 1.25/1.20  no_belief
        1.33/1.33  coupled 1.00/1.00  gc_after_conv_only_no_belief 1.00/1.00
    MADGRAD: default 0.75/0.75  no_momentum 1.00/1.00
    NAdamW: default 1.00/1.00  amsgrad 1.00/1.00
    AdamP: default 1.00/1.00  nesterov 1.00/1.00
    SGDP: default 1.00/1.00  momentum 1.00/1.00  nesterov 1.00/1.00
    SGD_GC: default 0.50/0.50  momentum 1.00/1.00  nesterov 1.00/1.00
    SGD_GCC: momentum 1.08/1.00
(b) per configuration and case (worst entry of parameter and state):
    AdaBelief: 1d_1 1.50  1d_255 1.00  1d_256 1.00  1d_257 1.00  1d_1023 1.25  1d_1024 1.00  1d_1025 1.00
        1d_4095 1.00  1d_4096 1.50  1d_4097 1.00  1d_8193 1.00  5x63 1.00  5x64 1.00  5x65 1.33  3x255 1.00
        3x256 1.00  3x257 1.33  3x4097 1.00  64x1x1 1.00  4x3x2x2_conv_and_fc 1.00  mixed_300 1.00
    RangerAdaBelief: 1d_1 1.00  1d_255 1.00  1d_256 1.00  1d_257 1.00  1d_1023 1.00  1d_1024 1.00  1d_1025 1.00
        1d_4095 1.00  1d_4096 1.25  1d_4097 1.00  1d_8193 1.00  5x63 1.00  5x64 1.00  5x65 1.00  3x255 1.00
        3x256 1.00  3x257 1.00  3x4097 1.00  64x1x1 1.00  4x3x2x2_conv_only 1.00  4x3x2x2_conv_and_fc 1.25
        mixed_300 1.00
    RangerAdaBelief-gc_after: 1d_1 1.00  1d_255 1.00  1d_256 1.00  1d_257 1.00  1d_1023 1.00  1d_1024 1.00
        1d_1025 1.00  1d_4095 1.00  1d_4096 1.25  1d_4097 1.00  1d_8193 1.00  5x63 1.00  5x64 1.50  5x65 1.00
        3x255 1.00  3x256 1.00  3x257 1.00  3x4097 1.00  64x1x1 1.00  4x3x2x2_conv_only 0.75
        4x3x2x2_conv_and_fc 1.00  mixed_300 1.00
    MADGRAD: 1d_1 1.00  1d_255 1.00  1d_256 1.00  1d_257 1.00  1d_1023 1.00  1d_1024 1.00  1d_1025 1.00  1d_4095
        1.00  1d_4096 1.00  1d_4097 1.00  1d_8193 1.00  5x63 1.00  5x64 1.00  5x65 1.00  3x255 1.00  3x256 1.00
        3x257 1.00  3x4097 1.00  64x1x1 1.00  4x3x2x2_conv_and_fc 1.50  mixed_300 1.00
    NAdamW: 1d_1 1.00  1d_255 2.00  1d_256 1.00  1d_257 1.60  1d_1023 1.00  1d_1024 1.00  1d_1025 1.00  1d_4095
        1.20  1d_4096 1.00  1d_4097 1.00  1d_8193 1.00  5x63 1.20  5x64 1.25  5x65 1.25  3x255 1.25  3x256 1.25
        3x257 1.00  3x4097 1.00  64x1x1 1.33  4x3x2x2_conv_and_fc 1.67  mixed_300 1.40
    AdamP: 1d_1 1.00  1d_255 2.00  1d_256 1.00  1d_257 1.60  1d_1023 1.00  1d_1024 1.00  1d_1025 1.00  1d_4095
        1.00  1d_4096 1.00  1d_4097 1.00  1d_8193 1.00  5x63 1.20  5x64 1.00  5x65 1.00  3x255 1.00  3x256 1.00
        3x257 1.00  3x4097 1.00  64x1x1 1.33  4x3x2x2_conv_and_fc 1.00  mixed_300 1.00  steer_5x65 1.00
        steer_3x4097 1.20
    SGDP: 1d_1 1.00  1d_255 1.00  1d_256 1.00  1d_257 1.00  1d_1023 1.50  1d_1024 1.00  1d_1025 1.00  1d_4095
        1.00  1d_4096 1.00  1d_4097 1.00  1d_8193 1.00  5x63 1.00  5x64 1.00  5x65 1.33  3x255 1.00  3x256 1.00
        3x257 1.00  3x4097 1.00  64x1x1 1.50  4x3x2x2_conv_and_fc 1.00  mixed_300 1.00  steer_5x65 1.00
        steer_3x4097 1.00
    SGD_GC: 1d_1 0.50  1d_255 1.00  1d_256 1.00  1d_257 1.00  1d_1023 1.00  1d_1024 1.00  1d_1025 1.00  1d_4095
        1.00  1d_4096 0.92  1d_4097 1.00  1d_8193 1.00  5x63 1.00  5x64 1.00  5x65 1.00  3x255 1.00  3x256 1.00
        3x257 1.25  3x4097 1.00  64x1x1 0.00  4x3x2x2_conv_and_fc 1.50  mixed_300 1.00
    SGD_GCC: 1d_1 1.00  1d_255 1.00  1d_256 1.00  1d_257 1.00  1d_1023 1.00  1d_1024 1.00  1d_1025 1.50  1d_4095
        1.00  1d_4096 1.00  1d_4097 1.00  1d_8193 1.00  5x63 1.00  5x64 1.00  5x65 1.00  3x255 1.00  3x256 1.00
        3x257 1.00  3x4097 1.00  64x1x1 0.80  4x3x2x2_conv_and_fc 0.75  mixed_300 1.00
The worst is 2.00, twice: exp_avg of AdamP and of NAdamW at 1d_255 (the same moment update on the same seeded gradients).
Both sides of the ratio are small whole numbers of fp32 ulps of the largest value, so it moves in steps; 2.00 is at MULT,
not above it.  No class needs more than MULT = 2: neither the cube root nor the ``p_n . perturb`` cancellation shows
(MADGRAD <= 1.50, the steered projection cases <= 1.20).
"""
import copy

import numpy as np
import pytest
import torch

from tests import optim_oracle as OO
from tests.optim_fixture import fixture, grads_for_step, reference_state, reference_state_dict, split_flat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MULT = 2.0   # see the module docstring


def _fused(cls):
    from catre_amd import optimizers

    return getattr(optimizers, cls)


def _dev_params(params):
    return [torch.nn.Parameter(p.clone().to(DEV)) for p in params]


def _groups(ps, groups=OO.GROUPS):
    return [dict({k: v for k, v in g.items() if k != "idx"}, params=[ps[i] for i in g["idx"] if i < len(ps)]) for g in groups]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().reshape(-1)


def _snap(opt, p):
    """Bits of the parameter and of its whole optimizer state; scalar state as it is."""
    st = opt.state[p] if p in opt.state else {}
    out = dict(p=_bits(p))
    for key, val in st.items():
        out[key] = _bits(val) if torch.is_tensor(val) else val
    return out


def _assert_same_bits(a, b, msg):
    assert set(a) == set(b), f"{msg}: keys {sorted(a)} != {sorted(b)}"
    for key in a:
        if torch.is_tensor(a[key]):
            n = int((a[key] != b[key]).sum())
            assert n == 0, f"{msg}: {key} differs in {n} of {a[key].numel()} elements"
        else:
            assert a[key] == b[key], f"{msg}: {key} {a[key]} != {b[key]}"


class _Track:
    """max |fused - fp64|, max |fp32 reference - fp64| and the largest fp64 value per kind of tensor."""

    def __init__(self):
        self.kern, self.yard, self.top = {}, {}, {}

    def add(self, key, got, ref32, ref64):
        ref64 = ref64.double()
        self.kern[key] = max(self.kern.get(key, 0.0), float((got.double() - ref64).abs().max()))
        self.yard[key] = max(self.yard.get(key, 0.0), float((ref32.double() - ref64).abs().max()))
        self.top[key] = max(self.top.get(key, 0.0), float(ref64.abs().max()))

    def check(self, tag):
        ratios = {}
        for key in self.kern:
            bound = max(self.yard[key], OO.ulp_of(self.top[key]))
            ratios[key] = self.kern[key] / bound
        print(f"OPTIM_RATIO {tag}: " + "  ".join(f"{k} {r:.2f}" for k, r in ratios.items()))
        for key, r in ratios.items():
            assert r <= MULT, (f"{tag} {key}: |fused - fp64| {self.kern[key]:.3e} > {MULT} x max(fp32 reference's own "
                               f"{self.yard[key]:.3e}, ulp {OO.ulp_of(self.top[key]):.3e})")


def _track_state(track, opt, ps, ref32, ref64):
    for i, p in enumerate(ps):
        st = opt.state[p] if p in opt.state else {}
        assert set(st) == set(ref64[i]) == set(ref32[i]), f"state keys of tensor {i}: {sorted(st)} vs {sorted(ref64[i])}"
        for key, val in ref64[i].items():
            if torch.is_tensor(val):
                track.add(key, st[key].cpu(), ref32[i][key], val)
            else:
                assert type(st[key]) is type(ref32[i][key]) and st[key] == pytest.approx(ref32[i][key], rel=1e-15, abs=0), key


# --------------------------------------------------------------------------------------------- (a) fixture variants
@pytest.mark.parametrize("name", OO.variant_names())
def test_fixture_variant_and_resume_from_the_reference_state_dict(name):
    cls, vname = name.split("/")
    ctor = OO.VARIANTS[cls][vname]
    z = fixture()
    params, draws = OO.make_problem(cls, int(z["meta_seed"]))
    shapes = [tuple(p.shape) for p in params]
    n = len(params)
    recorded = [split_flat(row, shapes) for row in z[f"{name}/params"]]
    grads = [grads_for_step(cls, t, draws, params, recorded[t - 1] if t else params) for t in range(OO.STEPS)]
    r64 = OO.Restated(cls, [p.double() for p in params], OO.hypers_for(cls, ctor, n), storage=torch.float32)
    ps = _dev_params(params)
    opt = _fused(cls)(_groups(ps), **ctor)
    ps2, opt2 = None, None
    track, track2 = _Track(), _Track()
    for t in range(OO.STEPS):
        for i, p in enumerate(ps):
            p.grad = None if grads[t][i] is None else grads[t][i].to(DEV)
        opt.step()
        if opt2 is not None:
            for i, p in enumerate(ps2):
                p.grad = None if grads[t][i] is None else grads[t][i].to(DEV)
            opt2.step()
        r64.step(grads[t], t)
        for i in range(n):
            track.add("p", ps[i].detach().cpu(), recorded[t][i], r64.params[i])
            if opt2 is not None:
                track2.add("p", ps2[i].detach().cpu(), recorded[t][i], r64.params[i])
        if t + 1 in OO.STATE_STEPS:
            ref32 = reference_state(z, name, t + 1, shapes)
            _track_state(track, opt, ps, ref32, r64.state)
            if opt2 is not None:
                _track_state(track2, opt2, ps2, ref32, r64.state)
            if cls == "MADGRAD":
                assert int(opt.state["k"]) == t + 1 == int(z[f"{name}/s{t + 1}/k"][0])
        if t + 1 == 6:   # a fresh fused optimizer picks the reference's run up from its state_dict
            ps2 = _dev_params(recorded[t])
            opt2 = _fused(cls)(_groups(ps2), **ctor)
            opt2.load_state_dict(reference_state_dict(z, name, shapes))
    if cls in OO.PROJECTION:
        assert all(r < 0.5 or r > 1.5 for rs in r64.ratios.values() for r in rs), "a projection decision depends on rounding"
    track.check(f"fixture {name}")
    track2.check(f"resumed {name}")


# --------------------------------------------------------------------------------------------- (b) tiling edges
EDGE_STEPS = 7   # the RAdam / rectify switch and a lookahead merge at 6; the host arithmetic of later steps is (a)'s
EDGE_GROUPS = [dict(idx=None, lr=2e-2), dict(idx=None, lr=5e-3, weight_decay=0.1)]   # tensor i goes to group i % 2
# one configuration per class that takes its longest path (RangerAdaBelief twice: the two places of centralization)
EDGE_CONFIGS = {
    "AdaBelief": dict(rectify=True, amsgrad=True), "RangerAdaBelief": {}, "RangerAdaBelief-gc_after": dict(gc_loc=False),
    "MADGRAD": {}, "NAdamW": dict(amsgrad=True), "AdamP": dict(nesterov=True), "SGDP": dict(momentum=0.9, dampening=0.1),
    "SGD_GC": dict(momentum=0.9, nesterov=True), "SGD_GCC": dict(momentum=0.9, dampening=0.1),
}


def _mixed_shapes(n=300, seed=7):
    """Small odd shapes of every rank: long row_off and chunk tables, row lengths on both sides of the wave width."""
    rs = np.random.RandomState(seed)
    shapes = []
    for j in range(n):
        kind = j % 4
        if kind == 0:
            shapes.append((int(rs.randint(1, 140)),))
        elif kind == 1:
            shapes.append((int(rs.randint(1, 10)), int(rs.randint(1, 131))))
        elif kind == 2:
            shapes.append((int(rs.randint(1, 8)), int(rs.randint(1, 12)), int(rs.randint(1, 8))))
        else:
            shapes.append((int(rs.randint(1, 6)), int(rs.randint(1, 5)), 3, int(rs.randint(1, 4))))
    return shapes


EDGE_CASES = {f"1d_{n}": dict(shapes=[(n,), (n,)]) for n in (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)}
EDGE_CASES.update({"x".join(map(str, s)): dict(shapes=[s, s]) for s in (
    (5, 63), (5, 64), (5, 65), (3, 255), (3, 256), (3, 257), (3, 4097), (64, 1, 1))})
# (6, 7) rides along: centralized with gc_conv_only=False / by SGD_GC, not with True / by SGD_GCC
EDGE_CASES["4x3x2x2_conv_only"] = dict(shapes=[(4, 3, 2, 2), (6, 7), (6, 7), (4, 3, 2, 2)], ctor=dict(gc_conv_only=True))
EDGE_CASES["4x3x2x2_conv_and_fc"] = dict(shapes=[(4, 3, 2, 2), (6, 7), (6, 7), (4, 3, 2, 2)])
EDGE_CASES["mixed_300"] = dict(shapes=_mixed_shapes())
# the projection's three constructions (none / channel view / layer view only), one tensor each, in both groups' turn
# (the random tensor's cosines are what they are: the seeds are the first from 3000 on with every ratio outside [0.5, 1.5] in
# the CPU restatement's runs, fp64 and fp32, of both classes)
for _s, _seed in (((5, 65), 3002), ((3, 4097), 3000)):
    EDGE_CASES["steer_" + "x".join(map(str, _s))] = dict(shapes=[_s] * 4, seed=_seed,
                                                         steer={0: "none", 1: "channel", 2: "layer", 3: "channel"})


def _edge_params():
    out = []
    for config in EDGE_CONFIGS:
        cls = config.split("-")[0]
        for case, spec in EDGE_CASES.items():
            if "ctor" in spec and cls != "RangerAdaBelief":
                continue   # gc_conv_only is RangerAdaBelief's option; SGD_GC / SGD_GCC are the two forms of the others
            if "steer" in spec and cls not in OO.PROJECTION:
                continue
            out.append((config, case))
    return out


def _edge_groups(n):
    return [dict(g, idx=tuple(range(j, n, 2))) for j, g in enumerate(EDGE_GROUPS)]


@pytest.mark.parametrize("config,case", _edge_params(), ids=[f"{a}-{b}" for a, b in _edge_params()])
def test_tiling_edges_match_the_fp64_restatement(config, case):
    cls, spec = config.split("-")[0], EDGE_CASES[case]
    ctor = dict(EDGE_CONFIGS[config], **spec.get("ctor", {}))
    shapes, steer = spec["shapes"], spec.get("steer", {})
    n = len(shapes)
    params, draws = OO.make_problem(cls, seed=spec.get("seed", 2000 + list(EDGE_CASES).index(case)), shapes=shapes,
                                    steps=EDGE_STEPS, steer=steer)
    groups = _edge_groups(n)
    hypers = OO.hypers_for(cls, ctor, n, groups)
    r64 = OO.Restated(cls, [p.double() for p in params], hypers, storage=torch.float32)
    r32 = OO.Restated(cls, [p.clone() for p in params], hypers)
    ps = _dev_params(params)
    opt = _fused(cls)(_groups(ps, groups), **ctor)
    track = _Track()
    for t in range(EDGE_STEPS):
        grads = [OO.gradient(steer.get(i), draws[t][i], params[i], r32.params[i]) for i in range(n)]
        for i, p in enumerate(ps):
            p.grad = grads[i].to(DEV)
        opt.step()
        r64.step(grads, t)
        r32.step(grads, t)
        for i in range(n):
            track.add("p", ps[i].detach().cpu(), r32.params[i], r64.params[i])
    _track_state(track, opt, ps, r32.state, r64.state)
    if steer:   # no decision depends on rounding, and each construction did what it is for, at every step
        assert len(r64.ratios) == n * EDGE_STEPS
        for (i, t), v in r64.ratios.items():
            assert all(r < 0.5 or r > 1.5 for r in v), f"{case}: a projection decision of tensor {i}, step {t} depends on rounding: {v}"
            want = {"none": [False, False], "channel": [True], "layer": [False, True]}[steer[i]]
            assert [r < 1 for r in v] == want, (case, i, t, v)
    track.check(f"edge {config} {case}")


# --------------------------------------------------------------------------------------------- (c) exact properties
PROP_CTOR = {
    "AdaBelief": dict(rectify=True), "RangerAdaBelief": dict(gc_loc=False), "MADGRAD": {}, "NAdamW": {}, "AdamP": {},
    "SGDP": dict(momentum=0.9), "SGD_GC": dict(momentum=0.9), "SGD_GCC": dict(momentum=0.9),
}
PROP_STEPS = 7


def _problem(shapes, seed, steps=PROP_STEPS):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) + (0.5 * params[i] if len(s) > 1 else 0) for i, s in enumerate(shapes)]
             for _ in range(steps)]
    return params, grads


def _make(cls, ps, **extra):
    return _fused(cls)([dict(params=ps, lr=2e-2, weight_decay=0.1)], **dict(PROP_CTOR[cls], **extra))


def _run(cls, params, grads, steps=PROP_STEPS, grad_of=None, opt_ps=None, first=0, **extra):
    ps = _dev_params(params) if opt_ps is None else opt_ps[1]
    opt = _make(cls, ps, **extra) if opt_ps is None else opt_ps[0]
    for t in range(first, steps):
        for i, p in enumerate(ps):
            g = grads[t][i]
            p.grad = None if g is None else (g.to(DEV) if grad_of is None else grad_of(t, i, g.to(DEV)))
        opt.step()
    torch.cuda.synchronize()
    return opt, ps, [_snap(opt, p) for p in ps]


@pytest.mark.parametrize("cls", OO.CLASSES)
def test_alone_or_among_300_tensors_same_bits(cls):
    shapes = _mixed_shapes()
    params, grads = _problem(shapes, seed=61)
    _, _, many = _run(cls, params, grads)
    for j in (0, 1, 2, 3, 150, 297, 299):
        _, _, (one,) = _run(cls, [params[j]], [[g[j]] for g in grads])
        _assert_same_bits(one, many[j], f"{cls}: tensor {j} {shapes[j]} alone vs among 300")


@pytest.mark.parametrize("cls", [c for c in OO.CLASSES if c not in OO.PROJECTION])
def test_a_row_alone_or_inside_a_tensor_same_bits(cls):
    """Not for AdamP / SGDP: their projection decides per whole tensor, so a row's result depends on its neighbours."""
    J, L = 5, 1091
    (x,), grads = _problem([(J, L, 1, 1)], seed=62)   # four dimensions: SGD_GCC and gc_conv_only centralize it too
    _, _, (whole,) = _run(cls, [x], grads)
    _, _, rows = _run(cls, [x[j:j + 1] for j in range(J)], [[g[0][j:j + 1] for j in range(J)] for g in grads])
    for key in whole:
        if torch.is_tensor(whole[key]):
            got = torch.cat([r[key] for r in rows])
            assert int((got != whole[key]).sum()) == 0, f"{cls}: {key} of [{J},{L},1,1] vs {J} x [1,{L},1,1]"


_RUN_SHAPES = [(9, 1091), (5000,), (4, 3, 2, 2), (3, 193), (1,), (64, 1, 1), (6, 7), (4097,)]


@pytest.mark.parametrize("cls", OO.CLASSES)
def test_two_identical_runs_same_bits_and_a_skipped_tensor_is_untouched(cls):
    params, grads = _problem(_RUN_SHAPES, seed=63)
    absent = (0, 1, 4)
    for t in absent:
        grads[t][3] = None
    _, _, a = _run(cls, params, grads)
    _, _, b = _run(cls, params, grads)
    for i, s in enumerate(_RUN_SHAPES):
        _assert_same_bits(a[i], b[i], f"{cls}: two runs, tensor {i} {s}")
    # step by step: the tensor without a gradient keeps its bits and its state
    ps = _dev_params(params)
    opt = _make(cls, ps)
    for t in range(PROP_STEPS):
        for i, p in enumerate(ps):
            p.grad = None if grads[t][i] is None else grads[t][i].to(DEV)
        before = _snap(opt, ps[3])
        opt.step()
        if t in absent:
            _assert_same_bits(_snap(opt, ps[3]), before, f"{cls}: skipped at step {t + 1}")
    if "step" in OO.SCALAR_STATE[cls]:
        assert [opt.state[p]["step"] for p in ps] == [PROP_STEPS if i != 3 else PROP_STEPS - len(absent) for i in range(len(ps))]
    # the neighbours do not notice (MADGRAD: its own counter k advances with the optimizer's steps, as in the reference)
    others = [i for i in range(len(params)) if i != 3]
    _, _, o = _run(cls, [params[i] for i in others], [[g[i] for i in others] for g in grads])
    for j, i in enumerate(others):
        _assert_same_bits(a[i], o[j], f"{cls}: neighbour {i} of the skipped tensor")


@pytest.mark.parametrize("cls", OO.CLASSES)
def test_resume_from_state_dict_continues_bit_equal(cls):
    params, grads = _problem(_RUN_SHAPES, seed=64)
    _, _, full = _run(cls, params, grads)
    opt, ps, _ = _run(cls, params, grads, steps=4)
    sd = copy.deepcopy(opt.state_dict())
    ps2 = _dev_params([p.detach().cpu() for p in ps])
    del opt
    opt2 = _make(cls, ps2)
    opt2.load_state_dict(sd)
    _, _, resumed = _run(cls, None, grads, opt_ps=(opt2, ps2), first=4)
    for i, s in enumerate(_RUN_SHAPES):
        _assert_same_bits(resumed[i], full[i], f"{cls}: resumed after step 4, {s}")


@pytest.mark.parametrize("cls", OO.CLASSES)
def test_clean_grads_equals_nan_to_num_on_the_host(cls):
    shapes = [(9, 1091), (5000,), (3, 193)]
    params, grads = _problem(shapes, seed=65)
    limit = 7.5
    for t, i, idx, val in ((0, 0, (4, 1000), "inf"), (2, 0, (8, 1090), "-inf"), (3, 1, (4096,), "inf"), (3, 1, (4999,), "nan"),
                           (5, 2, (0, 0), "-inf"), (5, 2, (2, 192), "nan"), (6, 0, (0, 0), "nan")):
        grads[t][i][idx] = float(val)
    cleaned = [[torch.nan_to_num(g, nan=0.0, posinf=limit, neginf=-limit) for g in gs] for gs in grads]
    _, _, a = _run(cls, params, grads, clean_grads=True, grad_limit=limit)
    _, _, b = _run(cls, params, cleaned, clean_grads=False)
    _, _, c = _run(cls, params, cleaned, clean_grads=True, grad_limit=limit)
    for i, s in enumerate(shapes):
        assert torch.isfinite(a[i]["p"].view(torch.float32)).all()
        _assert_same_bits(a[i], b[i], f"{cls}: grad_limit={limit} in the kernel vs nan_to_num on the host, {s}")
        _assert_same_bits(c[i], b[i], f"{cls}: clean_grads on finite gradients, {s}")


def test_unknown_kind_and_bad_sizes_return_the_library_status_codes():
    import ctypes

    from catre_amd import hip

    lib = hip.load()
    buf = torch.zeros(64, device=DEV)
    args = lambda kind, n, ws_bytes: (kind, hip.ptr(buf), n, hip.ptr(buf), 1, hip.ptr(buf), 0, 0, hip.ptr(buf), ws_bytes, 0, 1e5,
                                      hip.stream_ptr(DEV))
    unsupported, bad = lib.catre_op_optim_step(*args(7, 1, 256)), lib.catre_op_optim_step(*args(0, 1, 8))
    assert lib.catre_status_string(unsupported) == b"unsupported configuration" and unsupported != 0
    assert bad not in (0, unsupported) and lib.catre_op_optim_step(*args(0, 0, 256)) == bad
    assert lib.catre_op_optim_step(0, ctypes.c_void_p(0), 1, hip.ptr(buf), 1, hip.ptr(buf), 0, 0, hip.ptr(buf), 256, 0, 1e5,
                                   hip.stream_ptr(DEV)) == bad


# --------------------------------------------------------------------------------------------- (d) through the model
def _model_setup(typ, B=2, N=64, M=64, **okw):
    from catre_amd import synth
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg
    from oracle.catre_oracle import y_axis_symmetries

    cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=1, device=DEV)
    cfg.SOLVER.OPTIMIZER_CFG = dict(dict(type=typ, lr=1e-4), **okw)
    model, opt = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()})
    model.train()
    raw = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=33).items()}
    b = dict(raw)
    batch_updater_test(cfg, b)
    sym = [y_axis_symmetries(12) if i % 2 == 0 else None for i in range(B)]
    return cfg, model, opt, raw, b, sym


def _forward(model, b, sym, cur_iter=1):
    return model(b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
                 obj_class=b.get("obj_cls"), gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"],
                 obj_kps=b["obj_kps"], mean_scales=b["obj_mean_scales"], sym_info=sym, do_loss=True, cur_iter=cur_iter)


def _check_trained_model(cfg, model, opt, raw, before, used):
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    assert type(opt).__name__ == cfg.SOLVER.OPTIMIZER_CFG["type"] and len(used) >= 60
    for k, p in model.named_parameters():
        assert torch.isfinite(p).all(), k
        if k in used:
            assert not torch.equal(p.detach(), before[k]), f"{k} has a gradient but did not move"
        else:
            assert torch.equal(p.detach(), before[k]), f"{k} has no gradient but moved"
    # the kernels wrote the parameters behind torch's back: the packed-weight caches must have noticed (bump_param_epoch)
    model.eval()
    with torch.no_grad():
        got = model.refine(dict(raw), n_iter=1)
        fresh, _ = build_model_optimizer(cfg, is_test=True)
        fresh.load_state_dict(copy.deepcopy(model.state_dict()))
        want = fresh.eval().refine(dict(raw), n_iter=1)
    for key in ("pose_1", "scale_1"):
        assert torch.equal(got[key], want[key]), f"{key}: the stepped model refines with stale packed weights"


@pytest.mark.parametrize("typ", OO.CLASSES)
def test_two_training_iterations_through_the_model(typ):
    okw = dict(lr=0.1) if typ in ("SGDP", "SGD_GC", "SGD_GCC") else {}   # unnormalized steps: large enough to move fp32 bits
    cfg, model, opt, raw, b, sym = _model_setup(typ, **okw)
    with torch.no_grad():
        model.eval().refine(dict(raw), n_iter=1)   # fills the packed-weight caches with the initial weights
    model.train()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    used = set()
    for it in range(2):
        _, loss_dict = _forward(model, b, sym)
        sum(loss_dict.values()).backward()
        used |= {k for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        opt.zero_grad(set_to_none=True)
    _check_trained_model(cfg, model, opt, raw, before, used)


def test_reference_amp_branch_with_clean_grads():
    """engine.py:304,333-347 as written (``autocast`` + ``GradScaler``) on a fused AdamP built with ``clean_grads=True``."""
    from torch.cuda.amp import GradScaler, autocast

    cfg, model, opt, raw, b, sym = _model_setup("AdamP", clean_grads=True, weight_decay=1e-2)
    assert opt.clean_grads is True
    with torch.no_grad():
        model.eval().refine(dict(raw), n_iter=1)
    model.train()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    grad_scaler = GradScaler()
    used = set()
    for it in range(2):
        with autocast(enabled=True):
            _, loss_dict = _forward(model, b, sym)
            losses = sum(loss_dict.values())
        grad_scaler.scale(losses).backward()
        used |= {k for k, p in model.named_parameters() if p.grad is not None}
        grad_scaler.step(opt)
        grad_scaler.update()
        opt.zero_grad(set_to_none=True)
    assert grad_scaler.get_scale() == 65536.0, "no step may have been skipped"
    assert all(opt.state[p]["step"] == 2 for g in opt.param_groups for p in g["params"] if p in opt.state)
    _check_trained_model(cfg, model, opt, raw, before, used)


# --------------------------------------------------------------------------------------------- (e) no host sync
@pytest.mark.parametrize("cls", OO.CLASSES)
def test_steps_after_the_first_do_not_synchronize(cls):
    """``torch.cuda.set_sync_debug_mode("error")`` makes torch raise on every synchronizing call it issues itself (``.item()``,
    ``.cpu()``, blocking copies, ``nonzero`` ...).  The first step is outside: it allocates state and builds the layout
    (a blocking upload of the chunk tables, once).  The library's own calls are launches and one asynchronous copy."""
    params, grads = _problem(_RUN_SHAPES, seed=66)
    ps = _dev_params(params)
    opt = _make(cls, ps)
    dev_grads = [[g.to(DEV) for g in gs] for gs in grads]
    for i, p in enumerate(ps):
        p.grad = dev_grads[0][i]
    opt.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):   # the mode works on this build: a synchronizing call raises
            ps[0].detach().sum().item()
        for t in range(1, PROP_STEPS):
            for i, p in enumerate(ps):
                p.grad = dev_grads[t][i]
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _, _, want = _run(cls, params, grads)
    for i, s in enumerate(_RUN_SHAPES):
        _assert_same_bits(_snap(opt, ps[i]), want[i], f"{cls}: {s} stepped under sync_debug_mode('error')")
