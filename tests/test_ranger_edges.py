"""The fused Ranger step (k_ranger_rowmean + k_ranger_update, catre_amd/ranger.py) at its tiling edges and under every
option the reference class has.

(a) every variant of tests/golden/ranger_options.npz (the reference class's own recorded runs) through the fused class;
(b) chunk / trip / row-length edges against the oracle in fp64 with fp32 storage.  The bound is MULT times the worst
    deviation of the SAME oracle run in fp32 on the CPU from that fp64 run (floored at one fp32 ulp of the largest
    reference value) - never anything the fused step produced;
(c) properties that hold bit for bit because each element's arithmetic does not depend on where the element sits.

Measured on an MI355X, (b): worst |kernel - fp64| / max(|fp32 oracle - fp64|, 1 ulp) per case, for p / exp_avg / exp_avg_sq:
    1d_1 0.75/1.00/0.59   1d_255 1.00/0.64/0.87   1d_256 1.00/1.00/0.82   1d_257 1.00/0.91/0.87
    1d_1023 1.00/0.89/1.00   1d_1024 1.33/1.18/0.98   1d_1025 1.00/0.84/0.68   1d_4095 1.00/0.73/0.69
    1d_4096 1.00/0.72/0.87   1d_4097 1.00/0.74/0.78   1d_8193 1.00/0.75/0.72   5x63 1.00/0.89/0.85
    5x64 1.00/0.78/0.88   5x65 1.00/1.16/0.97   3x191 1.00/0.75/0.74   3x192 1.00/0.89/1.20
    3x193 1.00/0.85/0.71   3x256 1.00/0.82/0.77   3x257 1.00/0.60/0.74   3x449 1.00/0.63/0.71
    9x1091 1.00/0.87/0.86   3x4097 1.00/0.80/0.76   64x1x1 0.00/0.00/0.00   1024x512x1 1.00/0.67/0.79
    4x3x2x2_conv_only 1.00/0.77/0.74   4x3x2x2_conv_and_fc 1.00/0.49/0.96   mixed_300 1.00/0.82/0.85
The worst is 1.33 (1d_1024, parameters: 4 ulps of the largest parameter against the fp32 oracle's 3); 64x1x1 is exact on both
sides.  MULT = 2: the kernel is one more fp32 evaluation of the same formulas, rounded in another sequence than torch's
(contracted multiply-adds, a wave-tree row sum), so it may stray about as far from fp64 as the fp32 oracle does and no further.
"""
import copy

import numpy as np
import pytest
import torch

from oracle.make_golden import RANGER_STEPS, RANGER_VARIANTS, ranger_problem, ranger_variant_groups
from oracle.ranger_oracle import clean_grad, ranger_step
from tests.util import assert_close_same_nonfinite, ranger_options_golden

pytestmark = pytest.mark.gpu

STEPS = 13   # five non-adaptive steps, the switch to the adaptive branch at 6, lookahead merges at 6 and 12
LR = 2e-2
MULT = 2.0   # see the module docstring


def _ranger(*a, **k):
    from catre_amd.ranger import Ranger

    return Ranger(*a, **k)


def _problem(shapes, seed, steps=STEPS):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(steps)]
    return params, grads


def _dev_params(params):
    return [torch.nn.Parameter(p.clone().cuda()) for p in params]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().reshape(-1)


def _snap(opt, p):
    """Bits of the parameter and its whole optimizer state."""
    st = opt.state[p]
    return dict(p=_bits(p), exp_avg=_bits(st["exp_avg"]), exp_avg_sq=_bits(st["exp_avg_sq"]), slow=_bits(st["slow_buffer"]),
                step=st["step"])


def _assert_same_bits(a, b, msg):
    assert a["step"] == b["step"], f"{msg}: step {a['step']} != {b['step']}"
    for key in ("p", "exp_avg", "exp_avg_sq", "slow"):
        n = int((a[key] != b[key]).sum())
        assert n == 0, f"{msg}: {key} differs in {n} of {a[key].numel()} elements"


def _cat(snaps):
    assert len({s["step"] for s in snaps}) == 1
    return dict({k: torch.cat([s[k] for s in snaps]) for k in ("p", "exp_avg", "exp_avg_sq", "slow")}, step=snaps[0]["step"])


def _run(ps, grads, make_opt, steps=STEPS, grad_of=None):
    """Step ``make_opt(ps)`` with grads[t][i] on the device (``grad_of(t, i, g)`` may replace or drop one); snapshots."""
    opt = make_opt(ps)
    for t in range(steps):
        for i, p in enumerate(ps):
            g = grads[t][i].cuda()
            p.grad = g if grad_of is None else grad_of(t, i, g)
        opt.step()
    torch.cuda.synchronize()
    return opt, [_snap(opt, p) for p in ps]


# --------------------------------------------------------------------------------------------- (a) reference options
@pytest.mark.parametrize("name", list(RANGER_VARIANTS))
def test_fused_options_match_reference_class(name):
    z, var = ranger_options_golden(), RANGER_VARIANTS[name]
    params, grads = ranger_problem()
    ps = _dev_params(params)
    clean = var.get("clean", True)
    opt = _ranger(ranger_variant_groups(ps, var), lr=1e-2, clean_grads=clean, **var["ctor"])
    for t in range(RANGER_STEPS):
        for i, p in enumerate(ps):
            # NaN / inf left in: cleaned inside the fused step, or (no_clean) propagated like the reference does
            p.grad = None if t in var.get("none", {}).get(i, ()) else grads[t][i].clone().cuda()
        opt.step()
        for i, p in enumerate(ps):
            assert_close_same_nonfinite(p.detach().cpu().numpy(), z[f"{name}/p{i}_step{t + 1}"], 2e-6, 2e-9,
                                        f"{name} p{i} step {t + 1}")
    for i, p in enumerate(ps):
        st = opt.state[p]
        assert st["step"] == int(z[f"{name}/step{i}"]) and set(st) == {"step", "exp_avg", "exp_avg_sq", "slow_buffer"}
        assert_close_same_nonfinite(st["exp_avg"].cpu().numpy(), z[f"{name}/exp_avg{i}"], 3e-5, 1e-6, f"{name} exp_avg{i}")
        assert_close_same_nonfinite(st["exp_avg_sq"].cpu().numpy(), z[f"{name}/exp_avg_sq{i}"], 3e-6, 1e-12, f"{name} exp_avg_sq{i}")
        assert_close_same_nonfinite(st["slow_buffer"].cpu().numpy(), z[f"{name}/slow{i}"], 2e-6, 2e-9, f"{name} slow{i}")


# --------------------------------------------------------------------------------------------- (b) tiling edges
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


def _case(shape, **ctor):
    # two tensors of the shape, one per group (the second group has weight decay)
    return dict(shapes=[shape, shape], ctor=ctor)


EDGE_CASES = {f"1d_{n}": _case((n,)) for n in (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)}
EDGE_CASES.update({"x".join(map(str, s)): _case(s) for s in (
    (5, 63), (5, 64), (5, 65), (3, 191), (3, 192), (3, 193), (3, 256), (3, 257), (3, 449),
    (9, 1091),      # chunk boundaries fall mid-row
    (3, 4097),      # a row longer than a chunk
    (64, 1, 1),     # row_len 1: every centralized gradient is exactly 0
    (1024, 512, 1),  # model-sized, once
)})
# (6, 7) rides along: centralized with gc_conv_only=False, not with True
EDGE_CASES["4x3x2x2_conv_only"] = dict(shapes=[(4, 3, 2, 2), (6, 7), (6, 7), (4, 3, 2, 2)], ctor=dict(gc_conv_only=True))
EDGE_CASES["4x3x2x2_conv_and_fc"] = dict(shapes=[(4, 3, 2, 2), (6, 7), (6, 7), (4, 3, 2, 2)], ctor=dict(gc_conv_only=False))
EDGE_CASES["mixed_300"] = dict(shapes=_mixed_shapes(), ctor={})
_WD = (0.0, 0.1)   # tensor i goes to group i % 2


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_fused_tiling_edges_match_fp64_oracle(name):
    case = EDGE_CASES[name]
    shapes = case["shapes"]
    params, grads = _problem(shapes, seed=1000 + list(EDGE_CASES).index(name))
    gc_threshold = 3 if case["ctor"].get("gc_conv_only", False) else 1
    ps = _dev_params(params)
    opt = _ranger([dict(params=ps[j::2], lr=LR, weight_decay=_WD[j]) for j in (0, 1)], lr=1e-3, **case["ctor"])
    p64, p32 = [p.double() for p in params], [p.clone() for p in params]
    s64, s32 = [dict() for _ in params], [dict() for _ in params]
    kern, yard, top = dict(p=0.0, exp_avg=0.0, exp_avg_sq=0.0), dict(p=0.0, exp_avg=0.0, exp_avg_sq=0.0), dict(p=0.0, exp_avg=0.0, exp_avg_sq=0.0)

    def track(key, got, ref32, ref64):
        kern[key] = max(kern[key], float((got.double() - ref64).abs().max()))
        yard[key] = max(yard[key], float((ref32.double() - ref64).abs().max()))
        top[key] = max(top[key], float(ref64.abs().max()))

    for t in range(STEPS):
        for i, p in enumerate(ps):
            p.grad = grads[t][i].cuda()
        opt.step()
        for i in range(len(shapes)):
            kw = dict(weight_decay=_WD[i % 2], gc_threshold=gc_threshold)
            p64[i] = ranger_step(p64[i], grads[t][i].double(), s64[i], LR, storage=torch.float32, **kw)
            p32[i] = ranger_step(p32[i], grads[t][i], s32[i], LR, storage=torch.float32, **kw)
            track("p", ps[i].detach().cpu(), p32[i], p64[i])
    for i, p in enumerate(ps):
        st = opt.state[p]
        assert st["step"] == STEPS
        for key in ("exp_avg", "exp_avg_sq"):
            track(key, st[key].cpu(), s32[i][key], s64[i][key])
        # the slow weights were merged at step 12 from the checked parameters; compare them like the parameters
        track("p", st["slow_buffer"].cpu(), s32[i]["slow_buffer"], s64[i]["slow_buffer"])
    bound, ratio = {}, {}
    for key in kern:
        ulp = float(np.spacing(np.float32(top[key])))
        bound[key] = max(yard[key], ulp)
        ratio[key] = kern[key] / bound[key]
    print(f"RANGER_EDGE {name}: " + "  ".join(
        f"{key}: kernel {kern[key]:.3e} fp32-oracle {yard[key]:.3e} ratio {ratio[key]:.2f}" for key in kern))
    for key in kern:
        assert kern[key] <= MULT * bound[key], (
            f"{name} {key}: |kernel - fp64| {kern[key]:.3e} > {MULT} x {bound[key]:.3e} (fp32 oracle's own deviation)")


# --------------------------------------------------------------------------------------------- (c) exact properties
def _two_groups(ps, first, **ctor):
    """Parameters whose index is in ``first`` form a plain group, the rest one with weight decay, another lr and k."""
    a = [p for i, p in enumerate(ps) if i in first]
    b = [p for i, p in enumerate(ps) if i not in first]
    return _ranger([dict(params=a, lr=LR), dict(params=b, lr=5e-3, weight_decay=0.1, k=4)], lr=1e-3, **ctor)


def test_split_1d_tensor_same_bits():
    (x,), grads = _problem([(10000,)], seed=51)
    cuts = [(8192, 10000), (0, 4096), (4096, 8192)]   # another parameter order than the data's
    whole = _dev_params([x])
    parts = _dev_params([x[a:b] for a, b in cuts])
    mk = lambda ps: _ranger(ps, lr=LR, weight_decay=0.1)
    _, (sw,) = _run(whole, grads, mk)
    _, sp = _run(parts, [[g[0][a:b] for a, b in cuts] for g in grads], mk)
    _assert_same_bits(_cat([sp[1], sp[2], sp[0]]), sw, "10000 = 4096 + 4096 + 1808")


def test_rows_as_one_tensor_or_many_same_bits():
    J, L = 9, 1091
    (x,), grads = _problem([(J, L)], seed=52)
    mk = lambda ps: _ranger(ps, lr=LR, weight_decay=0.1)
    _, (s2d,) = _run(_dev_params([x]), grads, mk)
    rows = _dev_params([x[j:j + 1] for j in range(J)])
    _, srows = _run(rows, [[g[0][j:j + 1] for j in range(J)] for g in grads], mk)
    _assert_same_bits(_cat(srows), s2d, f"[{J},{L}] vs {J} x [1,{L}]")
    for a, b in ((L, 1), (1, L)):   # 1091 is prime
        _, (s3d,) = _run(_dev_params([x.reshape(J, a, b)]), [[g[0].reshape(J, a, b)] for g in grads], mk)
        _assert_same_bits(s3d, s2d, f"[{J},{L}] vs [{J},{a},{b}]")


_PERM_SHAPES = [(9, 1091), (5000,), (4, 3, 2, 2), (3, 193), (1,), (64, 1, 1), (6, 7), (4097,)]


def test_parameter_and_group_order_changes_no_bits():
    params, grads = _problem(_PERM_SHAPES, seed=53)
    first = {0, 2, 4, 5}
    _, base = _run(_dev_params(params), grads, lambda ps: _two_groups(ps, first))

    def permuted(ps):
        a = [ps[i] for i in (5, 0, 4, 2)]
        b = [ps[i] for i in (7, 3, 6, 1)]
        return _ranger([dict(params=b, lr=5e-3, weight_decay=0.1, k=4), dict(params=a, lr=LR)], lr=1e-3)

    _, perm = _run(_dev_params(params), grads, permuted)
    for i, s in enumerate(_PERM_SHAPES):
        _assert_same_bits(perm[i], base[i], f"tensor {i} {s} after permuting parameters and groups")


def test_grad_none_skips_the_tensor_and_keeps_its_own_step_count():
    shapes = [(9, 1091), (7, 300), (5000,)]
    params, grads = _problem(shapes, seed=54)
    absent = (0, 1, 2, 8)
    mk = lambda ps: _ranger([dict(params=ps[:1], lr=LR), dict(params=ps[1:], lr=5e-3, weight_decay=0.1)], lr=1e-3)
    ps = _dev_params(params)
    opt = mk(ps)
    for t in range(STEPS):
        for i, p in enumerate(ps):
            p.grad = None if (i == 1 and t in absent) else grads[t][i].cuda()
        before = _snap(opt, ps[1]) if opt.state[ps[1]] else _bits(ps[1])
        opt.step()
        if t in absent:
            if opt.state[ps[1]]:
                _assert_same_bits(_snap(opt, ps[1]), before, f"skipped at step {t + 1}")
            else:   # never stepped yet: no state, untouched bits
                assert t < 3 and torch.equal(_bits(ps[1]), before)
    assert [opt.state[p]["step"] for p in ps] == [STEPS, STEPS - len(absent), STEPS]
    got = [_snap(opt, p) for p in ps]
    # its neighbours do not notice
    others = _dev_params([params[0], params[2]])
    _, so = _run(others, [[g[0], g[2]] for g in grads],
                 lambda q: _ranger([dict(params=q[:1], lr=LR), dict(params=q[1:], lr=5e-3, weight_decay=0.1)], lr=1e-3))
    _assert_same_bits(got[0], so[0], "neighbour before the skipped tensor")
    _assert_same_bits(got[2], so[1], "neighbour after the skipped tensor")
    # its own step count decides rectification (adaptive from ITS 6th step) and its lookahead merge (ITS 6th step)
    present = [t for t in range(STEPS) if t not in absent]
    _, (alone,) = _run(_dev_params([params[1]]), [[grads[t][1]] for t in present],
                       lambda q: _ranger(q, lr=5e-3, weight_decay=0.1), steps=len(present))
    _assert_same_bits(got[1], alone, "tensor with missing gradients vs the same tensor stepped alone")


def test_noncontiguous_gradient_same_bits_as_its_contiguous_copy():
    shapes = [(37, 53), (5, 1091), (300,)]
    params, _ = _problem(shapes, seed=55, steps=0)
    gen = torch.Generator().manual_seed(56)
    raw = [[torch.randn(53, 37, generator=gen), torch.randn(1, 1091, generator=gen), torch.randn(600, generator=gen)]
           for _ in range(STEPS)]

    def view(t, i, contiguous):
        r = raw[t][i].cuda()
        g = r.t() if i == 0 else r.expand(5, 1091) if i == 1 else r[::2]   # transposed, expanded (stride 0), strided
        assert not g.is_contiguous()
        return g.contiguous() if contiguous else g

    mk = lambda ps: _two_groups(ps, {0})
    _, a = _run(_dev_params(params), raw, mk, grad_of=lambda t, i, g: view(t, i, False))
    _, b = _run(_dev_params(params), raw, mk, grad_of=lambda t, i, g: view(t, i, True))
    for i, s in enumerate(shapes):
        _assert_same_bits(a[i], b[i], f"non-contiguous gradient of {s}")


def test_clean_grads_on_finite_gradients_changes_no_bits():
    params, grads = _problem(_PERM_SHAPES, seed=57)
    _, a = _run(_dev_params(params), grads, lambda ps: _two_groups(ps, {0, 1}, clean_grads=True))
    _, b = _run(_dev_params(params), grads, lambda ps: _two_groups(ps, {0, 1}, clean_grads=False))
    for i, s in enumerate(_PERM_SHAPES):
        _assert_same_bits(a[i], b[i], f"clean_grads on finite gradients, {s}")


def test_grad_limit_equals_clamping_on_the_host():
    shapes = [(9, 1091), (5000,), (3, 193)]
    params, grads = _problem(shapes, seed=58)
    limit = 7.5
    for t, i, idx, val in ((0, 0, (4, 1000), "inf"), (2, 0, (8, 1090), "-inf"), (3, 1, (4096,), "inf"), (3, 1, (4999,), "nan"),
                           (7, 2, (0, 0), "-inf"), (7, 2, (2, 192), "nan"), (11, 0, (0, 0), "nan")):
        grads[t][i][idx] = float(val)
    _, a = _run(_dev_params(params), grads, lambda ps: _two_groups(ps, {0}, clean_grads=True, grad_limit=limit))
    _, b = _run(_dev_params(params), [[clean_grad(g, limit) for g in gs] for gs in grads],
                lambda ps: _two_groups(ps, {0}, clean_grads=False))
    for i, s in enumerate(shapes):
        assert torch.isfinite(a[i]["p"].view(torch.float32)).all()
        _assert_same_bits(a[i], b[i], f"grad_limit={limit} in the kernel vs nan_to_num on the host, {s}")


def test_resume_from_state_dict_continues_bit_equal():
    shapes = [(9, 1091), (5000,), (4, 3, 2, 2), (3, 193)]
    params, grads = _problem(shapes, seed=59)
    mk = lambda ps: _two_groups(ps, {0, 2}, alpha=0.8)
    _, full = _run(_dev_params(params), grads, mk)
    ps = _dev_params(params)
    opt, _ = _run(ps, grads, mk, steps=7)
    sd = copy.deepcopy(opt.state_dict())
    ps2 = _dev_params([p.detach().cpu() for p in ps])
    del opt
    opt2 = mk(ps2)
    opt2.load_state_dict(sd)
    assert [opt2.state[p]["step"] for p in ps2] == [7] * len(ps2)
    for t in range(7, STEPS):
        for i, p in enumerate(ps2):
            p.grad = grads[t][i].cuda()
        opt2.step()
    torch.cuda.synchronize()
    for i, s in enumerate(shapes):
        _assert_same_bits(_snap(opt2, ps2[i]), full[i], f"resumed after step 7, {s}")
