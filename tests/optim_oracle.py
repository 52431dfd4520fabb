"""Test infrastructure (a helper, not a test file): the project's own restatement in torch of the eight optimizer steps
that ``catre_amd/optimizers.py`` fuses - ``lib/torch_utils/solver/{AdaBelief,ranger_adabelief,madgrad,nadamw,adamp,sgdp,
sgd_gc}.py`` of the reference - and the problem set of ``tests/golden/optim_steps.npz`` (``tools/make_optim_golden.py``
records that file from the reference classes themselves; the tests pin this restatement to it).

The restatement is dtype-generic.  On fp32 tensors it issues the reference's torch ops in the reference's order, so it
reproduces the reference's bits.  On fp64 tensors with ``storage=torch.float32`` the arithmetic is double and everything
the reference keeps in an fp32 tensor (parameter, state) is rounded to fp32 where it is stored, like
``oracle/ranger_oracle.py``: that run is the yardstick the fp32 runs are measured against.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

# constructor defaults of the reference classes (settings, not code)
DEFAULTS = {
    "AdaBelief": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, weight_decouple=False,
                      fixed_decay=False, rectify=False),
    "RangerAdaBelief": dict(lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0,
                            use_gc=True, gc_conv_only=False, gc_loc=True, adabelief=True, weight_decouple=True),
    "MADGRAD": dict(lr=1e-2, momentum=0.9, weight_decay=0, eps=1e-6),
    "NAdamW": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, momentum_decay=4e-3, amsgrad=False),
    "AdamP": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, delta=0.1, wd_ratio=0.1, nesterov=False),
    "SGDP": dict(momentum=0, dampening=0, weight_decay=0, nesterov=False, eps=1e-8, delta=0.1, wd_ratio=0.1),
    "SGD_GC": dict(momentum=0, dampening=0, weight_decay=0, nesterov=False),
    "SGD_GCC": dict(momentum=0, dampening=0, weight_decay=0, nesterov=False),
}
CLASSES = tuple(DEFAULTS)
PROJECTION = ("AdamP", "SGDP")
# per-parameter state that is a Python scalar
SCALAR_STATE = {
    "AdaBelief": dict(rho_inf=float, step=int, rho_t=float), "RangerAdaBelief": dict(step=int), "MADGRAD": {},
    "NAdamW": dict(step=int, mu_product=float), "AdamP": dict(step=int), "SGDP": {}, "SGD_GC": {}, "SGD_GCC": {},
}

# ------------------------------------------------------------------------------------------------ the fixture's problem
STEPS = 13            # RAdam / rectify threshold crossings at 6, lookahead merges at 6 and 12
STATE_STEPS = (6, 13)
SHAPES = [(8,), (1,), (6, 5), (8, 4, 1), (4, 3, 2, 2), (8, 24)]
STEER_SHAPES = [(8, 24), (8, 24)]          # projection classes only: channel view fires / only the layer view fires
STEER = {5: "none", 6: "channel", 7: "layer"}
GROUPS = [dict(idx=(0, 2, 4, 5), lr=2e-2), dict(idx=(1, 3, 6, 7), lr=5e-3, weight_decay=0.1)]
NONE_AT = {2: (2, 8)}   # tensor 2 has no gradient at (0-based) steps 2 and 8
VARIANTS = {
    "AdaBelief": dict(default={}, amsgrad=dict(amsgrad=True), decouple=dict(weight_decouple=True),
                      fixed_decay=dict(weight_decouple=True, fixed_decay=True, weight_decay=1e-3), rectify=dict(rectify=True)),
    "RangerAdaBelief": dict(default={}, no_gc=dict(use_gc=False), conv_only=dict(gc_conv_only=True),
                            gc_after=dict(gc_loc=False), no_belief=dict(adabelief=False),
                            coupled=dict(weight_decouple=False), gc_after_conv_only_no_belief=dict(
                                gc_loc=False, gc_conv_only=True, adabelief=False)),
    "MADGRAD": dict(default={}, no_momentum=dict(momentum=0)),
    "NAdamW": dict(default={}, amsgrad=dict(amsgrad=True)),
    "AdamP": dict(default={}, nesterov=dict(nesterov=True)),
    "SGDP": dict(default={}, momentum=dict(momentum=0.9, dampening=0.1), nesterov=dict(momentum=0.9, nesterov=True)),
    "SGD_GC": dict(default={}, momentum=dict(momentum=0.9, dampening=0.1), nesterov=dict(momentum=0.9, nesterov=True)),
    "SGD_GCC": dict(momentum=dict(momentum=0.9)),
}
PROBLEM_SEED = 47   # the first seed from 20 on that tools/make_optim_golden.py accepts


def problem_shapes(cls):
    return SHAPES + (STEER_SHAPES if cls in PROJECTION else [])


def variant_names():
    return [f"{c}/{v}" for c in CLASSES for v in VARIANTS[c]]


def make_problem(cls, seed=PROBLEM_SEED, shapes=None, steps=STEPS, steer=None):
    """Initial parameters and the seeded draws the gradients are made from (``gradient`` below)."""
    shapes = problem_shapes(cls) if shapes is None else shapes
    steer = (STEER if cls in PROJECTION else {}) if steer is None else steer
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=gen) for s in shapes]
    for i, kind in steer.items():
        if kind == "layer":
            params[i][0] *= 1e-4
    draws = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(steps)]
    return params, draws


def gradient(kind, draw, p0, p_prev):
    """The gradient of one tensor at one step.  ``kind`` None: the seeded draw, for tensors with rows plus half the initial
    parameter (so that no projection view is ever close to firing).  The steered tensors depend on ``p_prev``, the fp32
    parameter the REFERENCE run holds before the step (recorded in the fixture): "channel" makes every row orthogonal to
    the parameter's row, "layer" does so for every row but the first, which is 1e-3 times the parameter's own first row (cosine 1
    in that row; the factor, and the row's initial scale of 1e-4, keep the whole-tensor cosine tiny while the row drifts with the
    steps), "none" is the plain draw."""
    if kind is None:
        return draw + 0.5 * p0 if draw.dim() > 1 else draw.clone()
    if kind == "none":
        return draw.clone()
    d, p = draw.double(), p_prev.double()
    g = d - p * ((d * p).sum(1, keepdim=True) / (p * p).sum(1, keepdim=True))
    if kind == "layer":
        g[0] = 1e-3 * p[0]
    return g.float()


def hyper(cls, ctor, group):
    h = dict(DEFAULTS[cls])
    h.update(ctor)
    h.update({k: v for k, v in group.items() if k not in ("idx", "params")})
    return h


# ------------------------------------------------------------------------------------------------ the restatement
def _centralize(x, dims):
    return x.add(-(x.mean(dim=tuple(range(1, x.dim())), keepdim=True))) if x.dim() > dims else x


def _projection(p, g, perturb, h, ratios):
    """adamp.py:48-62 / sgdp.py:50-64 -> (perturb, wd_ratio); appends cosine_max / threshold per view tried."""
    expand = [-1] + [1] * (p.dim() - 1)
    for view in (lambda x: x.reshape(x.size(0), -1), lambda x: x.reshape(1, -1)):
        cos = F.cosine_similarity(view(g), view(p), dim=1, eps=h["eps"]).abs()
        thr = h["delta"] / math.sqrt(view(p).size(1))
        if ratios is not None:
            ratios.append(float(cos.max()) / thr)
        if cos.max() < thr:
            p_n = p / view(p).norm(dim=1).view(expand).add(h["eps"])
            perturb = perturb - p_n * view(p_n * perturb).sum(dim=1).view(expand)
            return perturb, h["wd_ratio"]
    return perturb, 1


def restated_step(cls, p, g, st, h, k_opt=0, storage=None, ratios=None):
    """One step of one tensor: returns the new parameter, creates / advances ``st`` in place.  ``h``: the hyper-parameters
    (``hyper``), ``k_opt``: MADGRAD's optimizer-level counter before the step."""
    S = (lambda t: t) if storage is None else (lambda t: t.to(storage).to(t.dtype))
    lr, wd = h["lr"], h["weight_decay"]
    Z = lambda: torch.zeros_like(p)
    if cls == "AdaBelief":
        b1, b2 = h["betas"]
        if not st:
            st.update(rho_inf=2.0 / (1.0 - b2) - 1.0, step=0, exp_avg=Z(), exp_avg_var=Z())
            if h["amsgrad"]:
                st["max_exp_avg_var"] = Z()
        st["step"] += 1
        step = st["step"]
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        if h["weight_decouple"]:
            p = S(p.mul(1.0 - wd if h["fixed_decay"] else 1.0 - lr * wd))
        elif wd != 0:
            g = g.add(p, alpha=wd)
        st["exp_avg"] = S(st["exp_avg"].mul(b1).add(g, alpha=1 - b1))
        r = g - st["exp_avg"]
        var = st["exp_avg_var"].mul(b2).addcmul(r, r, value=1 - b2)
        if h["amsgrad"]:
            st["exp_avg_var"] = S(var)
            st["max_exp_avg_var"] = S(torch.max(st["max_exp_avg_var"], st["exp_avg_var"]).add(h["eps"]))
            denom = (st["max_exp_avg_var"].sqrt() / math.sqrt(bc2)).add(h["eps"])
        else:
            st["exp_avg_var"] = S(var.add(h["eps"]))
            denom = (st["exp_avg_var"].sqrt() / math.sqrt(bc2)).add(h["eps"])
        if not h["rectify"]:
            return S(p.addcdiv(st["exp_avg"], denom, value=-(lr / bc1)))
        st["rho_t"] = st["rho_inf"] - 2 * step * b2 ** step / (1.0 - b2 ** step)
        if st["rho_t"] > 4:
            ri, rt = st["rho_inf"], st["rho_t"]
            rt = math.sqrt((rt - 4.0) * (rt - 2.0) * ri / (ri - 4.0) / (ri - 2.0) / rt)
            return S(p.addcdiv(st["exp_avg"], denom, value=-(rt * lr / bc1)))
        return S(p.add(st["exp_avg"], alpha=-lr))
    if cls == "RangerAdaBelief":
        b1, b2 = h["betas"]
        dims = 3 if h["gc_conv_only"] else 1
        if not h["weight_decouple"]:
            g = g.add(p * wd)
        if not st:
            st.update(step=0, exp_avg=Z(), exp_avg_sq=Z(), slow_buffer=p.clone())
        if h["gc_loc"] and h["use_gc"]:
            g = _centralize(g, dims)
        st["step"] += 1
        step = st["step"]
        st["exp_avg"] = S(st["exp_avg"].mul(b1).add(g, alpha=1 - b1))
        d = g - st["exp_avg"] if h["adabelief"] else g
        sq = st["exp_avg_sq"].mul(b2).addcmul(d, d, value=1 - b2)
        b2t = b2 ** step
        n_max = 2 / (1 - b2) - 1
        n_sma = n_max - 2 * step * b2t / (1 - b2t)
        adaptive = n_sma > h["N_sma_threshhold"]
        if adaptive:
            size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** step)
            if h["adabelief"]:
                sq = S(sq.add(h["eps"]))
            st["exp_avg_sq"] = S(sq)
            G = st["exp_avg"] / st["exp_avg_sq"].sqrt().add(h["eps"])
        else:
            size = 1.0 / (1 - b1 ** step)
            st["exp_avg_sq"] = S(sq)
            G = st["exp_avg"]
        if h["weight_decouple"] and wd != 0:
            G = G.add(p, alpha=wd)
        if not h["gc_loc"] and h["use_gc"]:
            G = _centralize(G, dims)
        if not adaptive:
            st["exp_avg"] = G = S(G)   # G_grad IS exp_avg here: both edits above were in place
        p = S(p.add(G, alpha=-size * lr))
        if step % h["k"] == 0:
            st["slow_buffer"] = S(st["slow_buffer"].add(p - st["slow_buffer"], alpha=h["alpha"]))
            p = st["slow_buffer"].clone()
        return p
    if cls == "MADGRAD":
        eps, momentum = h["eps"], h["momentum"]
        lr = lr + eps
        ck = 1 - momentum
        lamb = lr * math.pow(k_opt + 1, 0.5)
        if "grad_sum_sq" not in st:
            st.update(grad_sum_sq=Z(), s=Z())
            if momentum != 0:
                st["x0"] = p.clone()
        if wd != 0:
            g = g.add(p, alpha=wd)
        if momentum == 0:
            x0 = p.addcdiv(st["s"], st["grad_sum_sq"].pow(1 / 3).add(eps), value=1)
        else:
            x0 = st["x0"]
        st["grad_sum_sq"] = S(st["grad_sum_sq"].addcmul(g, g, value=lamb))
        rms = st["grad_sum_sq"].pow(1 / 3).add(eps)
        st["s"] = S(st["s"].add(g, alpha=lamb))
        z = x0.addcdiv(st["s"], rms, value=-1)
        return S(z) if momentum == 0 else S(p.mul(1 - ck).add(z, alpha=ck))
    if cls == "NAdamW":
        b1, b2 = h["betas"]
        p = S(p.mul(1 - lr * wd))
        if not st:
            st.update(step=0, mu_product=1.0, exp_avg=Z(), exp_avg_sq=Z())
            if h["amsgrad"]:
                st["max_exp_avg_sq"] = Z()
        st["step"] += 1
        step = st["step"]
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        mu = b1 * (1.0 - 0.5 * (0.96 ** (step * h["momentum_decay"])))
        mu_next = b1 * (1.0 - 0.5 * (0.96 ** ((step + 1) * h["momentum_decay"])))
        mu_product = st["mu_product"] * mu
        mu_product_next = mu_product * mu * mu_next
        st["mu_product"] = mu_product
        st["exp_avg"] = S(st["exp_avg"].mul(b1).add(g, alpha=1 - b1))
        st["exp_avg_sq"] = S(st["exp_avg_sq"].mul(b2).addcmul(g, g, value=1 - b2))
        if h["amsgrad"]:
            st["max_exp_avg_sq"] = torch.max(st["max_exp_avg_sq"], st["exp_avg_sq"])
            denom = (st["max_exp_avg_sq"].sqrt() / math.sqrt(bc2)).add(h["eps"])
        else:
            denom = (st["exp_avg_sq"].sqrt() / math.sqrt(bc2)).add(h["eps"])
        size = lr / bc1
        p = S(p.addcdiv(g, denom, value=-size * (1.0 - mu) / (1.0 - mu_product)))
        return S(p.addcdiv(st["exp_avg"], denom, value=-size * mu_next / (1.0 - mu_product_next)))
    if cls == "AdamP":
        b1, b2 = h["betas"]
        if not st:
            st.update(step=0, exp_avg=Z(), exp_avg_sq=Z())
        st["step"] += 1
        step = st["step"]
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        st["exp_avg"] = S(st["exp_avg"].mul(b1).add(g, alpha=1 - b1))
        st["exp_avg_sq"] = S(st["exp_avg_sq"].mul(b2).addcmul(g, g, value=1 - b2))
        denom = (st["exp_avg_sq"].sqrt() / math.sqrt(bc2)).add(h["eps"])
        perturb = (b1 * st["exp_avg"] + (1 - b1) * g) / denom if h["nesterov"] else st["exp_avg"] / denom
        ratio = 1
        if p.dim() > 1:
            perturb, ratio = _projection(p, g, perturb, h, ratios)
        if wd > 0:
            p = S(p.mul(1 - lr * wd * ratio))
        return S(p.add(perturb, alpha=-(lr / bc1)))
    if cls == "SGDP":
        momentum = h["momentum"]
        if not st:
            st["momentum"] = Z()
        buf = S(st["momentum"].mul(momentum).add(g, alpha=1 - h["dampening"]))
        d_p = g + momentum * buf if h["nesterov"] else buf
        ratio = 1
        if p.dim() > 1:
            d_p, ratio = _projection(p, g, d_p, h, ratios)
        st["momentum"] = buf if h["nesterov"] else S(d_p)   # without nesterov d_p IS the buffer
        d_p = d_p if h["nesterov"] else st["momentum"]
        if wd > 0:
            p = S(p.mul(1 - lr * wd * ratio / (1 - momentum)))
        return S(p.add(d_p, alpha=-lr))
    if cls in ("SGD_GC", "SGD_GCC"):
        momentum = h["momentum"]
        if wd != 0:
            g = g.add(p, alpha=wd)
        g = _centralize(g, 1 if cls == "SGD_GC" else 3)
        d_p = g
        if momentum != 0:
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = S(g.clone())
            else:
                st["momentum_buffer"] = S(st["momentum_buffer"].mul(momentum).add(g, alpha=1 - h["dampening"]))
            d_p = g.add(st["momentum_buffer"], alpha=momentum) if h["nesterov"] else st["momentum_buffer"]
        return S(p.add(d_p, alpha=-lr))
    raise ValueError(cls)


class Restated:
    """The restatement over a list of tensors: ``step(grads)`` with ``None`` for a tensor without a gradient."""

    def __init__(self, cls, params, hypers, storage=None, record_ratios=True):
        self.cls, self.params, self.hypers, self.storage = cls, list(params), hypers, storage
        self.record_ratios = record_ratios   # False: no read-back beyond the reference's own `cosine_sim.max() < ...`
        self.state = [dict() for _ in params]
        self.k = 0
        self.ratios = {}   # (tensor, step index) -> [cosine_max / threshold per view tried]

    def step(self, grads, t=None):
        for i, g in enumerate(grads):
            if g is None:
                continue
            r = [] if self.record_ratios else None
            self.params[i] = restated_step(self.cls, self.params[i], g.to(self.params[i].dtype), self.state[i], self.hypers[i],
                                           k_opt=self.k, storage=self.storage, ratios=r)
            if r:
                self.ratios[(i, t)] = r
        self.k += 1


def hypers_for(cls, ctor, n, groups=GROUPS):
    out = [None] * n
    for grp in groups:
        for i in grp["idx"]:
            if i < n:
                out[i] = hyper(cls, ctor, grp)
    return out


def ulp_of(x):
    return float(np.spacing(np.float32(x)))
