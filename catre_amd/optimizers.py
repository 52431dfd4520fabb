"""The reference's other optimizers (``core/utils/solver_utils.py:28-87``, classes under ``lib/torch_utils/solver/``) as
fused multi-tensor HIP steps: ``AdaBelief``, ``RangerAdaBelief``, ``MADGRAD``, ``NAdamW``, ``AdamP``, ``SGDP``, ``SGD_GC``,
``SGD_GCC``.

Each class keeps the reference class's name, constructor signature, defaults, argument validation, ``param_groups`` keys
and per-parameter ``state`` keys, so an optimizer ``state_dict`` written by either side loads into the other and the run
continues the same way - quirks included (each class's docstring names the ones that are observable in the state).
The update of all parameter tensors is one ``catre_op_optim_step`` call: up to five small reduction launches and one
elementwise launch instead of a Python loop of 10-25 tiny torch ops per tensor, K times per data batch.

Like :class:`catre_amd.ranger.Ranger` every class takes ``clean_grads=False, grad_limit=1e5`` (the train loop's
``nan_to_num(grad, nan=0, posinf=1e5, neginf=-1e5)`` folded into the first read of the gradient), computes every scalar
term on the host in double exactly as the reference does, and runs everything per element in fp32 on the device.
``step()`` is stream-ordered on the current stream: no device-to-host copy, no synchronisation.  Two things differ from
the reference on purpose: ``p.grad`` is left as it was (the reference classes add weight decay / centralize it in place;
the loop zeroes it right after, ``engine.py:355``), and sparse gradients always raise.
"""
import math

import numpy as np
import torch
from torch.optim.optimizer import Optimizer, required

from . import hip

_CHUNK = 4096
_REC = np.dtype([("p", "<u8"), ("g", "<u8"), ("s", "<u8", (4,)), ("numel", "<i4"), ("row_len", "<i4"), ("row_off", "<i4"),
                 ("flags", "<i4"), ("f", "<f4", (12,))])
assert _REC.itemsize == 112

# enum catre_optim_kind / OPT_F_* of catre_amd/csrc/catre_optim.h
K_ADABELIEF, K_RANGER_ADABELIEF, K_MADGRAD, K_NADAMW, K_ADAMP, K_SGDP, K_SGD_GC = range(7)
F_ADAPT, F_AMS, F_PMUL, F_WDGRAD, F_BELIEF, F_WDDEC, F_GC_IN, F_GC_OUT, F_LOOK, F_MOM, F_FIRST, F_NEST, F_PROJ = (
    1 << i for i in range(13))
_NEEDS_INPUT_REDUCTIONS = F_GC_IN | F_PROJ
_NEEDS_DIRECTION_REDUCTIONS = F_GC_OUT | F_PROJ


class FusedOptimizer(Optimizer):
    """Host half shared by the fused classes (it follows ``Ranger.prepare_step`` / ``launch_step``): a layout cache keyed
    on the (address, numel, row length) tuple, a pinned record table in two alternating slots that is uploaded
    asynchronously, gradients copied to contiguous when needed and kept alive past the launch."""

    _KIND = None             # enum catre_optim_kind
    _SPARSE_MESSAGE = None   # the reference class's message, where it has one
    _CALLS_CLOSURE = True

    def _init_fused(self, clean_grads, grad_limit):
        self.clean_grads = bool(clean_grads)
        self.grad_limit = float(grad_limit)
        self._layout = None
        self._pending = None

    # -------------------------------------------------------------------------------------------- subclass interface
    def _collect(self, add):
        """Walk the param groups like the reference's ``step()``: initialise and advance the state, and call
        ``add(p, g, states, row_len, flags, f)`` for every parameter that has a gradient."""
        raise NotImplementedError

    def _sparse_error(self, group):
        return RuntimeError(self._SPARSE_MESSAGE or f"{type(self).__name__} does not support sparse gradients")

    def _grad(self, p, group):
        """The gradient the kernels read (None: skip the parameter), checked like ``Ranger.prepare_step`` does."""
        g = p.grad
        if g is None:
            return None
        if g.is_sparse:
            raise self._sparse_error(group)
        if not (p.is_cuda and p.dtype is torch.float32):
            hip.require_dev_f32(p, "parameter")   # raises with the library's message
        if not g.is_contiguous():
            g = g.contiguous()
        if not (g.is_cuda and g.dtype is torch.float32):
            hip.require_dev_f32(g, "gradient")
        if not p.is_contiguous():
            raise ValueError(f"fused {type(self).__name__} needs contiguous parameters")
        return g

    # -------------------------------------------------------------------------------------------- the two halves
    def prepare_step(self):
        """Host half of a step: state initialisation, step counters, every scalar term -> the pinned record table.
        Returns False when no parameter has a gradient."""
        recs = []

        def add(p, g, states, row_len, flags, f):
            if p.numel() == 0:
                return
            for s in states:
                if not (s.is_cuda and s.dtype is torch.float32 and s.is_contiguous() and s.numel() == p.numel()):
                    hip.require_dev_f32(s, "optimizer state")
                    raise ValueError(f"fused {type(self).__name__}: optimizer state must match its parameter's size")
            recs.append((p, g, states, row_len, flags, f))

        self._collect(add)
        if not recs:
            self._pending = None
            return False
        nrec = len(recs)
        dev = recs[0][0].device
        p_ptr = [r[0].data_ptr() for r in recs]
        c_n = [r[0].numel() for r in recs]
        c_rl = [r[3] for r in recs]
        key = tuple(zip(p_ptr, c_n, c_rl))
        if self._layout is None or self._layout["key"] != key:
            chunks, row_tensor, row_off, off = [], [], [], 0
            for ti in range(nrec):
                chunks += [(ti, o) for o in range(0, c_n[ti], _CHUNK)]
                row_off.append(off)
                if c_rl[ti] > 0:
                    rows = c_n[ti] // c_rl[ti]
                    row_tensor += [ti] * rows
                    off += rows
            # two pinned slots, used alternately: the host may fill one while the asynchronous upload of the other is
            # still queued behind earlier GPU work
            hosts = [torch.empty(nrec * _REC.itemsize, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self._layout = dict(
                key=key, n_chunks=len(chunks), n_rows=len(row_tensor), row_off=row_off,
                chunks=torch.tensor(chunks, dtype=torch.int32).to(dev),
                rows=torch.tensor(row_tensor if row_tensor else [0], dtype=torch.int32).to(dev),
                ws=torch.empty(5 * len(row_tensor) + 4 * nrec, dtype=torch.float32, device=dev),
                hosts=hosts, tables=[h.numpy().view(_REC) for h in hosts], events=[None, None], slot=0,
                dev=torch.empty(nrec * _REC.itemsize, dtype=torch.uint8, device=dev),
            )
        L = self._layout
        L["slot"] ^= 1
        if L["events"][L["slot"]] is not None:
            L["events"][L["slot"]].synchronize()  # its previous upload (two steps ago) has long been consumed
        table = L["tables"][L["slot"]]
        table["p"] = p_ptr
        table["g"] = [r[1].data_ptr() for r in recs]
        table["s"] = [[s.data_ptr() for s in r[2]] + [0] * (4 - len(r[2])) for r in recs]
        table["numel"], table["row_len"], table["row_off"] = c_n, c_rl, L["row_off"]
        table["flags"] = [r[4] for r in recs]
        table["f"] = [tuple(r[5]) + (0.0,) * (12 - len(r[5])) for r in recs]   # double -> fp32, round to nearest
        any_flags = 0
        for r in recs:
            any_flags |= r[4]
        phases = (1 if any_flags & _NEEDS_INPUT_REDUCTIONS else 0) | (2 if any_flags & _NEEDS_DIRECTION_REDUCTIONS else 0)
        # the (possibly copied-to-contiguous) gradients must outlive the launch
        self._pending = dict(n=nrec, device=dev, phases=phases, keep=[r[1] for r in recs])
        return True

    def launch_step(self):
        """Device half: one asynchronous copy of the record table and the kernels, on the current stream."""
        pend, L = self._pending, self._layout
        if pend is None:
            return
        dev = pend["device"]
        with torch.cuda.device(dev):
            L["dev"].copy_(L["hosts"][L["slot"]], non_blocking=True)
            ev = L["events"][L["slot"]] or torch.cuda.Event()
            ev.record()
            L["events"][L["slot"]] = ev
            hip.check(hip.load().catre_op_optim_step(
                self._KIND, hip.ptr(L["dev"]), pend["n"], hip.ptr(L["chunks"]), L["n_chunks"], hip.ptr(L["rows"]), L["n_rows"],
                pend["phases"], hip.ptr(L["ws"]), L["ws"].numel() * 4, int(self.clean_grads), self.grad_limit,
                hip.stream_ptr(dev)), "catre_op_optim_step")
        hip.bump_param_epoch()  # the kernel wrote the parameters behind torch's back: invalidate packed-weight caches

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None and self._CALLS_CLOSURE:
            with torch.enable_grad():
                loss = closure()
        if self.prepare_step():
            self.launch_step()
        return loss


def _zeros(p):
    return torch.zeros_like(p, memory_format=torch.contiguous_format)


def _rows(p):
    return p.numel() // p.shape[0]


class AdaBelief(FusedOptimizer):
    """``lib/torch_utils/solver/AdaBelief.py:38-218``.  Kept quirks: ``eps`` is added IN PLACE to ``exp_avg_var`` (with
    ``amsgrad``: to ``max_exp_avg_var``) on every step (``:191-193``); the state carries ``rho_inf``, and ``rho_t`` under
    ``rectify``; weight decay that is not decoupled goes into the gradient."""

    _KIND = K_ADABELIEF
    _SPARSE_MESSAGE = "AdaBelief does not support sparse gradients, please consider SparseAdam instead"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, weight_decouple=False,
                 fixed_decay=False, rectify=False, clean_grads=False, grad_limit=1e5):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults)
        self.weight_decouple = weight_decouple
        self.rectify = rectify
        self.fixed_decay = fixed_decay
        self._init_fused(clean_grads, grad_limit)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)

    def reset(self):
        for group in self.param_groups:
            for p in group["params"]:
                state = self.state[p]
                state["step"] = 0
                state["exp_avg"] = _zeros(p)
                state["exp_avg_var"] = _zeros(p)
                if group["amsgrad"]:
                    state["max_exp_avg_var"] = _zeros(p)

    def _collect(self, add):
        for group in self.param_groups:
            lr, wd, eps, ams = group["lr"], group["weight_decay"], group["eps"], group["amsgrad"]
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                g = self._grad(p, group)
                if g is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["rho_inf"] = 2.0 / (1.0 - beta2) - 1.0
                    st["step"] = 0
                    st["exp_avg"] = _zeros(p)
                    st["exp_avg_var"] = _zeros(p)
                    if ams:
                        st["max_exp_avg_var"] = _zeros(p)
                st["step"] += 1
                step = st["step"]
                bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
                flags, pmul, wdg = (F_AMS if ams else 0), 1.0, 0.0
                if self.weight_decouple:
                    flags |= F_PMUL
                    pmul = 1.0 - wd if self.fixed_decay else 1.0 - lr * wd
                elif wd != 0:
                    flags |= F_WDGRAD
                    wdg = wd
                if not self.rectify:
                    size, flags = lr / bc1, flags | F_ADAPT
                else:
                    st["rho_t"] = st["rho_inf"] - 2 * step * beta2 ** step / (1.0 - beta2 ** step)
                    if st["rho_t"] > 4:
                        rho_inf, rho_t = st["rho_inf"], st["rho_t"]
                        rt = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / (rho_inf - 4.0) / (rho_inf - 2.0) / rho_t)
                        size, flags = rt * lr / bc1, flags | F_ADAPT
                    else:
                        size = lr
                states = [st["exp_avg"], st["exp_avg_var"]] + ([st["max_exp_avg_var"]] if ams else [])
                add(p, g, states, 0, flags, (beta1, 1 - beta1, beta2, 1 - beta2, eps, pmul, wdg, math.sqrt(bc2), size))


class RangerAdaBelief(FusedOptimizer):
    """``lib/torch_utils/solver/ranger_adabelief.py:52-264``.  Kept quirks: ``use_gc`` IS consulted (Ranger ignores it);
    ``gc_loc=False`` centralizes ``G_grad`` instead of the gradient; in the adaptive adabelief branch ``eps`` is added in
    place to ``exp_avg_sq`` (``:232``); outside the adaptive branch ``G_grad`` IS ``exp_avg``, so decoupled weight decay
    and the ``gc_loc=False`` centralization edit ``exp_avg`` (``:238-249``); lookahead per parameter at ``step % k == 0``.
    The closure is not called (``:138-139``).  (The reference class's ``__setstate__`` names an undefined class, so its own
    ``load_state_dict`` raises; this one loads.)"""

    _KIND = K_RANGER_ADABELIEF
    _SPARSE_MESSAGE = "Ranger optimizer does not support sparse gradients"
    _CALLS_CLOSURE = False

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0,
                 use_gc=True, gc_conv_only=False, gc_loc=True, adabelief=True, weight_decouple=True, clean_grads=False,
                 grad_limit=1e5):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not eps > 0:
            raise ValueError(f"Invalid eps: {eps}")
        defaults = dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k
        self.gc_loc = gc_loc
        self.use_gc = use_gc
        self.gc_conv_only = gc_conv_only
        self.adabelief = adabelief
        self.weight_decouple = weight_decouple
        self._init_fused(clean_grads, grad_limit)

    def _step_terms(self, step, beta1, beta2):   # :201-223
        beta2_t = beta2 ** step
        n_max = 2 / (1 - beta2) - 1
        n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
        if n_sma > self.N_sma_threshhold:
            size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (
                1 - beta1 ** step)
            return size, True
        return 1.0 / (1 - beta1 ** step), False

    def _collect(self, add):
        gc_dims = 3 if self.gc_conv_only else 1
        for group in self.param_groups:
            lr, wd, eps, k = group["lr"], group["weight_decay"], group["eps"], group["k"]
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                g = self._grad(p, group)
                if g is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = _zeros(p)
                    st["exp_avg_sq"] = _zeros(p)
                    st["slow_buffer"] = p.detach().clone(memory_format=torch.contiguous_format)
                st["step"] += 1
                step = st["step"]
                size, adaptive = self._step_terms(step, beta1, beta2)
                gc = bool(self.use_gc) and p.dim() > gc_dims
                flags = (F_ADAPT if adaptive else 0) | (F_BELIEF if self.adabelief else 0)
                if not self.weight_decouple:
                    flags |= F_WDGRAD
                elif wd != 0:
                    flags |= F_WDDEC
                if gc:
                    flags |= F_GC_IN if self.gc_loc else F_GC_OUT
                if step % k == 0:
                    flags |= F_LOOK
                add(p, g, [st["exp_avg"], st["exp_avg_sq"], st["slow_buffer"]], _rows(p) if gc else 0, flags,
                    (beta1, 1 - beta1, beta2, 1 - beta2, eps, wd, wd, size * lr, self.alpha))


class MADGRAD(FusedOptimizer):
    """``lib/torch_utils/solver/madgrad.py``.  Kept quirks: the optimizer-level ``state["k"]`` is a long tensor (kept on the
    host: reading it costs no device synchronisation) and advances on every ``step()``; the step uses ``lr + eps``;
    ``momentum == 0`` keeps no ``x0``; the cube root is ``pow(1 / 3)``."""

    _KIND = K_MADGRAD

    def __init__(self, params, lr=1e-2, momentum=0.9, weight_decay=0, eps=1e-6, clean_grads=False, grad_limit=1e5):
        if momentum < 0 or momentum >= 1:
            raise ValueError(f"Momentum {momentum} must be in the range [0,1]")
        if lr <= 0:
            raise ValueError(f"Learning rate {lr} must be positive")
        if weight_decay < 0:
            raise ValueError(f"Weight decay {weight_decay} must be non-negative")
        if eps < 0:
            raise ValueError("Eps must be non-negative")
        defaults = dict(lr=lr, eps=eps, momentum=momentum, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._init_fused(clean_grads, grad_limit)

    @property
    def supports_memory_efficient_fp16(self):
        return False

    @property
    def supports_flat_params(self):
        return True

    def _sparse_error(self, group):
        if group["momentum"] != 0.0:
            return RuntimeError("momentum != 0 is not compatible with sparse gradients")
        if group["weight_decay"] != 0:
            return RuntimeError("weight_decay option is not compatible with sparse gradients")
        return RuntimeError("fused MADGRAD does not support sparse gradients")

    def _collect(self, add):
        if "k" not in self.state:
            self.state["k"] = torch.tensor([0], dtype=torch.long)
        elif self.state["k"].is_cuda:   # a checkpoint mapped to the device: bring the counter back once
            self.state["k"] = self.state["k"].cpu()
        k = self.state["k"].item()
        for group in self.param_groups:
            eps = group["eps"]
            lr = group["lr"] + eps
            decay, momentum = group["weight_decay"], group["momentum"]
            ck = 1 - momentum
            lamb = lr * math.pow(k + 1, 0.5)
            for p in group["params"]:
                g = self._grad(p, group)
                if g is None:
                    continue
                st = self.state[p]
                if "grad_sum_sq" not in st:
                    st["grad_sum_sq"] = _zeros(p)
                    st["s"] = _zeros(p)
                    if momentum != 0:
                        st["x0"] = p.detach().clone(memory_format=torch.contiguous_format)
                flags = (F_WDGRAD if decay != 0 else 0) | (F_MOM if momentum != 0 else 0)
                states = [st["grad_sum_sq"], st["s"]] + ([st["x0"]] if momentum != 0 else [])
                add(p, g, states, 0, flags, (lamb, eps, decay, ck, 1 - ck))
        self.state["k"] += 1


class NAdamW(FusedOptimizer):
    """``lib/torch_utils/solver/nadamw.py:33-132``.  Kept quirks: weight decay is applied first; ``mu_product`` is a Python
    float in the state; ``mu_product_next`` multiplies by ``mu`` once more (``:116``)."""

    _KIND = K_NADAMW
    _SPARSE_MESSAGE = "NAdamW does not support sparse gradients, please consider SparseAdam instead"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, momentum_decay=4e-3, amsgrad=False,
                 clean_grads=False, grad_limit=1e5):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if not 0.0 <= momentum_decay:
            raise ValueError("Invalid momentum_decay value: {}".format(momentum_decay))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum_decay=momentum_decay, amsgrad=amsgrad)
        super().__init__(params, defaults)
        self._init_fused(clean_grads, grad_limit)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)

    def _collect(self, add):
        for group in self.param_groups:
            lr, wd, eps, ams, momentum_decay = (group["lr"], group["weight_decay"], group["eps"], group["amsgrad"],
                                                group["momentum_decay"])
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                g = self._grad(p, group)
                if g is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["mu_product"] = 1.0
                    st["exp_avg"] = _zeros(p)
                    st["exp_avg_sq"] = _zeros(p)
                    if ams:
                        st["max_exp_avg_sq"] = _zeros(p)
                mu_product = st["mu_product"]
                st["step"] += 1
                step = st["step"]
                bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
                mu = beta1 * (1.0 - 0.5 * (0.96 ** (step * momentum_decay)))
                mu_next = beta1 * (1.0 - 0.5 * (0.96 ** ((step + 1) * momentum_decay)))
                mu_product = mu_product * mu
                mu_product_next = mu_product * mu * mu_next
                st["mu_product"] = mu_product
                size = lr / bc1
                states = [st["exp_avg"], st["exp_avg_sq"]] + ([st["max_exp_avg_sq"]] if ams else [])
                add(p, g, states, 0, F_AMS if ams else 0,
                    (beta1, 1 - beta1, beta2, 1 - beta2, eps, 1 - lr * wd, 0.0, math.sqrt(bc2),
                     -size * (1.0 - mu) / (1.0 - mu_product), -size * mu_next / (1.0 - mu_product_next)))


def _projection_terms(p, delta):
    """(row length, delta / sqrt(channel view width), delta / sqrt(layer view width)) of ``_projection`` (adamp.py:55)."""
    rl = _rows(p)
    return rl, delta / math.sqrt(rl), delta / math.sqrt(p.numel())


class AdamP(FusedOptimizer):
    """``lib/torch_utils/solver/adamp.py:13-123``.  The projection applies only to ``p.dim() > 1``, channel view first, then
    layer view; which one fires is decided on the device with the reference's comparison
    ``cosine_sim.max() < delta / sqrt(view width)``; ``wd_ratio`` applies only when a view fires."""

    _KIND = K_ADAMP

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, delta=0.1, wd_ratio=0.1, nesterov=False,
                 clean_grads=False, grad_limit=1e5):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, delta=delta, wd_ratio=wd_ratio,
                        nesterov=nesterov)
        super().__init__(params, defaults)
        self._init_fused(clean_grads, grad_limit)

    def _collect(self, add):
        for group in self.param_groups:
            lr, wd, eps, delta, wd_ratio = group["lr"], group["weight_decay"], group["eps"], group["delta"], group["wd_ratio"]
            beta1, beta2 = group["betas"]
            base = (F_NEST if group["nesterov"] else 0) | (F_PMUL if wd > 0 else 0)
            for p in group["params"]:
                g = self._grad(p, group)
                if g is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = _zeros(p)
                    st["exp_avg_sq"] = _zeros(p)
                st["step"] += 1
                step = st["step"]
                bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
                proj = p.dim() > 1 and p.numel() > 0
                rl, thr_c, thr_l = _projection_terms(p, delta) if proj else (0, 0.0, 0.0)
                add(p, g, [st["exp_avg"], st["exp_avg_sq"]], rl, base | (F_PROJ if proj else 0),
                    (beta1, 1 - beta1, beta2, 1 - beta2, eps, 1 - lr * wd * 1, 1 - lr * wd * wd_ratio, math.sqrt(bc2), lr / bc1,
                     delta, thr_c, thr_l))


class SGDP(FusedOptimizer):
    """``lib/torch_utils/solver/sgdp.py``.  The projection of :class:`AdamP`.  Kept quirk: without ``nesterov`` ``d_p`` IS
    the momentum buffer, so the projection's in-place subtraction edits ``state["momentum"]`` (``sgdp.py:87-104``)."""

    _KIND = K_SGDP

    def __init__(self, params, lr=required, momentum=0, dampening=0, weight_decay=0, nesterov=False, eps=1e-8, delta=0.1,
                 wd_ratio=0.1, clean_grads=False, grad_limit=1e5):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, eps=eps,
                        delta=delta, wd_ratio=wd_ratio)
        super().__init__(params, defaults)
        self._init_fused(clean_grads, grad_limit)

    def _collect(self, add):
        for group in self.param_groups:
            lr, wd, eps, delta, wd_ratio = group["lr"], group["weight_decay"], group["eps"], group["delta"], group["wd_ratio"]
            momentum, dampening = group["momentum"], group["dampening"]
            base = (F_NEST if group["nesterov"] else 0) | (F_PMUL if wd > 0 else 0)
            pmul = (1 - lr * wd * 1 / (1 - momentum), 1 - lr * wd * wd_ratio / (1 - momentum)) if wd > 0 else (1.0, 1.0)
            for p in group["params"]:
                g = self._grad(p, group)
                if g is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["momentum"] = _zeros(p)
                proj = p.dim() > 1 and p.numel() > 0
                rl, thr_c, thr_l = _projection_terms(p, delta) if proj else (0, 0.0, 0.0)
                add(p, g, [st["momentum"]], rl, base | (F_PROJ if proj else 0),
                    (momentum, 1 - dampening, 0.0, 0.0, eps, pmul[0], pmul[1], 0.0, lr, delta, thr_c, thr_l))


class SGD_GC(FusedOptimizer):
    """``lib/torch_utils/solver/sgd_gc.py:95-180``: SGD with the gradient centralized for conv and fc weights
    (``dim > 1``).  Weight decay goes into the gradient first; the first step's buffer is a copy of that gradient; no state
    is kept when ``momentum == 0``."""

    _KIND = K_SGD_GC
    _GC_DIMS = 1

    def __init__(self, params, lr=required, momentum=0, dampening=0, weight_decay=0, nesterov=False, clean_grads=False,
                 grad_limit=1e5):
        if lr is not required and lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, defaults)
        self._init_fused(clean_grads, grad_limit)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("nesterov", False)

    def _collect(self, add):
        for group in self.param_groups:
            lr, wd, momentum, dampening = group["lr"], group["weight_decay"], group["momentum"], group["dampening"]
            base = (F_WDGRAD if wd != 0 else 0) | (F_NEST if group["nesterov"] else 0) | (F_MOM if momentum != 0 else 0)
            for p in group["params"]:
                g = self._grad(p, group)
                if g is None:
                    continue
                flags, states = base, []
                if momentum != 0:
                    st = self.state[p]
                    if "momentum_buffer" not in st:
                        st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)  # written below
                        flags |= F_FIRST
                    states = [st["momentum_buffer"]]
                gc = p.dim() > self._GC_DIMS
                add(p, g, states, _rows(p) if gc else 0, flags | (F_GC_IN if gc else 0),
                    (momentum, 1 - dampening, 0.0, 0.0, 0.0, 0.0, wd, 0.0, lr))


class SGD_GCC(SGD_GC):
    """``lib/torch_utils/solver/sgd_gc.py:7-92``: :class:`SGD_GC` for conv weights only (``dim > 3``)."""

    _GC_DIMS = 3


FUSED_OPTIMIZERS = {c.__name__: c for c in (AdaBelief, RangerAdaBelief, MADGRAD, NAdamW, AdamP, SGDP, SGD_GC, SGD_GCC)}
