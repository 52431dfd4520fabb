"""Fixture for the fused optimizer steps (``catre_amd/optimizers.py``), recorded from the UNMODIFIED reference classes
(needs the reference tree, see ``oracle/ref_shim.py``; never needed to build, test or run the product):

    python tools/make_optim_golden.py            # tests/golden/optim_steps.npz

The problem set and the variants are those of ``tests/optim_oracle.py`` (shapes, two param groups with different ``lr`` and
``weight_decay``, one tensor without a gradient at two steps, seeded gradients).  Per variant ``<class>/<variant>``:

* ``params``: [13, sum of numel] - all parameters, flattened and concatenated in index order, after step t = 1..13;
* ``s<t>/<key>``: the whole per-parameter state after steps 6 and 13 - tensor entries concatenated like the parameters,
  Python scalars as an int64 / float64 array with one entry per parameter (every parameter of a variant has the same
  keys) - and ``s<t>/k`` for MADGRAD's optimizer-level counter;
* ``sd6_param_groups``: ``repr`` of the ``param_groups`` of the reference's ``state_dict()`` after step 6.  Its ``state`` is
  asserted here to be exactly the recorded step-6 state, keyed by parameter index, so it is not stored twice;
* ``ratios`` (AdamP / SGDP): rows of (tensor, step, view, cosine_max / threshold) for every view the projection looked at.

The projection's decisions must not depend on rounding: every ratio must lie outside [0.5, 1.5], on the side the
construction intends (asserted).  The steered tensors are built for that; the plainly random one is not, so seeds are
tried in order until the whole set passes.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import optim_oracle as OO  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "optim_steps.npz")


def reference_classes():
    if not os.path.isdir(ref_shim.REFERENCE_ROOT):
        raise RuntimeError(f"reference tree not found at {ref_shim.REFERENCE_ROOT}")
    if ref_shim.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_shim.REFERENCE_ROOT)
    from lib.torch_utils.solver.AdaBelief import AdaBelief
    from lib.torch_utils.solver.adamp import AdamP
    from lib.torch_utils.solver.madgrad import MADGRAD
    from lib.torch_utils.solver.nadamw import NAdamW
    from lib.torch_utils.solver.ranger_adabelief import RangerAdaBelief
    from lib.torch_utils.solver.sgd_gc import SGD_GC, SGD_GCC
    from lib.torch_utils.solver.sgdp import SGDP

    return dict(AdaBelief=AdaBelief, RangerAdaBelief=RangerAdaBelief, MADGRAD=MADGRAD, NAdamW=NAdamW, AdamP=AdamP, SGDP=SGDP,
                SGD_GC=SGD_GC, SGD_GCC=SGD_GCC)


def _ratios(p, g, h):
    """cosine_max / threshold of the views adamp.py:51-60 looks at (the layer view only if the channel view did not fire)."""
    out = []
    for v, view in enumerate((lambda x: x.reshape(x.size(0), -1), lambda x: x.reshape(1, -1))):
        cos = F.cosine_similarity(view(g), view(p), dim=1, eps=h["eps"]).abs()
        r = float(cos.max()) / (h["delta"] / np.sqrt(view(p).size(1)))
        out.append((v, r))
        if r < 1:
            break
    return out


def _state_arrays(cls, opt, ps, prefix, out):
    keys = list(opt.state[ps[0]]) if opt.state[ps[0]] else []
    for p in ps:
        assert list(opt.state[p]) == keys or set(opt.state[p]) == set(keys), "every parameter of a variant has the same keys"
    for key in keys:
        vals = [opt.state[p][key] for p in ps]
        if torch.is_tensor(vals[0]):
            out[f"{prefix}/{key}"] = np.concatenate([v.detach().numpy().reshape(-1) for v in vals])
        else:
            assert all(type(v) is type(vals[0]) for v in vals) and type(vals[0]) in (int, float)
            out[f"{prefix}/{key}"] = np.asarray(vals)
    out[f"{prefix}/keys"] = np.asarray(",".join(keys))
    if cls == "MADGRAD":
        out[f"{prefix}/k"] = opt.state["k"].numpy().copy()


def _expected_side(kind, view):
    """True: the view must fire (ratio < 0.5), False: it must not (ratio > 1.5)."""
    return (kind == "channel" and view == 0) or (kind == "layer" and view == 1)


def record_variant(cls, ref_cls, vname, ctor, seed):
    """-> dict of arrays, or None if a projection ratio came too close to 1."""
    params, draws = OO.make_problem(cls, seed)
    n = len(params)
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    groups = [dict({k: v for k, v in g.items() if k != "idx"}, params=[ps[i] for i in g["idx"] if i < n]) for g in OO.GROUPS]
    opt = ref_cls(groups, **ctor)
    hypers = OO.hypers_for(cls, ctor, n)
    steer = OO.STEER if cls in OO.PROJECTION else {}
    out, ratios, rows = {}, [], []
    for t in range(OO.STEPS):
        for i, p in enumerate(ps):
            if t in OO.NONE_AT.get(i, ()):
                p.grad = None
                continue
            p.grad = OO.gradient(steer.get(i), draws[t][i], params[i], p.detach().clone())
            if cls in OO.PROJECTION and p.dim() > 1:
                for v, r in _ratios(p.detach(), p.grad, hypers[i]):
                    if not (r < 0.5 if _expected_side(steer.get(i), v) else r > 1.5):
                        return None
                    ratios.append((i, t, v, r))
        opt.step()
        rows.append(np.concatenate([p.detach().numpy().reshape(-1) for p in ps]))
        if t + 1 in OO.STATE_STEPS:
            _state_arrays(cls, opt, ps, f"s{t + 1}", out)
        if t + 1 == 6:
            sd = opt.state_dict()
            index = {id(p): j for j, p in enumerate(q for g in opt.param_groups for q in g["params"])}
            for i, p in enumerate(ps):   # the state_dict's state is the recorded state, keyed by the packed index
                packed = sd["state"].get(index[id(p)], {})
                assert set(packed) == set(opt.state[p]), (cls, vname, i)
                for key, val in packed.items():
                    same = torch.equal(val, opt.state[p][key]) if torch.is_tensor(val) else val == opt.state[p][key]
                    assert same and type(val) is type(opt.state[p][key]), (cls, vname, i, key)
            out["sd6_param_groups"] = np.asarray(repr(sd["param_groups"]))
    out["params"] = np.stack(rows)
    if cls in OO.PROJECTION:
        out["ratios"] = np.asarray(ratios, dtype=np.float64)
    return out


def main():
    refs = reference_classes()
    for seed in range(OO.PROBLEM_SEED, OO.PROBLEM_SEED + 400):
        arrays, ok = {"meta_seed": np.asarray(seed)}, True
        for cls in OO.CLASSES:
            for vname, ctor in OO.VARIANTS[cls].items():
                rec = record_variant(cls, refs[cls], vname, ctor, seed) if ok else None
                if rec is None:
                    ok = False
                    break
                arrays.update({f"{cls}/{vname}/{k}": v for k, v in rec.items()})
            if not ok:
                break
        if ok:
            break
    else:
        raise RuntimeError("no seed keeps every projection ratio outside [0.5, 1.5]")
    if seed != OO.PROBLEM_SEED:
        raise RuntimeError(f"seed {seed} passes: set tests/optim_oracle.py PROBLEM_SEED to it and run again")
    fired = [r for k, v in arrays.items() if k.endswith("/ratios") for r in v[:, 3] if r < 1]
    quiet = [r for k, v in arrays.items() if k.endswith("/ratios") for r in v[:, 3] if r >= 1]
    print(f"seed {seed}: ratios where a view fires <= {max(fired):.2e}, where none does >= {min(quiet):.2f}")
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
