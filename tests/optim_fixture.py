"""Reading ``tests/golden/optim_steps.npz`` (written by ``tools/make_optim_golden.py``): a helper, not a test file."""
import ast
import functools
import os

import numpy as np
import torch

from tests import optim_oracle as OO
from tests.util import GOLDEN_DIR


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN_DIR, "optim_steps.npz")) as z:
        return {k: z[k] for k in z.files}


def split_flat(flat, shapes):
    """One row of ``params`` / one concatenated state entry -> a tensor per parameter."""
    out, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(torch.from_numpy(np.array(flat[o:o + n])).reshape(s))
        o += n
    assert o == len(flat)
    return out


def grads_for_step(cls, t, draws, params0, prev, steer=None):
    """The gradients of (0-based) step t, ``None`` where the tensor has none; ``prev``: the fp32 parameters the reference
    run held before the step (the steered tensors' gradients are built from them)."""
    steer = (OO.STEER if cls in OO.PROJECTION else {}) if steer is None else steer
    return [None if t in OO.NONE_AT.get(i, ()) else OO.gradient(steer.get(i), draws[t][i], params0[i], prev[i])
            for i in range(len(params0))]


def reference_state(z, name, step, shapes):
    """The reference's per-parameter state after ``step`` as a list of dicts (tensors and Python scalars, in key order)."""
    keys = [k for k in str(z[f"{name}/s{step}/keys"]).split(",") if k]
    out = [dict() for _ in shapes]
    for key in keys:
        arr = z[f"{name}/s{step}/{key}"]
        if arr.dtype == np.float32:
            for st, v in zip(out, split_flat(arr, shapes)):
                st[key] = v
        else:
            for st, v in zip(out, arr.tolist()):   # int64 -> int, float64 -> float
                st[key] = v
    return out


def reference_state_dict(z, name, shapes):
    """The ``state_dict()`` the reference class wrote after step 6."""
    groups = ast.literal_eval(str(z[f"{name}/sd6_param_groups"]))
    order = [i for g in groups for i in g["params"]]
    # the packed index counts parameters in group order; OO.GROUPS says which tensor that is
    tensor_of = [i for g in OO.GROUPS for i in g["idx"] if i < len(shapes)]
    assert order == list(range(len(tensor_of)))
    state = {j: st for j, st in ((j, reference_state(z, name, 6, shapes)[i]) for j, i in enumerate(tensor_of)) if st}
    if name.startswith("MADGRAD/"):
        state["k"] = torch.from_numpy(np.array(z[f"{name}/s6/k"]))
    return dict(state=state, param_groups=groups)
