"""Step time of the fused optimizers (catre_amd/optimizers.py) on the shipped model's parameter set, against the same
steps run as torch ops on the device (tests/optim_oracle.py in fp32: the reference classes' op sequence, what a user
would otherwise run - the reference tree itself is not needed).

    python profiles/optim_step_time.py            # writes profiles/optim_step_time.json

One process.  Per class: both forms step the same parameters with the same seeded gradients; WARMUP steps each, then
REPEATS windows per form, alternating the two forms, each window a host clock around N steps that ends in a device
synchronise.  Reported: median / min / max ms per step over the windows, and the ratio of the medians.
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from catre_amd import optimizers  # noqa: E402
from catre_amd.CATRE_disR_shared import expected_state_shapes  # noqa: E402
from catre_amd.config import default_cfg  # noqa: E402
from tests import optim_oracle as OO  # noqa: E402

DEV = "cuda:0"
WARMUP, REPEATS, FUSED_STEPS, TORCH_STEPS = 20, 7, 200, 20
CTOR = {"SGDP": dict(momentum=0.9), "SGD_GC": dict(momentum=0.9), "SGD_GCC": dict(momentum=0.9)}
OUT = os.path.join(ROOT, "profiles", "optim_step_time.json")


def window(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    shapes = [tuple(s) for k, s in expected_state_shapes(default_cfg()).items() if "running" not in k and "num_batches" not in k]
    gen = torch.Generator().manual_seed(5)
    init = [0.1 * torch.randn(s, generator=gen) for s in shapes]
    grads = [(0.01 * torch.randn(s, generator=gen) + 0.005 * p).to(DEV) for s, p in zip(shapes, init)]
    result = dict(device=torch.cuda.get_device_name(0), tensors=len(shapes), elements=sum(p.numel() for p in init),
                  warmup=WARMUP, repeats=REPEATS, fused_steps_per_window=FUSED_STEPS, torch_steps_per_window=TORCH_STEPS,
                  classes={})
    for cls in OO.CLASSES:
        ctor = dict(CTOR.get(cls, {}))
        ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in init]
        for p, g in zip(ps, grads):
            p.grad = g
        fused = getattr(optimizers, cls)([dict(params=ps, lr=1e-4, weight_decay=1e-2)], **ctor)
        hyp = OO.hyper(cls, ctor, dict(lr=1e-4, weight_decay=1e-2))
        loop = OO.Restated(cls, [p.clone().to(DEV) for p in init], [hyp] * len(init), record_ratios=False)
        torch_step = lambda: loop.step(grads)
        for _ in range(WARMUP):
            fused.step()
            torch_step()
        tf, tt = [], []
        for _ in range(REPEATS):
            tf.append(window(fused.step, FUSED_STEPS))
            tt.append(window(torch_step, TORCH_STEPS))
        row = dict(fused_ms=statistics.median(tf), fused_ms_min=min(tf), fused_ms_max=max(tf),
                   torch_ops_ms=statistics.median(tt), torch_ops_ms_min=min(tt), torch_ops_ms_max=max(tt))
        row["torch_ops_over_fused"] = row["torch_ops_ms"] / row["fused_ms"]
        result["classes"][cls] = row
        print(cls, json.dumps(row), flush=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
