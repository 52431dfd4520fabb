"""Loss-kernel times of the point-matching forms at the benchmark's shape (B = 256, M = 1024, half the objects
y-symmetric with 313 candidates), from ONE rocprofv3 kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/pm_loss_kernel_times.py      # on the GPU
    python profiles/pm_loss_kernel_times.py --summarize DIR/.../run_results.db profiles/pm_loss_kernel_times.json

Every form runs WARM + ITERS loss forwards and backwards in the fixed order of FORMS, so the trace's k_loss_* dispatches
split into equal blocks by launch order; the summary is the median of the last ITERS of each block, in microseconds.
A record, not a bar: the loss is three launches of a 15 ms iteration.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARM, ITERS = 3, 20
B, M, NSYM = 256, 1024, 313
# (label, LOSS_CFG overrides); the first is the shipped configuration
FORMS = [
    ("shipped: R only, L1", {}),
    ("R+t (base config), L1", dict(PM_R_ONLY=False, PM_DISENTANGLE_T=False, PM_DISENTANGLE_Z=False)),
    ("R+t, Smooth_L1", dict(PM_R_ONLY=False, PM_LOSS_TYPE="Smooth_L1", PM_SMOOTH_L1_BETA=0.05)),
    ("R+t, L2", dict(PM_R_ONLY=False, PM_LOSS_TYPE="L2")),
    ("R / t on points, L1", dict(PM_R_ONLY=False, PM_DISENTANGLE_T=True, PM_T_USE_POINTS=True)),
    ("R / xy / z on points, L1", dict(PM_R_ONLY=False, PM_DISENTANGLE_Z=True, PM_T_USE_POINTS=True)),
    ("R / xy / z on points, L2", dict(PM_R_ONLY=False, PM_DISENTANGLE_Z=True, PM_T_USE_POINTS=True, PM_LOSS_TYPE="L2")),
    ("R / xy / z direct, MSE", dict(PM_R_ONLY=False, PM_DISENTANGLE_Z=True, PM_T_USE_POINTS=False, PM_LOSS_TYPE="MSE")),
    ("R+t, L1, bbox points (M = 8)", dict(PM_R_ONLY=False, PM_USE_BBOX=True)),
]


def run():
    import torch

    from catre_amd import synth
    from catre_amd.config import default_cfg
    from catre_amd.losses import SymTensors, catre_loss
    from oracle.catre_oracle import y_axis_symmetries

    dev = "cuda:0"
    inp = {k: v.to(dev) for k, v in synth.make_inputs(B, 64, M, seed=7).items()}
    sym = SymTensors.from_list([y_axis_symmetries(NSYM + 1) if i % 2 else None for i in range(B)], dev)
    g = torch.Generator().manual_seed(1)
    pose = torch.cat([inp["gt_rot"], (inp["gt_trans"] + 0.05 * torch.randn(B, 3, generator=g).to(dev)).unsqueeze(-1)], -1)
    scale = inp["gt_scale"] + 0.02 * torch.randn(B, 3, generator=g).to(dev)
    for label, over in FORMS:
        cfg = default_cfg(num_pcl=64, num_kps=M, device=dev)
        for k, v in over.items():
            cfg.MODEL.CATRE.LOSS_CFG[k] = v
        for _ in range(WARM + ITERS):
            p, s = pose.clone().requires_grad_(True), scale.clone().requires_grad_(True)
            ld = catre_loss(cfg, p[:, :3, :3], p[:, :3, 3], s, inp["gt_rot"], inp["gt_trans"], inp["gt_scale"], inp["obj_kps"],
                            sym, pose=p)
            sum(ld.values()).backward()
        torch.cuda.synchronize()
        print(label, list(ld))


def summarize(db, out):
    import sqlite3
    import statistics

    c = sqlite3.connect(db)
    res = {"shape": {"B": B, "M": M, "sym_candidates": NSYM, "symmetric_objects": B // 2}, "iters": ITERS, "unit": "us (median)",
           "forms": {}}
    for kern in ("k_loss_fwd", "k_loss_reduce", "k_loss_bwd"):
        d = [r[0] for r in c.execute("select duration from kernels where name like ? order by start", (kern + "%",))]
        n = WARM + ITERS
        assert len(d) == n * len(FORMS), (kern, len(d))
        for i, (label, _) in enumerate(FORMS):
            res["forms"].setdefault(label, {})[kern] = round(statistics.median(d[i * n + WARM:(i + 1) * n]) / 1e3, 2)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for label, v in res["forms"].items():
        print(f"{label:40s}", v)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        run()
