"""A/B of the two reduced-precision inference modes, bf16 vs fp16 operands (COMPUTE_DTYPE="bf16" / "fp16"), in ONE process.

Same model, seeded recipe weights, inputs and timed region as bench.py's refine leg (warm-up, then `--steps` x
model.refine(batch, n_iter=K) between device synchronises), at the headline shape (B=256, N=M=1024, K=4) and at config 5
(B=256, N=2048, M=1024, K=8).  The two modes alternate for `--rounds` rounds so that clock / thermal drift hits both; one
JSON line per (shape, round, mode) and a summary line per shape (median rate of each mode, fp16 / bf16).

    python profiles/fp16_ab.py [--rounds 3] [--steps 20] [--warmup 3] > profiles/<tag>_fp16_ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"headline": (256, 1024, 1024, 4), "config5": (256, 2048, 1024, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="headline,config5")
    ap.add_argument("--modes", default="bf16,fp16", help="one mode alone: a run to put under rocprofv3")
    args = ap.parse_args()

    from catre_amd import hip, synth
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    hip.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for shape in args.shapes.split(","):
        B, N, M, K = SHAPES[shape]
        cfg = default_cfg(num_pcl=N, num_kps=M, n_iter=K, device=str(dev))
        model, _ = build_model_optimizer(cfg, is_test=True)
        sd = synth.recipe_state_dict(expected_state_shapes(cfg))
        model.load_state_dict({k: v.to(dev) for k, v in sd.items()}, strict=True)
        model.eval()
        batch = {k: v.to(dev) for k, v in synth.make_inputs(B, N, M, seed=1000).items()}  # bench.py's rank-0 inputs
        modes = args.modes.split(",")
        rates = {m: [] for m in modes}
        for mode in rates:  # both packs made and every kernel loaded before the first timed round
            model.cfg.MODEL.CATRE.COMPUTE_DTYPE = mode
            for _ in range(args.warmup):
                model.refine(batch, n_iter=K)
        for r in range(args.rounds):
            for mode in modes if r % 2 == 0 else modes[::-1]:
                model.cfg.MODEL.CATRE.COMPUTE_DTYPE = mode
                for _ in range(args.warmup):
                    model.refine(batch, n_iter=K)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    out = model.refine(batch, n_iter=K)
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                assert torch.isfinite(out[f"pose_{K}"]).all()
                rate = B * K * args.steps / dt
                rates[mode].append(rate)
                print(json.dumps({"shape": shape, "B": B, "N": N, "M": M, "K": K, "round": r, "mode": mode,
                                  "steps": args.steps, "ms_per_refine": round(dt / args.steps * 1e3, 3),
                                  "object_iterations_per_s": round(rate, 1)}), flush=True)
        med = {m: statistics.median(v) for m, v in rates.items()}
        if len(med) < 2:
            continue
        print(json.dumps({"shape": shape, "summary": True, "median_object_iterations_per_s": {m: round(v, 1) for m, v in med.items()},
                          "fp16_over_bf16": round(med["fp16"] / med["bf16"], 4)}), flush=True)


if __name__ == "__main__":
    main()
