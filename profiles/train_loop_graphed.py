"""The refine loop of a data batch on batches whose object count changes every step: eager vs GraphedTrainLoop.

    python profiles/train_loop_graphed.py [--parent DIR] [--rounds R] [--out profiles/train_loop_graphed.json]

Workload: a seeded stream of 40 batches with 40..110 objects (what the reference's loader builds from 16 images,
engine/batching.py:66), N = M = 1024, n_iter = 4, fp32 and autocast.  Arms, each in a process of its own, run in alternation
R times (the median round is reported):
  eager_parent  the hand-written loop (engine.py:293-355) on the package found under --parent, a checkout of the parent
                commit with its library built (skipped without --parent)
  eager         the same loop on this tree: the shipped path must not move
  graphed       catre_amd.graphed.GraphedTrainLoop (default buckets): the first pass over the stream captures the buckets
                (time and reserved device memory per bucket are recorded), the timed passes replay
Wall time per refine iteration = time of a pass over the stream (device idle before and after) / (40 * 4); the eager arms
enqueue without reading any loss back (the reference reads eight .item() per iteration), which favours them.
"""
import argparse
import json
import logging
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N = M = 1024
N_BATCHES, N_ITER, LO, HI = 40, 4, 40, 110


def stream_counts():
    import random

    rng = random.Random(20240)
    return [rng.randint(LO, HI) for _ in range(N_BATCHES)]


def arm(name, root, amp, passes):
    sys.path.insert(0, root)
    logging.disable(logging.CRITICAL)
    import torch

    from catre_amd import synth
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg
    from catre_amd.synth import y_axis_symmetries

    cfg = default_cfg(num_pcl=N, num_kps=M, device="cuda:0")
    sd = {k: v.cuda() for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()}
    model, opt = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict(sd)
    model.train()
    sym = y_axis_symmetries(12)
    counts = stream_counts()
    big = {k: v.cuda() for k, v in synth.make_inputs(HI, N, M, seed=7).items()}
    batches = [({k: v[:n] for k, v in big.items()}, [sym if i % 3 == 0 else None for i in range(n)]) for n in counts]
    res = dict(arm=name, autocast=bool(amp), counts=counts)

    if name == "graphed":
        from catre_amd.graphed import GraphedTrainLoop

        loop = GraphedTrainLoop(model, opt, N, M, max_sym=12, amp=bool(amp))

        def one_pass():
            for b, s in batches:
                loop(b, N_ITER, s)
    else:
        def one_pass():
            for b, s in batches:
                b, poses_est, scales_est = dict(b), None, None
                for r in range(1, N_ITER + 1):
                    batch_updater_test(cfg, b, poses_est=poses_est, scales_est=scales_est)
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(amp)):
                        out, ld = model(b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"],
                                        K_zoom=b["K"], gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"],
                                        obj_kps=b["obj_kps"], mean_scales=b["obj_mean_scales"], sym_info=s, do_loss=True,
                                        cur_iter=r)
                        losses = sum(ld.values())
                    poses_est, scales_est = out[f"pose_{r}"].detach(), out[f"scale_{r}"].detach()
                    losses.backward()
                    opt.step()
                    opt.zero_grad(set_to_none=True)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one_pass()   # warm-up: allocations, and for the graphed arm the captures
    torch.cuda.synchronize()
    res["first_pass_s"] = round(time.perf_counter() - t0, 3)
    if name == "graphed":
        res["buckets"] = {str(C): dict(reserved_mib=round(v["bytes"] / 2 ** 20, 1), capture_s=round(v["capture_s"], 3))
                          for C, v in sorted(loop.stats().items())}
    times = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_pass()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / (N_BATCHES * N_ITER) * 1e3)
    res["ms_per_iteration"] = round(statistics.median(times), 4)
    res["ms_per_iteration_passes"] = [round(t, 4) for t in times]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "train_loop_graphed.json"))
    ap.add_argument("--arm", default=None)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--amp", type=int, default=0)
    a = ap.parse_args()
    if a.arm:
        return arm(a.arm, a.root, a.amp, a.passes)
    arms = ([("eager_parent", a.parent)] if a.parent else []) + [("eager", ROOT), ("graphed", ROOT)]
    runs = []
    for amp in (0, 1):
        for rnd in range(a.rounds):
            for name, root in arms:   # alternation: parent, this tree, graphed, parent, ...
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", name, "--root", root, "--amp", str(amp),
                                      "--passes", str(a.passes)], check=True, capture_output=True, text=True, timeout=600).stdout
                r = json.loads(out.strip().splitlines()[-1])
                r["round"] = rnd
                runs.append(r)
                print(name, "autocast" if amp else "fp32", rnd, r["ms_per_iteration"], flush=True)
    summary = {}
    for amp in (False, True):
        for name, _ in arms:
            sel = [r for r in runs if r["arm"] == name and r["autocast"] == amp]
            summary[f"{name}_{'autocast' if amp else 'fp32'}_ms_per_iteration"] = round(
                statistics.median(r["ms_per_iteration"] for r in sel), 4)
    doc = dict(workload=dict(N=N, M=M, n_iter=N_ITER, batches=N_BATCHES, objects=[LO, HI], counts=stream_counts()),
               summary=summary, buckets={("autocast" if r["autocast"] else "fp32"): r["buckets"] for r in runs if "buckets" in r},
               runs=[{k: v for k, v in r.items() if k != "counts"} for r in runs])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
