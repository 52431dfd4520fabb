"""Point-cloud prep of a data batch: one ``sample_frames`` call against the loop of ``sample_instances`` it replaces.

    python profiles/pcl_frames_probe.py            # -> profiles/pcl_frames_times.json

Workload: ``synth.make_depth_scene(H=480, W=640, n_inst=5)`` frames, F = 16 and 32 (``IMS_PER_BATCH`` of the two shipped
configs), ``num_points=1024``, device sampling.  In one process, per F:

  (a) loop      a loop of the unchanged ``sample_instances(..., sample="device")`` over the frames
  (b) frames    one ``sample_frames`` call
  (c) aug       ``augment_depth`` in device mode (fill, drop and noise on in every frame), then (b) on its output

Each is warmed up, then timed with device events around ``--inner`` back-to-back executions (a single one takes a
fraction of a millisecond; launch gaps count), reported per execution; the three alternate inside every repetition and
the medians of ``--reps`` (>= 20) repetitions are reported, with the C-ABI calls one execution makes ((a): three per
frame, counted from the loop; (b), (c): ``pcl_prep.abi_call_count``).  (a) and (b) must give the same clouds: checked
before anything is timed."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from catre_amd import pcl_prep, synth  # noqa: E402

DEV = "cuda:0"
N_INST, NUM_POINTS = 5, 1024


def make_frames(F, H, W):
    sc = [synth.make_depth_scene(H=H, W=W, n_inst=N_INST, seed=f) for f in range(F)]
    dev = lambda k: [s[k].to(DEV) for s in sc]
    per = dict(depth=dev("depth"), masks=dev("masks"), poses=dev("poses"), scales=dev("scales"), K=[s["K"] for s in sc])
    cat = dict(depth=torch.stack(per["depth"]), K=torch.stack(per["K"]), masks=torch.cat(per["masks"]),
               poses=torch.cat(per["poses"]), scales=torch.cat(per["scales"]),
               frame_of=[f for f in range(F) for _ in range(N_INST)])
    return per, cat


def run_loop(per, seeds):
    return [pcl_prep.sample_instances(per["depth"][f], per["K"][f], per["masks"][f], per["poses"][f], per["scales"][f],
                                      num_points=NUM_POINTS, sample="device", seed=seeds[f]) for f in range(len(seeds))]


def run_frames(cat, seeds, depth=None):
    return pcl_prep.sample_frames(cat["depth"] if depth is None else depth, cat["K"], cat["frame_of"], cat["poses"],
                                  cat["scales"], masks=cat["masks"], num_points=NUM_POINTS, sample="device", seed=seeds)


def run_aug(cat, seeds):
    F = cat["depth"].shape[0]
    depth = pcl_prep.augment_depth(cat["depth"], fill_holes=True, drop=[True] * F, drop_ratio=0.2, noise_level=[0.005] * F,
                                   seed=1)
    return run_frames(cat, seeds, depth)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcl_frames_times.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcl_frames_probe needs a HIP device: there is no CPU timing to report")
    if args.reps < 20:
        raise SystemExit("--reps must be >= 20")
    rows = []
    for F in args.frames:
        per, cat = make_frames(F, args.height, args.width)
        seeds = list(range(100, 100 + F))
        forms = {"loop": lambda: run_loop(per, seeds), "frames": lambda: run_frames(cat, seeds),
                 "aug_frames": lambda: run_aug(cat, seeds)}
        same = torch.equal(torch.cat(forms["loop"]()), forms["frames"]())
        calls = {"loop": 3 * F}
        for name in ("frames", "aug_frames"):
            before = pcl_prep.abi_call_count()
            forms[name]()
            calls[name] = pcl_prep.abi_call_count() - before
        for _ in range(args.warmup):
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, fn in forms.items():
                times[name].append(timed(fn, args.inner))
        row = dict(F=F, H=args.height, W=args.width, instances=F * N_INST, num_points=NUM_POINTS, reps=args.reps, inner=args.inner,
                   loop_equals_frames=bool(same), abi_calls=calls,
                   median_ms={k: statistics.median(v) for k, v in times.items()},
                   min_ms={k: min(v) for k, v in times.items()}, max_ms={k: max(v) for k, v in times.items()})
        rows.append(row)
        print(json.dumps(row))
    result = dict(device=torch.cuda.get_device_name(0), workload="synth.make_depth_scene frames, device sampling",
                  forms=dict(loop="sample_instances per frame", frames="one sample_frames call",
                             aug_frames="augment_depth (device mode) + one sample_frames call"), rows=rows)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
