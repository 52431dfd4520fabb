"""Time the six point-cloud entry points (``catre_pcl_{candidates,sample,fps}`` on one frame, ``catre_pclf_*`` on a batch)
through the raw C ABI, for an A/B of two builds of the same ABI:

    python profiles/pcl_unify_probe.py --out run.json                               # the library of this tree
    CATRE_HIP_LIB=/path/to/other/libcatre_hip.so python profiles/pcl_unify_probe.py --out other.json

Workload: the frames of ``profiles/pcl_frames_probe.py`` - ``synth.make_depth_scene(H=480, W=640, n_inst=5)``, 1024
points, ball crop, device sampling: one frame with its 5 instances for ``catre_pcl_*``, F = 16 frames with 80 instances
for ``catre_pclf_*``.  Each entry point is warmed up, then timed with device events around ``--inner`` (40) back-to-back
calls; the median of ``--reps`` such windows is reported in ms per call.  ``profiles/pcl_unify_ab.json`` holds three
such runs of the build before the two kernel sets were merged and three of the build after, taken alternately in fresh
processes."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from catre_amd import hip, synth  # noqa: E402

DEV = "cuda:0"
F, N_INST, NUM_POINTS, H, W = 16, 5, 1024, 480, 640


def tiled(c, n):
    while 0 < c < n:
        c *= 2
    return c


def entry_points():
    """-> {name: callable making one ABI call}; candidates have run once, so sample / fps read a filled workspace"""
    sc = [synth.make_depth_scene(H=H, W=W, n_inst=N_INST, seed=f) for f in range(F)]
    return {**one_set("pcl", sc[:1]), **one_set("pclf", sc)}


def one_set(name, sc):
    lib, p = hip.load(), hip.ptr
    nf, table = len(sc), name == "pclf"
    I = nf * N_INST
    dev = lambda k: torch.cat([s[k] for s in sc]).to(DEV).contiguous()
    st = hip.stream_ptr(torch.device(DEV))
    depth = torch.stack([s["depth"] for s in sc]).to(DEV).contiguous()
    masks, poses, scales = dev("masks").to(torch.uint8), dev("poses"), dev("scales")
    k9 = (ctypes.c_float * (9 * nf))(*[float(v) for s in sc for v in s["K"].reshape(-1)])
    nbytes = lib.catre_pclf_workspace_bytes(nf, I, H, W) if table else lib.catre_pcl_workspace_bytes(I, H, W)
    ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=DEV)
    counts = torch.zeros(I, dtype=torch.int32, device=DEV)
    fo = (ctypes.c_int32 * I)(*[f for f in range(nf) for _ in range(N_INST)])
    seeds = (ctypes.c_uint64 * nf)(*range(100, 100 + nf))
    pre = (p(depth), k9, fo) if table else (p(depth), k9)
    dims = (nf, I, H, W) if table else (I, H, W)
    if table:
        cand = lambda: lib.catre_pclf_candidates(*pre, p(masks), None, 0, None, p(poses), p(scales), 0.5, 1, *dims, p(ws),
                                                 nbytes, p(counts), st)
    else:
        cand = lambda: lib.catre_pcl_candidates(*pre, p(masks), p(poses), p(scales), 0.5, 1, *dims, p(ws), nbytes,
                                                p(counts), st)
    hip.check(cand(), name + "_candidates")
    cl = counts.cpu().tolist()
    assert min(cl) > 0, cl
    cap = max(tiled(c, NUM_POINTS) for c in cl)
    scratch = torch.zeros(I * 4 * cap, dtype=torch.float32, device=DEV)
    sidx = torch.zeros(I, NUM_POINTS, dtype=torch.int64, device=DEV)
    pcl = torch.zeros(I, NUM_POINTS, 3, device=DEV)
    if table:
        samp = lambda: lib.catre_pclf_sample(*pre, None, p(ws), nbytes, None, seeds, *dims, NUM_POINTS, p(pcl), None, st)
        fps = lambda: lib.catre_pclf_fps(*pre, p(ws), nbytes, *dims, NUM_POINTS, p(scratch), cap, p(sidx), st)
    else:
        samp = lambda: lib.catre_pcl_sample(*pre, p(ws), nbytes, None, 100, *dims, NUM_POINTS, p(pcl), None, st)
        fps = lambda: lib.catre_pcl_fps(*pre, p(ws), nbytes, *dims, NUM_POINTS, p(scratch), cap, p(sidx), st)
    return {f"catre_{name}_{what}": (lambda fn=fn, what=what: hip.check(fn(), what))
            for what, fn in (("candidates", cand), ("sample", samp), ("fps", fps))}


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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcl_unify_probe needs a HIP device: there is no CPU timing to report")
    calls = entry_points()
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            times[k].append(timed(fn, args.inner))
    row = dict(device=torch.cuda.get_device_name(0), F=F, H=H, W=W, instances_per_frame=N_INST,
               num_points=NUM_POINTS, reps=args.reps, inner=args.inner,
               median_ms={k: statistics.median(v) for k, v in times.items()}, min_ms={k: min(v) for k, v in times.items()},
               max_ms={k: max(v) for k, v in times.items()})
    print(json.dumps(row))
    with open(args.out, "w") as fh:
        json.dump(row, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
