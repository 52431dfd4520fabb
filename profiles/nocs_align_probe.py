"""Time and parity of the NOCS-map alignment (``catre_amd/nocs_align.py``) on the GPU:

    python profiles/nocs_align_probe.py --out DIR     # DIR/nocs_align_time.json, DIR/nocs_align_parity.json

Time: ``estimate_similarity`` at I = 256 instances of N = 1024 points (30 % outliers, the fixture's generator), device
draws, HIP events around ``--reps`` calls after a warm-up, against ``tests/nocs_align_ref.py`` (the numpy restatement) on
the same draws in a pool of 16 processes on the same machine.  Parity: the fixture's ragged batch against the values the
reference wrote (largest |difference| of s, R, t per case) and the count of discrete mismatches."""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import nocs_align_ref as REF  # noqa: E402
from tools.make_align_golden import make_case  # noqa: E402  (the fixture's generator; the reference is not loaded)

I, N, SEED = 256, 1024, 3


def _one(args):
    out = REF.estimate_similarity(*args)
    return out.scale, out.R, out.t, out.valid, out.n_inliers, out.iters, out.best_it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5000)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--instances", type=int, default=I)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    n_inst = a.instances
    cases = [make_case(N, 0.3, 1000 + i)[:2] for i in range(n_inst)]
    draws = REF.draw_indices([N] * n_inst, seed=SEED)
    # the host side first: the pool forks before this process opens the GPU
    with mp.Pool(a.procs) as pool:
        jobs = [(s, d, draws[i]) for i, (s, d) in enumerate(cases)]
        pool.map(_one, jobs[:a.procs])                   # warm the workers
        t0 = time.perf_counter()
        host = pool.map(_one, jobs, chunksize=max(1, n_inst // a.procs))
        host_s = time.perf_counter() - t0

    import torch

    from catre_amd import nocs_align

    dev = "cuda:0"
    src = torch.from_numpy(np.stack([c[0] for c in cases])).to(dev)
    dst = torch.from_numpy(np.stack([c[1] for c in cases])).to(dev)
    for _ in range(10):
        out = nocs_align.estimate_similarity(src, dst, seed=SEED)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    windows = []
    for _ in range(5):                                   # five windows: the spread of the same measurement
        e0.record()
        for _ in range(a.reps):
            out = nocs_align.estimate_similarity(src, dst, seed=SEED)
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / a.reps)
    got = [v.cpu().numpy() for v in out[:7]]
    same = sum(int(got[3][i] == h[3] and got[4][i] == h[4] and got[5][i] == h[5] and got[6][i] == h[6]) for i, h in enumerate(host))
    err = max(max(abs(got[0][i] - h[0]), np.abs(got[1][i] - h[1]).max(), np.abs(got[2][i] - h[2]).max())
              for i, h in enumerate(host) if got[6][i] == h[6] and got[4][i] == h[4])
    res = dict(what="estimate_similarity, device draws, max_iter 128", instances=n_inst, points=N, outlier_share=0.3,
               device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName, device_ms_per_call=round(float(np.median(windows)), 4),
               device_ms_windows=[round(w, 4) for w in windows], calls_per_window=a.reps,
               device_note="HIP events around back-to-back calls after 10 warm-up calls; includes the launches and the "
                           "allocations of the Python wrapper",
               numpy_restatement_s=round(host_s, 3), numpy_processes=a.procs,
               numpy_note="tests/nocs_align_ref.py on the same draws, one wall-clock run of a process pool on the same machine",
               iterations_mean=float(got[5].mean()), instances_with_equal_discrete_outputs=same,
               max_abs_err_where_equal=float(err))
    json.dump(res, open(os.path.join(a.out, "nocs_align_time.json"), "w"), indent=1)
    print(json.dumps(res))

    # parity against the reference's fixture
    z = np.load(os.path.join(ROOT, "tests", "golden", "nocs_align.npz"))
    meta = json.loads(str(z["meta"]))
    counts = [c["n"] for c in meta["cases"]]
    J, Nmax = len(counts), max(counts)
    s_ = np.full((J, Nmax, 3), np.nan, np.float32)
    d_ = np.full((J, Nmax, 3), np.nan, np.float32)
    dr = np.zeros((J, 128, 5), np.int32)
    for j, n in enumerate(counts):
        s_[j, :n], d_[j, :n], dr[j] = z[f"c{j}/src"], z[f"c{j}/dst"], z[f"c{j}/draws"]
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    out = nocs_align.estimate_similarity(t(s_), t(d_), t(np.asarray(counts, np.int32)), draws=t(dr), return_inliers=True)
    g = [v.cpu().numpy() for v in out]
    rows = []
    for j, c in enumerate(meta["cases"]):
        mask = np.zeros(Nmax, np.uint8)
        mask[z[f"c{j}/inliers"]] = 1
        rows.append(dict(n=c["n"], outliers=c["outliers"], iters=int(g[5][j]), best_it=int(g[6][j]), n_inliers=int(g[4][j]),
                         valid=int(g[3][j]),
                         discrete_equal=bool(g[5][j] == c["iters"] and g[6][j] == c["best_it"] and g[3][j] == (not c["none"])
                                             and np.array_equal(g[7][j], mask)),
                         max_abs_err=float(max(abs(g[0][j] - float(z[f"c{j}/s"])), np.abs(g[1][j] - z[f"c{j}/R"]).max(),
                                               np.abs(g[2][j] - z[f"c{j}/t"]).max()))))
    par = dict(what="catre_nocs_align on the reference's draws vs tests/golden/nocs_align.npz (written by the unmodified "
                    "reference); largest |difference| over s, R, t", bound=1e-12, device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
               worst=max(r["max_abs_err"] for r in rows), cases=rows)
    json.dump(par, open(os.path.join(a.out, "nocs_align_parity.json"), "w"), indent=1)
    print(json.dumps(par))


if __name__ == "__main__":
    main()
