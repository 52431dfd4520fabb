"""Worst deviation / bound ratios of the BOP pose errors on the GPU against the fp64 restatement, over the edge cases of
``tests/test_pose_errors.py`` (``tests/pose_errors_cases.py``; the bounds: ``tests/pose_errors_ref.py``):

    python profiles/bop_parity.py --out profiles     # profiles/bop_parity.json

A ratio of 1 would be a deviation as large as the derived bound; the tests assert ratios of at most 1.  VSD is compared
exactly and has no ratio: the file records the golden cases that matched bit for bit."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    import torch

    from catre_amd import pose_errors
    from tests import pose_errors_cases as C

    assert torch.cuda.is_available(), "bop_parity.py compares on a HIP device"
    cases = {}
    worst = {"e3": 0.0, "e2": 0.0, "p2": 0.0}
    for name in sorted(C.EDGE_CASES):
        d, refs = C.edge_data(name), C.edge_reference(name)
        got = C.run_sym(d)
        tabs = [t.cpu().numpy().astype(np.float64) for t in (got.e3, got.e2, got.p2)]
        row = {}
        for q, what in enumerate(("e3", "e2", "p2")):
            ratios, devs, bounds = [], [], []
            for i, r in enumerate(refs):
                S = C.SET_SIZES[i]
                want, bound = ((r.e3, r.b3), (r.e2, r.b2), (r.p2, r.bp))[q]
                dev = np.abs(tabs[q][i, :S] - want)
                ratios.append(float((dev / bound).max()))
                devs.append(float(dev.max()))
                bounds.append(float(bound.max()))
            row[what] = dict(worst_ratio=round(max(ratios), 4), worst_deviation=max(devs), largest_bound=max(bounds))
            worst[what] = max(worst[what], max(ratios))
        best = np.stack([t.cpu().numpy() for t in (got.best_mssd, got.best_mspd, got.best_proj)], 1)
        row["winners_equal"] = bool(all(np.array_equal(best[i], r.best) for i, r in enumerate(refs)))
        row["points"], row["set_sizes"] = C.EDGE_CASES[name][0], list(C.SET_SIZES)
        cases[name] = row
    g = C.golden()
    vsd = []
    for j, c in enumerate(C.golden_meta(g)["vsd_cases"]):
        errors, counts = pose_errors.vsd(C.dev(g[f"v{j}/d_est"])[None], C.dev(g[f"v{j}/d_gt"])[None], C.dev(g[f"v{j}/d_test"])[None],
                                         g["vsd/K"], delta=float(g["vsd/delta"]), taus=g["vsd/taus"].tolist(),
                                         diameter=float(g["vsd/diameter"]) if c["normalized"] else None, visib_mode=c["mode"])
        vsd.append(dict(c, counts_equal=bool(np.array_equal(counts.cpu().numpy()[0], g[f"v{j}/counts"])),
                        errors_equal=bool(np.array_equal(errors.cpu().numpy()[0], g[f"v{j}/errors"]))))
    res = dict(what="catre_sym_err against tests/pose_errors_ref.py; catre_vsd against tests/golden/pose_error_bop.npz",
               device=torch.cuda.get_device_name(0), units="e3: metres; e2, p2: pixels; ratio = deviation / derived bound",
               worst_ratio={k: round(v, 4) for k, v in worst.items()}, cases=cases, vsd_golden=vsd)
    json.dump(res, open(os.path.join(a.out, "bop_parity.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
