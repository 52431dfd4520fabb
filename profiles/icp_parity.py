"""One trimmed-ICP step on the GPU against the fp64 restatement (``tests/icp_ref.py``), every configuration of
``tests/test_icp.py::test_one_step_against_the_restatement``:

    python profiles/icp_parity.py --out profiles   # profiles/icp_parity.json

Per n_src: the number of rows compared, how many were fitted (status 0), whether every kept mask and count was equal, and
the worst |device - restatement| / (2^-23 |ref| + 1e-11) over pose, scale and rmse."""
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

    from tests import icp_cases as C

    assert torch.cuda.is_available(), "icp_parity.py compares on a HIP device"
    rows = []
    for n_src in C.STEP_N_SRC:
        worst, n, fits, equal = 0.0, 0, 0, True
        for row in C.step_rows(n_src):
            n += 1
            fits += row["ref"].status == 0
            equal = equal and np.array_equal(row["got"][5].astype(bool), row["ref"].mask) and int(row["got"][3]) == row["ref"].kept \
                and int(row["got"][4]) == row["ref"].status
            worst = max(worst, C.step_ratio(row))
        rows.append(dict(n_src=n_src, n_dst=C.N_DST, rows=n, fitted=int(fits), masks_counts_status_equal=bool(equal),
                         worst_ratio_to_bound=round(worst, 4)))
    res = dict(what="catre_icp_step vs tests/icp_ref.py", device=torch.cuda.get_device_name(0), bound="2^-23 |ref| + 1e-11",
               cases=rows, worst_ratio_to_bound=max(r["worst_ratio_to_bound"] for r in rows))
    json.dump(res, open(os.path.join(a.out, "icp_parity.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
