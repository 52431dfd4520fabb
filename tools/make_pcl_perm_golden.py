"""Fixture that pins the device permutation of the point-cloud preparation (``sample="device"`` of
``catre_amd.pcl_prep.sample_instances`` / ``sample_frames``).  That mode has no reference to compare against - it is "a
different but equally uniform sample" - so the library is pinned with its own output, recorded on the commit BEFORE the
single-frame and the frame-batch kernels were merged into one body (needs a HIP device and that commit's build):

    python tools/make_pcl_perm_golden.py            # tests/golden/pcl_device_perm.npz

Inputs and keys: ``tests/pcl_frames_ref.device_perm_outputs`` (two frames each of 48x40 and 72x64, 3 instances per frame,
64 points, seeds 0 and 2^63+5, ball crop and mask crop).  ``tests/test_pcl_unify.py`` compares a later build with it byte
for byte.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import pcl_frames_ref as R  # noqa: E402


def pinned(got):
    """``sample_frames`` and the loop of ``sample_instances`` gave the same bytes on the recorded commit: the fixture holds
    them once, under the key without the ``frames_`` / ``inst_`` prefix"""
    out = {}
    for k, v in got.items():
        who, _, key = k.partition("_")
        assert who in ("frames", "inst") and got["frames_" + key].tobytes() == got["inst_" + key].tobytes(), k
        out[key] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pcl_device_perm.npz"))
    a = ap.parse_args()
    got = pinned(R.device_perm_outputs())
    np.savez_compressed(a.out, **got)
    print("wrote", a.out, os.path.getsize(a.out), "bytes;", {k: v.tolist() for k, v in got.items() if k.endswith("_counts")})


if __name__ == "__main__":
    main()
