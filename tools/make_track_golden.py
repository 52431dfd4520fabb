"""Fixture for the nearest-neighbour statistics (``catre_amd/tracking.py``, ``evaluation.add_errors``), written by the
UNMODIFIED reference (needs the reference tree, see ``oracle/ref_shim.py``; never needed to build, test or run the product):

    python tools/make_track_golden.py            # tests/golden/pose_error_add.npz

``lib/pysixd/pose_error.py`` is loaded as it is.  Its module-level imports that ``add`` (:256-271), ``adi`` (:274-296) and
``transform_pts_Rt`` (:223-233) never touch - ``lib.utils.logger``, ``lib.pysixd.misc``, ``lib.pysixd.visibility`` - are
replaced by empty stand-in modules; numpy and SciPy (``spatial.cKDTree``) are the real ones.

A case is a seeded point set of n points on a box-shaped object of about 0.2 m, a ground-truth pose in front of the camera
and an estimate a few degrees and about a centimetre off; every stored value is fp32-representable (the device reads fp32)
and is handed to the reference widened to float64.  ``sym`` cases turn the estimate by 180 degrees about the y axis of a
point set that is symmetric under that turn, where ADD is of the object's size and ADD-S stays small."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pose_error_add.npz")
# (points, seed, symmetric set)
CASES = ((1, 1, False), (2, 2, False), (63, 3, False), (64, 4, False), (65, 5, False), (128, 6, True), (255, 7, False),
         (256, 8, False), (257, 9, False), (257, 10, True))


def load_reference():
    if not os.path.isdir(ref_shim.REFERENCE_ROOT):
        raise RuntimeError(f"reference tree not found at {ref_shim.REFERENCE_ROOT}")
    path = os.path.join(ref_shim.REFERENCE_ROOT, "lib", "pysixd", "pose_error.py")
    for name in ("lib", "lib.utils", "lib.utils.logger", "lib.pysixd", "lib.pysixd.misc", "lib.pysixd.visibility"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    sys.modules["lib.utils"].logger = sys.modules["lib.utils.logger"]
    sys.modules["lib.pysixd"].misc = sys.modules["lib.pysixd.misc"]
    sys.modules["lib.pysixd"].visibility = sys.modules["lib.pysixd.visibility"]
    spec = importlib.util.spec_from_file_location("ref_pose_error", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * K @ K


def make_case(n, seed, sym):
    rng = np.random.default_rng(seed)
    ext = rng.uniform(0.05, 0.12, 3)
    pts = rng.uniform(-1, 1, (n, 3)) * ext
    if sym:   # closed under (x, y, z) -> (-x, y, -z); an odd count keeps one point on the axis
        half, on_axis = pts[: n // 2], pts[n - n % 2:] * np.array([0.0, 1.0, 0.0])
        pts = np.concatenate((half, half * np.array([-1.0, 1.0, -1.0]), on_axis))
    pts = pts.astype(np.float32)
    R_gt = _rot(rng.normal(size=3), rng.uniform(0, 180))
    t_gt = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.6, 1.4)])
    dR = _rot(rng.normal(size=3), rng.uniform(1, 6))
    if sym:
        dR = dR @ _rot([0, 1, 0], 180)
    R_est = R_gt @ dR
    t_est = t_gt + rng.normal(0, 0.008, 3)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    return pts, f32(R_est), f32(t_est), f32(R_gt), f32(t_gt)


def main():
    mod = load_reference()
    out, meta = {}, []
    for j, (n, seed, sym) in enumerate(CASES):
        pts, R_est, t_est, R_gt, t_gt = make_case(n, seed, sym)
        assert pts.shape == (n, 3), pts.shape
        w = lambda a: a.astype(np.float64)
        add = float(mod.add(w(R_est), w(t_est).reshape(3, 1), w(R_gt), w(t_gt).reshape(3, 1), w(pts)))
        adi = float(mod.adi(w(R_est), w(t_est).reshape(3, 1), w(R_gt), w(t_gt).reshape(3, 1), w(pts)))
        for k, v in (("pts", pts), ("R_est", R_est), ("t_est", t_est), ("R_gt", R_gt), ("t_gt", t_gt),
                     ("add", np.float64(add)), ("adi", np.float64(adi))):
            out[f"c{j}/{k}"] = v
        meta.append({"n": n, "seed": seed, "sym": sym})
        print(f"case {j}: n {n} sym {sym} add {add:.6f} adi {adi:.6f}")
    out["meta"] = np.array(json.dumps({"cases": meta, "source": "lib/pysixd/pose_error.py add :256-271, adi :274-296"}))
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
