"""Fixture for the BOP pose errors (``catre_amd/pose_errors.py``), written by the UNMODIFIED reference (needs the reference
tree, see ``oracle/ref_shim.py``; never needed to build, test or run the product):

    python tools/make_pose_error_golden.py            # tests/golden/pose_error_bop.npz

``lib/pysixd/pose_error.py``, ``misc.py``, ``transform.py`` and ``visibility.py`` are loaded as they are.  The module-level
imports that the functions used here never touch are stand-ins: ``cv2``, ``mmcv``, ``PIL`` (any attribute is a dummy),
``numba`` (``jit`` / ``njit`` hand the function back), ``lib.utils.logger``, ``lib.vis_utils.colormap`` and
``lib.pysixd.inout``.  numpy and SciPy are the real ones.  Used: ``misc.get_symmetry_transformations`` (:234-282),
``misc.get_axis_symmetry_transformations`` (:220-231), ``pose_error.mssd`` (:131-153), ``mspd`` (:156-179), ``proj_sym``
(:196-217) and ``vsd`` (:22-128) with a stand-in renderer object that returns prepared depth images.

Every stored input is fp32-representable (the device reads fp32) and handed to the reference widened to float64; results
are float64.  ``vsd`` hard-codes ``visib_mode="bop19"``; for the ``bop18`` cases the two ``visibility.estimate_visib_mask_*``
functions it calls are wrapped to pass ``"bop18"`` on, everything else runs as written.

* ``info<k>/syms``: the sets of four ``model_info`` entries - no symmetry, discrete only, one continuous axis with a non-zero
  offset, both.
* ``sets/<name>``: the fp32 sets the point errors use: ``one`` (identity), ``two`` (identity and the half turn about y),
  ``y314`` (identity and the 313 turns about y by multiples of 2 pi / 314 - ``synth.y_axis_symmetries(314)``, the loader-shaped
  set the benchmark uses - from ``get_axis_symmetry_transformations`` at a step of pi / 313.5; at 0.01 the reference itself
  discretizes into 315 steps, 314 turns: ``info2`` and ``axis_y``).
* ``s<j>/...``: point counts 1, 63, 64, 65, 257 x the three sets; the estimate is a few degrees and about a centimetre off
  a NON-identity member of the set, so the winning symmetry is not index 0.
* ``v<j>/...``: 24 x 32 depth triples with ``K = [[16,0,16],[0,16,12],[0,0,1]]``; both visibility modes, diameter
  normalisation on and off, an empty union.  Threshold pixels: rows where ``fl32(dist_model) - fl32(dist_test)`` equals
  ``delta = 2^-6`` exactly and where it lies one fp32 step to either side (found by search: the distances are square roots),
  for the ground-truth render (rows 5-7) and the estimate (rows 15-17); and the pixels where ``(x - cx) / fx, (y - cy) / fy,
  1`` is a dyadic Pythagorean quadruple - there ``dist = c * depth`` exactly (c = 1, 9/8, 5/4, 3/2), and ``|dist_gt -
  dist_est|`` (divided by the diameter 1/4 in the normalised cases) sits exactly on a tau of the list."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "pose_error_bop.npz")
STEP = 0.01
POINT_COUNTS = (1, 63, 64, 65, 257)
SET_NAMES = ("one", "two", "y314")
H, W, DELTA, DIAMETER = 24, 32, 2.0 ** -6, 0.25
K_VSD = np.array([[16, 0, 16], [0, 16, 12], [0, 0, 1]], np.float32)
TAUS = (2.0 ** -5, 9 * 2.0 ** -8, 5 * 2.0 ** -7, 3 * 2.0 ** -6, 0.05, 0.2)         # c * 2^-5 for c = 1, 9/8, 5/4, 3/2
# (x - cx, y - cy) in pixels with ((x - cx) / 16)^2 + ((y - cy) / 16)^2 + 1 = c^2, c dyadic
EXACT = {(0, 0): 1.0, (12, 0): 1.25, (-12, 0): 1.25, (0, -12): 1.25, (2, 8): 1.125, (-2, 8): 1.125, (2, -8): 1.125,
         (-2, -8): 1.125, (8, 2): 1.125, (-8, 2): 1.125, (8, -2): 1.125, (-8, -2): 1.125, (-16, 8): 1.5, (-16, -8): 1.5}
MODEL_INFOS = (
    {"diameter": 0.2},
    {"symmetries_discrete": [[-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1],
                             [1, 0, 0, 0.01, 0, -1, 0, 0, 0, 0, -1, 0.02, 0, 0, 0, 1]]},
    {"symmetries_continuous": [{"axis": [0, 1, 0], "offset": [0.01, 0, -0.02]}]},
    {"symmetries_discrete": [[1, 0, 0, 0, 0, -1, 0, 0.004, 0, 0, -1, 0, 0, 0, 0, 1]],
     "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0.003, -0.002, 0]}]},
)


class _Any(types.ModuleType):
    """a module whose every attribute is a dummy (constants read at ``def`` time, names imported ``from`` it)"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return 0


def _identity_jit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda f: f


def load_reference():
    if not os.path.isdir(ref_shim.REFERENCE_ROOT):
        raise RuntimeError(f"reference tree not found at {ref_shim.REFERENCE_ROOT}")
    pys = os.path.join(ref_shim.REFERENCE_ROOT, "lib", "pysixd")
    for name in ("cv2", "mmcv", "PIL", "numba", "lib", "lib.utils", "lib.utils.logger", "lib.vis_utils", "lib.vis_utils.colormap",
                 "lib.pysixd", "lib.pysixd.inout"):
        m = _Any(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["numba"].jit = sys.modules["numba"].njit = _identity_jit
    sys.modules["lib.utils"].logger = sys.modules["lib.utils.logger"]

    def load(name):
        spec = importlib.util.spec_from_file_location(f"lib.pysixd.{name}", os.path.join(pys, f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"lib.pysixd.{name}"] = mod
        setattr(sys.modules["lib.pysixd"], name, mod)
        spec.loader.exec_module(mod)
        return mod

    load("transform")
    load("visibility")
    misc = load("misc")
    return load("pose_error"), misc, sys.modules["lib.pysixd.visibility"]


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def w64(a):
    return np.asarray(a).astype(np.float64)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * Kx + (1 - np.cos(r)) * Kx @ Kx


def as34(trans):
    return np.stack([np.hstack([np.asarray(t["R"], np.float64), np.asarray(t["t"], np.float64).reshape(3, 1)]) for t in trans])


def sym_case(n, seed, syms):
    """points of a box-shaped object of about 0.2 m, a pose in view of a 600 px camera, the estimate off member `pick`"""
    rng = np.random.default_rng(seed)
    pts = f32(rng.uniform(-1, 1, (n, 3)) * rng.uniform(0.05, 0.12, 3))
    if n == 1:
        pts = f32([[0.09, 0.03, -0.07]])                                   # off the axis: the symmetries differ
    R_gt = _rot(rng.normal(size=3), rng.uniform(0, 180))
    t_gt = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15), rng.uniform(0.6, 1.4)])
    pick = 0 if len(syms) == 1 else (1 if len(syms) == 2 else int(rng.integers(20, len(syms) - 20)))
    Rs, ts = w64(syms[pick, :, :3]), w64(syms[pick, :, 3])
    dR = _rot(rng.normal(size=3), rng.uniform(2, 5))
    R_est = R_gt @ Rs @ dR
    t_est = R_gt @ ts + t_gt + rng.normal(0, 0.006, 3)
    K = np.array([[600 + seed, 0, 320.5], [0, 598, 239.25], [0, 0, 1]], np.float32)
    return dict(pts=pts, R_est=f32(R_est), t_est=f32(t_est), R_gt=f32(R_gt), t_gt=f32(t_gt), K=K), pick


# ---- VSD images ---------------------------------------------------------------------------------------------------------
def dist32(d, x, y):
    """fl32 of the reference's distance at pixel (x, y) for the fp32 depth d (misc.py:643-645)"""
    K = w64(K_VSD)
    px, py = (x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1]
    d = np.float64(d)
    return np.float32(np.sqrt((px * d) ** 2 + (py * d) ** 2 + d ** 2))


def on_delta(x, y, rng):
    """(d_test, d_model on, one step above, one step below): fl32(dist_model) - fl32(dist_test) == delta exactly for the
    first, the next larger / smaller value of that fp32 difference for the others"""
    dl = np.float32(DELTA)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    for _ in range(4000):
        dt = np.float32(1 + rng.integers(0, 512) / 1024)
        Dt = dist32(dt, x, y)
        target = np.float32(Dt + dl)
        if np.float32(target - Dt) != dl:
            continue
        c = np.float64(Dt) / np.float64(dt)
        dm = np.float32(np.float64(target) / c)
        for _ in range(8):
            dm = np.nextafter(dm, down)
        for _ in range(17):
            if dist32(dm, x, y) == target:
                hi, lo = np.nextafter(dm, up), np.nextafter(dm, down)
                while dist32(hi, x, y) == target:
                    hi = np.nextafter(hi, up)
                while dist32(lo, x, y) == target:
                    lo = np.nextafter(lo, down)
                if np.float32(dist32(hi, x, y) - Dt) > dl > np.float32(dist32(lo, x, y) - Dt):
                    return dt, dm, hi, lo
            dm = np.nextafter(dm, up)
    raise RuntimeError(f"no depth pair on the threshold at pixel {(x, y)}")


def vsd_images(seed, empty=False):
    rng = np.random.default_rng(seed)
    d_gt = rng.uniform(0.7, 1.3, (H, W)).astype(np.float32)
    d_est = (d_gt + rng.normal(0, 0.06, (H, W))).astype(np.float32)                      # around the taus
    d_test = (d_gt + rng.normal(0, 0.02, (H, W))).astype(np.float32)                     # both sides of delta
    d_gt[rng.random((H, W)) < 0.3] = 0                                                    # background of either render
    d_est[rng.random((H, W)) < 0.3] = 0
    d_test[rng.random((H, W)) < 0.15] = 0                                                 # holes
    if empty:                                                                             # a wall in front of everything
        return np.full((H, W), 0.3, np.float32), d_gt, d_est
    for row, model, other in ((5, d_gt, d_est), (15, d_est, d_gt)):
        for x in range(W):
            for k in range(3):           # row: on the threshold, row + 1: one step above, row + 2: one step below
                found = on_delta(x, row + k, rng)
                d_test[row + k, x], model[row + k, x] = found[0], found[1 + k]
        other[row:row + 3] = 0           # the other render is background here: the threshold alone decides union and comp
    cx, cy = int(K_VSD[0, 2]), int(K_VSD[1, 2])
    for j, ((ox, oy), c) in enumerate(EXACT.items()):
        x, y = cx + ox, cy + oy
        de = np.float32(1 + rng.integers(0, 256) / 1024)
        gap = np.float32(2.0 ** -5 if j % 2 == 0 else 2.0 ** -7)                           # on a tau without / with the diameter
        d_est[y, x], d_gt[y, x] = (de, de + gap) if j % 4 < 2 else (de + gap, de)
        d_test[y, x] = np.float32(max(d_est[y, x], d_gt[y, x]) + 2.0 ** -8)              # in front of nothing: visible in both modes
        assert np.float64(dist32(d_gt[y, x], x, y)) == c * np.float64(d_gt[y, x])
    return d_test, d_gt, d_est


class Renderer:
    """stands in for the renderer of ``vsd``: hands out the prepared depth images, the estimate first (``pose_error.py:63-64``)"""

    def __init__(self, d_est, d_gt):
        self.images = [d_est, d_gt]

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        return {"depth": self.images.pop(0)}


def main():
    pe, misc, visibility = load_reference()
    out, meta = {}, {"sym_cases": [], "vsd_cases": []}
    for k, info in enumerate(MODEL_INFOS):
        syms = as34(misc.get_symmetry_transformations(info, STEP))
        out[f"info{k}/syms"] = syms
        print(f"model_info {k}: {len(syms)} transforms")
    out["model_infos"] = np.array(json.dumps(MODEL_INFOS))
    yaxis = as34(misc.get_axis_symmetry_transformations([0, 1, 0], STEP))
    out["axis_y/syms"] = yaxis
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])[None]
    y313 = as34(misc.get_axis_symmetry_transformations([0, 1, 0], np.pi / 313.5))
    sets = {"one": f32(eye), "two": f32(np.concatenate([eye, np.hstack([_rot([0, 1, 0], 180), np.zeros((3, 1))])[None]])),
            "y314": f32(np.concatenate([eye, y313]))}
    assert len(sets["y314"]) == 314
    for name, s in sets.items():
        out[f"sets/{name}"] = s
    j = 0
    for n in POINT_COUNTS:
        for name in SET_NAMES:
            case, pick = sym_case(n, 100 + j, sets[name])
            syms = [{"R": w64(s[:, :3]), "t": w64(s[:, 3]).reshape(3, 1)} for s in sets[name]]
            a = [w64(case["R_est"]), w64(case["t_est"]).reshape(3, 1), w64(case["R_gt"]), w64(case["t_gt"]).reshape(3, 1)]
            res = {"mssd": pe.mssd(*a, w64(case["pts"]), syms), "mspd": pe.mspd(*a, w64(case["K"]), w64(case["pts"]), syms),
                   "proj": pe.proj_sym(*a, w64(case["K"]), w64(case["pts"]), syms)}
            for key, v in case.items():
                out[f"s{j}/{key}"] = v
            for key, v in res.items():
                out[f"s{j}/{key}"] = np.float64(v)
            meta["sym_cases"].append({"n": n, "set": name, "pick": pick})
            print(f"sym case {j}: n {n} set {name} pick {pick} mssd {res['mssd']:.6f} mspd {res['mspd']:.4f} proj {res['proj']:.4f}")
            j += 1
    plain_gt, plain_est = visibility.estimate_visib_mask_gt, visibility.estimate_visib_mask_est
    j = 0
    for mode in ("bop19", "bop18"):
        for normalized in (False, True):
            for empty in (False, True):
                if empty and (normalized or mode == "bop18"):
                    continue
                d_test, d_gt, d_est = vsd_images(200 + j, empty)
                if mode == "bop18":
                    visibility.estimate_visib_mask_gt = lambda a, b, c, visib_mode=None: plain_gt(a, b, c, visib_mode="bop18")
                    visibility.estimate_visib_mask_est = lambda a, b, v, c, visib_mode=None: plain_est(a, b, v, c, visib_mode="bop18")
                try:
                    errs = pe.vsd(None, None, None, None, d_test, w64(K_VSD), DELTA, list(TAUS), normalized, DIAMETER,
                                  Renderer(d_est, d_gt), 1, cost_type="step")
                finally:
                    visibility.estimate_visib_mask_gt, visibility.estimate_visib_mask_est = plain_gt, plain_est
                # the counts behind the errors, from the same reference functions (pose_error.py:85-118 composed by hand)
                dist = [misc.depth_im_to_dist_im_fast(d, w64(K_VSD)) for d in (d_test, d_gt, d_est)]
                vis_gt = visibility.estimate_visib_mask_gt(dist[0], dist[1], DELTA, visib_mode=mode)
                vis_est = visibility.estimate_visib_mask_est(dist[0], dist[2], vis_gt, DELTA, visib_mode=mode)
                inter, union = np.logical_and(vis_gt, vis_est), np.logical_or(vis_gt, vis_est)
                dd = np.abs(dist[1][inter] - dist[2][inter]) / (DIAMETER if normalized else 1.0)
                counts = np.array([union.sum(), inter.sum()] + [(dd >= tau).sum() for tau in TAUS], np.int64)
                want = [1.0] * len(TAUS) if counts[0] == 0 else [(c + counts[0] - counts[1]) / float(counts[0]) for c in counts[2:]]
                assert list(errs) == want, (errs, want)
                for key, v in (("d_test", d_test), ("d_gt", d_gt), ("d_est", d_est), ("errors", np.asarray(errs, np.float64)),
                               ("counts", counts)):
                    out[f"v{j}/{key}"] = v
                meta["vsd_cases"].append({"mode": mode, "normalized": normalized, "empty": empty})
                print(f"vsd case {j}: {mode} normalized {normalized} empty {empty} errors {np.round(errs, 4).tolist()}")
                j += 1
    out["vsd/K"], out["vsd/taus"] = K_VSD, np.asarray(TAUS, np.float64)
    out["vsd/delta"], out["vsd/diameter"] = np.float32(DELTA), np.float64(DIAMETER)
    meta["source"] = ("lib/pysixd/misc.py get_symmetry_transformations :234-282, get_axis_symmetry_transformations :220-231; "
                      "pose_error.py mssd :131-153, mspd :156-179, proj_sym :196-217, vsd :22-128")
    meta["step"] = STEP
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
