"""Fixture for the NOCS-map alignment (``catre_amd/nocs_align.py``), written by the UNMODIFIED reference (needs the
reference tree, see ``oracle/ref_shim.py``; never needed to build, test or run the product):

    python tools/make_align_golden.py            # tests/golden/nocs_align.npz

``preprocess/pose_data.py`` is loaded as it is (``oracle/ref_shim.install()`` stubs its ``cv2`` / ``mmcv`` / ``tqdm``
imports).  Its ``estimateSimilarityTransform`` (:109-165) is called on float32 inputs widened to float64 after
``np.random.seed(k)``; ``np.random.randint`` and ``estimateSimilarityUmeyama`` are wrapped with recorders while it runs,
which gives the draws, the number of iterations, every hypothesis and the inlier columns of the final fit.  The stream is
then re-seeded and drawn again (``np.random.randint(n, size=5)`` per iteration, nothing else) and must repeat the
recorded draws; it is drawn on to 128 iterations so that ``draws`` is a full table.

A case is (n, share of outliers): inliers are ``s R src + t`` with noise 1e-3 s, outliers are displaced by 1-2 object
diagonals.  Discrete choices must not depend on rounding, so a seed is skipped (the next one taken) unless, for every
hypothesis evaluated before the stop: (1) every residual is at least 1e-9 (relative) away from its threshold, (2) the
5-point covariance has sigma_2 / sigma_1 >= 1e-3 (five draws with replacement can hit two distinct points; the SVD is
then not unique), (3) the stop expression is at least 1e-9 away from 0.99.

``u/*`` holds plain ``estimateSimilarityUmeyama`` (:56-87) results: m = 5, 64, 65, 1000, a mirrored pair (the ``det < 0``
branch), a planar source (rank 2), a byte-mask and a ``counts`` variant.
"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "nocs_align.npz")
MAX_ITER, CONFIDENCE = 128, 0.99
MARGIN, MIN_SV_RATIO = 1e-9, 1e-3
# (n, share of outliers, first seed).  Seed 1 of (1024, 0.5) draws no all-inlier sample in 128 iterations (the chance of
# that is (31/32)^128 = 1.7 %) and ends valid at a ratio of 0.127; both that run and the next seed's are kept.
CASES = ((37, 0.2, 1), (63, 0.3, 1), (64, 0.3, 1), (65, 0.3, 1), (1000, 0.3, 1), (1024, 0.5, 1), (1024, 0.5, 2), (5000, 0.3, 1),
         (1024, 0.95, 1), (5, 0.0, 1), (0, 0.0, 1))


def load_reference():
    ref_shim.install()
    path = os.path.join(ref_shim.REFERENCE_ROOT, "preprocess", "pose_data.py")
    if not os.path.exists(path):
        raise RuntimeError(f"reference tree not found at {ref_shim.REFERENCE_ROOT}")
    spec = importlib.util.spec_from_file_location("ref_pose_data", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_case(n, outliers, seed):
    """-> src [n,3] fp32 in [-0.5, 0.5], dst [n,3] fp32 (metres), true inlier flags, (s, R, t)"""
    rng = np.random.default_rng(seed)
    ext = rng.uniform(0.25, 0.5, 3)                       # half extents of the normalised object
    ext *= 0.5 / np.linalg.norm(ext)                      # its diagonal is 1, as NOCS normalises
    src = (rng.uniform(-1, 1, (n, 3)) * ext).astype(np.float32)
    s, R = rng.uniform(0.15, 0.4), _rot(rng)
    t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.6, 1.4)])
    dst = s * src.astype(np.float64) @ R.T + t + rng.normal(0, 1e-3 * s, (n, 3))
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:int(round(outliers * n))]] = True
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dst[bad] += (d * rng.uniform(1.0, 2.0, (n, 1)) * s)[bad]   # the object's diagonal is s
    return src, dst.astype(np.float32), ~bad, (s, R, t)


def run_reference(mod, src, dst, seed):
    """One recorded call of the unmodified estimateSimilarityTransform -> dict, or None if a precondition fails."""
    n = len(src)
    s64, d64 = src.astype(np.float64), dst.astype(np.float64)
    drawn, fits = [], []
    orig_randint, orig_fit = np.random.randint, mod.estimateSimilarityUmeyama

    def randint(*a, **k):
        out = orig_randint(*a, **k)
        drawn.append(np.array(out))
        return out

    def fit(S, T):
        out = orig_fit(S, T)
        fits.append((np.array(S), np.array(T), out))
        return out

    np.random.seed(seed)
    np.random.randint, mod.estimateSimilarityUmeyama = randint, fit
    try:
        s, R, t, _ = mod.estimateSimilarityTransform(s64, d64, False)
    finally:
        np.random.randint, mod.estimateSimilarityUmeyama = orig_randint, orig_fit
    iters, none = len(drawn), s is None
    assert len(fits) == iters + (0 if none else 1)
    np.random.seed(seed)                                  # the stream is randint(n, size=5) per iteration, nothing else
    draws = np.stack([np.random.randint(n, size=5) for _ in range(MAX_ITER)]).astype(np.int32)
    assert np.array_equal(draws[:iters], np.stack(drawn))

    # distances to the discrete decisions, from the reference's own hypotheses
    SH, TH = np.vstack([s64.T, np.ones(n)]), np.vstack([d64.T, np.ones(n)])
    inlier_t = 2 * np.linalg.norm(s64.T - s64.mean(0)[:, None], axis=0).max() / 10.0
    best, best_it, best_set, margin, sv, stop_margin = 0.0, -1, np.arange(n), np.inf, np.inf, np.inf
    for it in range(iters):
        S5, T5, (scale, _, _, M) = fits[it]
        assert np.array_equal(S5, SH[:, draws[it]])
        thr = scale * inlier_t
        res = np.linalg.norm((TH - M @ SH)[:3], axis=0)
        if not np.isfinite(thr) or thr == 0:
            return None
        margin = min(margin, float(np.abs(res - thr).min() / abs(thr)))
        C = (T5[:3] - T5[:3].mean(1, keepdims=True)) @ (S5[:3] - S5[:3].mean(1, keepdims=True)).T / 5
        sig = np.linalg.svd(C, compute_uv=False)
        sv = min(sv, float(sig[1] / sig[0]))
        idx = np.where(res < thr)[0]
        if len(idx) / n > best:
            best, best_it, best_set = len(idx) / n, it, idx
        stop = 1 - (1 - best ** 5) ** it
        stop_margin = min(stop_margin, abs(stop - CONFIDENCE))
        assert (stop > CONFIDENCE) == (it == iters - 1 and iters < MAX_ITER) or it == MAX_ITER - 1
    assert none == (best < 0.1)
    if not none:
        assert np.array_equal(fits[-1][0], SH[:, best_set]) and np.array_equal(fits[-1][1], TH[:, best_set])
    if margin < MARGIN or sv < MIN_SV_RATIO or stop_margin < MARGIN:
        return None
    return dict(draws=draws, iters=iters, none=none, best_it=best_it, inliers=best_set.astype(np.int32), best_ratio=best,
                s=1.0 if none else float(s), R=np.eye(3) if none else np.array(R), t=np.zeros(3) if none else np.array(t),
                margin=margin, sv_ratio=sv, stop_margin=stop_margin)


def umeyama_cases(mod):
    """-> {name: dict(src, dst, count, mask, s, R, t)}: the reference's plain fit of the rows k < count with mask[k] set"""
    out = {}

    def add(name, src, dst, count=None, mask=None):
        src, dst = src.astype(np.float32), dst.astype(np.float32)
        count = len(src) if count is None else count
        mask = np.ones(len(src), np.uint8) if mask is None else mask.astype(np.uint8)
        keep = np.where(mask[:count] != 0)[0]
        S = np.vstack([src[keep].astype(np.float64).T, np.ones(len(keep))])
        T = np.vstack([dst[keep].astype(np.float64).T, np.ones(len(keep))])
        s, R, t, _ = mod.estimateSimilarityUmeyama(S, T)
        out[name] = dict(src=src, dst=dst, count=np.int32(count), mask=mask, s=np.float64(s), R=np.array(R), t=np.array(t))

    for m in (5, 64, 65, 1000):
        src, dst, _, _ = make_case(m, 0.0, 100 + m)
        dst = dst + np.random.default_rng(m).normal(0, 0.01, dst.shape).astype(np.float32)   # no exact similarity
        add(f"m{m}", src, dst)
    src, dst, _, _ = make_case(200, 0.0, 7)
    add("mirrored", src, dst * np.array([1, 1, -1], np.float32) + np.array([0, 0, 2], np.float32))
    src, dst, _, (s, R, t) = make_case(300, 0.0, 8)
    flat = src.copy()
    flat[:, 2] = 0
    add("planar", flat, (s * flat.astype(np.float64) @ R.T + t + np.random.default_rng(8).normal(0, 1e-3, flat.shape)))
    src, dst, _, _ = make_case(333, 0.2, 9)
    add("mask", src, dst, mask=np.random.default_rng(9).random(333) < 0.6)
    add("counts", src, dst, count=101)
    add("mask_counts", src, dst, count=200, mask=np.random.default_rng(10).random(333) < 0.5)
    return out


def main():
    mod = load_reference()
    arrays, meta = {}, dict(max_iter=MAX_ITER, confidence=CONFIDENCE, margin=MARGIN, min_sv_ratio=MIN_SV_RATIO, cases=[])
    for j, (n, outliers, seed) in enumerate(CASES):
        src, dst, true_in, (s, R, t) = make_case(n, outliers, 40 + j)
        pre = f"c{j}/"
        arrays.update({pre + "src": src, pre + "dst": dst, pre + "true_inlier": true_in.astype(np.uint8)})
        if n == 0:                                        # the reference raises here; the contract says invalid
            arrays.update({pre + "draws": np.zeros((MAX_ITER, 5), np.int32), pre + "inliers": np.zeros(0, np.int32),
                           pre + "s": np.float64(1), pre + "R": np.eye(3), pre + "t": np.zeros(3)})
            meta["cases"].append(dict(n=0, outliers=0.0, seed=None, iters=0, best_it=-1, none=True))
            continue
        while True:
            rec = run_reference(mod, src, dst, seed)
            print(f"case {j} n={n} outliers={outliers} seed={seed}", "SKIPPED" if rec is None else
                  {k: rec[k] for k in ("iters", "best_it", "none", "best_ratio", "margin", "sv_ratio", "stop_margin")})
            if rec is not None:
                break
            seed += 1
        if not rec["none"]:
            print("   exact true inlier set:", np.array_equal(np.where(true_in)[0], rec["inliers"]),
                  " |s - s_true| =", abs(rec["s"] - s))
        arrays.update({pre + k: rec[k] for k in ("draws", "inliers", "s", "R", "t")})
        meta["cases"].append(dict(n=n, outliers=outliers, seed=seed, iters=rec["iters"], best_it=rec["best_it"],
                                  none=bool(rec["none"]), best_ratio=rec["best_ratio"], margin=rec["margin"],
                                  sv_ratio=rec["sv_ratio"], stop_margin=rec["stop_margin"]))
    um = umeyama_cases(mod)
    for name, d in um.items():
        arrays.update({f"u/{name}/{k}": v for k, v in d.items()})
    meta["umeyama"] = list(um)
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(GOLDEN, **arrays)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
