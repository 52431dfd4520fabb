"""Fixture for the pixel classes of the splat render (``catre_amd/render.py``), written by the UNMODIFIED reference (needs
the reference tree, see ``oracle/ref_shim.py``; never needed to build, test or run the product):

    python tools/make_render_golden.py            # tests/golden/visib_mask.npz

``lib/pysixd/visibility.py`` is loaded as it is (it imports numpy alone; the stand-in modules only give it the package
path it lives under) and ``estimate_visib_mask_gt(d_test, d_model, delta, mode)`` is recorded for ``bop18`` and ``bop19``.

The images are 24 x 32, seeded, every value fp32-representable: a rendered depth ``d_model`` with a background of zeros, an
observed depth ``d_test`` with holes (zeros), and rows of pixels that sit on the visibility threshold - ``d_model - d_test``
equal to ``+delta`` and ``-delta`` exactly and one ulp of ``d_model`` to either side of both.  ``delta = 2^-6`` m and
``d_test`` on a grid of 2^-10 m there, so that the fp32 difference the reference takes is exact."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "visib_mask.npz")
H, W, SEED, DELTA = 24, 32, 20, 2.0 ** -6


def load_reference():
    if not os.path.isdir(ref_shim.REFERENCE_ROOT):
        raise RuntimeError(f"reference tree not found at {ref_shim.REFERENCE_ROOT}")
    path = os.path.join(ref_shim.REFERENCE_ROOT, "lib", "pysixd", "visibility.py")
    for name in ("lib", "lib.pysixd"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("ref_visibility", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_images():
    rng = np.random.default_rng(SEED)
    d_model = rng.uniform(0.6, 1.4, (H, W)).astype(np.float32)
    d_test = (d_model + rng.normal(0, 0.02, (H, W)).astype(np.float32)).astype(np.float32)   # both sides of +-delta
    d_model[rng.random((H, W)) < 0.3] = 0                                                   # background
    d_test[rng.random((H, W)) < 0.15] = 0                                                   # holes
    # threshold rows: d_test on a 2^-10 grid in [1, 1.5), d_model = d_test +- delta, and one ulp to either side
    dl = np.float32(DELTA)
    for row, sign in ((4, 1), (12, -1)):
        base = (1 + rng.integers(0, 512, W) / 1024).astype(np.float32)
        on = (base + np.float32(sign) * dl).astype(np.float32)
        d_test[row:row + 3] = base
        d_model[row] = on
        d_model[row + 1] = np.nextafter(on, np.float32(np.inf))
        d_model[row + 2] = np.nextafter(on, np.float32(-np.inf))
        assert ((on - base) == np.float32(sign) * dl).all()
        assert ((d_model[row + 1] - base) != (on - base)).all() and ((d_model[row + 2] - base) != (on - base)).all()
    return d_test, d_model


def main():
    mod = load_reference()
    d_test, d_model = make_images()
    assert (d_test == 0).any() and (d_model == 0).any() and ((d_test == 0) & (d_model > 0)).any()
    out = {"d_test": d_test, "d_model": d_model, "delta": np.float32(DELTA)}
    for mode in ("bop18", "bop19"):
        mask = mod.estimate_visib_mask_gt(d_test, d_model, DELTA, mode)
        out[mode] = np.asarray(mask, bool)
        print(mode, int(mask.sum()), "visible of", int((d_model > 0).sum()), "rendered")
    out["meta"] = np.array(json.dumps({"seed": SEED, "source": "lib/pysixd/visibility.py estimate_visib_mask_gt :44-54"}))
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
