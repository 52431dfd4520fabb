"""Row f3, one kernel body for two frame sources (``csrc/catre_pcl.h``: ``PclOneFrame`` behind ``catre_pcl_*``,
``PclFrameTable`` behind ``catre_pclf_*``).

* ``sample="device"`` has no reference to compare against, so it is pinned to what the library gave before the two kernel
  sets were merged: ``tests/golden/pcl_device_perm.npz`` (``tools/make_pcl_perm_golden.py``), byte for byte.
* For F = 1 and ``frame_of = 0`` the two sets of entry points must leave the same bits in the raw workspace (candidate
  lists, counts), in the farthest-point index table and in the device-mode cloud.
* A depth map with a ``+inf`` pixel in the camera's centre column makes every farthest-point distance NaN: both entry
  points then give the result the reference's ``argmax`` gives on an all-NaN tensor - index 0 - and indices in range.

Shapes: 48x40 (one ragged 4096-pixel chunk) and 72x64 (a full chunk and a ragged one), 64 points: one instance's list is
shorter than that (tiled) and the others are longer (the farthest-point loop runs)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from catre_amd import hip, pcl_prep
from oracle import pcl_oracle as PO
from tests import pcl_frames_ref as R
from tests.util import GOLDEN_DIR

DEV = "cuda:0"
N = R.PERM_POINTS


def _golden():
    z = np.load(os.path.join(GOLDEN_DIR, "pcl_device_perm.npz"))
    return {k: z[k] for k in z.files}


# ---- without a GPU --------------------------------------------------------------------------------------------------
def test_pinned_scenes_are_the_recorded_ones_and_reach_both_list_lengths():
    """The fixture's counts against the oracle on the scenes as this machine generates them (an input that drifted would
    show here, not as a kernel failure), and the coverage the pin is there for: with the ball crop every frame has a list
    of 10..63 candidates (tiled up to 64) and lists longer than 64."""
    g = _golden()
    for H, W in R.PERM_SHAPES:
        b = R.perm_batch(H, W)
        for ball in (True, False):
            want = [len(PO.candidates(b["depth"][f], b["K"][f], b["masks"][i], b["poses"][i], b["scales"][i], 0.5,
                                      use_ball=ball)[0]) for i, f in enumerate(b["frame_of"])]
            assert g[f"{H}x{W}_{'ball' if ball else 'mask'}_counts"].tolist() == want
            if ball:
                assert all(10 <= want[i] < N for i in (0, 3)) and all(want[i] > N for i in (1, 2, 4, 5)), want


# ---- on the GPU -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_permutation_keeps_the_recorded_bits():
    g = _golden()
    got = R.device_perm_outputs(DEV)
    assert sorted(got) == sorted(f"{who}_{k}" for who in ("frames", "inst") for k in g)
    for k in sorted(got):                                   # both entry points against the one recorded copy
        w = g[k.partition("_")[2]]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and got[k].tobytes() == w.tobytes(), k


def _up64(n):
    return (n + 63) // 64 * 64


class _Both:
    """One frame through the raw C ABI of both sets of entry points (F = 1, ``frame_of = 0``), each on its own
    zero-filled workspace; ``self.one`` / ``self.table`` hold what each left behind."""

    def __init__(self, sc, use_ball, num_points, seed=0):
        self.lib = hip.load()
        self.d = {k: sc[k].to(DEV).contiguous() for k in ("depth", "poses", "scales")}
        self.m8 = sc["masks"].to(torch.uint8).to(DEV).contiguous()
        self.I, (self.H, self.W) = self.m8.shape[0], sc["depth"].shape
        self.n, self.seed, self.use_ball = num_points, seed, int(use_ball)
        self.k9 = (ctypes.c_float * 9)(*[float(v) for v in sc["K"].reshape(-1)])
        self.fo = (ctypes.c_int32 * self.I)(*([0] * self.I))
        self.st = hip.stream_ptr(torch.device(DEV))
        self.one, self.table = self._run(False), self._run(True)

    def _run(self, table):
        lib, p, I, H, W, n, d = self.lib, hip.ptr, self.I, self.H, self.W, self.n, self.d
        single = lib.catre_pcl_workspace_bytes(I, H, W)
        nbytes = lib.catre_pclf_workspace_bytes(1, I, H, W) if table else single
        ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=DEV)
        counts = torch.full((I,), -7, dtype=torch.int32, device=DEV)
        if table:
            pre = (p(d["depth"]), self.k9, self.fo)
            hip.check(lib.catre_pclf_candidates(*pre, p(self.m8), None, 0, None, p(d["poses"]), p(d["scales"]), 0.5,
                                                self.use_ball, 1, I, H, W, p(ws), nbytes, p(counts), self.st), "candidates")
        else:
            pre = (p(d["depth"]), self.k9)
            hip.check(lib.catre_pcl_candidates(*pre, p(self.m8), p(d["poses"]), p(d["scales"]), 0.5, self.use_ball, I, H, W,
                                               p(ws), nbytes, p(counts), self.st), "candidates")
        cl = counts.cpu().tolist()
        cap = max(pcl_prep._tiled(max(c, 1), n) for c in cl)
        scratch = torch.zeros(I * 4 * cap, dtype=torch.float32, device=DEV)
        sidx = torch.full((I, n), -7, dtype=torch.int64, device=DEV)
        dims = (1, I, H, W, n) if table else (I, H, W, n)
        fps = lib.catre_pclf_fps if table else lib.catre_pcl_fps
        hip.check(fps(*pre, p(ws), nbytes, *dims, p(scratch), cap, p(sidx), self.st), "fps")
        out = dict(counts=counts, sidx=sidx, cap=cap)
        for mode, slots in (("fps", sidx), ("device", None)):
            pcl = torch.full((I, n, 3), -7.0, device=DEV)
            pix = torch.full((I, n), -7, dtype=torch.int32, device=DEV)
            if table:
                seeds = (ctypes.c_uint64 * 1)(self.seed)
                hip.check(lib.catre_pclf_sample(*pre, None, p(ws), nbytes, p(slots), seeds, *dims, p(pcl), p(pix), self.st),
                          "sample")
            else:
                hip.check(lib.catre_pcl_sample(*pre, p(ws), nbytes, p(slots), self.seed, *dims, p(pcl), p(pix), self.st),
                          "sample")
            out[mode + "_pcl"], out[mode + "_pix"] = pcl.view(torch.int32).cpu(), pix.cpu()
        torch.cuda.synchronize()
        # the single-frame layout (catre_pcl_api.inc: bins, choose, offsets, total, cand, each padded to 64 ints) is the
        # tail of the frame-batch workspace
        body = ws[(nbytes - single) // 4:].cpu()
        nchunks, HW = (H * W + 4095) // 4096, H * W
        at_total = _up64(I * nchunks * 12) + _up64(I) + _up64(I * nchunks)
        at_cand = at_total + _up64(I)
        assert at_cand + _up64(I * HW) == single // 4
        out.update(body=body, total=body[at_total:at_total + I], cand=body[at_cand:at_cand + I * HW].view(I, HW),
                   counts=counts.cpu(), sidx=sidx.cpu())
        return out


@pytest.mark.gpu
@pytest.mark.parametrize("use_ball", [True, False])
@pytest.mark.parametrize("H,W", R.PERM_SHAPES)
def test_both_frame_sources_leave_the_same_bits(H, W, use_ball):
    sc = R.perm_scene(H, W, 0)
    both = _Both(sc, use_ball, N, seed=R.PERM_SEEDS[1])
    a, b = both.one, both.table
    want = [PO.candidates(sc["depth"], sc["K"], sc["masks"][i], sc["poses"][i], sc["scales"][i], 0.5, use_ball=use_ball)[0]
            for i in range(3)]
    assert a["counts"].tolist() == [len(w) for w in want] and (a["counts"] > 0).all()
    for i, w in enumerate(want):                       # ... and the lists themselves are the oracle's
        assert a["cand"][i, :len(w)].tolist() == torch.as_tensor(w).reshape(-1).tolist()
    for k in ("counts", "total", "cand", "body", "sidx", "fps_pcl", "fps_pix", "device_pcl", "device_pix"):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert torch.equal(a["counts"], a["total"])
    assert ((a["sidx"] >= 0) & (a["sidx"] < both.one["cap"])).all()
    for k in ("fps_pix", "device_pix"):
        assert ((a[k] >= 0) & (a[k] < H * W)).all(), k


@pytest.mark.gpu
def test_non_finite_depth_gives_a_defined_farthest_point_order():
    """A ``+inf`` pixel in the column ``u == cx`` back-projects to x = 0 * inf = NaN: the centroid and with it every
    initial distance is NaN, so the first arg-max finds no maximum.  Both entry points must then pick index 0 (the
    reference's ``argmax`` of an all-NaN tensor) and stay inside the list and the frame."""
    H, W, n = 48, 40, 32
    g = torch.Generator().manual_seed(11)
    depth = 0.5 + 1.5 * torch.rand(H, W, generator=g)
    depth[10, 20] = float("inf")
    K = torch.tensor([[60.0, 0.0, 20.0], [0.0, 62.0, 23.5], [0.0, 0.0, 1.0]])
    masks = torch.zeros(1, H, W, dtype=torch.bool)
    masks[0, :, 16:25] = True
    sc = dict(depth=depth, K=K, masks=masks, poses=torch.eye(3, 4)[None].contiguous(), scales=torch.ones(1, 3))
    both = _Both(sc, False, n)
    a, b = both.one, both.table
    L = 9 * H
    assert a["counts"].tolist() == [L] and L > n            # longer than num_points: the farthest-point loop runs
    for r in (a, b):
        assert ((r["sidx"] >= 0) & (r["sidx"] < L)).all()
        assert ((r["fps_pix"] >= 0) & (r["fps_pix"] < H * W)).all()
        assert r["sidx"][0, 0] == 0
        assert len(set(r["sidx"][0].tolist())) == n         # after the fallback the order is a farthest-point order again
    for k in ("counts", "cand", "sidx", "fps_pcl", "fps_pix"):
        assert torch.equal(a[k], b[k]), k
    # the same through the public API
    d = {k: v.to(DEV) for k, v in sc.items() if k != "K"}
    kw = dict(num_points=n, use_ball=False, fps_sample=True, return_pixels=True)
    one = pcl_prep.sample_instances(d["depth"], K, d["masks"], **kw)
    tab = pcl_prep.sample_frames(d["depth"][None], K, [0], d["poses"], d["scales"], masks=d["masks"], **kw)
    bits = lambda t: t.view(torch.int32).cpu()                # the cloud holds NaNs: compare bit patterns
    assert torch.equal(one[1].cpu(), a["fps_pix"]) and torch.equal(bits(one[0]), a["fps_pcl"])
    for x, y in zip(one, tab):
        assert x.dtype == y.dtype and torch.equal(bits(x), bits(y))
