"""Test helper (not a test): CPU restatements the frame-batch tests compare against.

* the loader's depth augmentation (``core/catre/datasets/data_loader.py:448-449, 530-543``,
  ``core/utils/depth_aug.py:5-23``) in numpy, with the draws made explicit - pinned bit for bit by
  ``tests/golden/depth_aug.npz`` (``tools/make_depth_aug_golden.py``);
* :func:`frames_loop`: a frame batch answered by looping ``oracle.pcl_oracle`` frame by frame.
"""
import os

import numpy as np
import torch

from oracle import pcl_oracle as PO
from tests.util import GOLDEN_DIR


def depth_aug_golden():
    z = np.load(os.path.join(GOLDEN_DIR, "depth_aug.npz"))
    return {k: z[k] for k in z.files}


def to_metres(raw, depth_div=1000.0):
    """uint16 -> float32 metres: a float32 division (the python scalar does not promote the array)"""
    return raw.astype("float32") / depth_div


def fill_holes(depth, draw):
    """zero pixels take their N(0, 0.1) draw (float64 rounded to float32 by the assignment); the median the reference
    adds is that of the zero pixels themselves, 0"""
    out = depth.copy()
    holes = depth == 0
    out[holes] = draw[holes]
    return out


def drop_pixels(depth, draw, ratio):
    """float32 times a boolean keep mask: dropped pixels become 0 with the sign of what was there"""
    return depth * (draw > ratio)


def add_noise(depth, level, draw):
    """depth > 0 pixels get level * draw added in float64, rounded to float32 by the assignment"""
    gauss = level * draw
    out = depth.copy()
    valid = depth > 0
    out[valid] = depth[valid] + gauss[valid]
    return out


def augment(raw_or_metres, fill=None, keep=None, ratio=None, level=None, gauss=None, depth_div=1000.0):
    """all stages of one frame: dict(metres, after_fill, after_drop, after_noise); a step whose draws are None is skipped"""
    d = to_metres(raw_or_metres, depth_div) if raw_or_metres.dtype == np.uint16 else raw_or_metres.astype(np.float32)
    out = {"metres": d}
    d = out["after_fill"] = fill_holes(d, fill) if fill is not None else d
    d = out["after_drop"] = drop_pixels(d, keep, ratio) if keep is not None else d
    out["after_noise"] = add_noise(d, level, gauss) if gauss is not None and level > 0 else d
    return out


PERM_SHAPES = ((48, 40), (72, 64))             # one ragged 4096-pixel chunk / one full chunk and a ragged one
PERM_POINTS = 64
PERM_SEEDS = (0, 2 ** 63 + 5)                  # the seed of frame 0 / of frame 1


def perm_scene(H, W, seed):
    """One small frame for the device-permutation pin (``tests/golden/pcl_device_perm.npz``) -> dict of CPU tensors: a wall
    at about 1 m with a few holes, three half-full random masks, and balls of three sizes - the first holds between 10
    and ``PERM_POINTS`` candidates (the list is tiled), the other two hold more."""
    g = torch.Generator().manual_seed(1000 * H + seed)
    depth = 1.0 + 0.05 * torch.rand(H, W, generator=g)
    depth[torch.rand(H, W, generator=g) < 0.03] = 0.0
    K = torch.tensor([[60.0, 0.0, W / 2 - 0.5], [0.0, 62.0, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    masks = torch.rand(3, H, W, generator=g) < 0.5
    poses = torch.zeros(3, 3, 4)
    for i, (u, v) in enumerate(((W / 4, H / 2), (W / 2, H / 2), (3 * W / 4, H / 3))):
        poses[i, :, :3] = torch.eye(3)
        poses[i, :, 3] = torch.tensor([(u - K[0, 2]) / K[0, 0] * 1.02, (v - K[1, 2]) / K[1, 1] * 1.02, 1.02])
    scales = torch.tensor([[0.1] * 3, [0.5] * 3, [0.3] * 3])
    return dict(depth=depth, K=K, masks=masks, poses=poses, scales=scales)


def perm_batch(H, W):
    """the two frames of a shape as ``sample_frames`` takes them, instances frame by frame"""
    sc = [perm_scene(H, W, f) for f in range(2)]
    cat = lambda k: torch.cat([s[k] for s in sc])
    return dict(depth=torch.stack([s["depth"] for s in sc]), K=torch.stack([s["K"] for s in sc]), frame_of=[0] * 3 + [1] * 3,
                masks=cat("masks"), poses=cat("poses"), scales=cat("scales"))


def device_perm_outputs(dev="cuda:0"):
    """``sample="device"`` of the build that is loaded, on both shapes and both crops -> {name: array}: per shape
    ``frames_*`` from one ``sample_frames`` call on the two frames and ``inst_*`` from ``sample_instances`` frame by frame
    (rows in the same order), each as counts, pixel indices and the points' bit patterns."""
    from catre_amd import pcl_prep

    bits = lambda t: t.cpu().contiguous().view(torch.int32).numpy().copy()
    out = {}
    for H, W in PERM_SHAPES:
        b = perm_batch(H, W)
        d = {k: v.to(dev) for k, v in b.items() if k not in ("K", "frame_of")}
        for ball in (True, False):
            kw = dict(num_points=PERM_POINTS, use_ball=ball, sample="device", return_pixels=True)
            got = {"frames": pcl_prep.sample_frames(d["depth"], b["K"], b["frame_of"], d["poses"], d["scales"], masks=d["masks"],
                                                    seed=list(PERM_SEEDS), **kw)}
            per = [pcl_prep.sample_instances(d["depth"][f], b["K"][f], d["masks"][3 * f:3 * f + 3], d["poses"][3 * f:3 * f + 3],
                                             d["scales"][3 * f:3 * f + 3], seed=PERM_SEEDS[f], **kw) for f in range(2)]
            got["inst"] = tuple(torch.cat([p[k] for p in per]) for k in range(3))
            for who, (pcl, pix, counts) in got.items():
                tag = f"{who}_{H}x{W}_{'ball' if ball else 'mask'}"
                out[tag + "_pcl_bits"], out[tag + "_pix"], out[tag + "_counts"] = bits(pcl), pix.cpu().numpy(), counts.cpu().numpy()
    return out


def frames_loop(depth, K, frame_of, masks, poses, scales, ratio=0.5, num_points=1024, use_ball=True, sample_idx=None,
                fps=False):
    """depth [F,H,W], K [3,3] / [F,3,3], masks [I,H,W] bool (CPU tensors) -> dict(counts [I], pcl [I,N,3], pix [I,N]):
    frame after frame, every instance of the frame in the order given, through ``oracle.pcl_oracle``.  The slot choice is
    ``sample_idx[i]`` if given, the farthest point order with ``fps``, else a fresh ``torch.randperm`` of the tiled
    list per instance (drawn frame by frame, as a loop over single frames consumes the generator)."""
    F = depth.shape[0]
    K = K.expand(F, 3, 3) if K.ndim == 2 else K
    I = len(frame_of)
    counts = torch.zeros(I, dtype=torch.int32)
    pcl = torch.zeros(I, num_points, 3)
    pix = torch.full((I, num_points), -1, dtype=torch.long)
    for f in range(F):
        for i in [j for j in range(I) if int(frame_of[j]) == f]:
            cand, bp = PO.candidates(depth[f], K[f], masks[i], poses[i], scales[i], ratio, use_ball=use_ball)
            counts[i] = len(cand)
            if len(cand) == 0:
                continue
            if sample_idx is not None:
                s = torch.as_tensor(sample_idx[i])
            elif fps:
                s = PO.fps_sample_idx(cand, bp, num_points)
            elif use_ball:
                s = torch.randperm(PO.tiled_length(len(cand), num_points))[:num_points]
            else:
                s = PO.random_sample_idx(len(cand), num_points)
            pcl[i], pix[i] = PO.sample(cand, bp, s)
    return dict(counts=counts, pcl=pcl, pix=pix)
