"""Point-cloud preparation on the device - what the reference's data loader does per instance on
the CPU (``core/catre/datasets/data_loader.py:576-603``): back-project the depth map, keep the instance's masked pixels
with depth > 0, crop a ball around the pose centre (radius grown x1.1 until it holds >= 10 points) and sample
``NUM_PCL`` of them (``core/utils/cat_data_utils.py:209-226,289-320,352-400``; ``lib/pysixd/misc.py:360-378``).

All instances of a frame go through four launches.  ``sample="host"`` draws ``torch.randperm`` per instance exactly
like the reference (same global-generator consumption, bit-identical clouds; costs one device->host copy of the
candidate counts); ``sample="device"`` uses a keyed permutation evaluated on the GPU (no host round trip, a different
but equally uniform sample without replacement).

A data batch goes through :func:`sample_frames`: every instance of every frame in the same four launches, with a camera,
a sampling seed and (for NOCS) a label image per frame, and at most one copy of the candidate counts per batch.  The
depth augmentation the loader applies before any cloud is cut (``INPUT.AUG_DEPTH``: fill holes, drop pixels, add noise -
``data_loader.py:530-543``, ``core/utils/depth_aug.py:5-23``) is :func:`augment_depth` / :func:`augment_depth_cfg`.
"""
import ctypes
import random

import numpy as np
import torch

from . import hip


def backproject_th(depth, K):
    """``lib/pysixd/misc.py:360-378``: organised cloud map [H,W,3] (plain tensor ops; not on the hot path)."""
    assert depth.ndim == 2, depth.ndim
    H, W = depth.shape
    Y, X = torch.meshgrid(torch.arange(H, device=depth.device, dtype=depth.dtype) - float(K[1][2]),
                          torch.arange(W, device=depth.device, dtype=depth.dtype) - float(K[0][2]), indexing="ij")
    return torch.stack((X * depth / float(K[0][0]), Y * depth / float(K[1][1]), depth), dim=2)


def _k9(K):
    K = torch.as_tensor(K, dtype=torch.float32).reshape(3, 3).cpu()
    return (ctypes.c_float * 9)(*[float(v) for v in K.reshape(-1)])


def _random_sample(n, npoint):
    """``random_sample`` of the reference (``cat_data_utils.py:322-329``), same random stream."""
    idx = torch.randperm(n)[:npoint]
    while len(idx) < npoint:
        idx = torch.cat((idx, _random_sample(n, npoint - len(idx))), dim=0)
    return idx


def _byte_masks(masks):
    """bool / uint8 masks -> the contiguous uint8 the kernels read"""
    return (masks.to(torch.uint8) if masks.dtype == torch.bool else masks).contiguous()


def _tiled(c, num_points):
    """``while len(idx) < num_points: idx = cat([idx, idx])``: the length of the tiled candidate list"""
    while c < num_points:
        c *= 2
    return c


def _require_candidates(counts, who=lambda j: "an instance"):
    for j, c in enumerate(counts):
        if c == 0:
            # the reference recurses with a 1.2x larger ratio for ever here (cat_data_utils.py:390-393)
            raise ValueError(f"{who(j)} has no masked pixel with depth > 0")


def _host_draws(counts, num_points, use_ball):
    """The reference's draws, instance by instance in the order given (= the data loader's loop order) -> [I,num_points].
    Ball crop: the candidate list is tiled until it holds num_points entries, then one permutation
    (cat_data_utils.py:301-309, 322-329); crop_mask_depth_image: random_sample tops a short list up with further
    permutations."""
    return torch.stack([torch.randperm(_tiled(c, num_points))[:num_points] if use_ball else _random_sample(c, num_points)
                        for c in counts])


def sample_instances(depth, K, masks, poses=None, scales=None, ratio=0.5, num_points=1024, use_ball=True, sample="host",
                     seed=0, fps_sample=False, return_pixels=False):
    """depth [H,W] (device fp32, metres), K 3x3, masks [I,H,W] bool/uint8 (or None: whole frame, I from poses),
    poses [I,3,4], scales [I,3] -> pcl [I,num_points,3] (+ flat pixel indices [I,num_points] with ``return_pixels``).
    ``use_ball=True`` = ``crop_ball_from_depth_image`` (``INPUT.SAMPLE_DEPTH_FROM_BALL``), ``False`` =
    ``crop_mask_depth_image``."""
    if sample not in ("host", "device"):
        raise ValueError(f"sample={sample!r}: expected 'host' or 'device'")
    lib = hip.load()
    depth = hip.require_dev_f32(depth.contiguous(), "depth")
    H, W = depth.shape
    dev = depth.device
    if masks is not None:
        if masks.dtype not in (torch.bool, torch.uint8) or masks.device != dev or masks.shape[1:] != (H, W):
            raise ValueError("masks must be [I,H,W] bool / uint8 on the depth map's device")
        masks = _byte_masks(masks)
        I = masks.shape[0]
    else:
        I = poses.shape[0]
    if poses is None or scales is None:
        if use_ball:
            raise ValueError("the ball crop needs poses and scales")
        poses = torch.zeros(I, 3, 4, device=dev)
        scales = torch.ones(I, 3, device=dev)
    poses = hip.require_dev_f32(poses.contiguous(), "poses", (I, 3, 4))
    scales = hip.require_dev_f32(scales.contiguous(), "scales", (I, 3))
    k9 = _k9(K)
    nbytes = lib.catre_pcl_workspace_bytes(I, H, W)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(I, dtype=torch.int32, device=dev)
    st = hip.stream_ptr(dev)
    hip.check(lib.catre_pcl_candidates(hip.ptr(depth), k9, hip.ptr(masks), hip.ptr(poses), hip.ptr(scales), float(ratio),
                                       int(bool(use_ball)), I, H, W, hip.ptr(ws), nbytes, hip.ptr(counts), st),
              "catre_pcl_candidates")
    sidx = None
    if fps_sample or sample == "host":
        cl = counts.cpu().tolist()
        _require_candidates(cl)
    if fps_sample:
        # INPUT.FPS_SAMPLE: farthest point sampling of the tiled candidate list (cat_data_utils.py:305-306 with
        # device="cpu" as the data loader passes -> farthest_points_torch.py:6-62), one workgroup per instance
        cap = max(_tiled(c, num_points) for c in cl)
        scratch = torch.empty(I * 4 * cap, dtype=torch.float32, device=dev)
        sidx = torch.empty(I, num_points, dtype=torch.int64, device=dev)
        hip.check(lib.catre_pcl_fps(hip.ptr(depth), k9, hip.ptr(ws), nbytes, I, H, W, num_points, hip.ptr(scratch), cap,
                                    hip.ptr(sidx), st), "catre_pcl_fps")
    elif sample == "host":
        sidx = _host_draws(cl, num_points, use_ball).to(dev)
    pcl = torch.empty(I, num_points, 3, dtype=torch.float32, device=dev)
    pix = torch.empty(I, num_points, dtype=torch.int32, device=dev) if return_pixels else None
    hip.check(lib.catre_pcl_sample(hip.ptr(depth), k9, hip.ptr(ws), nbytes, hip.ptr(sidx), int(seed) & (2**64 - 1), I, H, W,
                                   num_points, hip.ptr(pcl), hip.ptr(pix), st), "catre_pcl_sample")
    if return_pixels:
        return pcl, pix, counts
    return pcl


def crop_ball_from_depth_image(image, depth, mask, pose, scale, ratio, cam_intrinsics, coord=None, num_points=None,
                               device=None, fps_sample=False):
    """Single-instance signature of the reference (``cat_data_utils.py:380-400``) on top of :func:`sample_instances`;
    ``depth`` is the [H,W] depth map or the [H,W,3] cloud map the reference passes.  -> (rgb, pts, nocs)."""
    d = depth[..., 2] if depth.ndim == 3 else depth
    pcl, pix, _ = sample_instances(d, cam_intrinsics, mask[None], pose[None], scale[None], ratio=ratio,
                                   num_points=num_points, use_ball=True, sample="host", fps_sample=fps_sample,
                                   return_pixels=True)
    flat = pix[0].long()
    rgb = image.reshape(-1, image.shape[-1])[flat.to(image.device)] if image is not None else None
    nocs = coord.reshape(-1, 3)[flat.to(coord.device)] if coord is not None else None
    return rgb, pcl[0], nocs


# ---- a whole data batch ----------------------------------------------------------------------------------------------
ABI_CALLS = {"catre_pclf_workspace_bytes": 0, "catre_pclf_candidates": 0, "catre_pclf_sample": 0, "catre_pclf_fps": 0,
             "catre_depth_augment": 0}
DAUG_FILL, DAUG_DROP, DAUG_NOISE = 1, 2, 4    # CATRE_DAUG_* of include/catre_hip.h
_DAUG_FRAME = np.dtype([("drop_ratio", "<f8"), ("noise_level", "<f8"), ("key", "<u8"), ("flags", "<i4"), ("reserved", "<i4")])
_U64 = 2 ** 64 - 1


def abi_call_count():
    """C-ABI calls made by :func:`sample_frames` / :func:`augment_depth` so far (constant per batch, whatever the number
    of frames; see ``max_workspace_bytes`` for the one way it grows)."""
    return sum(ABI_CALLS.values())


def _call(name, *args):
    ABI_CALLS[name] += 1
    hip.check(getattr(hip.load(), name)(*args), name)


def _per_frame(v, F, name, cast):
    """scalar or F values -> list of F"""
    if isinstance(v, torch.Tensor):
        v = v.tolist()
    elif isinstance(v, np.ndarray):
        v = v.tolist()
    if isinstance(v, (list, tuple)):
        if len(v) != F:
            raise ValueError(f"{name}: expected one value or {F} (one per frame), got {len(v)}")
        return [cast(x) for x in v]
    return [cast(v)] * F


def sample_frames(depth, K, frame_of, poses, scales, masks=None, labels=None, label_of=None, ratio=0.5, num_points=1024,
                  use_ball=True, sample="device", seed=0, fps_sample=False, return_pixels=False,
                  max_workspace_bytes=1 << 30):
    """:func:`sample_instances` for a data batch: depth [F,H,W] (device fp32, metres), K [3,3] or [F,3,3], ``frame_of``
    (list / CPU tensor, [I]) = the frame of every instance, poses [I,3,4], scales [I,3] -> pcl [I,num_points,3]
    (+ pix [I,num_points], the pixel index inside the instance's frame, and counts [I] with ``return_pixels``).

    The pixels of an instance are given in exactly one of two forms: ``masks`` [I,H,W] bool / uint8, or ``labels``
    [F,H,W] uint8 / int32 (one label image per frame, as NOCS ships them) with ``label_of`` [I] (list / CPU tensor):
    instance i owns the pixels where ``labels[frame_of[i]] == label_of[i]``.

    ``seed``: an int (every frame) or F ints.  ``sample="device"`` keys the permutation by (seed of the frame, rank of the
    instance within its frame), so a frame gets the cloud ``sample_instances(..., sample="device", seed=...)`` gives it
    alone - bit for bit, like every other mode: per frame the kernels run the single-frame arithmetic.  Instances may come
    in any order.  ``sample="device"`` without ``fps_sample`` makes a fixed number of ABI calls and no device->host
    copy, whatever F and I; ``sample="host"`` and ``fps_sample=True`` copy the counts once per batch, and ``"host"`` draws
    ``torch.randperm`` instance by instance in the order given (with the instances listed frame by frame that consumes
    the global generator exactly as a loop of ``sample_instances`` over the frames does) and raises ``ValueError`` for
    an instance without candidates.  ``sample="device"`` gives such an instance zeros, pix -1 and count 0.

    The candidate lists take I*H*W ints of workspace.  If that exceeds ``max_workspace_bytes`` the instance list is cut
    into consecutive groups that fit (at least one instance each) and the results are concatenated: the number of ABI
    calls (and of count copies) then grows with I - with the number of groups - never with F."""
    if sample not in ("host", "device"):
        raise ValueError(f"sample={sample!r}: expected 'host' or 'device'")
    if not isinstance(depth, torch.Tensor) or depth.ndim != 3:
        raise ValueError("depth must be a [F,H,W] tensor")
    F, H, W = depth.shape
    if (masks is None) == (labels is None):
        raise ValueError("give exactly one of masks [I,H,W] and labels [F,H,W] (+ label_of [I])")
    fo = [int(v) for v in (frame_of.tolist() if isinstance(frame_of, (torch.Tensor, np.ndarray)) else frame_of)]
    I = len(fo)
    if I == 0:
        raise ValueError("frame_of is empty: no instance to sample")
    for i, f in enumerate(fo):
        if not 0 <= f < F:
            raise ValueError(f"frame_of[{i}] = {f} is outside the {F} frames of depth")
    Kt = torch.as_tensor(K, dtype=torch.float32).cpu()
    if tuple(Kt.shape) == (3, 3):
        Kt = Kt.expand(F, 3, 3)
    elif tuple(Kt.shape) != (F, 3, 3):
        raise ValueError(f"K must be [3,3] or [{F},3,3], got {tuple(Kt.shape)}")
    seeds = _per_frame(seed, F, "seed", lambda v: int(v) & _U64)
    if labels is not None:
        if label_of is None:
            raise ValueError("labels needs label_of [I]: the label id of every instance")
        lo = [int(v) for v in (label_of.tolist() if isinstance(label_of, (torch.Tensor, np.ndarray)) else label_of)]
        if len(lo) != I:
            raise ValueError(f"label_of holds {len(lo)} ids for {I} instances")
        if labels.dtype not in (torch.uint8, torch.int32) or tuple(labels.shape) != (F, H, W):
            raise ValueError(f"labels must be [{F},{H},{W}] uint8 / int32")
    else:
        if label_of is not None:
            raise ValueError("label_of goes with labels, not with masks")
        if masks.dtype not in (torch.bool, torch.uint8) or tuple(masks.shape) != (I, H, W):
            raise ValueError(f"masks must be [{I},{H},{W}] bool / uint8")
    if poses is None or scales is None:
        raise ValueError("sample_frames needs poses [I,3,4] and scales [I,3]")

    lib = hip.load()
    depth = hip.require_dev_f32(depth.contiguous(), "depth")
    dev = depth.device
    if labels is not None:
        if labels.device != dev:
            raise ValueError("labels must be on the depth maps' device")
        labels = labels.contiguous()
        label_bytes = labels.element_size()
    else:
        if masks.device != dev:
            raise ValueError("masks must be on the depth maps' device")
        masks = _byte_masks(masks)
        label_bytes = 0
    poses = hip.require_dev_f32(poses.contiguous(), "poses", (I, 3, 4))
    scales = hip.require_dev_f32(scales.contiguous(), "scales", (I, 3))
    k9 = (ctypes.c_float * (9 * F))(*[float(v) for v in Kt.reshape(-1)])
    seeds_c = (ctypes.c_uint64 * F)(*seeds)
    seen, ranks = [0] * F, []
    for f in fo:   # rank of an instance within its frame, over the whole batch (groups below pass their slice)
        ranks.append(seen[f])
        seen[f] += 1

    def ws_bytes(n):
        ABI_CALLS["catre_pclf_workspace_bytes"] += 1
        return lib.catre_pclf_workspace_bytes(F, n, H, W)

    group, nbytes = I, ws_bytes(I)
    if nbytes > max_workspace_bytes and I > 1:
        lo_g, hi_g = 1, I          # largest group whose workspace fits (the size grows with the group); at least 1
        while hi_g - lo_g > 1:
            mid = (lo_g + hi_g) // 2
            lo_g, hi_g = (mid, hi_g) if ws_bytes(mid) <= max_workspace_bytes else (lo_g, mid)
        group, nbytes = lo_g, ws_bytes(lo_g)
    if nbytes == 0:
        raise ValueError(f"frames of {H}x{W} are outside what the kernels index (H*W < 2^30)")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(I, dtype=torch.int32, device=dev)
    pcl = torch.empty(I, num_points, 3, dtype=torch.float32, device=dev)
    pix = torch.empty(I, num_points, dtype=torch.int32, device=dev) if return_pixels else None
    st = hip.stream_ptr(dev)
    i32 = lambda vals: (ctypes.c_int32 * len(vals))(*vals)
    for s in range(0, I, group):
        e = min(I, s + group)
        n = e - s
        nb = nbytes if n == group else ws_bytes(n)
        fo_c = i32(fo[s:e])
        _call("catre_pclf_candidates", hip.ptr(depth), k9, fo_c, hip.ptr(masks[s:e]) if masks is not None else None,
              hip.ptr(labels), label_bytes, i32(lo[s:e]) if labels is not None else None, hip.ptr(poses[s:e]),
              hip.ptr(scales[s:e]), float(ratio), int(bool(use_ball)), F, n, H, W, hip.ptr(ws), nb, hip.ptr(counts[s:e]), st)
        sidx = None
        if fps_sample or sample == "host":
            cl = counts[s:e].cpu().tolist()   # the one device->host copy of the batch (of the group)
            _require_candidates(cl, lambda j: f"instance {s + j} (frame {fo[s + j]})")
        if fps_sample:
            cap = max(_tiled(c, num_points) for c in cl)
            scratch = torch.empty(n * 4 * cap, dtype=torch.float32, device=dev)
            sidx = torch.empty(n, num_points, dtype=torch.int64, device=dev)
            _call("catre_pclf_fps", hip.ptr(depth), k9, fo_c, hip.ptr(ws), nb, F, n, H, W, num_points, hip.ptr(scratch), cap,
                  hip.ptr(sidx), st)
        elif sample == "host":   # the draws of sample_instances, instance by instance in the order given
            sidx = _host_draws(cl, num_points, use_ball).to(dev)
        _call("catre_pclf_sample", hip.ptr(depth), k9, fo_c, i32(ranks[s:e]), hip.ptr(ws), nb, hip.ptr(sidx), seeds_c, F, n,
              H, W, num_points, hip.ptr(pcl[s:e]), hip.ptr(pix[s:e]) if return_pixels else None, st)
    if return_pixels:
        return pcl, pix, counts
    return pcl


def augment_depth(depth, *, fill_holes, drop, drop_ratio, noise_level, seed=0, frame_keys=None, draws=None, depth_div=None):
    """The loader's depth augmentation (``INPUT.AUG_DEPTH``; ``data_loader.py:530-543``, ``core/utils/depth_aug.py:5-23``)
    of a batch in one launch: depth [F,H,W] on the device, fp32 metres or uint16 (converted as ``(float)v / depth_div``,
    default 1000 = the loader's ``depth.astype("float32") / 1000.0``, bit for bit) -> a new fp32 [F,H,W].  Per frame, in
    the loader's order: ``fill_holes`` (bool, or one per frame) replaces ``depth == 0`` by a draw from N(0, 0.1) (negative
    fills stay and fail the ``depth > 0`` test of the sampling, as in the reference); ``drop`` (a bool per frame) multiplies by
    ``u > drop_ratio``, u ~ U(0,1); ``noise_level`` (a float per frame, 0 = off) adds ``noise_level * N(0,1)`` where the
    depth is > 0 after the first two steps.

    Two contracts.  With ``draws`` - a dict of float64 [F,H,W] device tensors ``fill`` / ``keep`` / ``gauss`` holding
    numpy's draws at the pixels that consume one - the result is the reference's bit for bit.  Without, the randomness
    is a counter-based generator evaluated per (``seed``, ``frame_keys[f]``, pixel, step): equally distributed, a
    different stream than numpy's (the contract of ``sample="device"``); a frame's result depends on its seed and key
    only (default keys: 0..F-1), not on the batch around it."""
    if not isinstance(depth, torch.Tensor) or depth.ndim != 3:
        raise ValueError("depth must be a [F,H,W] tensor")
    if depth.dtype not in (torch.float32, torch.uint16):
        raise ValueError(f"depth must be float32 (metres) or uint16, got {depth.dtype}")
    is_u16 = depth.dtype == torch.uint16
    if not is_u16 and depth_div is not None:
        raise ValueError("depth_div goes with uint16 depth; float32 depth is in metres already")
    div = float(1000.0 if depth_div is None else depth_div)
    if not div > 0:
        raise ValueError(f"depth_div must be > 0, got {depth_div}")
    F, H, W = depth.shape
    fill_l = _per_frame(fill_holes, F, "fill_holes", bool)
    drop_l = _per_frame(drop, F, "drop", bool)
    ratio_l = _per_frame(drop_ratio, F, "drop_ratio", float)
    level_l = _per_frame(noise_level, F, "noise_level", float)
    keys = list(range(F)) if frame_keys is None else _per_frame(list(frame_keys), F, "frame_keys", lambda v: int(v) & _U64)
    if any(not 0.0 <= r <= 1.0 for r in ratio_l) or any(not l >= 0.0 for l in level_l):
        raise ValueError("drop_ratio must lie in [0, 1] and noise_level must be >= 0")
    table = np.zeros(F, dtype=_DAUG_FRAME)
    table["drop_ratio"], table["noise_level"], table["key"] = ratio_l, level_l, keys
    table["flags"] = [DAUG_FILL * fi + DAUG_DROP * dr + DAUG_NOISE * (lv > 0) for fi, dr, lv in zip(fill_l, drop_l, level_l)]
    if draws is not None:
        unknown = set(draws) - {"fill", "keep", "gauss"}
        if unknown:
            raise ValueError(f"draws: unknown keys {sorted(unknown)} (expected fill / keep / gauss)")
        for key, flag in (("fill", DAUG_FILL), ("keep", DAUG_DROP), ("gauss", DAUG_NOISE)):
            t = draws.get(key)
            if t is None:
                if (table["flags"] & flag).any():
                    raise ValueError(f"draws has no {key!r} array but a frame runs that step")
            elif t.dtype != torch.float64 or tuple(t.shape) != (F, H, W):
                raise ValueError(f"draws[{key!r}] must be float64 [{F},{H},{W}]")
    hip.load()
    if not depth.is_cuda:
        raise hip.CatreHipError(f"depth is on {depth.device}; catre_amd runs on HIP devices only (no CPU fallback)")
    dev = depth.device
    depth = depth.contiguous()
    d = {}
    for key in ("fill", "keep", "gauss"):
        t = draws.get(key) if draws is not None else None
        if t is not None and t.device != dev:
            raise ValueError(f"draws[{key!r}] must be on the depth maps' device")
        d[key] = t.contiguous() if t is not None else None
    frames = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    out = torch.empty(F, H, W, dtype=torch.float32, device=dev)
    _call("catre_depth_augment", hip.ptr(depth), int(is_u16), div, hip.ptr(frames), int(draws is not None), hip.ptr(d["fill"]),
          hip.ptr(d["keep"]), hip.ptr(d["gauss"]), int(seed) & _U64, hip.ptr(out), F, H, W, hip.stream_ptr(dev))
    return out


def augment_depth_cfg(cfg, depth, seed=0, frame_keys=None):
    """``INPUT.AUG_DEPTH`` as the loader applies it (``data_loader.py:530-543``): returns ``depth`` itself unless
    ``cfg.INPUT.AUG_DEPTH``; otherwise draws per frame, in the loader's order, ``np.random.rand(1) < DROP_DEPTH_PROB``,
    ``np.random.rand(1) < ADD_NOISE_DEPTH_PROB`` and - only if the second coin came up - ``random.uniform(0,
    ADD_NOISE_DEPTH_LEVEL)`` (defaults 0.5 / 0.9 / 0.01, drop ratio 0.2: ``configs/_base_/common_base.py:34-39``), then
    calls :func:`augment_depth` with the hole filling on.

    The per-frame coins and level come from numpy's / ``random``'s global generators like the loader's; the per-pixel
    randomness is a different, equally distributed stream than numpy's (device mode of :func:`augment_depth`, keyed by
    ``seed`` and ``frame_keys``) - the contract of ``sample="device"``.  ``INPUT.BP_DEPTH`` (three-channel depth) is not
    implemented."""
    inp = cfg.INPUT
    if not inp.get("AUG_DEPTH", False):
        return depth
    if inp.get("BP_DEPTH", False):
        raise NotImplementedError("INPUT.BP_DEPTH=True (three-channel depth) is not augmented on the device")
    p_drop, p_noise = inp.get("DROP_DEPTH_PROB", 0.5), inp.get("ADD_NOISE_DEPTH_PROB", 0.9)
    ratio, level = inp.get("DROP_DEPTH_RATIO", 0.2), inp.get("ADD_NOISE_DEPTH_LEVEL", 0.01)
    drop, levels = [], []
    for _ in range(depth.shape[0]):
        drop.append(bool(np.random.rand(1) < p_drop))
        levels.append(random.uniform(0, level) if np.random.rand(1) < p_noise else 0.0)
    return augment_depth(depth, fill_holes=True, drop=drop, drop_ratio=ratio, noise_level=levels, seed=seed,
                         frame_keys=frame_keys)
