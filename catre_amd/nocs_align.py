"""Initial pose and scale of every instance from a NOCS coordinate map, on the device: the RANSAC-wrapped Umeyama
similarity fit the reference's init-pose files were produced with (``preprocess/pose_data.py:56-165``:
``estimateSimilarityUmeyama`` / ``estimateSimilarityTransform``; invalid instances get what ``align_nocs_to_depth``
substitutes, ``:38-47``) for a ragged batch of instances, over ``catre_umeyama`` / ``catre_nocs_align``
(``csrc/catre_align.h``).  Inputs fp32, arithmetic and results float64.

With the reference's draws (``draws``: a replayed ``np.random.randint(n, size=5)`` stream) the discrete results are the
reference's; without, the draws come from a counter-based generator evaluated on the device - equally distributed, a
different stream (the contract of ``pcl_prep``'s ``sample="device"``), keyed by ``seed`` and a key per instance, so an
instance's result does not depend on the batch around it.  Not reproduced: the reference raises for fewer than five
points and returns NaN for non-finite input; both come back as invalid instances here.

:func:`init_from_frames` chains the pieces: depth maps + a NOCS coordinate map per frame -> clouds
(``pcl_prep.sample_frames``) -> ``obj_pose_est`` / ``obj_scale_est``, with no host round trip."""
import ctypes
from collections import namedtuple

import torch

from . import hip, pcl_prep

MAX_ITER, CONFIDENCE, MIN_INLIER_RATIO = 128, 0.99, 0.1   # pose_data.py:121-122, :151
ABI_CALLS = {"catre_umeyama": 0, "catre_nocs_align": 0, "catre_nocs_align_draws": 0, "catre_nocs_align_workspace_bytes": 0}
_U64 = 2 ** 64 - 1

Similarity = namedtuple("Similarity", "scale R t valid n_inliers iters best_it inliers")


def abi_call_count():
    """C-ABI calls made by this module so far (constant per batch, whatever the number of instances)."""
    return sum(ABI_CALLS.values())


def _call(name, *args):
    ABI_CALLS[name] += 1
    hip.check(getattr(hip.load(), name)(*args), name)


def _pairs(src, dst):
    hip.load()
    src = hip.require_dev_f32(src, "src", (None, None, 3), contiguous=False).contiguous()
    dst = hip.require_dev_f32(dst, "dst", tuple(src.shape), contiguous=False).contiguous()
    if dst.device != src.device:
        raise ValueError("src and dst must be on one device")
    if src.shape[0] == 0 or src.shape[1] == 0:
        raise ValueError(f"src / dst must hold at least one instance and one row, got {tuple(src.shape)}")
    return src, dst


def _i32(t, name, shape, dev):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if not t.is_cuda:
        raise hip.CatreHipError(f"{name} is on {t.device}; catre_amd runs on HIP devices only (no CPU fallback)")
    if t.device != dev or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)} on {dev}, got {tuple(t.shape)} on {t.device}")
    return t.to(torch.int32).contiguous()


def _keys(keys, I, dev):
    if keys is None:
        return None
    if not isinstance(keys, torch.Tensor):
        keys = torch.as_tensor(keys, dtype=torch.int64)
    if tuple(keys.shape) != (I,):
        raise ValueError(f"keys: expected {I} values, got {tuple(keys.shape)}")
    return keys.to(device=dev, dtype=torch.int64).contiguous()


def _check_iter(max_iter):
    if not 1 <= int(max_iter) <= MAX_ITER:
        raise ValueError(f"max_iter must lie in 1..{MAX_ITER}, got {max_iter}")
    return int(max_iter)


def umeyama(src, dst, counts=None, mask=None):
    """The least-squares similarity of ``estimateSimilarityUmeyama``: src, dst [I,N,3] fp32 on the device, ``counts`` [I]
    (rows used per instance; default all), ``mask`` [I,N] bool / uint8 (rows kept; default all) -> (scale [I], R [I,3,3],
    t [I,3]) float64 with ``dst ~ scale * R @ src + t``.  An instance without a kept row gives the identity."""
    src, dst = _pairs(src, dst)
    I, N, dev = src.shape[0], src.shape[1], src.device
    counts = _i32(counts, "counts", (I,), dev)
    if mask is not None:
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (I, N) or mask.device != dev:
            raise ValueError(f"mask must be [{I},{N}] bool / uint8 on the points' device")
        mask = mask.to(torch.uint8).contiguous()
    scale = torch.empty(I, dtype=torch.float64, device=dev)
    R = torch.empty(I, 3, 3, dtype=torch.float64, device=dev)
    t = torch.empty(I, 3, dtype=torch.float64, device=dev)
    _call("catre_umeyama", hip.ptr(src), hip.ptr(dst), hip.ptr(counts), hip.ptr(mask), I, N, hip.ptr(scale), hip.ptr(R),
          hip.ptr(t), None, hip.stream_ptr(dev))
    return scale, R, t


def draw_indices(counts, seed=0, keys=None, max_iter=MAX_ITER):
    """The draws ``estimate_similarity(draws=None, seed=..., keys=...)`` uses: counts [I] int32 on the device ->
    int32 [I,max_iter,5], draw j of iteration ``it`` of instance i = mulhi32(word j of Philox4x32-10 at counter
    (keys[i], it, word block) under key ``seed``, counts[i]).  ``keys`` default to 0..I-1."""
    max_iter = _check_iter(max_iter)
    hip.load()
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda:
        raise hip.CatreHipError("counts must be a tensor on a HIP device (no CPU fallback)")
    I, dev = counts.shape[0], counts.device
    counts = _i32(counts, "counts", (I,), dev)
    keys = _keys(keys, I, dev)
    out = torch.empty(I, max_iter, 5, dtype=torch.int32, device=dev)
    _call("catre_nocs_align_draws", hip.ptr(counts), int(seed) & _U64, hip.ptr(keys), I, max_iter, hip.ptr(out),
          hip.stream_ptr(dev))
    return out


def estimate_similarity(src, dst, counts=None, *, draws=None, seed=0, keys=None, max_iter=MAX_ITER, confidence=CONFIDENCE,
                        min_inlier_ratio=MIN_INLIER_RATIO, return_inliers=False):
    """``estimateSimilarityTransform`` for I instances: src [I,N,3] (NOCS coordinates in [-0.5, 0.5]), dst [I,N,3] (camera
    points) fp32 on the device, instance i uses its first ``counts[i]`` rows (default N; the others are never read).

    ``draws`` [I,max_iter,5] int32: the five indices of every iteration (the reference's stream replayed); None: evaluated
    on the device from ``seed`` and ``keys`` [I] (int64, default 0..I-1), see :func:`draw_indices`.

    -> ``Similarity``: scale [I], R [I,3,3], t [I,3] float64; valid [I], n_inliers [I] (of the best hypothesis), iters [I]
    (iterations evaluated), best_it [I] (-1: none) int32; inliers [I,N] uint8 with ``return_inliers`` (else None).  An
    invalid instance (best inlier ratio below ``min_inlier_ratio``, fewer than five rows, non-finite input) has scale 1,
    R = I, t = 0.  No host synchronisation, no device->host copy."""
    max_iter = _check_iter(max_iter)
    src, dst = _pairs(src, dst)
    I, N, dev = src.shape[0], src.shape[1], src.device
    counts = _i32(counts, "counts", (I,), dev)
    draws = _i32(draws, "draws", (I, max_iter, 5), dev)
    keys = _keys(keys, I, dev)
    lib = hip.load()
    ABI_CALLS["catre_nocs_align_workspace_bytes"] += 1
    nbytes = lib.catre_nocs_align_workspace_bytes(I, N, max_iter)
    if nbytes == 0:
        raise ValueError(f"{I} instances of {N} rows are outside what the kernels index")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    scale = torch.empty(I, dtype=torch.float64, device=dev)
    R = torch.empty(I, 3, 3, dtype=torch.float64, device=dev)
    t = torch.empty(I, 3, dtype=torch.float64, device=dev)
    ints = torch.empty(4, I, dtype=torch.int32, device=dev)
    inl = torch.empty(I, N, dtype=torch.uint8, device=dev) if return_inliers else None
    _call("catre_nocs_align", hip.ptr(src), hip.ptr(dst), hip.ptr(counts), hip.ptr(draws), int(seed) & _U64, hip.ptr(keys), I,
          N, max_iter, float(confidence), float(min_inlier_ratio), hip.ptr(ws), nbytes, hip.ptr(scale), hip.ptr(R), hip.ptr(t),
          hip.ptr(ints[0]), hip.ptr(ints[1]), hip.ptr(ints[2]), hip.ptr(ints[3]), hip.ptr(inl), hip.stream_ptr(dev))
    return Similarity(scale, R, t, ints[0], ints[1], ints[2], ints[3], inl)


def init_pose_from_nocs(pcl, nocs, extents, counts=None, **kw):
    """pcl [I,N,3] (camera points, metres), nocs [I,N,3] (their NOCS coordinates in [-0.5, 0.5]), extents [I,3] (box extents
    of the normalised model) fp32 on the device -> (obj_pose_est [I,3,4] = [R | t], obj_scale_est [I,3] = s * extents, both
    fp32, valid [I] bool): the reference's convention (``datasets/nocs.py:311-329``: ``abs_scale = extent * nocs_scale``;
    ``tools/prepare_spd_init_results.py:61-65``).  An invalid instance gets the identity rotation, t = 0 and scale = extents.
    ``counts`` and ``**kw`` go to :func:`estimate_similarity`."""
    kw.pop("return_inliers", None)
    sim = estimate_similarity(nocs, pcl, counts, **kw)
    I = sim.scale.shape[0]
    extents = hip.require_dev_f32(extents, "extents", (I, 3), contiguous=False)
    pose = torch.cat((sim.R, sim.t[:, :, None]), dim=2).to(torch.float32)
    scale = (sim.scale[:, None] * extents.to(torch.float64)).to(torch.float32)
    return pose, scale, sim.valid != 0


def init_from_frames(depth, K, frame_of, coord, *, labels=None, label_of=None, masks=None, extents, num_points=1024, seed=0,
                     **kw):
    """A data batch from depth maps to initial poses: depth [F,H,W] (fp32 metres), K, ``frame_of``, ``labels`` + ``label_of``
    or ``masks`` as :func:`pcl_prep.sample_frames` takes them, coord [F,H,W,3] fp32 = the NOCS coordinate map of every
    frame, already in [-0.5, 0.5] (``data_loader.py:435-439``), extents [I,3].  Samples ``num_points`` masked pixels per
    instance (``use_ball=False, sample="device"``, keyed by ``seed``), gathers ``coord`` at them and calls
    :func:`init_pose_from_nocs` (RANSAC draws keyed by ``seed`` too unless ``**kw`` says otherwise).  An instance with no
    candidate pixel is invalid.  -> (obj_pose_est [I,3,4], obj_scale_est [I,3], valid [I], pcl [I,num_points,3])."""
    if not isinstance(coord, torch.Tensor) or coord.ndim != 4 or coord.shape[-1] != 3 or tuple(coord.shape[:3]) != tuple(depth.shape):
        raise ValueError("coord must be a [F,H,W,3] tensor matching depth [F,H,W]")
    hip.require_dev_f32(coord, "coord", contiguous=False)
    I = len(frame_of)
    dev = depth.device
    pcl, pix, cand = pcl_prep.sample_frames(depth, K, frame_of, torch.zeros(I, 3, 4, device=dev), torch.ones(I, 3, device=dev),
                                            masks=masks, labels=labels, label_of=label_of, num_points=num_points,
                                            use_ball=False, sample="device", seed=seed, return_pixels=True)
    F, H, W = depth.shape
    fo = torch.as_tensor([int(v) for v in (frame_of.tolist() if isinstance(frame_of, torch.Tensor) else frame_of)],
                         dtype=torch.int64).to(dev)
    flat = fo[:, None] * (H * W) + pix.clamp(min=0).long()
    nocs = coord.contiguous().reshape(-1, 3)[flat]
    counts = torch.where(cand > 0, torch.full_like(cand, num_points), torch.zeros_like(cand))
    kw.setdefault("seed", seed if isinstance(seed, int) else 0)
    pose, scale, valid = init_pose_from_nocs(pcl, nocs, extents, counts=counts, **kw)
    return pose, scale, valid, pcl
