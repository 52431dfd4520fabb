"""Trimmed ICP on the device (``csrc/catre_icp.h``): moves a pose towards the observed points without the network - the
classical registration baseline, and the second candidate ``tracking.Tracker(recover="icp")`` falls back on.

Direction: observed point -> nearest posed prior point.  Of the candidates (rows below ``counts``, within ``tau`` if given,
finite) the ``trim`` share with the smallest squared distances is kept - exact ties to the lower indices - and the fp64
least-squares fit of the kept pairs (rigid, or a similarity with ``estimate_scale``) updates pose and scale.

* :func:`icp_step` - ``catre_icp_step``: one step from the neighbours ``tracking.nn_stats(..., return_nn=True)`` found.
* :func:`icp` - ``catre_icp``: ``n_iter`` rounds of neighbours + step and a final evaluation in ONE ABI call, no host
  synchronisation; bit-identical to the rounds issued one by one.

Status bits (sticky over the iterations; with any set, pose and scale pass through bit for bit): FEW (fewer than three rows
kept), DEGENERATE (the kept pairs fix no unique rotation), NONFINITE (pose, scale or fit)."""
from collections import namedtuple

import torch

from . import hip
from .tracking import _opt, _points

FEW, DEGENERATE, NONFINITE = 1, 2, 4      # CATRE_ICP_* of include/catre_hip.h
MAX_ITER = 256                            # CATRE_ICP_MAX_ITER
ABI_CALLS = {"catre_icp_workspace_bytes": 0, "catre_icp_step": 0, "catre_icp": 0}

ICPStep = namedtuple("ICPStep", "pose scale rmse kept status mask")
ICPResult = namedtuple("ICPResult", "pose scale rmse kept status")


def abi_call_count():
    """C-ABI calls made by this module so far (constant per call, whatever the number of instances and iterations)."""
    return sum(ABI_CALLS.values())


def _call(name, *args):
    ABI_CALLS[name] += 1
    hip.check(getattr(hip.load(), name)(*args), name)


def _check(pcl, kps, pose, scale, counts, tau, trim):
    """Shapes and values, before the device is touched -> I."""
    pcl = _points(pcl, "pcl")
    I = pcl.shape[0]
    _points(kps, "kps", I)
    if _opt(pose, "pose", (I, 3, 4)) is None or _opt(scale, "scale", (I, 3)) is None:
        raise ValueError("pose [I,3,4] and scale [I,3] are required")
    _opt(counts, "counts", (I,))
    if counts is not None and counts.dtype != torch.int32:
        raise ValueError(f"counts must be int32, got {counts.dtype}")
    if isinstance(tau, torch.Tensor):
        _opt(tau, "tau", (I,))
    trim = float(trim)
    if not (0.0 < trim <= 1.0):
        raise ValueError(f"trim must lie in (0, 1], got {trim}")
    return I


def _on_device(pcl, kps, pose, scale, counts, tau, I):
    """fp32 / int32, contiguous, one device -> (pcl, kps, pose, scale, counts, tau, dev)."""
    pcl = hip.require_dev_f32(pcl, "pcl", contiguous=False).contiguous()
    dev = pcl.device
    f32 = lambda t, name: hip.require_dev_f32(t, name, contiguous=False).contiguous()
    kps, pose, scale = f32(kps, "kps"), f32(pose, "pose"), f32(scale, "scale")
    if tau is not None and not isinstance(tau, torch.Tensor):
        tau = torch.full((I,), float(tau), dtype=torch.float32, device=dev)
    if tau is not None:
        tau = f32(tau, "tau")
    if counts is not None:
        if not counts.is_cuda:
            raise hip.CatreHipError(f"counts is on {counts.device}; catre_amd runs on HIP devices only")
        counts = counts.contiguous()
    for t, name in ((kps, "kps"), (pose, "pose"), (scale, "scale"), (tau, "tau"), (counts, "counts")):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, pcl on {dev}")
    return pcl, kps, pose, scale, counts, tau, dev


def icp_step(pcl, kps, pose, scale, nn, counts=None, tau=None, trim=0.7, estimate_scale=False, update=True,
             return_mask=False, status=None):
    """One trimmed-ICP step.  pcl [I,N,3] observed points, kps [I,M,3] prior, pose [I,3,4], scale [I,3]: fp32 on the device;
    ``nn``: the ``NNStats`` of ``tracking.nn_stats(pcl, kps, dst_pose=pose, dst_scale=scale, return_nn=True)`` (or the pair
    ``(nn_d2, nn_j)``).  counts [I] int32: rows of every instance in use (None: all); tau: a float or [I] fp32, absolute
    metres (None: no threshold); status [I] int32: the bits of earlier steps (None: zeros; not modified).

    -> ``ICPStep(pose, scale, rmse [I], kept [I] int32, status [I] int32, mask [I,N] uint8 or None)``, new tensors; rmse
    and kept describe the INCOMING pose.  ``update=False`` measures only: pose, scale and status come back as given."""
    I = _check(pcl, kps, pose, scale, counts, tau, trim)
    n_src, n_dst = pcl.shape[1], kps.shape[1]
    nn_d2, nn_j = (nn.nn_d2, nn.nn_j) if hasattr(nn, "nn_d2") else nn
    if _opt(nn_d2, "nn.nn_d2", (I, n_src)) is None or _opt(nn_j, "nn.nn_j", (I, n_src)) is None:
        raise ValueError("nn needs nn_d2 and nn_j [I,N]: tracking.nn_stats(..., return_nn=True)")
    if nn_j.dtype != torch.int32:
        raise ValueError(f"nn.nn_j must be int32, got {nn_j.dtype}")
    _opt(status, "status", (I,))
    if status is not None and status.dtype != torch.int32:
        raise ValueError(f"status must be int32, got {status.dtype}")
    hip.load()
    pcl, kps, pose, scale, counts, tau, dev = _on_device(pcl, kps, pose, scale, counts, tau, I)
    nn_d2 = hip.require_dev_f32(nn_d2, "nn.nn_d2", contiguous=False).contiguous()
    for t, name in ((nn_d2, "nn.nn_d2"), (nn_j, "nn.nn_j"), (status, "status")):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, pcl on {dev}")
    nn_j = nn_j.contiguous()
    rmse = torch.empty(I, dtype=torch.float32, device=dev)
    kept = torch.empty(I, dtype=torch.int32, device=dev)
    mask = torch.empty(I, n_src, dtype=torch.uint8, device=dev) if return_mask else None
    status = torch.zeros(I, dtype=torch.int32, device=dev) if status is None else status.clone()
    pose_out = torch.empty_like(pose) if update else None
    scale_out = torch.empty_like(scale) if update else None
    _call("catre_icp_step", hip.ptr(pcl), n_src, hip.ptr(counts), hip.ptr(kps), n_dst, hip.ptr(pose), hip.ptr(scale),
          hip.ptr(nn_d2), hip.ptr(nn_j), hip.ptr(tau), float(trim), int(bool(estimate_scale)), int(bool(update)), I,
          hip.ptr(pose_out), hip.ptr(scale_out), hip.ptr(rmse), hip.ptr(kept), hip.ptr(mask), hip.ptr(status),
          hip.stream_ptr(dev))
    return ICPStep(pose_out if update else pose, scale_out if update else scale, rmse, kept, status, mask)


def icp(pcl, kps, pose, scale, n_iter=20, counts=None, tau=None, tau_rel=None, trim=0.7, estimate_scale=False):
    """``n_iter`` trimmed-ICP iterations from (pose, scale) -> ``ICPResult(pose [I,3,4], scale [I,3], rmse [n_iter+1,I],
    kept [n_iter+1,I] int32, status [I] int32)``.  Row ``it`` of rmse / kept is measured before update ``it``; the last
    row is the fit of the returned pose.  ``tau``: a float or [I] fp32 in metres, fixed over the iterations; ``tau_rel``:
    ``tau = tau_rel * |scale|`` of the incoming scale, computed on the device (as ``tracking.fit_score``); not both.
    One ABI call after the workspace query, nothing read back."""
    I = _check(pcl, kps, pose, scale, counts, tau, trim)
    if tau is not None and tau_rel is not None:
        raise ValueError("give tau (metres) or tau_rel (a share of |scale|), not both")
    n_iter = int(n_iter)
    if not 0 <= n_iter <= MAX_ITER:
        raise ValueError(f"n_iter must lie in 0 .. {MAX_ITER}, got {n_iter}")
    n_src, n_dst = pcl.shape[1], kps.shape[1]
    lib = hip.load()
    if tau_rel is not None:
        hip.require_dev_f32(scale, "scale", contiguous=False)
        tau = float(tau_rel) * torch.linalg.vector_norm(scale, dim=1)
    pcl, kps, pose, scale, counts, tau, dev = _on_device(pcl, kps, pose, scale, counts, tau, I)
    ABI_CALLS["catre_icp_workspace_bytes"] += 1
    nbytes = lib.catre_icp_workspace_bytes(I, n_src, n_dst, n_iter)
    if nbytes == 0:
        raise ValueError(f"{I} instances of {n_src} x {n_dst} points are outside what the kernels index")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    pose_out, scale_out = torch.empty_like(pose), torch.empty_like(scale)
    rmse = torch.empty(n_iter + 1, I, dtype=torch.float32, device=dev)
    kept = torch.empty(n_iter + 1, I, dtype=torch.int32, device=dev)
    status = torch.zeros(I, dtype=torch.int32, device=dev)
    _call("catre_icp", hip.ptr(pcl), n_src, hip.ptr(counts), hip.ptr(kps), n_dst, hip.ptr(pose), hip.ptr(scale), hip.ptr(tau),
          float(trim), int(bool(estimate_scale)), n_iter, I, hip.ptr(pose_out), hip.ptr(scale_out), hip.ptr(rmse),
          hip.ptr(kept), hip.ptr(status), hip.ptr(ws), nbytes, hip.stream_ptr(dev))
    return ICPResult(pose_out, scale_out, rmse, kept, status)
