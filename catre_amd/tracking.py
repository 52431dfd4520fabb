"""Following objects through a depth sequence on the device: frame t's refined pose centres frame t+1's ball crop and is
its initial estimate (the paper's tracking experiment; why the reference trains with ``INIT_POSE_TYPE_TRAIN =
"last_frame"``), with a fit score after every refine and a gate that decides what a track carries on.

* :func:`nn_stats` - ``catre_nn_stats`` (``csrc/catre_track.h``): for a batch of point-set pairs, every src point's
  nearest dst point, the mean distance and the share of src points within ``tau``.  Also what ADD / ADD-S are made of
  (``evaluation.add_errors``).
* :func:`fit_score` - does the posed prior lie on the observed points?  Two calls: observed -> prior and prior -> observed.
* :func:`track_gate` - ``catre_track_gate``: status bits, carried pose / scale, age.
* :class:`Tracker` - ``pcl_prep.sample_frames`` -> ``model.refine`` -> :func:`fit_score` (-> with ``recover="icp"`` the
  trimmed-ICP candidate of ``catre_amd/icp.py`` and its score) -> :func:`track_gate`, state on
  the device, no device->host copy and a constant number of ABI calls per frame.  ``crop="render"`` crops with the depth-consistent
  mask of the carried pose's splat (``catre_amd/render.py``) instead of the ball alone.

Two contracts: a ``Tracker.step`` is bit-identical to that composition written out by hand, and an instance's results do
not depend on the batch around it (``nn_stats`` reduces in a fixed order, without atomics)."""
from collections import namedtuple

import torch

from . import hip, pcl_prep

EMPTY, LOW_FIT, NONFINITE = 1, 2, 4      # CATRE_TRACK_* of include/catre_hip.h
ABI_CALLS = {"catre_nn_stats_workspace_bytes": 0, "catre_nn_stats": 0, "catre_track_gate": 0}

NNStats = namedtuple("NNStats", "mean_d inlier nn_d2 nn_j")
FitScore = namedtuple("FitScore", "d_obs inlier_obs d_prior")


def abi_call_count():
    """C-ABI calls made by this module so far (constant per call, whatever the number of instances)."""
    return sum(ABI_CALLS.values())


def _call(name, *args):
    ABI_CALLS[name] += 1
    hip.check(getattr(hip.load(), name)(*args), name)


def _points(t, name, I=None):
    if not isinstance(t, torch.Tensor) or t.ndim != 3 or t.shape[-1] != 3:
        raise ValueError(f"{name}: expected a [I,n,3] tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError(f"{name}: needs at least one instance and one point, got {tuple(t.shape)}")
    if I is not None and t.shape[0] != I:
        raise ValueError(f"{name}: expected {I} instances, got {t.shape[0]}")
    return t


def _opt(t, name, shape):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a tensor of shape {tuple(shape)}, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    return t


def nn_stats(src, dst, src_pose=None, src_scale=None, dst_pose=None, dst_scale=None, paired=False, tau=None, return_nn=False):
    """src [I,n_src,3], dst [I,n_dst,3] fp32 on the device; a point x of a set with (pose [I,3,4], scale [I,3]) stands at
    ``R (s * x) + t`` (None: identity).  For every src point the nearest dst point (``paired``: dst point of the same
    index, n_src == n_dst), by fp32 squared distances of coordinate differences, the lowest index on an exact tie.

    -> ``NNStats``: mean_d [I] (mean distance), inlier [I] (share of src points with ``d^2 <= tau^2``; ``tau``: a float or
    [I] fp32 on the device; None without ``tau``), and with ``return_nn`` nn_d2 [I,n_src] (squared distances) and nn_j
    [I,n_src] int32.  Shapes are checked (``ValueError``) before the device is touched; no host synchronisation."""
    src = _points(src, "src")
    I = src.shape[0]
    dst = _points(dst, "dst", I)
    n_src, n_dst = src.shape[1], dst.shape[1]
    if paired and n_src != n_dst:
        raise ValueError(f"paired=True needs n_src == n_dst, got {n_src} and {n_dst}")
    src_pose, dst_pose = _opt(src_pose, "src_pose", (I, 3, 4)), _opt(dst_pose, "dst_pose", (I, 3, 4))
    src_scale, dst_scale = _opt(src_scale, "src_scale", (I, 3)), _opt(dst_scale, "dst_scale", (I, 3))
    if isinstance(tau, torch.Tensor):
        tau = _opt(tau, "tau", (I,))
    lib = hip.load()
    src = hip.require_dev_f32(src, "src", contiguous=False).contiguous()
    dev = src.device
    f32 = lambda t, name: None if t is None else hip.require_dev_f32(t, name, contiguous=False).contiguous()
    dst, src_pose, src_scale, dst_pose, dst_scale = (f32(t, n) for t, n in (
        (dst, "dst"), (src_pose, "src_pose"), (src_scale, "src_scale"), (dst_pose, "dst_pose"), (dst_scale, "dst_scale")))
    if tau is not None and not isinstance(tau, torch.Tensor):
        tau = torch.full((I,), float(tau), dtype=torch.float32, device=dev)
    tau = f32(tau, "tau")
    for t, name in ((dst, "dst"), (src_pose, "src_pose"), (src_scale, "src_scale"), (dst_pose, "dst_pose"),
                    (dst_scale, "dst_scale"), (tau, "tau")):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, src on {dev}")
    ABI_CALLS["catre_nn_stats_workspace_bytes"] += 1
    nbytes = lib.catre_nn_stats_workspace_bytes(I, n_src, n_dst)
    if nbytes == 0:
        raise ValueError(f"{I} instances of {n_src} x {n_dst} points are outside what the kernels index")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    mean_d = torch.empty(I, dtype=torch.float32, device=dev)
    inlier = torch.empty(I, dtype=torch.float32, device=dev) if tau is not None else None
    nn_d2 = torch.empty(I, n_src, dtype=torch.float32, device=dev) if return_nn else None
    nn_j = torch.empty(I, n_src, dtype=torch.int32, device=dev) if return_nn else None
    _call("catre_nn_stats", hip.ptr(src), n_src, hip.ptr(dst), n_dst, hip.ptr(src_pose), hip.ptr(src_scale), hip.ptr(dst_pose),
          hip.ptr(dst_scale), int(bool(paired)), hip.ptr(tau), I, hip.ptr(mean_d), hip.ptr(inlier), hip.ptr(nn_d2),
          hip.ptr(nn_j), hip.ptr(ws), nbytes, hip.stream_ptr(dev))
    return NNStats(mean_d, inlier, nn_d2, nn_j)


def fit_score(pcl, kps, pose, scale, tau_rel=0.1):
    """How well the prior ``kps`` [I,M,3] at (pose [I,3,4], scale [I,3]) lies on the observed points ``pcl`` [I,N,3] (camera
    frame) -> ``FitScore``, [I] fp32 each: d_obs = mean distance observed point -> nearest posed prior point, inlier_obs =
    share of observed points within ``tau = tau_rel * |scale|`` of the prior (the norm the ball radius of the crop uses,
    ``cat_data_utils.py:386``, with R orthonormal), d_prior = mean distance posed prior point -> nearest observed point.
    d_obs grows when the estimate drifts off the object; d_prior also grows where the object is occluded."""
    pcl = _points(pcl, "pcl")
    I = pcl.shape[0]
    kps = _points(kps, "kps", I)
    pose, scale = _opt(pose, "pose", (I, 3, 4)), _opt(scale, "scale", (I, 3))
    if pose is None or scale is None:
        raise ValueError("fit_score needs pose [I,3,4] and scale [I,3]")
    hip.require_dev_f32(scale, "scale", contiguous=False)
    tau = float(tau_rel) * torch.linalg.vector_norm(scale, dim=1)
    obs = nn_stats(pcl, kps, dst_pose=pose, dst_scale=scale, tau=tau)
    pri = nn_stats(kps, pcl, src_pose=pose, src_scale=scale)
    return FitScore(obs.mean_d, obs.inlier, pri.mean_d)


def track_gate(pose_new, scale_new, pose_prev, scale_prev, counts, inlier, mean_d, age, min_inlier=0.0, hold=True):
    """``catre_track_gate``: status [I] int32 = EMPTY (``counts == 0``) | LOW_FIT (``inlier < min_inlier``) | NONFINITE (a
    NaN / infinity in the new pose, new scale, ``inlier`` or ``mean_d``).  status == 0 carries the new pose and scale and
    resets the age; otherwise the age grows by one and the previous pose and scale are carried if ``hold`` or NONFINITE is
    set, else the new ones.  -> (pose [I,3,4], scale [I,3], status [I], age [I]) as new tensors; ``age`` is not modified."""
    if not isinstance(pose_new, torch.Tensor) or pose_new.ndim != 3 or tuple(pose_new.shape[1:]) != (3, 4) or pose_new.shape[0] == 0:
        raise ValueError("pose_new: expected a [I,3,4] tensor with at least one instance")
    I = pose_new.shape[0]
    for t, name, shape in ((scale_new, "scale_new", (I, 3)), (pose_prev, "pose_prev", (I, 3, 4)), (scale_prev, "scale_prev", (I, 3)),
                           (counts, "counts", (I,)), (inlier, "inlier", (I,)), (mean_d, "mean_d", (I,)), (age, "age", (I,))):
        if _opt(t, name, shape) is None:
            raise ValueError(f"{name} is required")
    hip.load()
    f32 = lambda t, name: hip.require_dev_f32(t, name, contiguous=False).contiguous()
    pose_new, scale_new, pose_prev, scale_prev, inlier, mean_d = (f32(t, n) for t, n in (
        (pose_new, "pose_new"), (scale_new, "scale_new"), (pose_prev, "pose_prev"), (scale_prev, "scale_prev"),
        (inlier, "inlier"), (mean_d, "mean_d")))
    dev = pose_new.device
    for t, name in ((counts, "counts"), (age, "age")):
        if not t.is_cuda or t.dtype != torch.int32 or t.device != dev:
            raise ValueError(f"{name} must be int32 on {dev}")
    pose = torch.empty(I, 3, 4, dtype=torch.float32, device=dev)
    scale = torch.empty(I, 3, dtype=torch.float32, device=dev)
    status = torch.empty(I, dtype=torch.int32, device=dev)
    age = age.clone()
    _call("catre_track_gate", hip.ptr(pose_new), hip.ptr(scale_new), hip.ptr(pose_prev), hip.ptr(scale_prev),
          hip.ptr(counts.contiguous()), hip.ptr(inlier), hip.ptr(mean_d), float(min_inlier), int(bool(hold)), I, hip.ptr(pose),
          hip.ptr(scale), hip.ptr(status), hip.ptr(age), hip.stream_ptr(dev))
    return pose, scale, status, age


class Tracker:
    """Tracks ``I = kps.shape[0]`` objects seen by one camera ``K`` [3,3] through a depth sequence.

    ``model``: a ``CATRE_disR_shared`` in eval mode (its refusals stay its own; every ``out_dim`` and head form ``refine``
    runs at works here).  ``kps`` [I,M,3]: the prior points of every object, ``mean_scales`` [I,3] where the scale type
    needs them.  ``num_points`` / ``ratio`` default to ``cfg.INPUT.NUM_PCL`` / ``cfg.INPUT.DEPTH_SAMPLE_BALL_RATIO`` (0.5
    where the config has none), ``n_iter`` to ``N_ITER_TEST``.  Frame t is sampled with seed ``seed + t``.

    ``crop``: what ``step`` takes for an object's pixels when it is given neither masks nor labels.  ``"ball"`` (default):
    every pixel with depth > 0 inside the ball.  ``"render"``: the pixels where the splat of the carried pose
    (``render.splat_prior``) agrees with the frame's depth to within ``crop_delta`` metres - ``labels_fit``, which leaves out
    a table the object stands on and a hand in front of it.  ``crop_delta`` defaults to 0.05 m, the floor the reference
    puts under the ball radius (``cat_data_utils.py``): a parameter, looser than the 15 mm of the visibility test because
    the object has moved since the carried pose.  ``rho_rel`` / ``r_max``: the splat's disc size (``render.splat_prior``).

    ``reset(pose0, scale0)`` sets the carried state (e.g. from ``nocs_align.init_from_frames``); ``step(depth, ...)``
    advances one frame; ``track(depth_seq, ...)`` loops it.

    ``recover``: None (default) - the only policy is the gate, and a track whose refine goes wrong holds its last good pose.
    ``"icp"`` - every step also runs ``recover_iters`` rigid trimmed-ICP iterations (``catre_amd/icp.py``, ``trim =
    recover_trim``) from the CARRIED pose and scale on the same sampled points, scores that candidate as the refined pose
    is scored, and takes it where ICP raised no status bit and the refined pose does not reach its ``inlier_obs`` (a NaN
    refine score takes the candidate); then the unchanged gate.  No motion model, no re-detection."""

    def __init__(self, model, kps, K, mean_scales=None, num_points=None, ratio=None, n_iter=None, tau_rel=0.1, min_inlier=0.0,
                 hold_on_lost=True, seed=0, crop="ball", crop_delta=0.05, rho_rel=0.06, r_max=24.0, recover=None, recover_iters=20,
                 recover_trim=0.7):
        if recover not in (None, "icp"):
            raise ValueError(f"recover={recover!r}: expected None or 'icp'")
        self.recover, self.recover_iters, self.recover_trim = recover, int(recover_iters), float(recover_trim)
        if recover is not None and (self.recover_iters < 0 or not 0.0 < self.recover_trim <= 1.0):
            raise ValueError(f"recover_iters must be >= 0 and recover_trim in (0, 1], got {recover_iters} and {recover_trim}")
        if crop not in ("ball", "render"):
            raise ValueError(f"crop={crop!r}: expected 'ball' or 'render'")
        self.crop, self.crop_delta, self.rho_rel, self.r_max = crop, float(crop_delta), float(rho_rel), float(r_max)
        kps = _points(kps, "kps")
        I = kps.shape[0]
        mean_scales = _opt(mean_scales, "mean_scales", (I, 3))
        Kt = torch.as_tensor(K, dtype=torch.float32)
        if tuple(Kt.shape) != (3, 3):
            raise ValueError(f"K must be [3,3] (one camera), got {tuple(Kt.shape)}")
        cfg = model.cfg
        self.model, self.I = model, I
        # arguments are validated here; that the tensors live on a HIP device is checked by the kernels' wrappers in step
        self.kps = kps.contiguous()
        dev = self.kps.device
        self.mean_scales = None if mean_scales is None else mean_scales.to(dev).contiguous()
        self._K_host = Kt.cpu().contiguous()                       # sample_frames reads K on the host: copied once, here
        self._K_dev = self._K_host.to(dev).expand(I, 3, 3).contiguous()
        self.num_points = int(cfg.INPUT.NUM_PCL if num_points is None else num_points)
        self.ratio = float(cfg.INPUT.get("DEPTH_SAMPLE_BALL_RATIO", 0.5) if ratio is None else ratio)
        self.n_iter = int(cfg.MODEL.CATRE.N_ITER_TEST if n_iter is None else n_iter)
        if self.n_iter < 1:
            raise ValueError(f"n_iter must be at least 1, got {self.n_iter}")
        self.tau_rel, self.min_inlier, self.hold_on_lost, self.seed = float(tau_rel), float(min_inlier), bool(hold_on_lost), int(seed)
        self._frame_of = [0] * I
        self._label_ids = list(range(1, I + 1))
        self._zero_labels = None
        self.pose = self.scale = self.age = None
        self.t = 0

    def reset(self, pose0, scale0):
        """Set the carried pose [I,3,4] and scale [I,3] (copied), clear the ages and the frame counter."""
        pose0, scale0 = _opt(pose0, "pose0", (self.I, 3, 4)), _opt(scale0, "scale0", (self.I, 3))
        if pose0 is None or scale0 is None:
            raise ValueError("reset needs pose0 [I,3,4] and scale0 [I,3]")
        dev = self.kps.device
        self.pose = pose0.to(device=dev, dtype=torch.float32).contiguous().clone()
        self.scale = scale0.to(device=dev, dtype=torch.float32).contiguous().clone()
        self.age = torch.zeros(self.I, dtype=torch.int32, device=dev)
        self.t = 0
        return self

    def _pixels(self, depth, masks, labels, label_of):
        """-> the (masks, labels, label_of) ``sample_frames`` gets; without masks and labels the crop is the ball alone:
        an all-zero label image that every instance owns (label id 0)."""
        H, W = depth.shape[1:]
        if masks is not None and labels is not None:
            raise ValueError("give masks [I,H,W] or labels [H,W] (+ label_of [I]), not both")
        if labels is not None:
            if label_of is None:
                raise ValueError("labels needs label_of [I]: the label id of every object")
            if not isinstance(labels, torch.Tensor) or tuple(labels.shape) not in ((H, W), (1, H, W)):
                raise ValueError(f"labels must be [{H},{W}] or [1,{H},{W}], got {tuple(getattr(labels, 'shape', ()))}")
            return None, labels.reshape(1, H, W), label_of
        if label_of is not None:
            raise ValueError("label_of goes with labels")
        if masks is not None:
            if not isinstance(masks, torch.Tensor) or tuple(masks.shape) != (self.I, H, W):
                raise ValueError(f"masks must be [{self.I},{H},{W}], got {tuple(getattr(masks, 'shape', ()))}")
            return masks, None, None
        z = self._zero_labels
        if z is None or tuple(z.shape) != (1, H, W) or z.device != depth.device:
            z = self._zero_labels = torch.zeros(1, H, W, dtype=torch.uint8, device=depth.device)
        return None, z, self._frame_of

    def step(self, depth, masks=None, labels=None, label_of=None):
        """One frame: depth [H,W] or [1,H,W] fp32 on the device (metres); the objects' pixels as ``masks`` [I,H,W], as
        ``labels`` [H,W] with ``label_of`` [I], or neither (every pixel with depth > 0 inside the ball is a candidate).

        With ``crop="render"`` and neither masks nor labels, the pixels are ``labels_fit`` of the carried pose's splat against
        this depth map (``delta = crop_delta``), and the dict gains ``splat_counts`` [I,5] (``render.Splat.counts``); giving
        masks or labels in that mode is a ``ValueError``.

        Crops and samples around the carried pose, refines ``n_iter`` times, scores the last iterate, gates.  ->
        ``dict(pose [I,3,4], scale [I,3]`` (what is carried on), ``pose_iters [n_iter+1,I,3,4], score`` (``FitScore`` of the
        last iterate), ``status [I], age [I]`` int32 (:func:`track_gate`), ``pcl [I,num_points,3])``, all on the device.
        With ``recover="icp"``: also ``recovered [I]`` bool (the ICP candidate was taken; ``score`` is then its score) and
        ``icp`` (the ``ICPResult``); ``pose_iters`` stays the refine's.
        No device->host copy; the number of ABI calls does not depend on the frame."""
        if not isinstance(depth, torch.Tensor) or depth.ndim not in (2, 3) or (depth.ndim == 3 and depth.shape[0] != 1):
            raise ValueError("depth must be a [H,W] or [1,H,W] tensor")
        if self.pose is None:
            raise ValueError("Tracker.step before reset(pose0, scale0): there is no pose to crop around")
        depth = depth.reshape(1, *depth.shape[-2:])
        splat = None
        if self.crop == "render":
            if masks is not None or labels is not None or label_of is not None:
                raise ValueError('crop="render" renders the objects\' pixels itself: give neither masks nor labels')
            from . import render
            splat = render.splat_prior(self.kps, self.pose, self.scale, self._K_host, depth.shape[1:], rho_rel=self.rho_rel,
                                       r_max=self.r_max, depth=depth, delta=self.crop_delta)
            labels, label_of = splat.labels_fit, self._label_ids
        else:
            masks, labels, label_of = self._pixels(depth, masks, labels, label_of)
        pcl, _, counts = pcl_prep.sample_frames(depth, self._K_host, self._frame_of, self.pose, self.scale, masks=masks,
                                                labels=labels, label_of=label_of, ratio=self.ratio, num_points=self.num_points,
                                                use_ball=True, sample="device", seed=self.seed + self.t, return_pixels=True)
        batch = {"pcl": pcl, "obj_kps": self.kps, "obj_pose_est": self.pose, "obj_scale_est": self.scale, "K": self._K_dev}
        if self.mean_scales is not None:
            batch["obj_mean_scales"] = self.mean_scales
        out = self.model.refine(batch, n_iter=self.n_iter)
        pose_n, scale_n = out[f"pose_{self.n_iter}"], out[f"scale_{self.n_iter}"]
        score = fit_score(pcl, self.kps, pose_n, scale_n, self.tau_rel)
        cand = recovered = None
        if self.recover == "icp":
            from . import icp as _icp
            cand = _icp.icp(pcl, self.kps, self.pose, self.scale, n_iter=self.recover_iters, trim=self.recover_trim)
            score_c = fit_score(pcl, self.kps, cand.pose, cand.scale, self.tau_rel)
            recovered = (cand.status == 0) & ~(score.inlier_obs >= score_c.inlier_obs)
            pose_n = torch.where(recovered[:, None, None], cand.pose, pose_n)
            scale_n = torch.where(recovered[:, None], cand.scale, scale_n)
            score = FitScore(*(torch.where(recovered, c, r) for c, r in zip(score_c, score)))
        pose, scale, status, age = track_gate(pose_n, scale_n, self.pose, self.scale, counts, score.inlier_obs, score.d_obs,
                                              self.age, self.min_inlier, self.hold_on_lost)
        self.pose, self.scale, self.age = pose, scale, age
        self.t += 1
        res = {"pose": pose, "scale": scale, "pose_iters": torch.stack([out[f"pose_{i}"] for i in range(self.n_iter + 1)]),
               "score": score, "status": status, "age": age, "pcl": pcl}
        if splat is not None:
            res["splat_counts"] = splat.counts
        if cand is not None:
            res["recovered"], res["icp"] = recovered, cand
        return res

    def track(self, depth_seq, masks=None, labels=None, label_of=None):
        """``step`` over depth_seq [T,H,W]; ``masks`` [T,I,H,W] / ``labels`` [T,H,W] per frame (``label_of`` [I] for all).
        -> the dict of ``step`` with every tensor stacked along a leading T (``score``: a ``FitScore`` of [T,I])."""
        if not isinstance(depth_seq, torch.Tensor) or depth_seq.ndim != 3 or depth_seq.shape[0] == 0:
            raise ValueError("depth_seq must be a [T,H,W] tensor with at least one frame")
        T = depth_seq.shape[0]
        for t, name in ((masks, "masks"), (labels, "labels")):
            if t is not None and (not isinstance(t, torch.Tensor) or t.shape[0] != T):
                raise ValueError(f"{name} must hold one entry per frame ({T})")
        steps = [self.step(depth_seq[f], None if masks is None else masks[f], None if labels is None else labels[f], label_of)
                 for f in range(T)]
        out = {k: torch.stack([s[k] for s in steps]) for k in steps[0] if k not in ("score", "icp")}
        for key, nt in (("score", FitScore),) + ((("icp", type(steps[0]["icp"])),) if "icp" in steps[0] else ()):
            out[key] = nt(*(torch.stack([getattr(s[key], f) for s in steps]) for f in nt._fields))
        return out
