"""BOP pose errors on the device (``csrc/catre_bop.h``), beside ``evaluation.add_errors``: the symmetry-aware errors of
``lib/pysixd/pose_error.py`` - MSSD (``mssd`` :131-153), MSPD (``mspd`` :156-179), ``proj_sym`` (:196-217) - in one
``catre_sym_err`` call for a batch, and VSD (``vsd`` :22-128, ``cost_type="step"``) for given depth images in one ``catre_vsd`` call.

* :func:`symmetry_transforms`, :func:`axis_symmetry_transforms` - host numpy: a ``models_info.json`` entry -> ``[S,3,4]``
  (``misc.get_symmetry_transformations`` / ``get_axis_symmetry_transformations``, ``misc.py:220-282``).
* :class:`SymSets` - the sets of a batch as one ragged table on the device.
* :func:`sym_errors` - MSSD, MSPD and proj_sym with the winning symmetry of each.
* :func:`vsd` - visible surface discrepancy of two rendered depth images against an observed one, from ANY renderer.
* :func:`vsd_prior` - two ``render.splat_prior`` calls and :func:`vsd`: the VSD of the splatted point prior.
* :func:`vsd_mesh` - two ``render.render_mesh`` calls and :func:`vsd`: the VSD of the rasterised model mesh, BOP's own.

Everything is bit-reproducible: the maxima and minima do not depend on an order, the mean is a fixed tree, the VSD counts
are integer sums.  An instance's results do not depend on the batch around it.  A NaN in a pose, scale or point makes the
instance's three symmetry errors NaN; the reference's python ``min()`` over a list with NaNs depends on where they stand
and is not reproduced.  There is no CPU fallback."""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import hip

BOP19, BOP18 = 0, 1          # CATRE_VSD_BOP19 / CATRE_VSD_BOP18 of include/catre_hip.h
MAX_TAUS = 16                # CATRE_VSD_MAX_TAUS
DEFAULT_TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))      # 0.05 .. 0.5, the BOP challenge's range
ABI_CALLS = {"catre_sym_err_workspace_bytes": 0, "catre_sym_err": 0, "catre_vsd": 0}

SymErrors = namedtuple("SymErrors", "mssd mspd proj best_mssd best_mspd best_proj e3 e2 p2")


def abi_call_count():
    """C-ABI calls made by this module so far (constant per call, whatever the number of instances, symmetries and taus)."""
    return sum(ABI_CALLS.values())


# ---- symmetry sets -------------------------------------------------------------------------------------------------------
def _axis_rotation(angle, axis):
    """Rodrigues: the rotation by ``angle`` about the direction ``axis`` (``transform.rotation_matrix`` without a point)."""
    d = np.array(axis, dtype=np.float64).reshape(-1)[:3]
    d = d / math.sqrt(float(d @ d))
    c, s = math.cos(angle), math.sin(angle)
    R = np.diag([c, c, c]) + np.outer(d, d) * (1.0 - c)
    d = d * s
    return R + np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])


def _continuous(axis, offset, max_sym_disc_step):
    """Turns by k * 2 pi / count, k = 1 .. count - 1 (no identity), about the axis through ``offset`` -> list of (R, t)."""
    count = int(np.ceil(np.pi / max_sym_disc_step))
    step = 2.0 * np.pi / count
    off = np.asarray(offset, np.float64).reshape(3, 1)
    out = []
    for k in range(1, count):
        R = _axis_rotation(k * step, axis)
        out.append((R, -(R @ off) + off))
    return out


def _stack(pairs):
    return np.stack([np.hstack([R, np.reshape(t, (3, 1))]) for R, t in pairs]).astype(np.float64)


def axis_symmetry_transforms(axis, max_sym_disc_step=0.01):
    """The discretized turns about ``axis`` through the origin -> [S,3,4] float64, S = ceil(pi / step) - 1.  The identity
    is NOT in the list (``misc.get_axis_symmetry_transformations``, ``misc.py:220-231``)."""
    return _stack(_continuous(axis, np.zeros(3), max_sym_disc_step))


def symmetry_transforms(model_info, max_sym_disc_step=0.01):
    """A ``models_info.json`` entry (``symmetries_discrete``: 4x4 matrices as 16 numbers, ``symmetries_continuous``:
    ``{"axis", "offset"}``) -> [S,3,4] float64 (``misc.get_symmetry_transformations``, ``misc.py:234-282``).  The identity
    leads the discrete symmetries; every discrete one is combined with every discretized continuous turn,
    ``R = R_c R_d``, ``t = R_c t_d + t_c``.  The reference's shape is kept: WITH a continuous symmetry the turns start at
    k = 1, so the identity itself is not in the list (:class:`SymSets` puts it first)."""
    disc = [(np.eye(3), np.zeros((3, 1)))]
    for sym in model_info.get("symmetries_discrete", ()):
        m = np.reshape(np.asarray(sym, np.float64), (4, 4))
        disc.append((m[:3, :3], m[:3, 3].reshape(3, 1)))
    cont = []
    for sym in model_info.get("symmetries_continuous", ()):
        cont += _continuous(sym["axis"], sym["offset"], max_sym_disc_step)
    if not cont:
        return _stack(disc)
    return _stack([(Rc @ Rd, Rc @ td + tc) for Rd, td in disc for Rc, tc in cont])


_EYE34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def _one_set(s, where):
    """None, [S,3,3] or [S,3,4] -> [S',3,4] float32 with the identity first (not duplicated if it already leads)."""
    if s is None:
        return _EYE34[None].astype(np.float32)
    a = np.asarray(s.detach().cpu() if isinstance(s, torch.Tensor) else s, dtype=np.float64)
    if a.ndim != 3 or a.shape[1] != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{where}: expected None, [S,3,3] rotations or [S,3,4] transforms, got {a.shape}")
    if a.shape[2] == 3:
        a = np.concatenate([a, np.zeros((a.shape[0], 3, 1))], 2)
    if a.shape[0] == 0 or not np.array_equal(a[0], _EYE34):
        a = np.concatenate([_EYE34[None], a], 0)
    return a.astype(np.float32)


class SymSets:
    """The symmetry sets of a batch as a ragged table on the device: ``syms`` [S_tot,3,4] fp32, ``sym_off`` [G+1] int32 (set
    g is rows ``sym_off[g] .. sym_off[g+1] - 1``), ``sym_of`` [I] int32 (the set of instance i; None: instance i reads set i).
    ``sizes`` (host) are the set sizes, ``s_max`` the largest; ``host`` keeps the fp32 sets as numpy arrays."""

    def __init__(self, syms, sym_off, sym_of, host, n_inst):
        self.syms, self.sym_off, self.sym_of, self.host, self.n_inst = syms, sym_off, sym_of, host, n_inst
        self.sizes = tuple(len(h) for h in host)
        self.s_max, self.s_tot, self.n_sets = max(self.sizes), sum(self.sizes), len(host)

    @classmethod
    def from_list(cls, sym_infos, device, sym_of=None):
        """``sym_infos``: per set None (no symmetry: the identity alone), [S,3,3] rotations (the loader's ``sym_info``,
        what ``losses.SymTensors.from_list`` takes) or [S,3,4] transforms (:func:`symmetry_transforms`).  The identity is
        put first, as ``losses._sym_tensor`` does, unless the list already starts with it.  ``sym_of`` (a list of I set
        indices) lets the instances of a batch share sets; None: one set per instance, in order."""
        sym_infos = list(sym_infos)
        if not sym_infos:
            raise ValueError("sym_infos: needs at least one set")
        host = [_one_set(s, f"sym_infos[{g}]") for g, s in enumerate(sym_infos)]
        if sym_of is None:
            sym_of = list(range(len(host)))
        sym_of = _int_list(sym_of, "sym_of")
        for i, g in enumerate(sym_of):
            if not 0 <= g < len(host):
                raise ValueError(f"sym_of[{i}] = {g} is outside the {len(host)} sets")
        off = np.concatenate([[0], np.cumsum([len(h) for h in host])]).astype(np.int32)
        return cls(torch.from_numpy(np.concatenate(host, 0)).to(device), torch.from_numpy(off).to(device),
                   torch.tensor(sym_of, dtype=torch.int32).to(device), host, len(sym_of))

    def padded(self):
        """Host view -> (cands [G,S_max,3,4] fp32 padded with the identity, valid [G,S_max] bool)."""
        cands = np.tile(_EYE34.astype(np.float32), (self.n_sets, self.s_max, 1, 1))
        valid = np.zeros((self.n_sets, self.s_max), bool)
        for g, h in enumerate(self.host):
            cands[g, :len(h)] = h
            valid[g, :len(h)] = True
        return cands, valid


def _int_list(v, name):
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise ValueError(f"{name}: a list or a CPU tensor (it is checked on the host), got a tensor on {v.device}")
        v = v.tolist()
    try:
        return [int(x) for x in v]
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected a list of integers, got {v!r}") from None


# ---- argument checks (before the device is touched) -------------------------------------------------------------------------
def _shape(t, name, shape):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a tensor of shape {tuple(shape)}, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    return t


def _same_device(dev, **tensors):
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, expected {dev}")


def _camera(K, I, dev):
    """[3,3] or [I,3,3] (tensor, on the device or on the host, or an array) -> [I,3,3] fp32.  Host tables go up with
    ``non_blocking`` copies (the runtime stages pageable memory before it returns): nothing waits on the device."""
    Kt = torch.as_tensor(K)
    if tuple(Kt.shape) not in ((3, 3), (I, 3, 3)):
        raise ValueError(f"K must be [3,3] or [{I},3,3], got {tuple(Kt.shape)}")
    if Kt.is_cuda and Kt.device != dev:
        raise ValueError(f"K is on {Kt.device}, expected {dev}")
    return Kt, (lambda: Kt.to(device=dev, dtype=torch.float32, non_blocking=True).expand(I, 3, 3).contiguous())


def _f32(t, name):
    return None if t is None else hip.require_dev_f32(t, name, contiguous=False).contiguous()


# ---- MSSD, MSPD, proj_sym ----------------------------------------------------------------------------------------------------
def sym_errors(pose_est, pose_gt, pts, K, syms, sym_of=None, scale_est=None, scale_gt=None, per_sym=False):
    """MSSD, MSPD and proj_sym of I instances -> ``SymErrors``.

    pose_est, pose_gt [I,3,4], pts [I,n,3] or [n,3] (the model points, shared), optional scale_est / scale_gt [I,3] applied to
    the points as in ``evaluation.add_errors``: fp32 on the device.  K [3,3] or [I,3,3].  ``syms``: a :class:`SymSets`;
    ``sym_of`` (a list, or an int32 tensor on the device) overrides its instance -> set map.  For symmetry ``(R_s, t_s)``:
    ``x_est = R_est (s_est * p) + t_est``, ``x_gt = R_gt (s_gt * (R_s p + t_s)) + t_gt``,
    ``e3 = max_n |x_est - x_gt|``, ``e2 = max_n |pi(x_est) - pi(x_gt)|``, ``p2 = mean_n`` of that pixel distance, with
    ``pi(x) = (fx x / z + cx, fy y / z + cy)``; points behind the camera are not special, as in the reference.

    ``SymErrors``: mssd, mspd, proj [I] fp32 = the minimum over the set of e3 (metres), e2, p2 (pixels); best_mssd, best_mspd,
    best_proj [I] int32 = the index of the winning symmetry in the instance's set (0: the identity), the lowest on an exact
    tie; with ``per_sym`` e3, e2, p2 [I,S_max] fp32, ``+inf`` behind the end of a set (else None).  A NaN in a pose, scale
    or point gives NaN in all three errors of that instance.  Shapes and devices are checked (``ValueError``) before the device is
    touched; nothing is read back."""
    if not isinstance(syms, SymSets):
        raise ValueError(f"syms: expected a SymSets, got {type(syms).__name__}")
    if not isinstance(pose_est, torch.Tensor) or pose_est.ndim != 3 or tuple(pose_est.shape[1:]) != (3, 4) or pose_est.shape[0] == 0:
        raise ValueError("pose_est: expected a [I,3,4] tensor with at least one instance")
    I, dev = pose_est.shape[0], pose_est.device
    _shape(pose_gt, "pose_gt", (I, 3, 4))
    if not isinstance(pts, torch.Tensor) or pts.ndim not in (2, 3) or pts.shape[-1] != 3 or pts.shape[-2] == 0 or \
            (pts.ndim == 3 and pts.shape[0] != I):
        raise ValueError(f"pts: expected [{I},n,3] or [n,3] with n > 0, got {tuple(getattr(pts, 'shape', ()))}")
    n = pts.shape[-2]
    if scale_est is not None:
        _shape(scale_est, "scale_est", (I, 3))
    if scale_gt is not None:
        _shape(scale_gt, "scale_gt", (I, 3))
    _, k_dev = _camera(K, I, dev)
    if sym_of is None:
        sym_of = syms.sym_of
        if syms.n_inst != I:
            raise ValueError(f"syms maps {syms.n_inst} instances to sets, the batch holds {I}")
    elif isinstance(sym_of, torch.Tensor) and sym_of.is_cuda:
        if sym_of.dtype != torch.int32 or tuple(sym_of.shape) != (I,):
            raise ValueError(f"sym_of: expected a [{I}] int32 tensor, got {tuple(sym_of.shape)} {sym_of.dtype}")
    else:
        sym_of = _int_list(sym_of, "sym_of")
        if len(sym_of) != I:
            raise ValueError(f"sym_of holds {len(sym_of)} entries for {I} instances")
        for i, g in enumerate(sym_of):
            if not 0 <= g < syms.n_sets:
                raise ValueError(f"sym_of[{i}] = {g} is outside the {syms.n_sets} sets")
        sym_of = torch.tensor(sym_of, dtype=torch.int32)
    _same_device(dev, pose_gt=pose_gt, pts=pts, scale_est=scale_est, scale_gt=scale_gt, syms=syms.syms)
    if sym_of.is_cuda:
        _same_device(dev, sym_of=sym_of)
    lib = hip.load()
    pose_est, pose_gt, pts, scale_est, scale_gt = (_f32(t, nm) for t, nm in (
        (pose_est, "pose_est"), (pose_gt, "pose_gt"), (pts, "pts"), (scale_est, "scale_est"), (scale_gt, "scale_gt")))
    sym_of = sym_of.to(dev, non_blocking=True).contiguous()
    Kd = k_dev()
    S_max = syms.s_max
    ABI_CALLS["catre_sym_err_workspace_bytes"] += 1
    nbytes = lib.catre_sym_err_workspace_bytes(I, S_max)
    if nbytes == 0:
        raise ValueError(f"{I} instances of {S_max} symmetries are outside what the kernels index")
    tables = torch.empty(3, I, S_max, dtype=torch.float32, device=dev) if per_sym else None
    ws = None if per_sym else torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    err = torch.empty(3, I, dtype=torch.float32, device=dev)
    best = torch.empty(3, I, dtype=torch.int32, device=dev)
    ABI_CALLS["catre_sym_err"] += 1
    hip.check(lib.catre_sym_err(hip.ptr(pts), int(pts.ndim == 2), n, hip.ptr(pose_est), hip.ptr(pose_gt), hip.ptr(scale_est),
                                hip.ptr(scale_gt), hip.ptr(Kd), hip.ptr(syms.syms), hip.ptr(syms.sym_off), hip.ptr(sym_of),
                                syms.n_sets, syms.s_tot, S_max, I, hip.ptr(ws), 0 if ws is None else nbytes, hip.ptr(err),
                                hip.ptr(best), hip.ptr(tables), hip.stream_ptr(dev)), "catre_sym_err")
    t = (None, None, None) if tables is None else (tables[0], tables[1], tables[2])
    return SymErrors(err[0], err[1], err[2], best[0], best[1], best[2], *t)


# ---- VSD ---------------------------------------------------------------------------------------------------------------------
def _vsd_options(taus, visib_mode, cost_type):
    if cost_type == "tlinear":
        raise NotImplementedError("cost_type='tlinear' (the ECCVW'16 truncated linear cost) is not built; only 'step' is")
    if cost_type != "step":
        raise ValueError(f"Unknown pixel matching cost: {cost_type!r}")
    if visib_mode not in ("bop19", "bop18"):
        raise ValueError(f"Unknown visibility mode: {visib_mode!r}")
    try:
        taus = [float(t) for t in taus]
    except (TypeError, ValueError):
        raise ValueError(f"taus: expected a sequence of numbers, got {taus!r}") from None
    if not 1 <= len(taus) <= MAX_TAUS or any(t != t for t in taus):
        raise ValueError(f"taus: 1 .. {MAX_TAUS} numbers, none of them NaN; got {taus}")
    return taus, BOP18 if visib_mode == "bop18" else BOP19


def _frames(frame_of, I, F, dev):
    """None (frame 0), a list / CPU tensor (checked here) or an int32 tensor on the device -> a thunk of the device tensor"""
    if frame_of is None:
        return lambda: None
    if isinstance(frame_of, torch.Tensor) and frame_of.is_cuda:
        if frame_of.dtype != torch.int32 or tuple(frame_of.shape) != (I,) or frame_of.device != dev:
            raise ValueError(f"frame_of: expected a [{I}] int32 tensor on {dev}")
        return lambda: frame_of.contiguous()
    fo = _int_list(frame_of, "frame_of")
    if len(fo) != I:
        raise ValueError(f"frame_of holds {len(fo)} frames for {I} instances")
    for i, f in enumerate(fo):
        if not 0 <= f < F:
            raise ValueError(f"frame_of[{i}] = {f} is outside the {F} frames")
    return lambda: torch.tensor(fo, dtype=torch.int32).to(dev, non_blocking=True)


def _origins(origin, I, dev):
    if origin is None:
        return lambda: None
    if isinstance(origin, torch.Tensor) and origin.is_cuda:
        if origin.dtype != torch.int32 or tuple(origin.shape) != (I, 2) or origin.device != dev:
            raise ValueError(f"origin: expected a [{I},2] int32 tensor on {dev}")
        return lambda: origin.contiguous()
    try:
        o = np.asarray(origin.tolist() if isinstance(origin, torch.Tensor) else origin).astype(np.int64)
    except (TypeError, ValueError):
        raise ValueError(f"origin: expected [{I},2] integers, got {origin!r}") from None
    if o.shape != (I, 2) or np.abs(o).max(initial=0) >= 2 ** 30:
        raise ValueError(f"origin: expected [{I},2] integers (u0, v0) below 2^30, got shape {o.shape}")
    return lambda: torch.from_numpy(o.astype(np.int32)).to(dev, non_blocking=True)


def vsd(depth_est, depth_gt, depth_test, K, delta=0.015, taus=DEFAULT_TAUS, diameter=None, frame_of=None, origin=None,
        visib_mode="bop19", cost_type="step"):
    """Visible surface discrepancy of I pairs of rendered depth images against observed ones -> (errors [I,T] fp64, counts
    [I,2+T] int32).  Everything of the reference's ``vsd`` after its two renders; the depth images may come from any
    renderer.

    depth_est, depth_gt [I,h,w] fp32 on the device, metres, 0 = nothing rendered; depth_test [F,H,W] (or [H,W]) fp32 on the
    device; K [3,3] or [I,3,3] of the FULL image.  ``frame_of`` [I] (None: frame 0) picks the observed frame, ``origin`` [I,2]
    = (u0, v0) places the [h,w] window in it (None: the window is the frame's top-left corner - the whole frame when the sizes
    agree); both are lists / CPU tensors (checked here) or int32 tensors on the device.  Window pixels outside the frame are
    ignored.  ``delta``: the visibility tolerance (metres; the reference's 15 mm); ``taus``: 1 .. 16 misalignment tolerances;
    ``diameter``: None (``normalized_by_diameter`` off), a number or [I] (tensor / array) - the pixel distances are divided
    by it in double; ``visib_mode``: "bop19" (a pixel without observed depth counts as visible; the reference's ``vsd``
    uses this one) or "bop18".  ``cost_type``: "step" only ("tlinear" raises ``NotImplementedError``).

    Per pixel the reference's arithmetic in its precisions: distance images in double (``misc.depth_im_to_dist_im_fast``),
    the visibility test on their fp32 casts with ``delta`` as fp32, ``d_test == 0`` as written there (the splat render's HOLE
    is ``!(d > 0)``: the two differ for negative or NaN observed depths only), the cost ``|dist_gt - dist_est| / diameter
    >= tau`` in double.  counts: pixels of the union of the two visibility masks, of their intersection, and of cost 1 per
    tau; errors = ``(cost + union - inter) / union``, 1.0 for an empty union.  Bit-reproducible; nothing is read back."""
    taus, mode = _vsd_options(taus, visib_mode, cost_type)
    if not isinstance(depth_est, torch.Tensor) or depth_est.ndim != 3 or 0 in depth_est.shape:
        raise ValueError("depth_est: expected a [I,h,w] tensor")
    I, h, w = depth_est.shape
    dev = depth_est.device
    _shape(depth_gt, "depth_gt", (I, h, w))
    if not isinstance(depth_test, torch.Tensor) or depth_test.ndim not in (2, 3) or 0 in depth_test.shape:
        raise ValueError("depth_test: expected a [F,H,W] or [H,W] tensor")
    if depth_test.ndim == 2:
        depth_test = depth_test[None]
    F, H, W = depth_test.shape
    if h * w >= 2 ** 30 or H * W >= 2 ** 30:
        raise ValueError(f"windows of {h}x{w} in frames of {H}x{W} are outside what the kernels index (below 2^30 pixels)")
    _same_device(dev, depth_gt=depth_gt, depth_test=depth_test)
    _, k_dev = _camera(K, I, dev)
    fo, org = _frames(frame_of, I, F, dev), _origins(origin, I, dev)
    if delta != delta:
        raise ValueError("delta is NaN")
    if diameter is not None:
        if isinstance(diameter, torch.Tensor):
            if tuple(diameter.shape) != (I,) or (diameter.is_cuda and diameter.device != dev):
                raise ValueError(f"diameter: expected [{I}] on {dev} or on the host, got {tuple(diameter.shape)} on {diameter.device}")
        else:
            try:
                diameter = torch.as_tensor(np.broadcast_to(np.asarray(diameter, np.float64), (I,)).copy())
            except ValueError:
                raise ValueError(f"diameter: expected a number or [{I}] values") from None
    lib = hip.load()
    depth_est, depth_gt, depth_test = _f32(depth_est, "depth_est"), _f32(depth_gt, "depth_gt"), _f32(depth_test, "depth_test")
    Kd, fo, org = k_dev(), fo(), org()
    if diameter is not None:
        diameter = diameter.to(dtype=torch.float64).to(dev, non_blocking=True).contiguous()
    T = len(taus)
    counts = torch.empty(I, 2 + T, dtype=torch.int32, device=dev)
    errors = torch.empty(I, T, dtype=torch.float64, device=dev)
    ABI_CALLS["catre_vsd"] += 1
    hip.check(lib.catre_vsd(hip.ptr(depth_est), hip.ptr(depth_gt), hip.ptr(depth_test), hip.ptr(Kd), hip.ptr(fo), hip.ptr(org),
                            hip.ptr(diameter), (ctypes.c_double * T)(*taus), float(delta), mode, I, h, w, F, H, W, T,
                            hip.ptr(counts), hip.ptr(errors), hip.stream_ptr(dev)), "catre_vsd")
    return errors, counts


def _vsd_rendered(check, draw, pose_est, scale_est, pose_gt, scale_gt, K, depth_test, frame_of, origin, size, delta, taus,
                  diameter, visib_mode):
    """What :func:`vsd_prior` and :func:`vsd_mesh` share: the checks, the windowed camera, the two renders, :func:`vsd`.
    ``check(pose, scale, Kw, size, own, I)`` refuses (``ValueError``) what the render ``draw(pose, scale, Kw, size, own, I)``
    would; ``own`` = [0..I): every instance in a frame of its own.  Everything is refused before the device is touched."""
    if not isinstance(pose_est, torch.Tensor) or pose_est.ndim != 3:
        raise ValueError("pose_est: expected a [I,3,4] tensor")
    I = pose_est.shape[0]
    if not isinstance(depth_test, torch.Tensor) or depth_test.ndim not in (2, 3):
        raise ValueError("depth_test: expected a [F,H,W] or [H,W] tensor")
    if size is None:
        if origin is not None:
            raise ValueError("origin needs size = (h, w), the window it places")
        size = tuple(depth_test.shape[-2:])
    Kh = torch.as_tensor(K, dtype=torch.float32).cpu()
    if tuple(Kh.shape) not in ((3, 3), (I, 3, 3)):
        raise ValueError(f"K must be [3,3] or [{I},3,3], got {tuple(Kh.shape)}")
    Kw = Kh.expand(I, 3, 3).clone()
    if origin is not None:
        o = _origins(origin, I, torch.device("cpu"))().float()
        Kw[:, 0, 2] -= o[:, 0]
        Kw[:, 1, 2] -= o[:, 1]
    own = list(range(I))
    _vsd_options(taus, visib_mode, "step")
    for pose, scale in ((pose_est, scale_est), (pose_gt, scale_gt)):
        check(pose, scale, Kw, size, own, I)
    _frames(frame_of, I, 1 if depth_test.ndim == 2 else depth_test.shape[0], depth_test.device)
    est, gt = draw(pose_est, scale_est, Kw, size, own, I), draw(pose_gt, scale_gt, Kw, size, own, I)
    return vsd(est.zbuf, gt.zbuf, depth_test, Kh, delta=delta, taus=taus, diameter=diameter, frame_of=frame_of, origin=origin,
               visib_mode=visib_mode)


def vsd_prior(kps, pose_est, scale_est, pose_gt, scale_gt, K, depth_test, frame_of=None, origin=None, size=None, delta=0.015,
              taus=DEFAULT_TAUS, diameter=None, visib_mode="bop19", rho_rel=0.06, r_max=24.0, rho=None):
    """VSD of the SPLATTED POINT PRIOR -> (errors [I,T] fp64, counts [I,2+T] int32): two ``render.splat_prior`` calls - the
    prior ``kps`` [I,M,3] at (pose_est, scale_est) and at (pose_gt, scale_gt) - and :func:`vsd` on their depth images.

    This is NOT the VSD of a mesh render: a disc splat of the prior's points stands in for the model surface, so the numbers
    depend on ``rho_rel`` / ``r_max`` / ``rho`` (``render.splat_prior``) and on how densely the prior samples the surface.
    :func:`vsd` itself takes depth images from any renderer.

    Every instance is rendered into a frame of its own - no object occludes another, as BOP renders them.  ``size`` = (h, w)
    and ``origin`` [I,2] = (u0, v0) (a list, needed on the host) render a window of the frame instead of all of it: the
    render's camera is K with ``cx - u0``, ``cy - v0`` (fp32), :func:`vsd` gets the full-image K.  K [3,3] or [I,3,3]:
    ``splat_prior`` reads it on the host - pass it there and nothing is copied back.  The ABI-call count is constant."""
    from . import render

    def check(pose, scale, Kw, size, own, I):
        render._check_args(kps=kps, poses=pose, scales=scale, K=Kw, size=size, frame_of=own, n_frames=I, depth=None, rho=rho)

    def draw(pose, scale, Kw, size, own, I):
        return render.splat_prior(kps, pose, scale, Kw, size, frame_of=own, n_frames=I, rho_rel=rho_rel, r_max=r_max, rho=rho)

    return _vsd_rendered(check, draw, pose_est, scale_est, pose_gt, scale_gt, K, depth_test, frame_of, origin, size, delta, taus,
                         diameter, visib_mode)


def vsd_mesh(meshes, pose_est, scale_est, pose_gt, scale_gt, K, depth_test, frame_of=None, origin=None, size=None,
             pixel_center=0.0, delta=0.015, taus=DEFAULT_TAUS, diameter=None, visib_mode="bop19"):
    """VSD of the RASTERISED MODEL MESH, as BOP defines it -> (errors [I,T] fp64, counts [I,2+T] int32): two
    ``render.render_mesh`` calls - the meshes (a ``meshes.MeshSet`` of I instances) at (pose_est, scale_est) and at (pose_gt,
    scale_gt) - and :func:`vsd` on their depth images.

    Every instance is rendered into a frame of its own - no object occludes another, as BOP renders them; occlusion BETWEEN
    the instances of a scene is therefore not part of the error (it enters through ``depth_test`` alone).  ``size`` = (h, w) and
    ``origin`` [I,2] = (u0, v0) (a list, needed on the host) render a window of the frame instead of all of it, with the same
    windowed camera as :func:`vsd_prior`: K with ``cx - u0``, ``cy - v0`` (fp32); :func:`vsd` gets the full-image K.
    ``pixel_center``: as ``render_mesh``; :func:`vsd` back-projects an integer pixel as its own centre, which is what 0.0
    renders.  K [3,3] or [I,3,3] is read on the host.  Everything either render or the comparison would refuse is refused
    before the device is touched; the ABI-call count is constant."""
    from . import render

    def check(pose, scale, Kw, size, own, I):
        if delta != delta:
            raise ValueError("delta is NaN")
        render._check_mesh_args(meshes, pose, scale, Kw, size, own, I, None, pixel_center)

    def draw(pose, scale, Kw, size, own, I):
        return render.render_mesh(meshes, pose, scale, Kw, size, frame_of=own, n_frames=I, pixel_center=pixel_center)

    return _vsd_rendered(check, draw, pose_est, scale_est, pose_gt, scale_gt, K, depth_test, frame_of, origin, size, delta, taus,
                         diameter, visib_mode)
