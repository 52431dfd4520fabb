"""Which pixels does the posed prior cover?  A z-buffered disc splat of every object's prior points on the device
(``catre_splat_render``, ``csrc/catre_render.h``): instance labels, a depth image, the winning point, and - against an
observed depth map - the BOP visibility test of ``lib/pysixd/visibility.py`` per pixel and per point.

* :func:`splat_prior` - the render.  Its ``labels`` / ``labels_fit`` images have the form
  ``pcl_prep.sample_frames(labels=..., label_of=[1..I])`` consumes.
* :func:`fit_score_visible` - ``tracking.fit_score`` plus the prior -> observed distance over the VISIBLE prior points only:
  an occluded but well-tracked object keeps a small ``d_prior_visible`` where ``d_prior`` grows.
* ``tracking.Tracker(..., crop="render")`` crops with ``labels_fit`` of the carried pose instead of the ball alone.

Pixel classes (``cls``; ``CATRE_SPLAT_*`` of ``include/catre_hip.h``), with an observed depth ``d`` and ``diff = zbuf - d``:
``BACKGROUND`` nothing rendered, ``HOLE`` ``!(d > 0)``, ``OCCLUDED`` ``diff > delta`` (something stands in front),
``FREE`` ``diff < -delta`` (the camera sees through the place), ``AGREE`` otherwise.  The reference's ``bop18`` visibility
mask is ``AGREE | FREE``, its ``bop19`` mask ``AGREE | FREE | HOLE``.

The image is the minimum of an integer key per pixel, which does not depend on the order of arrival: every output is
bit-reproducible, and a frame's outputs do not depend on the other frames of the call.  The mesh rasteriser below
(:func:`render_mesh`, ``csrc/catre_mesh.h``) writes the same key image with the same tie rule and classes: both renderers
stand on one z-buffer core (``csrc/catre_zbuf.h``), and on one argument check and one set of buffers here.  There is no
CPU fallback."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import hip, tracking

BACKGROUND, AGREE, OCCLUDED, FREE, HOLE = 0, 1, 2, 3, 4    # CATRE_SPLAT_* of include/catre_hip.h
MAX_INSTANCES, MAX_POINTS = 65535, 65536                     # 16 bits of the key each
ABI_CALLS = {"catre_splat_workspace_bytes": 0, "catre_splat_render": 0}
_OUTSIDE = "{F} frames of {H}x{W} are outside what the kernels index (F*H*W < 2^30)"

Splat = namedtuple("Splat", "labels zbuf point cls labels_fit counts visible")


def abi_call_count():
    """C-ABI calls made by this module so far (constant per call, whatever the number of instances and frames)."""
    return sum(ABI_CALLS.values())


def _check_frames(I, size, n_frames, depth, frame_of, K, rho=None, index_limit=False):
    """``size`` / ``n_frames`` / ``depth`` / ``frame_of`` / ``K`` of either renderer (``ValueError``) ->
    (F, H, W, frame_of list, K [F,3,3] on the host).  ``rho``: the splat's radii, refused where the splat refuses them;
    ``index_limit``: refuse ``F*H*W >= 2^30`` here (the rasteriser; the splat learns it from its workspace size)."""
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (H, W), got {size!r}") from None
    F = int(n_frames)
    if H < 1 or W < 1 or F < 1:
        raise ValueError(f"size and n_frames must be positive, got {(H, W)} and {F}")
    if index_limit and F * H * W >= 2 ** 30:
        raise ValueError(_OUTSIDE.format(F=F, H=H, W=W))
    if depth is not None and (not isinstance(depth, torch.Tensor) or tuple(depth.shape) not in ((F, H, W), (H, W))
                              or (depth.ndim == 2 and F != 1)):
        raise ValueError(f"depth must be [{F},{H},{W}], got {tuple(getattr(depth, 'shape', ()))}")
    if rho is not None and tracking._opt(rho, "rho", (I,)) is None:
        raise ValueError("rho must be a [I] tensor")
    fo = [0] * I if frame_of is None else [int(v) for v in (frame_of.tolist() if hasattr(frame_of, "tolist") else frame_of)]
    if len(fo) != I:
        raise ValueError(f"frame_of holds {len(fo)} frames for {I} instances")
    for i, f in enumerate(fo):
        if not 0 <= f < F:
            raise ValueError(f"frame_of[{i}] = {f} is outside the {F} frames")
    Kt = torch.as_tensor(K, dtype=torch.float32).cpu()
    if tuple(Kt.shape) == (3, 3):
        Kt = Kt.expand(F, 3, 3)
    elif tuple(Kt.shape) != (F, 3, 3):
        raise ValueError(f"K must be [3,3] or [{F},3,3], got {tuple(Kt.shape)}")
    return F, H, W, fo, Kt


def _buffers(dev, nbytes, I, F, H, W, fo, Kt):
    """What both renders allocate -> (workspace, labels, zbuf, the winning point or face, cls, labels_fit, counts, and K
    and frame_of as the ABI reads them on the host)"""
    if nbytes == 0:
        raise ValueError(_OUTSIDE.format(F=F, H=H, W=W))
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    labels, won, labels_fit, counts = i32(F, H, W), i32(F, H, W), i32(F, H, W), i32(I, 5)
    zbuf = torch.empty(F, H, W, dtype=torch.float32, device=dev)
    cls = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
    k9 = (ctypes.c_float * (9 * F))(*[float(v) for v in Kt.reshape(-1)])
    return ws, labels, zbuf, won, cls, labels_fit, counts, k9, (ctypes.c_int32 * I)(*fo)


def _check_args(kps, poses, scales, K, size, frame_of, n_frames, depth, rho=None):
    """Shapes (``ValueError``), before the device is touched -> (I, M, F, H, W, frame_of list, K [F,3,3] on the host).
    ``pose_errors.vsd_prior`` calls this too, by keyword, to refuse both of its renders before the first: keep the names."""
    kps = tracking._points(kps, "kps")
    I, M = kps.shape[0], kps.shape[1]
    if tracking._opt(poses, "poses", (I, 3, 4)) is None or tracking._opt(scales, "scales", (I, 3)) is None:
        raise ValueError("splat_prior needs poses [I,3,4] and scales [I,3]")
    if I > MAX_INSTANCES or M > MAX_POINTS:
        raise ValueError(f"at most {MAX_INSTANCES} instances of {MAX_POINTS} points (the pixel key holds 16 bits of each), got {I} x {M}")
    return (I, M) + _check_frames(I, size, n_frames, depth, frame_of, K, rho=rho)


def splat_prior(kps, poses, scales, K, size, frame_of=None, n_frames=1, rho_rel=0.06, r_max=24.0, depth=None, delta=0.015,
                return_visible=False, rho=None):
    """Render I posed priors into ``n_frames`` images of ``size = (H, W)`` -> ``Splat``.

    kps [I,M,3], poses [I,3,4], scales [I,3]: fp32 on the device; a prior point stands at ``R (s * x) + t``.  K [3,3] or
    [F,3,3] (read on the host); ``frame_of`` [I] (list / CPU tensor; None: frame 0).  ``depth`` [F,H,W] fp32 metres on the
    device, or None.  Every point is drawn as a disc of ``rho = rho_rel * |scale|`` metres (the norm ``fit_score`` uses
    for ``tau``), at most ``r_max`` pixels, centred on ``(fx x / z + cx, fy y / z + cy)``; the nearest depth wins a pixel,
    then the lower instance, then the lower point.  ``rho_rel`` and ``r_max`` are parameters with defaults, not tuned
    values: 0.06 closes the silhouette of a 1024-point box prior at 0.5 - 1.2 m (disc radii of 11 - 16 px, 0.83 of the
    bounding box of a randomly turned box covered); a sparser prior needs a larger one.  ``rho`` [I] (fp32 metres on the
    device) sets the radii directly instead.  ``delta`` (metres) is the tolerance of the visibility test, by default the
    reference's ``visib_delta`` of 15 mm (``lib/pysixd/eval_loc.py:240``).

    ``Splat``: labels [F,H,W] int32 (i + 1, 0 = background), zbuf [F,H,W] fp32 (0 = background), point [F,H,W] int32 (the
    winning point, -1), cls [F,H,W] uint8 (the module's class constants; without ``depth`` every rendered pixel is
    ``AGREE``), labels_fit [F,H,W] int32 (``labels`` where ``cls == AGREE``), counts [I,5] int32 (pixels won, then how many
    of them are AGREE, OCCLUDED, FREE, HOLE: column = class), and with ``return_visible`` visible [I,M] bool: the point was
    drawn, its centre pixel is inside the image and its own instance's, the point is at most ``delta`` behind the z-buffer
    there and the pixel is not ``OCCLUDED`` - nothing of the object's own, of another object or of the scene stands in front
    of it.  Shapes are checked (``ValueError``) before the device is touched; nothing is copied back to the host."""
    I, M, F, H, W, fo, Kt = _check_args(kps, poses, scales, K, size, frame_of, n_frames, depth, rho)
    lib = hip.load()
    kps = hip.require_dev_f32(kps, "kps", contiguous=False).contiguous()
    dev = kps.device
    poses = hip.require_dev_f32(poses, "poses", contiguous=False).contiguous()
    scales = hip.require_dev_f32(scales, "scales", contiguous=False).contiguous()
    if depth is not None:
        depth = hip.require_dev_f32(depth, "depth", contiguous=False).contiguous()
    for t, name in ((poses, "poses"), (scales, "scales"), (depth, "depth")):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, kps on {dev}")
    if rho is None:
        rho = float(rho_rel) * torch.linalg.vector_norm(scales, dim=1)
    rho = hip.require_dev_f32(rho, "rho", contiguous=False).contiguous()
    if rho.device != dev:
        raise ValueError(f"rho is on {rho.device}, kps on {dev}")
    ABI_CALLS["catre_splat_workspace_bytes"] += 1
    nbytes = lib.catre_splat_workspace_bytes(F, H, W)
    ws, labels, zbuf, point, cls, labels_fit, counts, k9, fo_c = _buffers(dev, nbytes, I, F, H, W, fo, Kt)
    vis = torch.empty(I, M, dtype=torch.uint8, device=dev) if return_visible else None
    ABI_CALLS["catre_splat_render"] += 1
    hip.check(lib.catre_splat_render(hip.ptr(kps), hip.ptr(poses), hip.ptr(scales), hip.ptr(rho), hip.ptr(depth), k9, fo_c,
                                     float(r_max), float(delta), F, I, M, H, W, hip.ptr(ws), nbytes, hip.ptr(labels),
                                     hip.ptr(zbuf), hip.ptr(point), hip.ptr(cls), hip.ptr(labels_fit), hip.ptr(counts),
                                     hip.ptr(vis), hip.stream_ptr(dev)), "catre_splat_render")
    return Splat(labels, zbuf, point, cls, labels_fit, counts, None if vis is None else vis.bool())


def fit_score_visible(pcl, kps, pose, scale, K, depth, tau_rel=0.1, rho_rel=0.06, r_max=24.0, delta=0.015):
    """``tracking.fit_score`` and the prior -> observed distance over the visible prior points ->
    (``FitScore``, d_prior_visible [I], visible_share [I]).

    pcl [I,N,3]: the observed points of every object; kps, pose, scale: as :func:`splat_prior`; K [3,3]; depth [H,W] or
    [1,H,W]: the frame all I objects are seen in.  The definition, in plain torch ops on the kernels' outputs:
    ``visible = splat_prior(kps, pose, scale, K, depth.shape, depth=depth, delta=delta, return_visible=True).visible``;
    ``nn_d2 = tracking.nn_stats(kps, pcl, src_pose=pose, src_scale=scale, return_nn=True).nn_d2``;
    ``d_prior_visible[i] = mean(sqrt(nn_d2[i][visible[i]]))`` (accumulated in double, NaN for an instance without a visible
    point) and ``visible_share[i] = mean(visible[i])``."""
    if not isinstance(depth, torch.Tensor) or depth.ndim not in (2, 3) or (depth.ndim == 3 and depth.shape[0] != 1):
        raise ValueError("depth must be a [H,W] or [1,H,W] tensor")
    H, W = depth.shape[-2:]
    score = tracking.fit_score(pcl, kps, pose, scale, tau_rel)
    sp = splat_prior(kps, pose, scale, K, (H, W), rho_rel=rho_rel, r_max=r_max, depth=depth.reshape(1, H, W), delta=delta,
                     return_visible=True)
    nn = tracking.nn_stats(kps, pcl, src_pose=pose, src_scale=scale, return_nn=True)
    vis = sp.visible
    n_vis = vis.sum(dim=1)
    d = torch.where(vis, torch.sqrt(nn.nn_d2).double(), torch.zeros((), dtype=torch.float64, device=vis.device)).sum(dim=1)
    d_vis = (d / n_vis.double()).float()          # 0 / 0 = NaN: no visible point
    return score, d_vis, n_vis.float() / vis.shape[1]


# ---- mesh rasteriser ---------------------------------------------------------------------------------------------------------
ABI_CALLS.update({"catre_mesh_workspace_bytes": 0, "catre_mesh_render": 0})

MeshRender = namedtuple("MeshRender", "labels zbuf face cls labels_fit counts culled coord projected")


def _check_mesh_args(meshes, poses, scales, K, size, frame_of, n_frames, depth, pixel_center=0.0):
    """Everything :func:`render_mesh` refuses (``ValueError``), before the device is touched ->
    (I, F, H, W, frame_of list, K [F,3,3] on the host, pixel_center_half, inst_vert_off, inst_face_off).
    ``pose_errors.vsd_mesh`` calls this too, to refuse both of its renders before the first."""
    from .meshes import MeshSet

    if not isinstance(meshes, MeshSet):
        raise ValueError(f"meshes: expected a MeshSet, got {type(meshes).__name__}")
    I = meshes.n_inst
    if tracking._opt(poses, "poses", (I, 3, 4)) is None or tracking._opt(scales, "scales", (I, 3)) is None:
        raise ValueError("render_mesh needs poses [I,3,4] and scales [I,3]")
    if pixel_center not in (0.0, 0.5):
        raise ValueError(f"pixel_center must be 0.0 (an integer pixel is its own centre) or 0.5, got {pixel_center!r}")
    F, H, W, fo, Kt = _check_frames(I, size, n_frames, depth, frame_of, K, index_limit=True)
    ivo, ifo = meshes.instance_offsets()
    if ivo[-1] >= 2 ** 31 or ifo[-1] >= 2 ** 31:
        raise ValueError(f"{int(ivo[-1])} posed vertices and {int(ifo[-1])} posed faces: both must stay below 2^31")
    for t, name in ((poses, "poses"), (scales, "scales"), (depth, "depth")):
        if t is not None and t.device != meshes.device:
            raise ValueError(f"{name} is on {t.device}, the meshes on {meshes.device}")
    return I, F, H, W, fo, Kt, int(pixel_center == 0.5), ivo, ifo


def render_mesh(meshes, poses, scales, K, size, frame_of=None, n_frames=1, depth=None, delta=0.015, pixel_center=0.0,
                return_coords=False, return_projected=False):
    """Rasterise I posed triangle meshes into ``n_frames`` images of ``size = (H, W)`` -> ``MeshRender``.

    meshes: a ``meshes.MeshSet`` on the device (instance i draws mesh ``mesh_of[i]``); poses [I,3,4], scales [I,3]: fp32 on
    the device, a vertex stands at ``R (s * x) + t``.  K [3,3] or [F,3,3] (read on the host); ``frame_of`` [I] (list / CPU
    tensor; None: frame 0); ``depth`` [F,H,W] fp32 metres on the device, or None; ``delta``: the tolerance of the
    visibility test, as in :func:`splat_prior`.  ``pixel_center``: 0.0 - an integer pixel is its own centre, the convention of
    :func:`splat_prior` and ``pcl_prep`` - or 0.5 - pixel (px, py) is sampled at (px + 0.5, py + 0.5), where the GL
    renderers of ``lib/pysixd`` sample; anything else raises ``ValueError``.

    Vertices are projected like the splat's points and snapped to 1/256 pixel; coverage is exact integer arithmetic on the
    snapped corners with the top-left fill rule (a sample on an edge shared by two faces belongs to exactly one), depth is
    perspective-correct in fp64; the nearest depth wins a pixel, then the lower instance, then the lower face.  There is NO
    clipping: a face with a vertex at or behind the camera plane (or with an index outside its mesh) is culled whole and
    counted in ``culled``.  The full contract stands at ``catre_mesh_render`` in ``include/catre_hip.h``.

    ``MeshRender``: labels [F,H,W] int32 (i + 1, 0 = background), zbuf [F,H,W] fp32 (0 = background), face [F,H,W] int32 (the
    winning face's index in its mesh, -1), cls [F,H,W] uint8, labels_fit [F,H,W] int32 and counts [I,5] int32 as ``Splat``
    has them, culled [I] int32; with ``return_coords`` coord [F,H,W,3] fp32, the model-space point (unposed, unscaled) under
    the pixel, 0 on background - for a NOCS-normalised model its NOCS map minus the 0.5 offset; with ``return_projected``
    projected [NV,4] int32, the vertex records (xi, yi, bits of z, ok) instance-major.  ``labels`` / ``labels_fit`` have the form
    ``pcl_prep.sample_frames(labels=..., label_of=[1..I])`` consumes, ``zbuf`` is a depth image for it, for
    ``nocs_align.init_from_frames`` (with ``coord + 0.5``) and for ``pose_errors.vsd``.  Everything is bit-reproducible, and a
    frame's outputs do not depend on the other frames of the call.  Arguments are checked (``ValueError``) before the device
    is touched; nothing is copied back to the host; the number of ABI calls is constant."""
    if delta != delta:
        raise ValueError("delta is NaN")
    I, F, H, W, fo, Kt, half, ivo, ifo = _check_mesh_args(meshes, poses, scales, K, size, frame_of, n_frames, depth, pixel_center)
    lib = hip.load()
    poses = hip.require_dev_f32(poses, "poses", contiguous=False).contiguous()
    dev = poses.device
    scales = hip.require_dev_f32(scales, "scales", contiguous=False).contiguous()
    if depth is not None:
        depth = hip.require_dev_f32(depth, "depth", contiguous=False).contiguous()
    NV, NF = int(ivo[-1]), int(ifo[-1])
    off = torch.from_numpy(np.stack([ivo, ifo]).astype(np.int32)).to(dev, non_blocking=True)
    ABI_CALLS["catre_mesh_workspace_bytes"] += 1
    nbytes = lib.catre_mesh_workspace_bytes(F, H, W, NV)
    ws, labels, zbuf, face, cls, labels_fit, counts, k9, fo_c = _buffers(dev, nbytes, I, F, H, W, fo, Kt)
    culled = torch.empty(I, dtype=torch.int32, device=dev)
    coord = torch.empty(F, H, W, 3, dtype=torch.float32, device=dev) if return_coords else None
    projected = torch.empty(NV, 4, dtype=torch.int32, device=dev) if return_projected else None
    ABI_CALLS["catre_mesh_render"] += 1
    hip.check(lib.catre_mesh_render(hip.ptr(meshes.verts), hip.ptr(meshes.faces), hip.ptr(meshes.vert_off), hip.ptr(meshes.face_off),
                                    hip.ptr(meshes.mesh_of), hip.ptr(off[0]), hip.ptr(off[1]), hip.ptr(poses), hip.ptr(scales),
                                    hip.ptr(depth), k9, fo_c, float(delta), half, meshes.n_meshes, meshes.v_tot, meshes.t_tot, F, I,
                                    NV, NF, H, W, hip.ptr(ws), nbytes, hip.ptr(labels), hip.ptr(zbuf), hip.ptr(face), hip.ptr(cls),
                                    hip.ptr(labels_fit), hip.ptr(counts), hip.ptr(culled), hip.ptr(coord), hip.ptr(projected),
                                    hip.stream_ptr(dev)), "catre_mesh_render")
    return MeshRender(labels, zbuf, face, cls, labels_fit, counts, culled, coord, projected)
