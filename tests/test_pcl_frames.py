"""Row f3 for a data batch: ``catre_amd.pcl_prep.sample_frames`` over ``catre_pclf_*`` - every instance of every frame in
the launches one frame takes.  Per frame the kernels run the single-frame device functions, so the yardstick is exact:
``torch.equal`` against a loop of the unchanged ``sample_instances`` over the frames, in every sampling mode; the
reference itself is reached through ``tests/golden/pcl_prep.npz`` (1e-6 abs on the points, the bound
``tests/test_pcl_prep.py`` uses for the same arithmetic) and ``tests/pcl_frames_ref.frames_loop``.

Shapes: 120x160 frames (four full 4096-pixel chunks and a partial one), 64x64 (exactly one chunk) and 7x9 (a single
partial chunk)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from catre_amd import hip, pcl_prep, synth
from tests import pcl_frames_ref as R
from tests.util import GOLDEN_DIR

DEV = "cuda:0"
N = 96
NEW_SYMBOLS = ("catre_pclf_workspace_bytes", "catre_pclf_candidates", "catre_pclf_sample", "catre_pclf_fps",
               "catre_depth_augment")


def _tiny_scene(seed, n_inst, H=7, W=9):
    """a hand-made frame small enough for a single partial chunk: a wall with two holes, half-frame masks"""
    g = torch.Generator().manual_seed(seed)
    depth = 1.0 + 0.05 * torch.rand(H, W, generator=g)
    depth[seed % H, (2 * seed + 1) % W] = 0.0
    depth[(seed + 3) % H, (seed + 4) % W] = 0.0
    K = torch.tensor([[8.0 + seed, 0.0, W / 2 - 0.5], [0.0, 8.5, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    masks = torch.zeros(n_inst, H, W, dtype=torch.bool)
    poses = torch.zeros(n_inst, 3, 4)
    for i in range(n_inst):
        masks[i, :, i * 3:i * 3 + 4] = True
        poses[i, :, :3] = torch.eye(3)
        poses[i, :, 3] = torch.tensor([(i * 3 + 1.5 - K[0, 2]) / K[0, 0], 0.0, 1.02])
    scales = torch.full((n_inst, 3), 0.3)
    scales[0] *= 0.1                                      # the 0.05 radius floor and its growth
    return dict(depth=depth, K=K, masks=masks, poses=poses, scales=scales)


def make_batch(H, W, per_frame=(5, 0, 3)):
    """F frames with their own K and ``per_frame`` instances each (frame by frame) -> dict of CPU tensors"""
    sc = []
    for f, n in enumerate(per_frame):
        s = _tiny_scene(f, max(n, 1)) if H * W < 1000 else synth.make_depth_scene(H=H, W=W, n_inst=5, seed=20 + f)
        s["K"] = s["K"].clone()
        s["K"][0, 0] *= 1.0 + 0.05 * f                    # a camera per frame
        s["K"][1, 2] += 0.25 * f
        sc.append(s)
    if H * W < 1000:
        per_frame = tuple(min(n, 2) for n in per_frame)
    frame_of = [f for f, n in enumerate(per_frame) for _ in range(n)]
    cat = lambda k: torch.cat([s[k][:n] for s, n in zip(sc, per_frame)])
    return dict(depth=torch.stack([s["depth"] for s in sc]), K=torch.stack([s["K"] for s in sc]), frame_of=frame_of,
                masks=cat("masks"), poses=cat("poses"), scales=cat("scales"))


def to_dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "K" else v) for k, v in b.items()}


def frames(b, **kw):
    return pcl_prep.sample_frames(b["depth"], b["K"], b["frame_of"], b["poses"], b["scales"], masks=b["masks"], num_points=N,
                                  return_pixels=True, **kw)


def loop(b, seeds, **kw):
    """the parent's way: the unchanged sample_instances frame by frame (frames without an instance are skipped)"""
    out = []
    for f in range(b["depth"].shape[0]):
        sel = [i for i, fo in enumerate(b["frame_of"]) if fo == f]
        if sel:
            out.append(pcl_prep.sample_instances(b["depth"][f], b["K"][f], b["masks"][sel], b["poses"][sel], b["scales"][sel],
                                                 num_points=N, seed=seeds[f], return_pixels=True, **kw))
    return tuple(torch.cat([o[k] for o in out]) for k in range(3))


# ---- without a GPU --------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    lib = hip.load()
    for n in NEW_SYMBOLS:
        assert n in hip.EXPORTED_SYMBOLS and hasattr(lib, n), n


def test_workspace_bytes_without_a_device():
    lib = hip.load()
    size, single = lib.catre_pclf_workspace_bytes, lib.catre_pcl_workspace_bytes
    assert size(0, 5, 48, 64) == 0 and size(2, 0, 48, 64) == 0 and size(2, 5, 0, 64) == 0 and size(2, 5, 48, -1) == 0
    assert size(-1, 5, 48, 64) == 0 and size(2, -5, 48, 64) == 0
    assert size(2, 5, 1 << 15, 1 << 15) == 0 and size(2, 5, 1 << 16, 1 << 16) == 0          # H*W >= 2^30 (and its int wrap)
    assert size(2, 5, 1 << 15, (1 << 15) - 1) > 0
    prev = 0
    for I in (1, 2, 3, 63, 64, 65, 160):
        for F, H, W in ((1, 7, 9), (3, 64, 64), (32, 120, 160)):
            assert size(F, I, H, W) >= single(I, H, W) > 0
        now = size(3, I, 120, 160)
        assert now > prev
        prev = now
    assert size(32, 160, 480, 640) >= 160 * 480 * 640 * 4


class _Abi:
    """valid host-side argument lists for the entry points (F = 2, I = 3, 8x8); the pointers that would be device memory
    are host memory that is never dereferenced, because the checks come first"""
    F, I, H, W = 2, 3, 8, 8

    def __init__(self):
        self.lib = hip.load()
        self.buf = (ctypes.c_double * 4096)()
        self.ok = ctypes.cast(self.buf, ctypes.c_void_p)
        self.nul = ctypes.c_void_p(0)
        self.K = (ctypes.c_float * 18)(*([50.0, 0, 4, 0, 50.0, 4, 0, 0, 1] * 2))
        self.frame_of = (ctypes.c_int32 * 3)(0, 1, 1)
        self.label_of = (ctypes.c_int32 * 3)(1, 2, 3)
        self.seeds = (ctypes.c_uint64 * 2)(1, 2)
        self.nbytes = self.lib.catre_pclf_workspace_bytes(self.F, self.I, self.H, self.W)

    def args(self, name, **kw):
        a = dict(depth=self.ok, K=self.K, frame_of=self.frame_of, rank_of=self.nul, masks=self.ok, labels=self.nul, label_bytes=0,
                 label_of=self.nul, poses=self.ok, scales=self.ok, ratio=0.5, use_ball=1, F=self.F, I=self.I, H=self.H, W=self.W,
                 ws=self.ok, ws_bytes=self.nbytes, counts=self.nul, sample_idx=self.nul, seeds=self.seeds, N=16, pcl=self.ok,
                 pix=self.nul, scratch=self.ok, cap=64, sidx_out=self.ok, stream=self.nul)
        a.update(kw)
        order = {"catre_pclf_candidates": "depth K frame_of masks labels label_bytes label_of poses scales ratio use_ball F I H W "
                                          "ws ws_bytes counts stream",
                 "catre_pclf_sample": "depth K frame_of rank_of ws ws_bytes sample_idx seeds F I H W N pcl pix stream",
                 "catre_pclf_fps": "depth K frame_of ws ws_bytes F I H W N scratch cap sidx_out stream"}[name]
        return [a[k] for k in order.split()]

    def __call__(self, name, **kw):
        return getattr(self.lib, name)(*self.args(name, **kw))


REQUIRED = {"catre_pclf_candidates": ("depth", "K", "frame_of", "poses", "scales", "ws"),
            "catre_pclf_sample": ("depth", "K", "frame_of", "ws", "pcl"),
            "catre_pclf_fps": ("depth", "K", "frame_of", "ws", "scratch", "sidx_out")}


@pytest.mark.parametrize("name", sorted(REQUIRED))
def test_entry_points_refuse_bad_arguments_before_any_launch(name):
    """No device is needed (or touched): every refusal below comes back before the staging copy and the first launch -
    on a machine without a GPU anything later would come back as a launch error (-3), not as -1 / -2."""
    abi = _Abi()
    for k in REQUIRED[name]:
        assert abi(name, **{k: abi.nul}) == -1, k                                           # null required pointers
    for k in ("F", "I", "H", "W"):
        assert abi(name, **{k: 0}) == -1 and abi(name, **{k: -2}) == -1, k                  # non-positive sizes
    assert abi(name, H=1 << 15, W=1 << 15) == -1                                             # H*W >= 2^30
    assert abi(name, I=65536, frame_of=(ctypes.c_int32 * 65536)()) == -1                     # instances are a grid dimension
    assert abi(name, frame_of=(ctypes.c_int32 * 3)(0, -1, 1)) == -1                          # frame index below 0
    assert abi(name, frame_of=(ctypes.c_int32 * 3)(0, 1, abi.F)) == -1                       # ... and at F
    for at in (0, 4, 9, 13):                                                                 # fx / fy of either frame
        K = (ctypes.c_float * 18)(*abi.K)
        K[at] = 0.0
        assert abi(name, K=K) == -1, at
    K = (ctypes.c_float * 18)(*abi.K)
    K[9] = float("nan")
    assert abi(name, K=K) == -1
    assert abi(name, ws_bytes=abi.nbytes - 1) == -2 and abi(name, ws_bytes=0) == -2          # a short workspace
    if name != "catre_pclf_candidates":
        assert abi(name, N=0) == -1
    if name == "catre_pclf_candidates":
        assert abi(name, labels=abi.ok, label_bytes=1, label_of=abi.label_of) == -1          # masks and labels
        assert abi(name, masks=abi.nul, labels=abi.ok, label_bytes=1) == -1                  # labels without label_of
        assert abi(name, masks=abi.nul, labels=abi.ok, label_bytes=2, label_of=abi.label_of) == -1
    if name == "catre_pclf_sample":
        assert abi(name, seeds=abi.nul) == -1                                                # neither slots nor seeds
    if name == "catre_pclf_fps":
        assert abi(name, cap=0) == -1


def test_sample_frames_checks_its_arguments_before_touching_a_device():
    b = make_batch(7, 9)
    I, F = len(b["frame_of"]), b["depth"].shape[0]
    labels = torch.zeros(F, 7, 9, dtype=torch.uint8)
    call = lambda **kw: pcl_prep.sample_frames(**{**dict(depth=b["depth"], K=b["K"], frame_of=b["frame_of"], poses=b["poses"],
                                                         scales=b["scales"], masks=b["masks"]), **kw})
    with pytest.raises(ValueError, match="exactly one"):
        call(masks=None)
    with pytest.raises(ValueError, match="exactly one"):
        call(labels=labels, label_of=[1] * I)
    with pytest.raises(ValueError, match="label_of"):
        call(masks=None, labels=labels)
    with pytest.raises(ValueError, match="label_of"):
        call(masks=None, labels=labels, label_of=[1] * (I + 1))
    with pytest.raises(ValueError, match="uint8 / int32"):
        call(masks=None, labels=labels.long(), label_of=[1] * I)
    with pytest.raises(ValueError, match="K must be"):
        call(K=b["K"][:2])
    with pytest.raises(ValueError, match="K must be"):
        call(K=torch.eye(4))
    with pytest.raises(ValueError, match="seed"):
        call(seed=[1, 2])
    with pytest.raises(ValueError, match=r"frame_of\[1\] = 3"):
        call(frame_of=[0, 3] + b["frame_of"][2:])
    with pytest.raises(ValueError, match=r"frame_of\[0\] = -1"):
        call(frame_of=torch.tensor([-1] + b["frame_of"][1:]))
    with pytest.raises(ValueError, match="masks must be"):
        call(masks=b["masks"][:-1])
    with pytest.raises(ValueError, match="F,H,W"):
        call(depth=b["depth"][0])
    with pytest.raises(ValueError, match="sample="):
        call(sample="numpy")
    with pytest.raises(hip.CatreHipError):                            # and there is no CPU fallback
        call()


def _golden():
    z = np.load(os.path.join(GOLDEN_DIR, "pcl_prep.npz"))
    return {k: z[k] for k in z.files}


def test_frames_loop_reproduces_the_single_frame_golden():
    g = _golden()
    t = lambda k: torch.from_numpy(g[k])
    n = int(g["meta"][0])
    for mode, ball in (("ball", True), ("mask", False)):
        got = R.frames_loop(t("in_depth")[None], t("in_K"), [0] * 5, t("in_masks"), t("in_poses"), t("in_scales"),
                            num_points=n, use_ball=ball, sample_idx=g[f"{mode}_sample_idx"])
        assert got["counts"].tolist() == g[f"{mode}_counts"].tolist()
        assert np.abs(got["pcl"].numpy() - g[f"{mode}_pcl"]).max() < 1e-7
    got = R.frames_loop(t("in_depth")[None], t("in_K"), [0] * 5, t("in_masks"), t("in_poses"), t("in_scales"), num_points=n,
                        fps=True)
    assert np.abs(got["pcl"].numpy() - g["fps_pcl"]).max() < 1e-7


# ---- on the GPU -----------------------------------------------------------------------------------------------------
SHAPES = [(120, 160), (64, 64), (7, 9)]
_cache = {}


def batch(H, W):
    if (H, W) not in _cache:
        _cache[H, W] = to_dev(make_batch(H, W))
    return _cache[H, W]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["device", "host", "fps"])
@pytest.mark.parametrize("use_ball", [True, False])
@pytest.mark.parametrize("H,W", SHAPES)
def test_batched_equals_the_per_frame_loop_bit_for_bit(H, W, use_ball, mode):
    b = batch(H, W)
    F = b["depth"].shape[0]
    assert sorted(set(b["frame_of"])) == [0, 2] and F == 3          # the middle frame has no instance
    seeds = [7, 8, 9]
    kw = dict(use_ball=use_ball, sample="host" if mode == "host" else "device", fps_sample=mode == "fps")
    torch.manual_seed(3)
    got = frames(b, seed=seeds, **kw)
    torch.manual_seed(3)
    want = loop(b, seeds, **kw)
    for name, a, w in zip(("pcl", "pix", "counts"), got, want):
        assert a.dtype == w.dtype and torch.equal(a, w), name
    assert (got[2] > 0).all() and torch.isfinite(got[0]).all()
    if mode == "device":                                               # one seed for every frame
        again = frames(b, seed=7, **kw)
        want = loop(b, [7] * F, **kw)
        assert all(torch.equal(a, w) for a, w in zip(again, want))
        assert not torch.equal(again[1], got[1])                       # the seeds of frame 2 differ


@pytest.mark.gpu
def test_instance_order_is_free():
    b = batch(120, 160)
    base = frames(b, seed=[4, 5, 6])
    order_of = [2, 0, 0, 2, 0, 2, 0, 0]
    nxt = {0: iter(range(0, 5)), 2: iter(range(5, 8))}
    src = [next(nxt[f]) for f in order_of]          # the row each interleaved instance has in frame order
    mixed = dict(b, frame_of=order_of, masks=b["masks"][src].contiguous(), poses=b["poses"][src].contiguous(),
                 scales=b["scales"][src].contiguous())
    got = frames(mixed, seed=[4, 5, 6])
    for a, w in zip(got, base):
        assert torch.equal(a, w[src])


@pytest.mark.gpu
def test_one_camera_serves_every_frame():
    b = batch(64, 64)
    K = b["K"][1]
    want = frames(dict(b, K=K[None].repeat(3, 1, 1)), seed=2)
    got = frames(dict(b, K=K), seed=torch.tensor([2, 2, 2]))
    assert all(torch.equal(a, w) for a, w in zip(got, want))
    assert not torch.equal(got[0], frames(b, seed=2)[0])               # the batch's own cameras differ from it


def _labelled(b, dtype):
    """one label image per frame painted from the masks in instance order (ids 3, 13, 23, ...) and the byte masks
    `labels == id` they stand for; plus one instance whose id (200) no pixel of its frame carries"""
    F, H, W = b["depth"].shape
    labels = torch.zeros(F, H, W, dtype=torch.int32, device=DEV)
    ids = []
    for i, f in enumerate(b["frame_of"]):
        ids.append(3 + 10 * i)
        labels[f][b["masks"][i]] = ids[-1]
    frame_of, label_of = b["frame_of"] + [2], ids + [200]
    masks = torch.stack([labels[f] == lid for f, lid in zip(frame_of, label_of)])
    ext = lambda t: torch.cat([t, t[-1:]])
    return dict(b, frame_of=frame_of, masks=masks, poses=ext(b["poses"]), scales=ext(b["scales"])), labels.to(dtype), label_of


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
@pytest.mark.parametrize("use_ball", [True, False])
def test_label_images_equal_the_byte_masks_they_stand_for(dtype, use_ball):
    b, labels, label_of = _labelled(batch(120, 160), dtype)
    want = frames(b, seed=[1, 2, 3], use_ball=use_ball)
    got = pcl_prep.sample_frames(b["depth"], b["K"], b["frame_of"], b["poses"], b["scales"], labels=labels,
                                 label_of=torch.tensor(label_of), num_points=N, seed=[1, 2, 3], use_ball=use_ball,
                                 return_pixels=True)
    for a, w in zip(got, want):
        assert torch.equal(a, w)
    assert got[2][-1] == 0 and (got[2][:-1] > 0).all()                      # the absent id selects nothing
    assert (got[0][-1] == 0).all() and (got[1][-1] == -1).all()
    fps = pcl_prep.sample_frames(b["depth"], b["K"], b["frame_of"][:-1], b["poses"][:-1], b["scales"][:-1], labels=labels,
                                 label_of=label_of[:-1], num_points=N, fps_sample=True, use_ball=use_ball)
    assert torch.equal(fps, pcl_prep.sample_frames(b["depth"], b["K"], b["frame_of"][:-1], b["poses"][:-1], b["scales"][:-1],
                                                   masks=b["masks"][:-1], num_points=N, fps_sample=True, use_ball=use_ball))


@pytest.mark.gpu
def test_golden_frame_inside_a_batch():
    g = _golden()
    n, seed = int(g["meta"][0]), int(g["meta"][1])
    t = lambda k: torch.from_numpy(g[k])
    other = make_batch(120, 160, per_frame=(0, 2, 3))
    b = to_dev(dict(depth=torch.cat([t("in_depth")[None], other["depth"][1:]]),
                    K=torch.cat([t("in_K")[None], other["K"][1:]]), frame_of=[0] * 5 + other["frame_of"],
                    masks=torch.cat([t("in_masks"), other["masks"]]), poses=torch.cat([t("in_poses"), other["poses"]]),
                    scales=torch.cat([t("in_scales"), other["scales"]])))
    call = lambda **kw: pcl_prep.sample_frames(b["depth"], b["K"], b["frame_of"], b["poses"], b["scales"], masks=b["masks"],
                                               num_points=n, return_pixels=True, **kw)
    for mode, ball in (("ball", True), ("mask", False)):
        torch.manual_seed(seed)          # the golden's draws: frame 0's instances come first
        pcl, pix, counts = call(sample="host", use_ball=ball)
        assert counts[:5].cpu().tolist() == g[f"{mode}_counts"].tolist()
        assert np.abs(pcl[:5].cpu().numpy() - g[f"{mode}_pcl"]).max() < 1e-6
    pcl, pix, counts = call(fps_sample=True)
    assert counts[:5].cpu().tolist() == g["ball_counts"].tolist()
    assert np.abs(pcl[:5].cpu().numpy() - g["fps_pcl"]).max() < 1e-6
    # the candidate counts of every frame against the oracle loop
    cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    ref = R.frames_loop(cpu["depth"], cpu["K"], cpu["frame_of"], cpu["masks"], cpu["poses"], cpu["scales"], num_points=n, fps=True)
    assert ref["counts"].tolist() == counts.cpu().tolist()


@pytest.mark.gpu
def test_an_instance_without_candidates_inside_a_batch():
    b = batch(120, 160)
    base = frames(b, seed=[4, 5, 6])
    ext = lambda t: torch.cat([t, t[:1]])
    empty = torch.zeros_like(b["masks"][:1])
    for frame in (1, 2):                      # alone in the instance-free frame / last in a frame that has others
        e = dict(b, frame_of=b["frame_of"] + [frame], masks=torch.cat([b["masks"], empty]), poses=ext(b["poses"]),
                 scales=ext(b["scales"]))
        pcl, pix, counts = frames(e, seed=[4, 5, 6])
        assert counts[-1] == 0 and (pcl[-1] == 0).all() and (pix[-1] == -1).all()
        for a, w in zip((pcl, pix, counts), base):
            assert torch.equal(a[:-1], w)
        with pytest.raises(ValueError, match=r"instance 8 \(frame %d\)" % frame):
            frames(e, sample="host")
        with pytest.raises(ValueError, match="instance 8"):
            frames(e, fps_sample=True)


@pytest.mark.gpu
def test_abi_call_count_does_not_grow_with_the_number_of_frames():
    one = to_dev(make_batch(64, 64, per_frame=(4,)))
    four = to_dev(make_batch(64, 64, per_frame=(1, 1, 1, 1)))
    assert one["depth"].shape[0] == 1 and four["depth"].shape[0] == 4 and len(one["frame_of"]) == len(four["frame_of"])
    for kw in (dict(sample="device"), dict(sample="host"), dict(fps_sample=True)):
        grew = []
        for b in (one, four):
            before = pcl_prep.abi_call_count()
            frames(b, **kw)
            grew.append(pcl_prep.abi_call_count() - before)
        assert grew[0] == grew[1] and 0 < grew[0] <= 4, (kw, grew)
    # a workspace cap cuts the INSTANCE list into groups: more calls, the same answer
    b = batch(120, 160)
    whole = frames(b, seed=[4, 5, 6])
    before = pcl_prep.abi_call_count()
    cut = frames(b, seed=[4, 5, 6], max_workspace_bytes=hip.load().catre_pclf_workspace_bytes(3, 3, 120, 160))
    assert pcl_prep.abi_call_count() - before > 6
    assert all(torch.equal(a, w) for a, w in zip(cut, whole))


@pytest.mark.gpu
def test_augmented_depth_to_clouds_to_refine_end_to_end():
    """The seam dataset -> model: augment_depth_cfg -> sample_frames -> model.refine on a 2-frame batch runs and returns
    finite poses of the right shapes (a smoke check, no parity claim)."""
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    n_pts, n_kps, n_iter = 200, 100, 2
    cfg = default_cfg(num_pcl=n_pts, num_kps=n_kps, n_iter=n_iter, device=DEV)
    cfg.INPUT.AUG_DEPTH = True
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=True)
    b = to_dev(make_batch(120, 160, per_frame=(3, 2)))
    I = len(b["frame_of"])
    np.random.seed(0)
    depth = pcl_prep.augment_depth_cfg(cfg, b["depth"], seed=1)
    assert depth is not b["depth"] and depth.shape == b["depth"].shape
    pcl = pcl_prep.sample_frames(depth, b["K"], b["frame_of"], b["poses"], b["scales"], masks=b["masks"], num_points=n_pts)
    assert pcl.shape == (I, n_pts, 3) and torch.isfinite(pcl).all()
    inputs = {k: v.to(DEV) for k, v in synth.make_inputs(I, n_pts, n_kps, seed=2).items()}
    inputs.update(pcl=pcl, obj_pose_est=b["poses"], obj_scale_est=b["scales"], K=b["K"][b["frame_of"]].to(DEV))
    out = model.eval().refine(inputs, n_iter=n_iter)
    torch.cuda.synchronize()
    pose, scale = out[f"pose_{n_iter}"], out[f"scale_{n_iter}"]
    assert pose.shape == (I, 3, 4) and scale.shape == (I, 3)
    assert torch.isfinite(pose).all() and torch.isfinite(scale).all()
