"""Row f3 at its edges: the point-cloud preparation kernels (``csrc/catre_pcl.h``) against ``oracle.pcl_oracle`` on the
CPU, at the frame shapes, list lengths and ties the golden of ``tests/test_pcl_prep.py`` (120x160, 5 instances) never
reaches: frames below one thread's 16 pixels, exactly one chunk, ragged tails, more than 256 chunks (``k_pcl_pick`` with
several chunks per thread), ``masks == NULL``, every branch of the radius search, farthest point sampling with several
slots per thread, and the keyed device permutation as a bijection.  Indices, counts and orders are compared exactly,
points to 1e-6 m absolute.

Two comparisons are exact although the kernels round differently from torch (the ball test may contract
``dx*dx + dy*dy + dz*dz`` into FMAs, the FPS centre is summed in another order).  Each rests on a precondition that an
unmarked CPU test checks on every machine: no pixel of the radius scenes lies within 4 fp32 ulps of a radius, and the
oracle's FPS picks do not move when the initial centre moves by one ulp.  With them a device mismatch is the kernel's."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pcl_oracle as PO

DEV = "cuda:0"
CHUNK = 4096  # PCL_CHUNK
TOL = 1e-6    # metres, absolute: the tolerance of tests/test_pcl_prep.py


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _k9(K):
    return (ctypes.c_float * 9)(*[float(v) for v in torch.as_tensor(K, dtype=torch.float32).reshape(-1)])


def _intrinsics(H, W):
    return torch.tensor([[0.9 * W, 0.0, W / 2 - 0.5], [0.0, 0.9 * W, H / 2 - 0.5], [0.0, 0.0, 1.0]], dtype=torch.float32)


def _run_candidates(depth, K, masks, poses, scales, ratio, use_ball):
    """``catre_pcl_candidates`` through ctypes on a ZERO-FILLED workspace (a scan mistake then gives wrong but in-range
    list positions, not wild ones).  Inputs are CPU tensors, ``masks`` may be None.  -> (workspace, bytes, counts) on
    the device plus the tensors that must outlive the call."""
    from catre_amd import hip

    lib = hip.load()
    I, (H, W) = len(poses), depth.shape
    d = depth.to(DEV).contiguous()
    m8 = masks.to(torch.uint8).to(DEV).contiguous() if masks is not None else None
    p, s = poses.to(DEV).contiguous(), scales.to(DEV).contiguous()
    nbytes = lib.catre_pcl_workspace_bytes(I, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=DEV)
    counts = torch.zeros(I, dtype=torch.int32, device=DEV)
    hip.check(lib.catre_pcl_candidates(hip.ptr(d), _k9(K), hip.ptr(m8), hip.ptr(p), hip.ptr(s), float(ratio),
                                       int(use_ball), I, H, W, hip.ptr(ws), nbytes, hip.ptr(counts), hip.stream_ptr(DEV)),
              "catre_pcl_candidates")
    torch.cuda.synchronize()
    return ws, nbytes, counts, d


def _candidates(depth, K, masks, poses, scales, ratio=0.5, use_ball=True):
    """-> (counts [I] as a list, the I ordered candidate lists as CPU int64 tensors)."""
    I, HW = len(poses), depth.numel()
    ws, _, counts, _ = _run_candidates(depth, K, masks, poses, scales, ratio, use_ball)
    cand = ws[-(((I * HW + 63) // 64) * 64):][: I * HW].reshape(I, HW).cpu()
    counts = counts.cpu().tolist()
    assert all(0 <= n <= HW for n in counts), counts
    return counts, [cand[i, :n].long() for i, n in enumerate(counts)]


def _assert_lists_equal_oracle(depth, K, masks, poses, scales, use_ball, what, ratio=0.5):
    counts, lists = _candidates(depth, K, masks, poses, scales, ratio, use_ball)
    for i in range(len(poses)):
        want, _ = PO.candidates(depth, K, None if masks is None else masks[i], poses[i], scales[i], ratio,
                                use_ball=use_ball)
        assert counts[i] == len(want), (what, i, counts[i], len(want))
        assert torch.equal(lists[i], want), (what, i)


def _small_frame(H, W, seed, n_inst=3):
    """Random depth in [0.5, 2] m, about 10 % of the pixels invalid (0, -1 and NaN in turn), random half-full masks,
    pose centres at a valid pixel's 3-D point and radii from a few centimetres to more than the frame's extent."""
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    depth = 0.5 + 1.5 * torch.rand(HW, generator=g)
    bad = (torch.rand(HW, generator=g) < 0.10).nonzero().reshape(-1)
    invalid = torch.tensor([0.0, -1.0, float("nan")])
    depth[bad] = invalid[torch.arange(len(bad)) % 3]
    if not bool((depth > 0).any()):
        depth[0] = 1.0
    depth = depth.reshape(H, W)
    K = _intrinsics(H, W)
    masks = torch.rand(n_inst, H, W, generator=g) < 0.5
    bp = PO.backproject(depth, K).reshape(-1, 3)
    valid = (depth.reshape(-1) > 0).nonzero().reshape(-1)
    poses = torch.zeros(n_inst, 3, 4)
    poses[:, :, :3] = torch.eye(3)
    for i in range(n_inst):
        poses[i, :, 3] = bp[valid[int(torch.randint(len(valid), (1,), generator=g))]]
    scales = 0.02 + 1.5 * torch.rand(n_inst, 3, generator=g) * torch.rand(n_inst, 1, generator=g)
    return dict(depth=depth, K=K, masks=masks, poses=poses, scales=scales)


def _large_frame(H, W):
    from catre_amd import synth

    sc = synth.make_depth_scene(H, W, n_inst=3, seed=2)
    g = torch.Generator().manual_seed(H * 7 + W)
    sc["rand_masks"] = torch.rand(3, H, W, generator=g) < 0.3  # the scene's blobs are empty on a one-row frame
    return sc


SMALL_FRAMES = [(1, 1), (1, 15), (1, 17), (3, 5), (64, 64), (1, 4097), (61, 67), (130, 63)]
LARGE_FRAMES = [(1040, 1024), (1, 1052677)]


def _frame(H, W):
    if (H, W) in SMALL_FRAMES:
        return _small_frame(H, W, seed=1000 * H + W)
    return _large_frame(H, W)


def _host_draws(counts, N, use_ball):
    """the draws ``sample_instances(sample="host")`` makes, in its order (instance by instance)."""
    rows = []
    for c in counts:
        rows.append(torch.randperm(PO.tiled_length(c, N))[:N] if use_ball else PO.random_sample_idx(c, N))
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# 1. candidate lists at frame-shape edges
# ---------------------------------------------------------------------------------------------------------------------
def test_frame_list_hits_the_chunk_and_scan_edges():
    """The frames are what the docstrings say they are (plain arithmetic, no kernel)."""
    px = {hw: hw[0] * hw[1] for hw in SMALL_FRAMES + LARGE_FRAMES}
    nch = {hw: -(-n // CHUNK) for hw, n in px.items()}
    assert px[(1, 15)] < 16 < px[(1, 17)] and px[(64, 64)] == CHUNK and px[(1, 4097)] == CHUNK + 1
    assert px[(61, 67)] == 4087 and px[(61, 67)] % 16 == 7
    assert px[(130, 63)] == 8190 and nch[(130, 63)] == 2
    # per = ceil(nchunks / 256) = 2: 260 chunks -> threads 0..129 own two chunks each, 130..255 none;
    # 258 chunks -> thread 128 is the last with work, the tail chunk is ragged and its last thread straddles H*W
    assert nch[(1040, 1024)] == 260 and -(-260 // 256) == 2
    assert nch[(1, 1052677)] == 258 and px[(1, 1052677)] % 16 == 5 and px[(1, 1052677)] % CHUNK != 0
    # the small frames hold a radius search that stops early with exactly 10 points (">= 10", not "> 10"), lists shorter
    # than 10 and empty ones
    ends = set()
    for H, W in SMALL_FRAMES:
        sc = _frame(H, W)
        for masks in (sc["masks"], torch.ones_like(sc["masks"])):
            for i in range(len(masks)):
                stop, _, n, _ = _radius_trace(sc["depth"], sc["K"], masks[i], sc["poses"][i], sc["scales"][i])
                ends.add((stop < 9, n))
    assert (True, 10) in ends and (False, 0) in ends and any(0 < n < 10 for _, n in ends)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SMALL_FRAMES + LARGE_FRAMES, ids=lambda v: str(v))
def test_hip_candidate_lists_at_frame_shape_edges(H, W):
    """Counts and ordered lists equal the oracle's for every instance: with and without the ball, with masks and with
    ``masks == NULL`` (whole frame).  Depth 0, -1 and NaN never become candidates."""
    sc = _frame(H, W)
    depth, K, poses, scales = sc["depth"], sc["K"], sc["poses"], sc["scales"]
    mask_sets = [("masks", sc["masks"]), ("null", None)]
    if "rand_masks" in sc:
        mask_sets.append(("rand_masks", sc["rand_masks"]))
    for (mname, masks), use_ball in itertools.product(mask_sets, (False, True)):
        _assert_lists_equal_oracle(depth, K, masks, poses, scales, use_ball, (H, W, mname, use_ball))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,N", [(61, 67, 64), (1040, 1024, 256)])
def test_hip_host_sampling_at_frame_shape_edges(H, W, N):
    """``sample_instances(sample="host")`` under the same ``torch.manual_seed`` returns the oracle's points and pixels,
    with masks and with ``masks=None``, ball and mask crop."""
    from catre_amd import pcl_prep

    sc = _frame(H, W)
    depth, K, poses, scales = sc["depth"], sc["K"], sc["poses"], sc["scales"]
    for masks, use_ball in itertools.product((sc["masks"], None), (True, False)):
        lists = [PO.candidates(depth, K, None if masks is None else masks[i], poses[i], scales[i], 0.5,
                               use_ball=use_ball) for i in range(len(poses))]
        torch.manual_seed(11)
        draws = _host_draws([len(p) for p, _ in lists], N, use_ball)
        torch.manual_seed(11)
        pcl, pix, counts = pcl_prep.sample_instances(depth.to(DEV), K, None if masks is None else masks.to(DEV),
                                                     poses.to(DEV), scales.to(DEV), ratio=0.5, num_points=N,
                                                     use_ball=use_ball, sample="host", return_pixels=True)
        assert counts.cpu().tolist() == [len(p) for p, _ in lists]
        for i, ((cand, bp), idx) in enumerate(zip(lists, draws)):
            want, sel = PO.sample(cand, bp, idx)
            assert torch.equal(pix[i].cpu().long(), sel), (masks is None, use_ball, i)
            assert (pcl[i].cpu() - want).abs().max().item() <= TOL, (masks is None, use_ball, i)


# ---------------------------------------------------------------------------------------------------------------------
# 2. radius search over many instances
# ---------------------------------------------------------------------------------------------------------------------
RADIUS_SEEDS = (0, 1, 2)
N_RADIUS_INST = 64


@functools.lru_cache(maxsize=None)
def _radius_scene(seed):
    """64 instances on the 120x160 scene: its masks round-robin, pose centres at a random masked point moved by 0,
    0.03, 0.2 or 2.0 m in a random direction, scales multiplied by a factor in [0.02, 1.5].  Even instances draw offset
    and factor at random.  Odd instances are aimed, because a random factor rarely lands in the narrow window of one
    particular growth step: offset 0.2 m and the factor that puts the 10th nearest masked point (on a mask of a few
    pixels: the gap after the 6th) into the middle of a growth step ``j`` that cycles through 0..9 - kept only if that
    factor lies in [0.02, 1.5] and the radius above the 0.05 floor, otherwise the random draw stands."""
    from catre_amd import synth

    sc = synth.make_depth_scene(seed=seed)
    g = torch.Generator().manual_seed(7000 + seed)
    depth, K = sc["depth"], sc["K"]
    bp = PO.backproject(depth, K).reshape(-1, 3)
    n0 = len(sc["masks"])
    masks = torch.stack([sc["masks"][i % n0] for i in range(N_RADIUS_INST)])
    poses = torch.stack([sc["poses"][i % n0] for i in range(N_RADIUS_INST)]).clone()
    scales = torch.stack([sc["scales"][i % n0] for i in range(N_RADIUS_INST)]).clone()
    offsets = (0.0, 0.03, 0.2, 2.0)
    for i in range(N_RADIUS_INST):
        pix = torch.logical_and(masks[i].reshape(-1), depth.reshape(-1) > 0).nonzero().reshape(-1)
        at = bp[pix[int(torch.randint(len(pix), (1,), generator=g))]]
        direction = torch.randn(3, generator=g)
        off = offsets[int(torch.randint(4, (1,), generator=g))]
        factor = 0.02 + 1.48 * float(torch.rand(1, generator=g))
        if i % 2 == 1:
            off, j = 0.2, (i // 2 + i // 20) % 10  # the shift per decade keeps j from pairing with one mask
        poses[i, :, 3] = at + off * direction / direction.norm()
        if i % 2 == 1:
            d = torch.sqrt(((bp[pix] - poses[i, :, 3]) ** 2).sum(-1)).sort()[0].double()
            if len(d) >= 20:      # the 10th nearest point in the middle of step j (j = 0: inside the first radius)
                r0 = float(d[9]) / 1.1 ** (j - 0.5)
            elif len(d) >= 7:     # a mask of a few pixels: six points inside the last radius, the seventh outside
                r0 = 0.5 * float(d[5] + d[6]) / 1.1 ** 9
            else:
                r0 = 0.0
            aimed = r0 / float(0.5 * torch.norm(poses[i, :, :3] @ scales[i]))
            if 0.02 <= aimed <= 1.5 and r0 > 0.051:
                factor = aimed
        scales[i] = scales[i] * factor
    return dict(depth=depth, K=K, masks=masks, poses=poses, scales=scales)


def _radius_trace(depth, K, mask, pose, scale, ratio=0.5):
    """The loop of ``PO.candidates`` with its bookkeeping exposed: -> (radius index at which it stopped, fell back to
    every masked pixel?, final list length, masked pixels whose float64 distance lies within 4 fp32 ulps of one of
    the ten radii)."""
    bp = PO.backproject(depth, K).reshape(-1, 3)
    pix = torch.logical_and(mask.reshape(-1), bp[:, 2] > 0).nonzero().reshape(-1)
    pts = bp[pix]
    centre = pose[:, 3]
    radius = ratio * torch.norm(pose[:, :3] @ scale)
    distance = torch.sqrt(((pts - centre) ** 2).sum(-1))
    d64 = torch.sqrt(((pts.double() - centre.double()) ** 2).sum(-1)).numpy()
    radius = max(radius, 0.05)
    stop, idx, borderline = None, None, 0
    for i in range(10):  # all ten radii, also past the one the oracle stops at: the kernel bins against every one
        r32 = np.float32(float(radius))
        borderline += int((np.abs(d64 - np.float64(r32)) <= 4.0 * np.float64(np.spacing(r32))).sum())
        if stop is None:
            inside = torch.where(distance <= radius)[0]
            if len(inside) >= 10 or i == 9:
                stop, idx = i, inside
        radius *= 1.10
    fallback = len(idx) == 0
    n = len(pix) if fallback else len(idx)
    want, _ = PO.candidates(depth, K, mask, pose, scale, ratio)
    assert len(want) == n, "the trace drifted from the oracle"
    return stop, fallback, n, borderline


@pytest.mark.parametrize("seed", RADIUS_SEEDS)
def test_radius_scenes_cover_every_branch_and_have_no_borderline_pixel(seed):
    """Precondition of the exact comparison below, on the CPU: no masked pixel within 4 fp32 ulps of any of an
    instance's ten radii (the kernel may round ``d`` and ``r`` a little differently from torch), and coverage: every
    radius index 0..9 stops the search somewhere, the every-masked-pixel fallback occurs, a list shorter than 10
    occurs."""
    sc = _radius_scene(seed)
    stops, fallbacks, short, borderline = set(), 0, 0, 0
    for i in range(N_RADIUS_INST):
        stop, fb, n, bl = _radius_trace(sc["depth"], sc["K"], sc["masks"][i], sc["poses"][i], sc["scales"][i])
        borderline += bl
        fallbacks += fb
        if not fb:
            stops.add(stop)
            short += 0 < n < 10
    assert borderline == 0
    assert stops == set(range(10)), sorted(stops)
    assert fallbacks > 0
    assert short > 0


def test_radius_scene_2_holds_an_instance_that_ends_with_six_candidates():
    sc = _radius_scene(2)
    ns = [len(PO.candidates(sc["depth"], sc["K"], sc["masks"][i], sc["poses"][i], sc["scales"][i], 0.5)[0])
          for i in range(N_RADIUS_INST)]
    assert 6 in ns, sorted(set(n for n in ns if n < 10))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", RADIUS_SEEDS)
def test_hip_radius_search_over_many_instances(seed):
    """All 64 instances in one call: counts and ordered lists exactly the oracle's, nothing skipped."""
    sc = _radius_scene(seed)
    _assert_lists_equal_oracle(sc["depth"], sc["K"], sc["masks"], sc["poses"], sc["scales"], True, ("radius", seed))


def _on_the_radius_scene():
    """5x5 frame whose centre pixel lies on the optical axis at depth 1.0; pose centre (0, 0, 0.75), R = 1,
    scale (0.5, 0, 0): radius 0.5 * 0.5 = 0.25 and the centre pixel's distance sqrt(0 + 0 + 0.25^2) = 0.25, both exact
    in fp32 under any rounding or contraction.  The other 24 pixels (depth 0.8) lie well inside."""
    depth = torch.full((5, 5), 0.8)
    depth[2, 2] = 1.0
    K = torch.tensor([[100.0, 0.0, 2.0], [0.0, 100.0, 2.0], [0.0, 0.0, 1.0]])
    pose = torch.cat([torch.eye(3), torch.tensor([[0.0], [0.0], [0.75]])], dim=1)
    return depth, K, torch.ones(1, 5, 5, dtype=torch.bool), pose[None], torch.tensor([[0.5, 0.0, 0.0]])


def test_on_the_radius_scene_has_a_pixel_at_exactly_the_radius():
    depth, K, masks, poses, scales = _on_the_radius_scene()
    bp = PO.backproject(depth, K).reshape(-1, 3)
    d = torch.sqrt(((bp - poses[0, :, 3]) ** 2).sum(-1))
    assert float(d[12]) == 0.25 == float(0.5 * torch.norm(poses[0, :, :3] @ scales[0])) and int((d < 0.25).sum()) == 24
    assert len(PO.candidates(depth, K, masks[0], poses[0], scales[0], 0.5)[0]) == 25


@pytest.mark.gpu
def test_hip_pixel_exactly_on_the_radius_is_inside():
    """``distance <= radius``: the reference keeps a point at exactly the radius."""
    depth, K, masks, poses, scales = _on_the_radius_scene()
    _assert_lists_equal_oracle(depth, K, masks, poses, scales, True, "on the radius")
    _assert_lists_equal_oracle(depth, K, None, poses, scales, True, "on the radius, no mask")


# ---------------------------------------------------------------------------------------------------------------------
# 3. farthest point sampling, exact and complete
# ---------------------------------------------------------------------------------------------------------------------
FPS_SCENES = {
    # name: (make_depth_scene arguments, num_points, the oracle's candidate counts)
    "A": (dict(seed=5, H=240, W=320, n_inst=5), 128, [1972, 32, 435, 1974, 12]),
    "B": (dict(seed=5, H=480, W=640, n_inst=3), 256, [7881, 45, 1383]),
    # mask crops of exactly 512 and 300 pixels with N = 1100: lists tiled to 2048 and 1200 slots.  Slot j and slot
    # j + 1024 of the first are the same point and belong to the same thread (an exact tie inside the strided per-thread
    # arg-max); after 512 (300) picks every slot ties at |(1e-6, 1e-6, 1e-6)| and the reference picks slot 0 from there on.
    "C": (None, 1100, [512, 300]),
}


@functools.lru_cache(maxsize=None)
def _fps_scene(name):
    """The scene, its candidate lists and the oracle's picks: computed once, shared, never modified."""
    from catre_amd import synth

    kw, N, counts = FPS_SCENES[name]
    if kw is None:
        depth, K = _perm_frame()
        sc = dict(depth=depth, K=K, masks=_masks_with(counts, seed=512), poses=None, scales=None, use_ball=False)
    else:
        sc = dict(synth.make_depth_scene(**kw), use_ball=True)
    lists, picks, bp = [], [], None
    for i in range(len(sc["masks"])):
        pose, scale = (sc["poses"][i], sc["scales"][i]) if sc["use_ball"] else (None, None)
        pix, bp = PO.candidates(sc["depth"], sc["K"], sc["masks"][i], pose, scale, 0.5, use_ball=sc["use_ball"])
        lists.append(pix)
        picks.append(PO.fps_sample_idx(pix, bp, N))
    return dict(sc, N=N, lists=lists, picks=torch.stack(picks), bp=bp)


def _tiled_points(sc, i):
    pix = sc["lists"][i]
    L = PO.tiled_length(len(pix), sc["N"])
    return sc["bp"][pix[torch.arange(L) % len(pix)]]


def _fps_from_centres(points, centres, n):
    """``PO.farthest_points`` run for M initial centres at once (one row each): -> picks [M, n]."""
    M, L = len(centres), len(points)
    every = points.unsqueeze(0).expand(M, L, 3)
    dist = F.pairwise_distance(centres.unsqueeze(1).expand(M, L, 3), every)
    picks = torch.zeros(M, n, dtype=torch.long)
    for i in range(n):
        c = torch.argmax(dist, dim=1)
        picks[:, i] = c
        dist = torch.min(dist, F.pairwise_distance(points[c].unsqueeze(1).expand(M, L, 3), every))
    return picks


def test_fps_scenes_have_the_list_lengths_the_tests_rely_on():
    for name, (_, N, counts) in FPS_SCENES.items():
        sc = _fps_scene(name)
        assert [len(p) for p in sc["lists"]] == counts, name
    # scene A, N = 128: two slots per thread twice, one list below 1024, 12 tiled x16 to 192, 32 tiled to 128 = N
    assert [PO.tiled_length(c, 128) for c in FPS_SCENES["A"][2]] == [1972, 128, 435, 1974, 192]
    assert torch.equal(_fps_scene("A")["picks"][1], torch.arange(128))
    # scene B, N = 256: 7881 slots = 8 per thread (the last round partly empty), 45 tiled x8 to 360
    assert -(-7881 // 1024) == 8 and PO.tiled_length(45, 256) == 360
    # scene C, N = 1100: 2048 = 2 * 1024 slots, every pick after the last distinct point is slot 0
    c = _fps_scene("C")
    assert [PO.tiled_length(n, 1100) for n in FPS_SCENES["C"][2]] == [2048, 1200]
    assert sorted(c["picks"][0][:512].tolist()) == list(range(512)) and (c["picks"][0][512:] == 0).all()
    assert sorted(c["picks"][1][:300].tolist()) == list(range(300)) and (c["picks"][1][300:] == 0).all()


@pytest.mark.parametrize("name", sorted(FPS_SCENES))
def test_fps_oracle_picks_do_not_move_with_the_centre_rounding(name):
    """Precondition of the exact FPS comparison, on the CPU.  The kernel sums the centre in another order than
    ``torch.mean``; the oracle's picks stay the same when the centre - the fp32 mean, or the float64 mean rounded -
    moves by +-1 ulp in any combination of coordinates, so no rounding of the centre changes a pick."""
    sc = _fps_scene(name)
    N = sc["N"]
    for i in range(len(sc["lists"])):
        pts = _tiled_points(sc, i)
        if N >= len(pts):
            continue
        centres = [pts.mean(0)]  # row 0: the oracle's own centre, which must reproduce its picks
        for centre in (pts.mean(0), pts.double().mean(0).float()):
            c = centre.numpy()
            lo, hi = np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))
            for sel in itertools.product(range(3), repeat=3):
                centres.append(torch.tensor([(lo[k], c[k], hi[k])[s] for k, s in enumerate(sel)], dtype=torch.float32))
        got = _fps_from_centres(pts, torch.stack(centres), N)
        for row in range(len(centres)):
            assert torch.equal(got[row], sc["picks"][i]), (name, i, row)


def _device_fps(sc):
    from catre_amd import pcl_prep

    poses, scales = (sc["poses"].to(DEV), sc["scales"].to(DEV)) if sc["use_ball"] else (None, None)
    return pcl_prep.sample_instances(sc["depth"].to(DEV), sc["K"], sc["masks"].to(DEV), poses, scales, ratio=0.5,
                                     num_points=sc["N"], use_ball=sc["use_ball"], fps_sample=True, return_pixels=True)


def _picked_pixels(sc):
    return torch.stack([pix[s % len(pix)] for pix, s in zip(sc["lists"], sc["picks"])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FPS_SCENES))
def test_hip_fps_full_pick_order_equals_the_oracle(name):
    """Every pick of every instance, in order: lists with 2 and 8 slots per thread, a list tiled x16 (duplicated
    points: exact ties that only "first maximum wins" resolves), ``N >= L`` (identity), all sharing one slot_cap; on
    scene C ties between the two slots of one thread and, once every point is taken, between all slots."""
    sc = _fps_scene(name)
    pcl, pix, counts = _device_fps(sc)
    assert counts.cpu().tolist() == FPS_SCENES[name][2]
    want_pix = _picked_pixels(sc)
    got = pix.cpu().long()
    for i in range(len(want_pix)):
        bad = (got[i] != want_pix[i]).nonzero().reshape(-1)
        assert len(bad) == 0, f"scene {name} instance {i}: first differing pick {int(bad[0])} of {sc['N']}"
    assert (pcl.cpu() - sc["bp"][want_pix]).abs().max().item() <= TOL


@pytest.mark.gpu
def test_hip_fps_every_pick_is_greedy_farthest_on_scene_b():
    """Independent of the oracle's picks: in float64, pick k has the largest running min-distance over all slots given
    the centre distances and picks 0..k-1, for all N picks (slack 1e-6 m: more than 4 fp32 ulps of the scene's largest
    coordinate, which is below 4 m)."""
    sc = _fps_scene("B")
    assert float(sc["bp"][torch.cat(sc["lists"])].abs().max()) < 4.0
    _, pix, _ = _device_fps(sc)
    pix = pix.cpu().long()
    for i, cand in enumerate(sc["lists"]):
        pts = _tiled_points(sc, i).double()
        assert sc["N"] < len(pts)
        # slot of each device pick: the first copy of its pixel in the tiled list (every copy is the same point and
        # so carries the same running distance)
        pos = {int(p): j for j, p in enumerate(cand.tolist())}
        slots = torch.tensor([pos[int(p)] for p in pix[i]])
        run = (pts.mean(0) - pts + 1e-6).norm(dim=1)
        for k in range(sc["N"]):
            s = int(slots[k])
            assert run[s] >= run.max() - 1e-6, (i, k, float(run[s]), float(run.max()))
            run = torch.minimum(run, (pts[s] - pts + 1e-6).norm(dim=1))


@pytest.mark.gpu
def test_hip_fps_stays_inside_its_scratch():
    """``catre_pcl_fps`` called directly on scene A with a sentinel-filled scratch of ``I*4*cap + 1024`` floats: the tail
    comes back untouched, an instance with a list shorter than ``cap`` leaves the rest of its four arrays alone, the
    identity instance writes nothing, and the picks are the wrapper's."""
    from catre_amd import hip

    sc = _fps_scene("A")
    N, I = sc["N"], len(sc["lists"])
    H, W = sc["depth"].shape
    lens = [PO.tiled_length(len(p), N) for p in sc["lists"]]
    cap = max(lens)
    lib = hip.load()
    ws, nbytes, counts, d = _run_candidates(sc["depth"], sc["K"], sc["masks"], sc["poses"], sc["scales"], 0.5, True)
    assert counts.cpu().tolist() == FPS_SCENES["A"][2]
    sentinel = -12345.0
    scratch = torch.full((I * 4 * cap + 1024,), sentinel, dtype=torch.float32, device=DEV)
    sidx = torch.full((I, N), -1, dtype=torch.int64, device=DEV)
    hip.check(lib.catre_pcl_fps(hip.ptr(d), _k9(sc["K"]), hip.ptr(ws), nbytes, I, H, W, N, hip.ptr(scratch), cap,
                                hip.ptr(sidx), hip.stream_ptr(DEV)), "catre_pcl_fps")
    torch.cuda.synchronize()
    got = scratch.cpu()
    assert (got[I * 4 * cap:] == sentinel).all(), "wrote past I*4*slot_cap floats"
    per_inst = got[: I * 4 * cap].reshape(I, 4, cap)
    for i, L in enumerate(lens):
        used = L if N < L else 0  # N >= L: identity order, no scratch
        assert (per_inst[i, :, used:] == sentinel).all(), (i, L)
        assert (per_inst[i, :, :used] != sentinel).all(), (i, L)
    assert torch.equal(sidx.cpu(), sc["picks"])
    _, pix, _ = _device_fps(sc)
    assert torch.equal(pix.cpu().long(), _picked_pixels(sc))


# ---------------------------------------------------------------------------------------------------------------------
# 4. device permutation
# ---------------------------------------------------------------------------------------------------------------------
PERM_H, PERM_W = 72, 64  # 4608 px: more than one chunk, room for 4097 masked pixels


@functools.lru_cache(maxsize=None)
def _perm_frame():
    g = torch.Generator().manual_seed(99)
    depth = 0.5 + 1.5 * torch.rand(PERM_H, PERM_W, generator=g)  # positive everywhere
    return depth, _intrinsics(PERM_H, PERM_W)


def _masks_with(counts, seed):
    """one mask per entry of ``counts`` holding exactly that many pixels."""
    g = torch.Generator().manual_seed(seed)
    masks = torch.zeros(len(counts), PERM_H * PERM_W, dtype=torch.bool)
    for i, c in enumerate(counts):
        masks[i, torch.randperm(PERM_H * PERM_W, generator=g)[:c]] = True
    return masks.reshape(len(counts), PERM_H, PERM_W)


def _device_sample(masks, N, seed):
    from catre_amd import pcl_prep

    depth, K = _perm_frame()
    pcl, pix, counts = pcl_prep.sample_instances(depth.to(DEV), K, masks.to(DEV), num_points=N, use_ball=False,
                                                 sample="device", seed=seed, return_pixels=True)
    pix = pix.cpu().long()
    assert counts.cpu().tolist() == masks.reshape(len(masks), -1).sum(1).tolist()
    bp = PO.backproject(depth, K).reshape(-1, 3)
    assert (pcl.cpu() - bp[pix]).abs().max().item() <= TOL
    return pix


def _candidate_set(mask):
    depth, K = _perm_frame()
    return PO.candidates(depth, K, mask, use_ball=False)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_hip_device_permutation_is_a_bijection(c):
    """``N = c``: the returned pixels are exactly the candidate set, each pixel once - at every bit-width edge of the
    Feistel walk (``L = 1..4`` on 2 bits, odd bit counts rounded up, ``L`` one below, at and one above a power of two).
    Three instances with their own masks share the call."""
    masks = _masks_with([c, c, c], seed=c)
    pix = _device_sample(masks, c, seed=3)
    for i in range(len(masks)):
        assert torch.equal(pix[i].sort()[0], _candidate_set(masks[i])), (c, i)


@pytest.mark.gpu
def test_hip_device_permutation_multiplicities_on_tiled_lists():
    """``N = 64``.  ``c`` a power of two: the list is tiled to exactly 64 slots and the permutation visits each once, so
    every candidate appears exactly ``64 / c`` times.  ``c`` in {3, 5, 33}: tiled to ``L`` = 96, 80, 66 slots of which 64
    are drawn, no candidate more than ``L / c`` times and none from outside the set."""
    N = 64
    exact, bounded = [1, 2, 4, 8, 16, 32, 64], [3, 5, 33]
    masks = _masks_with(exact + bounded, seed=64)
    pix = _device_sample(masks, N, seed=9)
    for i, c in enumerate(exact + bounded):
        want = _candidate_set(masks[i])
        values, times = pix[i].unique(return_counts=True)
        assert set(values.tolist()) <= set(want.tolist()), c
        if c in exact:
            assert torch.equal(values, want) and (times == N // c).all(), (c, times.tolist())
        else:
            L = PO.tiled_length(c, N)
            assert L % c == 0 and int(times.max()) <= L // c, (c, times.tolist())


@pytest.mark.gpu
def test_hip_device_permutation_depends_on_seed_and_instance_only():
    """``c = N = 1024``, two instances with the same mask: the same seed repeats the result, another seed and the other
    instance give another order of the same set (an accidental match of 1024! orders does not happen)."""
    one = _masks_with([1024], seed=1024)
    masks = torch.cat([one, one])
    a = _device_sample(masks, 1024, seed=5)
    b = _device_sample(masks, 1024, seed=5)
    c = _device_sample(masks, 1024, seed=6)
    assert torch.equal(a, b)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    assert not torch.equal(a[0], a[1])
    want = _candidate_set(one[0])
    for row in (a[0], a[1], c[0], c[1]):
        assert torch.equal(row.sort()[0], want)


# ---------------------------------------------------------------------------------------------------------------------
# 5. entry-point contracts
# ---------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_is_zero_for_every_frame_the_library_refuses():
    """Host arithmetic only.  ``I``, ``H`` or ``W`` <= 0 -> 0; ``H*W >= 2^30`` (the limit ``catre_pcl_candidates``
    enforces) -> 0 as well, with the product taken in ``size_t``: 65536 x 65536 wraps to 0 in ``int``."""
    from catre_amd import hip

    size = hip.load().catre_pcl_workspace_bytes
    assert size(1, 120, 160) > 0
    for bad in [(0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, 4), (1, 4, -4), (0, 0, 0)]:
        assert size(*bad) == 0, bad
    for H, W in [(65536, 65536), (32768, 32768), (1, 1 << 30), (1 << 30, 1), (46341, 46341), (2**31 - 1, 2**31 - 1),
                 (65536, 32768), (3, 1 << 29)]:
        assert H * W >= 1 << 30
        assert size(1, H, W) == 0, (H, W)
    # just below the limit the size is the real one: every array of the layout, at least the I*H*W list entries
    H, W = 32768, 32767
    assert size(2, H, W) >= 2 * H * W * 4 + 2 * (-(-H * W // CHUNK)) * 13 * 4


class _PclCall:
    """valid arguments of the three entry points on a tiny frame, for one-at-a-time spoiling."""

    def __init__(self):
        from catre_amd import hip

        self.hip, self.lib = hip, hip.load()
        self.I, self.H, self.W, self.N, self.cap = 2, 8, 16, 32, 128
        sc = _small_frame(self.H, self.W, seed=5, n_inst=self.I)
        self.k9 = _k9(sc["K"])
        self.depth = sc["depth"].to(DEV)
        self.masks = sc["masks"].to(torch.uint8).to(DEV)
        self.poses, self.scales = sc["poses"].to(DEV), sc["scales"].to(DEV)
        self.nbytes = self.lib.catre_pcl_workspace_bytes(self.I, self.H, self.W)
        self.ws = torch.zeros(self.nbytes // 4, dtype=torch.int32, device=DEV)
        self.counts = torch.zeros(self.I, dtype=torch.int32, device=DEV)
        self.scratch = torch.zeros(self.I * 4 * self.cap, dtype=torch.float32, device=DEV)
        self.sidx = torch.zeros(self.I, self.N, dtype=torch.int64, device=DEV)
        self.pcl = torch.zeros(self.I, self.N, 3, dtype=torch.float32, device=DEV)
        self.pix = torch.zeros(self.I, self.N, dtype=torch.int32, device=DEV)
        self.st = hip.stream_ptr(DEV)

    def args(self, name):
        p = self.hip.ptr
        if name == "catre_pcl_candidates":
            return [p(self.depth), self.k9, p(self.masks), p(self.poses), p(self.scales), 0.5, 1, self.I, self.H, self.W,
                    p(self.ws), self.nbytes, p(self.counts), self.st]
        if name == "catre_pcl_sample":
            return [p(self.depth), self.k9, p(self.ws), self.nbytes, None, 7, self.I, self.H, self.W, self.N, p(self.pcl),
                    p(self.pix), self.st]
        return [p(self.depth), self.k9, p(self.ws), self.nbytes, self.I, self.H, self.W, self.N, p(self.scratch), self.cap,
                p(self.sidx), self.st]


# position of the workspace size and of every required pointer in each argument list
PCL_ENTRY_POINTS = {
    "catre_pcl_candidates": dict(ws_bytes=11, required=[0, 1, 3, 4, 10]),
    "catre_pcl_sample": dict(ws_bytes=3, required=[0, 1, 2, 10]),
    "catre_pcl_fps": dict(ws_bytes=3, required=[0, 1, 2, 8, 10]),
}
ERR_WORKSPACE = -2  # CATRE_ERR_WORKSPACE


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PCL_ENTRY_POINTS))
def test_hip_pcl_entry_points_refuse_a_short_workspace_and_null_pointers(name):
    """A workspace one byte short and any required NULL pointer: a non-zero status and nothing launched (every output
    buffer still holds its zeros).  The unspoiled call succeeds, so the refusals are the spoiled argument's."""
    call = _PclCall()
    fn, spec = getattr(call.lib, name), PCL_ENTRY_POINTS[name]
    outputs = [call.ws, call.counts, call.scratch, call.sidx, call.pcl, call.pix]
    short = call.args(name)
    short[spec["ws_bytes"]] -= 1
    assert fn(*short) == ERR_WORKSPACE
    for k in spec["required"]:
        spoiled = call.args(name)
        spoiled[k] = None
        assert fn(*spoiled) != 0, (name, k)
    torch.cuda.synchronize()
    assert all(int(t.count_nonzero()) == 0 for t in outputs), "a refused call wrote something"
    if name != "catre_pcl_candidates":
        call.hip.check(call.lib.catre_pcl_candidates(*call.args("catre_pcl_candidates")), "catre_pcl_candidates")
    call.hip.check(fn(*call.args(name)), name)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(65536, 65536), (32768, 32768), (1, 1 << 30)])
def test_hip_pcl_candidates_refuses_frames_of_2_to_the_30_pixels(H, W):
    """Sizes only: the argument check comes before any access, so the tiny buffers are never touched."""
    call = _PclCall()
    a = call.args("catre_pcl_candidates")
    a[8], a[9] = H, W
    assert call.lib.catre_pcl_candidates(*a) != 0
    torch.cuda.synchronize()
    assert int(call.ws.count_nonzero()) == 0 and int(call.counts.count_nonzero()) == 0
