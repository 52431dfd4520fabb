"""Depth augmentation of the loader (``INPUT.AUG_DEPTH``: fill holes, drop pixels, add noise) on the device -
``catre_amd.pcl_prep.augment_depth`` / ``augment_depth_cfg`` over ``catre_depth_augment``.

Two contracts.  Draws mode: with the reference's float64 draws the kernel gives the reference's bits - every stage of
``tests/golden/depth_aug.npz`` (recorded with the reference's ``add_noise_depth``, ``tools/make_depth_aug_golden.py``),
compared as bit patterns so that -0.0 is not 0.0.  Device mode: a counter-based stream of its own; its distribution is
checked with 5-sigma bounds of the stated distributions (false-alarm rate ~6e-7 per check), derived from the sample
sizes, and its independence of launch geometry, batch size and slot is checked exactly."""
import ctypes
import random

import numpy as np
import pytest
import torch

from catre_amd import hip, pcl_prep
from catre_amd.config import CfgNode
from tests import pcl_frames_ref as R

DEV = "cuda:0"
STAGES = ("after_fill", "after_drop", "after_noise")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _frame(g, k):
    return {n[len(f"f{k}/"):]: v for n, v in g.items() if n.startswith(f"f{k}/")}


# ---- without a GPU --------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    assert "catre_depth_augment" in hip.EXPORTED_SYMBOLS and hasattr(hip.load(), "catre_depth_augment")
    assert pcl_prep._DAUG_FRAME.itemsize == 32          # sizeof(catre_depth_aug_frame), asserted in the library too


def test_bad_arguments_return_bad_arg_without_a_device():
    lib, nul = hip.load(), ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    ok = ctypes.cast(buf, ctypes.c_void_p)      # host memory: never dereferenced, the checks come first
    call = lambda **kw: lib.catre_depth_augment(*[{**dict(din=ok, u16=0, div=1000.0, fr=ok, draws=0, a=nul, b=nul, c=nul, seed=0,
                                                         out=ok, F=2, H=4, W=4, st=nul), **kw}[k]
                                                  for k in ("din", "u16", "div", "fr", "draws", "a", "b", "c", "seed", "out", "F",
                                                            "H", "W", "st")])
    assert call(din=nul) == -1 and call(fr=nul) == -1 and call(out=nul) == -1          # null arrays
    assert call(F=0) == -1 and call(H=0) == -1 and call(W=-3) == -1                    # non-positive sizes
    assert call(F=65536) == -1                                                         # frames are a grid dimension
    assert call(H=1 << 15, W=1 << 15) == -1                                            # H*W >= 2^30
    assert call(u16=1, div=0.0) == -1 and call(u16=1, div=float("nan")) == -1          # no division by zero


def test_augment_depth_checks_its_arguments_before_touching_a_device():
    d = torch.ones(2, 4, 5)
    kw = dict(fill_holes=True, drop=[True, False], drop_ratio=0.2, noise_level=[0.01, 0.0])
    with pytest.raises(ValueError, match="F,H,W"):
        pcl_prep.augment_depth(d[0], **kw)
    with pytest.raises(ValueError, match="float32"):
        pcl_prep.augment_depth(d.double(), **kw)
    with pytest.raises(ValueError, match="drop"):
        pcl_prep.augment_depth(d, **{**kw, "drop": [True, False, True]})
    with pytest.raises(ValueError, match="noise_level"):
        pcl_prep.augment_depth(d, **{**kw, "noise_level": [0.01]})
    with pytest.raises(ValueError, match="frame_keys"):
        pcl_prep.augment_depth(d, frame_keys=[1, 2, 3], **kw)
    with pytest.raises(ValueError, match="drop_ratio"):
        pcl_prep.augment_depth(d, **{**kw, "drop_ratio": 1.5})
    with pytest.raises(ValueError, match="depth_div"):
        pcl_prep.augment_depth(d, depth_div=1000.0, **kw)
    z = torch.zeros(2, 4, 5, dtype=torch.float64)
    with pytest.raises(ValueError, match="keep"):                     # a step that runs needs its draws
        pcl_prep.augment_depth(d, draws=dict(fill=z, gauss=z), **kw)
    with pytest.raises(ValueError, match="gauss"):
        pcl_prep.augment_depth(d, draws=dict(fill=z, keep=z, gauss=z.float()), **kw)
    with pytest.raises(ValueError, match="unknown"):
        pcl_prep.augment_depth(d, draws=dict(fill=z, keep=z, gauss=z, extra=z), **kw)
    with pytest.raises(hip.CatreHipError):                            # and there is no CPU fallback
        pcl_prep.augment_depth(d, **kw)


def test_numpy_restatement_reproduces_every_golden_stage_bit_for_bit():
    g = R.depth_aug_golden()
    ratio = float(g["drop_ratio"])
    for k in range(2):
        f = _frame(g, k)
        got = R.augment(f["raw"], fill=f["draw_fill"], keep=f["draw_keep"], ratio=ratio, level=float(f["level"]),
                        gauss=f["draw_gauss"])
        for stage in ("metres",) + STAGES:
            assert got[stage].dtype == np.float32 and np.array_equal(_bits(got[stage]), _bits(f[stage])), (k, stage)
        # the fixture exercises what the steps have to get right: negative fills, dropped ones (-0.0), untouched pixels
        assert (f["after_fill"] < 0).any() and np.signbit(f["after_drop"][f["after_drop"] == 0]).any()
        assert (f["after_noise"][f["after_drop"] <= 0] == f["after_drop"][f["after_drop"] <= 0]).all()
        assert (f["after_noise"] != f["after_drop"])[f["after_drop"] > 0].mean() > 0.99


def test_augment_depth_cfg_draws_the_loaders_coins_in_the_loaders_order(monkeypatch):
    g = R.depth_aug_golden()
    seen = {}
    monkeypatch.setattr(pcl_prep, "augment_depth", lambda depth, **kw: seen.update(kw) or "augmented")
    F = len(g["cfg_drop"])
    cfg = CfgNode(INPUT=dict(AUG_DEPTH=True))          # the probabilities, ratio and level default to the base config's
    np.random.seed(int(g["cfg_np_seed"]))
    random.seed(int(g["cfg_py_seed"]))
    assert pcl_prep.augment_depth_cfg(cfg, torch.zeros(F, 2, 2), seed=9, frame_keys=list(range(10, 10 + F))) == "augmented"
    assert seen["fill_holes"] is True and seen["drop_ratio"] == float(g["drop_ratio"]) and seen["seed"] == 9
    assert seen["drop"] == g["cfg_drop"].tolist()
    assert seen["noise_level"] == g["cfg_level"].tolist()          # exact: the same generator calls in the same order
    assert [lv > 0 for lv in seen["noise_level"]] == g["cfg_noise"].tolist()
    assert seen["frame_keys"] == list(range(10, 10 + F))
    # explicit values win over the defaults
    cfg2 = CfgNode(INPUT=dict(AUG_DEPTH=True, DROP_DEPTH_PROB=1.0, ADD_NOISE_DEPTH_PROB=0.0, DROP_DEPTH_RATIO=0.3))
    pcl_prep.augment_depth_cfg(cfg2, torch.zeros(3, 2, 2))
    assert seen["drop"] == [True] * 3 and seen["noise_level"] == [0.0] * 3 and seen["drop_ratio"] == 0.3


def test_augment_depth_cfg_off_returns_its_input_and_bp_depth_is_refused():
    d = torch.zeros(2, 3, 3)
    assert pcl_prep.augment_depth_cfg(CfgNode(INPUT=dict(AUG_DEPTH=False)), d) is d
    assert pcl_prep.augment_depth_cfg(CfgNode(INPUT=dict()), d) is d
    with pytest.raises(NotImplementedError):
        pcl_prep.augment_depth_cfg(CfgNode(INPUT=dict(AUG_DEPTH=True, BP_DEPTH=True)), d)


# ---- draws mode: the reference's bits -------------------------------------------------------------------------------
def _golden_batch(order=(0, 1)):
    g = R.depth_aug_golden()
    fr = [_frame(g, k) for k in order]
    t = lambda n: torch.from_numpy(np.stack([f[n] for f in fr])).to(DEV)
    draws = dict(fill=t("draw_fill"), keep=t("draw_keep"), gauss=t("draw_gauss"))
    return fr, t("raw"), draws, float(g["drop_ratio"]), [float(f["level"]) for f in fr]


@pytest.mark.gpu
def test_draws_mode_reproduces_every_golden_stage_bit_for_bit():
    fr, raw, draws, ratio, levels = _golden_batch()
    assert raw.dtype == torch.uint16
    want = lambda n: _bits(np.stack([f[n] for f in fr]))
    off = dict(fill_holes=False, drop=False, drop_ratio=ratio, noise_level=0.0)
    # the uint16 -> metres conversion alone, without and with (unused) draws
    assert np.array_equal(_bits(pcl_prep.augment_depth(raw, **off)), want("metres"))
    assert np.array_equal(_bits(pcl_prep.augment_depth(raw, draws=draws, depth_div=1000.0, **off)), want("metres"))
    steps = {"after_fill": dict(off, fill_holes=True),
             "after_drop": dict(off, fill_holes=True, drop=[True, True]),
             "after_noise": dict(off, fill_holes=True, drop=True, noise_level=levels)}
    metres = torch.from_numpy(np.stack([f["metres"] for f in fr])).to(DEV)
    for stage, kw in steps.items():
        assert np.array_equal(_bits(pcl_prep.augment_depth(raw, draws=draws, **kw)), want(stage)), stage
        assert np.array_equal(_bits(pcl_prep.augment_depth(metres, draws=draws, **kw)), want(stage)), stage + " from fp32"
    # a step alone, from the stage before it
    mid = torch.from_numpy(np.stack([f["after_fill"] for f in fr])).to(DEV)
    assert np.array_equal(_bits(pcl_prep.augment_depth(mid, draws=dict(keep=draws["keep"]), **dict(off, drop=True))),
                          want("after_drop"))
    mid = torch.from_numpy(np.stack([f["after_drop"] for f in fr])).to(DEV)
    assert np.array_equal(_bits(pcl_prep.augment_depth(mid, draws=dict(gauss=draws["gauss"]), **dict(off, noise_level=levels))),
                          want("after_noise"))


@pytest.mark.gpu
def test_draws_mode_switches_are_per_frame():
    fr, raw, draws, ratio, levels = _golden_batch()
    got = pcl_prep.augment_depth(raw, fill_holes=[True, False], drop=[True, False], drop_ratio=ratio,
                                 noise_level=[levels[0], 0.0], draws=draws)
    assert np.array_equal(_bits(got[0]), _bits(fr[0]["after_noise"]))
    assert np.array_equal(_bits(got[1]), _bits(fr[1]["metres"]))         # untouched: exactly its converted input
    fr, raw, draws, ratio, levels = _golden_batch(order=(1, 0))           # the other slot, and a ratio per frame
    got = pcl_prep.augment_depth(raw, fill_holes=[False, True], drop=[False, True], drop_ratio=[0.9, ratio],
                                 noise_level=[0.0, levels[1]], draws=draws)
    assert np.array_equal(_bits(got[1]), _bits(fr[1]["after_noise"])) and np.array_equal(_bits(got[0]), _bits(fr[0]["metres"]))


# ---- device mode: its own stream, the same distribution ---------------------------------------------------------------
H, W, NF = 120, 160, 4
N_PIX = NF * H * W          # 76 800
OFF = dict(fill_holes=False, drop=False, drop_ratio=0.2, noise_level=0.0)


@pytest.fixture(scope="module")
def maps():
    from catre_amd import synth

    holes = torch.stack([synth.make_depth_scene(H=H, W=W, seed=40 + k)["depth"] for k in range(NF)])   # ~3 % zeros
    solid = torch.where(holes == 0, torch.full_like(holes, 1.25), holes)                                # every pixel > 0
    assert (holes == 0).sum() > 1500 and (solid > 0).all() and solid.numel() == N_PIX
    return holes.to(DEV), solid.to(DEV)


@pytest.mark.gpu
def test_device_mode_drop_share(maps):
    _, solid = maps
    p = 0.2
    out = pcl_prep.augment_depth(solid, **dict(OFF, drop=True, drop_ratio=p), seed=11)
    dropped = (out == 0).double().mean().item()
    kept = out != 0
    assert torch.equal(out[kept], solid[kept])                      # a kept pixel is untouched
    bound = 5 * np.sqrt(p * (1 - p) / N_PIX)
    print(f"dropped share {dropped:.5f} (ratio {p}, bound +-{bound:.5f})")
    assert abs(dropped - p) <= bound


@pytest.mark.gpu
def test_device_mode_noise_moments_and_independence(maps):
    _, solid = maps
    level = 0.01
    kw = dict(OFF, noise_level=level)
    out = pcl_prep.augment_depth(solid, seed=11, **kw)
    noise = (out.double() - solid.double()).cpu().numpy()            # fp32 rounding of the sum: <= 6e-8, far below the bounds
    mean, std = noise.mean(), noise.std()
    print(f"noise mean {mean:.3e} (bound {5 * level / np.sqrt(N_PIX):.3e}), std {std:.6f} (bound +-{5 * level / np.sqrt(2 * N_PIX):.6f})")
    assert abs(mean) <= 5 * level / np.sqrt(N_PIX)
    assert abs(std - level) <= 5 * level / np.sqrt(2 * N_PIX)
    lag1 = np.corrcoef(noise[:, :, :-1].ravel(), noise[:, :, 1:].ravel())[0, 1]
    other = pcl_prep.augment_depth(solid, seed=11, frame_keys=[4, 5, 6, 7], **kw)        # the same frames under other keys
    cross = np.corrcoef(noise.ravel(), (other.double() - solid.double()).cpu().numpy().ravel())[0, 1]
    print(f"lag-1 row correlation {lag1:.5f}, correlation across keys {cross:.5f} (bound {5 / np.sqrt(N_PIX):.5f})")
    assert abs(lag1) <= 5 / np.sqrt(N_PIX)
    assert abs(cross) <= 5 / np.sqrt(N_PIX)
    # deterministic per (seed, keys); another seed is another stream
    assert torch.equal(out, pcl_prep.augment_depth(solid, seed=11, **kw))
    assert torch.equal(out, pcl_prep.augment_depth(solid, seed=11, frame_keys=[0, 1, 2, 3], **kw))
    assert not torch.equal(out, pcl_prep.augment_depth(solid, seed=12, **kw))


@pytest.mark.gpu
def test_device_mode_hole_fills(maps):
    holes, _ = maps
    out = pcl_prep.augment_depth(holes, **dict(OFF, fill_holes=True), seed=11)
    was = holes == 0
    assert torch.equal(out[~was], holes[~was])
    fills = out[was].double().cpu().numpy()
    h = fills.size
    pos, std = (fills > 0).mean(), fills.std()
    print(f"{h} holes: positive share {pos:.4f} (bound +-{5 * np.sqrt(0.25 / h):.4f}), std {std:.5f} (bound +-{5 * 0.1 / np.sqrt(2 * h):.5f})")
    assert abs(pos - 0.5) <= 5 * np.sqrt(0.25 / h)
    assert abs(std - 0.1) <= 5 * 0.1 / np.sqrt(2 * h)


@pytest.mark.gpu
def test_device_mode_unfilled_holes_stay_exactly_zero(maps):
    holes, _ = maps
    out = pcl_prep.augment_depth(holes, **dict(OFF, drop=True, noise_level=0.01), seed=3)
    was = holes == 0
    assert (out[was] == 0).all() and not torch.signbit(out[was]).any()
    assert (out[~was] != holes[~was]).any()


@pytest.mark.gpu
def test_device_mode_a_frame_depends_on_its_seed_and_key_only(maps):
    """A frame with key k gives the same result alone as in a batch of four, in any slot - with every step on."""
    holes, _ = maps
    kw = dict(fill_holes=True, drop_ratio=0.2)
    key, level = 77, 0.004
    alone = pcl_prep.augment_depth(holes[2:3], drop=[True], noise_level=[level], frame_keys=[key], seed=5, **kw)
    assert (alone[0] != holes[2]).float().mean() > 0.7
    for slot in range(NF):
        order = [j for j in range(NF) if j != 2]
        order.insert(slot, 2)
        keys = [100 + j for j in range(NF)]
        keys[slot] = key
        drop = [j % 2 == 0 for j in range(NF)]
        drop[slot] = True
        levels = [0.01 * (j + 1) for j in range(NF)]
        levels[slot] = level
        batch = pcl_prep.augment_depth(holes[order].contiguous(), drop=drop, noise_level=levels, frame_keys=keys, seed=5, **kw)
        assert torch.equal(batch[slot], alone[0]), slot
    # uint16 input takes the same stream
    mm = (holes[2:3] * 1000).round().to(torch.int32).cpu().numpy().astype(np.uint16)
    a = pcl_prep.augment_depth(torch.from_numpy(mm).to(DEV), drop=[True], noise_level=[level], frame_keys=[key], seed=5, **kw)
    b = pcl_prep.augment_depth(torch.from_numpy(mm.astype(np.float32) / 1000.0).to(DEV), drop=[True], noise_level=[level],
                               frame_keys=[key], seed=5, **kw)
    assert torch.equal(a, b)
