"""Host-side checks of the pooled replay (kernel-form switch `screen_pool`, csrc/catre_screen.h): how many rounds of 64 list
entries a wave replays per tile on the recipe weights and synthetic clouds (the CPU emulation of tests/test_screen_bound.py),
the resource rows of the pooled kernels, and the switch itself.

A wave owns 256 consecutive channels of a tile; its list holds every candidate of these channels, at least one per channel,
so a (wave, tile) unit replays ceil(entries / 64) rounds (its list of 512 entries is never full on these clouds).  Measured
with this emulation when the form was designed: trunk 5.67 / 5.87 rounds (observed / prior cloud), at most 7; both STN
layers 5.00, at most 5 - against 14.9 / 15.8 and 8.3 - 8.5 chain-trips of the per-channel replay."""
import os

import pytest

from tests.test_screen_bound import LAYER_K, device_eps, layers, screen_exact  # noqa: F401  (`layers` is a fixture)

ROUNDS = {"trunk": (6.2, 8), "stn3d": (5.2, None), "stnkd": (5.2, None)}   # mean at most, unit at most
POOLED = ("k_trunk4sp", "k_stn3d_pair_sp", "k_stnkd_pair_sp")


@pytest.mark.parametrize("layer", ["trunk", "stn3d", "stnkd"])
def test_rounds_per_wave_and_tile(layers, layer):  # noqa: F811
    K = LAYER_K[layer]
    mean_max, unit_max = ROUNDS[layer]
    for cloud in ("obs", "prior"):
        W, a = layers[layer, cloud]
        B, _, n = a.shape
        A = a.permute(1, 0, 2).reshape(K, -1)
        s = screen_exact(W, A).float()
        eps = device_eps(W, A, K)
        lo, hi = (s - eps).view(-1, B * n // 64, 64), (s + eps).view(-1, B * n // 64, 64)
        cnt = (hi >= lo.max(dim=2, keepdim=True)[0]).sum(2)                # [1024 channels, tiles]
        assert (cnt >= 1).all(), (layer, cloud)                            # every channel has an entry
        entries = cnt.view(4, 256, -1).sum(1)                              # [wave, tile]
        rounds = (entries + 63) // 64
        mean, worst = rounds.float().mean().item(), rounds.max().item()
        print(f"{layer} {cloud}: {entries.float().mean().item():.1f} entries, {mean:.2f} rounds per (wave, tile), max {worst}")
        assert mean <= mean_max, (layer, cloud, mean)
        if unit_max is not None:
            assert worst <= unit_max, (layer, cloud, worst)
        assert entries.max().item() <= 512, (layer, cloud)                 # one batch: the list never fills up here


def test_pooled_kernels_fit_the_one_wave_per_simd_shape():
    from tests.test_resources import _rows

    by = {r["kernel"]: r for r in _rows()}
    for k in POOLED:
        if k not in by:      # a pooled form that lost its A/B is deleted, not kept: then its row is gone too
            assert k != "k_trunk4sp", "the trunk's pooled kernel is missing from the build"
            continue
        r = by[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
        assert r["vgpr"] <= 256 and r["lds"] <= 160 * 1024, (k, r)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "r06_resource_usage.txt")).read()
    assert "k_trunk4sp" in text


def test_switch_is_listed():
    from catre_amd import hip

    assert hip.FORM_IDS["screen_pool"] == 7
    assert len(set(hip.FORM_IDS.values())) == len(hip.FORM_IDS)
