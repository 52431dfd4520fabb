"""Host-side checks of the screened STN pair kernels (k_stn3d_pair_s / k_stnkd_pair_s, csrc/catre_screen.h): the replay work
the selection leaves, from the CPU emulation of tests/test_screen_bound.py, and the kernels' compiled resources."""
import pytest
import torch

from tests.test_resources import _rows
from tests.test_screen_bound import device_eps, layers, screen_exact  # noqa: F401  (`layers` is the module's fixture)


@pytest.mark.parametrize("layer", ["stn3d", "stnkd"])
def test_replay_trips_stay_where_the_design_measured_them(layers, layer):  # noqa: F811
    """A wave replays an m-block (32 channels of one tile) in trips of two candidates per channel - the two half-wave lanes of a
    channel share its candidates - so a block costs max over its channels of ceil(candidates / 2) trips.  On
    `make_inputs(6, seed=1000)` with recipe weights: mean trips per block <= 1.10 and at most 0.5 % of the blocks above two
    trips (measured: 1.034 - 1.067 and at most 0.13 %)."""
    K = 128
    for cloud in ("obs", "prior"):
        W, a = layers[layer, cloud]
        B, _, n = a.shape
        A = a.permute(1, 0, 2).reshape(K, -1)
        s = screen_exact(W, A).float()
        eps = device_eps(W, A, K)
        lo, hi = (s - eps).view(-1, B * n // 64, 64), (s + eps).view(-1, B * n // 64, 64)
        cnt = (hi >= lo.max(dim=2, keepdim=True)[0]).sum(2)                    # [1024 channels, tiles]
        blk = cnt.view(32, 32, -1).max(dim=1)[0]                               # largest count inside a 32-channel block
        trips = torch.clamp((blk + 1) // 2, min=1).float()
        mean_cnt, mean_blk, mean_trips = cnt.float().mean().item(), blk.float().mean().item(), trips.mean().item()
        above2 = (trips > 2).float().mean().item()
        print(f"{layer} {cloud}: candidates {mean_cnt:.4f}, block maximum {mean_blk:.4f}, trips {mean_trips:.4f}, "
              f"second trip {(trips > 1).float().mean().item():.4f}, above two {above2:.5f}, most {int(trips.max())}")
        assert (cnt >= 1).all()
        assert mean_trips <= 1.10, (layer, cloud, mean_trips)
        assert above2 <= 0.005, (layer, cloud, above2)


def test_screened_stn_kernels_use_no_scratch_and_fit_one_workgroup_per_cu():
    by = {r["kernel"]: r for r in _rows()}
    for k in ("k_stn3d_pair_s", "k_stnkd_pair_s"):
        assert k in by, (k, sorted(n for n in by if "pair" in n))
        r = by[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
        assert r["vgpr"] <= 256 and r["lds"] <= 160 * 1024, (k, r)
