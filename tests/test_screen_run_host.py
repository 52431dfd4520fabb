"""Host-side checks of the run form of the screened max-pool (kernel-form switch `screen_run`, k_trunk4sr in
csrc/catre_screen.h): list entries per (wave, tile) when a workgroup carries the exact running maximum over S consecutive
tiles of a cloud (the CPU emulation of tests/test_screen_bound.py), the run -> tile mapping and the host rule for S, the
switch, and the resource row of the new kernel.

Emulation: recipe weights, `make_inputs(6, seed=1000)`, the exact product rounded to fp32 as the running maximum, runs that
never cross a cloud.  Measured with it when the form was designed (entries per (wave, tile), observed / prior cloud):
  trunk conv4   S = 1: 337.3 / 348.8   S = 4: 175.0 / 191.6   S = 8: 117.3 / 130.9   S = 16: 74.2 / 89.1
  stn.conv3     S = 1: 265.0 / 266.9   S = 4: 135.8 / 142.6   S = 8:  88.2 /  94.2   S = 16: 55.3 / 60.0
  fstn.conv3    S = 1: 266.7 / 268.4   S = 4: 136.8 / 141.8   S = 8:  90.2 /  93.9   S = 16: 55.8 / 58.9
The largest unit keeps its size (375 - 418): the first tile of a run has no running maximum."""
import os

import pytest
import torch

from tests.test_screen_bound import LAYER_K, device_eps, layers, screen_exact  # noqa: F401  (`layers` is a fixture)

# mean entries per (wave, tile) at most, for S = 4 / 8 / 16
MEANS = {"trunk": {4: 200, 8: 140, 16: 95}, "stn3d": {4: 150, 8: 100, 16: 65}, "stnkd": {4: 150, 8: 100, 16: 65}}
TP = 64


@pytest.mark.parametrize("layer", ["trunk", "stn3d", "stnkd"])
def test_entries_per_wave_and_tile_under_a_running_maximum(layers, layer):  # noqa: F811
    K = LAYER_K[layer]
    for cloud in ("obs", "prior"):
        W, a = layers[layer, cloud]
        B, _, n = a.shape
        T = n // TP                                                        # tiles of a cloud
        A = a.permute(1, 0, 2).reshape(K, -1)
        s = screen_exact(W, A).float()
        eps = device_eps(W, A, K)
        y = (W.double() @ A.double()).float().view(-1, B, T, TP).max(dim=3)[0]          # exact tile maxima [C, B, T]
        lo = (s - eps).view(-1, B, T, TP).max(dim=3)[0]
        hi = (s + eps).view(-1, B, T, TP)
        for S, mean_max in MEANS[layer].items():
            F = torch.full_like(y, float("-inf"))                          # running maximum in front of tile t of its run
            for t in range(T):
                if t % S:
                    F[:, :, t] = torch.maximum(F[:, :, t - 1], y[:, :, t - 1])
            L = torch.maximum(F, lo)
            cnt = (hi >= L[..., None]).sum(3)                              # [1024 channels, B, T]
            first = cnt[:, :, ::S]
            assert (first >= 1).all(), (layer, cloud, S)                   # the first tile of a run keeps every channel
            entries = cnt.view(4, 256, B, T).sum(1)                        # [wave, cloud, tile]
            mean, worst = entries.float().mean().item(), entries.max().item()
            empty = (entries == 0).float().mean().item()
            print(f"{layer} {cloud} S={S}: {mean:.1f} entries, {((entries + 63) // 64).float().mean().item():.2f} rounds per "
                  f"(wave, tile), max {worst}, empty units {empty:.4f}, channels without a candidate "
                  f"{(cnt == 0).float().mean().item():.3f}")
            assert mean <= mean_max, (layer, cloud, S, mean)
            assert worst <= 512, (layer, cloud, S, worst)
            # exactness: the candidates' maximum joined with F is the maximum of the run so far
            ymax = torch.maximum(F, torch.where(hi >= L[..., None], (W.double() @ A.double()).float().view(-1, B, T, TP),
                                                torch.tensor(float("-inf"))).max(dim=3)[0])
            want = torch.maximum(F, y)
            assert torch.equal(ymax, want), (layer, cloud, S)


def _runs_reference(B, N, M, S):
    """[(first tile, tile count)] of every run, observed clouds first: the three-line reference."""
    TN, TM = (N + TP - 1) // TP, (M + TP - 1) // TP
    obs = [(b * TN + k, min(S, TN - k)) for b in range(B) for k in range(0, TN, S)]
    return obs + [(B * TN + b * TM + k, min(S, TM - k)) for b in range(B) for k in range(0, TM, S)]


def _run_info(rid, B, N, M, S):
    """run_info of catre_screen.h, mirrored line by line."""
    TN, TM = (N + TP - 1) // TP, (M + TP - 1) // TP
    RN, RM = (TN + S - 1) // S, (TM + S - 1) // S
    if rid < B * RN:
        k = rid % RN
        return (rid // RN) * TN + k * S, min(S, TN - k * S)
    r = rid - B * RN
    k = r % RM
    return B * TN + (r // RM) * TM + k * S, min(S, TM - k * S)


@pytest.mark.parametrize("N,M", [(1024, 1024), (960, 448), (100, 70)])
@pytest.mark.parametrize("S", [1, 3, 4, 16])
def test_run_to_tile_mapping(N, M, S):
    B = 5
    TN, TM = (N + TP - 1) // TP, (M + TP - 1) // TP
    want = _runs_reference(B, N, M, S)
    assert len(want) == B * ((TN + S - 1) // S + (TM + S - 1) // S)        # the grid launch_trunk computes
    got = [_run_info(r, B, N, M, S) for r in range(len(want))]
    assert got == want
    tiles = [t for t0, nt in got for t in range(t0, t0 + nt)]
    assert tiles == list(range(B * (TN + TM)))                             # every tile once, in order
    for t0, nt in got:                                                     # no run crosses a cloud
        assert 1 <= nt <= S
        cloud = lambda t: t // TN if t < B * TN else B + (t - B * TN) // TM
        assert cloud(t0) == cloud(t0 + nt - 1)


def _pair_run_info(rid, B, N, M, SP):
    """pair_run_info of catre_screen.h (the STN pair kernels' runs, in pair_info32's numbering), mirrored line by line."""
    PN, PM = ((N + TP - 1) // TP + 1) // 2, ((M + TP - 1) // TP + 1) // 2
    RN, RM = (PN + SP - 1) // SP, (PM + SP - 1) // SP
    if rid < B * RN:
        k = rid % RN
        return (rid // RN) * PN + k * SP, min(SP, PN - k * SP)
    r = rid - B * RN
    k = r % RM
    return B * PN + (r // RM) * PM + k * SP, min(SP, PM - k * SP)


@pytest.mark.parametrize("N,M", [(1024, 1024), (960, 448), (100, 70)])
@pytest.mark.parametrize("S", [2, 3, 4, 16])
def test_run_to_pair_mapping_of_the_stn_kernels(N, M, S):
    B, SP = 5, S // 2                                                      # what launch_stn3d / launch_stnkd pass
    PN, PM = ((N + TP - 1) // TP + 1) // 2, ((M + TP - 1) // TP + 1) // 2
    want = [(b * PN + k, min(SP, PN - k)) for b in range(B) for k in range(0, PN, SP)]
    want += [(B * PN + b * PM + k, min(SP, PM - k)) for b in range(B) for k in range(0, PM, SP)]
    assert len(want) == B * ((PN + SP - 1) // SP + (PM + SP - 1) // SP)    # stn_pair_runs
    got = [_pair_run_info(r, B, N, M, SP) for r in range(len(want))]
    assert got == want
    assert [p for p0, n in got for p in range(p0, p0 + n)] == list(range(B * (PN + PM)))


def _rule(B, N, M, cus):
    """screen_run_rule of catre_kernels.hip: the largest S <= 16 whose ceil(runs / cus) * S tile slots do not exceed the
    one-tile grid's ceil(tiles / cus), else 1."""
    TN, TM = (N + TP - 1) // TP, (M + TP - 1) // TP
    slots1 = -(-B * (TN + TM) // cus)
    for S in range(16, 1, -1):
        if -(-B * (-(-TN // S) + -(-TM // S)) // cus) * S <= slots1:
            return S
    return 1


def test_host_rule_for_the_run_length():
    from catre_amd import hip

    assert hip.screen_run_rule(256, 1024, 1024, 256) == 16      # 512 runs: two full rounds
    assert hip.screen_run_rule(128, 1024, 1024, 256) == 16      # 256 runs: one full round
    assert hip.screen_run_rule(64, 1024, 1024, 256) == 8        # 16 would leave half the chip idle
    assert hip.screen_run_rule(200, 1024, 1024, 256) == 1       # no S fills its last round: the one-tile kernel
    for B in (1, 9, 33, 64, 100, 200, 256, 300):
        for N, M in ((1024, 1024), (960, 448), (100, 70), (2048, 1024)):
            for cus in (256, 304, 64):
                S = hip.screen_run_rule(B, N, M, cus)
                assert S == _rule(B, N, M, cus), (B, N, M, cus, S)
                assert 1 <= S <= 16
    assert hip.screen_run_rule(0, 64, 64, 256) == -1 and hip.screen_run_rule(4, 64, 64, 0) == -1


def test_switch_is_listed():
    from catre_amd import hip

    assert hip.FORM_IDS["screen_run"] == 8
    assert len(set(hip.FORM_IDS.values())) == len(hip.FORM_IDS)
    assert "catre_screen_run_len" in hip.EXPORTED_SYMBOLS and "catre_screen_run_rule" in hip.EXPORTED_SYMBOLS


def test_run_kernel_fits_the_one_wave_per_simd_shape():
    from tests.test_resources import _rows

    by = {r["kernel"]: r for r in _rows()}
    new = [k for k in by if k.startswith(("k_trunk4sr", "k_stn3d_pair_sr", "k_stnkd_pair_sr"))]
    assert any(k.startswith("k_trunk4sr") for k in new), "the trunk's run kernel is missing from the build"
    for k in new:
        r = by[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["vgpr"] <= 256 and r["lds"] <= 160 * 1024, (k, r)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "k_trunk4sr" in open(os.path.join(root, "profiles", "r06_resource_usage.txt")).read()
