"""The fp16 screen (kernel-form switch `screen_f16`, ScreenPipeF16 / ScreenBoundF16 in csrc/catre_screen.h) on the CPU: a
torch emulation of the scaled fp16 product and of eps as the device computes it - row scale 2^sw from nw, one tile scale
2^sa from the largest row norm of the tile, the weights' measured rounding error dw, gamma_K = 2^-11 + 2^-21 + 2 K 2^-23,
the delta term, the inflation - with |y - S| <= eps checked in double against the exact product and the float32 matmul.

Two emulations of the accumulation, as in tests/test_screen_bound.py: `exact` (the one product summed exactly) and `worst`
(k by k, every fp32 add truncated, every fp16-subnormal operand flushed to zero - the matrix pipe may do that).

Entries per (wave, tile) with the exact product as the running maximum (recipe weights, `make_inputs(6, seed=1000)`, runs
that never cross a cloud), measured with this emulation, observed / prior cloud, entries (rounds of 64):
  trunk conv4   S = 1: 559.1 (9.25) / 589.4 (9.70)   S = 4: 297.1 / 334.7   S = 8: 206.6 / 241.9   S = 16: 137.6 (2.63) / 179.3 (3.29)
  stn.conv3     S = 1: 356.4 (6.09) / 371.6 (6.39)   S = 4: 186.1 / 207.1   S = 8: 123.3 / 143.9   S = 16:  79.4 (1.74) /  99.4 (2.02)
  fstn.conv3    S = 1: 375.9 (6.43) / 392.2 (6.66)   S = 4: 197.2 / 216.3   S = 8: 132.9 / 151.0   S = 16:  84.5 (1.83) / 103.5 (2.09)
(split-bf16 screen, tests/test_screen_run_host.py: 74 - 89 and 55 - 60 at S = 16.)  The largest unit is 883 entries for the trunk
(3 % of the units at S = 16, 54 % at S = 1 exceed the 512-entry list and take a second batch of `screen_pool_store`), 509 and
577 for the STN layers.  The worst |y - S| / eps seen on these layers is 0.09 (trunk) and 0.22 (STN layers).
The device's rule gives eps 2^-11 where the weights' worst case would be and uses the measured rounding error of the
packed weights instead; with the worst case for both operands (2^-10) the headline batch replays 212.8 entries per (wave,
tile) in the trunk instead of what profiles/screen_candidates.txt now reports."""
import os

import pytest
import torch

from tests.test_screen_bound import LAYER_K, _trunc32, layers  # noqa: F401  (`layers` is a fixture)

TP = 64
F32 = torch.float32


def gamma(K):
    return 2.0 ** -11 + 2.0 ** -21 + 2 * K * 2.0 ** -23


def f16_exp(n):
    """screen_f16_exp: 14 - (biased exponent - 127) of the float32 n, at most 60 (int64 tensor)."""
    e = ((n.to(F32).contiguous().view(torch.int32).to(torch.int64) >> 23) & 0xff) - 127
    return torch.clamp(14 - e, max=60)


def pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())


def half(t):
    """float32 -> fp16 (RNE) -> float64"""
    return t.to(F32).to(torch.float16).double()


def scales(W, A):
    """nw [C], na [P], sw [C], sa [P] (one value per tile of 64 columns), as the device computes them."""
    nw = (W.double().pow(2).sum(1).sqrt().to(F32) * (1 + 2.0 ** -21)).to(F32)          # k_screen_wnorm
    na = (A.to(F32).pow(2).sum(0).sqrt() * (1 + 2.0 ** -12) + 2.0 ** -58).to(F32)       # screen_row_norms
    sw = f16_exp(nw)
    sa = f16_exp(na.view(-1, TP).max(dim=1)[0]).repeat_interleave(TP)                   # screen_tile_scale
    return nw, na, sw, sa


def operands(W, A, sw, sa):
    """The scaled fp32 operands the device rounds to fp16: w' [C, K], a' [K, P] (float32; clamped scales as the device's)."""
    Ws = (W.double() * pow2(torch.clamp(sw, min=-60))[:, None]).to(F32)
    As = (A.double() * pow2(torch.clamp(sa, min=-60))[None, :]).to(F32)
    return Ws, As


def device_eps(W, A, K):
    """eps [C, P] of catre_screen.h's fp16 screen and `every` [C, P]: channels / tiles that cannot be scaled (every point is
    a candidate there, S is not used).  float64 arithmetic rounded to float32 at the device's rounding points."""
    nw, na, sw, sa = scales(W, A)
    Ws, _ = operands(W, A, sw, sa)
    uw = pow2(-torch.clamp(sw, min=-60)).to(F32)
    dw = ((Ws.double() - half(Ws)).pow(2).sum(1).sqrt() * uw.double()).to(F32) * (1 + 2.0 ** -21)  # k_screen_f16_dw
    ua = pow2(-torch.clamp(sa, min=-60)).to(F32)
    every = (sw < -60)[:, None] | (sa < -60)[None, :]
    g = torch.tensor(gamma(K), dtype=F32)
    rk = torch.tensor((11.32 if K == 128 else 22.63) * 2.0 ** -12, dtype=F32)
    infl = (1 + torch.tensor(2.0 ** -22, dtype=F32) / g + 2.0 ** -19).to(F32)
    e1 = ((g * nw).double() + ((1 + 2.0 ** -10) * dw).double() + (rk * uw).double()).to(F32) * infl       # [C]
    e0 = ((rk * nw)[:, None].double() * ua[None, :].double() + (K * 2.0 ** -24 * uw)[:, None].double() * ua[None, :].double()
          + K * 2.0 ** -122).to(F32) * infl                                                                  # [C, P]
    eps = (e1[:, None].double() * na[None, :].double() + e0.double()).to(F32)
    return eps, every


def screen(W, A, worst):
    """S [C, P] in float64 (unscaled): the fp16 product of the scaled operands, summed exactly or k by k with truncating
    fp32 adds and fp16-subnormal operands flushed."""
    _, _, sw, sa = scales(W, A)
    Ws, As = operands(W, A, sw, sa)
    wh, ah = half(Ws), half(As)
    if worst:
        flush = lambda t: torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)
        wh, ah = flush(wh), flush(ah)
        acc = torch.zeros(W.shape[0], A.shape[1], dtype=torch.float64)
        for k in range(W.shape[1]):
            acc = _trunc32(acc + wh[:, k, None] * ah[None, k, :])
    else:
        acc = wh @ ah
    return acc * pow2(-torch.clamp(sw, min=-60))[:, None] * pow2(-torch.clamp(sa, min=-60))[None, :]


def assert_bound(W, A, K, what, worst=True):
    assert A.shape[1] % TP == 0
    eps, every = device_eps(W, A, K)
    eps = eps.double()
    y = W.double() @ A.double()
    y32 = (W @ A).double()
    ratio = 0.0
    for name in ("exact",) + (("worst",) if worst else ()):
        s = screen(W, A, name == "worst")
        err = torch.maximum((y - s).abs(), (y32 - s).abs())
        assert not torch.isnan(eps).any() and (eps > 0).all(), (what, name)
        bad = (err > eps) & ~every
        assert torch.isfinite(s[~every]).all(), (what, name)
        assert not bad.any(), f"{what} ({name}): {int(bad.sum())} outputs beyond eps, worst ratio {(err / eps)[~every].max():.3f}"
        if (~every).any():
            ratio = max(ratio, (err / eps)[~every].max().item())
    return ratio


@pytest.mark.parametrize("layer", ["stn3d", "stnkd", "trunk"])
def test_bound_holds_on_recipe_weights_and_synthetic_clouds(layers, layer):  # noqa: F811
    K = LAYER_K[layer]
    for cloud in ("obs", "prior"):
        W, a = layers[layer, cloud]
        A = a.permute(1, 0, 2).reshape(K, -1)                     # [K, 6 * 1024 points], tiles of 64 consecutive points
        r = assert_bound(W, A, K, f"{layer} {cloud}", worst=False)
        r2 = assert_bound(W[::16], A[:, :128], K, f"{layer} {cloud} subset", worst=True)   # 64 channels x 2 tiles, k by k
        print(f"{layer} {cloud}: worst |y - S| / eps {r:.3f} (exact sum), {r2:.3f} (truncating sum, 64 x 128 subset)")


@pytest.mark.parametrize("K", [128, 512])
def test_bound_holds_where_cauchy_schwarz_is_tight(K):
    """All-positive, parallel rows: sum |w_k a_k| = ||w|| ||a||, truncation errors all point one way; constants that sit on
    an fp16 rounding tie (1 + 2^-11 rounds to 1: the full half ulp, for every element of both operands)."""
    g = torch.Generator().manual_seed(K)
    base = torch.rand(K, generator=g) + 0.5
    W = base[None, :] * (torch.rand(32, 1, generator=g) + 0.5)
    a = base[:, None] * (torch.rand(1, 64, generator=g) + 0.5)
    assert_bound(W, a, K, f"parallel K={K}")
    ones = torch.ones(K)
    for cw, ca in ((1.0078125, 1.00390625), (1 + 2.0 ** -11, 1 + 2.0 ** -11), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11),
                   (2 - 2.0 ** -11, 2 - 2.0 ** -11)):
        r = assert_bound(ones[None, :].repeat(4, 1) * cw, ones[:, None].repeat(1, 64) * ca, K, f"constant {cw} {ca} K={K}")
        assert r <= 1.0


@pytest.mark.parametrize("K", [128, 512])
def test_bound_holds_over_the_exponent_range_with_zeros_and_denormals(K):
    """Rows whose elements span far more than the fp16 range: what the scale pushes below 2^-14 is rounded to a subnormal or
    flushed, and delta covers it; one tile holds points of very different size (one scale per tile)."""
    g = torch.Generator().manual_seed(7 * K)

    def draw(n, m, lo, hi):
        mant = (torch.rand(n, m, generator=g) + 1) * torch.where(torch.rand(n, m, generator=g) < 0.5, -1.0, 1.0)
        ex = torch.randint(lo, hi + 1, (n, m), generator=g)
        v = (mant.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), ex.double())).float()
        return torch.where(torch.rand(n, m, generator=g) < 0.2, torch.zeros_like(v), v)

    for lo, hi in ((-60, 60), (-60, -30), (30, 60), (-149, -120), (-140, 20), (-20, 0), (-30, 10)):
        W, a = draw(24, K, lo, hi), draw(K, 64, lo, hi)
        if not torch.isfinite((W.double().abs() @ a.double().abs()).float()).all():
            continue   # (products past the float32 range are outside the contract: Inf in the dense form too)
        assert_bound(W, a, K, f"exponents {lo}..{hi} K={K}")
    # columns of one tile 2^40 apart, rows 2^40 apart
    a = draw(K, 64, -4, 4) * torch.pow(torch.tensor(2.0), torch.randint(-40, 1, (1, 64), generator=g).float())
    W = draw(24, K, -4, 4) * torch.pow(torch.tensor(2.0), torch.randint(-20, 21, (24, 1), generator=g).float())
    assert_bound(W, a, K, f"points of one tile 2^40 apart K={K}")
    Z = torch.zeros(8, K)
    assert_bound(Z, draw(K, 64, -10, 10), K, "zero weights")
    assert_bound(draw(8, K, -10, 10), torch.zeros(K, 64), K, "zero activations")


def test_operands_never_overflow_and_unscalable_ones_are_flagged():
    K = 128
    g = torch.Generator().manual_seed(3)
    for e in (-100, -46, 0, 15, 60, 70):      # (row norms: fp32 sums of squares, inf from 2^64 on - such a tile is unscalable)
        W = (torch.rand(8, K, generator=g) - 0.5) * 2.0 ** e
        A = (torch.rand(K, 64, generator=g) - 0.5) * 2.0 ** min(e, 58)
        nw, na, sw, sa = scales(W, A)
        Ws, As = operands(W, A, sw, sa)
        eps, every = device_eps(W, A, K)
        assert not every.any(), e
        assert torch.isfinite(half(Ws)).all() and torch.isfinite(half(As)).all(), e
        assert half(Ws).abs().max() <= 2.0 ** 15 and half(As).abs().max() <= 2.0 ** 15, e
        if -46 <= e <= 60:          # not clamped: the largest element sits near the top of the range
            assert half(Ws).abs().amax(dim=1).min() >= 2.0 ** 14 / K ** 0.5 / 2 and half(As).abs().max() >= 2.0 ** 14 / K ** 0.5 / 2
    W = (torch.rand(8, K, generator=g) - 0.5) * 2.0 ** 80
    A = torch.rand(K, 128, generator=g)
    A[:, 64:] *= 2.0 ** 80
    _, every = device_eps(W, A, K)
    assert every.all()
    _, every = device_eps(W * 2.0 ** -80, A, K)
    assert not every[:, :64].any() and every[:, 64:].all()


# mean entries per (wave, tile) at most: a modest margin over what this emulation measures (module docstring)
MEANS = {"trunk": {1: 650, 4: 370, 8: 265, 16: 200}, "stn3d": {1: 410, 4: 230, 8: 160, 16: 110},
         "stnkd": {1: 430, 4: 240, 8: 166, 16: 114}}


@pytest.mark.parametrize("layer", ["trunk", "stn3d", "stnkd"])
def test_entries_per_wave_and_tile_under_a_running_maximum(layers, layer):  # noqa: F811
    K = LAYER_K[layer]
    for cloud in ("obs", "prior"):
        W, a = layers[layer, cloud]
        B, _, n = a.shape
        T = n // TP
        A = a.permute(1, 0, 2).reshape(K, -1)
        s = screen(W, A, False)
        eps, every = device_eps(W, A, K)
        assert not every.any()
        yf = (W.double() @ A.double()).float()
        y = yf.view(-1, B, T, TP).max(dim=3)[0]                               # exact tile maxima [C, B, T]
        lo = (s - eps.double()).float().view(-1, B, T, TP).max(dim=3)[0]      # fl(S - eps), fl(S + eps) as the device's fma
        hi = (s + eps.double()).float().view(-1, B, T, TP)
        for S, mean_max in MEANS[layer].items():
            F = torch.full_like(y, float("-inf"))
            for t in range(T):
                if t % S:
                    F[:, :, t] = torch.maximum(F[:, :, t - 1], y[:, :, t - 1])
            L = torch.maximum(F, lo)
            cnt = (hi >= L[..., None]).sum(3)                                  # [1024 channels, B, T]
            assert (cnt[:, :, ::S] >= 1).all(), (layer, cloud, S)              # the first tile of a run keeps every channel
            entries = cnt.view(4, 256, B, T).sum(1)                            # [wave, cloud, tile]
            mean, worst = entries.float().mean().item(), entries.max().item()
            rounds = ((entries + 63) // 64).float().mean().item()
            print(f"{layer} {cloud} S={S}: {mean:.1f} entries, {rounds:.2f} rounds per (wave, tile), max {worst}, units above "
                  f"the 512-entry list {(entries > 512).float().mean().item():.4f}")
            assert mean <= mean_max, (layer, cloud, S, mean)
            # what the batch loop of screen_pool_store handles: whole channels of at most 64 entries, up to 32 batches
            assert cnt.max().item() <= TP and worst <= 32 * 512, (layer, cloud, S, worst)
            assert worst <= 1024, (layer, cloud, S, worst)                     # measured: never more than a second batch
            # exactness: the candidates' maximum joined with F is the maximum of the run so far
            ymax = torch.maximum(F, torch.where(hi >= L[..., None], yf.view(-1, B, T, TP),
                                                torch.tensor(float("-inf"))).max(dim=3)[0])
            assert torch.equal(ymax, torch.maximum(F, y)), (layer, cloud, S)


def test_switch_and_symbols_are_listed():
    from catre_amd import hip

    assert hip.FORM_IDS["screen_f16"] == 9
    assert len(set(hip.FORM_IDS.values())) == len(hip.FORM_IDS)
    assert "catre_form_switch" in hip.EXPORTED_SYMBOLS and "catre_trunk_screen_probe" in hip.EXPORTED_SYMBOLS


def test_fp16_kernels_fit_the_one_wave_per_simd_shape():
    from tests.test_resources import _rows

    by = {r["kernel"]: r for r in _rows()}
    want = ("k_trunk4sp16", "k_trunk4sr16", "k_stn3d_pair_sp16", "k_stn3d_pair_sr16", "k_stnkd_pair_sp16", "k_stnkd_pair_sr16",
            "k_pack_screen_f16", "k_screen_f16_dw")
    table = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                              "r06_resource_usage.txt")).read()
    for name in want:
        rows = [r for k, r in by.items() if k.split("(")[0].strip() == name]
        assert rows, f"{name} is missing from the build"
        for r in rows:
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
            assert r["vgpr"] <= 256 and r["lds"] <= 160 * 1024, (name, r)
        assert name in table, name
