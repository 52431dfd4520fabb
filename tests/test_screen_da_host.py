"""`screen_da` (csrc/catre_screen.h: the fp16 screen's eps with the activations' rounding measured per tile and the weights'
rounding error split by sign) on the CPU, beside tests/test_screen_f16_host.py whose operands, scales and screen values it
reuses: an emulation of rho_p, rho_t, dws_c and eps in float32 at the device's rounding points, with |Y - S| <= eps checked
in double against the exact product and the float32 matmul, for the recipe layers of `make_inputs(6, seed=1000)` and for
rows built to sit on the bound's edges.

Measured with this emulation (recipe weights, observed / prior cloud, exact product as the running maximum, runs of 16
tiles), entries per (wave, tile), shipped eps -> `screen_da` eps:
  trunk conv4   137.6 -> 100.2 / 179.3 -> 128.1 (rounds 2.63 -> 2.00 / 3.29 -> 2.48)
  stn.conv3      79.4 ->  68.6 /  99.4 ->  82.2       fstn.conv3   84.5 -> 72.0 / 103.5 -> 84.3
(the device counters on the headline batch: 164.9 -> 117.4, profiles/screen_candidates.txt).  The worst |Y - S| / eps on
these layers is 0.14 (trunk) and 0.35 (STN layers); rho_t measures 0.48 and 0.53 - 0.55 of 2^-11, dws 0.74 and 0.76 - 0.77
of dw."""
import pytest
import torch

from tests.test_screen_bound import LAYER_K, layers  # noqa: F401  (`layers` is a fixture)
from tests.test_screen_f16_host import TP, device_eps, half, operands, pow2, scales, screen

F32 = torch.float32
F64 = torch.float64


def f32(x):
    return x.to(F32)


def rne11_err(A):
    """screen_rne11_err: x - (x with 13 of its 24 significand bits dropped, half an 11-bit ulp added first), exact in float32."""
    bits = A.to(F32).contiguous().view(torch.int32)
    hi = ((bits + 0x1000) & -8192).view(F32)
    return (A.to(F32).double() - hi.double()).to(F32)


def tile_rho(A, na):
    """rho_p [P] (screen_row_norms with `da`) and rho_t [P] (screen_tile_rho, repeated over the tile's 64 points)."""
    r = rne11_err(A)
    d = f32(r.double().pow(2).sum(0))                                              # fp32 sum of squares
    rho_p = f32(f32(f32(d.sqrt()) * f32(torch.tensor(1 + 2.0 ** -12))) / na) * f32(torch.tensor(1 + 2.0 ** -20))
    rho_t = torch.clamp(rho_p.view(-1, TP).max(dim=1)[0], max=2.0 ** -11).repeat_interleave(TP)
    return rho_p, rho_t


def weight_errors(W, sw):
    """dw [C] and dws [C] of k_screen_f16_dw (double sums, rounded up)."""
    Ws = (W.double() * pow2(torch.clamp(sw, min=-60))[:, None]).to(F32)
    uw = pow2(-torch.clamp(sw, min=-60))
    r = Ws.double() - half(Ws)
    up = f32(torch.tensor(1 + 2.0 ** -21))
    dw = f32(r.pow(2).sum(1).sqrt() * uw) * up
    sp, sn = r.clamp(min=0).pow(2).sum(1), r.clamp(max=0).pow(2).sum(1)
    dws = f32(torch.maximum(sp, sn).sqrt() * uw) * up
    return dw, dws


def device_eps_da(W, A, K, relu_input=True):
    """eps [C, P] with `screen_da` on, `every` as device_eps, rho_t [P].  relu_input = False: the layer's image may hold
    negative elements, so the sign-split dws is not used (dw instead) - rho_t is."""
    nw, na, sw, sa = scales(W, A)
    uw = f32(pow2(-torch.clamp(sw, min=-60)))
    ua = f32(pow2(-torch.clamp(sa, min=-60)))
    every = (sw < -60)[:, None] | (sa < -60)[None, :]
    dw, dws = weight_errors(W, sw)
    dwx = dws if relu_input else dw
    _, rho_t = tile_rho(A, na)
    g0 = f32(torch.tensor(2.0 ** -21 + 2 * K * 2.0 ** -23))
    rk = f32(torch.tensor((11.32 if K == 128 else 22.63) * 2.0 ** -12))
    infl = f32(1 + f32(torch.tensor(2.0 ** -22)) / g0 + 2.0 ** -18)
    gam = f32(rho_t + g0)                                                            # [P]
    inner = f32((1 + 2.0 ** -10) * dwx.double() + (rk * uw).double())                 # [C]
    e1 = f32(gam[None, :].double() * nw[:, None].double() + inner[:, None].double()) * infl          # [C, P]
    t = f32(f32(K * 2.0 ** -24 * uw)[:, None].double() * ua[None, :].double() + K * 2.0 ** -122)
    t = f32(2.0 ** -58 * nw[:, None].double() + t.double())
    e0 = f32((rk * nw)[:, None].double() * ua[None, :].double() + t.double()) * infl
    eps = f32(e1.double() * na[None, :].double() + e0.double())
    return eps, every, rho_t


def assert_bound(W, A, K, what, worst=True, relu_input=True, expect_violation=False):
    """|Y - S| <= eps for every (channel, point); returns the largest ratio."""
    assert A.shape[1] % TP == 0
    eps, every, _ = device_eps_da(W, A, K, relu_input)
    eps = eps.double()
    y = W.double() @ A.double()
    y32 = (W @ A).double()
    ratio = 0.0
    for name in ("exact",) + (("worst",) if worst else ()):
        s = screen(W, A, name == "worst")
        err = torch.maximum((y - s).abs(), (y32 - s).abs())
        assert not torch.isnan(eps).any() and (eps > 0).all(), (what, name)
        assert torch.isfinite(s[~every]).all(), (what, name)
        if (~every).any():
            ratio = max(ratio, (err / eps)[~every].max().item())
        if not expect_violation:
            bad = (err > eps) & ~every
            assert not bad.any(), f"{what} ({name}): {int(bad.sum())} outputs beyond eps, worst ratio {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("layer", ["stn3d", "stnkd", "trunk"])
def test_bound_holds_on_recipe_weights_and_synthetic_clouds(layers, layer):  # noqa: F811
    K = LAYER_K[layer]
    for cloud in ("obs", "prior"):
        W, a = layers[layer, cloud]
        assert (a >= 0).all(), "the pooled layers read post-ReLU images"
        A = a.permute(1, 0, 2).reshape(K, -1)
        r = assert_bound(W, A, K, f"{layer} {cloud}", worst=False)
        r2 = assert_bound(W[::16], A[:, :128], K, f"{layer} {cloud} subset", worst=True)
        nw, na, sw, _ = scales(W, A)
        dw, dws = weight_errors(W, sw)
        rho_p, rho_t = tile_rho(A, na)
        assert (dws <= dw).all() and (rho_t <= 2.0 ** -11).all() and (rho_t > 0).all()
        print(f"{layer} {cloud}: worst |y - S| / eps {r:.3f} (exact sum), {r2:.3f} (truncating sum, 64 x 128 subset); "
              f"rho_t / 2^-11 mean {(rho_t * 2048).mean():.3f} max {(rho_t * 2048).max():.3f} (a point's own rho_p / rho_t: mean "
              f"{(rho_p / rho_t).mean():.3f}); "
              f"dws / dw mean {(dws / dw).mean():.3f}; dw / (2^-11 nw) mean {(dw * 2048 / nw).mean():.3f}")


@pytest.mark.parametrize("K", [128, 512])
def test_operands_on_fp16_rounding_ties(K):
    """Every element of both operands on a tie of the 11-bit rounding (the full half ulp; the emulated rounding sends a tie
    away from zero, the conversion to even: the same distance).  rho_t then is the largest any tile can measure."""
    ones = torch.ones(K)
    for cw, ca in ((1 + 2.0 ** -11, 1 + 2.0 ** -11), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11), (2 - 2.0 ** -11, 2 - 2.0 ** -11),
                   (1 + 2.0 ** -11, 1.5 + 2.0 ** -11)):
        W, A = ones[None, :].repeat(4, 1) * cw, ones[:, None].repeat(1, 64) * ca
        r = assert_bound(W, A, K, f"ties {cw} {ca} K={K}")
        _, na, _, _ = scales(W, A)
        _, rho_t = tile_rho(A, na)
        # the measured ratio is the true one, 2^-11 / ca, up to the (1 + 2^-12)^2 (1 + 2^-20) inflation
        assert (rho_t >= 2.0 ** -11 / ca * (1 - 2.0 ** -20)).all() and (rho_t <= 2.0 ** -11 / ca * (1 + 2.0 ** -10)).all()
        assert r <= 1.0


@pytest.mark.parametrize("K", [128, 512])
def test_sign_split_bound_is_approached_not_exceeded(K):
    """A weight row whose rounding errors all have one sign against a constant positive activation row: Cauchy-Schwarz is
    tight on sum_k dW_k a_k, the activations sit on the 11-bit grid (rho_t = 0), so |Y - S| is dws_c na_p and eps is little
    more.  The errors are 0.4 of an 11-bit ulp on values in [0.5, 1): dws / nw >= 0.4 * 2^-11, so
    ratio >= 1 / (1 + 2^-10 + gamma0 / (0.4 * 2^-11) + 0.02) - 0.84 at K = 128, 0.60 at K = 512; 0.5 is asserted."""
    g = torch.Generator().manual_seed(11 * K)
    grid = (torch.randint(1025, 2047, (8, K), generator=g).double() * 2.0 ** -11)           # fp16-representable, (0.5, 1)
    for sign in (1.0, -1.0):
        W = (grid + sign * 0.4 * 2.0 ** -11).to(F32)
        A = torch.full((K, 64), 0.75)
        _, na, sw, _ = scales(W, A)
        dw, dws = weight_errors(W, sw)
        _, rho_t = tile_rho(A, na)
        assert (rho_t == 0).all() and torch.allclose(dw, dws, rtol=1e-6, atol=0)
        r = assert_bound(W, A, K, f"one-signed errors {sign} K={K}")
        print(f"K={K} sign {sign}: |Y - S| / eps = {r:.3f}")
        assert 0.5 < r <= 1.0, r


def test_sign_split_needs_a_non_negative_image():
    """Errors of alternating sign and activations whose signs follow them: sum_k dW_k a_k = ||dW|| ||a||, which the
    sign-split bound (0.71 of it) does not cover - an image with negative elements must keep dw, and with dw (relu_input =
    False, what a layer that is not post-ReLU gets) the bound holds.  K = 128: gamma0 is small enough to show it."""
    K = 128
    g = torch.Generator().manual_seed(5)
    grid = torch.randint(1024, 2048, (8, K), generator=g).double() * 2.0 ** -11
    alt = torch.where(torch.arange(K) % 2 == 0, 1.0, -1.0).double()
    W = (grid + alt[None, :] * 0.4 * 2.0 ** -11).to(F32)
    A = (0.75 * alt)[:, None].repeat(1, 64).to(F32)
    r_split = assert_bound(W, A, K, "alternating, sign split", expect_violation=True)
    r_dw = assert_bound(W, A, K, "alternating, dw", relu_input=False)
    print(f"negative activations: ratio {r_split:.3f} with dws (violated), {r_dw:.3f} with dw")
    assert r_split > 1.0 and r_dw <= 1.0
    # the same weights against the rectified image: covered
    assert assert_bound(W, A.clamp(min=0), K, "alternating weights, rectified image") <= 1.0


@pytest.mark.parametrize("K", [128, 512])
def test_activations_on_the_11_bit_grid_give_the_tightest_eps(K):
    g = torch.Generator().manual_seed(13 * K)
    A = (torch.randint(0, 2048, (K, 128), generator=g).float() * 2.0 ** -8)                 # <= 11 significant bits
    A[:, 64:] *= 2.0 ** -5
    W = torch.randn(24, K, generator=g)
    _, na, _, _ = scales(W, A)
    _, rho_t = tile_rho(A, na)
    assert (rho_t == 0).all()
    r = assert_bound(W, A, K, f"11-bit activations K={K}")
    eps_da, _, _ = device_eps_da(W, A, K)
    eps_old, _ = device_eps(W, A, K)
    print(f"K={K}: rho_t = 0, worst ratio {r:.3f}, eps / shipped eps {(eps_da / eps_old).mean():.3f}")
    assert (eps_da < eps_old).all()


@pytest.mark.parametrize("K", [128, 512])
def test_one_point_far_larger_than_its_tile(K):
    """One point 2^12 above the rest and elements spread over 2^-16 .. 1 inside every point: under the tile's one scale many
    elements of the small points fall below 2^-14 (fp16-subnormal or flushed) - eta and delta cover them whatever the
    emulated rounding measured for them."""
    g = torch.Generator().manual_seed(17 * K)
    mag = torch.pow(torch.tensor(2.0), -16 * torch.rand(K, 64, generator=g))
    A = (mag * (torch.rand(K, 64, generator=g) + 0.5)).to(F32)
    A[:, 9] *= 2.0 ** 12
    W = torch.randn(24, K, generator=g)
    _, _, sw, sa = scales(W, A)
    _, As = operands(W, A, sw, sa)
    sub = (As.abs() < 2.0 ** -14) & (As != 0)
    assert sub[:, :9].any() and sub.float().mean() > 0.05
    r = assert_bound(W, A, K, f"huge point K={K}")
    print(f"K={K}: {sub.float().mean():.2f} of the elements fp16-subnormal, worst ratio {r:.3f}")


def test_zero_rows_and_unscalable_tiles():
    K = 128
    g = torch.Generator().manual_seed(19)
    W = torch.randn(8, K, generator=g)
    A = torch.rand(K, 128, generator=g)
    A[:, 3] = 0                                   # a zero row measures rho_p = 0 and does not widen its tile
    _, na, _, _ = scales(W, A)
    rho_p, rho_t = tile_rho(A, na)
    assert rho_p[3] == 0 and (rho_t < 2.0 ** -11).all()
    assert_bound(W, A, K, "zero row")
    assert_bound(W, torch.zeros(K, 64), K, "zero image")
    A[:, 64:] *= 2.0 ** 80                         # unscalable tile: every point a candidate, eps not used
    _, every, _ = device_eps_da(W, A, K)
    assert not every[:, :64].any() and every[:, 64:].all()


@pytest.mark.parametrize("layer", ["trunk", "stn3d", "stnkd"])
def test_candidates_fall_against_the_shipped_bound(layers, layer):  # noqa: F811
    """Entries per (wave, tile) under a running maximum (runs of S tiles that never cross a cloud), shipped eps against the
    `screen_da` eps on the same screen values; and the candidates' maximum still is the exact one."""
    K = LAYER_K[layer]
    for cloud in ("obs", "prior"):
        W, a = layers[layer, cloud]
        B, _, n = a.shape
        T = n // TP
        A = a.permute(1, 0, 2).reshape(K, -1)
        s = screen(W, A, False)
        eps_old, _ = device_eps(W, A, K)
        eps_new, every, _ = device_eps_da(W, A, K)
        assert not every.any() and (eps_new < eps_old).all()
        yf = (W.double() @ A.double()).float()
        y = yf.view(-1, B, T, TP).max(dim=3)[0]
        for S in (1, 16):
            F = torch.full_like(y, float("-inf"))
            for t in range(T):
                if t % S:
                    F[:, :, t] = torch.maximum(F[:, :, t - 1], y[:, :, t - 1])
            means = []
            for eps in (eps_old, eps_new):
                lo = (s - eps.double()).float().view(-1, B, T, TP).max(dim=3)[0]
                hi = (s + eps.double()).float().view(-1, B, T, TP)
                L = torch.maximum(F, lo)
                keep = hi >= L[..., None]
                entries = keep.sum(3).view(4, 256, B, T).sum(1)
                means.append((entries.float().mean().item(), ((entries + 63) // 64).float().mean().item()))
                ymax = torch.maximum(F, torch.where(keep, yf.view(-1, B, T, TP), torch.tensor(float("-inf"))).max(dim=3)[0])
                assert torch.equal(ymax, torch.maximum(F, y)), (layer, cloud, S)
            (e0, r0), (e1, r1) = means
            print(f"{layer} {cloud} S={S}: entries {e0:.1f} -> {e1:.1f} ({e1 / e0:.2f}), rounds {r0:.2f} -> {r1:.2f} per (wave, tile)")
            assert e1 < e0 and r1 <= r0, (layer, cloud, S, means)


def test_switches_are_listed_outside_the_form_word():
    from catre_amd import hip

    assert hip.FORM_IDS["screen_da"] == 14 and hip.FORM_IDS["screen_da_stn"] == 15
    assert "screen_da" not in hip.SWITCH_BITS and "screen_da_stn" not in hip.SWITCH_BITS
    assert len(set(hip.FORM_IDS.values())) == len(hip.FORM_IDS)


def test_no_kernel_was_added_and_the_fp16_screen_kernels_keep_their_shape():
    from tests.test_resources import _rows

    names = {r["kernel"].split("(")[0].strip() for r in _rows()}
    assert not [k for k in names if k.startswith(("k_trunk4s", "k_stn3d_pair_s", "k_stnkd_pair_s")) and "da" in k.split("_")[-1]]
    for r in _rows():
        k = r["kernel"].split("(")[0].strip()
        if k in ("k_trunk4sr16e", "k_trunk4sp16e", "k_trunk4sp16", "k_stn3d_pair_sr16e", "k_stnkd_pair_sr16e", "k_stn3d_pair_sp16e",
                 "k_stnkd_pair_sp16e", "k_stn3d_pair_sp16", "k_stnkd_pair_sp16", "k_screen_f16_dw"):
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["vgpr"] <= 256, r
