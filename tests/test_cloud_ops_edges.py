"""The small training ops on point-cloud rows at their edges, against the fp64 references of tests/cloud_ops_ref.py:
per-cloud transforms (k_cloud_matmul<3>, <64>, k_cloud_matmul64, the two bwd_t kernels), the plain max-pool (k_maxpool_fwd,
k_maxpool_scatter), the per-cloud bias (k_rowbias_add, k_rowbias_bwd), conv_p's weighted point sum (k_wsum_fwd, k_wsum_bwd,
k_wsum_bias, k_reduce_splits_wide) and the column sums (k_colsum, k_reduce_splits).

Everything runs through the `train_ops` wrappers, forward and `backward()`; the C ABI is called directly only where no
wrapper reaches: odd leading dimensions, `catre_op_wsum_bwd_n`, `accumulate = 1`.

Two kinds of input per case:
  exact    integers in [-8, 8] as fp32: every product and partial sum is an exact fp32 number (test_cloud_ops_host.py asserts
           the headroom), so the device result must EQUAL the reference whatever the order of the additions - a dropped,
           duplicated or neighbouring cloud's row, a wrong tile limit or a transposed index cannot hide in a tolerance;
  rounded  N(0, 1) against fp64 within `cloud_ops_ref.bound`: 2 n 2^-24 sum|terms| for a sum of n terms.  Derived, not
           measured; each case prints `RATIO <what> <max err / bound>`.  It is there to notice a precision change.
The max-pool (values, rows, scatter) and `rowbias_add` (one fp32 add) are exact for either kind.

Not asserted: a NaN inside a pooled column.  k_maxpool_fwd skips it (`v > m` is false) where torch.max propagates it; the
fused encoder pools behave the same way, so no case here holds a NaN.
"""
import numpy as np
import pytest
import torch

from tests import cloud_ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("exact", "rounded")
SENTINEL = 12345.0      # fills what a kernel must not read (columns past kd) or must not write (padding of an odd ld)


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _equal(got, want, what):
    """Bit for bit (as values: the fp32 result converted to fp64 equals the fp64 reference; +-inf included)."""
    np.testing.assert_array_equal(_np(got).astype(np.float64), np.asarray(want, dtype=np.float64), err_msg=what)


def _within(got, want, bnd, what):
    err = np.abs(_np(got).astype(np.float64) - want)
    bnd = np.broadcast_to(np.asarray(bnd, dtype=np.float64), err.shape)
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    print(f"RATIO {what} {ratio:.4f}")
    assert (err <= bnd).all(), f"{what}: max err / bound = {ratio:.3f}"      # (a zero bound asks for a zero error)


def _check(kind, got, want, n, abs_sum, what):
    if kind == "exact":
        _equal(got, want, what)
    else:
        _within(got, want, R.bound(n, abs_sum), what)


def _stream():
    from catre_amd import hip
    return hip.stream_ptr(torch.device(DEV))


# ------------------------------------------------------------------------------------------------- per-cloud transforms
def _cloud_matmul_case(kind, shape, kd, xcols, oc, tag):
    """x [R, xcols] (columns past kd hold a sentinel: never read), T [C, kd, kd], dy [R, oc] (columns past kd are live data
    the transposed product must ignore) -> forward, dx, dT through train_ops.cloud_matmul, checked against the reference."""
    from catre_amd import train_ops as T

    B, N, M = shape
    rows, C = B * (N + M), R.n_clouds(B, M)
    xn = R.operand(kind, (rows, xcols), "x", shape, kd, tag)
    xn[:, kd:] = SENTINEL
    Tn = R.operand(kind, (C, kd, kd), "T", shape, kd, tag)
    dyn = R.operand(kind, (rows, oc), "dy", shape, kd, tag)
    x, Tm = _dev(xn, True), _dev(Tn, True)
    y = T.cloud_matmul(x, Tm, B, N, M, out_cols=oc)
    assert tuple(y.shape) == (rows, oc)
    y.backward(_dev(dyn))
    what = f"cloud_matmul[{kind} kd={kd} {B}x{N}x{M} {tag}]"
    n_c = R.cloud_rows(B, N, M).reshape(C, 1, 1)
    ax, aT, ady = np.abs(xn), np.abs(Tn), np.abs(dyn)
    asum = (lambda f, *a: f(*a)) if kind == "rounded" else (lambda f, *a: None)     # the bound's sum of |terms|: rounded only
    _check(kind, y[:, :kd], R.cloud_matmul(xn, Tn, B, N, M), kd, asum(R.cloud_matmul, ax, aT, B, N, M), what + " y")
    _check(kind, x.grad[:, :kd], R.cloud_matmul_dx(dyn, Tn, B, N, M), kd, asum(R.cloud_matmul_dx, ady, aT, B, N, M), what + " dx")
    _check(kind, Tm.grad, R.cloud_matmul_dT(xn, dyn, B, N, M, kd), n_c, asum(R.cloud_matmul_dT, ax, ady, B, N, M, kd),
           what + " dT")
    if oc > kd:
        assert float(y.detach()[:, kd:].abs().max()) == 0.0, what + ": padded output columns"
    if xcols > kd:
        assert float(x.grad[:, kd:].abs().max()) == 0.0, what + ": dx past kd"
    return y.detach(), x.grad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kd,xcols,oc", [(3, 8, 8), (3, 3, 3), (64, 64, 64), (64, 72, 64)])
@pytest.mark.parametrize("shape", R.CLOUD_SHAPES, ids=str)
def test_cloud_matmul_forward_dx_and_dT_at_every_cloud_shape(shape, kd, xcols, oc, kind):
    """out_cols 8 for kd 3 and 64 for kd 64 as the encoder calls them; (3, 3, 3) is the unpadded form, (64, 72, 64) a wider
    aligned input (ldx = 72: still the matrix-pipe kernels)."""
    _cloud_matmul_case(kind, shape, kd, xcols, oc, f"x{xcols}")


@pytest.mark.parametrize("shape", list(R.ROUTE_SHAPES), ids=str)
def test_cloud_matmul64_routes_are_exact_and_take_the_route_they_claim(shape):
    """Four tiles per workgroup with a ragged last tile, N != M, a second workgroup that returns early, M = 0 - and one tile
    per workgroup just under the rule."""
    from catre_amd import hip

    assert hip.cloud_matmul_tpw(*shape) == R.ROUTE_SHAPES[shape]
    _cloud_matmul_case("exact", shape, 64, 64, 64, "route")


def test_cloud_matmul64_gives_the_same_bits_with_four_tiles_per_workgroup_as_with_one():
    """(256, 500, 130) groups four tiles per workgroup, (255, 500, 130) on the same data one: the same MFMA sequence per
    tile, so the rows of the first 255 objects are bit-equal, forward and transposed.  Rounded inputs."""
    from catre_amd import hip
    from catre_amd import train_ops as T

    (B, N, M), B1 = (256, 500, 130), 255
    assert hip.cloud_matmul_tpw(B, N, M) == 4 and hip.cloud_matmul_tpw(B1, N, M) == 1
    xn, Tn = R.rounded((B * (N + M), 64), "x", "same-bits"), R.rounded((2 * B, 64, 64), "T", "same-bits")
    dyn = R.rounded((B * (N + M), 64), "dy", "same-bits")
    rows = np.r_[0:B1 * N, B * N:B * N + B1 * M]          # the first 255 objects' observed and prior rows
    clouds = np.r_[0:B1, B:B + B1]
    x, Tm = _dev(xn, True), _dev(Tn)
    y = T.cloud_matmul(x, Tm, B, N, M)
    y.backward(_dev(dyn))
    x1 = _dev(xn[rows], True)
    y1 = T.cloud_matmul(x1, _dev(Tn[clouds]), B1, N, M)
    y1.backward(_dev(dyn[rows]))
    ridx = torch.from_numpy(rows).to(DEV)
    assert torch.equal(y.detach()[ridx], y1.detach()), "forward"
    assert torch.equal(x.grad[ridx], x1.grad), "transposed"
    aT = np.abs(Tn)
    _within(y, R.cloud_matmul(xn, Tn, B, N, M), R.bound(64, R.cloud_matmul(np.abs(xn), aT, B, N, M)), "cloud_matmul[route tpw=4] y")
    _within(x.grad, R.cloud_matmul_dx(dyn, Tn, B, N, M), R.bound(64, R.cloud_matmul_dx(np.abs(dyn), aT, B, N, M)),
            "cloud_matmul[route tpw=4] dx")


@pytest.mark.parametrize("kind", KINDS)
def test_cloud_matmul_fallback_kernels_for_odd_leading_dimensions(kind):
    """ld % 4 != 0 sends kd = 64 to k_cloud_matmul<64> and k_cloud_matmul_bwd_t<64>: ldx = 66, ldy = 65 through the C ABI
    (no wrapper builds such tensors).  The padding of the output rows keeps its sentinel."""
    from catre_amd import hip

    lib, st = hip.load(), _stream()
    B, N, M = R.FALLBACK_SHAPE
    ldx, ldy, kd = R.FALLBACK_LDX, R.FALLBACK_LDY, 64
    rows, C = B * (N + M), R.n_clouds(B, M)
    an = R.operand(kind, (rows, kd), "a", "fallback")          # the input of either product (x, or dy for the transposed one)
    bn = R.operand(kind, (rows, kd), "b", "fallback")          # the second operand of dT
    Tn = R.operand(kind, (C, kd, kd), "T", "fallback")

    def padded(data, ld):
        buf = torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=DEV)
        buf[:, :kd] = _dev(data)
        return buf

    Tm, n_c = _dev(Tn), R.cloud_rows(B, N, M).reshape(C, 1, 1)
    a_odd, b_odd, a_al, b_al = padded(an, ldx), padded(bn, ldy), _dev(an), _dev(bn)
    aa, ab, aT = np.abs(an), np.abs(bn), np.abs(Tn)
    for transpose, ref, asum in ((0, R.cloud_matmul(an, Tn, B, N, M), R.cloud_matmul(aa, aT, B, N, M)),
                                 (1, R.cloud_matmul_dx(an, Tn, B, N, M), R.cloud_matmul_dx(aa, aT, B, N, M))):
        out = torch.full((rows, ldy), SENTINEL, dtype=torch.float32, device=DEV)
        hip.check(lib.catre_op_cloud_matmul(hip.ptr(a_odd), ldx, hip.ptr(Tm), hip.ptr(out), ldy, kd, B, N, M, transpose,
                                            st), "catre_op_cloud_matmul")
        aligned = torch.empty(rows, kd, dtype=torch.float32, device=DEV)
        hip.check(lib.catre_op_cloud_matmul(hip.ptr(a_al), kd, hip.ptr(Tm), hip.ptr(aligned), kd, kd, B, N, M, transpose, st),
                  "catre_op_cloud_matmul")
        for got, nm in ((out[:, :kd], "fallback"), (aligned, "aligned")):
            _check(kind, got, ref, kd, asum, f"cloud_matmul[{kind} {nm} ld={ldx},{ldy} transpose={transpose}]")
        assert bool((out[:, kd:] == SENTINEL).all()), "padding of the output rows written"
    dT = torch.full((C, kd, kd), SENTINEL, dtype=torch.float32, device=DEV)
    hip.check(lib.catre_op_cloud_matmul_bwd_t(hip.ptr(a_odd), ldx, hip.ptr(b_odd), ldy, hip.ptr(dT), kd, B, N,
                                              M, st), "catre_op_cloud_matmul_bwd_t")
    dTa = torch.empty(C, kd, kd, dtype=torch.float32, device=DEV)
    hip.check(lib.catre_op_cloud_matmul_bwd_t(hip.ptr(a_al), kd, hip.ptr(b_al), kd, hip.ptr(dTa), kd, B, N, M, st),
              "catre_op_cloud_matmul_bwd_t")
    for got, nm in ((dT, "fallback"), (dTa, "aligned")):
        _check(kind, got, R.cloud_matmul_dT(an, bn, B, N, M, kd), n_c, R.cloud_matmul_dT(aa, ab, B, N, M, kd),
               f"cloud_matmul[{kind} {nm} ld={ldx},{ldy}] dT")


# ------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("J", R.POOL_J)
@pytest.mark.parametrize("shape", R.CLOUD_SHAPES + R.TIE_SHAPES, ids=str)
def test_maxpool_points_gives_the_first_maximum_and_scatters_to_it(shape, J):
    """Crafted ties, integers (natural ties) and N(0, 1): the pooled value equals the reference's, and the backward of a
    gradient that is nonzero everywhere puts dout[c, j] at the row of the FIRST maximum of (c, j) and zero elsewhere - which
    pins the arg-max table entry by entry.  A column of -inf pools to -inf at the cloud's row 0."""
    from catre_amd import train_ops as T

    B, N, M = shape
    rows = B * (N + M)
    for nm, yn in (("ties", R.tie_case(B, N, M, J)), ("exact", R.exact((rows, J), "pool", shape, J)),
                   ("rounded", R.rounded((rows, J), "pool", shape, J))):
        val, idx = R.maxpool(yn, B, N, M)
        dout = R.nonzero(val.shape, "dpool", shape, J)
        y = _dev(yn, True)
        p = T.maxpool_points(y, B, N, M)
        p.backward(_dev(dout))
        what = f"maxpool[{nm} {B}x{N}x{M} J={J}]"
        _equal(p, val, what + " value")
        _equal(y.grad, R.maxpool_bwd(dout, idx, rows), what + " scatter (arg-max rows)")
        if nm == "ties":
            e = np.flatnonzero(np.isneginf(val[0]))
            assert len(e) and np.array_equal(idx[:, e], np.broadcast_to(np.array([r0 for r0, _ in R.cloud_slices(B, N, M)])[:, None],
                                                                       idx[:, e].shape))


# ------------------------------------------------------------------------------------------------- per-cloud bias
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("J", R.BIAS_J)
@pytest.mark.parametrize("shape", R.CLOUD_SHAPES, ids=str)
def test_rowbias_add_clones_a_leaf_and_works_in_place_on_an_intermediate(shape, J, kind):
    from catre_amd import train_ops as T

    B, N, M = shape
    rows, C = B * (N + M), R.n_clouds(B, M)
    yn, bn = R.operand(kind, (rows, J), "y", shape, J), R.operand(kind, (C, J), "b", shape, J)
    dzn = R.operand(kind, (rows, J), "dz", shape, J)
    want = R.rowbias_add(yn, bn, B, N, M, dtype=np.float32)      # one fp32 add per element: equal for either kind
    what = f"rowbias[{kind} {B}x{N}x{M} J={J}]"

    def check_grads(y_leaf, bias):
        _equal(y_leaf.grad, dzn, what + " dy")
        _check(kind, bias.grad, R.rowbias_bwd(dzn, B, N, M), R.cloud_rows(B, N, M).reshape(C, 1),
               R.rowbias_bwd(np.abs(dzn), B, N, M), what + " dbias")

    # a leaf is cloned and left alone
    y0, b0 = _dev(yn, True), _dev(bn, True)
    z0 = T.rowbias_add(y0, b0, B, N, M)
    assert z0.data_ptr() != y0.data_ptr()
    _equal(y0, yn, what + " leaf input modified")
    _equal(z0, want, what + " z (clone)")
    z0.backward(_dev(dzn))
    check_grads(y0, b0)
    # a contiguous intermediate is updated in place
    y1, b1 = _dev(yn, True), _dev(bn, True)
    mid = y1.clone()
    z1 = T.rowbias_add(mid, b1, B, N, M)
    assert z1.data_ptr() == mid.data_ptr()
    _equal(y1, yn, what + " the intermediate's source modified")
    assert torch.equal(z1.detach(), z0.detach()), what + " z (in place)"
    z1.backward(_dev(dzn))
    check_grads(y1, b1)
    assert torch.equal(b1.grad, b0.grad)


# ------------------------------------------------------------------------------------------------- conv_p
def _wsum_operands(kind, B, P, tag):
    return (R.operand(kind, (B * P, 3), "y3", B, P, tag), R.operand(kind, (P,), "w", B, P, tag),
            R.operand(kind, (1,), "bp", B, P, tag), R.operand(kind, (B, 3), "dout", B, P, tag))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B", R.WSUM_B)
def test_weighted_point_sum_forward_and_backward(B, with_bias, kind):
    """B objects are the `splits` of k_reduce_splits_wide behind dw (16 partial groups; four partials in flight once
    k + 48 < splits); P walks k_wsum_fwd's 256-thread stride and the 64-output workgroups of the reduction."""
    from catre_amd import train_ops as T

    for P in R.WSUM_P:
        yn, wn, bpn, dn = _wsum_operands(kind, B, P, "wrapper")
        y3, w = _dev(yn, True), _dev(wn.reshape(1, P, 1), True)
        bp = _dev(bpn, True) if with_bias else None
        out = T.weighted_point_sum(y3, w, bp, B, P)
        out.backward(_dev(dn))
        what = f"wsum[{kind} B={B} P={P} {'bias' if with_bias else 'nobias'}]"
        ay, aw, ad = np.abs(yn), np.abs(wn), np.abs(dn)
        _check(kind, out, R.wsum(yn, wn, bpn if with_bias else None, B, P), P + 1,
               R.wsum(ay, aw, np.abs(bpn) if with_bias else None, B, P), what + " out")
        _check(kind, y3.grad, R.wsum_dY(dn, wn, B, P), 1, R.wsum_dY(ad, aw, B, P), what + " dY")
        _check(kind, w.grad.reshape(-1), R.wsum_dw(dn, yn, B, P), 3 * B, R.wsum_dw(ad, ay, B, P), what + " dw")
        if with_bias:
            _check(kind, bp.grad.reshape(()), R.wsum_dbias(dn), 3 * B, R.wsum_dbias(ad), what + " dbias")
        else:
            assert bp is None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B", R.WSUM_B)
def test_wsum_bwd_n_also_gives_the_neck_bias_gradient_and_accumulates(B, accumulate, kind):
    """catre_op_wsum_bwd_n: dY, dw, dbias and dbn = (sum_p w_p)(sum_b dout_b).  accumulate = 1 adds exactly the sums to what
    dw, dbias and dbn held; accumulate = 0 overwrites it.  dbn sums P + B terms in its factored form (and the prefill)."""
    from catre_amd import hip

    lib, st = hip.load(), _stream()
    for P in R.WSUM_P:
        yn, wn, _, dn = _wsum_operands(kind, B, P, "abi")
        pre_w, pre_b, pre_n = (R.operand(kind, s, "prefill", B, P, i) for i, s in enumerate(((P,), (1,), (3,))))
        dY = torch.full((B * P, 3), SENTINEL, dtype=torch.float32, device=DEV)
        dw, dbias, dbn = _dev(pre_w), _dev(pre_b), _dev(pre_n)
        dout, y3, w = _dev(dn), _dev(yn), _dev(wn)
        ws = torch.empty(B * P, dtype=torch.float32, device=DEV)
        hip.check(lib.catre_op_wsum_bwd_n(hip.ptr(dout), hip.ptr(y3), hip.ptr(w), hip.ptr(dY), hip.ptr(dw),
                                          hip.ptr(dbias), hip.ptr(dbn), accumulate, hip.ptr(ws), ws.numel() * 4, B, P, st),
                  "catre_op_wsum_bwd_n")
        what = f"wsum_bwd_n[{kind} B={B} P={P} acc={accumulate}]"
        ay, aw, ad = np.abs(yn), np.abs(wn), np.abs(dn)
        k = float(accumulate)
        _check(kind, dY, R.wsum_dY(dn, wn, B, P), 1, R.wsum_dY(ad, aw, B, P), what + " dY")
        _check(kind, dw, k * pre_w + R.wsum_dw(dn, yn, B, P), 3 * B + 1, k * np.abs(pre_w) + R.wsum_dw(ad, ay, B, P), what + " dw")
        _check(kind, dbias, k * pre_b + R.wsum_dbias(dn), 3 * B + 1, k * np.abs(pre_b) + R.wsum_dbias(ad), what + " dbias")
        _check(kind, dbn, k * pre_n + R.wsum_dbn(dn, wn), P + B + 1, k * np.abs(pre_n) + R.wsum_dbn(ad, aw), what + " dbn")


# ------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("J", R.COLSUM_J)
@pytest.mark.parametrize("rows", R.COLSUM_R)
def test_colsum_overwrites_and_accumulates(rows, J):
    """J < 256 repartitions the 256 threads into 256 // J row lanes (idle threads when 256 % J != 0); rows walks the
    eight-in-flight loop of a lane, the 32-row granularity of a split and more than one split (4097, 70001).  accumulate = 0
    through train_ops._colsum, accumulate = 1 through the C ABI on rows with a leading dimension of J + 3."""
    from catre_amd import hip
    from catre_amd import train_ops as T

    lib, st = hip.load(), _stream()
    for kind in KINDS:
        xn = R.operand(kind, (rows, J), "colsum", rows, J, amp=R.colsum_amp(rows))
        ref, asum = R.colsum(xn), R.colsum(np.abs(xn))
        what = f"colsum[{kind} R={rows} J={J}]"
        x = _dev(xn)
        _check(kind, T._colsum(x), ref, rows, asum, what)
        pre = R.operand(kind, (J,), "prefill", rows, J)
        wide = torch.full((rows, J + 3), SENTINEL, dtype=torch.float32, device=DEV)
        wide[:, :J] = x
        out = _dev(pre)
        ws = torch.empty(256 * J, dtype=torch.float32, device=DEV)
        hip.check(lib.catre_op_colsum(hip.ptr(wide), J + 3, rows, J, hip.ptr(out), 1, hip.ptr(ws), ws.numel() * 4, st),
                  "catre_op_colsum")
        _check(kind, out, pre + ref, rows + 1, np.abs(pre) + asum, what + " accumulate")
