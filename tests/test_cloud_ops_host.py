"""CPU checks behind tests/test_cloud_ops_edges.py: the fp64 references of tests/cloud_ops_ref.py against torch fp64
autograd (`torch.bmm`-style products, `x.max(0)`, `F.conv1d`) at every small case shape, and the preconditions of the cases,
asserted here so that a later edit of a generator or a shape list cannot silently void a GPU test:

  - integer cases: the largest sum of absolute terms any output can reach stays below 2^24 (fp32 exact in any order);
  - tie cases: every cloud holds the column types a) - f) of `cloud_ops_ref.tie_cloud` that its row count admits - a) needs three rows,
    b) needs 33 - and every type is present at the n that admit all of them;
  - route cases: each kd = 64 route shape takes the tiles-per-workgroup value it claims, asked of the library's own rule
    (`catre_op_cloud_matmul_tpw`, the function the launch calls - no GPU needed), and has the geometry its comment claims.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from catre_amd import hip
from tests import cloud_ops_ref as R


def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(grad)


def _same(got, want, what):
    np.testing.assert_allclose(np.asarray(got), want.detach().numpy(), rtol=1e-12, atol=1e-12, err_msg=what)


# ------------------------------------------------------------------------------------------------- reference against autograd
@pytest.mark.parametrize("shape", R.CLOUD_SHAPES + R.TIE_SHAPES, ids=str)
@pytest.mark.parametrize("kd,xcols", [(3, 8), (64, 64)])
def test_cloud_matmul_reference_matches_autograd(shape, kd, xcols):
    B, N, M = shape
    rows, C = B * (N + M), R.n_clouds(B, M)
    x, T = _t(R.rounded((rows, xcols), "x", shape, kd), True), _t(R.rounded((C, kd, kd), "T", shape, kd), True)
    dy = R.rounded((rows, kd), "dy", shape, kd)
    # cloud-major rows as two batches of equal clouds
    y = torch.cat([torch.bmm(x[:B * N, :kd].view(B, N, kd), T[:B]).view(B * N, kd)]
                  + ([torch.bmm(x[B * N:, :kd].view(B, M, kd), T[B:]).view(B * M, kd)] if M else []))
    y.backward(_t(dy))
    xn, Tn = x.detach().numpy(), T.detach().numpy()
    _same(R.cloud_matmul(xn, Tn, B, N, M), y, "y")
    _same(R.cloud_matmul_dx(dy, Tn, B, N, M), x.grad[:, :kd], "dx")
    assert float(x.grad[:, kd:].abs().sum()) == 0.0
    _same(R.cloud_matmul_dT(xn, dy, B, N, M, kd), T.grad, "dT")


def _torch_pool(y, B, N, M):
    out = [y[r0:r0 + n].max(0) for r0, n in R.cloud_slices(B, N, M)]
    return torch.stack([o[0] for o in out]), np.stack([o[1].numpy() + r0 for o, (r0, _) in zip(out, R.cloud_slices(B, N, M))])


@pytest.mark.parametrize("shape", R.CLOUD_SHAPES + R.TIE_SHAPES, ids=str)
@pytest.mark.parametrize("J", R.POOL_J)
def test_maxpool_reference_matches_torch_max_and_its_backward(shape, J):
    B, N, M = shape
    for data in (R.tie_case(B, N, M, J), R.exact((B * (N + M), J), "pool", shape, J), R.rounded((B * (N + M), J), "pool", shape, J)):
        y = _t(data, True)
        val, idx = _torch_pool(y, B, N, M)
        rv, ri = R.maxpool(data, B, N, M)
        np.testing.assert_array_equal(rv, val.detach().numpy())      # -inf / +inf included
        np.testing.assert_array_equal(ri, idx)                       # torch.max: "the indices of the first maximal value"
        dout = R.nonzero(rv.shape, "dpool", shape, J)
        val.backward(_t(dout))
        np.testing.assert_array_equal(R.maxpool_bwd(dout, ri, data.shape[0]), y.grad.numpy())


@pytest.mark.parametrize("shape", R.CLOUD_SHAPES, ids=str)
@pytest.mark.parametrize("J", R.BIAS_J)
def test_rowbias_reference_matches_autograd(shape, J):
    B, N, M = shape
    y, b = _t(R.rounded((B * (N + M), J), "y", shape, J), True), _t(R.rounded((R.n_clouds(B, M), J), "b", shape, J), True)
    dz = R.rounded((B * (N + M), J), "dz", shape, J)
    # [obs | prior] per object: the bias rows of an object's two clouds, repeated over their points
    full = torch.cat([b[:B].unsqueeze(1).expand(B, N, J)] + ([b[B:].unsqueeze(1).expand(B, M, J)] if M else []), 1)
    z = y + full.reshape(B * (N + M), J)
    z.backward(_t(dz))
    _same(R.rowbias_add(y.detach().numpy(), b.detach().numpy(), B, N, M), z, "z")
    _same(R.rowbias_bwd(dz, B, N, M), b.grad, "dbias")
    _same(dz, y.grad, "dy")
    # the fp32 form the kernel is held to, bit for bit: one fp32 add per element
    y32, b32 = R.rounded((B * (N + M), J), "y", shape, J), R.rounded((R.n_clouds(B, M), J), "b", shape, J)
    r = np.arange(B * (N + M))
    cloud = np.where(r % (N + M) < N, r // (N + M), B + r // (N + M))
    want = torch.from_numpy(y32) + torch.from_numpy(b32)[torch.from_numpy(cloud)]
    np.testing.assert_array_equal(R.rowbias_add(y32, b32, B, N, M, dtype=np.float32), want.numpy())


@pytest.mark.parametrize("B", R.WSUM_B)
@pytest.mark.parametrize("with_bias", [True, False])
def test_wsum_reference_matches_conv1d_autograd(B, with_bias):
    for P in R.WSUM_P:
        a = _t(R.rounded((B * P, 3), "a", B, P), True)          # the neck's output before its bias
        bn = _t(R.rounded((3,), "bn", B, P), True)
        w = _t(R.rounded((1, P, 1), "w", B, P), True)
        bias = _t(R.rounded((1,), "bp", B, P), True) if with_bias else None
        dout = R.rounded((B, 3), "dout", B, P)
        y3 = a + bn
        y3.retain_grad()
        out = F.conv1d(y3.view(B, P, 3), w, bias).squeeze(1)    # Conv1d(P, 1, 1) over the point axis
        out.backward(_t(dout))
        yn, wn = y3.detach().numpy(), w.detach().numpy().reshape(-1)
        _same(R.wsum(yn, wn, None if bias is None else bias.detach().numpy(), B, P), out, "out")
        _same(R.wsum_dY(dout, wn, B, P), y3.grad, "dY")
        _same(R.wsum_dw(dout, yn, B, P), w.grad.reshape(-1), "dw")
        _same(R.wsum_dbn(dout, wn), bn.grad, "dbn")
        if with_bias:
            _same(R.wsum_dbias(dout), bias.grad.reshape(()), "dbias")


@pytest.mark.parametrize("rows", [r for r in R.COLSUM_R if r <= 4097])
def test_colsum_reference_matches_torch(rows):
    for J in R.COLSUM_J:
        x = R.rounded((rows, J), "colsum", rows, J)
        _same(R.colsum(x), torch.from_numpy(x).double().sum(0), "colsum")


# ------------------------------------------------------------------------------------------------- preconditions: integer cases
def test_integer_cases_stay_exact_in_fp32_in_any_order():
    lim = R.EXACT_LIMIT
    for B, N, M in R.CLOUD_SHAPES + tuple(R.ROUTE_SHAPES) + (R.FALLBACK_SHAPE,):
        for kd in (3, 64):
            assert R.worst_abs_sum("cloud_matmul", kd=kd) < lim
        assert R.worst_abs_sum("cloud_matmul_dT", N=N, M=M) < lim
        assert R.worst_abs_sum("rowbias_bwd", N=N, M=M) < lim
    assert R.worst_abs_sum("rowbias_add") < lim
    for B in R.WSUM_B:
        for P in R.WSUM_P:
            for op in ("wsum", "wsum_dw", "wsum_dbias", "wsum_dbn"):
                assert R.worst_abs_sum(op, B=B, P=P) < lim, (op, B, P)
    for rows in R.COLSUM_R:
        assert R.worst_abs_sum("colsum", R=rows, amp=R.colsum_amp(rows)) < lim, rows
    assert R.worst_abs_sum("colsum", R=70001, amp=R.AMP) < lim and R.colsum_amp(70001) == 4   # (the longest sum runs on [-4, 4]; [-8, 8] would hold too)
    # the generators keep their word: integers, inside the amplitude, both ends reached, seeded per case
    for amp in (R.AMP, 4):
        x = R.exact((4096, 3), "probe", amp=amp)
        assert x.dtype == np.float32 and np.array_equal(x, np.round(x)) and x.min() == -amp and x.max() == amp
    assert np.array_equal(R.exact((5, 5), "k", 1), R.exact((5, 5), "k", 1))
    assert not np.array_equal(R.exact((5, 5), "k", 1), R.exact((5, 5), "k", 2))
    d = R.nonzero((4096,), "probe")
    assert np.array_equal(d, np.round(d)) and np.abs(d).min() == 1 and np.abs(d).max() == R.AMP and (d < 0).any() and (d > 0).any()
    # the worst case is a bound on what the references give for the data actually used (abs operands -> sum of |terms|)
    B, N, M = 2, 130, 45
    x, T = np.abs(R.exact((B * (N + M), 64), "x")), np.abs(R.exact((2 * B, 64, 64), "T"))
    assert R.cloud_matmul(x, T, B, N, M).max() <= R.worst_abs_sum("cloud_matmul", kd=64)
    assert R.cloud_matmul_dT(x, x, B, N, M, 64).max() <= R.worst_abs_sum("cloud_matmul_dT", N=N, M=M)


# ------------------------------------------------------------------------------------------------- preconditions: tie cases
def test_tie_cases_hold_every_column_type_their_row_count_admits():
    assert set(R.TIE_N) == {1, 3, 4, 5, 33, 65, 130}
    assert {n for _, n, _ in R.TIE_SHAPES} == set(R.TIE_N) == {m for _, _, m in R.TIE_SHAPES}
    assert R.tie_types_possible(1) == set("cdef") and R.tie_types_possible(3) == set("acdef")
    assert R.tie_types_possible(32) == set("acdef") and R.tie_types_possible(33) == set("abcdef")
    full = 0
    for B, N, M in R.TIE_SHAPES:
        for J in R.POOL_J:
            y = R.tie_case(B, N, M, J)
            assert y.shape == (B * (N + M), J) and y.dtype == np.float32 and not np.isnan(y).any()
            for r0, n in R.cloud_slices(B, N, M):
                found, want = R.tie_types_found(y[r0:r0 + n]), R.tie_types_possible(n)
                assert want <= found, (B, N, M, J, r0, sorted(want - found))
                full += want == set(R.TIE_TYPES)
    assert full >= 3 * 2 * len(R.POOL_J)            # n = 33, 65, 130, as N and as M: all six types in one cloud


def test_tie_types_are_read_from_the_data():
    """The classifier itself: hand-made columns, one type each."""
    n = 40
    base = np.full((n, 1), -1.0, dtype=np.float32)

    def col(**rows):
        y = base.copy()
        for r, v in rows.items():
            y[int(r[1:]), 0] = v
        return R.tie_types_found(y)

    assert col(r1=5, r2=5) == {"a"} and col(r6=5, r9=5) == {"a"}
    assert col(r0=5, r1=5) == {"c"}                      # the earlier row in lane 0: not a)
    assert col(r1=5, r5=5) == set()                      # same lane, same batch: neither
    assert col(r1=5, r33=5) == {"b"} and col(r0=5, r32=5) == {"b", "c"}
    assert col(r39=5) == {"d"} and col(r0=5) == {"c"}
    assert col(r7=np.inf) == {"f"} and col(r7=np.inf, r8=np.inf) == {"a"}
    assert R.tie_types_found(np.full((n, 1), -np.inf, dtype=np.float32)) == {"e"}


# ------------------------------------------------------------------------------------------------- preconditions: routes
def _tpw_rule(B, N, M):
    """The rule as catre_op_cloud_matmul carried it inline: 4 tiles per workgroup once that leaves >= 1024 workgroups."""
    C, tiles = R.n_clouds(B, M), (max(N, M) + 63) // 64
    return 4 if tiles >= 4 and C * (tiles // 4) >= 1024 else 1


def test_route_shapes_take_the_tiles_per_workgroup_they_claim():
    for (B, N, M), tpw in R.ROUTE_SHAPES.items():
        assert hip.cloud_matmul_tpw(B, N, M) == tpw == _tpw_rule(B, N, M), (B, N, M)
    for B, N, M in R.CLOUD_SHAPES + R.TIE_SHAPES + (R.FALLBACK_SHAPE,):
        assert hip.cloud_matmul_tpw(B, N, M) == 1
    # what the route shapes are there for
    tiles = lambda n: (n + 63) // 64
    assert tiles(500) == 8 and 500 - 7 * 64 == 52               # two workgroups per observed cloud, a 52-row last tile
    assert tiles(130) == 3 and 130 <= 4 * 64                    # priors end in the first workgroup's third tile: the second returns
    assert tiles(200) == 4 and 200 - 3 * 64 == 8 and R.n_clouds(1024, 0) * (4 // 4) == 1024   # exactly on the threshold
    assert R.n_clouds(255, 130) * (8 // 4) == 1020              # just under it


def test_the_exported_rule_is_the_inline_rule_everywhere_near_its_thresholds():
    lib = hip.load()
    for B in (1, 2, 127, 128, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4096):
        for N in (1, 63, 64, 192, 193, 255, 256, 257, 448, 449, 500, 511, 512, 513, 1024, 4096):
            for M in (0, 1, 64, 130, 256, 257, 512, 1024, 4096):
                assert lib.catre_op_cloud_matmul_tpw(B, N, M) == _tpw_rule(B, N, M), (B, N, M)
    for bad in ((0, 64, 64), (4, 0, 64), (4, 64, -1)):
        assert lib.catre_op_cloud_matmul_tpw(*bad) == -1
        with pytest.raises(hip.CatreHipError):
            hip.cloud_matmul_tpw(*bad)
