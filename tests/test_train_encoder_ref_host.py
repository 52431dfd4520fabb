"""CPU: tests/train_encoder_ref.py, the fp64 reference of tests/test_train_encoder_fwd.py, against the oracle.

The restatement runs END TO END here (free-running: every layer reads the previous one's output), handed the oracle's own
STN transforms, and must reproduce `oracle.catre_oracle.pointnet_feat(detail=True)` - plain and under
`operand_rounding("bf16")` - within 2e-5, the oracle's own accuracy against the reference
(test_hip_bf16.py::test_oracle_emulation...).  Both run in fp64 on the same inputs, so a rounding applied at another place
than the oracle's shows as >= 2^-9 relative and everything else as ~1e-15.

The rest holds the GPU test's preconditions from the reference alone: the crafted first-maximum inputs are what their
helpers claim, and on the exact inputs and transforms of the GPU cases the share of (cloud, channel) pairs whose arg-max
the margin leaves undecided stays under the caps (5 % fp32 / bf16, 15 % split)."""
import pytest
import torch

from tests import train_encoder_ref as R
from tests.util import recipe_sd


def _sd(N, M):
    from catre_amd.config import default_cfg

    return {k: v for k, v in recipe_sd(default_cfg(num_pcl=N, num_kps=M, device="cpu")).items() if k.startswith("pcl_net.")}


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_restatement_free_running_matches_the_oracle(mode):
    from oracle import catre_oracle as O

    B, N, M = 2, 192, 64
    sd = _sd(N, M)
    sdd = {k: v.double() for k, v in sd.items()}
    pts = R.case_points(B, N, M, R.SEED).double()
    (xo, _), (xp, _) = R.cloud_groups(pts, B, N, M)
    want = []
    with torch.no_grad(), O.operand_rounding("bf16" if mode == "bf16" else None):
        for x in (xo, xp):
            want.append(O.pointnet_feat(x.permute(0, 2, 1), sdd, detail=True)[1])
    cat = lambda k: torch.cat([w[k].reshape(B, -1) for w in want], 0)
    rows = lambda k: torch.cat([w[k].permute(0, 2, 1).reshape(-1, w[k].shape[1]) for w in want], 0)
    got = R.encoder_rows(pts, cat("trans"), cat("trans_feat"), sd, mode, B, N, M)
    assert set(got) == {"a1", "a2", "y_stn", "x1", "h1", "f1", "f2", "y_fstn", "pf", "c2", "c3", "y"}
    assert all(v.dtype == torch.float64 for v in got.values())
    assert got["x1"].shape == (B * (N + M), 8) and not got["x1"][:, 3:].any()
    pf = R.rne_bf16(got["pf"]) if mode == "bf16" else got["pf"]          # the oracle's pointfeat is the rounded image
    pairs = {"pointfeat": (pf, rows("pointfeat")), "g": (R.pool(got["y"], B, N, M, False), cat("g")),
             "stn_pool": (R.pool(got["y_stn"], B, N, M, True), cat("stn_pool")),
             "fstn_pool": (R.pool(got["y_fstn"], B, N, M, True), cat("fstn_pool"))}
    for k, (a, b) in pairs.items():
        err = float((a - b).abs().max())
        print(f"{mode} {k}: max abs difference to the oracle {err:.2e}")
        assert err <= 2e-5, (k, err)
    if mode == "bf16":   # the rounding does something: the two modes are bf16-far apart
        plain = R.encoder_rows(pts, cat("trans"), cat("trans_feat"), sd, "fp32", B, N, M)
        assert float((plain["y"] - got["y"]).abs().max()) > 1e-3


def test_teacher_forcing_reads_the_saved_rows():
    """With `saved` every layer starts from the saved input: a changed saved row changes the NEXT layer only."""
    B, N, M = 1, 64, 64
    sd = _sd(N, M)
    pts = R.case_points(B, N, M, R.SEED)
    t3, t64 = R.transforms(B, R.SEED)
    free = R.encoder_rows(pts, t3, t64, sd, "fp32", B, N, M)
    saved = {k: v.float() for k, v in free.items() if not k.startswith("y")}
    saved["c2"] = saved["c2"] + 1.0
    saved["a1"] = None                                                    # not saved: the reference's own value is used
    forced = R.encoder_rows(pts, t3, t64, sd, "fp32", B, N, M, saved=saved)
    assert float((forced["c3"] - free["c3"]).abs().max()) > 1e-2
    for k in ("a1", "a2", "y_stn", "x1", "h1", "f1", "f2", "y_fstn", "pf", "c2", "y"):
        assert float((forced[k] - free[k]).abs().max()) <= 1e-6, k         # (the saved rows are fp32 roundings)


def test_bounds_and_the_bf16_valued_interval():
    want = torch.tensor([1.0, -2.0, 0.0, 100.0], dtype=torch.float64)
    assert torch.allclose(R.bound(want, "fp32"), torch.tensor([4e-5, 6e-5, 2e-5, 2.02e-3], dtype=torch.float64))
    assert torch.allclose(R.bound(want, "split"), torch.tensor([1.2e-4, 1.4e-4, 1e-4, 2.1e-3], dtype=torch.float64))
    assert torch.allclose(R.bound(want, "bf16", "g"), torch.full((4,), 2e-3, dtype=torch.float64))
    assert torch.allclose(R.bound(want, "bf16", "c3"), 2e-3 + want.abs() / 256)
    # h1 / pf in bf16: the bf16 neighbours of `want` pass only where a rounding boundary lies within the fp32 bound
    w = torch.tensor([1.0 + 2 ** -8 - 1e-6, 1.25, 4.0], dtype=torch.float64)   # just under a boundary; exact; exact
    tol = 2e-5 * 4.0
    assert tol > 1e-6
    ok = torch.tensor([1.0 + 2 ** -7, 1.25, 4.0])
    assert R.rows_error(ok, w, "bf16", "h1")[0] == 0                      # the flip across the near boundary is allowed
    assert R.rows_error(torch.tensor([1.0, 1.25 + 2 ** -7, 4.0]), w, "bf16", "h1")[0] == 1   # a whole ulp off is not
    assert R.rows_error(torch.tensor([1.0, 1.25, 4.0 + 1e-4]), w, "bf16", "h1")[0] == 1      # nor an unrounded value
    assert R.rows_error(torch.tensor([1.0, 1.25, 4.0 + 2e-4]), w, "fp32", "h1")[0] == 2      # fp32: no rounding is forgiven


def test_crafted_inputs_are_what_they_claim():
    B, N, M = 2, 192, 64
    pts = R.case_points(B, N, M, R.SEED)
    lo, hi = R.cloud_ranges(B, N, M)
    assert lo.tolist() == [0, 192, 384, 448] and hi.tolist() == [192, 384, 448, 512]
    own = torch.repeat_interleave(lo, hi - lo)                            # first row of every row's cloud
    one = R.repeat_one_point(pts, B, N, M)
    assert one.shape == pts.shape and torch.equal(one, pts[own])
    assert torch.equal(R.first_identical_row(one, B, N, M), own)
    rep = R.repeat_first_tile(pts, B, N, M)
    rel = torch.arange(B * (N + M)) - own
    assert rep.shape == pts.shape and torch.equal(rep, pts[own + rel % 64])
    f = R.first_identical_row(rep, B, N, M)
    assert bool((f - own < 64).all()) and bool((f <= torch.arange(len(f))).all())
    mir = R.mirror_half_tiles(pts, B, N, M)
    r = torch.arange(B * (N + M))
    src = torch.where(r % 64 < 32, r, r - r % 64 + 63 - r % 64)
    assert torch.equal(mir, pts[src]) and torch.equal(mir.reshape(-1, 64, 3)[:, 32], mir.reshape(-1, 64, 3)[:, 31])
    f = R.first_identical_row(mir, B, N, M)
    assert bool((f[r % 64 >= 32] < r[r % 64 >= 32]).all())               # every second-half row has an earlier copy
    assert bool(((f - own) % 64 < 32).all())
    # the plain inputs: re-sampled with replacement, so identical points exist - and the first of them is found
    f = R.first_identical_row(pts, B, N, M)
    assert torch.equal(pts[f], pts) and bool((f <= r).all()) and bool((f >= own).all())


def test_pool_reference_names_the_first_row_of_the_winning_point():
    B, N, M = 1, 4, 2
    pts = torch.tensor([[0., 0, 0], [1, 0, 0], [1, 0, 0], [2, 0, 0], [5, 0, 0], [5, 0, 0]])
    y = torch.tensor([[1.0, 9.0], [3.0, 0.0], [3.0, 0.0], [2.0, 8.5], [7.0, -1.0], [7.0, -1.0]], dtype=torch.float64)
    first = R.first_identical_row(pts, B, N, M)
    assert first.tolist() == [0, 1, 1, 3, 4, 4]
    best, row, second = R.pool_reference(y, first, B, N, M)
    assert best.tolist() == [[3.0, 9.0], [7.0, -1.0]] and row.tolist() == [[1, 0], [4, 4]]
    assert second.tolist() == [[2.0, 8.5], [float("-inf")] * 2]
    assert R.pool(y, B, N, M, True).tolist() == [[3.0, 9.0], [7.0, 0.0]]
    assert R.skipped_share(y, first, B, N, M, "fp32", stn=True) == 0.0    # the channel with maximum -1 is not counted
    assert R.skipped_share(y, first, B, N, M, "fp32", stn=False) == 0.0
    y[3, 1] = 9.0 - 1e-5                                                  # inside the margin 2 (2e-5 + 2e-5 * 9)
    assert R.skipped_share(y, first, B, N, M, "fp32", stn=False) == 0.25


@pytest.mark.parametrize("shape", [(1, 64, 64), (2, 192, 64), (33, 128, 128)])
def test_the_margin_leaves_out_no_more_than_the_caps(shape):
    """The condition under which the GPU test's exact arg-max assertion means something, from the reference alone, on the
    inputs and transforms the GPU cases use.  (The two 192-point grids of the GPU test assert the same caps there, on the
    device's fp64 reference: they take a while on a CPU.)"""
    B, N, M = shape
    sd = _sd(N, M)
    pts = R.case_points(B, N, M, R.SEED)
    t3, t64 = R.transforms(B, R.SEED)
    first = R.first_identical_row(pts, B, N, M)
    for mode in R.MODES:
        ref = R.encoder_rows(pts, t3, t64, sd, mode, B, N, M)
        for k in ("y_stn", "y_fstn", "y"):
            share = R.skipped_share(ref[k], first, B, N, M, mode, stn=k != "y")
            print(f"{shape} {mode} {k}: {100 * share:.2f} % of the pairs inside the margin (cap {100 * R.SKIP_CAP[mode]:.0f} %)")
            assert share <= R.SKIP_CAP[mode], (shape, mode, k, share)
