"""Plain fp64 restatement of the PointNet encoder's three conv stacks, one layer at a time - the reference of
tests/test_train_encoder_fwd.py (the fused training forward `catre_train_{stn3d,stnkd,trunk}_fwd`) and of
tests/test_train_encoder_ref_host.py (this file against the oracle).  Written from catre_amd/pointnet.py and
train_forward.pointnet_rows_fused; torch only, no kernel code, runs on whatever device its inputs are on.

Rows are cloud-major like the kernels' buffers: B observed clouds of N rows, then B prior clouds of M rows; cloud c < B is
observed cloud c, cloud B + c is prior cloud c; `trans3` [2B,9] and `trans64` [2B,4096] hold one transform per CLOUD.

Every layer is fp64 `relu(W x + b)` of its input rows.  mode "bf16" rounds (RNE) the operands of a layer to bf16 where the
bf16-operand kernels round them (oracle/catre_oracle.py `operand_rounding`): the weights (at pack time) and the activation
rows (when they are staged) of every layer but the 3 -> 64 first layers, which are fp32 FMAs on unrounded operands, and
`trans64` in the feature transform.  Rounding happens at a layer's INPUT; the value a bf16-valued buffer must hold is the
rounding of what a layer returns here (`HOLDS_BF16`).  "fp32" and "split" round nothing.

`encoder_rows(..., saved=None)` runs the stacks free (each layer reads the previous one's output); with `saved` = the
kernels' own buffers every layer reads the SAVED input row instead (teacher forcing: one rounding flip does not travel
down the stack) and returns what that layer's saved output must be.  The last layer of a stack comes back before its pool
(`y_stn`, `y_fstn`, `y`); the pools and their arg-max rows are `pool` / `pool_reference`."""
import torch

MODES = ("fp32", "split", "bf16")
# (buffer a layer's output is saved in | pre-pool name, buffer of its input, layer, ReLU, fp32 FMAs on unrounded operands)
STACKS = {
    "stn": (("a1", "pts", "stn.conv1", True, True), ("a2", "a1", "stn.conv2", True, False), ("y_stn", "a2", "stn.conv3", False, False)),
    "fstn": (("f1", "h1", "fstn.conv1", True, False), ("f2", "f1", "fstn.conv2", True, False), ("y_fstn", "f2", "fstn.conv3", False, False)),
    "trunk": (("c2", "pf", "conv2", True, False), ("c3", "c2", "conv3", True, False), ("y", "c3", "conv4", False, False)),
}
# the buffers whose VALUES are bf16 in mode "bf16": bf16 tensors, and the two fp32 buffers written from a bf16 image
BF16_TENSORS = ("a1", "a2", "f1", "f2", "c2", "c3")
HOLDS_BF16 = BF16_TENSORS + ("h1", "pf")


def rne_bf16(t):
    """round to nearest even to bf16, back in fp64"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def dense(x, w, b, mode, relu=True, fma32=False):
    """fp64 act(x W^T + b) of the rows x [R,K]; w [J,K] or [J,K,1], b [J]"""
    x = x.to(torch.float64)
    w = w.reshape(w.shape[0], -1).to(x.device, torch.float64)
    if mode == "bf16" and not fma32:
        x, w = rne_bf16(x), rne_bf16(w)
    y = x @ w.t() + b.to(x.device, torch.float64)
    return y.clamp_min(0) if relu else y


def cloud_groups(t, B, N, M):
    """rows [B*N + B*M, ...] -> ((observed [B,N,...], first row of each cloud [B]), (prior [B,M,...], ...))"""
    ar = torch.arange(B, device=t.device)
    return ((t[:B * N].reshape(B, N, *t.shape[1:]), ar * N), (t[B * N:].reshape(B, M, *t.shape[1:]), B * N + ar * M))


def cloud_matmul(rows, T, k, B, N, M, mode="fp32", rounded=False):
    """rows[:, :k] of every cloud times that cloud's k x k transform (`torch.bmm(x^T, trans)`, pointnet.py:100-102,107-109)"""
    x = rows[:, :k].to(torch.float64)
    T = T.reshape(2 * B, k, k).to(x.device, torch.float64)
    if mode == "bf16" and rounded:
        x, T = rne_bf16(x), rne_bf16(T)
    (xo, _), (xp, _) = cloud_groups(x, B, N, M)
    return torch.cat([(xo @ T[:B]).reshape(B * N, k), (xp @ T[B:]).reshape(B * M, k)], 0)


def encoder_rows(pts, trans3, trans64, sd, mode, B, N, M, saved=None, prefix="pcl_net"):
    """pts [B*N + B*M, 3] cloud-major -> {a1 a2 y_stn x1 h1 f1 f2 y_fstn pf c2 c3 y}, fp64.  `saved`: the kernels' buffers
    by name (None entries: not saved, the free-running value is used)."""
    assert mode in MODES
    out = {"pts": pts.to(torch.float64)}

    def src(name):
        if saved is not None and name != "pts" and saved.get(name) is not None:
            return saved[name].to(torch.float64)
        return out[name]

    def stack(which):
        for name, inp, layer, relu, fma32 in STACKS[which]:
            out[name] = dense(src(inp), sd[f"{prefix}.{layer}.weight"], sd[f"{prefix}.{layer}.bias"], mode, relu, fma32)

    stack("stn")
    x1 = cloud_matmul(out["pts"], trans3, 3, B, N, M)
    out["x1"] = torch.cat([x1, torch.zeros(x1.shape[0], 5, dtype=torch.float64, device=x1.device)], 1)   # columns 0..2 of 8
    out["h1"] = dense(src("x1")[:, :3], sd[f"{prefix}.conv1.weight"], sd[f"{prefix}.conv1.bias"], mode, True, True)
    stack("fstn")
    out["pf"] = cloud_matmul(src("h1"), trans64, 64, B, N, M, mode, rounded=True)
    stack("trunk")
    del out["pts"]
    return out


def pool(y, B, N, M, relu):
    """max over each cloud's rows of the pre-pool rows y [R,J] -> [2B,J]; relu: the two STN stacks"""
    g = torch.cat([v.max(1).values for v, _ in cloud_groups(y, B, N, M)], 0)
    return g.clamp_min(0) if relu else g


def first_identical_row(pts, B, N, M):
    """[R] int64: for every row the first row of ITS cloud that holds the bit-identical input point"""
    first = []
    for p, base in cloud_groups(pts, B, N, M):
        n = p.shape[1]
        eq = (p[:, :, None, :] == p[:, None, :, :]).all(-1)                              # [B,n,n]
        ar = torch.arange(n, device=p.device)
        first.append((torch.where(eq, ar[None, None, :], n).min(-1).values + base[:, None]).reshape(-1))
    return torch.cat(first)


def pool_reference(y, first, B, N, M):
    """The max-pool of the pre-pool rows y [R,J] with what decides its arg-max: (best [2B,J], the row that must win = the
    first row holding the best row's input point [2B,J], second = the best value among rows with ANOTHER input point
    [2B,J], -inf where the cloud holds one point only)."""
    best, row, second = [], [], []
    for (v, base), (f, _) in zip(cloud_groups(y, B, N, M), cloud_groups(first, B, N, M)):
        m, am = v.max(1)                                                                  # [B,J]
        grp = torch.gather(f, 1, am)                                                      # first row of the winner's point
        other = f[:, :, None] != grp[:, None, :]
        second.append(v.masked_fill(~other, float("-inf")).max(1).values)
        best.append(m)
        row.append(grp)
    return torch.cat(best, 0), torch.cat(row, 0), torch.cat(second, 0)


def bound(want, mode, name=None):
    """The allowed |got - want| per element.  fp32: atol = rtol = 2e-5 (fp32 re-association on O(1) data,
    test_hip_train_ops._cmp); split: atol 1e-4, rtol 2e-5 (test_linear_fwd_bwd); bf16: 2e-5 max|want| (a product of rounded
    operands, test_weight_gradient_on_the_bf16_pipe), and one rounding to bf16, 2^-8 |want|, on top for a bf16 tensor."""
    a = want.abs()
    if mode == "fp32":
        return 2e-5 + 2e-5 * a
    if mode == "split":
        return 1e-4 + 2e-5 * a
    t = 2e-5 * a.max() + torch.zeros_like(a)
    return t + a / 256 if name in BF16_TENSORS else t


def pool_bound(y, best, mode):
    """`bound` of the pooled layer's rows y, taken at the pooled values `best`"""
    if mode == "bf16":
        return 2e-5 * y.abs().max() + torch.zeros_like(best)
    return bound(best, mode)


def rows_error(got, want, mode, name):
    """(elements out of bound, worst |got - expected|, worst bound) of a saved buffer against this reference.  A buffer
    of mode "bf16" that is an fp32 tensor but holds bf16 VALUES (h1, pf) is held to the fp32-buffer bound BEFORE the
    rounding the reference itself applies: rne(want - tol) <= got <= rne(want + tol), RNE being monotonic - where no bf16
    boundary lies within tol of want that is |got - rne(want)| = 0."""
    got = got.to(torch.float64)
    tol = bound(want, mode, name)
    if mode == "bf16" and name in HOLDS_BF16 and name not in BF16_TENSORS:
        bad = (got < rne_bf16(want - tol)) | (got > rne_bf16(want + tol))
        err = (got - rne_bf16(want)).abs()
    else:
        err = (got - want).abs()
        bad = ~(err <= tol)
    return int(bad.sum()), float(err.max()), float(tol.max())


def skipped_share(y, first, B, N, M, mode, stn):
    """The share of (cloud, channel) pairs whose arg-max this reference cannot decide: the best row beats the best row
    with another input point by no more than the margin, twice the bound.  stn: channels whose maximum is <= 0 carry no
    gradient (the pooled ReLU) and are not counted at all."""
    best, _, second = pool_reference(y, first, B, N, M)
    counted = best > 0 if stn else torch.ones_like(best, dtype=torch.bool)
    close = counted & ~(best - second > 2 * pool_bound(y, best, mode))
    return float(close.sum()) / max(int(counted.sum()), 1)


SKIP_CAP = {"fp32": 0.05, "bf16": 0.05, "split": 0.15}
SEED = 31


def cloud_ranges(B, N, M, device=None):
    """([2B] first row, [2B] one past the last row) of every cloud"""
    ar = torch.arange(B, device=device)
    lo = torch.cat([ar * N, B * N + ar * M])
    return lo, lo + torch.cat([torch.full_like(ar, N), torch.full_like(ar, M)])


# ---- inputs shared by the host test and the GPU test (CPU tensors, seeded) -----------------------------------------------
def case_points(B, N, M, seed):
    """`synth.make_inputs` posed like `batch_updater_test` does -> cloud-major point rows [B*N + B*M, 3] (fp32, CPU)"""
    from catre_amd import synth
    from oracle import catre_oracle as O

    b = synth.make_inputs(B, N, M, seed=seed)
    x, k = O.pose_apply(b["pcl"], b["obj_kps"], b["obj_pose_est"], b["obj_scale_est"])
    return torch.cat([x.permute(0, 2, 1).reshape(-1, 3), k.permute(0, 2, 1).reshape(-1, 3)], 0).contiguous()


def transforms(B, seed):
    """per-cloud trans3 = I + 0.3 randn [2B,9], trans64 = I + 0.05 randn [2B,4096]: no identities, not the STNs' own"""
    g = torch.Generator().manual_seed(7919 * seed + 11)
    t3 = torch.eye(3).reshape(1, 9) + 0.3 * torch.randn(2 * B, 9, generator=g)
    t64 = torch.eye(64).reshape(1, 4096) + 0.05 * torch.randn(2 * B, 4096, generator=g)
    return t3.contiguous(), t64.contiguous()


def repeat_one_point(pts, B, N, M):
    """every cloud is its first point, repeated"""
    return torch.cat([p[:, :1].expand_as(p).reshape(-1, 3) for p, _ in cloud_groups(pts, B, N, M)], 0).contiguous()


def repeat_first_tile(pts, B, N, M, tile=64):
    """every cloud is its first tile, repeated: tile t is a copy of tile 0"""
    return torch.cat([p[:, :tile].repeat(1, p.shape[1] // tile, 1).reshape(-1, 3) for p, _ in cloud_groups(pts, B, N, M)],
                     0).contiguous()


def mirror_half_tiles(pts, B, N, M, tile=64):
    """inside every tile, rows 32..63 are rows 0..31 in reversed order (row 32 + i = row 31 - i)"""
    t = pts.reshape(-1, tile, 3).clone()
    t[:, tile // 2:] = t[:, :tile // 2].flip(1)
    return t.reshape(-1, 3).contiguous()
