"""The row-sparse backward of the encoder's conv stacks (`pooled_chain`, `pointfeat_hub`) at the edges of its live-row
list, against fp64 torch autograd.

The backward reads only the arg-max table `idx`, the pooled values `gp` and the upstream gradient, so these tests CRAFT
the table (`make_idx`) instead of taking whatever random data gives: one live row per cloud, a live-row count on, one
below and one above the 64 / 128 row tiles, every row live, empty clouds in front / in the middle / at the end (the last
cloud writes the device-side count, a cloud's base is the sum of the counts in front of it), channels whose gradient is
+0.0 / -0.0 and whose arg-max rows must stay dead, and no live row at all.  `gp[c, j] = y2[idx[c, j]] . w3[j] + b3[j]`,
so every table is a legal forward result; behind a pooled ReLU b3 is chosen so that the ReLU passes (or, for the
`dead_channels` / `zero` patterns, kills) exactly the channels the pattern wants - the crafted count survives the ReLU.

Reference: fp64 autograd of the same three layers with the pool written as a gather at `idx`.  Its activations are the
rows the kernel under test is handed (fp32 rows, bf16 rows, or the rows the recompute kernel rebuilds): the ReLU masks and
the weight-gradient operands are taken from them, so a pre-activation within rounding of zero cannot flip a mask between
the reference and the kernel.  Bars (max abs error over the fp64 tensor's max abs, per gradient tensor) are those of
`test_pooled_chain_row_sparse_backward_matches_fp64_reference`; next to them the worst value measured on an MI355X over
every case of this file:

    fp32   2e-4   (saved rows 1.1e-6;  recompute 1.5e-6;  pointfeat hub 9.9e-7)
    split  1e-3   (1.4e-5)
    bf16   4e-2   (fp32 saved rows 5.7e-3;  bf16 saved rows 5.2e-3)

Shapes (B, N, M): (2, 64, 64) - R = 256 holds every count=k, sixteen workgroups per cloud in the row walk; (3, 128, 64)
unequal clouds; (2, 192, 0) one cloud per object; (40, 64, 64) 5120 rows of capacity around 65 live ones; (1, 4096, 64)
the largest cloud the kernels take; (352, 64, 64) / (512, 64, 64) two / one workgroup per cloud in the row walk (STN
widths only; the fp64 pool is evaluated as row gathers there).
"""
import collections
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
J3 = 1024
TOL = {"fp32": 2e-4, "split": 1e-3, "bf16": 4e-2}
ERR_UNSUPPORTED = -4  # CATRE_ERR_UNSUPPORTED

TRUNK = ("trunk", 64, 128, 512, False)   # pointfeat -> conv2 -> conv3 -> conv4 + max
FSTN = ("fstn", 64, 64, 128, True)       # h1 -> conv1 -> conv2 -> conv3 + max + ReLU
STN = ("stn", 3, 64, 128, True)          # points (no input gradient) -> ...

COUNTS = (1, 63, 64, 65, 127, 128, 129)
PATTERNS = (("one_row",) + tuple(f"count={k}" for k in COUNTS)
            + ("all_live", "empty_first", "empty_last", "empty_middle", "dead_channels", "zero"))
SMALL = ((2, 64, 64), (3, 128, 64), (2, 192, 0))
# (shape, pattern) pairs at every width ...
CASES = ([(s, p) for s in SMALL for p in PATTERNS]
         + [((40, 64, 64), "count=65"), ((1, 4096, 64), "one_row"), ((1, 4096, 64), "count=129:tail")])
# ... and at the STN widths only
BIG = [(s, p) for s in ((352, 64, 64), (512, 64, 64)) for p in PATTERNS]
BF16_ROW_CASES = [(s, p) for s in ((2, 64, 64), (3, 128, 64)) for p in ("one_row", "count=65", "dead_channels", "zero", "all_live")]
HUB_CASES = [(s, p) for s in ((2, 64, 64), (3, 128, 64)) for p in ("one_row", "count=65", "empty_middle", "all_live")]


def _id(case):
    (B, N, M), p = case
    return f"{B}x{N}x{M}-{p}"


def _seed(shape, pattern):
    B, N, M = shape
    return 1000 * B + 7 * N + 3 * M + sum(ord(ch) for ch in pattern)


# ------------------------------------------------------------------------------------------------- crafted tables
def cloud_ranges(B, N, M):
    """-> (r0 [C], n [C]): first row and point count of each cloud, rows cloud-major (B observed clouds, then B priors)."""
    C = 2 * B if M > 0 else B
    r0 = np.array([c * N if c < B else B * N + (c - B) * M for c in range(C)], dtype=np.int64)
    n = np.array([N if c < B else M for c in range(C)], dtype=np.int64)
    return r0, n


def live_rows(idx, dG):
    """The expected live-row list: ascending unique idx[c, j] over the entries with dG[c, j] != 0 (-0.0 is a zero)."""
    return np.unique(idx[dG != 0]).astype(np.int32)


Table = collections.namedtuple("Table", "idx dG live per_cloud")


def _count_of(pattern):
    """"count=129" / "count=129:tail" -> (129, tail?); any other pattern -> (None, False)."""
    if not pattern.startswith("count="):
        return None, False
    k, _, place = pattern[len("count="):].partition(":")
    return int(k), place == "tail"


def make_idx(B, N, M, J3, pattern, seed):
    """-> Table(idx [C, J3] int32, dG [C, J3] float32, live: the expected ascending live-row list, per_cloud: the local
    rows each cloud was MEANT to get - what the host test holds `live` against)."""
    rng = np.random.default_rng(seed)
    r0, n = cloud_ranges(B, N, M)
    C = len(n)
    dG = rng.standard_normal((C, J3)).astype(np.float32)
    dG[dG == 0] = 1.0
    idx = np.empty((C, J3), dtype=np.int32)
    want = [np.zeros(0, dtype=np.int64) for _ in range(C)]   # per cloud: local live rows, ascending

    def pick(c, m):
        return np.sort(rng.choice(n[c], size=m, replace=False))

    if pattern == "one_row":
        want = [np.array([n[c] - 1]) for c in range(C)]
    elif pattern.startswith("count="):
        k, tail = _count_of(pattern)
        if tail:                          # all k on the last rows of the largest cloud
            c = int(np.argmax(n))
            assert k <= n[c]
            want[c] = np.arange(n[c] - k, n[c])
        elif k < C:                       # one row each in k clouds spread over all of them
            for i in range(k):
                c = (i * C) // k
                want[c] = pick(c, 1)
        else:
            quota = np.array([k // C + (c < k % C) for c in range(C)])
            over = int(np.maximum(quota - n, 0).sum())
            quota = np.minimum(quota, n)
            for c in range(C):            # what did not fit goes to the clouds that still have room
                add = min(over, int(n[c] - quota[c]))
                quota[c] += add
                over -= add
            assert over == 0, "more live rows asked for than the shape has rows"
            want = [pick(c, int(quota[c])) for c in range(C)]
    elif pattern == "all_live":
        assert n.max() <= J3, "all_live needs a channel for every row of a cloud"
        want = [np.arange(n[c]) for c in range(C)]
    elif pattern in ("empty_first", "empty_last", "empty_middle"):
        ne = max(1, C // 4)
        lo = {"empty_first": 0, "empty_last": C - ne, "empty_middle": C // 2 - ne // 2}[pattern]
        for c in range(C):
            if not lo <= c < lo + ne:
                want[c] = pick(c, int(rng.integers(1, min(n[c], 40) + 1)))
    elif pattern == "dead_channels":
        want = [pick(c, int(rng.integers(1, min(n[c] // 2, 40) + 1))) for c in range(C)]
    elif pattern != "zero":
        raise ValueError(pattern)

    dead = np.arange(J3) % 3 == 0 if pattern == "dead_channels" else np.zeros(J3, dtype=bool)
    for c in range(C):
        rows = want[c]
        if pattern == "zero" or len(rows) == 0:     # no live row: zero gradient, the table still points inside the cloud
            dG[c] = 0.0
            idx[c] = r0[c] + rng.integers(0, n[c], size=J3)
            continue
        ch = np.flatnonzero(~dead)
        assert len(rows) <= len(ch)
        # the live channels cycle over the cloud's live rows (in a shuffled channel order: buckets are not contiguous runs)
        idx[c, ch[rng.permutation(len(ch))]] = r0[c] + rows[np.arange(len(ch)) % len(rows)]
        if dead.any():                              # zeroed channels point at rows no live channel uses
            other = np.setdiff1d(np.arange(n[c]), rows)
            other = other[rng.permutation(len(other))[:20]]
            dch = np.flatnonzero(dead)
            idx[c, dch] = r0[c] + other[np.arange(len(dch)) % len(other)]
            dG[c, dch[0::2]] = 0.0
            dG[c, dch[1::2]] = -0.0
    return Table(idx, dG, live_rows(idx, dG), want)


def _intended_count(shape, pattern):
    B, N, M = shape
    C, R = (2 * B if M > 0 else B), B * (N + M)
    if pattern == "one_row":
        return C
    if pattern.startswith("count="):
        return _count_of(pattern)[0]
    return {"all_live": R, "zero": 0}.get(pattern)   # None: the pattern draws its count


@functools.lru_cache(maxsize=4)
def _table(shape, pattern):
    return make_idx(*shape, J3, pattern, _seed(shape, pattern))


# ------------------------------------------------------------------------------------------------- A. host
@pytest.mark.parametrize("case", CASES + BIG, ids=_id)
def test_builder_delivers_the_intended_live_rows(case):
    """Every (shape, pattern) pair the device tests use (CASES + BIG; the bf16-row and hub lists are subsets, checked below)
    is feasible: the table stays inside its clouds and its live list is exactly the one the pattern names."""
    shape, pattern = case
    B, N, M = shape
    t = _table(shape, pattern)
    r0, n = cloud_ranges(B, N, M)
    C = len(n)
    assert t.idx.shape == t.dG.shape == (C, J3) and t.idx.dtype == np.int32 and t.dG.dtype == np.float32
    assert ((t.idx >= r0[:, None]) & (t.idx < (r0 + n)[:, None])).all()
    meant = np.concatenate([r0[c] + t.per_cloud[c] for c in range(C)]).astype(np.int32)
    assert np.array_equal(t.live, meant) and np.all(np.diff(t.live) > 0)
    k = _intended_count(shape, pattern)
    assert k is None or len(t.live) == k
    per = np.array([len(w) for w in t.per_cloud])
    if pattern == "one_row":
        assert np.array_equal(t.live, (r0 + n - 1).astype(np.int32))
    if _count_of(pattern)[1]:
        c = int(np.argmax(n))
        assert np.array_equal(t.live, np.arange(r0[c] + n[c] - k, r0[c] + n[c]))
    if pattern.startswith("empty_"):
        ne = max(1, C // 4)
        lo = {"empty_first": 0, "empty_last": C - ne, "empty_middle": C // 2 - ne // 2}[pattern]
        empty = np.zeros(C, dtype=bool)
        empty[lo: lo + ne] = True
        assert np.array_equal(per == 0, empty) and len(t.live) > 0
    for c in np.flatnonzero(per == 0):   # clouds without a live row: the whole gradient row is zero
        assert not t.dG[c].any()
    if pattern == "dead_channels":
        z = t.dG[:, 0::3]
        assert not z.any() and np.signbit(z).any() and not np.signbit(z).all()
        assert t.dG[:, np.arange(J3) % 3 != 0].all()
        assert len(np.intersect1d(np.unique(t.idx[:, 0::3]), t.live)) == 0
    if pattern == "zero":
        assert not t.dG.any()


def test_case_lists_and_the_largest_cloud():
    """The bf16-row and hub pairs are among CASES; N = 4160 is past the largest cloud the row-sparse chain takes."""
    from catre_amd import train_ops as T

    assert set(BF16_ROW_CASES) <= set(CASES) and set(HUB_CASES) <= set(CASES)
    x = torch.zeros(1, 64, requires_grad=True)
    w1, w2, w3 = torch.zeros(128, 64, 1), torch.zeros(512, 128, 1), torch.zeros(1024, 512, 1)
    assert T.pooled_chain_ok(x, w1, w2, w3, 4096, 64)
    assert not T.pooled_chain_ok(x, w1, w2, w3, 4160, 64) and not T.pooled_chain_ok(x, w1, w2, w3, 64, 4160)


# ------------------------------------------------------------------------------------------------- B. the live-row list
def _poison():
    """NaN into the caching allocator's free blocks, large and small, so that the `torch.empty` buffers of the code under
    test start out poisoned: what it never writes and still reads shows."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # ~570 MB in the large-block pool, in several sizes (a best-fit search then finds a poisoned block for a request of any
    # size, whether or not the allocator is set up to split large blocks), and 2 MB blocks' worth of small ones
    big = [torch.full((mb << 18,), float("nan"), device=DEV) for mb in (2, 8, 20, 32, 64, 64, 128, 256)]
    small = [torch.full((n,), float("nan"), device=DEV) for n in (1 << 17, 1 << 15, 1 << 12) for _ in range(48)]
    torch.cuda.synchronize()
    del big, small


def _dev_table(t):
    return torch.from_numpy(t.idx).to(DEV), torch.from_numpy(t.dG).to(DEV)


def _check_compaction(rows, rowpos, count, live, R):
    n = int(count.item())
    assert n == len(live), (n, len(live))
    assert np.array_equal(rows[:n].cpu().numpy(), live)
    want = np.full(R, -1, dtype=np.int32)
    want[live] = np.arange(len(live), dtype=np.int32)
    assert np.array_equal(rowpos.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + BIG, ids=_id)
def test_rows_compact_is_exact(case):
    from catre_amd import train_ops as T

    (B, N, M), pattern = case
    t = _table(*case)
    idx, dG = _dev_table(t)
    _poison()
    rows, rowpos, count = T._rows_compact(dG, idx, B, N, M)
    _check_compaction(rows, rowpos, count, t.live, B * (N + M))


@pytest.mark.gpu
def test_rows_compact_refuses_a_cloud_past_the_largest():
    from catre_amd import hip

    lib = hip.load()
    B, N, M = 1, 4160, 64
    i32 = dict(dtype=torch.int32, device=DEV)
    dG, idx = torch.zeros(2, J3, device=DEV), torch.zeros(2, J3, **i32)
    rows, rowpos, count, scratch = torch.zeros(N + M, **i32), torch.zeros(N + M, **i32), torch.zeros(1, **i32), torch.zeros(4, **i32)
    for (n, m) in ((N, M), (M, N)):
        r = lib.catre_op_rows_compact(hip.ptr(dG), hip.ptr(idx), J3, B, n, m, hip.ptr(rows), hip.ptr(rowpos), hip.ptr(count),
                                      hip.ptr(scratch), hip.stream_ptr(dG.device))
        assert r == ERR_UNSUPPORTED, r


# ------------------------------------------------------------------------------------------------- chains
def _stn_rows(kind, x, w1, b1, w2, b2):
    """y1 [R, 64], y2 [R, 128] of an STN stack for EVERY row by the recompute kernel itself (row list = all rows): the rows
    the forward kernels would have saved - same device code, same bits."""
    from catre_amd import hip

    lib = hip.load()
    R = x.shape[0]
    st = hip.stream_ptr(x.device)
    w1m, w2m = w1.reshape(w1.shape[0], -1).contiguous(), w2.reshape(w2.shape[0], -1).contiguous()
    assert w1m.shape[0] == 64 and w2m.shape == (128, 64) and R % 64 == 0
    rows = torch.arange(R, dtype=torch.int32, device=x.device)
    count = torch.full((1,), R, dtype=torch.int32, device=x.device)
    wp2 = torch.empty(w2m.numel(), dtype=torch.float32, device=x.device)
    hip.check(lib.catre_op_pack(hip.ptr(w2m), w2m.stride(0), 128, 64, 0, hip.ptr(wp2), st), "catre_op_pack")
    wp1 = None
    if kind == 1:
        wp1 = torch.empty(w1m.numel(), dtype=torch.float32, device=x.device)
        hip.check(lib.catre_op_pack(hip.ptr(w1m), w1m.stride(0), 64, 64, 0, hip.ptr(wp1), st), "catre_op_pack")
    y1 = torch.empty(R, 64, dtype=torch.float32, device=x.device)
    y2 = torch.empty(R, 128, dtype=torch.float32, device=x.device)
    hip.check(lib.catre_op_stn_recompute(kind, hip.ptr(x), x.stride(0), hip.ptr(rows), hip.ptr(count),
                                         hip.ptr(w1m) if kind == 0 else None, hip.ptr(wp1), hip.ptr(b1), hip.ptr(wp2), hip.ptr(b2),
                                         hip.ptr(y1), hip.ptr(y2), R, st), "catre_op_stn_recompute")
    return y1, y2


def _pool_pre_bias(y2, w3, idx):
    """p[c, j] = y2[idx[c, j]] . w3[j] in fp64 as row gathers, a few clouds at a time (never the dense [R, J3] product)."""
    C = idx.shape[0]
    step = max(1, (1 << 23) // (idx.shape[1] * y2.shape[1]))
    return torch.cat([(y2[idx[c: c + step].long()] * w3[None]).sum(-1) for c in range(0, C, step)], 0)


Problem = collections.namedtuple("Problem", "shape widths x params y1 y2 gp idx dG live ref")


def _problem(shape, pattern, widths, rows_kind, hub=None):
    """Inputs of one case (CPU), the rows the backward is handed and the fp64 reference gradients.
    rows_kind: "fp32" (layer-wise HIP ops), "bf16" (those, rounded as the autocast forward saves them), "stn" (the recompute
    kernel's own rows).  hub = (Gmax [C, K0] or None, Gobj [R, K0] or None): pointfeat's two other consumers."""
    from catre_amd import train_ops as T

    B, N, M = shape
    name, K0, J1, J2, relu_pool = widths
    R = B * (N + M)
    t = _table(shape, pattern)
    g = torch.Generator().manual_seed(_seed(shape, pattern) + K0 + J2)
    x = torch.randn(R, K0, generator=g)
    w1, w2, w3 = (torch.randn(j, k, 1, generator=g) / k ** 0.5 for (j, k) in ((J1, K0), (J2, J1), (J3, J2)))
    b1, b2, b3 = (0.1 * torch.randn(j, generator=g) for j in (J1, J2, J3))
    idx, dG = torch.from_numpy(t.idx), torch.from_numpy(t.dG).clone()
    with torch.no_grad(), T.amp_mode("fp32"):
        if rows_kind == "stn":
            y1, y2 = _stn_rows(0 if K0 == 3 else 1, x.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV))
            # the reference below takes these rows as its activations, so their VALUES get an fp64 check of their own:
            # fp32 sums of 3 / 64 / 64 products of O(1) data, two layers deep - 1e-5 of the tensor's largest entry
            y1r = F.relu(F.linear(x.double(), w1[:, :, 0].double(), b1.double()))
            y2r = F.relu(F.linear(y1r, w2[:, :, 0].double(), b2.double()))
            for got, want in ((y1, y1r), (y2, y2r)):
                assert float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
        else:
            y1 = T.linear(x.to(DEV), w1.to(DEV), b1.to(DEV), relu=True)
            if rows_kind == "bf16":
                y1 = y1.bfloat16()
            y2 = T.linear(y1.float(), w2.to(DEV), b2.to(DEV), relu=True)
            if rows_kind == "bf16":
                y2 = y2.bfloat16()
        y1, y2 = y1.cpu(), y2.cpu()
    p = _pool_pre_bias(y2.double(), w3[:, :, 0].double(), idx)
    if relu_pool:
        # the pooled ReLU passes every channel (min over the clouds of gp = 0.5) ...
        b3 = (0.5 - p.min(0)[0]).float()
        kill = torch.zeros(J3, dtype=torch.bool)
        if pattern == "dead_channels":   # ... but every second dead channel is dead BEHIND THE RELU, with a gradient arriving
            kill[3::6] = True
            dG[:, 3::6] = torch.randn(dG.shape[0], len(range(3, J3, 6)), generator=g)
        if pattern == "zero":            # ... and `zero` has gradient arriving at every second cloud, all of it killed
            kill[:] = True
            dG[1::2] = torch.randn(dG[1::2].shape, generator=g)
        b3[kill] = (-0.5 - p.max(0)[0]).float()[kill]
    gp = (p + b3.double()).float()
    geff = torch.where(gp > 0, dG, torch.zeros(())) if relu_pool else dG
    live = live_rows(t.idx, geff.numpy())
    assert np.array_equal(live, t.live)   # the ReLU changed nothing about the crafted list
    ref = _reference(x, (w1, b1, w2, b2, w3, b3), y1, y2, idx, geff, shape, hub)
    return Problem(shape, widths, x, (w1, b1, w2, b2, w3, b3), y1, y2, gp, idx, dG, live, ref)


def _reference(x, params, y1s, y2s, idx, geff, shape, hub):
    """fp64 autograd: x -> relu(conv1) -> relu(conv2) -> conv3 -> gather at idx, upstream gradient geff (the pooled ReLU
    already applied to it).  Values and ReLU masks of y1 / y2 are the saved rows'."""
    B, N, M = shape
    xr = x.double().requires_grad_(True)
    w1, b1, w2, b2, w3, b3 = (q.double().requires_grad_(True) for q in params)

    def layer(inp, w, b, saved):
        z = F.linear(inp, w[:, :, 0], b) * (saved > 0).double()   # == relu(.) wherever the masks agree, which is the premise
        return saved.double() + (z - z.detach())

    y2 = layer(layer(xr, w1, b1, y1s), w2, b2, y2s)
    ge = geff.double()
    if y2.shape[0] <= 1024:
        loss = (F.linear(y2, w3[:, :, 0], b3).gather(0, idx.long()) * ge).sum()
        if hub is not None:
            gmax, gobj = hub
            if gmax is not None:
                pm = torch.cat([xr[: B * N].view(B, N, -1).max(1)[0], xr[B * N:].view(B, M, -1).max(1)[0]], 0)
                loss = loss + (pm * gmax.double()).sum()
            if gobj is not None:
                po = torch.cat([xr[: B * N].view(B, N, -1), xr[B * N:].view(B, M, -1)], 1).reshape(B * (N + M), -1)
                loss = loss + (po * gobj.double()).sum()
        loss.backward()
    else:   # the pool as row gathers, a few clouds at a time; then the two thin layers
        assert hub is None
        y2d = y2.detach().requires_grad_(True)
        step = max(1, (1 << 23) // (J3 * y2.shape[1]))
        for c in range(0, idx.shape[0], step):
            pre = (y2d[idx[c: c + step].long()] * w3[None, :, :, 0]).sum(-1) + b3
            (pre * ge[c: c + step]).sum().backward()
        y2.backward(y2d.grad)
    out = {k: q.grad for k, q in zip(("w1", "b1", "w2", "b2", "w3", "b3"), (w1, b1, w2, b2, w3, b3))}
    out["x"] = xr.grad
    return out


def _run(pb, mode, rows="saved", hub=None, obj_copy=True):
    """One forward + backward of the node under test -> {name: gradient} (device tensors)."""
    from catre_amd import train_ops as T

    B, N, M = pb.shape
    relu_pool = pb.widths[4]
    x = pb.x.to(DEV).requires_grad_(pb.x.shape[1] != 3)   # the STN's input points carry no gradient
    ps = [q.to(DEV).requires_grad_(True) for q in pb.params]
    pre = ((pb.y1.to(DEV), pb.y2.to(DEV)) if rows == "saved" else (None, None)) + (pb.gp.to(DEV), pb.idx.to(DEV))
    dG = pb.dG.to(DEV)
    with T.amp_mode(mode):
        assert T.pooled_chain_ok(x, ps[0], ps[2], ps[4], N, M)
        if hub is None:
            out = T.pooled_chain(x, *ps, relu_pool, B, N, M, pre)
            assert torch.equal(out, torch.relu(pre[2]) if relu_pool else pre[2])
            out.backward(dG)
        else:
            gmax, gobj = hub
            out, pfmax, pfobj = T.pointfeat_hub(x, *ps, B, N, M, pre, obj_copy=obj_copy)
            outs, grads = [out], [dG]
            if gmax is not None:
                outs.append(pfmax)
                grads.append(gmax.to(DEV))
            if gobj is not None:
                outs.append(pfobj)
                grads.append(gobj.to(DEV))
            torch.autograd.backward(outs, grads)
    got = {k: q.grad for k, q in zip(("w1", "b1", "w2", "b2", "w3", "b3"), ps)}
    if x.requires_grad:
        got["x"] = x.grad
    else:
        assert x.grad is None
    return got


def _check(pb, got, tol, what, dead_rows_exact=True):
    """Every gradient against the fp64 reference at `tol`; exact zeros where the live-row list says so.  -> worst error."""
    worst = (0.0, "-")
    for k, gt in got.items():
        want = pb.ref[k]
        assert gt.shape == want.shape and gt.dtype == torch.float32, k
        scale = float(want.abs().max())
        err = float((gt.cpu().double() - want).abs().max()) / max(scale, 1e-30)
        worst = max(worst, (err, k)) if err == err else (err, k)
        assert err <= tol, (what, k, err)
    R = pb.x.shape[0]
    if "x" in got and dead_rows_exact:
        dead = np.ones(R, dtype=bool)
        dead[pb.live] = False
        if dead.any():
            dx = got["x"][torch.from_numpy(dead).to(DEV)]
            assert float(dx.abs().max()) == 0.0, (what, "rows outside the live list")
    if len(pb.live) == 0 and dead_rows_exact:
        for k, gt in got.items():
            assert bool(torch.isfinite(gt).all()) and float(gt.abs().max()) == 0.0, (what, k, "no live row: exact zeros")
    return worst


def _same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


def _chain_case(case, widths, rows_kind, modes):
    shape, pattern = case
    pb = _problem(shape, pattern, widths, rows_kind)
    for mode in modes:
        if pattern == "zero":
            _poison()
        got = _run(pb, mode)
        err, k = _check(pb, got, TOL[mode], mode)
        print(f"{_id(case)} {widths[0]} rows={rows_kind} {mode}: worst {err:.2e} ({k}), {len(pb.live)} live rows")
        _same_bits(got, _run(pb, mode), mode + ": second run")


# ------------------------------------------------------------------------------------------------- C. saved fp32 rows
@pytest.mark.gpu
@pytest.mark.parametrize("widths", [TRUNK, FSTN], ids=lambda w: w[0])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_saved_rows_chain_matches_fp64_at_crafted_counts(case, widths):
    _chain_case(case, widths, "fp32", ("fp32", "split", "bf16"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", BIG, ids=_id)
def test_saved_rows_chain_matches_fp64_with_few_workgroups_per_cloud(case):
    _chain_case(case, FSTN, "fp32", ("fp32", "split", "bf16"))


# ------------------------------------------------------------------------------------------------- D. saved bf16 rows
@pytest.mark.gpu
@pytest.mark.parametrize("widths", [TRUNK, FSTN], ids=lambda w: w[0])
@pytest.mark.parametrize("case", BF16_ROW_CASES, ids=_id)
def test_bf16_saved_rows_chain_matches_fp64_of_the_rounded_rows(case, widths):
    """y1 / y2 as the bf16 rows the autocast forward saves: `catre_op_maxlin_bwd_w_h`, `catre_op_maxlin_bwd_x_compact_h` and
    the CATRE_ROWS_BF16 flag of the device-count GEMMs.  The reference's masks and weight-gradient operands are those rows."""
    _chain_case(case, widths, "bf16", ("bf16",))


# ------------------------------------------------------------------------------------------------- E. recompute
def _recompute_case(case, widths):
    shape, pattern = case
    pb = _problem(shape, pattern, widths, "stn")
    saved = _run(pb, "fp32")
    _check(pb, saved, TOL["fp32"], "saved rows")
    if pattern == "zero":
        _poison()
    got = _run(pb, "fp32", rows="recompute")
    err, k = _check(pb, got, TOL["fp32"], "recompute")
    print(f"{_id(case)} {widths[0]} recompute fp32: worst {err:.2e} ({k}), {len(pb.live)} live rows")
    _same_bits(got, saved, "recompute vs saved rows")
    _same_bits(got, _run(pb, "fp32", rows="recompute"), "recompute: second run")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + BIG, ids=_id)
def test_recompute_chain_stn3d_matches_fp64_and_the_saved_rows_bits(case):
    """`pre = (None, None, gp, idx)`, K0 = 3: rows rebuilt by `catre_op_stn_recompute`, compact operands in
    `catre_op_maxlin_bwd_w_c` / `_x_compact_cm` and the masked row GEMM.  `zero` runs on a poisoned allocator: compact row 0
    is never written when no row is live, and nothing may be read from it."""
    _recompute_case(case, STN)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES + BIG if c[0][1] != 4096], ids=_id)
def test_recompute_chain_stnkd_matches_fp64_and_the_saved_rows_bits(case):
    _recompute_case(case, FSTN)


# ------------------------------------------------------------------------------------------------- F. pointfeat hub
@pytest.mark.gpu
@pytest.mark.parametrize("obj_copy", [True, False], ids=["copy", "nocopy"])
@pytest.mark.parametrize("case", HUB_CASES, ids=_id)
def test_pointfeat_hub_sums_three_gradients_at_crafted_counts(case, obj_copy):
    """Chain + max over points + the object-major copy as one node: all three gradients, then without the one of the max,
    without the one of the copy, and with the chain's alone (rows outside the live list exactly zero)."""
    shape, pattern = case
    B, N, M = shape
    C, R = (2 * B if M > 0 else B), B * (N + M)
    g = torch.Generator().manual_seed(11 + _seed(shape, pattern))
    gmax, gobj = torch.randn(C, 64, generator=g), torch.randn(R, 64, generator=g)
    for hub in ((gmax, gobj), (None, gobj), (gmax, None), (None, None)):
        pb = _problem(shape, pattern, TRUNK, "fp32", hub=hub)
        got = _run(pb, "fp32", hub=hub, obj_copy=obj_copy)
        which = "+".join(n for n, q in zip(("dmax", "dobj"), hub) if q is not None) or "chain only"
        err, k = _check(pb, got, TOL["fp32"], which, dead_rows_exact=hub == (None, None))
        print(f"{_id(case)} hub {which} fp32: worst {err:.2e} ({k}), {len(pb.live)} live rows")
        _same_bits(got, _run(pb, "fp32", hub=hub, obj_copy=obj_copy), which + ": second run")
