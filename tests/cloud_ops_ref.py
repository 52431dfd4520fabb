"""fp64 references and case generators for the small training ops on point-cloud rows (csrc/catre_train.h: the per-cloud
transforms, the plain max-pool, the per-cloud bias, conv_p's weighted point sum and the column sums).

Plain numpy, no autograd: one function per op and per gradient, written from the op's definition.  tests/
test_cloud_ops_host.py checks every one of them against torch fp64 autograd on the CPU and asserts what the cases below
promise; tests/test_cloud_ops_edges.py compares the HIP kernels with them.

Two row layouts, as in catre_amd/train_ops.py:
  cloud-major   B*N observed rows, then B*M prior rows           (`cloud_slices`)
  object-major  [N observed | M prior] rows per object           (`object_slices`)
Either way cloud c < B is the observed cloud of object c, cloud B + o the prior cloud of object o, and M = 0 leaves B clouds.

Every bilinear reference gives, when it is handed the absolute values of its operands, the sum of the absolute values of the
terms behind each output: that is the `abs_sum` of `bound`.
"""
import zlib

import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32
EXACT_LIMIT = 2 ** 24   # integers of magnitude up to here are exact in fp32, and so is any sum that stays below

# ------------------------------------------------------------------------------------------------- the cases
# (B, N, M) of the cloud layout: M = 0, one-row clouds, the 64-row tile of k_cloud_matmul* on both sides, the 32-row slab of
# k_cloud_matmul_bwd_t, the 28 / 29 / 32 / 33 edges of the eight-in-flight loops, a cloud shorter than one lane set
CLOUD_SHAPES = ((1, 1, 0), (1, 1, 1), (2, 129, 1), (3, 64, 64), (2, 63, 65), (5, 33, 31), (2, 130, 45), (4, 2, 300), (7, 29, 4),
                (1, 32, 28))
# kd = 64 routes: (B, N, M) -> the tiles per workgroup the launch takes
ROUTE_SHAPES = {(256, 500, 130): 4, (1024, 200, 0): 4, (255, 500, 130): 1}
FALLBACK_SHAPE = (2, 63, 65)           # the ld % 4 != 0 kernels, run with ldx = 66, ldy = 65
FALLBACK_LDX, FALLBACK_LDY = 66, 65
POOL_J = (8, 64, 100, 1024)            # a column block narrower than, equal to and ragged against 64
TIE_N = (1, 3, 4, 5, 33, 65, 130)
# every n of TIE_N once as N and once as M
TIE_SHAPES = tuple((2, n, TIE_N[(i + 1) % len(TIE_N)]) for i, n in enumerate(TIE_N))
BIAS_J = (4, 68, 256)
WSUM_B = (1, 15, 16, 17, 49, 64, 65, 113)      # k_reduce_splits_wide: splits on both sides of 16 and of k + 48 < splits
WSUM_P = (1, 3, 63, 64, 255, 256, 257, 576)
COLSUM_R = (1, 7, 64, 65, 4097, 70001)
COLSUM_J = (1, 3, 100, 256, 257, 1280)
AMP = 8                                         # exact cases: integers in [-AMP, AMP]


def colsum_amp(R):
    """Integers in [-4, 4] for the longest column sum, so that R * amp stays below 2^24."""
    return 4 if R > 65536 else AMP


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def exact(shape, *key, amp=AMP):
    """Pseudo-random integers in [-amp, amp] as fp32: products and sums of them are exact in fp32 in any order (as long as
    they stay below 2^24 - `worst_abs_sum`)."""
    rng = np.random.default_rng(seed_of("exact", *key))
    return rng.integers(-amp, amp + 1, size=shape, dtype=np.int8).astype(np.float32)


def rounded(shape, *key):
    """N(0, 1) as fp32."""
    rng = np.random.default_rng(seed_of("rounded", *key))
    return rng.standard_normal(size=shape, dtype=np.float32)


def operand(kind, shape, *key, amp=AMP):
    return exact(shape, *key, amp=amp) if kind == "exact" else rounded(shape, *key)


def nonzero(shape, *key):
    """Integers of magnitude 1 .. 8, either sign: an upstream gradient whose scatter shows every arg-max row."""
    rng = np.random.default_rng(seed_of("nonzero", *key))
    return (rng.integers(1, AMP + 1, size=shape) * rng.choice((-1, 1), size=shape)).astype(np.float32)


def bound(n, abs_sum):
    """|err| of an fp32 sum of n products or terms against the exact result: n * 2^-24 * sum|terms| to first order for any
    order of the additions (n - 1 additions and one rounding per product); the factor 2 covers the order and the matrix
    pipe's own rounding of its products."""
    return 2.0 * np.asarray(n, dtype=np.float64) * U * np.asarray(abs_sum, dtype=np.float64)


# ------------------------------------------------------------------------------------------------- layouts
def n_clouds(B, M):
    return 2 * B if M > 0 else B


def cloud_slices(B, N, M):
    """(first row, rows) of every cloud, rows cloud-major."""
    return [(c * N, N) if c < B else (B * N + (c - B) * M, M) for c in range(n_clouds(B, M))]


def object_slices(B, N, M):
    """(first row, rows) of every cloud, rows object-major."""
    return [(c * (N + M), N) if c < B else ((c - B) * (N + M) + N, M) for c in range(n_clouds(B, M))]


def cloud_rows(B, N, M):
    """Rows of every cloud [C] (the `n` of a per-cloud sum)."""
    return np.array([n for _, n in cloud_slices(B, N, M)], dtype=np.float64)


def _f64(*a):
    return [np.asarray(x, dtype=np.float64) for x in a]


# ------------------------------------------------------------------------------------------------- per-cloud transforms
def cloud_matmul(X, T, B, N, M):
    """Y[r] = X[r, :kd] @ T[cloud(r)] -> [R, kd]; X cloud-major [R, >= kd], T [C, kd, kd]."""
    X, T = _f64(X, T)
    kd = T.shape[-1]
    Y = np.empty((X.shape[0], kd))
    for c, (r0, n) in enumerate(cloud_slices(B, N, M)):
        Y[r0:r0 + n] = X[r0:r0 + n, :kd] @ T[c]
    return Y


def cloud_matmul_dx(dY, T, B, N, M):
    """dX[r] = dY[r, :kd] @ T[cloud(r)]^T -> [R, kd]."""
    return cloud_matmul(dY, np.swapaxes(np.asarray(T), 1, 2), B, N, M)


def cloud_matmul_dT(X, dY, B, N, M, kd):
    """dT[c] = X_c[:, :kd]^T dY_c[:, :kd] -> [C, kd, kd]."""
    X, dY = _f64(X, dY)
    return np.stack([X[r0:r0 + n, :kd].T @ dY[r0:r0 + n, :kd] for r0, n in cloud_slices(B, N, M)])


# ------------------------------------------------------------------------------------------------- max-pool
def maxpool(Y, B, N, M):
    """(max [C, J], row of the FIRST maximum [C, J], as a row of Y) over the rows of each cloud, rows cloud-major.
    np.argmax: "In case of multiple occurrences of the maximum values, the indices corresponding to the first occurrence are
    returned."  A column of -inf gives (-inf, the cloud's row 0).  (No NaN here: np.argmax stops at one, the kernel skips it.)"""
    Y = np.asarray(Y)
    assert not np.isnan(Y).any()
    val, idx = [], []
    for r0, n in cloud_slices(B, N, M):
        a = np.argmax(Y[r0:r0 + n], axis=0)
        idx.append(r0 + a)
        val.append(Y[r0 + a, np.arange(Y.shape[1])])
    return np.stack(val), np.stack(idx).astype(np.int64)


def maxpool_bwd(dout, idx, R):
    """dY [R, J]: dout[c, j] at row idx[c, j] of column j, zero elsewhere (a tie sends everything to the first row)."""
    dout = np.asarray(dout, dtype=np.float64)
    dY = np.zeros((R, dout.shape[1]))
    for c in range(dout.shape[0]):
        dY[idx[c], np.arange(dout.shape[1])] = dout[c]
    return dY


# ------------------------------------------------------------------------------------------------- per-cloud bias
def rowbias_add(Y, bias, B, N, M, dtype=np.float64):
    """Y[r] + bias[cloud(r)], rows object-major; dtype=np.float32 gives the fp32 sum the kernel must equal bit for bit."""
    out = np.array(Y, dtype=dtype)
    bias = np.asarray(bias, dtype=dtype)
    for c, (r0, n) in enumerate(object_slices(B, N, M)):
        out[r0:r0 + n] += bias[c]
    return out


def rowbias_bwd(dY, B, N, M):
    """dbias[c] = sum of the rows of cloud c, rows object-major -> [C, J]."""
    (dY,) = _f64(dY)
    return np.stack([dY[r0:r0 + n].sum(0) for r0, n in object_slices(B, N, M)])


# ------------------------------------------------------------------------------------------------- conv_p
def wsum(Y, w, bias, B, P):
    """out[b] = sum_p w[p] Y[b P + p] + bias -> [B, 3]; Y [B*P, 3], w [P], bias a scalar or None."""
    Y, w = _f64(Y, w)
    out = np.einsum("p,bpc->bc", w.reshape(-1), Y.reshape(B, P, 3))
    return out if bias is None else out + float(np.asarray(bias, dtype=np.float64).reshape(-1)[0])


def wsum_dY(dout, w, B, P):
    """dY[b P + p, c] = w[p] dout[b, c] -> [B*P, 3]."""
    dout, w = _f64(dout, w)
    return (w.reshape(1, P, 1) * dout.reshape(B, 1, 3)).reshape(B * P, 3)


def wsum_dw(dout, Y, B, P):
    """dw[p] = sum_b sum_c dout[b, c] Y[b P + p, c] -> [P] (3 B products each)."""
    dout, Y = _f64(dout, Y)
    return np.einsum("bc,bpc->p", dout, Y.reshape(B, P, 3))


def wsum_dbias(dout):
    """dbias = sum of dout (3 B terms)."""
    return _f64(dout)[0].sum()


def wsum_dbn(dout, w):
    """The bias gradient of the neck in front of conv_p, the column sums of dY, factored: (sum_p w_p)(sum_b dout_b) -> [3]."""
    dout, w = _f64(dout, w)
    return w.sum() * dout.sum(0)


# ------------------------------------------------------------------------------------------------- column sums
def colsum(X):
    return np.asarray(X).sum(0, dtype=np.float64)


# ------------------------------------------------------------------------------------------------- exactness of the integer cases
def worst_abs_sum(op, **d):
    """The largest sum of absolute terms any output of `op` can reach on `exact` operands (every operand at +-amp): each
    partial sum of the kernel, in whatever order, is at most this.  Below 2^24 every one of them is an exact fp32 integer."""
    a = d.get("amp", AMP)
    if op == "cloud_matmul":           # forward and dx: kd products
        return d["kd"] * a * a
    if op == "cloud_matmul_dT":        # one product per row of the cloud
        return max(d["N"], d["M"]) * a * a
    if op == "rowbias_add":
        return 2 * a
    if op == "rowbias_bwd":
        return max(d["N"], d["M"]) * a
    if op == "wsum":                   # P products and the bias
        return d["P"] * a * a + a
    if op == "wsum_dw":                # 3 B products and the accumulate prefill
        return 3 * d["B"] * a * a + a
    if op == "wsum_dbias":
        return 3 * d["B"] * a + a
    if op == "wsum_dbn":               # (sum_p w)(sum_b dout): P B products, and the prefill
        return d["P"] * a * d["B"] * a + a
    if op == "colsum":                 # R terms and the accumulate prefill
        return d["R"] * a + a
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------- tie cases of the max-pool
TIE_TYPES = "abcdef"


def tie_types_possible(n):
    """a) needs rows 1 and 2, b) needs rows r and r + 32."""
    return {t for t in TIE_TYPES if not (t == "a" and n < 3) and not (t == "b" and n < 33)}


def tie_cloud(n, J, *key):
    """[n, J] fp32: integers in [-8, 7] under crafted maxima (9), the column type cycling with j % 8:
      0  a) 9 in two rows of different row % 4, the earlier one not in lane 0 (n >= 3; else plain)
      1  b) 9 in two rows of the same row % 4 in different 32-row batches (n >= 33; else plain)
      2  c) 9 in row 0             3  d) 9 in row n - 1
      4  e) all -inf               5  f) +inf once
      6  plain integers (8 of them per 17 draws: natural ties)        7  one value in every row
    k_maxpool_fwd walks row r in lane r % 4, eight rows of a lane (a 32-row batch) in flight, and merges the four lanes'
    (max, row) pairs in lane order: a) makes the later row come first in that order for some columns, b) makes one lane meet
    its maximum twice."""
    rng = np.random.default_rng(seed_of("tie", n, J, *key))
    y = rng.integers(-AMP, AMP, size=(n, J)).astype(np.float32)
    for j in range(J):
        t = j % 8
        if t == 0 and n >= 3:
            r1 = int(rng.choice([r for r in range(n - 1) if r % 4 != 0]))
            r2 = int(rng.choice([r for r in range(r1 + 1, n) if r % 4 != r1 % 4]))
            y[[r1, r2], j] = 9
        elif t == 1 and n >= 33:
            r1 = int(rng.integers(0, n - 32))
            r2 = r1 + 32 * int(rng.integers(1, (n - 1 - r1) // 32 + 1))
            y[[r1, r2], j] = 9
        elif t == 2:
            y[0, j] = 9
        elif t == 3:
            y[n - 1, j] = 9
        elif t == 4:
            y[:, j] = -np.inf
        elif t == 5:
            y[int(rng.integers(0, n)), j] = np.inf
        elif t == 6:
            y[:, j] = rng.integers(-AMP, AMP + 1, size=n)
        elif t == 7:
            y[:, j] = y[0, j]
    return y


def tie_case(B, N, M, J):
    """[B*N + B*M, J] cloud-major, every cloud a `tie_cloud` of its own."""
    return np.concatenate([tie_cloud(n, J, B, N, M, c) for c, (_, n) in enumerate(cloud_slices(B, N, M))])


def tie_types_found(y):
    """The column types a) - f) present in one cloud's rows [n, J], read from the data alone."""
    n, J = y.shape
    found = set()
    for j in range(J):
        col = y[:, j]
        rows = np.flatnonzero(col == col.max())
        first = int(rows[0])
        if np.all(np.isneginf(col)):
            found.add("e")
            continue
        if np.count_nonzero(np.isposinf(col)) == 1:
            found.add("f")
        if len(rows) >= 2 and first % 4 != 0 and any(r % 4 != first % 4 for r in rows[1:]):
            found.add("a")
        if any(r % 4 == first % 4 and r // 32 != first // 32 for r in rows[1:]):
            found.add("b")
        if first == 0:
            found.add("c")
        if first == n - 1:
            found.add("d")
    return found
