"""Which graph a training forward builds: the ONE decision behind ``train_forward.forward_train`` and its helpers - the
Python-side counterpart of ``form_decision`` (csrc/catre_forms.h).

Pure functions of plain ints, bools and the ``TrainKernels`` tuple: no tensors, no thread-local state, no device - so the
route of any (mode, knobs, shapes) can be stated and tested on a host.  ``train_ops`` / ``train_forward`` keep their
``*_ok`` names as thin wrappers that read shapes off tensors and pass the compute mode and the knobs in.

mode: the compute mode of the forward (0 fp32, 1 bf16 operands - autocast -, 2 split), as ``train_ops._amp()`` returns it.
Weight shapes are (rows, columns) with every trailing dimension folded into the columns (Conv1d weights are [J,K,1])."""
import typing


class Stack(typing.NamedTuple):
    """One conv stack in front of a max-pool: conv a [j1,k1], conv b [j2,j1], the pooled conv [j3,j2]."""
    j1: int
    k1: int
    j2: int
    j3: int


class RotShape(typing.NamedTuple):
    """One rotation head: layers.0 [f0,k0] (k0 = out_dim + 64), layers.3 [f3,k3], and whether layers.3 has a bias."""
    f0: int
    k0: int
    f3: int
    k3: int
    l3_bias: bool


class Shapes(typing.NamedTuple):
    conv1: int                                  # pcl_net.conv1's width: the width of pointfeat
    stn: Stack
    fstn: typing.Optional[Stack]                # None: no feature transform in the model
    trunk: Stack
    rot: typing.Tuple[RotShape, RotShape]       # heads x, y


class EncRoute(typing.NamedTuple):
    kind: str       # "frozen": inference kernels, no nodes | "fused": catre_train_*_fwd + nodes with pre= | "layered"
    mode: int       # the compute mode the encoder's ops run in
    stn: str        # fused only, per stack: "chain" (row-sparse node) | "layered"; "" otherwise
    fstn: str
    trunk: str      # "hub" (the chain with pointfeat's other consumers: _PointfeatHub) | "layered"
    stn_rows: str   # fused only: "saved" | "recomputed" (the STN stacks store no activation rows)


class PerHead(typing.NamedTuple):
    first: str      # "lp_node" (the whole head: _RotHeadLP) | "l0_block" | "layered"
    second: str     # "" behind lp_node | "l1_block" | "l1_tail_lp" | "neck_tail" | "layered"


class TrainRoute(typing.NamedTuple):
    enc: EncRoute
    x_cm: bool      # the rotation heads read pointfeat in cloud-major rows: no object-major copy is made
    heads: str      # "form" | "fused_f32" (_RotHeads) | "split" | "lp_pair" (_RotHeadPairLP) | "per_head"
    split: typing.Optional[typing.Tuple[bool, bool]]      # heads == "split": first block / second block + tail as one node
    per_head: typing.Optional[typing.Tuple[PerHead, PerHead]]   # heads == "per_head": heads x, y
    ts: str         # "shipped" (gn_rows_gelu) | "form" (gn_rows_act)

    @property
    def obj_copy(self):
        return not self.x_cm


def _tiles(N, M):
    return N % 64 == 0 and M % 64 == 0


def tiled_gemm_ok(R, J, K, min_rows=2048):
    """Shapes the tiled row kernel (catre_op_gemm_rows) takes."""
    # (64-row tiles: under ~2048 rows - the FC tails, whose rows are clouds - the tiled kernel would put a handful of
    # workgroups on 256 CUs; the split-K catre_linear takes those)
    return (J % 32 == 0) and (J <= 256 or J in (512, 1024)) and (K in (8, 16, 32, 64, 128) or K % 256 == 0) and R >= min_rows


def rot_linear_ok(R, J, K, N, M):
    return _tiles(N, M) and tiled_gemm_ok(R, J, K, min_rows=64) and K % 8 == 0


def pooled_chain_ok(x_grad, s, N, M):
    """Shapes the row-sparse chain takes (the encoder's three conv stacks at N, M multiples of 64; every compute mode)."""
    if not _tiles(N, M) or max(N, M) > 4096:
        return False
    if x_grad and not tiled_gemm_ok(1, s.k1, s.j1, min_rows=0):
        return False  # the chain's input gradient is a tiled row GEMM with K1 outputs: a differentiable 3-d input takes the layer-wise ops
    return s.j1 in (64, 128) and s.j2 in (128, 512) and s.j3 <= 1024 and s.j3 % 32 == 0 and (s.k1 <= 8 or s.k1 in (64, 128))


def fused_lp_ok(pts_grad, sh, N, M):
    """The autocast fused encoder forward stores bf16 activation rows, which only the row-sparse chains read: every stack
    must take that form (it does at N, M multiples of 64 up to 4096 points per cloud, for inputs without gradient)."""
    # (only the first stack's input can be 3 wide: the clause on a differentiable input bites there alone)
    return pooled_chain_ok(pts_grad, sh.stn, N, M) and pooled_chain_ok(False, sh.fstn, N, M) and pooled_chain_ok(False, sh.trunk, N, M)


def rot_heads_ok(mode, pfw, N, M):
    return mode == 0 and pfw == 64 and _tiles(N, M) and N > 0 and M > 0


def rot_heads_shapes_ok(sh, D, N, M):
    return (sh.conv1 == 64 and _tiles(N, M) and N > 0 and M > 0
            and all(r.l3_bias and (r.f0, r.k0) == (256, D + 64) and (r.f3, r.k3) == (256, 256) for r in sh.rot))


def rot_head_lp_ok(mode, k, pfw, f0, k0, f3, k3, l3_bias, N, M):
    """(f0, k0): the POINT half of layers.0."""
    return (k.fused_lp_rot and k.lp_rot_bf16_rows and mode == 1 and pfw == 64 and (f0, k0) == (256, 64) and (f3, k3) == (256, 256)
            and l3_bias and _tiles(N, M) and N > 0 and M > 0)


def rot_l1_tail_lp_ok(mode, k, aw, f3, k3, l3_bias, N, M):
    return k.fused_lp_rot and mode == 1 and aw == 256 and (f3, k3) == (256, 256) and l3_bias and _tiles(N, M) and N > 0 and M > 0


def rot_l0_block_ok(mode, k, pfw, f0, k0, N, M):
    # autocast takes the node too (knob fused_lp_rot): bf16-operand forward, the one-pass backward
    return (mode == 0 or (mode == 1 and k.fused_lp_rot)) and (f0, k0) == (256, 64) and pfw == 64 and _tiles(N, M) and N > 0


def rot_l1_block_ok(mode, aw, f3, k3, N, M):
    return mode == 0 and aw == 256 and (f3, k3) == (256, 256) and _tiles(N, M) and N > 0


def per_head_route(mode, k, pfw, r, B, N, M):
    """One shipped-form rotation head on the per-head ops.  The ladder, in order:
    1. autocast, knobs fused_lp_rot and lp_rot_bf16_rows: the whole head is one node, "lp_node";
    2. first half: "l0_block" (fp32; autocast with fused_lp_rot) else "layered" (linear_cloudbias + gn_points_gelu);
    3. second half: "l1_block" (fp32), else "l1_tail_lp" (autocast with fused_lp_rot), else "neck_tail" when the linear's
       epilogue gives GroupNorm partials (a tiled 256-wide row GEMM) and N + M is a multiple of 64, else "layered"."""
    if rot_head_lp_ok(mode, k, pfw, r.f0, 64, r.f3, r.k3, r.l3_bias, N, M):
        return PerHead("lp_node", "")
    first = "l0_block" if rot_l0_block_ok(mode, k, pfw, r.f0, 64, N, M) else "layered"
    if rot_l1_block_ok(mode, r.f0, r.f3, r.k3, N, M) and r.l3_bias:
        return PerHead(first, "l1_block")
    if rot_l1_tail_lp_ok(mode, k, r.f0, r.f3, r.k3, r.l3_bias, N, M):
        return PerHead(first, "l1_tail_lp")
    if r.f3 == 256 and rot_linear_ok(B * (N + M), r.f3, r.k3, N, M) and (N + M) % 64 == 0:
        return PerHead(first, "neck_tail")
    return PerHead(first, "layered")


def encoder_route(mode, k, has_rt, D, feature_transform, N, M, nm_match, enc_frozen, pts_grad, sh):
    """The encoder of a training forward.  The ladder, in order (has_rt: the model's runtime exists; nm_match: N + M is the
    point count its packs were made for):
    1. "frozen" - runtime, nothing in front of the heads needs a gradient, and the encoder is fp32 (mode 0, or D != 1024:
       that encoder is fp32 in every mode);
    2. "fused" - runtime, D == 1024, feature transform, N and M multiples of 64; under autocast only when all three
       stacks are row-sparse chains (`fused_lp_ok`), else "layered" in the ambient mode;
    3. "layered" otherwise - in fp32 when D != 1024."""
    if has_rt and enc_frozen and (mode == 0 or D != 1024) and nm_match:
        return EncRoute("frozen", 0, "", "", "", "")
    if (has_rt and D == 1024 and feature_transform and _tiles(N, M) and nm_match
            and not (mode == 1 and not fused_lp_ok(pts_grad, sh, N, M))):
        return EncRoute("fused", mode,
                        "chain" if pooled_chain_ok(pts_grad, sh.stn, N, M) else "layered",
                        "chain" if pooled_chain_ok(False, sh.fstn, N, M) else "layered",
                        "hub" if pooled_chain_ok(False, sh.trunk, N, M) else "layered",
                        # fp32: the STN stacks store no activation rows (their row-sparse backward rebuilds them on its live rows)
                        "recomputed" if mode == 0 and k.stn_recompute and not pts_grad else "saved")
    return EncRoute("layered", mode if D == 1024 else 0, "", "", "", "")


def train_route(mode, k, has_rt, layered, rot_shipped, ts_shipped, D, feature_transform, B, N, M, nm_match, enc_frozen, pts_grad,
                sh):
    """The route of ``forward_train``: mode, knobs ``k`` (TrainKernels), whether a runtime exists and is ``layered`` (packs
    the encoder only), whether the heads have the shipped form, D = out_dim, the batch and cloud sizes, ``nm_match`` (N + M
    equals the runtime's), whether the encoder is frozen, whether the 3-d input needs a gradient, the layer shapes.

    The encoder first (:func:`encoder_route`).  Pointfeat leaves it through a hub - the frozen encoder's plain outputs, or the
    fused encoder's trunk as `_PointfeatHub` - or not (layered ops).  Then the heads' ladder, in order:
    1. "form" - a rotation head of another form than the shipped one: the generic layer-by-layer ops;
    2. "fused_f32" - mode 0, a runtime that packs the heads, feature transform, shipped head shapes, behind a hub;
    3. "split" - mode 2, the same runtime and shapes, behind a hub; its two halves per the split_l*_one_pass knobs;
    4. "lp_pair" - mode 1, D == 1024, knobs fused_lp_rot and lp_rot_bf16_rows, the same shapes, behind a hub;
    5. "per_head" - :func:`per_head_route` for each head.
    "fused_f32" and "lp_pair" read pointfeat cloud-major (``x_cm``): no object-major copy is made for them."""
    enc = encoder_route(mode, k, has_rt, D, feature_transform, N, M, nm_match, enc_frozen, pts_grad, sh)
    ts = "shipped" if ts_shipped else "form"
    if not rot_shipped:
        return TrainRoute(enc, False, "form", None, None, ts)
    # (a runtime whose ts head alone has another form packs the encoder only: the rotation heads' fused forwards, which read
    # the packed head image, are not taken then - the per-head ops are)
    # (a hub implies a runtime whose point count matches)
    if (enc.kind == "frozen" or enc.trunk == "hub") and rot_heads_shapes_ok(sh, D, N, M):
        if mode == 0 and not layered and feature_transform:
            return TrainRoute(enc, True, "fused_f32", None, None, ts)
        if mode == 2 and not layered:
            return TrainRoute(enc, False, "split", (k.split_l0_one_pass, k.split_l1_one_pass), None, ts)
        if mode == 1 and D == 1024 and feature_transform and k.fused_lp_rot and k.lp_rot_bf16_rows:
            return TrainRoute(enc, True, "lp_pair", None, None, ts)
    return TrainRoute(enc, False, "per_head", None,
                      tuple(per_head_route(mode, k, sh.conv1, r, B, N, M) for r in sh.rot), ts)
