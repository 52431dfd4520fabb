"""One training refine-iteration - forward, loss, backward, optimizer step - captured in a HIP graph.

The training path launches ~450 kernels per iteration, and everything in the iteration is shape-static and free of
host synchronisation (device-side loss, fused optimizer), so it can be captured once and replayed:

    step = GraphedTrainStep(model, optimizer, example_batch, sym_info)       # warm-up + capture
    out_dict, loss_dict = step(x=..., tfd_kps=..., init_pose=..., ..., sym_info=[...])

Per call the host only copies the batch into the static input buffers, advances the optimizer's scalar state
(``Ranger.prepare_step`` -> a pinned table that is uploaded right before the replay) and replays the graph.  The
outputs are static tensors that the next call overwrites (``clone()`` what must survive).  Shapes (B, N, M), the
loss configuration and the maximum number of symmetry candidates are fixed at capture time; the mix of symmetric /
non-symmetric objects may change freely (it lives in device tensors).

This is an opt-in wrapper around the same module, kernels and optimizer - the reference's eager train loop
(``core/catre/engine/engine.py:293-355``) keeps working unchanged.  Replays are bit-identical to the eager loop
(``tests/test_hip_train.py::test_graphed_train_step_replays_the_eager_iteration``).

Measured (``profiles/train_step_graphed.py``, one MI355X, N=M=1024): the eager loop has a host-side floor of
~4.85 ms per iteration (B <= 16: ~450 launches); replaying takes 3.5 / 3.9 / 4.7 ms at B = 4 / 8 / 16 (1.4x / 1.26x /
1.04x) and is on par with the eager loop from B = 32 up, where the GPU work itself (a serial chain of short kernels)
is the bound.  Besides the small-batch gain the graph removes the per-iteration host CPU load.

:class:`GraphedTrainLoop` is the same idea for the batches a real run sees - another object count every step: one graph per
capacity bucket, the batch padded to the bucket, the loss kernels told the count through a device int.
"""
import torch

from . import hip
from .losses import SymTensors
from .ranger import Ranger

_INPUTS = ("x", "tfd_kps", "init_pose", "init_scale", "K_zoom", "gt_ego_rot", "gt_trans", "gt_scale", "obj_kps",
           "mean_scales")


def _require_shipped_heads(model, what):
    """The captured chains are the fused ones: heads of another form run a host-side layer loop that is not captured."""
    out_dim = int(getattr(getattr(model, "pcl_net", None), "out_dim", 1024))
    if out_dim != 1024:
        raise NotImplementedError(f"{what} captures the fused kernels, which are built for PCLNET.INIT_CFG.out_dim=1024; with "
                                  f"out_dim={out_dim} call model.refine / model.forward directly (fp32, bf16 / autocast or "
                                  "split)")
    forms = getattr(model, "_head_forms", None)
    if forms is not None:
        from .heads import SHIPPED_FORM

        if any(f != SHIPPED_FORM for f in forms()):
            raise NotImplementedError(f"{what} captures the fused kernels of the shipped head form (feat_dim=256, "
                                      "num_layers=2, GN with 32 groups, gelu); with heads of another form call "
                                      "model.refine / model.forward directly (fp32, bf16 / autocast or split)")


def _snapshot_training_state(opt):
    """Parameters and the optimizer's per-parameter state, to be put back after a capture's warm-up steps."""
    params = [p for g in opt.param_groups for p in g["params"]]
    snap_p = [p.detach().clone() for p in params]
    snap_s = {p: (st["step"], st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["slow_buffer"].clone())
              for p, st in opt.state.items() if "exp_avg" in st}
    return params, snap_p, snap_s


def _restore_training_state(opt, snap):
    params, snap_p, snap_s = snap
    with torch.no_grad():
        for p, q in zip(params, snap_p):
            p.copy_(q)
        for p, st in opt.state.items():
            if "exp_avg" not in st:
                continue
            if p in snap_s:
                st["step"] = snap_s[p][0]
                st["exp_avg"].copy_(snap_s[p][1]); st["exp_avg_sq"].copy_(snap_s[p][2]); st["slow_buffer"].copy_(snap_s[p][3])
            else:  # state created by the warm-up: back to a fresh optimizer's
                st["step"] = 0
                st["exp_avg"].zero_(); st["exp_avg_sq"].zero_(); st["slow_buffer"].copy_(p)
    hip.bump_param_epoch()


class GraphedTrainStep:
    def __init__(self, model, optimizer, example, sym_info, max_sym=None, warmup=3, amp=False):
        if not isinstance(optimizer, Ranger):
            raise TypeError("GraphedTrainStep needs the fused catre_amd.ranger.Ranger (its step is capturable)")
        _require_shipped_heads(model, "GraphedTrainStep")
        self.model, self.opt, self.amp = model, optimizer, bool(amp)
        dev = example["x"].device
        self.static = {k: example[k].detach().clone().contiguous() for k in _INPUTS if example.get(k) is not None}
        B = self.static["x"].shape[0]
        if max_sym is None:
            max_sym = max([1] + [len(s) for s in sym_info if s is not None])
        self.s1 = int(max_sym) + 1
        self.sym = SymTensors.from_list(sym_info, dev, s1=self.s1)
        self.sym = SymTensors(self.sym.cands.clone(), self.sym.valid.clone(), self.sym.is_sym.clone())  # own static buffers
        self._B = B

        def iteration():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.amp):
                out, ld = self.model(self.static["x"], self.static["tfd_kps"], init_pose=self.static["init_pose"],
                                     init_scale=self.static["init_scale"], K_zoom=self.static.get("K_zoom"),
                                     gt_ego_rot=self.static["gt_ego_rot"], gt_trans=self.static["gt_trans"],
                                     gt_scale=self.static["gt_scale"], obj_kps=self.static["obj_kps"],
                                     mean_scales=self.static.get("mean_scales"), sym_info=self.sym, do_loss=True,
                                     cur_iter=1)
            loss = sum(ld.values())
            loss.backward()
            return out, ld

        # warm-up on a side stream (allocates scratch, optimizer state, the packed-weight buffers).  The steps it
        # takes are undone afterwards: parameters and optimizer state are restored to what the caller handed in.
        snap = _snapshot_training_state(self.opt)
        params = snap[0]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.opt.zero_grad(set_to_none=True)
                iteration()
                self.opt.step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        _restore_training_state(self.opt, snap)
        torch.cuda.synchronize(dev)

        # capture: gradients are allocated inside the graph's private pool, so their addresses are fixed
        self.opt.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        # captured on the warm-up stream, so the kernels point at THAT stream's scratch buffers (train_ops._ws and the
        # runtime's workspace are per (device, stream)), which the warm-up has already grown to their final size
        with torch.cuda.graph(self.graph, stream=side, capture_error_mode="relaxed"):
            self.out, self.losses = iteration()
            # host half runs now (addresses of the captured gradients go into the record table) ...
            self.opt.prepare_step(wait=False)
            # ... and only the kernels are captured; the table upload is issued eagerly before every replay
            self.opt.launch_step(upload=False)
        # the buffers whose addresses are baked into the graph are owned here, whatever the per-stream caches do later
        # (an eager step that outgrows a cache entry replaces it; the captured block must not be recycled under the graph)
        from . import train_ops

        rt = self.model._runtime() if hasattr(self.model, "_runtime") else None
        self._keep = (train_ops.scratch_of(dev, side), side,
                      None if rt is None or rt._ws is None else rt._ws.get((dev.index, side.cuda_stream)),
                      None if rt is None else rt._packed)
        # the gradient tensors the captured backward writes and the captured optimizer step reads: re-attached before every
        # replay (an eager `zero_grad(set_to_none=True)` in between detaches them, and the host half of the step would
        # then find no gradient to describe)
        self._grads = [(p, p.grad) for p in params if p.grad is not None]
        # the packs recorded above did not execute: the next eager forward must re-pack (HipRuntime.params also refuses
        # to call a pack fresh while capturing)
        hip.bump_param_epoch()
        # the capture did not execute anything: undo the step counter it advanced
        for st in self.opt.state.values():
            if "step" in st:
                st["step"] -= 1

    @torch.no_grad()
    def __call__(self, sym_info=None, **inputs):
        for k, v in inputs.items():
            if k not in self.static:
                raise KeyError(f"unknown or uncaptured input {k!r}")
            if v.shape != self.static[k].shape:
                raise ValueError(f"{k}: captured with shape {tuple(self.static[k].shape)}, got {tuple(v.shape)}")
            self.static[k].copy_(v, non_blocking=True)
        if sym_info is not None:
            new = SymTensors.from_list(sym_info, self.sym.cands.device, s1=self.s1)
            if new.cands.shape != self.sym.cands.shape:
                raise ValueError("more symmetry candidates than the graph was captured for (max_sym)")
            self.sym.cands.copy_(new.cands, non_blocking=True)
            self.sym.valid.copy_(new.valid, non_blocking=True)
            self.sym.is_sym.copy_(new.is_sym, non_blocking=True)
        for p, g in self._grads:
            if p.grad is not g:
                p.grad = g
        self.opt.prepare_step()   # host: step counters, RAdam scalars -> pinned table
        self.opt.upload_table()   # stream-ordered before the replay
        self.graph.replay()
        hip.bump_param_epoch()
        return self.out, self.losses


# --------------------------------------------------------------------------------- the refine loop, any object count
DEFAULT_BUCKETS = (16, 32, 48, 64, 96, 128)


def pick_bucket(n, buckets):
    """The smallest capacity of ``buckets`` (ascending) that holds ``n`` objects; None when none does."""
    for c in buckets:
        if c >= n:
            return c
    return None


def loop_rows(batch):
    """The per-object tensors one training iteration reads, picked from a batch as ``batch_updater``'s first call leaves
    it: ``pcl [n,N,3]``, ``obj_kps [n,M,3]``, ``obj_pose_est [n,3,4]``, ``obj_scale_est [n,3]``, optionally ``K`` and
    ``obj_mean_scales``, and the ground truth - the reference's ``obj_pose [n,3,4]`` / ``obj_scale`` (engine.py:312-314)
    or ``gt_rot`` / ``gt_trans`` / ``gt_scale`` as ``synth.make_inputs`` names them."""
    rows = {}
    for k in ("pcl", "obj_kps", "obj_pose_est", "obj_scale_est"):
        if batch.get(k) is None:
            raise KeyError(f"batch lacks {k!r} (call batch_updater once before the loop)")
        rows[k] = batch[k]
    for k in ("K", "obj_mean_scales"):
        if batch.get(k) is not None:
            rows[k] = batch[k]
    if batch.get("obj_pose") is not None:
        rows["gt_rot"], rows["gt_trans"] = batch["obj_pose"][:, :3, :3], batch["obj_pose"][:, :3, 3]
    elif batch.get("gt_rot") is not None and batch.get("gt_trans") is not None:
        rows["gt_rot"], rows["gt_trans"] = batch["gt_rot"], batch["gt_trans"]
    else:
        raise KeyError("batch lacks the ground truth pose ('obj_pose', or 'gt_rot' and 'gt_trans')")
    gs = batch.get("obj_scale") if batch.get("obj_scale") is not None else batch.get("gt_scale")
    if gs is not None:
        rows["gt_scale"] = gs
    return rows


def _fill_padded(dst_rows, dst_sym, idx, rows, sym, n):
    """Rows 0..n of every destination = the batch, rows n.. = copies of object 0 (finite, so the exact zeros the loss sends
    back to them stay zeros all the way down); the count goes into the device int the loss kernels read."""
    for k, dst in dst_rows.items():
        torch.index_select(hip.require_dev_f32(rows[k], k, contiguous=False), 0, idx, out=dst)
    torch.index_select(sym.cands, 0, idx, out=dst_sym.cands)
    torch.index_select(sym.valid, 0, idx, out=dst_sym.valid)
    torch.index_select(sym.is_sym, 0, idx, out=dst_sym.is_sym)
    dst_sym.n_obj.fill_(n)


def _alloc_padded(rows, s1, C, dev):
    dst = {k: torch.empty((C,) + tuple(v.shape[1:]), dtype=torch.float32, device=dev) for k, v in rows.items()}
    sym = SymTensors(torch.empty(C, s1, 3, 3, dtype=torch.float32, device=dev),
                     torch.empty(C, s1, dtype=torch.uint8, device=dev), torch.empty(C, dtype=torch.int32, device=dev),
                     torch.empty(1, dtype=torch.int32, device=dev))
    return dst, sym


def pad_rows(rows, sym, n, capacity):
    """-> (rows, SymTensors with ``n_obj``) of ``capacity`` objects: new tensors, the ``n`` objects first."""
    dev = rows["pcl"].device
    dst, dsym = _alloc_padded(rows, sym.cands.shape[1], capacity, dev)
    ar = torch.arange(capacity, device=dev)
    _fill_padded(dst, dsym, ar * (ar < n), rows, sym, n)
    return dst, dsym


def refine_iteration(model, rows, sym, amp=False):
    """Forward, loss and backward of ONE refine iteration on ``rows`` (engine.py:295-349 without the optimizer): the pose
    estimate is applied to the cloud and the prior, the model runs with ``do_loss=True`` and the summed loss dict is
    differentiated.  -> (out_dict, loss_dict) with ``cur_iter=1`` keys."""
    from .runtime import pose_apply

    x, tfd_kps = pose_apply(rows["pcl"], rows["obj_kps"], rows["obj_pose_est"], rows["obj_scale_est"],
                            zero_center=model.cfg.INPUT.ZERO_CENTER_INPUT)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(amp)):
        out, ld = model(x, tfd_kps, init_pose=rows["obj_pose_est"], init_scale=rows["obj_scale_est"], K_zoom=rows.get("K"),
                        gt_ego_rot=rows["gt_rot"], gt_trans=rows["gt_trans"], gt_scale=rows.get("gt_scale"),
                        obj_kps=rows["obj_kps"], mean_scales=rows.get("obj_mean_scales"), sym_info=sym, do_loss=True,
                        cur_iter=1)
        loss = sum(ld.values())
    loss.backward()
    return out, ld


@torch.no_grad()
def _feed_back(rows, out):
    """``poses_est = out_dict["pose_i"].detach()`` -> the next iteration's estimate (engine.py:324-325), in place."""
    rows["obj_pose_est"].copy_(out["pose_1"].detach())
    rows["obj_scale_est"].copy_(out["scale_1"].detach())


class LossLog:
    """What the reference's loop reads with ``.item()`` eight times per iteration, kept on the device: ``tensor``
    [n_iter, 22] - row r = the loss slots and the ``vis/`` scalars of refine iteration r + 1 - and ``keys``, the name of
    every column (None for a loss slot the configuration does not fill).  ``as_dicts()`` is ONE copy to the host."""

    def __init__(self, tensor, keys):
        self.tensor, self.keys = tensor, tuple(keys)

    def as_dicts(self):
        return [{k: v for k, v in zip(self.keys, row) if k is not None} for row in self.tensor.tolist()]


class _Bucket:
    pass


class GraphedTrainLoop:
    """The reference's refine loop for one data batch (``core/catre/engine/engine.py:293-355``) replayed from HIP graphs,
    for batches whose object count changes from step to step (``batching.py:66``: the instances of 16 images, 40..110):

        loop = GraphedTrainLoop(model, optimizer, N, M)                 # nothing is captured yet
        batch_updater(cfg, batch)                                       # initial estimates, obj_kps (once per batch)
        out_dict, loss_log = loop(batch, n_iter, batch.get("sym_info")) # replaces the body of the `for refine_i` loop

    One graph per capacity in ``buckets``, captured the first time a batch needs it; a batch of ``n`` objects runs in the
    smallest capacity >= n.  Rows n.. are copies of object 0 and the loss kernels read ``n`` from a device int
    (``SymTensors.n_obj``): padded rows enter no loss, get exact-zero gradients and drop out of the row-sparse backward by
    themselves.  A batch above the largest bucket runs the same iterations eagerly.  The captured unit is one refine
    iteration - ``pose_apply`` with the static estimate, forward with ``do_loss=True``, backward of the summed loss dict, the
    fused Ranger step, the new estimate copied back - so ``n_iter`` may change per call.  Per replay the host runs
    ``prepare_step()`` + ``upload_table()`` (learning-rate changes travel in that table) and one copy of the 22 logged floats.

    ``out_dict``: ``pose_{n_iter}`` / ``scale_{n_iter}`` as views of the first ``n`` static rows (overwritten by the next call
    in the same bucket); ``loss_log``: :class:`LossLog` on a static tensor the next call overwrites.  A lazy capture leaves parameters and optimizer state as it found
    them.  Every graph pins the scratch it was captured with (``stats()``); ``max_graphs`` keeps that many, evicting the
    least recently used.  Shipped head form and the fused ``Ranger`` only; the model is the bare module (no DDP wrapper
    inside a graph)."""

    def __init__(self, model, optimizer, N, M, buckets=DEFAULT_BUCKETS, max_sym=None, amp=False, max_graphs=None, warmup=2):
        if not isinstance(optimizer, Ranger):
            raise TypeError("GraphedTrainLoop needs the fused catre_amd.ranger.Ranger (its step is capturable)")
        _require_shipped_heads(model, "GraphedTrainLoop")
        if int(N) != N or int(M) != M or N <= 0 or M <= 0:
            raise ValueError(f"N, M: positive point counts, got {N!r}, {M!r}")
        buckets = tuple(buckets)
        if not buckets or any(int(c) != c or c <= 0 for c in buckets):
            raise ValueError(f"buckets: one or more positive capacities, got {buckets!r}")
        if max_graphs is not None and (int(max_graphs) != max_graphs or max_graphs < 1):
            raise ValueError(f"max_graphs: None or a count >= 1, got {max_graphs!r}")
        if max_sym is not None and (int(max_sym) != max_sym or max_sym < 0):
            raise ValueError(f"max_sym: None or a candidate count >= 0, got {max_sym!r}")
        if int(warmup) < 1:
            raise ValueError("warmup: at least one iteration (it allocates what the capture points at)")
        self.model, self.opt, self.amp = model, optimizer, bool(amp)
        self.N, self.M = int(N), int(M)
        self.buckets = tuple(sorted({int(c) for c in buckets}))
        self.max_graphs = None if max_graphs is None else int(max_graphs)
        self.s1 = None if max_sym is None else int(max_sym) + 1
        self.warmup = int(warmup)
        self._graphs = {}     # capacity -> _Bucket, least recently used first
        self._log = None
        self.captures = 0     # graphs captured so far (evicted ones included)

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def bucket_for(self, n):
        return pick_bucket(n, self.buckets)

    def stats(self):
        """capacity -> bytes of device memory reserved for the live graph (its pool, statics and scratch), seconds its
        capture took."""
        return {C: dict(bytes=bk.bytes, capture_s=bk.capture_s) for C, bk in self._graphs.items()}

    def _check(self, batch, n_iter, sym_info):
        rows = loop_rows(batch)
        n = int(rows["pcl"].shape[0])
        if n < 1:
            raise ValueError("an empty batch has no loss")
        if int(n_iter) != n_iter or n_iter < 1:
            raise ValueError(f"n_iter: a count >= 1, got {n_iter!r}")
        if tuple(rows["pcl"].shape) != (n, self.N, 3) or tuple(rows["obj_kps"].shape) != (n, self.M, 3):
            raise ValueError(f"the loop was built for pcl [n,{self.N},3] and obj_kps [n,{self.M},3], got "
                             f"{tuple(rows['pcl'].shape)} and {tuple(rows['obj_kps'].shape)}")
        if sym_info is None:
            sym_info = batch.get("sym_info")
        sym_info = [None] * n if sym_info is None else list(sym_info)
        if len(sym_info) != n:
            raise ValueError(f"sym_info holds {len(sym_info)} entries for {n} objects")
        return rows, n, int(n_iter), sym_info

    def _param_ptrs(self):
        return tuple(p.data_ptr() for g in self.opt.param_groups for p in g["params"])

    def _drop_all(self):
        if self._graphs:
            torch.cuda.synchronize()
        for C in list(self._graphs):
            self._drop(C)

    def _drop(self, C):
        bk = self._graphs.pop(C)
        for p, g in bk.grads:
            if p.grad is g:
                p.grad = None

    # ---------------------------------------------------------------------------------------------------- capture
    def _capture(self, C, rows, sym, n):
        import time

        from . import train_ops
        from .losses import loss_block

        dev = rows["pcl"].device
        torch.cuda.synchronize(dev)
        t0, mem0 = time.perf_counter(), torch.cuda.memory_reserved(dev)
        bk = _Bucket()
        bk.C = C
        bk.rows, bk.sym = _alloc_padded(rows, self.s1, C, dev)
        bk.ar = torch.arange(C, device=dev)
        bk.idx = torch.empty_like(bk.ar)
        self._stage(bk, rows, sym, n)

        # warm-up on a side stream (this stream's scratch, optimizer state and record table, packed weights), undone afterwards
        snap = _snapshot_training_state(self.opt)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(self.warmup):
                self.opt.zero_grad(set_to_none=True)
                refine_iteration(self.model, bk.rows, bk.sym, self.amp)
                self.opt.step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        _restore_training_state(self.opt, snap)
        torch.cuda.synchronize(dev)

        # capture on the warm-up stream (the kernels point at that stream's scratch); gradients live in the graph's pool
        self.opt.zero_grad(set_to_none=True)
        bk.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(bk.graph, stream=side, capture_error_mode="relaxed"):
            out, _ = refine_iteration(self.model, bk.rows, bk.sym, self.amp)
            self.opt.prepare_step(wait=False)   # host half now: the captured gradients' addresses go into the record table
            self.opt.launch_step(upload=False)  # only the kernels are captured; the table is uploaded before every replay
            _feed_back(bk.rows, out)
            bk.block = loss_block(self.model.vis_scalars.tensor)
        rt = self.model._runtime() if hasattr(self.model, "_runtime") else None
        bk.keep = (train_ops.scratch_of(dev, side), side,
                   None if rt is None or rt._ws is None else rt._ws.get((dev.index, side.cuda_stream)),
                   None if rt is None else rt._packed)
        del out
        bk.grads = [(p, p.grad) for p in snap[0] if p.grad is not None]
        bk.param_ptrs = self._param_ptrs()
        hip.bump_param_epoch()   # the packs recorded above did not execute
        for st in self.opt.state.values():   # nor did the step whose counter the capture advanced
            if "step" in st:
                st["step"] -= 1
        torch.cuda.synchronize(dev)
        # the graph's private pool, the statics and this stream's scratch, as the allocator had to reserve them
        bk.bytes, bk.capture_s = torch.cuda.memory_reserved(dev) - mem0, time.perf_counter() - t0
        self.captures += 1
        return bk

    def _stage(self, bk, rows, sym, n):
        torch.mul(bk.ar, bk.ar < n, out=bk.idx)   # 0 .. n-1, then zeros: the padding repeats object 0
        _fill_padded(bk.rows, bk.sym, bk.idx, rows, sym, n)

    def _bucket(self, C, rows, sym, n):
        bk = self._graphs.get(C)
        if bk is not None and (bk.param_ptrs != self._param_ptrs() or set(bk.rows) != set(rows)):
            self._drop_all()   # parameters were re-allocated, or the batch's optional inputs changed: stale addresses
            bk = None
        if bk is None:
            if self.max_graphs is not None and len(self._graphs) >= self.max_graphs:
                torch.cuda.synchronize()   # the graph that goes may still be replaying
                while len(self._graphs) >= self.max_graphs:
                    self._drop(next(iter(self._graphs)))
            bk = self._capture(C, rows, sym, n)
        else:
            del self._graphs[C]
        self._graphs[C] = bk   # most recently used last
        return bk

    # ------------------------------------------------------------------------------------------------------- run
    @torch.no_grad()
    def __call__(self, batch, n_iter, sym_info=None):
        rows, n, n_iter, sym_info = self._check(batch, n_iter, sym_info)
        C = self.bucket_for(n)
        if C is None:
            with torch.enable_grad():
                return self.run_eager(batch, n_iter, sym_info)
        dev = rows["pcl"].device
        with torch.cuda.device(dev):
            sym = SymTensors.from_list(sym_info, dev, s1=self.s1)
            if self.s1 is None or sym.cands.shape[1] > self.s1:   # more candidates than any graph was captured for
                self._drop_all()
                self.s1 = int(sym.cands.shape[1])
            with torch.enable_grad():
                bk = self._bucket(C, rows, sym, n)
            self._stage(bk, rows, sym, n)
            if self._log is None or self._log.shape[0] < n_iter or self._log.device != dev:
                self._log = torch.empty(n_iter, bk.block.numel(), dtype=torch.float32, device=dev)
            for p, g in bk.grads:   # an eager step or another bucket in between detached them
                if p.grad is not g:
                    p.grad = g
            for r in range(n_iter):
                self.opt.prepare_step()   # host: step counters, RAdam scalars, this bucket's gradient addresses
                self.opt.upload_table()   # stream-ordered before the replay
                bk.graph.replay()
                self._log[r].copy_(bk.block, non_blocking=True)
            hip.bump_param_epoch()
        return ({f"pose_{n_iter}": bk.rows["obj_pose_est"][:n], f"scale_{n_iter}": bk.rows["obj_scale_est"][:n]},
                LossLog(self._log[:n_iter], self._keys()))

    def _keys(self):
        from .losses import loss_block_keys

        return loss_block_keys(self.model.cfg)

    def run_eager(self, batch, n_iter, sym_info=None, capacity=None):
        """The same loop without a graph: what a batch above the largest bucket gets (``capacity=None``: the objects as they
        are, the plain loss entry points), and - with a capacity - the padded iteration a graph of that bucket replays."""
        from .losses import loss_block

        rows, n, n_iter, sym_info = self._check(batch, n_iter, sym_info)
        dev = rows["pcl"].device
        with torch.cuda.device(dev):
            sym = SymTensors.from_list(sym_info, dev, s1=self.s1)
            if capacity is None:
                rows = dict(rows)   # the estimates are updated in place: on copies, not in the caller's batch
                for k in ("obj_pose_est", "obj_scale_est"):
                    rows[k] = hip.require_dev_f32(rows[k], k, contiguous=False).detach().clone().contiguous()
            else:
                if capacity < n:
                    raise ValueError(f"capacity {capacity} below the {n} objects of the batch")
                rows, sym = pad_rows(rows, sym, n, int(capacity))
            log = None
            for r in range(n_iter):
                self.opt.zero_grad(set_to_none=True)
                out, _ = refine_iteration(self.model, rows, sym, self.amp)
                self.opt.step()
                _feed_back(rows, out)
                block = loss_block(self.model.vis_scalars.tensor)
                if log is None:
                    log = torch.empty(n_iter, block.numel(), dtype=torch.float32, device=dev)
                log[r].copy_(block)
            self.opt.zero_grad(set_to_none=True)
        return ({f"pose_{n_iter}": rows["obj_pose_est"][:n], f"scale_{n_iter}": rows["obj_scale_est"][:n]},
                LossLog(log, self._keys()))


_REFINE_INPUTS = ("pcl", "obj_kps", "obj_pose_est", "obj_scale_est", "K", "obj_mean_scales")


class GraphedRefine:
    """``model.refine`` for a fixed (B, N, M, K) as ONE HIP-graph replay.

    The evaluator's operating point (one image = a handful of objects per call, ``catre_evaluator.py:292-311``) is a chain
    of 14 short launches per iteration: at B=1 the K=4 loop is 0.60 ms of GPU time and 0.24 ms of host time, all of it
    ``hipLaunchKernel`` (56 launches).  One stream hides that behind the GPU; several images refined concurrently on
    separate streams do not - four streams saturate at 3.5 k refines/s because the HOST is busy launching
    (``profiles/multi_stream_probe.py``).  Replaying a captured graph costs the host one packed copy of the inputs (a
    single ``torch.cat`` into the static buffer) and one graph launch:

        g = GraphedRefine(model, example_batch)          # warm-up + capture on a side stream
        out = g(batch)                                   # pose_0..pose_K / scale_0..scale_K, same keys as model.refine

    The outputs are static tensors that the next call overwrites (``clone()`` what must survive).  Shapes and ``n_iter``
    are fixed at capture; the weights are re-checked on every call (an in-place update is re-packed before the replay, a
    re-allocated parameter triggers a new capture).  Replays are bit-identical to ``model.refine``.  One instance per
    stream for concurrent use (each owns its inputs, outputs and scratch).
    """

    def __init__(self, model, example, n_iter=None, warmup=2):
        _require_shipped_heads(model, "GraphedRefine")
        self.model = model
        self.n_iter = int(model.cfg.MODEL.CATRE.N_ITER_TEST if n_iter is None else n_iter)
        self.keys = [k for k in _REFINE_INPUTS if example.get(k) is not None]
        for k in ("pcl", "obj_kps", "obj_pose_est", "obj_scale_est"):
            if k not in self.keys:
                raise KeyError(f"example batch lacks {k!r}")
        dev = example["pcl"].device
        self.dev = dev
        self.shapes = {k: tuple(example[k].shape) for k in self.keys}
        sizes = [int(example[k].numel()) for k in self.keys]
        self.flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        self.static, off = {}, 0
        for k, n in zip(self.keys, sizes):
            self.static[k] = self.flat[off:off + n].view(self.shapes[k])
            off += n
        self._stage(example)
        self._capture(warmup)

    def _stage(self, batch):
        parts = []
        for k in self.keys:
            v = batch[k]
            if tuple(v.shape) != self.shapes[k]:
                raise ValueError(f"{k}: captured with shape {self.shapes[k]}, got {tuple(v.shape)}")
            parts.append(hip.require_dev_f32(v, k, contiguous=False).reshape(-1))
        torch.cat(parts, out=self.flat)  # one launch for all inputs

    def _param_ptrs(self):
        return tuple(t.data_ptr() if t is not None else 0 for t in self.model._runtime()._live_params())

    def _capture(self, warmup):
        dev, rt = self.dev, self.model._runtime()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(max(1, warmup)):  # allocates this stream's workspace, packs the weights
                self.model.refine(self.static, n_iter=self.n_iter)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, stream=side, capture_error_mode="relaxed"):
            self.out = self.model.refine(self.static, n_iter=self.n_iter)
        # the scratch buffer the captured kernels point at: owned here, whatever the runtime's per-stream cache does
        self._ws = rt._ws.get((dev.index, side.cuda_stream))
        self._packed = rt._packed
        # the packs the captured chain reads (its compute mode is fixed at capture: the fp16 one reads packs outside PACK_ALL)
        self._sel = rt._refine_packs(self.model._inference_opts())
        self._ptrs = self._param_ptrs()
        self._side = side

    @torch.no_grad()
    def __call__(self, batch):
        rt = self.model._runtime()
        with torch.cuda.device(self.dev):
            rt.params(self.dev, self._sel)  # stale packed weights are re-packed in place, stream-ordered before the replay
            if rt._packed is not self._packed or self._param_ptrs() != self._ptrs:
                self._capture(1)  # parameters moved: the captured pointers are stale
            self._stage(batch)
            self.graph.replay()
        return self.out
