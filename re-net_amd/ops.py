"""torch.autograd glue around the C-ABI kernels (renet_hip.py).  Each Function's forward AND backward
run hand-written HIP kernels; torch only owns the tensors and wires the graph.  No CPU / eager
fallback exists: on a non-HIP tensor these raise."""
import contextlib
import threading
import functools
import ctypes
import os

import numpy as np
import torch
from torch.autograd import Function

import renet_hip as K

_seed_state = {'counter': 0}

# A second HIP stream inside ONE autograd Function: independent kernel chains of a Function (the relation head next
# to the entity head, encoder_r's GEMMs next to encoder's, a bandwidth-bound bias column sum next to the matrix-bound
# GEMMs that read the same gradient) are enqueued on two streams between a fork and a join, so that the tail wave of
# one launch and the few-workgroup kernels of the small chain fill the CUs the other leaves idle.  Fork and join both
# lie inside the Function: everything outside sees plain stream order.  Memory: a tensor allocated under the side
# stream is only ever written there after a later fork (which orders the side stream behind every main-stream
# consumer enqueued so far), and the inputs the side chain reads stay referenced by the caller until after the join.
# RENET_SIDE_STREAM=0, or kernel timing (K.set_timer: per-kernel events want serial launches), keeps one stream.
SIDE_STREAM = os.environ.get('RENET_SIDE_STREAM', '1') != '0'
_side_streams = {}


class _Side(object):
    def __init__(self, device):
        self.on = SIDE_STREAM and device.type == 'cuda' and K._timer is None
        if self.on:
            key = device.index if device.index is not None else torch.cuda.current_device()
            if key not in _side_streams:
                _side_streams[key] = torch.cuda.Stream(device=device)
            self.main = torch.cuda.current_stream(device)
            self.side = _side_streams[key]
            self.side.wait_stream(self.main)                       # fork

    def __call__(self):
        return torch.cuda.stream(self.side) if self.on else contextlib.nullcontext()

    def join(self):
        if self.on:
            self.main.wait_stream(self.side)


# Deferred joins (round 4).  Some side-stream work has no consumer inside the backward pass at all -- the weight / bias
# gradients of the GRU input projections and recurrences feed nothing but the optimizer -- so its join can wait until
# the optimizer step instead of the end of the Function: the main stream goes on into sequence-assembly and RGCN
# backward (~0.5 ms of small, latency-bound kernels) while the side stream runs the dW GEMMs.  Only a caller that
# PROMISES the final join may turn this on: parallel.HipAdam's step_scope sets `DEFER_WEIGHT_GRADS` for the step and
# HipAdam.step() calls join_deferred() before it reads a gradient.  Outside such a scope (train.py's own loop with
# clip_grad_norm_ + torch Adam) every Function joins before it returns, as before.  Tensors the deferred kernels read
# are handed to the allocator with record_stream, so that freeing them on the main stream cannot recycle their memory
# under the side stream -- and EVERYTHING the deferred kernels read (those tensors, the batch graph with its index arrays and
# item plans, operand shells with their bound partials) is also kept alive by a strong reference in `_deferred` until
# join_deferred() has made the main stream wait: a caller that drops `loss` or the prepared batch between backward() and
# step() cannot let the allocator recycle memory the side stream is still reading.
DEFER_WEIGHT_GRADS = False
_deferred = []             # (main stream, side stream, keep-alive objects) of un-joined side work


def _deferred_scope(device, tensors, keep=()):
    """-> a _Side whose stream takes gradient-only work that stays UN-JOINED until join_deferred() (None when deferral
    is off or no side stream exists).  `tensors`: what that work reads and the caller frees afterwards; `keep`: further
    objects (the DeviceGraph, operand shells) whose device memory the work reads."""
    if not DEFER_WEIGHT_GRADS:
        return None
    sd = _Side(device)
    if not sd.on:
        return None
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            t.record_stream(sd.side)
    _deferred.append((sd.main, sd.side, (list(tensors), list(keep))))
    return sd


def join_deferred():
    """Make every stream that forked deferred work wait for it (no-op if nothing is pending); the kept objects are
    released after the wait has been enqueued (their memory returns to the allocator on the main stream, behind it)."""
    while _deferred:
        main, side, keep = _deferred.pop()
        main.wait_stream(side)
        del keep


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0


# Exact data-parallel split of ONE batch (graph.shard_sequences, bench --scaling exact): every rank evaluates the SAME
# batch graph, so the dropout masks of the graph-side sites (the RGCN layers' self-loop dropout) must be the same on
# every rank for the N-rank step to equal the 1-rank step; the per-sequence sites (sequence assembly, score heads) act
# on rows only this rank owns and keep rank-dependent seeds.  Set by the caller that shards a batch that way.
SHARED_GRAPH_SEEDS = False       # process default; a sharded batch sets it for ITS forward pass only (shared_graph_seeds)
_shared_tls = threading.local()  # .flag: the scope's value on THIS thread (seeds are drawn in forward, on the caller's thread)


@contextlib.contextmanager
def shared_graph_seeds(flag):
    """Forward pass of a batch whose GRAPH is replicated on every rank (RENet.loss_prepared_both on a batch prepared
    with shard=(rank, world)): the graph-side dropout sites draw rank-independent seeds inside this scope.  Seeds are
    only drawn in forward (the backward pass replays them from ctx), so a scope around the forward call suffices; the
    flag travels with the prepared batch instead of a module global that a caller has to set per step (review r3)."""
    old = getattr(_shared_tls, 'flag', None)
    _shared_tls.flag = bool(flag)
    try:
        yield
    finally:
        _shared_tls.flag = old


def next_seed(graph_site=False):
    """Fresh 63-bit seed for one dropout site, derived from torch's global seed (train.py:31 seeds it), the
    data-parallel rank (every rank runs with the same torch seed, and identical masks on every rank would
    correlate the ranks' dropout noise) and a per-process site counter.  graph_site: a site on the batch GRAPH --
    rank-independent when the ranks replicate one graph (SHARED_GRAPH_SEEDS)."""
    _seed_state['counter'] += 1
    scoped = getattr(_shared_tls, 'flag', None)
    shared = SHARED_GRAPH_SEEDS if scoped is None else scoped
    rank = 0 if (graph_site and shared) else _rank()
    x = torch.initial_seed() * 0x9E3779B1 + (rank + 1) * 0xC2B2AE3D27D4EB4F + _seed_state['counter'] * 0x85EBCA77
    return x & 0x7FFFFFFFFFFFFFFF


def reset_seed_counter(value=0):
    """Restart the per-process dropout site counter (reproducible runs: call next to torch.manual_seed)."""
    _seed_state['counter'] = int(value)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# When a parameter already owns a persistent .grad buffer (parallel.FlatGrads / zero_grad(set_to_none=False)),
# the backward kernels accumulate STRAIGHT into it (GEMM beta=1, segmented scatter-add) and return None for
# that input, instead of materialising a full-size gradient tensor that autograd then adds: for ent_embeds
# (4 uses per direction, 18 MB each) and linear.weight (55 MB) that removes ~45 add/fill kernels per step.
INPLACE_GRADS = True

# Registered by parallel.HipAdam when gradients are exchanged between ranks: callbacks keyed by PARAMETER identity,
# called with the parameter right after a Function accumulated its contribution into param.grad in place (the score
# head's weight and bias), so that the all-reduce of that bucket can start while the rest of the backward pass runs.
# A registry, not one global slot: two optimizers (RENet + RENet_global, tests) each keep their own hooks, and
# unregister_grad_done_hook releases everything the callback keeps alive.
_grad_done_hooks = {}          # id(param) -> {token: callback}
_hook_tokens = {'next': 0}


_hook_wanted = {}              # token -> predicate: does this hook want notifications right now (None: always)


def register_grad_done_hook(params, callback, wanted=None):
    """wanted: optional callable() -> bool; callers that pay for a notification (events, a hook stream: step_plan.StepFn) ask
    hooks_wanted(param) first -- the reducer of a process without a process group wants none."""
    _hook_tokens['next'] += 1
    token = _hook_tokens['next']
    for p in params:
        _grad_done_hooks.setdefault(id(p), {})[token] = callback
    _hook_wanted[token] = wanted
    return token


def hooks_wanted(param):
    cbs = _grad_done_hooks.get(id(param))
    if not cbs:
        return False
    for token in cbs:
        w = _hook_wanted.get(token)
        if w is None or w():
            return True
    return False


def unregister_grad_done_hook(token):
    _hook_wanted.pop(token, None)
    for pid in list(_grad_done_hooks):
        _grad_done_hooks[pid].pop(token, None)
        if not _grad_done_hooks[pid]:
            del _grad_done_hooks[pid]


def grad_done(param):
    cbs = _grad_done_hooks.get(id(param))
    if cbs:
        for cb in list(cbs.values()):
            cb(param)

# Test hook (tests/test_gpu_config.py): when set to a callable(name, tensor), the training path reports its
# internal activations (GRU final states, entity logits before the in-place CE) -- None in production.
debug_tap = None


def _fwd_mode(fwd):
    """Function.forward wrapper: remembers the GEMM mode the forward pass ran in (renet_hip.gemm_mode scopes are entered
    by the MODEL around its forward code; autograd runs backward later, on its own thread, outside any such scope)."""
    @functools.wraps(fwd)
    def forward(ctx, *a, **k):
        ctx.gemm_mode = K.current_mode()
        return fwd(ctx, *a, **k)
    return forward


def _bwd_mode(bwd):
    """Function.backward wrapper: runs the backward pass in the mode its forward pass ran in."""
    @functools.wraps(bwd)
    def backward(ctx, *g):
        with K.gemm_mode(getattr(ctx, 'gemm_mode', None)):
            return bwd(ctx, *g)
    return backward


def grad_target(t):
    """The slice of a leaf parameter's existing .grad that corresponds to tensor `t` (the parameter itself or
    a contiguous row-slice view of it), or None if there is nothing to accumulate into.
    Always called from BACKWARD (the Functions keep `t` on ctx, not the resolved buffer): a loop that calls
    zero_grad(set_to_none=True) or replaces .grad between forward and backward must not leave the kernels
    accumulating into an orphaned tensor -- with .grad gone the Functions fall back to returning a
    materialised gradient and autograd sets .grad as usual."""
    if not INPLACE_GRADS or t is None:
        return None
    base = t if t.is_leaf else getattr(t, '_base', None)
    if base is None or not base.is_leaf or not base.requires_grad or base.grad is None:
        return None
    if not base.grad.is_contiguous() or base.grad.shape != base.shape:
        return None
    if t is base:
        return base.grad
    if t.dim() == 2 and base.dim() == 2 and t.is_contiguous() and t.shape[1] == base.shape[1]:
        off = t.storage_offset() - base.storage_offset()
        if off >= 0 and off % base.shape[1] == 0:
            r0 = off // base.shape[1]
            return base.grad[r0:r0 + t.shape[0]]
    return None


# The three forms of "accumulate into the parameter's .grad slice and hand autograd None, else return a fresh gradient":
def _gemm_grad(a, b, tgt):
    """a^T @ b (auto split-K): accumulated into tgt (beta = 1) -> None, or -> the product."""
    if tgt is not None:
        K.gemm(a, b, ta=True, out=tgt, beta=1.0)
        return None
    return K.gemm(a, b, ta=True)


def _colsum_grad(x, tgt):
    """Column sums of x: accumulated into tgt -> None, or -> the sums."""
    if tgt is not None:
        K.colsum(x, out=tgt, beta=1.0)
        return None
    return K.colsum(x)


def _segment_grad(src, plan, tgt, shape):
    """Segment sums of src's rows (K.segment_add): added to tgt -> None, or -> zeros of `shape` plus the sums."""
    if tgt is not None:
        K.segment_add(src, plan, tgt)
        return None
    d = torch.zeros(shape, device=src.device, dtype=torch.float32)
    K.segment_add(src, plan, d)
    return d


class GatherRowsFn(Function):
    """out = table[idx]  (utils.py:239 h0 = ent_embeds[id]); backward = deterministic segmented add."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, table, idx, plan):
        ctx.plan, ctx.shape, ctx.src = plan, table.shape, table
        return K.gather_rows(_c(table), idx)

    @staticmethod
    @_bwd_mode
    def backward(ctx, g):
        return _segment_grad(_c(g), ctx.plan, grad_target(ctx.src), ctx.shape), None, None


class RGCNLayerFn(Function):
    """One RGCNBlockLayer (RGCN.py:33-51,79-94): self-loop GEMM + fused gather-SpMM epilogue.
    n_out < N evaluates the layer only for the first n_out rows (the batch builder numbers the rows that
    are read afterwards -- the subject rows, Aggregator.py:139-140 -- first); exact for those rows."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, h, weight, loop_weight, g, reverse, relu, drop_p, seed, n_out):
        ctx.src_w, ctx.src_loop = weight, loop_weight
        h, weight, loop_weight = _c(h), _c(weight), _c(loop_weight)
        n = h.shape[0]
        n_out = n if (n_out is None or n_out >= n) else int(n_out)
        pruned = n_out < n
        shift = g.num_types // 2 if reverse else 0                     # type_o = type_s +- R (utils.py:75-76)
        h_op = K.operand(h[:n_out])                                    # (bf16 mode: packed once, reused by backward)
        out = K.gemm(h_op, loop_weight)                                # RGCN.py:35
        K.rgcn_gather_items(h, g, weight, shift, False, out, drop_p, seed, relu, out, use_norm=True, pruned=pruned,
                            w16=K.gather_weight_bf16(weight))
        ctx.g, ctx.relu, ctx.drop_p, ctx.seed, ctx.shift, ctx.n_out = g, relu, drop_p, seed, shift, n_out
        ctx.h_op = h_op if K.is_handle(h_op) else None
        ctx.save_for_backward(h, weight, loop_weight, out)
        return out

    @staticmethod
    @_bwd_mode
    def backward(ctx, g_out):
        h, weight, loop_weight, out = ctx.saved_tensors
        g, n_out = ctx.g, ctx.n_out
        tgt_loop, tgt_w = grad_target(ctx.src_loop), grad_target(ctx.src_w)
        g_out = _c(g_out)
        n, d = h.shape
        pruned = n_out < n
        gn = torch.empty(n_out, d, device=h.device, dtype=torch.float32)
        g_loop = torch.empty(n_out, d, device=h.device, dtype=torch.float32)
        K.rgcn_bwd_prep(g_out, out, g.norm, ctx.relu, ctx.drop_p, ctx.seed, gn, g_loop)
        dh = torch.empty(n, d, device=h.device, dtype=torch.float32)
        # dh = sum over out-edges W[type]^T gn[dst]  == same CSR rows, the PAIRED edge's type; with a pruned
        # forward only destinations < n_out carry gradient: skip the other sources.  Launched right behind the
        # kernel that produced gn (still cache resident); the self-loop term is then ACCUMULATED by its GEMM
        # (beta = 1, rows < n_out): the matrix-bound GEMM hides the read of dh that the bandwidth-bound gather
        # would otherwise pay for as an addend (64 -> 76 us per launch on the merged batch).
        pair_shift = (ctx.shift + g.num_types // 2) % g.num_types
        K.rgcn_gather_items(gn, g, weight, pair_shift, True, None, 0.0, 0, False, dh, use_norm=False, pruned=pruned,
                            src_limit=n_out if pruned else 0, w16=K.gather_weight_bf16(weight))
        gl_op = K.operand(g_loop)
        h_op = ctx.h_op if ctx.h_op is not None else h[:n_out]
        K.gemm(gl_op, loop_weight, tb=True, out=dh[:n_out], beta=1.0)      # += g_loop @ W_loop^T (rows < n_out)
        acc = tgt_w is not None                                        # straight into weight.grad (beta = 1)
        d_w = tgt_w if acc else torch.empty_like(weight)

        def weight_grads():
            if pruned:
                K.rgcn_bwd_w(h, gn, g.e_src2, g.e_dst2, g.chunk_ptr2, g.chunk_type2, g.n_chunks2, g.type_chunk_ptr2,
                             g.num_types, ctx.shift, d_w, beta=1.0 if acc else 0.0)
            else:
                K.rgcn_bwd_w(h, gn, g.e_src, g.e_dst, g.chunk_ptr, g.chunk_type, g.n_chunks, g.type_chunk_ptr,
                             g.num_types, ctx.shift, d_w, beta=1.0 if acc else 0.0)
            return _gemm_grad(h_op, gl_op, tgt_loop)                   # h^T @ g_loop
        # the relation-block and self-loop weight gradients feed only the optimizer, and nothing else writes their
        # buffers: inside a declared step they run on the side stream, un-joined, under the rest of the backward pass
        sd = _deferred_scope(h.device, (h, gn, g_loop, getattr(gl_op, 'p', None), getattr(gl_op, 'part', None),
                                        getattr(h_op, 'p', None), getattr(h_op, 'part', None), getattr(h_op, 't', None),
                                        getattr(gl_op, 't', None)), keep=(g, h_op, gl_op, weight_grads)) \
            if (acc and tgt_loop is not None and K.current_mode() != 'bf16s') else None
        if sd is not None:
            if isinstance(gl_op, K.F32Op):
                gl_op.bound()                                          # (measured on this stream: before the fork below)
            if isinstance(h_op, K.F32Op):
                h_op.bound()
            sd.side.wait_stream(sd.main)
            with sd():
                weight_grads()
            d_loop = None
        else:
            d_loop = weight_grads()
        return dh, None if acc else d_w, d_loop, None, None, None, None, None, None


class TableRows(object):
    """Deferred `table[idx]` (utils.py:239: h0 = ent_embeds[id]): handed to the first RGCN layer as g.ndata['h'], which
    then reads the entity table through idx instead of a materialised [N, D] copy (RGCNTableLayerFn)."""
    __slots__ = ('table', 'idx', 'plan')

    def __init__(self, table, idx, plan):
        self.table, self.idx, self.plan = table, idx, plan

    def materialise(self):
        return GatherRowsFn.apply(self.table, self.idx, self.plan)


class RGCNTableLayerFn(Function):
    """The FIRST RGCNBlockLayer of a pass (RGCN.py:33-51,79-94 on h0 = ent_embeds[id], utils.py:239) without ever
    materialising h0: h0 @ W_loop == (ent_embeds @ W_loop)[id], so the self-loop GEMM runs on the N_ent rows of the
    entity table (23 k at ICEWS18 sizes) instead of the N rows of the batch graph (92 k on the merged batch), and the
    gather-SpMM reads its source rows and its addend through g.node_ent from the two [N_ent, D] tables (18 MB each:
    cache resident) -- renet_rgcn_gather_items_table.  Backward: the transposed gather on the [N, D] gradient as in
    RGCNLayerFn, then ONE reduction to entity rows: d_ent += segsum(dh) + segsum(g_loop) @ W_loop^T and
    dW_loop = ent^T @ segsum(g_loop) -- again GEMMs over N_ent rows."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, table, weight, loop_weight, g, reverse, relu, drop_p, seed):
        ctx.src_tab, ctx.src_w, ctx.src_loop = table, weight, loop_weight
        table, weight, loop_weight = _c(table), _c(weight), _c(loop_weight)
        shift = g.num_types // 2 if reverse else 0
        ew = K.gemm(table, loop_weight)                               # RGCN.py:35 on the entity table
        out = torch.empty(g.N, table.shape[1], device=table.device, dtype=torch.float32)
        K.rgcn_gather_items_table(table, g, weight, shift, ew, drop_p, seed, relu, out,
                                  table16=K.gather_weight_bf16(table), w16=K.gather_weight_bf16(weight))
        ctx.g, ctx.relu, ctx.drop_p, ctx.seed, ctx.shift = g, relu, drop_p, seed, shift
        ctx.save_for_backward(table, weight, loop_weight, out)
        return out

    @staticmethod
    @_bwd_mode
    def backward(ctx, g_out):
        table, weight, loop_weight, out = ctx.saved_tensors
        g = ctx.g
        tgt_tab, tgt_loop, tgt_w = grad_target(ctx.src_tab), grad_target(ctx.src_loop), grad_target(ctx.src_w)
        g_out = _c(g_out)
        n, d = out.shape
        dev = out.device
        gn = torch.empty(n, d, device=dev, dtype=torch.float32)
        g_loop = torch.empty(n, d, device=dev, dtype=torch.float32)
        K.rgcn_bwd_prep(g_out, out, g.norm, ctx.relu, ctx.drop_p, ctx.seed, gn, g_loop)
        dh = torch.empty(n, d, device=dev, dtype=torch.float32)
        pair_shift = (ctx.shift + g.num_types // 2) % g.num_types
        K.rgcn_gather_items(gn, g, weight, pair_shift, True, None, 0.0, 0, False, dh, use_norm=False,
                            w16=K.gather_weight_bf16(weight))
        acc = tgt_w is not None
        d_w = tgt_w if acc else torch.empty_like(weight)
        e_src_t = g.table_items()[3]
        sd = _deferred_scope(dev, (gn, e_src_t), keep=(g, table)) if acc else None      # (see RGCNLayerFn.backward)
        with (sd() if sd is not None else contextlib.nullcontext()):
            K.rgcn_bwd_w(table, gn, e_src_t, g.e_dst, g.chunk_ptr, g.chunk_type, g.n_chunks, g.type_chunk_ptr,
                         g.num_types, ctx.shift, d_w, beta=1.0 if acc else 0.0)
        # per-entity sums of the self-loop gradient, then the two self-loop GEMMs on N_ent rows
        gs = torch.zeros(table.shape, device=dev, dtype=torch.float32)
        d_tab = tgt_tab if tgt_tab is not None else torch.zeros(table.shape, device=dev, dtype=torch.float32)
        K.segment_add2(dh, g_loop, g.plan_node_ent, d_tab, gs)
        gs_op = K.operand(gs)
        K.gemm(gs_op, loop_weight, tb=True, out=d_tab, beta=1.0)          # += segsum(g_loop) @ W_loop^T
        d_loop = _gemm_grad(table, gs_op, tgt_loop)
        return (None if tgt_tab is not None else d_tab), None if acc else d_w, d_loop, None, None, None, None, None


class SeqAssembleFn(Function):
    """Aggregator.py:139-165: packed GRU inputs X [S,4D], Xr [S,3D] with fused dropout."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, h2, ent, rel, glob, g, drop_p, seed_x, seed_xr, _lazy_bf16=False):
        ctx.src_ent, ctx.src_rel = ent, rel
        h2, ent, rel, glob = _c(h2), _c(ent), _c(rel), _c(glob)
        if _lazy_bf16 and K.current_mode() == 'bf16s':
            # bf16-storage mode, internal callers only (RENet.loss_prepared*): X / Xr exist ONLY as bf16 operand
            # matrices; the fp32 tensors returned to autograd are uninitialised shells that carry them (K.operand
            # picks the attribute up) -- their values must never be read
            mx, mxr = K.seq_assemble_fwd_bf16(h2, ent, rel, glob, g.subj_row, g.row_ent, g.row_rel, g.glob_row,
                                              drop_p, seed_x, seed_xr)
            x, xr = K.lazy_shell(mx, h2.device), K.lazy_shell(mxr, h2.device)
        else:
            x, xr = K.seq_assemble_fwd(h2, ent, rel, glob, g.subj_row, g.row_ent, g.row_rel, g.glob_row,
                                       drop_p, seed_x, seed_xr)
        ctx.g, ctx.drop_p, ctx.seeds = g, drop_p, (seed_x, seed_xr)
        ctx.shapes = (h2.shape, ent.shape, rel.shape)
        return x, xr

    @staticmethod
    @_bwd_mode
    def backward(ctx, dx, dxr):
        g = ctx.g
        d = ctx.shapes[0][1]
        tgt_ent, tgt_rel = grad_target(ctx.src_ent), grad_target(ctx.src_rel)
        d_rows, d_ent_seq, d_rel_seq = K.seq_assemble_bwd(_c(dx), _c(dxr), g.step_off, g.L, g.B, d, ctx.drop_p,
                                                          *ctx.seeds)
        d_h2 = _segment_grad(d_rows, g.plan_subj_row, None, ctx.shapes[0])
        d_ent = _segment_grad(d_ent_seq, g.plan_s, tgt_ent, ctx.shapes[1])       # per-sequence sums, keyed by s[perm]
        d_rel = _segment_grad(d_rel_seq, g.plan_r, tgt_rel, ctx.shapes[2])
        return d_h2, d_ent, d_rel, None, None, None, None, None, None


class GRUFn(Function):
    """nn.GRU (1 layer, h0 = 0) on a packed sequence, returning h_n zero-padded to `total_rows`
    (model.py:86-88).  x: [S, I] packed time-major; step_off: ctypes int32[L+1] on the host."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, step_off, total_rows):
        x, w_ih, w_hh, b_ih, b_hh = _c(x), _c(w_ih), _c(w_hh), _c(b_ih), _c(b_hh)
        hdim = w_hh.shape[1]
        gi = K.gemm(x, w_ih, tb=True, bias=b_ih)                         # [S, 3H]
        full, saved = K.gru_fwd(gi, step_off, hdim, w_hh, b_hh, out_rows=total_rows)     # zero rows past nnz
        nnz = int(step_off[1] - step_off[0]) if len(step_off) > 1 else 0
        ctx.step_off, ctx.nnz, ctx.hdim = step_off, nnz, hdim
        ctx.save_for_backward(x, w_ih, w_hh, saved)
        return full.unsqueeze(0)                 # h_n layout of nn.GRU: [1, B, H]

    @staticmethod
    @_bwd_mode
    def backward(ctx, dh):
        x, w_ih, w_hh, saved = ctx.saved_tensors
        hdim, nnz = ctx.hdim, ctx.nnz
        dh_last = _c(dh[0, :nnz])
        d_gi, d_gh = K.gru_bwd(dh_last, ctx.step_off, hdim, w_hh, saved)
        s = x.shape[0]
        dx = K.gemm(d_gi, w_ih)                                          # [S, I]
        d_wih = K.gemm(d_gi, x, ta=True)
        d_bih = K.colsum(d_gi)
        h_prev = saved[:, 4 * hdim:]
        d_whh = K.gemm(d_gh, h_prev, ta=True)
        d_bhh = K.colsum(d_gh)
        return dx, d_wih, d_whh, d_bih, d_bhh, None, None


class MultiGRUFn(Function):
    """n <= 4 of RE-Net's history encoders in ONE persistent launch per direction of time (model.py:86,94):
    `encoder` (4D->D) and `encoder_r` (3D->D) of one pass share a packed layout; the subject and the object pass of
    a training step are independent until their losses are added, so a step may run all four side by side
    (RENet.loss_prepared_pair).  Input projections are one GEMM per problem.
    apply(step_offs, total_rows, live_cols, x_0, w_ih_0, w_hh_0, b_ih_0, b_hh_0, x_1, ...) -> (h_n_0 [1, rows_0, H], ...)
    live_cols: None, or per problem the number of leading columns of dX the caller reads (None = all)."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, step_offs, total_rows, live_cols, *ts):
        n = len(ts) // 5
        ctx.live_cols = live_cols
        ctx.src_w = [(ts[5 * k + 1], ts[5 * k + 2]) for k in range(n)]
        ctx.src_b = [(ts[5 * k + 3], ts[5 * k + 4]) for k in range(n)]
        ts = [_c(t) for t in ts]
        xs, w_ihs, w_hhs = ts[0::5], ts[1::5], ts[2::5]
        b_ihs, b_hhs = ts[3::5], ts[4::5]
        hdim = w_hhs[0].shape[1]
        x_ops = [K.operand(x) for x in xs]                              # (bf16 mode: packed once, reused by dW_ih)
        # the input projections of the problems are independent: odd problems on the side stream (_Side)
        sd = _Side(xs[0].device)
        gis = [None] * n
        with sd():
            for k in range(1, n, 2):
                gis[k] = K.gemm(x_ops[k], w_ihs[k], tb=True, bias=b_ihs[k])
        for k in range(0, n, 2):
            gis[k] = K.gemm(x_ops[k], w_ihs[k], tb=True, bias=b_ihs[k])
        sd.join()
        ctx.x_ops = x_ops if any(K.is_handle(x) for x in x_ops) else None
        hs, svs = K.gru_fwd_layouts(gis, step_offs, hdim, w_hhs, b_hhs, total_rows)     # rows past nnz are zero
        ctx.step_offs, ctx.hdim, ctx.n = step_offs, hdim, n
        ctx.nnz = [int(o[1] - o[0]) if len(o) > 1 else 0 for o in step_offs]
        ctx.save_for_backward(*(list(xs) + list(w_ihs) + list(w_hhs) + list(svs)))
        if debug_tap is not None:
            for k, h in enumerate(hs):
                debug_tap('h_n' if k % 2 == 0 else 'q_n', h)
        return tuple(h.unsqueeze(0) for h in hs)

    @staticmethod
    @_bwd_mode
    def backward(ctx, *dhs):
        n, hdim = ctx.n, ctx.hdim
        sv_ = ctx.saved_tensors
        xs, w_ihs, w_hhs, svs = sv_[:n], sv_[n:2 * n], sv_[2 * n:3 * n], sv_[3 * n:4 * n]
        d_gis, d_ghs = K.gru_bwd_layouts([_c(dh[0, :nz]) for dh, nz in zip(dhs, ctx.nnz)], ctx.step_offs, hdim,
                                         list(w_hhs), list(svs), out_bf16=(K.current_mode() == 'bf16s'))
        def param_grads(k, dgi_op):
            """dW_ih, dW_hh, db_ih, db_hh of problem k: consumed by the optimizer only."""
            t_ih, t_hh = (grad_target(t) for t in ctx.src_w[k])
            t_bi, t_bh = (grad_target(t) for t in ctx.src_b[k])
            dgi, dgh, xx, s_ = d_gis[k], d_ghs[k], xs[k], svs[k]
            x_op = ctx.x_ops[k] if ctx.x_ops is not None else xx
            dwi = _gemm_grad(dgi_op, x_op, t_ih)
            # |dGh| <= |dGi| elementwise (equal but for the n gate's factor r in (0, 1)) and |h| <= 1: both operand
            # bounds of the f16x3 GEMM are known without a pass over the tensors
            dgh_op = K.operand_like(dgh, dgi_op)
            hp_op = K.operand(s_[:, 4 * hdim:], bound=K.const_bound(1.0, s_.device))
            return [dwi, _gemm_grad(dgh_op, hp_op, t_hh), _colsum_grad(dgi, t_bi), _colsum_grad(dgh, t_bh)]

        def input_grad(k, dgi_op):
            xx = xs[k]
            live = ctx.live_cols[k] if ctx.live_cols is not None else None
            if live is not None and live < xx.shape[1]:
                # the caller never reads dX beyond column `live` (RE-Net: the last D input columns are the global
                # embedding, a constant, Aggregator.py:150-155): contract only the live columns of W_ih; the rest
                # of dX stays unwritten
                dxx = torch.empty_like(xx)
                K.gemm(dgi_op, w_ihs[k][:, :live], out=dxx[:, :live])
                dxx[:, live:].zero_()         # defined values for any other consumer (hooks, detect_anomaly): 6 MB
                return dxx
            return K.gemm(dgi_op, w_ihs[k])

        def problem(k):
            dgi_op = K.operand(d_gis[k])                               # consumed by dW_ih and dX
            return [input_grad(k, dgi_op)] + param_grads(k, dgi_op)

        all_in_place = all(grad_target(t) is not None for k in range(n) for t in ctx.src_w[k] + ctx.src_b[k])
        sd0 = _Side(d_gis[0].device if not isinstance(d_gis[0], K.BF16Mat) else d_gis[0].p.device)
        if DEFER_WEIGHT_GRADS and sd0.on and all_in_place and K.current_mode() != 'bf16s':
            # every parameter gradient accumulates in place and somebody joins before the optimizer reads it: dX of all
            # problems on this stream (what the rest of the backward pass waits for), all parameter gradients on the side
            # stream, NOT joined here
            ops_ = [K.operand(d_gis[k]) for k in range(n)]
            if K.current_mode() == 'f16x3':
                for o in ops_:
                    o.bound()                                          # measured on THIS stream, before the fork
            sd = _Side(sd0.main.device)                                # (fork: the side stream sees d_gis / bounds)
            res = [None] * n
            with sd():
                for k in range(n):
                    param_grads(k, ops_[k])
                _gru_grads_done(ctx)                                   # (on the side stream: the reducer orders behind it)
            live_ops = ops_ + (list(ctx.x_ops) if ctx.x_ops is not None else [])
            for t in list(d_gis) + list(d_ghs) + list(xs) + list(svs) + \
                    [getattr(o, 'part', None) for o in live_ops] + [getattr(o, 't', None) for o in live_ops]:
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(sd.side)
            for k in range(n):
                res[k] = [input_grad(k, ops_[k]), None, None, None, None]
            _deferred.append((sd.main, sd.side, (list(d_gis), list(d_ghs), list(xs), list(svs), live_ops)))
            out = [None, None, None]
            for k in range(n):
                out += res[k]
            return tuple(out)

        # problems with DIFFERENT parameters are independent of each other (encoder / encoder_r; two problems of the
        # same encoder accumulate into the same gradient buffers and stay on one stream): the second parameter set's
        # problems go to the side stream
        keys = [id(ctx.src_w[k][0]) for k in range(n)]
        uniq = list(dict.fromkeys(keys))
        on_side = [len(uniq) > 1 and keys[k] == uniq[1] for k in range(n)]
        res = [None] * n
        sd = sd0
        with sd():
            for k in range(n):
                if on_side[k]:
                    res[k] = problem(k)
        for k in range(n):
            if not on_side[k]:
                res[k] = problem(k)
        sd.join()
        if all_in_place:
            _gru_grads_done(ctx)
        out = [None, None, None]
        for k in range(n):
            out += res[k]
        return tuple(out)


def _gru_grads_done(ctx):
    """MultiGRUFn.backward accumulated into every encoder parameter's .grad: tell whoever registered (the reducer's middle
    bucket).  A parameter shared by two problems of one call (the subject / object pair) is reported once per problem."""
    if not _grad_done_hooks:
        return
    for k in range(len(ctx.src_w)):
        for t in list(ctx.src_w[k]) + list(ctx.src_b[k]):
            grad_done(t)


def dual_gru(x, xr, enc, enc_r, step_off, total_rows):
    """Both encoders of ONE pass: -> (h_n [1, rows, H], q_n [1, rows, H]).  x = [h2 | ent | rel | glob] and
    xr = [h2 | ent | glob] come from SeqAssembleFn, whose backward reads every column but the trailing glob block."""
    h = enc.weight_hh_l0.shape[1]
    return MultiGRUFn.apply([step_off, step_off], [total_rows, total_rows], [x.shape[1] - h, xr.shape[1] - h],
                            x, enc.weight_ih_l0, enc.weight_hh_l0, enc.bias_ih_l0, enc.bias_hh_l0,
                            xr, enc_r.weight_ih_l0, enc_r.weight_hh_l0, enc_r.bias_ih_l0, enc_r.bias_hh_l0)


def _head_forward(a, ia, hmid, c, ic, weight, bias, target, drop_p, seed, grad_scale, need_grad, row_loss=None, copy=None,
                  event=None):
    """One score head up to the per-row losses: [a[ia] | hmid | c[ic]] -> dropout -> Linear -> CE.
    -> (row_loss[B], feat, logits-or-gradient buffer, bf16 / planes gradient matrix or None, operand handle of feat or None,
    d_a or None).  copy = (a_row, q_row), fp32 device [B]: the loss goes THROUGH THE COPY MIX of the recurrence prior,
    row_loss = -log((1 - a) softmax[gold] + a q) (K.mix_ce_planes / K.mix_ce in the CE's place: the same gradient buffers,
    every row scaled by its s <= 1, so the f16x3 bound grad_scale stays valid) and d_a[B] = grad_scale * d row_loss / d a.
    event = (a_row, q_row, lp): the loss goes through the JOINT mix instead (K.joint_mix_ce_planes / K.joint_mix_ce),
    row_loss = -log((1 - a) softmax[gold] exp(lp) + a q); lp is a callable, called once the logits exist and right before the
    CE writer, that returns the other head's log-probability of its gold class (fp32 [B]) -- the caller joins that head's
    stream in it.  The tuple then ends with s_row[B], the scalar of every row."""
    if copy is not None and event is not None:
        raise ValueError('copy= and event= are two different losses: give one of them')
    if (copy is not None or event is not None) and K.current_mode() == 'bf16s':
        raise ValueError('the loss through the copy mix has no bf16-storage writer: use another GEMM mode with copy=')
    feat = K.concat3_fwd(a, ia, hmid, c, ic, drop_p, seed)
    if need_grad and debug_tap is None and K.use_planes(weight, weight.shape[0]):
        # PLANES path (round 6, the entity head): every operand of the head's three GEMMs is split into its bf16 terms ONCE
        # -- the weight per optimizer step, feat here, the CE gradient by the kernel that computes it -- and the GEMMs run
        # without conversion work (csrc/gemm_planes.hip).  The fp32 logits live in a scratch buffer with 16-byte aligned rows
        # and are dropped after the loss; no fp32 copy of the gradient exists.
        b_, c_ = feat.shape[0], weight.shape[0]
        w_pl = K.weight_planes(weight)
        logits = torch.empty(b_, (c_ + 3) & ~3, device=feat.device, dtype=torch.float32)[:, :c_]
        # feat is split ONCE, with a ones column: dW's GEMM then yields the bias gradient as one more output column
        # (col_out); the logits GEMM reads the same planes with K = 3D (the ones meet the zero k padding of the weight's
        # planes and add exactly 0)
        feat_pl1 = K.pack_planes(feat, ones_col=True)
        K.gemm_planes(K.PlanesMat(feat_pl1.p, feat_pl1.R, feat_pl1.C - 1), w_pl, tb=True, bias=bias, out=logits)
        d_a = None
        if event is not None:
            row_loss, dl_pl, d_a, s_row = K.joint_mix_ce_planes(logits, target, event[0], event[1], event[2](), grad_scale,
                                                                row_loss=row_loss)
            return row_loss, feat, feat.new_empty(0), dl_pl, feat_pl1, d_a, s_row
        if copy is None:
            row_loss, dl_pl = K.softmax_ce_planes(logits, target, grad_scale, row_loss=row_loss)
        else:
            row_loss, dl_pl, d_a = K.mix_ce_planes(logits, target, copy[0], copy[1], grad_scale, row_loss=row_loss)
        return row_loss, feat, feat.new_empty(0), dl_pl, feat_pl1, d_a
    feat_op = K.operand(feat)                                        # (bf16 mode: packed once, reused by dW)
    logits = K.gemm(feat_op, weight, tb=True, bias=bias)             # [B, C]
    if debug_tap is not None:
        debug_tap('logits', logits)
    dl_bf16 = d_a = None
    if event is not None:
        row_loss, d_a, s_row = K.joint_mix_ce(logits, target, event[0], event[1], event[2](), grad_scale, need_grad,
                                              row_loss=row_loss)
        return row_loss, feat, logits, None, (feat_op if K.is_handle(feat_op) else None), d_a, s_row
    if copy is not None:
        row_loss, d_a = K.mix_ce(logits, target, copy[0], copy[1], grad_scale, need_grad, row_loss=row_loss)
    elif need_grad and K.current_mode() == 'bf16s':
        # bf16-storage mode: the gradient is written as a bf16 operand matrix, the fp32 logits are dropped
        row_loss, dl_bf16 = K.softmax_ce_bf16(logits, target, grad_scale, row_loss=row_loss)
        logits = feat.new_empty(0)
    else:
        row_loss = K.softmax_ce(logits, target, grad_scale, need_grad, row_loss=row_loss)
    return row_loss, feat, logits, dl_bf16, (feat_op if K.is_handle(feat_op) else None), d_a


def _scale_ce_gradient(dlogits, g, grad_scale):
    """dlogits *= g (the upstream scalar, device memory) -> the bound |g| * grad_scale on max |dlogits| as a 1-element
    device tensor in f16x3 mode (those GEMMs scale their operands by a bound on the tensor's magnitude; |softmax -
    onehot| <= 1, so this one is known without a pass over the 188 MB), else None."""
    if isinstance(dlogits, K.PlanesMat):
        return None                      # (the planes GEMMs take the upstream scalar as alpha_dev: no pass over the gradient)
    if K.current_mode() == 'f16x3' and not isinstance(dlogits, K.BF16Mat) and dlogits.is_cuda:
        return K.scale_by_device_scalar(dlogits, g, bound_in=float(grad_scale))
    K.scale_by_device_scalar(dlogits, g)
    return None


def _head_backward(dlogits, feat, feat_op, weight, t_w, t_b, bias_side=None, bound=None, g=None):
    """The three gradient products of one score head from its (already scaled) CE gradient -> (dfeat, d_w, d_b).
    bias_side: a _Side whose stream takes the bias column sum (bandwidth bound, next to the matrix-bound GEMMs that
    read the same gradient).  bound: see _scale_ce_gradient.  g: the upstream scalar (device), applied here when the
    gradient arrives as planes (it was NOT scaled then)."""
    if isinstance(dlogits, K.PlanesMat):
        w_pl = K.weight_planes(weight)
        dfeat = K.gemm_planes(dlogits, w_pl, alpha_dev=g)            # [B, parts*D]: contraction over the classes
        # dW and db in ONE product: [C, parts*D | 1] = dl^T @ [feat | 1]
        acc = t_w is not None and t_b is not None
        d_w = t_w if acc else torch.empty_like(weight)
        d_b = t_b if acc else torch.empty(weight.shape[0], device=weight.device, dtype=torch.float32)
        K.gemm_planes(dlogits, feat_op, ta=True, out=d_w, col_out=d_b, alpha_dev=g, beta=1.0 if acc else 0.0)
        return dfeat, (None if acc else d_w), (None if acc else d_b)
    dl_op = K.operand(dlogits, bound=bound)                          # consumed by dfeat and dW
    f_op = feat_op if feat_op is not None else feat

    if bias_side is not None:
        with bias_side():
            d_b = _colsum_grad(dlogits, t_b)
    dfeat = K.gemm(dl_op, weight)                                    # [B, parts*D]
    # (the weight gradient stays BEHIND dfeat on this stream: next to it on the side stream the two chip-filling GEMMs
    # were measured 2 % slower per step than back to back, tools/sessions/r04_s11.sh)
    d_w = _gemm_grad(dl_op, f_op, t_w)
    if bias_side is None:
        d_b = _colsum_grad(dlogits, t_b)
    return dfeat, d_w, d_b


def _consume_ce_gradient(ctx):
    """The saved (softmax - onehot) buffers of a head Function serve ONE backward pass: it scales them in place."""
    if ctx.consumed:
        raise RuntimeError('%s: the saved (softmax - onehot) buffers were scaled in place by the first backward pass; a '
                           'second pass over the same graph is not supported' % type(ctx).__name__)
    ctx.consumed = True


def _scatter_head_rows(da_rows, dc_rows, plan_a, plan_c, t_a, t_c, a_shape, c_shape):
    """Row gradients of a head's gathered inputs a[ia] and c[ic] (dc_rows None: a head without c) -> (d_a, d_c)."""
    d_a = _segment_grad(da_rows, plan_a, t_a, a_shape)
    return d_a, (_segment_grad(dc_rows, plan_c, t_c, c_shape) if dc_rows is not None else None)


class HeadCEFn(Function):
    """model.py:89-91 / 98-100: mean CE( Linear( dropout([a[ia] | hmid | c[ic]]) ), target ).
    The logits never make a second HBM round trip as a separate softmax: the CE kernel turns them
    into (softmax - onehot)/B in place, which the backward GEMMs then consume."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, a, ia, hmid, c, ic, weight, bias, target, plan_a, plan_c, drop_p, seed, loss_scale=1.0, copy_a=None,
                copy_q=None):
        """copy_a / copy_q (both or neither; fp32 [B]): the loss through the copy mix (see _head_forward); copy_a may
        require grad -- a learned gate -- and receives g * d_a; copy_q may require grad -- a learned decay -- and receives
        g * d_q (copy_q_grad), else None.  Neither: today's path, launch for launch."""
        ctx.srcs = (a, c, weight, bias)
        copy = _copy_pair(copy_a, copy_q, hmid.shape[0])
        a, hmid, weight, bias = _c(a), _c(hmid), _c(weight), _c(bias)
        c = _c(c) if c is not None else None
        b, d = hmid.shape
        need_grad = any(ctx.needs_input_grad)
        # loss_scale (2 for the merged batch of both passes: sum of two B-row means = 2 x the 2B-row mean) goes into
        # the gradient the CE kernel writes, so that the upstream scalar stays 1 and the 188 MB are not rescaled
        ctx.grad_scale = float(loss_scale) / b
        row_loss, feat, logits, ctx.dl_bf16, feat_op, ctx.d_gate = _head_forward(
            a, ia, hmid, c, ic, weight, bias, target, drop_p, seed, ctx.grad_scale, need_grad, copy=copy)
        ctx.d_q = copy_q_grad(copy[0], row_loss, ctx.grad_scale) if copy is not None and ctx.needs_input_grad[14] else None
        ctx.meta = (d, 3 if c is not None else 2, drop_p, seed, plan_a, plan_c, a.shape,
                    c.shape if c is not None else None)
        if need_grad:
            ctx.save_for_backward(feat, logits, weight)
            ctx.consumed = False
            ctx.feat_op = feat_op
        return row_loss.mean() if loss_scale == 1.0 else row_loss.mean() * float(loss_scale)

    @staticmethod
    @_bwd_mode
    def backward(ctx, g):
        feat, dlogits, weight = ctx.saved_tensors
        d, parts, drop_p, seed, plan_a, plan_c, a_shape, c_shape = ctx.meta
        t_a, t_c, t_w, t_b = [grad_target(t) for t in ctx.srcs]
        _consume_ce_gradient(ctx)
        # every gradient below is linear in dlogits: fold the upstream scalar (1 for `loss_s + loss_o`, 0.1 for
        # the relation head) into it ONCE, from device memory, instead of scaling three results
        if ctx.dl_bf16 is not None:
            dlogits = ctx.dl_bf16
        bound = _scale_ce_gradient(dlogits, g, ctx.grad_scale)
        sd = _Side(feat.device)
        dfeat, d_w, d_b = _head_backward(dlogits, feat, ctx.feat_op, weight, t_w, t_b, bias_side=sd, bound=bound, g=g)
        sd.join()
        if t_w is not None and t_b is not None:
            grad_done(ctx.srcs[2])
            grad_done(ctx.srcs[3])
        da_rows, dh, dc_rows = K.concat3_bwd(dfeat, d, parts, drop_p, seed)
        d_a, d_c = _scatter_head_rows(da_rows, dc_rows, plan_a, plan_c, t_a, t_c, a_shape, c_shape)
        # (the per-row d_a is not scaled in place like the big buffer: nothing of it is consumed)
        d_gate = ctx.d_gate * g if ctx.d_gate is not None and ctx.needs_input_grad[13] else None
        d_q = ctx.d_q * g if ctx.d_q is not None else None
        return d_a, None, dh, d_c, None, d_w, d_b, None, None, None, None, None, None, d_gate, d_q


def copy_q_grad(a, row_loss, grad_scale):
    """grad_scale * d row_loss / d q of the loss through the copy mix, per row: with m = (1 - a) p_g + a q and row_loss =
    -log m, dL/dq = -a / m = -a exp(row_loss) -- from the row losses the CE writers already return, on [B] tensors.  A row
    whose gate is 0 (the prior abstains) gets exactly 0, whatever its loss, and so does a row whose m is below fp32's range
    (1 / m = exp(row_loss) overflows: p_g = 0 in fp32 and q = 0) -- it is not divided by, as d_a is not."""
    inv_m = torch.exp(row_loss)
    return torch.where((a > 0) & torch.isfinite(inv_m), a * inv_m, torch.zeros_like(a)) * (-float(grad_scale))


def _copy_pair(copy_a, copy_q, b):
    if copy_a is None and copy_q is None:
        return None
    if copy_a is None or copy_q is None:
        raise ValueError('the copy mix takes both a_row and q_row')
    pair = tuple(t.detach().contiguous() for t in (copy_a, copy_q))
    if any(t.dtype != torch.float32 or t.numel() != b for t in pair):
        raise ValueError('a_row and q_row must be float32 with one entry per row of the head')
    return pair


_loss_weights = {}


def _loss_weight_vector(b, w1, w2, device):
    key = (b, float(w1), float(w2), str(device))
    v = _loss_weights.get(key)
    if v is None:
        if len(_loss_weights) > 16:
            _loss_weights.clear()
        v = torch.cat((torch.full((b,), float(w1)), torch.full((b,), float(w2)))).to(device)
        _loss_weights[key] = v
    return v


class DualHeadCEFn(Function):
    """Both score heads of one pass and their weighted sum (model.py:89-103) as ONE Function:
        loss_scale * ( mean CE(Linear([ent[s] | s_h | rel[r]]), o)  +  rel_weight * mean CE(Linear_r([ent[s] | s_q]), r) )
    The relation head (C = 2R classes: three GEMMs of 16-32 workgroups and a handful of few-microsecond kernels per
    direction of the pass) runs on the side stream next to the entity head's chip-filling GEMMs, in forward and in
    backward; so does the entity head's bias column sum.  The two heads gather the SAME rows ent[s]: their row
    gradients are added before ONE segmented scatter-add.  Values: those of the two HeadCEFn calls it replaces (the
    weight rel_weight is folded into the relation head's CE gradient instead of being applied by autograd)."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, a, ia, h1, c, ic, w1, b1, target1, h2, w2, b2, target2, plan_a, plan_c, drop_p, seed1, seed2,
                loss_scale=1.0, rel_weight=0.1, row_tap=None, copy_a=None, copy_q=None, event_a=None, event_q=None):
        """row_tap: a list that receives (row losses [2b]: entity head rows then relation head rows, s1, s2) -- the weights
        with which the returned scalar sums them (RENet.forward's fused directions split the merged loss by direction).
        copy_a / copy_q: as for HeadCEFn (d_a and d_q included), for the ENTITY head only; the relation head is the plain
        CE.
        event_a / event_q (both or neither; never with copy_a / copy_q): the EVENT loss through the joint mix, per row
            L = -log((1 - a) p_gold pr_gold + a q),   returned: loss_scale / b * sum(L)
        with q the prior's mass on the gold (relation, partner) pair (K.joint_gold_rows).  Both terms of the joint have weight
        1: rel_weight is NOT applied.  The relation head runs first, on the side stream, with the ENTITY head's grad_scale;
        its row losses give lp = -row_loss; the side stream is joined before the entity head's CE writer (the joint entry),
        which returns s per row; the relation head's gradient rows are multiplied by it (a dense [B, R] matrix: a relation
        head wide enough for the planes path, renet_hip.PLANES_MIN_CLASSES classes, is refused before any launch).
        event_a / event_q receive g * d_a
        and g * d_q as copy_a / copy_q do.  row_tap receives L in the entity rows and zeros, with weight 0, in the relation
        rows."""
        ctx.srcs = (a, c, w1, b1, w2, b2)
        copy = _copy_pair(copy_a, copy_q, h1.shape[0])
        event = _copy_pair(event_a, event_q, h1.shape[0])
        if event is not None:
            if copy is not None:
                raise ValueError('copy_a / copy_q and event_a / event_q are two different losses: give one pair')
            if K.current_mode() == 'bf16s':
                raise ValueError('the loss through the joint mix has no bf16-storage writer: use another GEMM mode')
            return DualHeadCEFn._forward_event(ctx, a, ia, h1, c, ic, w1, b1, target1, h2, w2, b2, target2, plan_a, plan_c,
                                               drop_p, seed1, seed2, loss_scale, row_tap, event)
        a, h1, h2, c, w1, b1, w2, b2 = (_c(t) for t in (a, h1, h2, c, w1, b1, w2, b2))
        b, d = h1.shape
        need_grad = any(ctx.needs_input_grad)
        s1, s2 = float(loss_scale) / b, float(loss_scale) * float(rel_weight) / b
        rl = torch.empty(2 * b, device=h1.device, dtype=torch.float32)
        def head2():
            return _head_forward(a, ia, h2, None, None, w2, b2, target2, drop_p, seed2, s2, need_grad, row_loss=rl[b:])
        sd = _Side(h1.device)
        if debug_tap is None:
            with sd():
                _, feat2, lg2, dl2, fop2, _ = head2()
        _, feat1, lg1, dl1, fop1, ctx.d_gate = _head_forward(a, ia, h1, c, ic, w1, b1, target1, drop_p, seed1, s1, need_grad,
                                                             row_loss=rl[:b], copy=copy)
        ctx.d_q = copy_q_grad(copy[0], rl[:b], s1) if copy is not None and ctx.needs_input_grad[21] else None
        if debug_tap is not None:                            # test hook: the entity head reports first
            _, feat2, lg2, dl2, fop2, _ = head2()
        sd.join()
        ctx.meta = (d, drop_p, seed1, seed2, plan_a, plan_c, a.shape, c.shape)
        ctx.grad_scales = (s1, s2)
        if need_grad:
            ctx.save_for_backward(feat1, lg1, w1, feat2, lg2, w2)
            ctx.consumed = False
            ctx.bf16 = (dl1, fop1, dl2, fop2)
        if row_tap is not None:
            row_tap.append((rl.detach(), s1, s2))
        return torch.dot(rl, _loss_weight_vector(b, s1, s2, h1.device))

    @staticmethod
    def _forward_event(ctx, a, ia, h1, c, ic, w1, b1, target1, h2, w2, b2, target2, plan_a, plan_c, drop_p, seed1, seed2,
                       loss_scale, row_tap, event):
        a, h1, h2, c, w1, b1, w2, b2 = (_c(t) for t in (a, h1, h2, c, w1, b1, w2, b2))
        b, d = h1.shape
        need_grad = any(ctx.needs_input_grad)
        s1 = float(loss_scale) / b
        if need_grad and debug_tap is None and K.use_planes(w2, w2.shape[0]):
            # (before any launch.  The relation head's gradient rows are scaled by s as a dense [B, R] matrix; a relation head
            # wide enough for the planes GEMMs -- renet_hip.PLANES_MIN_CLASSES classes -- keeps no dense gradient)
            raise ValueError('the loss through the joint mix scales the relation head\'s dense gradient rows: a relation head '
                             'with %d or more classes (the planes path) is not supported' % K.PLANES_MIN_CLASSES)
        rl = torch.empty(2 * b, device=h1.device, dtype=torch.float32)
        sd = _Side(h1.device)
        # (the relation head FIRST, also under debug_tap, where the ordinary path lets the entity head report first: the entity
        # head's writer needs the relation head's row losses)
        with sd():
            _, feat2, lg2, dl2, fop2, _ = _head_forward(a, ia, h2, None, None, w2, b2, target2, drop_p, seed2, s1, need_grad,
                                                        row_loss=rl[b:])

        def lp():
            sd.join()                                        # an event wait: the relation head ended long before
            return torch.neg(rl[b:])
        _, feat1, lg1, dl1, fop1, ctx.d_gate, s_row = _head_forward(a, ia, h1, c, ic, w1, b1, target1, drop_p, seed1, s1,
                                                                    need_grad, row_loss=rl[:b], event=event + (lp,))
        if need_grad:
            lg2.mul_(s_row.unsqueeze(1))                     # the relation head's CE gradient times the row's s
        ctx.d_q = copy_q_grad(event[0], rl[:b], s1) if ctx.needs_input_grad[23] else None
        ctx.event = True
        ctx.meta = (d, drop_p, seed1, seed2, plan_a, plan_c, a.shape, c.shape)
        ctx.grad_scales = (s1, s1)                           # (s <= 1: the f16x3 bound of the relation head stays valid)
        if need_grad:
            ctx.save_for_backward(feat1, lg1, w1, feat2, lg2, w2)
            ctx.consumed = False
            ctx.bf16 = (dl1, fop1, dl2, fop2)
        if row_tap is not None:
            row_tap.append((torch.cat((rl[:b].detach(), torch.zeros_like(rl[b:]))), s1, 0.0))
        return rl[:b].sum() * s1

    @staticmethod
    @_bwd_mode
    def backward(ctx, g):
        feat1, dl1, w1, feat2, dl2, w2 = ctx.saved_tensors
        d, drop_p, seed1, seed2, plan_a, plan_c, a_shape, c_shape = ctx.meta
        t_a, t_c, t_w1, t_b1, t_w2, t_b2 = [grad_target(t) for t in ctx.srcs]
        _consume_ce_gradient(ctx)
        b1_, fop1, b2_, fop2 = ctx.bf16
        dl1 = b1_ if b1_ is not None else dl1
        dl2 = b2_ if b2_ is not None else dl2
        bound1 = _scale_ce_gradient(dl1, g, ctx.grad_scales[0])      # upstream scalar (1 in RE-Net's training step)
        sd = _Side(feat1.device)
        # (deferring the entity head's dW / db to the side stream until opt.step(), like the GRU parameter gradients, was
        # measured: no gain -- 2.975 vs 2.987 ms per step, tools/sessions/r04_s18.sh: a chip-filling GEMM only competes
        # with the GRU / RGCN backward kernels it would run beside)
        with sd():
            bound2 = _scale_ce_gradient(dl2, g, ctx.grad_scales[1])
            dfeat2, d_w2, d_b2 = _head_backward(dl2, feat2, fop2, w2, t_w2, t_b2, bound=bound2, g=g)
            da2, dh2, _ = K.concat3_bwd(dfeat2, d, 2, drop_p, seed2)
        dfeat1, d_w1, d_b1 = _head_backward(dl1, feat1, fop1, w1, t_w1, t_b1, bias_side=sd, bound=bound1, g=g)
        da1, dh1, dc1 = K.concat3_bwd(dfeat1, d, 3, drop_p, seed1)
        sd.join()
        if t_w1 is not None and t_b1 is not None:
            grad_done(ctx.srcs[2])
            grad_done(ctx.srcs[3])
        if t_w2 is not None and t_b2 is not None:
            grad_done(ctx.srcs[4])
            grad_done(ctx.srcs[5])
        da1.add_(da2)                                        # same rows ent[s] in both heads: one scatter-add
        d_a, d_c = _scatter_head_rows(da1, dc1, plan_a, plan_c, t_a, t_c, a_shape, c_shape)
        gate_slot = 22 if getattr(ctx, 'event', False) else 20
        d_gate = ctx.d_gate * g if ctx.d_gate is not None and ctx.needs_input_grad[gate_slot] else None
        d_q = ctx.d_q * g if ctx.d_q is not None else None
        if gate_slot == 22:
            return (d_a, None, dh1, d_c, None, d_w1, d_b1, None, dh2, d_w2, d_b2, None) + (None,) * 10 + (d_gate, d_q)
        return (d_a, None, dh1, d_c, None, d_w1, d_b1, None, dh2, d_w2, d_b2, None) + (None,) * 8 + (d_gate, d_q, None, None)


class SegmentPoolFn(Function):
    """dgl.max_nodes / mean_nodes over the member graphs (Aggregator.py:58-61)."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, h, seg_ptr, num_graphs, is_max):
        h = _c(h)
        out, arg = K.segment_pool_fwd(h, seg_ptr, num_graphs, is_max)
        ctx.meta = (seg_ptr, arg, num_graphs, is_max, h.shape[0])
        return out

    @staticmethod
    @_bwd_mode
    def backward(ctx, dout):
        seg_ptr, arg, num_graphs, is_max, n = ctx.meta
        return K.segment_pool_bwd(_c(dout), seg_ptr, arg, num_graphs, is_max, n), None, None, None


class NbrAttnProjFn(Function):
    """The two projections of the attentive encoder's score (Aggregator.py:333-334) with attn_s.weight = [W_o | W_s | W_r]:
        P = E W_o^T  [N_ent, D]   (one row per ENTITY instead of one per neighbour occurrence)
        q = E[s] W_s^T + R[r] W_r^T + b  [nseq, D]   (one row per kept sequence of the batch)
    so that the score of neighbour j is v . tanh(P[nbr_j] + q).  All products on the GEMM front (the process GEMM mode)."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, ent, rel, weight, bias, nb):
        ctx.srcs = (ent, rel, weight, bias)
        ent, rel, weight, bias = _c(ent), _c(rel), _c(weight), _c(bias)
        d = ent.shape[1]
        w_o, w_s, w_r = (_c(weight[:, k * d:(k + 1) * d]) for k in range(3))
        p = K.gemm(ent, w_o, tb=True)
        es, rr = K.gather_rows(ent, nb.s_sorted), K.gather_rows(rel, nb.r_sorted)
        q = K.gemm(es, w_s, tb=True, bias=bias)
        K.gemm(rr, w_r, tb=True, out=q, beta=1.0)
        ctx.nb = nb
        ctx.save_for_backward(ent, rel, w_o, w_s, w_r, es, rr)
        return p, q

    @staticmethod
    @_bwd_mode
    def backward(ctx, dp, dq):
        ent, rel, w_o, w_s, w_r, es, rr = ctx.saved_tensors
        nb, d = ctx.nb, ent.shape[1]
        t_ent, t_rel, t_w, t_b = [grad_target(t) for t in ctx.srcs]
        dp, dq = _c(dp), _c(dq)
        d_ent = t_ent if t_ent is not None else torch.zeros_like(ent)
        K.gemm(dp, w_o, out=d_ent, beta=1.0)                             # += dP W_o
        K.segment_add(K.gemm(dq, w_s), nb.plan_s, d_ent)                 # per-sequence rows -> their subject entity
        d_rel = _segment_grad(K.gemm(dq, w_r), nb.plan_r, t_rel, rel.shape)
        acc = t_w is not None
        d_w = t_w if acc else torch.empty(d, 3 * d, device=ent.device, dtype=torch.float32)
        beta = 1.0 if acc else 0.0
        K.gemm(dp, ent, ta=True, out=d_w[:, :d], beta=beta)
        K.gemm(dq, es, ta=True, out=d_w[:, d:2 * d], beta=beta)
        K.gemm(dq, rr, ta=True, out=d_w[:, 2 * d:], beta=beta)
        return (None if t_ent is not None else d_ent), d_rel, (None if acc else d_w), _colsum_grad(dq, t_b), None


class NbrPoolFn(Function):
    """Aggregator.py:249-285 (mean) / 316-346 (attention) up to the dropout: the packed GRU input of a
    graph.DeviceNeighbourBatch.  p / q / v None: mean mode, out [S, 2D] = [mean_j E[nbr_j] | E[s]]; else attention,
    out [S, 3D] = [sum_j softmax_j(v . tanh(P[nbr_j] + q)) E[nbr_j] | E[s] | R[r]] (p, q from NbrAttnProjFn).
    Backward: renet_nbr_pool_bwd's contribution rows, summed per entity / sequence by the deterministic segmented adds."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, ent, rel, p, q, v, nb):
        attn = p is not None
        if nb.max_ent >= ent.shape[0] or (attn and nb.max_rel >= rel.shape[0]):
            raise ValueError('batch entity / relation id beyond the embedding table')
        if attn and (p.shape != ent.shape or tuple(q.shape) != (nb.nseq, ent.shape[1]) or v.numel() != ent.shape[1]
                     or rel.shape[1] != ent.shape[1]):
            raise ValueError('NbrPoolFn: P must be [N_ent, D], q [sequences, D], v [D, 1], R [., D]')
        ctx.srcs = (ent, rel)
        ent = _c(ent)
        if attn:
            rel, p, q, v = _c(rel), _c(p), _c(q), _c(v)
        out, stats, w = K.nbr_pool_fwd(ent, rel if attn else None, p, q, v if attn else None, nb)
        ctx.nb, ctx.attn, ctx.stats = nb, attn, stats
        ctx.rel_shape = rel.shape if attn else None
        ctx.v_shape = v.shape if attn else None
        if attn:
            ctx.save_for_backward(ent, p, q, v, w, out)
        else:
            ctx.save_for_backward(ent)
        return out

    @staticmethod
    @_bwd_mode
    def backward(ctx, dout):
        nb, attn = ctx.nb, ctx.attn
        ent = ctx.saved_tensors[0]
        p, q, v, w, out = ctx.saved_tensors[1:] if attn else (None,) * 5
        dev, d = ent.device, ent.shape[1]
        t_ent, t_rel = grad_target(ctx.srcs[0]), (grad_target(ctx.srcs[1]) if attn else None)
        ce, cp, dq_rows, dv_rows, ds_rows, dr_rows = K.nbr_pool_bwd(_c(dout), out, ent, p, q, v, w, nb)
        d_ent = t_ent if t_ent is not None else torch.zeros(ent.shape, device=dev, dtype=torch.float32)
        ds_seq = torch.zeros(nb.nseq, d, device=dev, dtype=torch.float32)
        if not attn:
            K.segment_add(ce, nb.plan_nbr, d_ent)
            K.segment_add(ds_rows, nb.plan_seq, ds_seq)
            K.segment_add(ds_seq, nb.plan_s, d_ent)
            return (None if t_ent is not None else d_ent), None, None, None, None, None
        d_p = torch.zeros(ent.shape, device=dev, dtype=torch.float32)
        K.segment_add2(ce, cp, nb.plan_nbr, d_ent, d_p)
        dr_seq = torch.zeros(nb.nseq, d, device=dev, dtype=torch.float32)
        K.segment_add2(ds_rows, dr_rows, nb.plan_seq, ds_seq, dr_seq)
        K.segment_add(ds_seq, nb.plan_s, d_ent)
        d_rel = _segment_grad(dr_seq, nb.plan_r, t_rel, ctx.rel_shape)
        d_q = torch.zeros(nb.nseq, d, device=dev, dtype=torch.float32)
        K.segment_add(dq_rows, nb.plan_seq, d_q)
        d_v = K.colsum(dv_rows).reshape(ctx.v_shape)
        return (None if t_ent is not None else d_ent), d_rel, d_p, d_q, d_v, None


class DropoutFn(Function):
    """Counter-based inverted dropout (Aggregator.py:69); the mask is regenerated in backward."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, x, drop_p, seed):
        ctx.meta = (drop_p, seed)
        return K.dropout(_c(x), drop_p, seed)

    @staticmethod
    @_bwd_mode
    def backward(ctx, g):
        return K.dropout(_c(g), *ctx.meta), None, None


class LinearFn(Function):
    """y = x @ W^T + b on the MFMA GEMM (nn.Linear forward/backward; global_model.py:52)."""

    @staticmethod
    @_fwd_mode
    def forward(ctx, x, weight, bias):
        x, weight = _c(x), _c(weight)
        ctx.save_for_backward(x, weight)
        return K.gemm(x, weight, tb=True, bias=_c(bias))

    @staticmethod
    @_bwd_mode
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = _c(g)
        return (K.gemm(g, weight), K.gemm(g, x, ta=True), K.colsum(g))


class SparseTargets(object):
    """Soft target distributions of B rows in CSR form on the device (renet_soft_ce_sparse): `ptr` [B + 1] and `col` [nnz]
    (int32; per row distinct and ascending, in [0, num_cols)), `w` [nnz] (fp32, >= 0; a row need not sum to 1).  Built from
    host arrays, validated there, and uploaded in ONE copy."""

    def __init__(self, ptr, col, w, num_cols, device):
        ptr = np.ascontiguousarray(ptr, dtype=np.int64).reshape(-1)
        col = np.ascontiguousarray(col, dtype=np.int64).reshape(-1)
        w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
        if len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != len(col) or len(w) != len(col) or np.any(np.diff(ptr) < 0) or \
                len(col) >= 2 ** 31:
            raise ValueError('sparse targets: ptr / col / w do not describe a CSR matrix')
        if len(col):
            inner = np.ones(len(col), dtype=bool)
            inner[ptr[:-1][np.diff(ptr) > 0]] = False                  # (the first entry of every non-empty row)
            if col.min() < 0 or col.max() >= int(num_cols) or np.any(np.diff(col)[inner[1:]] <= 0):
                raise ValueError('sparse targets: the columns of a row must be distinct, ascending and inside the row')
            if not (w >= 0).all():
                raise ValueError('sparse targets: weights must be >= 0')
        self.rows, self.num_cols, self.nnz = len(ptr) - 1, int(num_cols), len(col)
        flat = np.concatenate((ptr.astype(np.int32), col.astype(np.int32), w.view(np.int32)))
        up = torch.from_numpy(flat).to(device, non_blocking=True)
        self.ptr, self.col = up[:len(ptr)], up[len(ptr):len(ptr) + len(col)]
        self.w = up[len(ptr) + len(col):].view(torch.float32)

    def rows_slice(self, a, b):
        """The targets of rows [a, b) as a VIEW of the same device arrays (ptr keeps its offsets into col / w)."""
        t = SparseTargets.__new__(SparseTargets)
        t.rows, t.num_cols, t.nnz = int(b) - int(a), self.num_cols, self.nnz
        t.ptr, t.col, t.w = self.ptr[a:b + 1], self.col, self.w
        return t


class SoftCESparseFn(Function):
    """scale * sum_b ( W_b logsumexp(logits[b]) - sum_k w_k logits[b, col_k] ): utils.soft_cross_entropy (global_model.py:53)
    for sparse soft targets with scale = 1 / B, on the fused kernel (csrc/soft_ce.hip).  The logits are OVERWRITTEN with their
    gradient scale * (W softmax - w) when one is needed -- hand in the result of LinearFn, whose backward takes it from there
    (it keeps no copy of its output) -- unless inplace=False, which works on a copy."""

    @staticmethod
    def forward(ctx, logits, targets, scale, inplace=True):
        if logits.dim() != 2 or logits.shape[0] != targets.rows or logits.shape[1] != targets.num_cols:
            raise ValueError('SoftCESparseFn: logits %s against targets [%d, %d]' % (tuple(logits.shape), targets.rows,
                                                                                   targets.num_cols))
        need_grad = ctx.needs_input_grad[0]
        buf = logits.detach()
        if not buf.is_contiguous():
            buf = buf.contiguous()                                     # (a copy of its own already)
        elif need_grad and not inplace:
            buf = buf.clone()
        row_loss = K.soft_ce_sparse(buf, targets.ptr, targets.col, targets.w, float(scale), need_grad)
        if need_grad:
            ctx.dlogits, ctx.consumed = buf, False
        return row_loss.sum() * float(scale)

    @staticmethod
    def backward(ctx, g):
        _consume_ce_gradient(ctx)
        dl, ctx.dlogits = ctx.dlogits, None
        K.scale_by_device_scalar(dl, _c(g.reshape(1)))                 # (the upstream scalar, from device memory: no sync)
        return dl, None, None, None


def host_offsets(step_off):
    """int array -> ctypes int32 array kept alive by the caller (the GRU entry points read it on the host)."""
    arr = np.ascontiguousarray(step_off, dtype=np.int32)
    return (ctypes.c_int32 * len(arr))(*arr.tolist())


class EventSelection(object):
    """The running global choice of one direction's generated events (K.select_events folded over the sub-blocks of a
    timestamp): owns the carry -- the winners so far, device tensors that nothing reads back until result() -- and the
    kernel's workspace, which every add() reuses (calls are ordered on one stream)."""

    def __init__(self, num_k, device):
        self.num_k, self.device = int(num_k), device
        if not 1 <= self.num_k <= K.SELECT_EVENTS_MAX:
            raise ValueError('num_k must lie in [1, %d] (renet_select_events)' % K.SELECT_EVENTS_MAX)
        self.carry = None
        self.workspace = torch.empty(max(K.lib().renet_select_events_workspace(1, 1, 1, self.num_k) // 8, 1), device=device,
                                     dtype=torch.int64)

    def add(self, ent, val, off, g_ent, g_lprior, g_mult):
        """One sub-block: topk_rows' (idx, val) [G * R, k], joint_row_offsets' off [G * R], and per group the entity, its
        log prior and its multiplicity."""
        self.carry = K.select_events(ent, val, off, g_ent, g_lprior, g_mult, self.num_k, self.carry, self.workspace)

    def _rows(self):
        c = self.carry                                   # [6, num_k] int32: the fp32 values as their bit patterns
        return torch.stack((c[0], c[1], c[2], c[3].view(torch.int32), c[4], c[5].expand(self.num_k)))

    @staticmethod
    def results(selections):
        """Per selection (given, rel, other, val, mult) as host arrays cut to the winners; ONE device-to-host copy for all
        of them (a selection nothing was added to gives empty arrays)."""
        live = [s for s in selections if s.carry is not None]
        back = iter(torch.cat([s._rows() for s in live]).cpu().numpy().reshape(len(live), 6, -1)) if live else iter(())
        out = []
        for s in selections:
            if s.carry is None:
                out.append(tuple(np.zeros(0, dtype=t) for t in (np.int32, np.int32, np.int32, np.float32, np.int32)))
                continue
            a = next(back)
            n = int(a[5, 0])
            out.append((a[0, :n], a[1, :n], a[2, :n], a[3, :n].copy().view(np.float32), a[4, :n]))
        return out
