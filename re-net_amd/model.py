"""RENet with the reference's constructor, attributes, parameter names and method signatures
(reference model.py:10-446), so that train.py / test.py drive it unchanged -- computing on the HIP
kernels of librenet_hip.so instead of DGL + cuDNN/cuBLAS.

state_dict keys (checkpoint compatible): rel_embeds, ent_embeds,
encoder.{weight,bias}_{ih,hh}_l0, encoder_r.*, aggregator.rgcn{1,2}.{weight,loop_weight},
linear.{weight,bias}, linear_r.{weight,bias}.
"""
import math
import os
from collections import defaultdict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import PackedSequence

import filter_index as FI
import graph as G
import ops
import renet_hip as K
from Aggregator import RGCNAggregator
from utils import *        # noqa: F401,F403  (the reference's model.py re-exports utils the same way)


def _moded(fn):
    """Runs a model method inside the model's own GEMM-mode scope (`self.gemm_mode`: None = the process default,
    'bf16x6' / 'f16x3' = this model's choice; renet_hip.gemm_mode).  Nested calls re-enter the same scope."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        with K.gemm_mode(getattr(self, 'gemm_mode', None)):
            return fn(self, *a, **k)
    return wrapped


class GRU(nn.Module):
    """Drop-in for nn.GRU(input_size, hidden_size, batch_first=True), one layer, h0 = 0, on the HIP
    recurrence.  Same parameter names/shapes/init as torch (weight_ih_l0 [3H,I], weight_hh_l0 [3H,H],
    bias_ih_l0, bias_hh_l0; U(-1/sqrt(H), 1/sqrt(H))).  Returns (None, h_n[1,B,H]): the reference only
    ever uses h_n (model.py:86-87,94-95)."""

    def __init__(self, input_size, hidden_size, batch_first=True):
        super().__init__()
        self.input_size, self.hidden_size, self.batch_first = input_size, hidden_size, batch_first
        k = 1.0 / math.sqrt(hidden_size)
        self.weight_ih_l0 = nn.Parameter(torch.empty(3 * hidden_size, input_size).uniform_(-k, k))
        self.weight_hh_l0 = nn.Parameter(torch.empty(3 * hidden_size, hidden_size).uniform_(-k, k))
        self.bias_ih_l0 = nn.Parameter(torch.empty(3 * hidden_size).uniform_(-k, k))
        self.bias_hh_l0 = nn.Parameter(torch.empty(3 * hidden_size).uniform_(-k, k))

    def forward(self, inp, total_rows=None):
        if isinstance(inp, PackedSequence):
            data, bs = inp.data, inp.batch_sizes.numpy()
        else:                                   # [B, L, I] dense, every sequence full length
            b, l, _ = inp.shape
            data = inp.transpose(0, 1).reshape(b * l, -1)
            bs = np.full(l, b, dtype=np.int64)
        off = ops.host_offsets(np.concatenate(([0], np.cumsum(bs))))
        nrows = int(bs[0]) if len(bs) else 0
        h = ops.GRUFn.apply(data, self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0,
                            off, max(total_rows or 0, nrows))
        return None, h


class RENet(nn.Module):
    def __init__(self, in_dim, h_dim, num_rels, dropout=0, model=0, seq_len=10, num_k=10):
        super().__init__()
        self.in_dim = in_dim
        self.h_dim = h_dim
        self.num_rels = num_rels
        self.model = model
        self.seq_len = seq_len
        self.num_k = num_k
        gain = nn.init.calculate_gain('relu')
        self.rel_embeds = nn.Parameter(torch.empty(2 * num_rels, h_dim))
        nn.init.xavier_uniform_(self.rel_embeds, gain=gain)
        self.ent_embeds = nn.Parameter(torch.empty(in_dim, h_dim))
        nn.init.xavier_uniform_(self.ent_embeds, gain=gain)

        self.drop_p = float(dropout or 0.0)
        self.dropout = nn.Dropout(dropout)
        self.encoder = GRU(4 * h_dim, h_dim, batch_first=True)
        self.encoder_r = GRU(3 * h_dim, h_dim, batch_first=True)
        self.aggregator = RGCNAggregator(h_dim, dropout, in_dim, num_rels, 100, model, seq_len)
        self.linear = nn.Linear(3 * h_dim, in_dim)
        self.linear_r = nn.Linear(2 * h_dim, num_rels)

        # inference-time state (saved/restored by train.py:189-195, test.py:70-81)
        self.global_emb = None
        self.s_hist_test = None
        self.o_hist_test = None
        self.s_hist_test_t = None
        self.o_hist_test_t = None
        self.s_his_cache = None
        self.o_his_cache = None
        self.s_his_cache_t = None
        self.o_his_cache_t = None
        self.graph_dict = None
        self.data = None
        self.latest_time = 0
        self._reset_candidates()
        self.criterion = nn.CrossEntropyLoss()
        # Reference quirk switch.  model.py:229-297 re-uses the names `s` / `o` as loop variables inside predict(),
        # so the FIRST quadruple evaluated at every new timestamp is scored (and its loss computed) for the entity
        # of the LAST candidate returned by the unsorted top-k over the sampled subjects (objects) instead of for
        # its own subject / object; evaluate_filter then ranks the quadruple's true entities in those scores.
        # False (default): score the quadruple's own entities.  True: reproduce the reference bit for bit in
        # behaviour (which entity shadows depends on the device's unsorted top-k order; `shadow_pick(side, cands)`
        # may override the choice -- the golden test drives it with the entities the reference run recorded).
        # fp32-class GEMM mode of THIS model: None = the process default (RENET_GEMM), or 'bf16x6' / 'f16x3'
        self.gemm_mode = None
        self.reference_shadowing = False
        # inference advance: one history per sampled entity, relation segment of the GRU input broadcast (see
        # _joint_topk_many); False builds the R-fold batches of rounds 1-3 (A/B runs, tests)
        self.broadcast_relations = os.environ.get('RENET_ADVANCE_BROADCAST', '1') != '0'
        # inference advance: score the (entity, relation) rows in blocks of descending upper bound p_r * prob and stop at the
        # first row that cannot reach the top num_k any more (_winners_pruned: exact, same winners).  Default since round 5
        # (0.179 -> 0.059 s per advance on a trained ICEWS18-shaped model at num_k 1000, identical predicted facts:
        # profiles/r05_a_advance_pruned.txt); RENET_ADVANCE_PRUNE=0 restores the exhaustive scoring (A/B runs, tests).
        self.prune_relations = os.environ.get('RENET_ADVANCE_PRUNE', '1') == '1'
        # forward(): run the two calls of train.py:136-137 as ONE merged pass (_forward_fused; opt-in, see its contract)
        self.fuse_directions = os.environ.get('RENET_FUSE_DIRECTIONS', '0') == '1'
        self._fused_pending = None
        # ... and build that merged batch with the DEVICE builder (_prepare_both_lists_device; RENET_DEVICE_BUILDER_LISTS=0:
        # the host builder)
        self.device_builder_lists = os.environ.get('RENET_DEVICE_BUILDER_LISTS', '1') != '0'
        # evaluate_filter(): answer the per-quadruple calls of test.py / train.py's validation from ONE batched evaluation
        # per timestamp (_lookahead_filter; opt-in, see its docstring)
        self.lookahead_eval = os.environ.get('RENET_LOOKAHEAD_EVAL', '0') == '1'
        self._la = self._la_at = None
        # evaluate_filter_batch(): ranks and loss from the resident filter index + one rank kernel per direction
        # (_device_ranks; opt-in: RENET_DEVICE_RANK=1; tools/run_reference_driver.py turns it on) instead of a host sort of
        # all_triplets per call and torch passes over the score matrix
        self.device_rank = os.environ.get('RENET_DEVICE_RANK', '0') == '1'
        self._filter_index = None
        self.last_prune = None
        self.shadow_pick = None
        self._shadow = {}

    def train(self, mode=True):
        """nn.Module.train / eval; also drops a half-finished fused step (a subject=True call whose subject=False
        partner never came -- an exception, an early exit -- must not leave its loss, histories and batch alive, nor make
        the next training step raise)."""
        self._fused_pending = None
        return super().train(mode)

    def _reset_candidates(self):
        self.preds_list_s = defaultdict(lambda: torch.zeros(self.num_k))
        self.preds_ind_s = defaultdict(lambda: torch.zeros(self.num_k))
        self.preds_list_o = defaultdict(lambda: torch.zeros(self.num_k))
        self.preds_ind_o = defaultdict(lambda: torch.zeros(self.num_k))

    # ------------------------------------------------------------------------------------------
    def _direction(self, triplets, subject):
        """model.py:65-78: pick (s, r, o), the rel_embeds half and the edge-type view."""
        if subject:
            return triplets[:, 0], triplets[:, 1], triplets[:, 2], self.rel_embeds[:self.num_rels], False
        return triplets[:, 2], triplets[:, 1], triplets[:, 0], self.rel_embeds[self.num_rels:], True

    def host_batch(self, triplets, hist, graph_dict, subject=True):
        """Pure host work of one direction of a step (no device access: safe in a worker process of
        pipeline.BatchPrefetcher): returns a picklable dict with the packed batch graph (or None when every
        history is empty) and the small label arrays."""
        trip = triplets.detach().cpu().numpy() if isinstance(triplets, torch.Tensor) else np.asarray(triplets)
        s, r, o, _, _ = self._direction(trip, subject)
        agg = self.aggregator
        fh = hist if isinstance(hist, G.FlatHistory) else G.FlatHistory.from_lists(hist[0], hist[1])
        out = {'subject': bool(subject), 'b': len(s), 's': s.astype(np.int32), 'r': r.astype(np.int32), 'pb': None}
        if fh.seq_ptr[-1] == 0:
            out['o'] = o.astype(np.int32)
            return out
        table = agg.glob_table.get_host(self.global_emb)
        hb = G.build_batch(G.store_for(graph_dict), self.in_dim, self.num_rels, s, r, fh, sort=True,
                           glob_index=table.index)
        if hb.L > self.seq_len:
            raise ValueError('history longer than seq_len (%d > %d)' % (hb.L, self.seq_len))
        out['pb'] = G.PackedBatch(hb)
        out['o'] = o[hb.perm].astype(np.int32)
        return out

    def prepare_from_host(self, hbatch):
        """Device half of prepare(): one upload of the packed batch + the label vector."""
        if hbatch.get('both'):
            return self.prepare_both_from_host(hbatch)
        dev = self.ent_embeds.device
        prep = PreparedBatch()
        prep.subject, prep.b = hbatch['subject'], hbatch['b']
        if hbatch['pb'] is None:    # every history empty: the reference crashes here; use h = 0
            prep.g = None
            prep.perm = np.arange(prep.b)
            prep.s_idx = torch.from_numpy(hbatch['s']).to(dev)
            prep.r_idx = torch.from_numpy(hbatch['r']).to(dev)
            prep.plan_s, prep.plan_r = _device_plan(hbatch['s'], dev), _device_plan(hbatch['r'], dev)
        else:
            g = G.DeviceGraph(hbatch['pb'], dev)
            g.glob = self.aggregator.glob_table.get(self.global_emb, self.h_dim, dev).mat
            prep.g, prep.perm = g, g.host.perm
            prep.s_idx, prep.r_idx, prep.plan_s, prep.plan_r = g.s_sorted, g.r_sorted, g.plan_s, g.plan_r
            prep.batch_sizes = torch.from_numpy(g.host.batch_sizes)
            prep.step_off = ops.host_offsets(g.host.step_off)
        prep.o_idx = torch.from_numpy(hbatch['o']).to(dev)
        return prep

    def host_batch_both(self, triplets, s_hist, o_hist, graph_dict, shard=None):
        """Host half of BOTH passes of a training step as one merged batch (graph.build_batch_both); None when
        either direction has no history at all (callers then fall back to the two separate passes)."""
        trip = triplets.detach().cpu().numpy() if isinstance(triplets, torch.Tensor) else np.asarray(triplets)
        fs = s_hist if isinstance(s_hist, G.FlatHistory) else G.FlatHistory.from_lists(s_hist[0], s_hist[1])
        fo = o_hist if isinstance(o_hist, G.FlatHistory) else G.FlatHistory.from_lists(o_hist[0], o_hist[1])
        if fs.seq_ptr[-1] == 0 or fo.seq_ptr[-1] == 0:
            return None
        table = self.aggregator.glob_table.get_host(self.global_emb)
        hb = G.build_batch_both(G.store_for(graph_dict), self.in_dim, self.num_rels, trip[:, 0], trip[:, 1],
                                trip[:, 2], fs, fo, glob_index=table.index)
        if hb.L > self.seq_len:
            raise ValueError('history longer than seq_len (%d > %d)' % (hb.L, self.seq_len))
        share = 1.0
        if shard is not None:            # (rank, world): this rank's sequences of the SAME batch (graph.shard_sequences)
            full = hb.B
            hb = G.shard_sequences(hb, int(shard[0]), int(shard[1]))
            share = hb.B / float(full)
        return {'both': True, 'b': hb.B, 'share': share, 'sharded': shard is not None, 'pb': G.PackedBatch(hb)}

    def prepare_both_from_host(self, hbatch):
        dev = self.ent_embeds.device
        prep = PreparedBatch()
        prep.subject, prep.b = None, hbatch['b']
        prep.share = hbatch.get('share', 1.0)
        prep.sharded = bool(hbatch.get('sharded', False))
        g = G.DeviceGraph(hbatch['pb'], dev)
        g.glob = self.aggregator.glob_table.get(self.global_emb, self.h_dim, dev).mat
        prep.g, prep.perm = g, g.host.perm
        prep.s_idx, prep.r_idx, prep.plan_s, prep.plan_r = g.s_sorted, g.r_sorted, g.plan_s, g.plan_r
        prep.o_idx, prep.r_label = g.ent_label, g.rel_label
        prep.batch_sizes = torch.from_numpy(g.host.batch_sizes)
        prep.step_off = ops.host_offsets(g.host.step_off)
        return prep

    def prepare_both_device(self, idx, dstore, stream=None):
        """prepare_both() with the batch graph built ON THE DEVICE from the quadruple indices `idx` of a resident dataset
        (gpu_builder.DeviceStore): enqueues the builder kernels (on `stream`, default the current one) and returns the
        pending gpu_builder.DeviceBatch at once; finish_prepare_device() turns it into a PreparedBatch."""
        import gpu_builder
        return gpu_builder.DeviceBatch(dstore, idx, self.seq_len, stream=stream)

    def finish_prepare_device(self, pending, glob=None):
        """Waits for the pending batch's counts (~256 bytes D2H).  Returns the PreparedBatch, or None if a capacity of the
        device builder was exceeded (the store's capacities have been raised: call prepare_both_device again).
        glob: the global-embedding matrix that belongs to the pending batch's store (rows in the order of its glob_times);
        None = the table of this model's own global_emb."""
        if not pending.finalize():
            return None
        g = pending
        if g.L > self.seq_len:
            raise ValueError('history longer than seq_len (%d > %d)' % (g.L, self.seq_len))
        dev = self.ent_embeds.device
        prep = PreparedBatch()
        prep.subject, prep.b, prep.share = None, g.B, 1.0
        g.glob = glob if glob is not None else self.aggregator.glob_table.get(self.global_emb, self.h_dim, dev).mat
        prep.g = g
        prep.perm = None                     # (g.host.perm fetches it on demand)
        prep.s_idx, prep.r_idx, prep.plan_s, prep.plan_r = g.s_sorted, g.r_sorted, g.plan_s, g.plan_r
        prep.o_idx, prep.r_label = g.ent_label, g.rel_label
        prep.batch_sizes = torch.from_numpy(g.host.batch_sizes)
        prep.step_off = ops.host_offsets(g.host.step_off)
        return prep

    def prepare_both(self, triplets, s_hist, o_hist, graph_dict, shard=None):
        """prepare() for the merged batch of both passes; None -> use prepare() twice.
        shard = (rank, world): keep this rank's share of the batch's sequences (exact data-parallel split: the
        ranks' losses and gradients SUM to those of the whole batch)."""
        hbatch = self.host_batch_both(triplets, s_hist, o_hist, graph_dict, shard=shard)
        return None if hbatch is None else self.prepare_both_from_host(hbatch)

    @_moded
    def loss_prepared_both(self, prep, row_tap=None, copy=None, event_copy=None):
        """loss_prepared(prep_s) + loss_prepared(prep_o) evaluated as ONE pass over the 2B sequences of the merged
        batch (extension of the reference API; train.py:136-138 adds the two losses of the same quadruples).  The
        aggregator, both encoders and both heads are shared between the directions (model.py:26-40), the directions
        differ only in which half of rel_embeds and which edge-type view they read (model.py:70-78) -- both baked
        into the merged batch's indices -- so every kernel simply sees twice the rows: half the launches, GEMMs
        with M (or K) doubled.  Each CE is a mean over its B rows: the sum of the two is 2 x the mean over 2B.
        copy: a recurrence.CopyRows of the batch, or its (a_row, q_row) in the batch's row order -- the ENTITY head's loss
        goes through the copy mix of the recurrence prior, -log((1 - a) softmax[gold] + a q) (ops._head_forward); a_row may
        require grad (a learned recurrence.CopyGate).  The relation head is unchanged.  Such a step is not in the C launch
        list: it runs the autograd path and pays its host enqueue.  None: today's path, launch for launch.
        event_copy: a recurrence.EventCopyRows of the batch, or its (a_row, q_row) -- the EVENT loss through the joint mix,
        -log((1 - a) softmax[gold] softmax_r[gold relation] + a q) per row with q the prior's mass on the gold (relation,
        partner) pair (ops.DualHeadCEFn, event_a / event_q): both heads train through it, the relation term has weight 1 (not
        0.1).  Never with copy=; refused for sharded batches and in bf16-storage mode as copy= is; not in the C launch list."""
        g = prep.g
        self.aggregator.last_batch = g
        copy_a = copy_q = event_a = event_q = None
        if event_copy is not None:
            if copy is not None:
                raise ValueError('loss_prepared_both: copy= and event_copy= are two different losses: give one of them')
            if getattr(prep, 'sharded', False):
                raise ValueError('loss_prepared_both: event_copy= with a sharded batch is not supported (the gate gradients of '
                                 'the ranks are not exchanged)')
            if K.current_mode() == 'bf16s':
                raise ValueError('loss_prepared_both: event_copy= has no bf16-storage writer: use another GEMM mode')
            event_a, event_q = event_copy.batch(prep)[:2] if hasattr(event_copy, 'batch') else event_copy
        if copy is not None:
            if getattr(prep, 'sharded', False):
                raise ValueError('loss_prepared_both: copy= with a sharded batch is not supported (the gate gradients of the '
                                 'ranks are not exchanged)')
            if K.current_mode() == 'bf16s':
                raise ValueError('loss_prepared_both: copy= has no bf16-storage writer: use another GEMM mode')
            copy_a, copy_q = copy.batch(prep)[:2] if hasattr(copy, 'batch') else copy
        # the same launch sequence issued from C (csrc/step.cpp): two C-ABI calls per step instead of ~55; bit-identical
        import step_plan
        if copy is None and event_copy is None and step_plan.eligible(self, prep):
            return step_plan.StepFn.apply(self, prep, row_tap, *step_plan.model_params(self))
        # a shard of a batch whose graph every rank replicates (prepare_both(shard=...)): rank-independent dropout
        # masks at the graph-side sites, so that the N-rank step equals the 1-rank step
        with ops.shared_graph_seeds(getattr(prep, 'sharded', False) or ops.SHARED_GRAPH_SEEDS):
            x, xr = self.aggregator.encode(g, self.ent_embeds, self.rel_embeds, reverse=False, _lazy_bf16=True)
        s_h, s_q = ops.dual_gru(x, xr, self.encoder, self.encoder_r, prep.step_off, prep.b)
        # [1, rows, H] -> [rows, H] as a VIEW: indexing with [0] would make autograd fill and copy a zeros tensor per
        # encoder in the backward pass (select_backward)
        s_h, s_q = s_h.view(s_h.shape[1:]), s_q.view(s_q.shape[1:])
        p = self.drop_p if self.training else 0.0
        # sum of two B-row means = 2 x the 2B-row mean; a rank holding a share of the batch's sequences (exact
        # data-parallel split) contributes share x that, so that the ranks' losses and gradients SUM to the batch's
        scale = 2.0 * getattr(prep, 'share', 1.0)
        seed1, seed2 = (ops.next_seed(), ops.next_seed()) if p > 0 else (0, 0)
        # both score heads as one autograd Function (ops.DualHeadCEFn: the relation head on a second stream)
        return ops.DualHeadCEFn.apply(self.ent_embeds, prep.s_idx, s_h, self.rel_embeds, prep.r_idx,
                                      self.linear.weight, self.linear.bias, prep.o_idx, s_q,
                                      self.linear_r.weight, self.linear_r.bias, prep.r_label, prep.plan_s,
                                      prep.plan_r, p, seed1, seed2, scale, 0.1, row_tap, copy_a, copy_q, event_a, event_q)

    def prepare(self, triplets, hist, graph_dict, subject=True):
        """Host + upload half of one direction of a training step: batch graph, packed layout and plans,
        uploaded once.  Everything `loss_prepared` needs is device-resident afterwards, so an input pipeline
        can run this ahead of the step (bench.py does; pipeline.BatchPrefetcher runs the host part in worker
        processes).  hist: (histories, timestamps) in the reference's nested-list layout, or a FlatHistory."""
        return self.prepare_from_host(self.host_batch(triplets, hist, graph_dict, subject))

    def _heads(self, prep, s_h, s_q):
        """model.py:89-103: both score heads + the weighted sum of their losses."""
        subject = prep.subject
        rel_embeds = self.rel_embeds[:self.num_rels] if subject else self.rel_embeds[self.num_rels:]
        p = self.drop_p if self.training else 0.0
        seed1, seed2 = (ops.next_seed(), ops.next_seed()) if p > 0 else (0, 0)
        return ops.DualHeadCEFn.apply(self.ent_embeds, prep.s_idx, s_h, rel_embeds, prep.r_idx,      # model.py:89-103
                                      self.linear.weight, self.linear.bias, prep.o_idx, s_q,
                                      self.linear_r.weight, self.linear_r.bias, prep.r_idx, prep.plan_s,
                                      prep.plan_r, p, seed1, seed2, 1.0, 0.1)

    def _encode(self, prep):
        rel_embeds = self.rel_embeds[:self.num_rels] if prep.subject else self.rel_embeds[self.num_rels:]
        self.aggregator.last_batch = prep.g
        return self.aggregator.encode(prep.g, self.ent_embeds, rel_embeds, reverse=not prep.subject, _lazy_bf16=True)

    @_moded
    def loss_prepared(self, prep):
        """Device half (model.py:82-103): RGCN x2 -> sequence assembly -> GRU x2 -> heads -> loss."""
        dev = self.ent_embeds.device
        b, g = prep.b, prep.g
        self.aggregator.last_batch = g
        if g is None:
            s_h = torch.zeros(b, self.h_dim, device=dev)
            s_q = torch.zeros(b, self.h_dim, device=dev)
        else:
            x, xr = self._encode(prep)
            s_h, s_q = ops.dual_gru(x, xr, self.encoder, self.encoder_r, prep.step_off, b)   # model.py:86-88, 94-96
            s_h, s_q = s_h.view(s_h.shape[1:]), s_q.view(s_q.shape[1:])
        return self._heads(prep, s_h, s_q)

    @_moded
    def loss_prepared_pair(self, prep_s, prep_o):
        """loss_prepared(prep_s) + loss_prepared(prep_o) -- the subject and the object pass of one training step
        (train.py:136-138) -- with the four GRU recurrences of the two passes in ONE launch per direction of time
        (extension of the reference API: the passes are independent until their losses are added, and a pass's two
        recurrences occupy only ~120 of the 256 CUs).  Same arithmetic, same results."""
        if prep_s.g is None or prep_o.g is None:
            return self.loss_prepared(prep_s) + self.loss_prepared(prep_o)
        xs, xrs = self._encode(prep_s)
        xo, xro = self._encode(prep_o)
        e, er = self.encoder, self.encoder_r
        w = (e.weight_ih_l0, e.weight_hh_l0, e.bias_ih_l0, e.bias_hh_l0)
        wr = (er.weight_ih_l0, er.weight_hh_l0, er.bias_ih_l0, er.bias_hh_l0)
        hd = self.h_dim
        hs, qs, ho, qo = ops.MultiGRUFn.apply([prep_s.step_off, prep_s.step_off, prep_o.step_off, prep_o.step_off],
                                              [prep_s.b, prep_s.b, prep_o.b, prep_o.b],
                                              [xs.shape[1] - hd, xrs.shape[1] - hd, xo.shape[1] - hd, xro.shape[1] - hd],
                                              xs, *w, xrs, *wr, xo, *w, xro, *wr)
        return self._heads(prep_s, hs[0], qs[0]) + self._heads(prep_o, ho[0], qo[0])

    @_moded
    def forward(self, triplets, s_hist, o_hist, graph_dict, subject=True):
        """Training loss of one direction (model.py:64-104): CE over objects + 0.1 * CE over relations.
        triplets: int tensor [B, >=3]; s_hist / o_hist: (histories, timestamps) in the reference's nested
        list layout, or graph.FlatHistory objects."""
        if not torch.is_grad_enabled():
            self._fused_pending = None                 # (a no_grad forward between the two calls of a fused step: start over)
        if self.fuse_directions and self.training and torch.is_grad_enabled():
            out = self._forward_fused(triplets, s_hist, o_hist, graph_dict, subject)
            if out is not None:
                return out
        return self.loss_prepared(self.prepare(triplets, s_hist if subject else o_hist, graph_dict, subject))

    def _prepare_both_lists_device(self, triplets, s_hist, o_hist, graph_dict):
        """prepare_both() for a batch that arrives through the reference's LIST API, with the batch graph built by the DEVICE
        builder (csrc/builder_both.hip): the nested lists are flattened on the host (graph.FlatHistory.from_lists), uploaded with
        the batch's (s, r, o) in one copy (gpu_builder.ListBatchStore) and everything else -- node sets, induced edges,
        norm, plans: utils.py:209-244 + 115-131 + dgl.batch -- is kernels; the arrays are those of the host builder
        (tests/test_gpu_builder.py).  None when a direction has no history at all (the caller takes the host path)."""
        import gpu_builder
        trip = triplets.detach().cpu().numpy() if isinstance(triplets, torch.Tensor) else np.asarray(triplets)
        fs = s_hist if isinstance(s_hist, G.FlatHistory) else G.FlatHistory.from_lists(s_hist[0], s_hist[1])
        fo = o_hist if isinstance(o_hist, G.FlatHistory) else G.FlatHistory.from_lists(o_hist[0], o_hist[1])
        if fs.seq_ptr[-1] == 0 or fo.seq_ptr[-1] == 0:
            return None
        longest = max(int(np.diff(fs.seq_ptr).max()), int(np.diff(fo.seq_ptr).max()))
        if longest > self.seq_len:
            raise ValueError('history longer than seq_len (%d > %d)' % (longest, self.seq_len))
        base = gpu_builder.graph_store_for(graph_dict, self.global_emb, self.in_dim, self.num_rels, self.ent_embeds.device)
        for _ in range(8):                                  # (a capacity grew: rebuild; first batches only)
            st = gpu_builder.ListBatchStore(base, trip, fs, fo)
            prep = self.finish_prepare_device(gpu_builder.DeviceBatch(st, np.arange(len(trip)), self.seq_len))
            if prep is not None:
                return prep
        raise RuntimeError('device batch builder did not converge on its capacities')

    def _forward_fused(self, triplets, s_hist, o_hist, graph_dict, subject):
        """train.py:136-138 calls  model(batch, s_hist, o_hist, graph_dict, subject=True)  and then the same with
        subject=False  and adds the two losses.  With `fuse_directions` (opt-in: RENET_FUSE_DIRECTIONS=1 or the attribute) the
        FIRST call runs both directions as the merged pass the product loop uses (ONE host batch build, every kernel over the
        2B sequences, loss_prepared_both) and returns a tensor whose VALUE is the subject-direction loss and whose autograd
        graph is that of the SUM; the SECOND call, recognised by the identity of its arguments, returns the
        object-direction loss as a constant.  loss_s + loss_o then has the reference's value and gradient with half the
        launches and half the host work.  The contract is train.py's: every subject=True call is followed by the
        subject=False call on the same argument objects and the two results enter the total with EQUAL weight; a
        subject=True call while another is still pending raises instead of training on a silently wrong gradient."""
        pend = self._fused_pending
        if not subject:
            if pend is None:
                return None                            # an object-direction call on its own: the plain path
            args, loss_o = pend
            def same(a, b):          # (train.py builds the (hist, hist_t) tuples anew at every call: compare their members)
                return a is b or (isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b) and
                                  all(x is y for x, y in zip(a, b)))
            if not (same(args[0], triplets) and same(args[1], s_hist) and same(args[2], o_hist) and args[3] is graph_dict):
                raise RuntimeError('fuse_directions: model(..., subject=False) did not receive the argument objects of the '
                                   'preceding subject=True call (train.py:136-137); set model.fuse_directions = False')
            self._fused_pending = None
            return loss_o
        if pend is not None:
            self._fused_pending = None
            raise RuntimeError('fuse_directions: model(..., subject=True) was called again before the subject=False call '
                               'of the previous batch (its gradient already contains both directions)')
        prep = None
        if self.device_builder_lists and self.ent_embeds.is_cuda:
            prep = self._prepare_both_lists_device(triplets, s_hist, o_hist, graph_dict)
        if prep is None:
            prep = self.prepare_both(triplets, s_hist, o_hist, graph_dict)
        if prep is None:
            return None                                # a direction without any history: two plain passes
        tap = []
        total = self.loss_prepared_both(prep, row_tap=tap)
        rl, s1, s2 = tap[0]
        b2 = prep.b                                    # 2B rows in sorted order; perm: sorted position -> sequence (>= B: object side)
        if prep.perm is None:                          # device-built: the permutation stays on the device
            is_obj = prep.g._v['perm'][:b2] >= (b2 // 2)
        else:
            is_obj = torch.from_numpy(np.asarray(prep.perm) >= (b2 // 2)).to(rl.device)
        w = torch.cat((is_obj.to(rl.dtype) * s1, is_obj.to(rl.dtype) * s2))
        loss_o = torch.dot(rl, w)                      # the object-direction rows' share of `total` (no autograd graph)
        self._fused_pending = ((triplets, s_hist, o_hist, graph_dict), loss_o)
        return total - loss_o


class PreparedBatch(object):
    """Device-resident inputs of one direction of one step (see RENet.prepare)."""
    __slots__ = ('g', 'subject', 'b', 'perm', 's_idx', 'r_idx', 'o_idx', 'plan_s', 'plan_r', 'batch_sizes',
                 'step_off', 'r_label', 'share', 'sharded', '_step_batch')


def _device_plan(idx, device):
    p = G.SegPlan.host(idx)
    for f in ('order', 'seg_ptr', 'target'):
        setattr(p, f, torch.from_numpy(getattr(p, f)).to(device))
    return p


# =================================================================================================
# Inference-time state machine (reference model.py:107-446), restated on the HIP path.  Same public
# methods / attributes / semantics; what differs is mechanical:
#   * per-entity prediction caches are int64 numpy arrays [k,2] (the reference keeps torch tensors);
#   * the num_k sampled subjects (objects) of a new timestamp are de-duplicated before the expensive
#     pred_r_rank2 call and the result reused for every duplicate (the reference's `s in s_done`
#     test compares tensor identities and never fires, model.py:229-235; results are identical);
#   * candidate bookkeeping is array based instead of dicts keyed by tensor objects.
# =================================================================================================
def _as_int(x):
    return int(x.item()) if isinstance(x, torch.Tensor) else int(x)


def _linear_eval(lin, x):
    """y = x W^T + b on the MFMA GEMM (no autograd: inference only)."""
    return K.gemm(x.contiguous(), lin.weight, tb=True, bias=lin.bias)


def _init_history(self, triples, s_history, o_history, valid_triples, s_history_valid, o_history_valid,
                  test_triples=None, s_history_test=None, o_history_test=None):
    """model.py:107-165: per-entity rolling windows as of the end of training (+ valid/test entries whose
    last step is not later than the last training time)."""
    n = self.in_dim
    self._la = None                                   # (look-ahead table of evaluate_filter: a new evaluation pass starts)
    self.s_hist_test = [[] for _ in range(n)]
    self.o_hist_test = [[] for _ in range(n)]
    self.s_hist_test_t = [[] for _ in range(n)]
    self.o_hist_test_t = [[] for _ in range(n)]
    self.s_his_cache = [[] for _ in range(n)]
    self.o_his_cache = [[] for _ in range(n)]
    self.s_his_cache_t = [None for _ in range(n)]
    self.o_his_cache_t = [None for _ in range(n)]
    last_t = None
    for k in range(len(triples)):
        s, o, last_t = _as_int(triples[k][0]), _as_int(triples[k][2]), triples[k][3]
        self.s_hist_test[s] = list(s_history[0][k])
        self.s_hist_test_t[s] = list(s_history[1][k])
        self.o_hist_test[o] = list(o_history[0][k])
        self.o_hist_test_t[o] = list(o_history[1][k])
    for trip, sh, oh in ((valid_triples, s_history_valid, o_history_valid),
                         (test_triples, s_history_test, o_history_test)):
        if trip is None:
            continue
        for k in range(len(trip)):
            s, o = _as_int(trip[k][0]), _as_int(trip[k][2])
            st, ot = sh[1][k], oh[1][k]
            if len(st) != 0 and st[-1] <= last_t:
                self.s_hist_test[s] = list(sh[0][k])
                self.s_hist_test_t[s] = list(st)
            if len(ot) != 0 and ot[-1] <= last_t:
                self.o_hist_test[o] = list(oh[0][k])
                self.o_hist_test_t[o] = list(ot)


def _update_cache(self, s_his_cache, r, o_candidate):
    cache = s_his_cache
    """model.py:421-446: add (r, o) pairs to an entity's prediction cache, keeping pairs unique."""
    r = _as_int(r)
    cand = np.asarray(o_candidate.cpu() if isinstance(o_candidate, torch.Tensor) else o_candidate,
                      dtype=np.int64).reshape(-1) % self.in_dim
    if len(cache) == 0:
        return np.stack((np.full(len(cand), r, np.int64), cand), axis=1)
    cache = np.asarray(cache.cpu() if isinstance(cache, torch.Tensor) else cache, dtype=np.int64).reshape(-1, 2)
    known = cache[cache[:, 0] == r][:, 1]
    new = cand[~np.isin(cand, known)]
    if len(new) == 0:
        return cache
    return np.concatenate((cache, np.stack((np.full(len(new), r, np.int64), new), axis=1)), axis=0)


def _pred_r_rank2(self, s, r, subject=True):
    """model.py:168-211: joint distribution p(r, o | s, history) as [num_rels, in_dim] for ONE entity
    (s holds num_rels copies of it, r = arange(num_rels))."""
    ent_id = _as_int(s[0])
    R, dev = self.num_rels, self.ent_embeds.device
    if subject:
        hist, hist_t = self.s_hist_test[ent_id], self.s_hist_test_t[ent_id]
        rel_embeds, reverse = self.rel_embeds[:R], False
    else:
        hist, hist_t = self.o_hist_test[ent_id], self.o_hist_test_t[ent_id]
        rel_embeds, reverse = self.rel_embeds[R:], True
    ent_row = self.ent_embeds[ent_id].view(1, -1)
    if len(hist) == 0:
        s_h = torch.zeros(R, self.h_dim, device=dev)
        s_q0 = torch.zeros(1, self.h_dim, device=dev)
    else:
        # the R sequences differ only in the relation segment of X: run the graph part for one
        # sequence per relation through the same batch path (identical node sets => identical graph)
        s_arr = np.full(R, ent_id, dtype=np.int64)
        px, pxr = self.aggregator.predict_batch(([list(hist)] * R, [list(hist_t)] * R), s_arr, np.arange(R),
                                                self.ent_embeds, rel_embeds, self.graph_dict, self.global_emb,
                                                reverse=reverse)
        _, s_h = self.encoder(px, total_rows=R)
        _, s_q = self.encoder_r(pxr, total_rows=R)
        s_h, s_q0 = s_h[0], s_q[0][:1]
    feat = torch.cat((ent_row.expand(R, -1), s_h, rel_embeds), dim=1)
    p_o = torch.softmax(_linear_eval(self.linear, feat), dim=1)                      # [R, N_ent]
    p_r = torch.softmax(_linear_eval(self.linear_r, torch.cat((ent_row, s_q0), dim=1)).view(-1), dim=0)
    return p_o * p_r.view(R, 1)


def _sample(self, prob):
    """model.py:225-227: num_k draws from the global model's entity distribution."""
    return torch.distributions.categorical.Categorical(prob).sample(torch.Size([self.num_k]))


def _joint_topk_many(self, ents, prob, subject=True):
    with G.async_uploads():
        return _joint_topk_many_body(self, ents, prob, subject)


def _joint_topk_many_body(self, ents, prob, subject=True):
    """pred_r_rank2 + the per-entity top-k of model.py:229-258 for SEVERAL entities in one batch:
    one batch graph with separate member graphs per entity (build_batch group=entity: identical to one call per
    entity), one GRU launch, one [n*R, 3h] x [3h, N_ent] GEMM.  Returns {entity: (values[num_k], flat indices
    into [R, N_ent])} -- the same numbers as num_k separate pred_r_rank2 calls."""
    R, dev, H = self.num_rels, self.ent_embeds.device, self.h_dim
    if subject:
        hist_all, hist_t_all, rel_embeds, reverse = self.s_hist_test, self.s_hist_test_t, self.rel_embeds[:R], False
    else:
        hist_all, hist_t_all, rel_embeds, reverse = self.o_hist_test, self.o_hist_test_t, self.rel_embeds[R:], True
    out = {}
    # bound the [n*R, N_ent] score block: 2^28 floats = 1 GiB (of 288 GB), ~45 entities at ICEWS18 sizes -- an advance
    # at num_k 1000 is ~44 chunks instead of the ~180 of the 2^26 bound of rounds 1-3 (fixed cost per chunk ~1.5 ms)
    chunk = max(1, (1 << int(os.environ.get('RENET_ADVANCE_BLOCK_LOG2', '28'))) // max(R * self.in_dim, 1))
    ents = [int(e) for e in ents]
    for c0 in range(0, len(ents), chunk):
        es = ents[c0:c0 + chunk]
        n = len(es)
        s_h = torch.zeros(n * R, H, device=dev)
        s_q = torch.zeros(n, H, device=dev)
        have = [i for i, e in enumerate(es) if len(hist_all[e]) != 0]
        if have and self.broadcast_relations:
            # ONE history per entity (round 4).  The R sequences of an entity share graph, RGCN rows, entity and global
            # segments of X; only the relation segment differs, and it is constant over the steps.  So the batch is built
            # for len(have) sequences instead of len(have) * R (the host-side construction of the R-fold batches was
            # what an advance spent its time on: profiles/r03_c_infer_advance.txt), and the GRU input projection is
            #     Gi[(e, r), step] = ([h2 | ent | . | glob] W_ih^T + b_ih)[e, step]  +  (rel[r] W_ih[:, 2H:3H]^T)
            # a broadcast sum of a [S, 3H] and an [R, 3H] matrix; encoder_r's input has no relation segment at all.
            # The recurrence runs over all len(have) * R sequences as before (h depends on r through Gi).
            ents_h = np.asarray([es[i] for i in have], dtype=np.int64)
            hists = [hist_all[e] for e in ents_h]
            hts = [hist_t_all[e] for e in ents_h]
            px, pxr = self.aggregator.forward_grouped((hists, hts), ents_h, np.zeros(len(have), dtype=np.int64),
                                                      self.ent_embeds, rel_embeds, self.graph_dict, self.global_emb,
                                                      reverse, ents_h)
            nh = len(have)
            x = px.data                                                              # [S, 4H] packed, time-major
            w_ih, b_ih = self.encoder.weight_ih_l0, self.encoder.bias_ih_l0
            p_base = K.gemm(x[:, :2 * H], w_ih[:, :2 * H], tb=True, bias=b_ih)        # [h2 | ent] part + bias
            K.gemm(x[:, 3 * H:], w_ih[:, 3 * H:], tb=True, out=p_base, beta=1.0)      # + glob part
            q_rel = K.gemm(rel_embeds.contiguous(), w_ih[:, 2 * H:3 * H], tb=True)    # [R, 3H]
            gi = (p_base.view(-1, 1, 3 * H) + q_rel.view(1, R, 3 * H)).reshape(-1, 3 * H)
            bs = px.batch_sizes.numpy()
            off = ops.host_offsets(np.concatenate(([0], np.cumsum(bs))) * R)          # every step R times as wide
            hh, _ = K.gru_fwd(gi, off, H, self.encoder.weight_hh_l0.contiguous(), self.encoder.bias_hh_l0.contiguous(),
                              out_rows=nh * R)                                        # [nh * R, H], sorted position major
            _, qq = self.encoder_r(pxr, total_rows=nh)
            perm = G.h2d(self.aggregator.last_batch.host.perm, dev)                 # sorted position -> sequence
            have_t = G.h2d(np.asarray(have, dtype=np.int64), dev)
            s_h.view(n, R, H)[have_t[perm]] = hh.view(nh, R, H)
            s_q[have_t[perm]] = qq[0]
        elif have:
            seq_ent = np.repeat(np.asarray([es[i] for i in have], dtype=np.int64), R)
            seq_rel = np.tile(np.arange(R, dtype=np.int64), len(have))
            hists = [hist_all[e] for e in seq_ent]
            hts = [hist_t_all[e] for e in seq_ent]
            px, pxr = self.aggregator.forward_grouped((hists, hts), seq_ent, seq_rel, self.ent_embeds, rel_embeds,
                                                      self.graph_dict, self.global_emb, reverse, seq_ent)
            m = len(seq_ent)
            _, hh = self.encoder(px, total_rows=m)
            _, qq = self.encoder_r(pxr, total_rows=m)
            perm = torch.from_numpy(self.aggregator.last_batch.host.perm).to(dev)   # sorted position -> sequence
            rows = torch.as_tensor(have, device=dev).repeat_interleave(R) * R + \
                torch.arange(R, device=dev).repeat(len(have))
            h_seq = torch.empty(m, H, device=dev)
            q_seq = torch.empty(m, H, device=dev)
            h_seq[perm] = hh[0]
            q_seq[perm] = qq[0]
            s_h[rows] = h_seq
            s_q[torch.as_tensor(have, device=dev)] = q_seq[::R]                      # the R copies are identical
        es_t = G.h2d(np.asarray(es, dtype=np.int64), dev)                              # (async: the host runs ahead)
        ent_rows = self.ent_embeds[es_t]                                              # [n, H]
        feat = torch.cat((ent_rows.repeat_interleave(R, dim=0), s_h, rel_embeds.repeat(n, 1)), dim=1)
        logits = _linear_eval(self.linear, feat)                                     # [n*R, N_ent]
        logits_r = _linear_eval(self.linear_r, torch.cat((ent_rows, s_q), dim=1))    # [n, R]
        prob_e = prob[es_t].contiguous()
        if self.reference_shadowing or R > 1024 or not logits.is_cuda or \
                os.environ.get('RENET_TOPK') == 'torch':
            # the ORDER of an unsorted torch.topk result is observable through the shadowing quirk: keep
            # the reference's op sequence there
            p_o = torch.softmax(logits, dim=1)
            p_r = torch.softmax(logits_r, dim=1)
            joint = (p_o * p_r.reshape(n * R, 1)).view(n, R * self.in_dim)
            joint = joint * prob_e.view(n, 1)
            vals, idx = torch.topk(joint, self.num_k, dim=1, sorted=False)
        else:
            # fused: softmax x softmax x prob in ONE pass over the block, then an exact radix-select top-k
            K.joint_softmax(logits, R, logits_r, prob_e)
            vals, idx = K.topk_positive(logits.view(n, R * self.in_dim), self.num_k)
        for i, e in enumerate(es):
            out[e] = (vals[i], idx[i])
    return out


def _advance_side(self, picks, prob, subject):
    """model.py:229-258 (subjects) / 266-297 (objects): rank (r, o) continuations of every sampled entity,
    keep the globally best num_k and write them into the prediction caches."""
    picks_np = picks.detach().cpu().numpy().astype(np.int64)
    if self.prune_relations and not self.reference_shadowing and \
            getattr(self.update_cache, '__func__', None) is _update_cache:
        with torch.no_grad():               # callers outside torch.no_grad() exist (the reference's predict is not wrapped)
            win_ent, codes_np = self._winners_pruned(picks_np, prob.detach(), subject)
        self._shadow['s' if subject else 'o'] = int(win_ent[-1])          # (read under reference_shadowing only)
        return self._apply_winners(win_ent, codes_np, subject)
    uniq = np.unique(picks_np)                           # identical entities give identical results: compute once
    per_ent = self._joint_topk_many(uniq, prob, subject=subject)
    all_vals = torch.cat([per_ent[int(e)][0] for e in picks_np])          # sample order, duplicates included
    _, best = torch.topk(all_vals, self.num_k, sorted=False)
    best_np = best.cpu().numpy()
    cands = [int(picks_np[c // self.num_k]) for c in best_np]          # model.py:254-255: s = s_to_id[idx.item()]
    side = 's' if subject else 'o'
    self._shadow[side] = self.shadow_pick(side, cands) if self.shadow_pick is not None else cands[-1]
    # the winners' (r, o) codes in ONE gather + ONE copy (an int(tensor[i]) per winner is a device sync each)
    win_ent = picks_np[best_np // self.num_k]
    codes = torch.stack([per_ent[int(e)][1] for e in uniq])                # [n_uniq, num_k]
    rows = torch.from_numpy(np.searchsorted(uniq, win_ent)).to(codes.device)
    codes_np = codes[rows, torch.from_numpy(best_np % self.num_k).to(codes.device)].cpu().numpy().astype(np.int64)
    self._apply_winners(win_ent, codes_np, subject)


def _apply_winners(self, win_ent, codes_np, subject):
    """model.py:254-258: the winners (entity, code = r * N_ent + other entity) go into the prediction caches."""
    cache, cache_t = (self.s_his_cache, self.s_his_cache_t) if subject else (self.o_his_cache, self.o_his_cache_t)
    now = _as_int(self.latest_time)
    touched = self._touched_sets()[0 if subject else 1]
    if getattr(self.update_cache, '__func__', None) is not _update_cache:
        # update_cache was overridden: one call per winner, as the reference does (model.py:254-258)
        for e, code in zip(win_ent.tolist(), codes_np.tolist()):
            rr, other = code // self.in_dim, code % self.in_dim
            cache[e] = self.update_cache(cache[e], rr, np.asarray([other]))
            cache_t[e] = now
            touched.add(e)
        return
    per = {}
    for e, code in zip(win_ent.tolist(), codes_np.tolist()):
        per.setdefault(e, []).append((code // self.in_dim, code % self.in_dim))
    for e, pairs in per.items():
        cache[e] = _bulk_update_cache(cache[e], pairs)
        cache_t[e] = now
        touched.add(e)


def _scaled_softmax_topk(logits, scale, k):
    """top-k of softmax(logits, dim 1) * scale[:, None] over the WHOLE block -> (values [k], flat indices [k]).  The block is
    overwritten on the GPU (fused joint-softmax with one "relation" per row, then the radix select over the block as one row)."""
    rows, n = logits.shape
    if logits.is_cuda and os.environ.get('RENET_TOPK') != 'torch':
        K.joint_softmax(logits, 1, torch.zeros(rows, 1, device=logits.device), scale.contiguous())
        vals, idx = K.topk_positive(logits.view(1, rows * n), k)
        return vals[0], idx[0]
    joint = torch.softmax(logits, dim=1) * scale.view(rows, 1)
    return torch.topk(joint.view(-1), k, sorted=False)


def _winners_pruned(self, picks_np, prob, subject):
    """The winners of _advance_side WITHOUT scoring every (entity, relation) row (RENet.prune_relations; exact).
    Every candidate of row (e, r) is  softmax_o(...) * p_r[e, r] * prob[e]  <=  bound[e, r] = p_r[e, r] * prob[e],  and the
    bound needs no relation-specific work (p_r comes from encoder_r, one sequence per entity).  Rows are scored in blocks of
    DESCENDING bound; after each block the num_k-th largest candidate found so far is a lower bound of the final
    threshold (the reference takes the top num_k of the candidate multiset in which an entity sampled m times counts m
    times: its num_k-th largest value is >= the num_k-th largest DISTINCT candidate), so scoring stops at the first row whose
    bound lies below it -- no candidate of an unscored row can be among the winners.  Per block: GRU over the block's
    (entity, relation) sequences (input projection = entity part + relation part, as in the broadcast path), ONE
    [rows, 3h] x [3h, N_ent] GEMM, fused softmax * bound, radix-select top-k over the block.  Returns (entity of every
    winner [num_k], code = r * N_ent + other entity [num_k]), multiplicities expanded."""
    R, dev, H, N = self.num_rels, self.ent_embeds.device, self.h_dim, self.in_dim
    if subject:
        hist_all, hist_t_all, rel_embeds, reverse = self.s_hist_test, self.s_hist_test_t, self.rel_embeds[:R], False
    else:
        hist_all, hist_t_all, rel_embeds, reverse = self.o_hist_test, self.o_hist_test_t, self.rel_embeds[R:], True
    uniq, counts = np.unique(picks_np, return_counts=True)
    n = len(uniq)
    with G.async_uploads():
        # ---- everything that does not depend on the relation, for ALL sampled entities in one batch ----
        have = np.asarray([i for i, e in enumerate(uniq) if len(hist_all[e]) != 0], dtype=np.int64)
        s_q = torch.zeros(n, H, device=dev)
        pos_of = np.full(n, -1, dtype=np.int64)            # entity index -> position in the length-sorted batch
        if len(have):
            ents_h = uniq[have]
            px, pxr = self.aggregator.forward_grouped(([hist_all[e] for e in ents_h], [hist_t_all[e] for e in ents_h]),
                                                      ents_h, np.zeros(len(have), dtype=np.int64), self.ent_embeds,
                                                      rel_embeds, self.graph_dict, self.global_emb, reverse, ents_h)
            nh = len(have)
            x = px.data                                                              # [S, 4H] packed, time-major
            w_ih, b_ih = self.encoder.weight_ih_l0, self.encoder.bias_ih_l0
            p_base = K.gemm(x[:, :2 * H], w_ih[:, :2 * H], tb=True, bias=b_ih)        # [h2 | ent] part + bias
            K.gemm(x[:, 3 * H:], w_ih[:, 3 * H:], tb=True, out=p_base, beta=1.0)      # + glob part
            q_rel = K.gemm(rel_embeds.contiguous(), w_ih[:, 2 * H:3 * H], tb=True)    # [R, 3H]
            bs = px.batch_sizes.numpy().astype(np.int64)
            step_off = np.concatenate(([0], np.cumsum(bs)))
            lens_sorted = (bs[:, None] > np.arange(nh)[None, :]).sum(axis=0)          # steps of sorted position s
            _, qq = self.encoder_r(pxr, total_rows=nh)
            perm = np.asarray(self.aggregator.last_batch.host.perm, dtype=np.int64)   # sorted position -> sequence
            pos_of[have[perm]] = np.arange(nh)
            s_q[G.h2d(have[perm], dev)] = qq[0]
        es_t = G.h2d(uniq, dev)
        ent_rows = self.ent_embeds[es_t]                                              # [n, H]
        logits_r = _linear_eval(self.linear_r, torch.cat((ent_rows, s_q), dim=1))    # [n, R]
        bound = (torch.softmax(logits_r, dim=1) * prob[es_t].view(n, 1)).reshape(-1)  # [n * R]
        bound_sorted, order = torch.sort(bound, descending=True)
        order_np, bound_np = order.cpu().numpy(), bound_sorted.cpu().numpy()
        block = max(1, (1 << int(os.environ.get('RENET_ADVANCE_BLOCK_LOG2', '28'))) // max(N, 1))
        w_hh, b_hh = self.encoder.weight_hh_l0.contiguous(), self.encoder.bias_hh_l0.contiguous()
        vals_all, rows_all, obj_all = [], [], []
        tau, pos, total = 0.0, 0, n * R
        self.last_prune = {'rows': total, 'scored': 0, 'blocks': 0}
        while pos < total:
            if tau > 0.0 and float(bound_np[pos]) * (1.0 + 1e-4) < tau:
                break                       # (the factor: the bound and the candidates round p_r * prob differently)
            blk = order_np[pos:pos + block]
            pos += len(blk)
            e_idx, r_idx = blk // R, blk % R
            m = len(blk)
            hh_rows = torch.zeros(m, H, device=dev)
            sp = pos_of[e_idx]
            sel = np.nonzero(sp >= 0)[0]
            if len(sel):
                # the block's sequences, ordered by (position of the entity in the sorted batch, relation): lengths descend
                o2 = sel[np.lexsort((r_idx[sel], sp[sel]))]
                sp_s, rr_s = sp[o2], r_idx[o2]
                ln = lens_sorted[sp_s]
                k_t = [int(np.count_nonzero(ln > t)) for t in range(int(ln[0]))]
                idx_rows = np.concatenate([step_off[t] + sp_s[:k] for t, k in enumerate(k_t)])
                idx_rel = np.concatenate([rr_s[:k] for k in k_t])
                gi = p_base[G.h2d(idx_rows, dev)] + q_rel[G.h2d(idx_rel, dev)]
                off = ops.host_offsets(np.concatenate(([0], np.cumsum(k_t))))
                hh, _ = K.gru_fwd(gi, off, H, w_hh, b_hh, out_rows=len(o2))
                hh_rows[G.h2d(o2, dev)] = hh
            e_dev, r_dev = G.h2d(e_idx, dev), G.h2d(r_idx, dev)
            feat = torch.cat((ent_rows[e_dev], hh_rows, rel_embeds[r_dev]), dim=1)
            logits = _linear_eval(self.linear, feat)                                  # [m, N_ent]
            k = min(self.num_k, m * N)
            vals, idx = _scaled_softmax_topk(logits, bound[G.h2d(blk, dev)], k)
            vals_all.append(vals)
            rows_all.append(G.h2d(blk, dev)[torch.div(idx, N, rounding_mode='floor')])
            obj_all.append(idx % N)
            self.last_prune['scored'] += m
            self.last_prune['blocks'] += 1
            if pos < total:
                seen = torch.cat(vals_all)
                if seen.numel() >= self.num_k:
                    tau = float(torch.topk(seen, self.num_k, sorted=False)[0].min())
        vals_np = torch.cat(vals_all).cpu().numpy()
        rows_np = torch.cat(rows_all).cpu().numpy().astype(np.int64)
        obj_np = torch.cat(obj_all).cpu().numpy().astype(np.int64)
    # the top num_k of the multiset: distinct candidates by descending value, each counted as often as its entity was sampled
    by_val = np.argsort(-vals_np, kind='stable')
    mult = counts[rows_np[by_val] // R]
    last = int(np.searchsorted(np.cumsum(mult), self.num_k))          # first position where the running count reaches num_k
    take = by_val[:last + 1]
    mult = mult[:last + 1].copy()
    if int(mult.sum()) > self.num_k:
        mult[-1] -= int(mult.sum()) - self.num_k                       # the last one may enter with fewer copies
    win_ent = np.repeat(uniq[rows_np[take] // R], mult)
    codes = np.repeat((rows_np[take] % R) * N + obj_np[take], mult)
    return win_ent, codes


def _bulk_update_cache(cache_e, pairs):
    """The result of `for (r, o) in pairs: cache_e = update_cache(cache_e, r, [o])` (model.py:421-446: a pair is appended
    unless the cache already holds it) with ONE array rebuild instead of an np.isin + np.stack per pair."""
    old = np.asarray(cache_e, dtype=np.int64).reshape(-1, 2)
    seen = set(map(tuple, old.tolist()))
    add = []
    for pr in pairs:
        if pr not in seen:
            seen.add(pr)
            add.append(pr)
    if not add:
        return old
    return np.concatenate((old, np.asarray(add, dtype=np.int64).reshape(-1, 2)), axis=0)


def _touched_sets(self):
    """(subjects, objects) whose prediction cache is non-empty, kept by _advance_side so that rolling the histories and
    collecting the predicted facts walk ~2 * num_k entities instead of all 2 * N_ent.  Rebuilt by one full scan at the start
    of every advance (_advance_time drops the key) and whenever the cache lists were replaced."""
    key = (id(self.s_his_cache), id(self.o_his_cache))
    if getattr(self, '_touched_key', None) != key:
        self._touched = tuple({e for e in range(self.in_dim) if len(c[e]) != 0}
                              for c in (self.s_his_cache, self.o_his_cache))
        self._touched_key = key
    return self._touched


def _roll_histories(self):
    """model.py:305-321: move every non-empty prediction cache into the entity's rolling window."""
    touched = self._touched_sets()
    for k, (hist, hist_t, cache, cache_t) in enumerate(
            ((self.s_hist_test, self.s_hist_test_t, self.s_his_cache, self.s_his_cache_t),
             (self.o_hist_test, self.o_hist_test_t, self.o_his_cache, self.o_his_cache_t))):
        for e in sorted(touched[k]):
            if len(cache[e]) != 0:
                while len(hist[e]) >= self.seq_len:
                    hist[e].pop(0)
                    hist_t[e].pop(0)
                hist[e].append(np.asarray(cache[e], dtype=np.int64).copy())
                hist_t[e].append(cache_t[e])
                cache[e] = []
                cache_t[e] = None
        touched[k].clear()


def _cached_facts(self):
    """utils.get_data (utils.py:95-113) restricted to the entities whose caches are non-empty: the same unique
    (s, r, o) rows."""
    touched = self._touched_sets()
    rows = []
    for e in sorted(touched[0]):
        a = np.asarray(self.s_his_cache[e], dtype=np.int64).reshape(-1, 2)
        if len(a):
            rows.append(np.stack((np.full(len(a), e), a[:, 0], a[:, 1]), axis=1))
    for e in sorted(touched[1]):
        a = np.asarray(self.o_his_cache[e], dtype=np.int64).reshape(-1, 2)
        if len(a):
            rows.append(np.stack((a[:, 1], a[:, 0], np.full(len(a), e)), axis=1))
    if not rows:
        return None
    return np.unique(np.concatenate(rows), axis=0)


def _advance_time(self, t, global_model):
    """model.py:222-328: executed once when the evaluated stream moves to a new timestamp."""
    # the touched sets are trusted only WITHIN one advance: callers own the cache lists between advances (test.py:70-81 restores
    # them from checkpoints, element writes are legal), so every advance starts with one full scan (~3 ms at N_ent 23 033)
    self._touched_key = None
    _, _, prob_sub = global_model.predict(self.latest_time, self.graph_dict, subject=True)
    self._advance_side(self.sample_entities(prob_sub), prob_sub, subject=True)
    _, ob, _ = global_model.predict(t, self.graph_dict, subject=False)
    prob_ob = torch.softmax(ob.view(-1), dim=0)
    self._advance_side(self.sample_entities(prob_ob), prob_ob, subject=False)
    now = _as_int(self.latest_time)
    self.data = self._cached_facts()                                                 # = get_data(s_his_cache, o_his_cache)
    if self.data is not None:
        self.graph_dict[now] = get_big_graph(self.data, self.num_rels)               # model.py:301
    emb, _, _ = global_model.predict(self.latest_time, self.graph_dict, subject=True)
    self.global_emb[now] = emb.detach()                                              # model.py:302-303
    self.aggregator.glob_table.invalidate()
    self._roll_histories()
    self.latest_time = t
    self.data = None
    self._reset_candidates()


def _predict(self, triplet, s_hist, o_hist, global_model):
    """model.py:216-363: scores of one test quadruple in both directions -> (loss, sub_pred, ob_pred)."""
    s, r, o = _as_int(triplet[0]), _as_int(triplet[1]), _as_int(triplet[2])
    t = triplet[3].cpu() if isinstance(triplet[3], torch.Tensor) else triplet[3]
    if _as_int(self.latest_time) != _as_int(t):
        self._advance_time(t, global_model)
        if self.reference_shadowing:                 # model.py:229-297: `s`, `o` now name the last candidates
            s, o = int(self._shadow['s']), int(self._shadow['o'])
    R, dev = self.num_rels, self.ent_embeds.device

    def encode(ent_id, given_hist, hist, hist_t, rel_embeds, reverse):
        if len(given_hist[0]) == 0 or len(hist) == 0:                                 # model.py:332,342
            return torch.zeros(1, self.h_dim, device=dev)
        inp, _ = self.aggregator.predict((hist, hist_t), np.asarray([ent_id]), np.asarray([r]), self.ent_embeds,
                                         rel_embeds, self.graph_dict, self.global_emb, reverse=reverse)
        _, h = self.encoder(inp.view(1, len(hist), 4 * self.h_dim))
        return h[0]

    s_h = encode(s, s_hist, self.s_hist_test[s], self.s_hist_test_t[s], self.rel_embeds[:R], False)
    o_h = encode(o, o_hist, self.o_hist_test[o], self.o_hist_test_t[o], self.rel_embeds[R:], True)
    ob_pred = _linear_eval(self.linear, torch.cat((self.ent_embeds[s].view(1, -1), s_h,
                                                   self.rel_embeds[r].view(1, -1)), dim=1)).view(-1)
    sub_pred = _linear_eval(self.linear, torch.cat((self.ent_embeds[o].view(1, -1), o_h,
                                                    self.rel_embeds[R + r].view(1, -1)), dim=1)).view(-1)
    tgt = torch.tensor([o, s], device=dev, dtype=torch.int32)
    loss = K.softmax_ce(ob_pred.view(1, -1), tgt[:1], 1.0, False)[0] + \
        K.softmax_ce(sub_pred.view(1, -1), tgt[1:], 1.0, False)[0]                   # model.py:358-361
    return loss, sub_pred, ob_pred


def _rank(scores, label, filter_ids=None):
    """model.py:368-376 / 391-418: rank = #greater + (#equal - 1)/2 + 1 (ties averaged); the filtered variant
    zeroes the (sigmoid) scores of all other known-true completions first."""
    if filter_ids is not None:
        scores = torch.sigmoid(scores)
        ground = scores[label].clone()
        scores[filter_ids] = 0
        scores[label] = ground
    else:
        ground = scores[label]
    greater = int((scores > ground).sum().item())
    equal = int((scores == ground).sum().item())
    return greater + (equal - 1.0) / 2 + 1


def _evaluate(self, triplet, s_hist, o_hist, global_model):
    s, o = _as_int(triplet[0]), _as_int(triplet[2])
    loss, sub_pred, ob_pred = self.predict(triplet, s_hist, o_hist, global_model)
    return np.array([_rank(sub_pred, s), _rank(ob_pred, o)]), loss


def _param_version(*modules):
    return tuple(p._version for m in modules for p in m.parameters())


def _lookahead_filter(self, triplet, s_hist, o_hist, global_model, all_triplets):
    """test.py:104-139 and train.py:160-172 call evaluate_filter once per quadruple (~2 ms of launch-bound work each: 40 s
    per validation pass over YAGO) -- but every call also hands over `all_triplets`, which holds the whole evaluated
    stream.  With `lookahead_eval` (opt-in: RENET_LOOKAHEAD_EVAL=1; tools/run_reference_driver.py turns it on) the FIRST call
    at a timestamp evaluates ALL quadruples of all_triplets that carry this timestamp in one evaluate_filter_batch (the
    per-timestamp state update of predict() runs inside it, exactly where the sequential loop runs it) and later calls are
    answered from that table.  Same ranks as the per-quadruple path up to fp32 summation order of a batched vs a one-row
    GEMM (tests/test_gpu_parity.py::test_evaluate_filter_stream_equals_sequential_calls: losses to 1e-5, >= 99 % of the ranks
    identical, the rest off by one).  The table assumes the call's GIVEN histories are non-empty (model.py:332,342 only test
    their emptiness); a call whose given history is empty while the entity's rolling window is not takes the plain path.
    Returns None whenever the table does not apply."""
    q = triplet.tolist() if isinstance(triplet, torch.Tensor) else [int(x) for x in triplet]
    s, r, o, t = int(q[0]), int(q[1]), int(q[2]), int(q[3])
    la = self._la
    ver = _param_version(self, global_model)
    if la is None or la['t'] != t or la['at'] is not all_triplets or la['ver'] != ver or _as_int(self.latest_time) != t:
        at = self._la_at
        if at is None or at[0] is not all_triplets:
            arr = all_triplets.detach().cpu().numpy() if isinstance(all_triplets, torch.Tensor) else np.asarray(all_triplets)
            at = self._la_at = (all_triplets, arr.astype(np.int64)[:, :4])
        rows = at[1][at[1][:, 3] == t]
        rows = np.unique(rows, axis=0)
        if len(rows) == 0 or not np.any((rows[:, 0] == s) & (rows[:, 1] == r) & (rows[:, 2] == o)):
            return None
        res = {}
        for c in range(0, len(rows), 4096):
            blk = rows[c:c + 4096]
            given = ([[0]] * len(blk), None)                  # "non-empty": only len(given[i]) is read (predict_batch)
            rk, ls = self.evaluate_filter_batch(blk, given, given, global_model, all_triplets)
            ls = ls.detach().float().cpu()
            for i, row in enumerate(blk.tolist()):
                res[(row[0], row[1], row[2])] = (rk[i], ls[i])
        la = self._la = {'t': t, 'at': all_triplets, 'ver': _param_version(self, global_model), 'res': res}
    hit = la['res'].get((s, r, o))
    if hit is None:
        return None
    if (len(s_hist[0]) == 0 and len(self.s_hist_test[s]) != 0) or (len(o_hist[0]) == 0 and len(self.o_hist_test[o]) != 0):
        return None                                           # zero state on that side (model.py:332,342): the plain path
    return np.array(hit[0]), hit[1]


def _evaluate_filter(self, triplet, s_hist, o_hist, global_model, all_triplets):
    """model.py:384-419: time-agnostic filtered ranks of the gold subject and object."""
    if self.lookahead_eval and not self.reference_shadowing and not torch.is_grad_enabled():
        hit = self._lookahead_filter(triplet, s_hist, o_hist, global_model, all_triplets)
        if hit is not None:
            return hit
    s, r, o = _as_int(triplet[0]), _as_int(triplet[1]), _as_int(triplet[2])
    loss, sub_pred, ob_pred = self.predict(triplet, s_hist, o_hist, global_model)
    at = all_triplets
    obj_known = at[(at[:, 0] == s) & (at[:, 1] == r), 2]
    sub_known = at[(at[:, 2] == o) & (at[:, 1] == r), 0]
    rank_ob = _rank(ob_pred.clone(), o, obj_known.to(ob_pred.device).long())
    rank_sub = _rank(sub_pred.clone(), s, sub_known.to(sub_pred.device).long())
    return np.array([rank_sub, rank_ob]), loss


def _time_aware_ids(at, s, r, o, t):
    """The time-aware filter sets of the quadruple (s, r, o, t): (objects o' with (s, r, o', t) in all_triplets, subjects s'
    with (s', r, o, t) in it) -- evaluate_filter's selection (model.py:392-401) with the query's own timestamp added."""
    return at[(at[:, 0] == s) & (at[:, 1] == r) & (at[:, 3] == t), 2], at[(at[:, 2] == o) & (at[:, 1] == r) & (at[:, 3] == t), 0]


def _evaluate_time_filter(self, triplet, s_hist, o_hist, global_model, all_triplets):
    """Time-aware filtered ranks of the gold subject and object (extension of the reference API; the setting of RE-GCN, xERTE,
    TITer): evaluate_filter (model.py:384-419) with the filter sets restricted to the facts that carry the query's own
    timestamp.  Same mechanism -- sigmoid(score), the other known completions set to 0 --, so the time-aware set being a
    subset of the time-agnostic one gives rank_filtered <= rank_time_filtered.  This is the written definition and the
    sequential baseline of evaluate_all_batch / evaluate_all_stream."""
    s, r, o, t = (_as_int(triplet[k]) for k in range(4))
    loss, sub_pred, ob_pred = self.predict(triplet, s_hist, o_hist, global_model)
    obj_known, sub_known = _time_aware_ids(all_triplets, s, r, o, t)
    rank_ob = _rank(ob_pred.clone(), o, torch.as_tensor(obj_known).to(ob_pred.device).long())
    rank_sub = _rank(sub_pred.clone(), s, torch.as_tensor(sub_known).to(sub_pred.device).long())
    return np.array([rank_sub, rank_ob]), loss


def _host_quads(triplets):
    tr = triplets.detach().cpu().numpy() if isinstance(triplets, torch.Tensor) else np.asarray(triplets)
    return tr.astype(np.int64).reshape(-1, 4)


def _predict_batch(self, triplets, s_hist, o_hist, global_model, want_loss=True):
    """predict() for n test quadruples that share ONE timestamp, in one batch: row i of the result equals
    predict(triplets[i], (s_hist[0][i], s_hist[1][i]), (o_hist[0][i], o_hist[1][i]), global_model).
    The reference (and predict) build the batch graph of every quadruple separately, so the member graphs are kept
    separate per entity here (build_batch group=entity: same entity => same rolling history => same graphs)
    instead of being merged per timestamp as in training.  s_hist / o_hist: (list of the n given histories,
    list of their timestamp lists), i.e. slices of test.py's s_history_test / s_history_test_t.
    Returns (loss[n], sub_pred[n, in_dim], ob_pred[n, in_dim]); want_loss=False: loss is None (the caller takes it from the
    rank kernel, which reads the scores anyway)."""
    tr = _host_quads(triplets)
    n = len(tr)
    if n == 0 or np.any(tr[:, 3] != tr[0, 3]):
        raise ValueError('predict_batch takes the quadruples of ONE timestamp')
    if _as_int(self.latest_time) != int(tr[0, 3]):
        self._advance_time(torch.tensor(int(tr[0, 3])), global_model)
        if self.reference_shadowing:                 # only the call that advances the time is affected
            tr = tr.copy()
            tr[0, 0], tr[0, 2] = int(self._shadow['s']), int(self._shadow['o'])
    R, dev = self.num_rels, self.ent_embeds.device

    def encode(ents, rels, given, hist, hist_t, rel_embeds, reverse):
        h = torch.zeros(n, self.h_dim, device=dev)
        act = np.asarray([i for i in range(n) if len(given[i]) != 0 and len(hist[ents[i]]) != 0], dtype=np.int64)
        if len(act):                                                              # model.py:332,342
            e = ents[act]
            px, _ = self.aggregator.forward_grouped(([hist[k] for k in e], [hist_t[k] for k in e]), e, rels[act],
                                                    self.ent_embeds, rel_embeds, self.graph_dict, self.global_emb,
                                                    reverse, e)
            _, hh = self.encoder(px, total_rows=len(act))
            perm = self.aggregator.last_batch.host.perm                          # sorted position -> sequence
            h[torch.from_numpy(act[perm]).to(dev)] = hh[0]
        return h

    with torch.no_grad():
        s, r, o = tr[:, 0], tr[:, 1], tr[:, 2]
        s_h = encode(s, r, s_hist[0], self.s_hist_test, self.s_hist_test_t, self.rel_embeds[:R], False)
        o_h = encode(o, r, o_hist[0], self.o_hist_test, self.o_hist_test_t, self.rel_embeds[R:], True)
        si, ri, oi = (torch.from_numpy(x).to(dev) for x in (s, r, o))
        ob_pred = _linear_eval(self.linear, torch.cat((self.ent_embeds[si], s_h, self.rel_embeds[ri]), dim=1))
        sub_pred = _linear_eval(self.linear, torch.cat((self.ent_embeds[oi], o_h, self.rel_embeds[R + ri]), dim=1))
        loss = None
        if want_loss:
            loss = K.softmax_ce(ob_pred, oi.int(), 1.0, False) + K.softmax_ce(sub_pred, si.int(), 1.0, False)
    return loss, sub_pred, ob_pred


def _rank_rows(scores, label, filt_rows=None, filt_cols=None):
    """_rank for every row of scores[n, C] at once (label[n]); filt_rows/filt_cols list the (row, column) pairs
    of the other known-true completions (filtered setting).  Returns float64 ranks [n] (ties averaged)."""
    rows = torch.arange(scores.shape[0], device=scores.device)
    if filt_rows is not None:
        scores = torch.sigmoid(scores)
        ground = scores[rows, label].clone()
        scores[filt_rows, filt_cols] = 0
        scores[rows, label] = ground
    else:
        ground = scores[rows, label]
    greater = (scores > ground[:, None]).sum(dim=1).double()
    equal = (scores == ground[:, None]).sum(dim=1).double()
    return (greater + (equal - 1.0) / 2 + 1).cpu().numpy()


def _known_pairs(at, key_cols, val_col, keys):
    """For every row i of keys[n, 2]: the values all_triplets[:, val_col] of the facts whose key_cols equal
    keys[i] -> (row index, value) pair lists (the time-agnostic filter sets of model.py:392-401)."""
    at = np.asarray(at.cpu() if isinstance(at, torch.Tensor) else at, dtype=np.int64)
    span = int(at[:, list(key_cols) + [val_col]].max()) + 2
    code = at[:, key_cols[0]] * span + at[:, key_cols[1]]
    order = np.argsort(code, kind='stable')
    code_sorted = code[order]
    want = keys[:, 0] * span + keys[:, 1]
    lo, hi = np.searchsorted(code_sorted, want, 'left'), np.searchsorted(code_sorted, want, 'right')
    cnt = hi - lo
    rows = np.repeat(np.arange(len(keys)), cnt)
    vals = at[order[G.ragged_arange(lo, cnt)], val_col]
    return rows, vals


def _evaluate_filter_batch(self, triplets, s_hist, o_hist, global_model, all_triplets):
    """evaluate_filter() for the n quadruples of ONE timestamp (extension of the reference API): returns
    (ranks[n, 2] = (rank_sub, rank_ob) per row, loss[n]), row i equal to
    evaluate_filter(triplets[i], (s_hist[0][i], s_hist[1][i]), (o_hist[0][i], o_hist[1][i]), ...)."""
    tr = _host_quads(triplets)
    if self.device_rank:
        return _device_ranks(self, tr, s_hist, o_hist, global_model, FI.filter_index_for(self, all_triplets))
    loss, sub_pred, ob_pred = self.predict_batch(tr, s_hist, o_hist, global_model)
    dev = ob_pred.device
    s, r, o = tr[:, 0], tr[:, 1], tr[:, 2]
    ro, co = _known_pairs(all_triplets, (0, 1), 2, np.stack((s, r), axis=1))       # objects known for (s, r)
    rs, cs = _known_pairs(all_triplets, (2, 1), 0, np.stack((o, r), axis=1))       # subjects known for (o, r)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rank_ob = _rank_rows(ob_pred, t(o), t(ro), t(co))
    rank_sub = _rank_rows(sub_pred, t(s), t(rs), t(cs))
    return np.stack((rank_sub, rank_ob), axis=1), loss


def _device_ranks(self, tr, s_hist, o_hist, global_model, index):
    """(ranks[n, 2] = (rank_sub, rank_ob), loss[n]) of the quadruples tr of ONE timestamp from one renet_rank_rows launch
    per direction (csrc/rank.hip: counts and the cross-entropy from one read of the scores, which are not copied).
    index: the FilterIndex of the known facts (filtered ranks, model.py:391-418), or None (raw ranks, model.py:365-381)."""
    # with reference_shadowing the loss of a timestamp's first quadruple belongs to the shadowing entities while the ranks
    # are those of its own (model.py:229-297): predict_batch computes that loss, the kernel only counts
    own_loss = self.reference_shadowing
    loss, sub_pred, ob_pred = self.predict_batch(tr, s_hist, o_hist, global_model, want_loss=own_loss)
    dev = ob_pred.device
    s, r, o = tr[:, 0], tr[:, 1], tr[:, 2]
    label = torch.from_numpy(np.stack((s, o)).astype(np.int32)).to(dev)
    counts = []
    for side, pred, lab, keys in (('s', sub_pred, label[0], (o, r)), ('o', ob_pred, label[1], (s, r))):
        ptr, col = index.lookup(side, np.stack(keys, axis=1), dev) if index is not None else (None, None)
        cnt, ls = K.rank_rows(pred, lab, ptr, col, filtered=index is not None, want_loss=not own_loss)
        counts.append(cnt)
        if not own_loss:
            loss = ls if loss is None else loss + ls
    g, e = torch.stack(counts, dim=2).cpu().numpy().astype(np.float64)             # [2, n, 2] -> greater, equal [n, 2]
    return g + (e - 1.0) / 2 + 1, loss


def _evaluate_batch(self, triplets, s_hist, o_hist, global_model):
    """evaluate() (model.py:365-381: the raw, unfiltered ranks) for the n quadruples of ONE timestamp: returns
    (ranks[n, 2] = (rank_sub, rank_ob) per row, loss[n]), row i equal to
    evaluate(triplets[i], (s_hist[0][i], s_hist[1][i]), (o_hist[0][i], o_hist[1][i]), global_model)."""
    return _device_ranks(self, _host_quads(triplets), s_hist, o_hist, global_model, None)


SETTINGS = ('raw', 'filtered', 'time_filtered')          # the metric settings of evaluate_all_batch, in renet_rank_rows3's order


def _evaluate_all_batch(self, triplets, s_hist, o_hist, global_model, all_triplets):
    """The raw (evaluate), filtered (evaluate_filter) and time-aware filtered (evaluate_time_filter) ranks of the n quadruples
    of ONE timestamp from one predict_batch and one renet_rank_rows3 launch per direction (extension of the reference API):
    returns ({'raw': r, 'filtered': r, 'time_filtered': r}, loss[n]), every r float64 [n, 2] = (rank_sub, rank_ob).  A pass
    is not repeatable in place (predict_batch advances the inference state), and the scores are what a pass costs: the
    three settings are one read of them.  Always on the device (whatever device_rank says), the filter lists addressed in
    place in the resident FilterIndex tables."""
    tr = _host_quads(triplets)
    index = FI.filter_index_for(self, all_triplets)
    own_loss = self.reference_shadowing                    # as in _device_ranks: predict_batch computes that loss
    loss, sub_pred, ob_pred = self.predict_batch(tr, s_hist, o_hist, global_model, want_loss=own_loss)
    dev = ob_pred.device
    s, r, o, t = tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3]
    label = torch.from_numpy(np.stack((s, o)).astype(np.int32)).to(dev)
    counts = []
    for side, pred, lab, key in (('s', sub_pred, label[0], o), ('o', ob_pred, label[1], s)):
        lists = index.ranges_both(side, np.stack((key, r, t), axis=1), dev)
        cnt, ls = K.rank_rows3(pred, lab, *lists, want_loss=not own_loss)
        counts.append(cnt)
        if not own_loss:
            loss = ls if loss is None else loss + ls
    c = torch.stack(counts, dim=2).cpu().numpy().astype(np.float64)                # [6, n, 2]: (greater, equal) per setting
    return {name: c[2 * k] + (c[2 * k + 1] - 1.0) / 2 + 1 for k, name in enumerate(SETTINGS)}, loss


def _stream_groups(total_data, s_history, o_history, max_batch, evaluate, width=2):
    """A time-ordered stream in groups of consecutive quadruples of one timestamp (at most max_batch each), every group
    through evaluate(quadruples, s_hist, o_hist) -> (ranks[len, width], loss[len])."""
    tr = _host_quads(total_data)
    ranks, losses = np.zeros((len(tr), width)), np.zeros(len(tr), dtype=np.float32)
    for c, d in _stream_cuts(tr, max_batch):
        rk, ls = evaluate(tr[c:d], (s_history[0][c:d], s_history[1][c:d]), (o_history[0][c:d], o_history[1][c:d]))
        ranks[c:d], losses[c:d] = rk, ls.cpu().numpy()
    return ranks, losses


def _stream_cuts(tr, max_batch):
    """The groups [c, d) of a time-ordered stream: consecutive quadruples of one timestamp, at most max_batch each."""
    cut = np.concatenate(([0], np.nonzero(np.diff(tr[:, 3]))[0] + 1, [len(tr)]))
    for a, b in zip(cut[:-1], cut[1:]):
        for c in range(a, b, max_batch):
            yield c, min(b, c + max_batch)


def _evaluate_filter_stream(self, total_data, s_history, o_history, global_model, all_triplets, max_batch=4096):
    """test.py:104-139 for a whole time-ordered test stream: groups consecutive quadruples by timestamp and
    evaluates each group with evaluate_filter_batch (the per-timestamp state update of predict() runs once per
    group, exactly as in the sequential loop).  s_history / o_history: (histories, timestamps) per quadruple,
    as loaded by test.py.  Returns (ranks[len, 2], loss[len])."""
    return _stream_groups(total_data, s_history, o_history, max_batch,
                          lambda q, sh, oh: self.evaluate_filter_batch(q, sh, oh, global_model, all_triplets))


def _evaluate_stream(self, total_data, s_history, o_history, global_model, max_batch=4096):
    """test.py:104-139 with --raw for a whole time-ordered test stream: evaluate_filter_stream with the raw ranks of
    evaluate() (evaluate_batch per group).  Returns (ranks[len, 2], loss[len])."""
    return _stream_groups(total_data, s_history, o_history, max_batch,
                          lambda q, sh, oh: self.evaluate_batch(q, sh, oh, global_model))


def _evaluate_all_stream(self, total_data, s_history, o_history, global_model, all_triplets, max_batch=4096):
    """evaluate_stream, evaluate_filter_stream and the time-aware filtered setting from ONE pass over a time-ordered test
    stream (evaluate_all_batch per group; extension of the reference API).  Returns ({'raw': r, 'filtered': r,
    'time_filtered': r}, loss[len]), every r float64 [len, 2] as utils.rank_metrics takes it."""
    def group(q, sh, oh):
        rk, ls = self.evaluate_all_batch(q, sh, oh, global_model, all_triplets)
        return np.concatenate([rk[name] for name in SETTINGS], axis=1), ls
    ranks, loss = _stream_groups(total_data, s_history, o_history, max_batch, group, width=2 * len(SETTINGS))
    return {name: np.ascontiguousarray(ranks[:, 2 * k:2 * k + 2]) for k, name in enumerate(SETTINGS)}, loss


def _predict_topk_batch(self, triplets, s_hist, o_hist, global_model, k=10, all_triplets=None, setting='raw',
                        keep_gold=False):
    """The k best-ranked subjects of (?, r, o, t) and objects of (s, r, ?, t) for the n quadruples of ONE timestamp, from one
    predict_batch and one renet_hip.topk_rows call per direction (csrc/topk_rows.hip: renet_topk_rows up to 32768 entities,
    renet_topk_rows_wide beyond, up to 2^20, with the same results; extension of the reference API): returns
    {'sub': (idx, score, logp, n_valid), 'ob': (...)} as device tensors, row i belonging to triplets[i] -- idx int32 [n, k] by
    score descending, then entity id ascending, score and logp (log-softmax over ALL entities) beside it, n_valid [n] the
    number of filled slots (the rest: idx -1, -inf).  setting (one of SETTINGS) says which known completions are no
    candidates: 'raw' none, 'filtered' those known at any time, 'time_filtered' those known at the query's own timestamp
    (the lists addressed in place in the resident FilterIndex tables of all_triplets).  keep_gold=True leaves the quadruple's
    own entity in (an evaluator reads hits@k off the list); keep_gold=False removes it when it is a known fact (a server
    offers only what is new).  Like every evaluation pass, a call advances the inference state."""
    if setting not in SETTINGS:
        raise ValueError('setting must be one of %s, not %r' % (', '.join(SETTINGS), setting))
    if setting != 'raw' and all_triplets is None:
        raise ValueError("setting %r needs all_triplets (the known facts)" % setting)
    tr = _host_quads(triplets)
    index = FI.filter_index_for(self, all_triplets) if setting != 'raw' else None
    # the keys and the gold entities are the rows' own, also under reference_shadowing (as the ranks of _device_ranks are)
    _, sub_pred, ob_pred = self.predict_batch(tr, s_hist, o_hist, global_model, want_loss=False)
    dev = ob_pred.device
    s, r, o, t = tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3]
    gold = torch.from_numpy(np.stack((s, o)).astype(np.int32)).to(dev) if keep_gold else (None, None)
    out = {}
    for name, side, pred, keep, key in (('sub', 's', sub_pred, gold[0], o), ('ob', 'o', ob_pred, gold[1], s)):
        lists = (None, None, None)
        if index is not None:
            lists = index.ranges(side, np.stack((key, r, t) if setting == 'time_filtered' else (key, r), axis=1), dev)
        out[name] = K.topk_rows(pred, k, *lists, keep=keep)
    return out


def _predict_topk_stream(self, total_data, s_history, o_history, global_model, k=10, all_triplets=None, setting='raw',
                         keep_gold=False, max_batch=4096):
    """predict_topk_batch for a whole time-ordered test stream, in the per-timestamp groups of evaluate_stream.  Returns
    host arrays {'sub': (idx [len, k], score [len, k], logp [len, k], n_valid [len]), 'ob': (...)}."""
    tr = _host_quads(total_data)
    n = len(tr)
    res = {name: (np.full((n, k), -1, dtype=np.int32), np.full((n, k), -np.inf, dtype=np.float32),
                  np.full((n, k), -np.inf, dtype=np.float32), np.zeros(n, dtype=np.int32)) for name in ('sub', 'ob')}
    for c, d in _stream_cuts(tr, max_batch):
        got = self.predict_topk_batch(tr[c:d], (s_history[0][c:d], s_history[1][c:d]), (o_history[0][c:d], o_history[1][c:d]),
                                      global_model, k, all_triplets, setting, keep_gold)
        for name, parts in got.items():
            for dst, src in zip(res[name], parts):
                dst[c:d] = src.cpu().numpy()
    return res


# =================================================================================================
# Observed-history (single-step, ground-truth history) evaluation: at query time t every fact before t is known, the
# evaluated split's own included -- the protocol under which RE-GCN, xERTE and TITer report the time-aware filter.  No
# query depends on a model output, so a whole stream goes through the TRAINING path (device-built merged batches that
# mix timestamps, encoder under no_grad) instead of one generated graph per timestamp.  Nothing here reads or writes the
# multi-step state above (latest_time, the rolling windows and caches, graph_dict, global_emb, the candidate tables): the
# stream, its graphs and its global-embedding table live in a preprocess.ObservedStream / gpu_builder.ObservedStore.
# =================================================================================================
def _observed_store(obs):
    """obs: a preprocess.ObservedStream that has been made resident, or the gpu_builder.ObservedStore itself."""
    store = obs if hasattr(obs, 'glob') else getattr(obs, 'device', None)
    if store is None or not hasattr(store, 'glob'):
        raise ValueError('the observed stream is not resident: call obs.resident(model, global_model) first')
    return store


def _observed_launch(self, store, idx):
    """Enqueues the device builder for the stream positions idx (at most gpu_builder.MAX_BOTH: a merged batch holds two
    sequences per quadruple, and one workgroup sorts their lengths) -> (idx, the pending gpu_builder.DeviceBatch)."""
    import gpu_builder
    if self.training and self.drop_p > 0:
        raise RuntimeError('the observed evaluation pass runs in eval mode (model.eval())')
    return idx, gpu_builder.DeviceBatch(store, idx, self.seq_len)


def _observed_prepared(self, store, pending):
    """Waits for ONE pending batch of _observed_launch -> (its positions, the PreparedBatch)."""
    import gpu_builder
    idx, pend = pending
    prep = self.finish_prepare_device(pend, glob=store.glob)
    for _ in range(8):                      # a capacity overflow: finalize() has raised the store's capacities, rebuild
        if prep is not None:
            break
        prep = self.finish_prepare_device(gpu_builder.DeviceBatch(store, idx, self.seq_len), glob=store.glob)
    if prep is None:
        raise RuntimeError('device batch builder did not converge on its capacities')
    return idx, prep


def _eval_rows_torch(ent, rel, h_sorted, q_sorted, perm, s, r, o, num_rels):
    """The GEMM-ready rows of both directions in quadruple order (model.py:89, 98 for subject=True / False):
    feat_ob[i] = [ent[s_i] | h(seq i) | rel[r_i]], feat_sub[i] = [ent[o_i] | h(seq n + i) | rel[R + r_i]] and the relation
    head's [ent | q] (q_sorted None: None); h(seq) is the row of h_sorted at the position that perm (sorted position ->
    sequence) maps to seq.  About eight small launches per batch; a fused copy kernel was measured and left out
    (profiles/observed_eval.md)."""
    n = s.numel()
    h_seq = torch.empty_like(h_sorted)
    h_seq[perm] = h_sorted
    es, eo = ent[s], ent[o]
    feat_ob, feat_sub = torch.cat((es, h_seq[:n], rel[r]), dim=1), torch.cat((eo, h_seq[n:], rel[num_rels + r]), dim=1)
    if q_sorted is None:
        return feat_ob, feat_sub, None, None
    q_seq = torch.empty_like(q_sorted)
    q_seq[perm] = q_sorted
    return feat_ob, feat_sub, torch.cat((es, q_seq[:n]), dim=1), torch.cat((eo, q_seq[n:]), dim=1)


def _observed_features(self, store, pending, relation=False):
    """Builder -> encoder -> rows for ONE pending batch of _observed_launch: (feat_ob [n, 3H], feat_sub [n, 3H],
    featr_ob [n, 2H] or None, featr_sub) in the order of its positions."""
    dev, H, R = self.ent_embeds.device, self.h_dim, self.num_rels
    idx, prep = _observed_prepared(self, store, pending)
    g, b2 = prep.g, prep.b
    if g.S == 0:
        # every history of the batch is empty (the first timestamp of a stream).  The builder accepts that -- an empty
        # graph, N = E = S = 0 (tests/test_gpu_builder.py) -- but the encoder kernels would be launched over zero rows:
        # zero states, as loss_prepared gives a batch without a graph
        h_sorted = torch.zeros(b2, H, device=dev)
        q_sorted = h_sorted
    else:
        x, xr = self.aggregator.encode(g, self.ent_embeds, self.rel_embeds, reverse=False, _lazy_bf16=True)
        h_sorted, q_sorted = ops.dual_gru(x, xr, self.encoder, self.encoder_r, prep.step_off, b2)
        h_sorted, q_sorted = h_sorted.view(b2, H), q_sorted.view(b2, H)           # rows behind the non-empty ones are zero
    pos = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
    s, r, o = (store.t[k][pos].long() for k in ('q_s', 'q_r', 'q_o'))
    perm = g._v['perm'][:b2].long()                                                 # sorted position -> sequence, on the device
    return _eval_rows_torch(self.ent_embeds, self.rel_embeds, h_sorted, q_sorted if relation else None, perm, s, r, o, R)


def _observed_chunks(self, store, idx, relation=False):
    """The rows of _observed_features for idx, one ENCODER CHUNK after the other: idx[0 : MAX_BOTH], idx[MAX_BOTH : 2 MAX_BOTH],
    ... -- each chunk one merged batch graph, the builder of chunk k + 1 enqueued before chunk k is encoded.  As in the
    reference, the histories of a batch graph are merged per timestamp (utils.py:149-170), so a row depends on which other
    positions share its chunk: the chunks are a function of idx alone, never of how the scoring is cut."""
    import gpu_builder
    step = gpu_builder.MAX_BOTH
    pending = _observed_launch(self, store, idx[:step])
    for c in range(0, len(idx), step):
        ahead = _observed_launch(self, store, idx[c + step:c + 2 * step]) if c + step < len(idx) else None
        yield _observed_features(self, store, pending, relation)
        pending = ahead


def _observed_cuts(chunks, max_batch):
    """Regroups the per-chunk rows into scoring batches of max_batch positions (the last one shorter): yields
    (c, d, rows) for the positions [c, d) of idx."""
    cat = lambda parts: [None if p[0] is None else p[0] if len(p) == 1 else torch.cat(p) for p in zip(*parts)]
    held, have, c = [], 0, 0
    for rows in chunks:
        held.append(rows)
        have += rows[0].shape[0]
        if have < max_batch:
            continue
        rows = cat(held)
        for a in range(0, have - max_batch + 1, max_batch):
            yield c, c + max_batch, [None if x is None else x[a:a + max_batch] for x in rows]
            c += max_batch
        rest = have % max_batch
        held, have = ([[None if x is None else x[have - rest:] for x in rows]], rest) if rest else ([], 0)
    if have:
        yield c, c + have, cat(held)


def _observed_positions(store, idx):
    idx = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64).reshape(-1)
    if len(idx) == 0 or idx.min() < 0 or idx.max() >= store.n_quads:
        raise ValueError('observed pass: positions outside the stream (or none)')
    return idx


def _observed_scores(self, obs, idx):
    """The scores of the stream positions idx (ONE batch) under observed histories: (sub_pred [n, N_ent], ob_pred
    [n, N_ent]), ob_pred[i] the logits row that forward(..., subject=True) computes for quadruple idx[i] in eval mode
    (model.py:82-90) from its TRUE history in the whole stream, sub_pred[i] that of subject=False.  Up to
    gpu_builder.MAX_BOTH positions are one batch graph, as in forward; more are encoded in chunks of that size
    (_observed_chunks)."""
    store = _observed_store(obs)
    idx = _observed_positions(store, idx)
    with torch.no_grad():
        (_, _, (feat_ob, feat_sub, _, _)), = _observed_cuts(_observed_chunks(self, store, idx), len(idx))
        return _linear_eval(self.linear, feat_sub), _linear_eval(self.linear, feat_ob)


def _prior_rows(prior, store, idx):
    """The recurrence.QueryRows of the rows idx of `store` for the `prior=` keyword of the observed family; None without a
    prior (nothing is imported, built or launched then)."""
    if prior is None:
        return None
    import recurrence
    recurrence._checked(prior)
    return recurrence.QueryRows(store, idx)


def _ranks_of(counts):
    """counts int [2 k, ...] = (greater, equal) per setting -> k float64 rank arrays (ties averaged, model.py:368-376)."""
    c = counts.cpu().numpy().astype(np.float64)
    return [c[2 * k] + (c[2 * k + 1] - 1.0) / 2 + 1 for k in range(len(c) // 2)]


def _evaluate_observed(self, obs, idx, all_triplets=None, max_batch=4096, relation=False, prior=None):
    """Raw, filtered and time-aware filtered ranks of the stream positions idx under OBSERVED histories (extension of the
    reference API): ({'raw': r, 'filtered': r, 'time_filtered': r}, loss[len]), every r float64 [len, 2] = (rank_sub,
    rank_ob) as utils.rank_metrics takes it, loss the sum of the two directions' entity cross-entropies per row.  idx may
    span any timestamps; scoring batches are cut every max_batch positions, not at timestamp borders.  The cut does not
    change what is computed: the encoder's batch graphs are chunks of idx of a fixed size (_observed_chunks), so the ranks are
    those of observed_scores(obs, idx) whatever max_batch is -- it bounds the two [max_batch, N_ent] score matrices.
    all_triplets: the known
    facts of the filtered settings (None: the stream itself).  The filter keys (s, r, t) / (o, r, t) are the quadruples'
    own: every host lookup is done, and uploaded, before the first batch runs, the builder of chunk k + 1 is enqueued before
    chunk k is encoded, and the counts come back in one copy at the end.  One renet_rank_rows3 launch per direction per
    batch, as evaluate_all_batch.  A pass is repeatable in place and leaves the multi-step state untouched.
    relation=True: a third result {'rank': [len, 2], 'loss': [len, 2], 'entity_loss': [len, 2]} -- raw rank and row loss
    of the gold relation under linear_r (model.py:98-100; the head trained at weight 0.1), column 0 from the subject=False
    pass ([ent[o] | o_q]), column 1 from subject=True ([ent[s] | s_q]), and the entity loss split the same way.
    prior: a recurrence.RecurrencePrior (None: today's path, launch for launch) -- every entity score matrix goes through
    one renet_recurrence_mix_rows launch before it is ranked; ranks and loss are then those of the mixed distribution."""
    store = _observed_store(obs)
    idx = _observed_positions(store, idx)
    dev, n = self.ent_embeds.device, len(idx)
    mix_rows = _prior_rows(prior, store, idx)
    max_batch = max(1, int(max_batch))
    tr = store.quads[idx]
    s, r, o, t = tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3]
    index = FI.filter_index_for(store, all_triplets if all_triplets is not None else store.quads)
    lists = np.stack(index.ranges_both_host('s', np.stack((o, r, t), axis=1)) +
                     index.ranges_both_host('o', np.stack((s, r, t), axis=1)) + (s, o, r)).astype(np.int32)
    up = torch.from_numpy(lists).to(dev)                                            # [11, n]: ONE upload for the whole pass
    cols = {side: (index.resident(side, dev), index.resident(side, dev, timed=True)) for side in ('s', 'o')}
    counts = torch.empty(6, n, 2, device=dev, dtype=torch.int32)
    ent_loss = torch.empty(n, 2, device=dev)
    rel_counts = torch.empty(2, n, 2, device=dev, dtype=torch.int32) if relation else None
    rel_loss = torch.empty(n, 2, device=dev) if relation else None
    with torch.no_grad():
        for c, d, (feat_ob, feat_sub, featr_ob, featr_sub) in _observed_cuts(_observed_chunks(self, store, idx, relation), max_batch):
            for col, side, feat, featr, lab, base in ((0, 's', feat_sub, featr_sub, up[8], 0), (1, 'o', feat_ob, featr_ob, up[9], 4)):
                pred = _linear_eval(self.linear, feat)
                if mix_rows is not None:
                    pred = mix_rows.mix(prior, 'sub' if side == 's' else 'ob', pred, c, d)
                cnt, ls = K.rank_rows3(pred, lab[c:d], cols[side][0], up[base][c:d], up[base + 1][c:d],
                                       cols[side][1], up[base + 2][c:d], up[base + 3][c:d], want_loss=True)
                counts[:, c:d, col] = cnt
                ent_loss[c:d, col] = ls
                if relation:
                    cnt, ls = K.rank_rows(_linear_eval(self.linear_r, featr), up[10][c:d], filtered=False, want_loss=True)
                    rel_counts[:, c:d, col] = cnt
                    rel_loss[c:d, col] = ls
    ranks = dict(zip(SETTINGS, _ranks_of(counts)))
    loss = ent_loss.sum(dim=1).cpu().numpy()
    if not relation:
        return ranks, loss
    return ranks, loss, {'rank': _ranks_of(rel_counts)[0], 'loss': rel_loss.cpu().numpy(), 'entity_loss': ent_loss.cpu().numpy()}


def _predict_topk_observed(self, obs, idx, k=10, all_triplets=None, setting='raw', keep_gold=False):
    """predict_topk_batch under observed histories, for the stream positions idx as ONE batch: {'sub': (idx, score, logp,
    n_valid), 'ob': (...)} as device tensors, the layout and the meaning of setting / keep_gold as there; all_triplets None:
    the stream itself is the set of known facts."""
    if setting not in SETTINGS:
        raise ValueError('setting must be one of %s, not %r' % (', '.join(SETTINGS), setting))
    store = _observed_store(obs)
    idx = _observed_positions(store, idx)
    index = FI.filter_index_for(store, all_triplets if all_triplets is not None else store.quads) if setting != 'raw' else None
    sub_pred, ob_pred = self.observed_scores(store, idx)
    dev = ob_pred.device
    tr = store.quads[idx]
    s, r, o, t = tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3]
    gold = torch.from_numpy(np.stack((s, o)).astype(np.int32)).to(dev) if keep_gold else (None, None)
    out = {}
    for name, side, pred, keep, key in (('sub', 's', sub_pred, gold[0], o), ('ob', 'o', ob_pred, gold[1], s)):
        lists = (None, None, None)
        if index is not None:
            lists = index.ranges(side, np.stack((key, r, t) if setting == 'time_filtered' else (key, r), axis=1), dev)
        out[name] = K.topk_rows(pred, k, *lists, keep=keep)
    return out


# =================================================================================================
# Event forecasts under observed history: "what will entity s do next, and with whom?" -- the pairs (r, o) of a subject
# (direction 'ob'; the pairs (r, s) of an object: 'sub') under the model's own factorisation p(o | s, r, history) *
# p(r | s, history) (model.py:89-103; the second factor is the linear_r / encoder_r head).  Per history ("group": the
# positions of an encoder chunk that share entity, timestamp and direction) the entity head gives a block B [R, N_ent], row r
# the logits of the query whose relation is r, and the joint log-probability of a pair is
#     J[r, c] = B[r, c] + off[r],   off[r] = fp32(logsoftmax64(linear_r logits)[r] - logsumexp64(B[r, :]))
# as ONE fp32 addition (csrc/joint_rank.hip); the joint is never stored.  History, RGCN rows and encoder_r's state do not
# depend on r: the chunk is built and encoded once for its positions' own sequences, and only the relation segment of the GRU
# input (Gi = p_base + q_rel[r], the broadcast of _joint_topk_many) and of the head's feature row is R-fold.  As in the rest
# of the observed pass nothing of the multi-step state is read or written.
# =================================================================================================
EVENT_DIRECTIONS = (('sub', 0, 's', 2, 0), ('ob', 1, 'o', 0, 2))      # name, result column, filter side, given / ranked column


class _EventChunk(object):
    """What one encoder chunk holds for its blocks: p_base [S, 3H] (the relation-free part of encoder's input projection, bias
    included; None: every history of the chunk is empty), the packed layout (step_off, lens of the sorted positions), q_seq
    [2 n, H] (encoder_r's states by sequence) and per direction its groups -- ent [G], t [G], sp [G] (sorted position of the
    group's sequence; ascending, so the lengths descend), seq [G] and, for the chunk's positions, gid [n]."""


def _event_chunks(self, store, idx, mix=None):
    """One _EventChunk per encoder chunk of idx (the chunks of _observed_chunks: the same batch graphs), the builder of chunk
    k + 1 enqueued before chunk k is encoded.  mix: the recurrence.EventMix of a `prior=` call (None: nothing of it is made)
    -- every direction then carries q = (ent, t, as_of) of its groups, int32 device [G], the as_of that of the group's history
    window: the query's own t on an ObservedStore, the as_of of the group's first query on a QueryStore."""
    import gpu_builder
    dev, H = self.ent_embeds.device, self.h_dim
    step = gpu_builder.MAX_BOTH
    pending = _observed_launch(self, store, idx[:step])
    for c in range(0, len(idx), step):
        ahead = _observed_launch(self, store, idx[c + step:c + 2 * step]) if c + step < len(idx) else None
        pos, prep = _observed_prepared(self, store, pending)
        pending = ahead
        g, b2, n = prep.g, prep.b, len(pos)
        ch = _EventChunk()
        ch.c, ch.n = c, n
        if g.S == 0:                        # (the first timestamp of a stream: zero states, as _observed_features)
            ch.p_base, ch.step_off, ch.lens = None, np.zeros(1, dtype=np.int64), np.zeros(b2, dtype=np.int64)
            ch.q_seq = torch.zeros(b2, H, device=dev)
            pos_of = np.arange(b2)
        else:
            x, xr = self.aggregator.encode(g, self.ent_embeds, self.rel_embeds, reverse=False)
            w_ih, b_ih = self.encoder.weight_ih_l0, self.encoder.bias_ih_l0
            ch.p_base = K.gemm(x[:, :2 * H], w_ih[:, :2 * H], tb=True, bias=b_ih)          # [h2 | ent] part + bias
            K.gemm(x[:, 3 * H:], w_ih[:, 3 * H:], tb=True, out=ch.p_base, beta=1.0)        # + glob part
            er = self.encoder_r
            q_sorted = ops.GRUFn.apply(xr, er.weight_ih_l0, er.weight_hh_l0, er.bias_ih_l0, er.bias_hh_l0, prep.step_off, b2)
            perm = g.host.perm[:b2]                                                         # sorted position -> sequence
            ch.q_seq = torch.empty(b2, H, device=dev)
            ch.q_seq[g._v['perm'][:b2].long()] = q_sorted.view(b2, H)
            bs = g.host.batch_sizes
            ch.step_off = np.concatenate(([0], np.cumsum(bs))).astype(np.int64)
            ch.lens = (bs[:, None] > np.arange(b2)[None, :]).sum(axis=0)                    # steps of sorted position
            pos_of = np.empty(b2, dtype=np.int64)
            pos_of[perm] = np.arange(b2)
        _event_groups(ch, store, pos, pos_of, mix)
        yield ch


def _event_groups(ch, store, pos, pos_of, mix=None):
    """Fills ch.dirs: per direction the groups of the chunk's positions pos -- the positions that share the given entity and
    the timestamp --, ordered by the sorted position pos_of [2 n] of the group's first sequence."""
    n = len(pos)
    tr = store.quads[pos]
    ch.dirs = {}
    for name, col, side, given, ranked in EVENT_DIRECTIONS:
        keys, first, inv = np.unique(tr[:, [given, 3]], axis=0, return_index=True, return_inverse=True)
        seq = first + (n if name == 'sub' else 0)                   # sequence i: direction ob of position i, n + i: sub
        order = np.argsort(pos_of[seq], kind='stable')
        rank = np.empty(len(order), dtype=np.int64)
        rank[order] = np.arange(len(order))
        d = ch.dirs[name] = _EventChunk()
        d.ent, d.t, d.seq, d.sp, d.gid = keys[order, 0], keys[order, 1], seq[order], pos_of[seq[order]], rank[inv.reshape(-1)]
        if mix is not None:
            d.q = mix.groups(store, d.ent, d.t, np.asarray(pos)[first[order]])


def _event_blocks(self, ch, name, q_rel, block_floats, mix=None):
    """The blocks of one direction of a chunk in sub-blocks of at most block_floats floats (at least one group): yields
    (g0, g1, B [(g1 - g0) * R, N_ent], off [(g1 - g0) * R]) for the groups [g0, g1), the rows group-major, then relation.  Per
    sub-block: the p_base rows of its groups' steps + the q_rel broadcast, ONE recurrence over the R-fold sequences (ordered
    by sorted position, then relation: the lengths descend, the row order of _winners_pruned), the rows [ent | h | rel_r], one
    score GEMM, renet_joint_row_offsets -- and, with mix (a recurrence.EventMix), ONE renet_joint_mix_rows call behind it: B and
    off then hold the mixed joint (off zero on the groups with history)."""
    d = ch.dirs[name]
    per = _event_groups_per_block(self, block_floats)
    for g0 in range(0, len(d.ent), per):
        g1 = min(len(d.ent), g0 + per)
        block, off = _event_block(self, ch, name, q_rel, np.arange(g0, g1))
        if mix is not None:
            mix.apply(name, block, off, d.q, g0, g1)
        yield g0, g1, block, off


def _event_groups_per_block(self, block_floats):
    return max(1, int(block_floats) // max(self.num_rels * self.in_dim, 1))


def _event_block(self, ch, name, q_rel, sel):
    """(B [m * R, N_ent], off [m * R]) of the groups sel [m] of one direction of a chunk -- ascending group indices, so that
    the lengths descend; rows in sel's order, group-major."""
    R, dev, H = self.num_rels, self.ent_embeds.device, self.h_dim
    d = ch.dirs[name]
    rel = self.rel_embeds[R:] if name == 'sub' else self.rel_embeds[:R]
    w_hh, b_hh = self.encoder.weight_hh_l0.contiguous(), self.encoder.bias_hh_l0.contiguous()
    m = len(sel)
    sp = d.sp[sel]
    ln = ch.lens[sp]                                                # descending
    if ch.p_base is not None and ln[0] > 0:
        k_t = [int(np.count_nonzero(ln > t)) for t in range(int(ln[0]))]
        rows = np.concatenate([ch.step_off[t] + sp[:k] for t, k in enumerate(k_t)])
        gi = (ch.p_base[G.h2d(rows, dev)].view(-1, 1, 3 * H) + q_rel.view(1, R, 3 * H)).reshape(-1, 3 * H)
        off = ops.host_offsets(np.concatenate(([0], np.cumsum(k_t))) * R)                  # every step R times as wide
        hh, _ = K.gru_fwd(gi, off, H, w_hh, b_hh, out_rows=m * R)                          # [m * R, H]; rows past k_t[0] * R zero
    else:
        hh = torch.zeros(m * R, H, device=dev)
    ent_rows = self.ent_embeds[G.h2d(d.ent[sel], dev)]                                      # [m, H]
    feat = torch.cat((ent_rows.repeat_interleave(R, dim=0), hh[:m * R], rel.repeat(m, 1)), dim=1)
    block = _linear_eval(self.linear, feat)                                                 # [m * R, N_ent]
    logits_r = _linear_eval(self.linear_r, torch.cat((ent_rows, ch.q_seq[G.h2d(d.seq[sel], dev)]), dim=1))
    return block, K.joint_row_offsets(block, R, logits_r)


def _event_mix(prior):
    """The recurrence.EventMix of the `prior=` keyword of the event family; None without a prior (nothing is imported, built
    or launched then)."""
    if prior is None:
        return None
    import recurrence
    return recurrence.EventMix(prior)


def _event_setup(self, obs, idx):
    store = _observed_store(obs)
    idx = _observed_positions(store, idx)
    if self.num_rels > 1024:
        raise ValueError('event forecasts take at most 1024 relations (renet_joint_row_offsets)')
    return store, idx


def _event_q_rel(self):
    """{direction: rel_embeds of the direction against the relation segment of encoder's w_ih, [R, 3H]}."""
    R, H = self.num_rels, self.h_dim
    w = self.encoder.weight_ih_l0[:, 2 * H:3 * H]
    return {'ob': K.gemm(self.rel_embeds[:R].contiguous(), w, tb=True), 'sub': K.gemm(self.rel_embeds[R:].contiguous(), w, tb=True)}


def _observed_event_scores(self, obs, idx, block_floats=1 << 28, prior=None):
    """The blocks of the stream positions idx under observed histories (for small n: tests, inspection): {'ob': (B [n, R,
    N_ent], off [n, R]), 'sub': (...)} as device tensors.  B[i, r] is the logits row observed_scores(obs, idx) computes for
    position i in that direction if the quadruple's relation were r (the same encoder chunks, true history and global table;
    the GRU input projection is associated differently), off[i, r] the row's offset: J = B + off[..., None] in fp32 is the
    joint log-probability that evaluate_events_observed ranks.  ValueError if n * R * N_ent exceeds block_floats.
    prior: a recurrence.RecurrencePrior or a CopyGate(per_relation=False) -- the pair is then (M, off) AFTER
    renet_joint_mix_rows: for a position whose given entity has history before its as_of, B holds the mixed joint M and off
    is ZERO (M + 0 is M); a position without history keeps its (B, off) bit for bit.  J = B + off[..., None] in fp32 holds
    either way."""
    store, idx = _event_setup(self, obs, idx)
    mix = _event_mix(prior)
    n, R, N = len(idx), self.num_rels, self.in_dim
    if n * R * N > int(block_floats):
        raise ValueError('observed_event_scores: %d positions x %d relations x %d entities exceed block_floats = %d'
                         % (n, R, N, int(block_floats)))
    dev = self.ent_embeds.device
    out = {name: (torch.empty(n, R, N, device=dev), torch.empty(n, R, device=dev)) for name in ('ob', 'sub')}
    with torch.no_grad():
        q_rel = _event_q_rel(self)
        for ch in _event_chunks(self, store, idx, mix):
            for name in ('sub', 'ob'):
                gid = G.h2d(ch.dirs[name].gid, dev)
                for g0, g1, block, off in _event_blocks(self, ch, name, q_rel[name], block_floats, mix):
                    here = torch.nonzero((gid >= g0) & (gid < g1)).view(-1)
                    out[name][0][ch.c + here] = block.view(g1 - g0, R, N)[gid[here] - g0]
                    out[name][1][ch.c + here] = off.view(g1 - g0, R)[gid[here] - g0]
    return out


def _event_known(d, R):
    """The filter keys of every (group, relation) row of one direction of a chunk, group-major: (entity, r', t) [G * R, 3]."""
    return np.stack((np.repeat(d.ent, R), np.tile(np.arange(R, dtype=np.int64), len(d.ent)), np.repeat(d.t, R)), axis=1)


def _evaluate_events_observed(self, obs, idx, all_triplets=None, block_floats=1 << 28, prior=None):
    """Ranks of the gold EVENT of the stream positions idx under observed histories (extension of the reference API):
    {'pair': {setting: float64 [len, 2]}, 'relation': {setting: float64 [len, 2]}, 'logp': float32 [len, 2]}, column 0 the
    direction sub (the object given: pairs (r, s)), column 1 ob (the subject given: pairs (r, o)); the settings are SETTINGS.
    With J the joint log-probabilities of the position's block (observed_event_scores) and v = J[r*, gold entity] (= logp):
      pair      rank of the gold pair among the R * N_ent pairs, greater + (equal - 1) / 2 + 1 on the fp32 values J; under
                'filtered' the pairs (r', e') for which (s, r', e') -- (e', r', o) for sub -- is a known fact at any time are no
                candidates at all, under 'time_filtered' those known at the query's own timestamp; the gold pair stays;
      relation  rank of r* among J[:, gold entity] (both endpoints given), ties averaged; the filtered settings drop the
                relations r' != r* for which the triple with both endpoints is known (at t).
    all_triplets: the known facts (None: the stream itself).  Per encoder chunk the host filter lookups of every (group,
    relation) row are done and uploaded before its sub-blocks run (block_floats bounds a sub-block's score block); one
    renet_joint_row_offsets and one renet_joint_rank_rows launch per sub-block; the counts come back in one copy at the end.
    Repeatable in place; the multi-step state is untouched.
    prior: a recurrence.RecurrencePrior or a CopyGate(per_relation=False) (None: today's launches and results) -- one
    renet_joint_mix_rows call per sub-block between the offsets and the rank launch; ranks and logp are then those of the
    MIXED joint (recurrence.py): to be reported with alpha and half_life, beside recurrence.evaluate_events' baseline."""
    store, idx = _event_setup(self, obs, idx)
    mix = _event_mix(prior)
    dev = self.ent_embeds.device
    with torch.no_grad():
        q_rel = _event_q_rel(self)
        return _rank_events(store, idx, self.num_rels, dev, all_triplets, _event_chunks(self, store, idx, mix),
                            lambda ch, name: _event_blocks(self, ch, name, q_rel[name], block_floats, mix))


def _rank_events(store, idx, R, dev, all_triplets, chunks, blocks):
    """The rank tail of evaluate_events_observed over any source of joint blocks: `chunks` yields the _EventChunks of idx (c,
    dirs), blocks(ch, name) the sub-blocks (g0, g1, B, off) of one direction of a chunk.  recurrence.evaluate_events runs it
    over uniform blocks: the same groups, filter lists and tie rule.  Called under no_grad."""
    n = len(idx)
    index = FI.filter_index_for(store, all_triplets if all_triplets is not None else store.quads)
    cols = {side: (index.resident(side, dev), index.resident(side, dev, timed=True)) for side in ('s', 'o')}
    gold = torch.from_numpy(np.ascontiguousarray(store.quads[idx][:, :3].T).astype(np.int32)).to(dev)      # s, r, o
    pair = torch.zeros(6, n, 2, device=dev, dtype=torch.int64)
    rel = torch.zeros(6, n, 2, device=dev, dtype=torch.int64)
    logp = torch.empty(n, 2, device=dev)
    rels = torch.arange(R, device=dev).view(1, R)
    for ch in chunks:
        # every host lookup of the chunk, and its upload, before the first sub-block runs
        ups = {}
        for name, col, side, given, ranked in EVENT_DIRECTIONS:
            d = ch.dirs[name]
            by_group = np.argsort(d.gid, kind='stable')                                # the chunk's positions, group-major
            lists = np.stack(index.ranges_both_host(side, _event_known(d, R))).astype(np.int32)
            ups[name] = (by_group, d.gid[by_group], G.h2d(by_group, dev), G.h2d(d.gid[by_group].astype(np.int32), dev),
                         torch.from_numpy(lists).to(dev).view(4, len(d.ent), R))
        for name, col, side, given, ranked in EVENT_DIRECTIONS:
            by_group, gid_h, here, gid, lists = ups[name]
            for g0, g1, block, off in blocks(ch, name):
                a, b = np.searchsorted(gid_h, (g0, g1))
                pos = ch.c + here[a:b]                                                  # positions of idx, group-major
                grp = gid[a:b] - g0
                gr, gc = gold[1][pos].contiguous(), gold[ranked][pos].contiguous()
                rows = lists[:, g0:g1][:, grp.long()].reshape(4, -1).contiguous()       # [4, Q * R]: per (query, relation)
                cnt, at_gold, listed, _ = K.joint_rank_rows(block, R, off, grp.contiguous(), gr, gc, cols[side][0], rows[0],
                                                            rows[1], cols[side][1], rows[2], rows[3])
                pair[:, pos, col] = cnt
                v = at_gold.gather(1, gr.long().view(-1, 1))
                logp[pos, col] = v.view(-1)
                own = rels == gr.long().view(-1, 1)
                for k, keep in enumerate((None, (listed[0] == 0) | own, (listed[1] == 0) | own)):
                    gt, eq = at_gold > v, at_gold == v
                    rel[2 * k, pos, col] = (gt if keep is None else gt & keep).sum(dim=1)
                    rel[2 * k + 1, pos, col] = (eq if keep is None else eq & keep).sum(dim=1)
    # ONE copy: the counts of both kinds and logp as [13, n, 2] float64 (counts and fp32 values are exact in it)
    back = torch.cat((pair.double(), rel.double(), logp.double().view(1, n, 2))).cpu().numpy()
    ranks = [{name: c[2 * k] + (c[2 * k + 1] - 1.0) / 2 + 1 for k, name in enumerate(SETTINGS)} for c in (back[0:6], back[6:12])]
    return {'pair': ranks[0], 'relation': ranks[1], 'logp': back[12].astype(np.float32)}


def _predict_events_observed(self, obs, idx, k=10, all_triplets=None, setting='raw', sides=('sub', 'ob'), prior=None):
    """The k most probable events of the stream positions idx under observed histories: {'ob': (rel int32 [n, k], ent int32
    [n, k], logp [n, k], n_valid int32 [n]), 'sub': (...)} as device tensors -- for 'ob' the pairs (r, o) of the position's
    subject, for 'sub' the pairs (r, s) of its object, by joint log-probability J descending, then relation, then entity
    ascending (deterministic); logp is J, bit for bit B + off of observed_event_scores.  setting (one of SETTINGS) says which
    known facts are no candidates, as in predict_topk_observed; there is no keep_gold: hits are read from the ranks of
    evaluate_events_observed.  n_valid = min(k, candidates); the slots behind it hold -1, -1, -inf.  Per sub-block one
    renet_topk_rows launch gives every relation row's k best entities, and the k best of those R * k candidates are taken
    (a pair outside its own row's k best by SCORE cannot enter: exact unless two distinct scores of a row round to one J at
    that row's k-th place).  k <= 1024; N_ent <= 2^20 (renet_hip.topk_rows: beyond 32768 entities the rows are taken in
    pieces by renet_topk_rows_wide, with the same results).  sides: the directions to compute; one left out costs no
    block and is missing from the result.  prior: as in evaluate_events_observed -- the k best of the mixed joint, logp its
    log-probability, bit for bit B + off of observed_event_scores(prior=)."""
    if setting not in SETTINGS:
        raise ValueError('setting must be one of %s, not %r' % (', '.join(SETTINGS), setting))
    store, idx = _event_setup(self, obs, idx)
    mix = _event_mix(prior)
    dev = self.ent_embeds.device
    with torch.no_grad():
        q_rel = _event_q_rel(self)
        return _topk_events(store, idx, int(k), self.num_rels, self.in_dim, dev, all_triplets, setting, sides,
                            _event_chunks(self, store, idx, mix),
                            lambda ch, name: _event_blocks(self, ch, name, q_rel[name], 1 << 28, mix))


def _topk_events(store, idx, k, R, N, dev, all_triplets, setting, sides, chunks, blocks):
    """The top-k tail of predict_events_observed over any source of joint blocks (chunks / blocks as in _rank_events);
    recurrence.topk_events runs it over uniform blocks.  Called under no_grad."""
    n = len(idx)
    index = FI.filter_index_for(store, all_triplets if all_triplets is not None else store.quads) if setting != 'raw' else None
    out = {name: (torch.full((n, k), -1, device=dev, dtype=torch.int32), torch.full((n, k), -1, device=dev, dtype=torch.int32),
                  torch.full((n, k), -np.inf, device=dev), torch.zeros(n, device=dev, dtype=torch.int32))
           for name in ('ob', 'sub') if name in sides}
    for ch in chunks:
        for name, col, side, given, ranked in EVENT_DIRECTIONS:
            if name not in sides:
                continue
            d = ch.dirs[name]
            lists = (None, None, None)
            if index is not None:
                keys = _event_known(d, R)
                lists = index.ranges(side, keys if setting == 'time_filtered' else keys[:, :2], dev)
            gid = G.h2d(d.gid, dev)
            for g0, g1, block, off in blocks(ch, name):
                m = g1 - g0
                row_lists = (lists[0], lists[1][g0 * R:g1 * R].contiguous(), lists[2][g0 * R:g1 * R].contiguous()) \
                    if index is not None else lists
                ent, val, _, _ = K.topk_rows(block, k, *row_lists, want_logp=False)      # [m * R, k] each
                cand = (val + off.view(-1, 1)).view(m, R * k)                           # J, fp32; empty slots -inf
                ent = ent.view(m, R * k).long()
                code = torch.where(ent >= 0, _event_slot_rels(R, k, dev) * N + ent, R * N)      # relation-major, entity ascending
                by_code = torch.sort(code, dim=1, stable=True)[1]
                best = torch.sort(cand.gather(1, by_code), dim=1, descending=True, stable=True)[1][:, :k]
                take = by_code.gather(1, best)                                          # [m, min(k, R * k)]
                j, e = cand.gather(1, take), ent.gather(1, take)
                ok = e >= 0
                here = torch.nonzero((gid >= g0) & (gid < g1)).view(-1)
                grp = gid[here] - g0
                o_rel, o_ent, o_logp, o_n = out[name]
                o_rel[ch.c + here] = torch.where(ok, torch.div(take, k, rounding_mode='floor'), -1).int()[grp]
                o_ent[ch.c + here] = e.int()[grp]
                o_logp[ch.c + here] = torch.where(ok, j, -np.inf)[grp]
                o_n[ch.c + here] = ok.sum(dim=1).int()[grp]
    return out


def _event_slot_rels(R, k, dev):
    """The relation of every slot of an [R * k] candidate row laid out relation-major."""
    return torch.arange(R, device=dev).repeat_interleave(k).view(1, R * k)


# =================================================================================================
# Open-query forecasts under the observed protocol: queries (s, r, o, t) that need not be facts of the stream -- a pair
# that did not occur at t, the timestamp after the stream's last, a side left open (-1) -- and histories AS OF an earlier
# timestamp (as_of <= t: the model forecasts t knowing only the facts before as_of; nothing is generated in between).  A
# gpu_builder.QueryStore gives such queries history windows on the resident tables (renet_query_histories); everything
# behind it is the observed pass above, run over the store's positions 0 .. n - 1.  As there, the queries are encoded in
# fixed chunks of gpu_builder.MAX_BOTH consecutive queries, each one merged batch graph, and a row inherits the reference's
# dependence on which other queries share its batch graph (utils.py:149-170); nothing of the multi-step state, and
# nothing resident of the base store, is written.
# =================================================================================================
def _query_store(obs, queries, as_of=None):
    """The gpu_builder.QueryStore of `queries` (int [n, 4] = (s, r, o, t), host array or device int32 tensor; -1: an absent
    side) on the resident stream obs, histories as of `as_of` (None: t; a scalar or [n]; as_of > t: ValueError)."""
    return _observed_store(obs).queries(queries, as_of)


def _forecast_rows(self, qs):
    """(feat_ob [n, 3H], feat_sub [n, 3H]) of every query of the QueryStore qs, in order (the chunks of _observed_chunks)."""
    idx = np.arange(qs.n_quads)
    (_, _, (feat_ob, feat_sub, _, _)), = _observed_cuts(_observed_chunks(self, qs, idx), len(idx))
    return feat_ob, feat_sub


def _forecast_scores(self, obs, queries, as_of=None, prior=None):
    """observed_scores for arbitrary queries: (sub_pred [n, N_ent], ob_pred [n, N_ent]), ob_pred[i] the logits of the
    objects of (s_i, r_i, ?, t_i) from the history of s_i before as_of, sub_pred[i] those of the subjects of (?, r_i, o_i,
    t_i).  For queries that are stream facts, forecast_scores(obs, obs.allq[idx]) is observed_scores(obs, idx) bit for bit.
    An absent side has an empty sequence, and the rows that would need it as the GIVEN entity are not computed: sub_pred is
    None when no query has an object (ob_pred: a subject); when only some lack it, their rows of that matrix are undefined.
    A batch whose histories are all empty takes the zero-state rows of _observed_features without an encoder launch.
    prior: a recurrence.RecurrencePrior -- the matrices are then the mixed log-probabilities (recurrence.py), the prior cut
    at the same as_of as the histories."""
    qs = _query_store(obs, queries, as_of)
    has_s, has_o = qs.sides_present()
    mix_rows = _prior_rows(prior, qs, np.arange(qs.n_quads))
    with torch.no_grad():
        feat_ob, feat_sub = _forecast_rows(self, qs)
        sub_pred = _linear_eval(self.linear, feat_sub) if has_o else None
        ob_pred = _linear_eval(self.linear, feat_ob) if has_s else None
        if mix_rows is not None:
            sub_pred = None if sub_pred is None else mix_rows.mix(prior, 'sub', sub_pred)
            ob_pred = None if ob_pred is None else mix_rows.mix(prior, 'ob', ob_pred)
        return sub_pred, ob_pred


def _forecast_topk(self, obs, queries, k=10, all_triplets=None, setting='raw', as_of=None, sides=('sub', 'ob'), prior=None):
    """predict_topk_observed for arbitrary queries, without gold: {side: (idx, score, logp, n_valid)} as device tensors for
    the sides asked for ('ob': the objects of (s, r, ?, t), 'sub': the subjects of (?, r, o, t)); a side left out costs no
    score GEMM.  setting / all_triplets as there (None: the base stream's facts, never the queries); the filter keys are the
    queries' own (s, r[, t]) / (o, r[, t]) -- a timestamp the facts do not hold gives empty time-aware lists.  With
    setting='raw' and queries that are a device tensor no query content is read back to the host.
    prior: a recurrence.RecurrencePrior -- the k best of the mixed distribution, score = logp = its log-probability."""
    if setting not in SETTINGS:
        raise ValueError('setting must be one of %s, not %r' % (', '.join(SETTINGS), setting))
    sides = tuple(sides)
    if not sides or any(name not in ('sub', 'ob') for name in sides):
        raise ValueError("sides must name 'sub', 'ob' or both")
    qs = _query_store(obs, queries, as_of)
    index = FI.filter_index_for(qs, all_triplets if all_triplets is not None else qs.facts) if setting != 'raw' else None
    out = {}
    with torch.no_grad():
        feat_ob, feat_sub = _forecast_rows(self, qs)
        dev = feat_ob.device
        # the score GEMMs are enqueued first: the host lookups of the filtered settings run while the device computes them
        preds = {name: _linear_eval(self.linear, feat) for name, feat in (('sub', feat_sub), ('ob', feat_ob)) if name in sides}
        if prior is not None:
            mix_rows = _prior_rows(prior, qs, np.arange(qs.n_quads))
            preds = {name: mix_rows.mix(prior, name, pred) for name, pred in preds.items()}
        for name, side, key_col in (('sub', 's', 2), ('ob', 'o', 0)):
            if name not in sides:
                continue
            lists = (None, None, None)
            if index is not None:
                tr = qs.quads
                key, r, t = tr[:, key_col], tr[:, 1], tr[:, 3]
                lists = index.ranges(side, np.stack((key, r, t) if setting == 'time_filtered' else (key, r), axis=1), dev)
            out[name] = K.topk_rows(preds[name], k, *lists, keep=None)
    return out


def _evaluate_forecast(self, obs, queries, as_of=None, all_triplets=None, max_batch=4096, relation=False, prior=None):
    """evaluate_observed for LABELLED queries (both sides present; the gold entities are the query's own s and o), with
    histories as of `as_of`: the same results in the same layout.  evaluate_forecast(obs, obs.allq[idx]) equals
    evaluate_observed(obs, idx) exactly; with as_of = obs.horizon_as_of(idx, h) it is the horizon-h stale-history evaluation
    (its numbers are not those of h = 1).  all_triplets None: the base stream's facts.  prior: as in evaluate_observed; its
    as_of is the one that cuts the histories -- a stale-history query gets a stale prior."""
    qs = _query_store(obs, queries, as_of)
    ents = qs.quads[:, [0, 2]]
    if ents.min() < 0 or ents.max() >= qs.num_ent:
        raise ValueError('evaluate_forecast takes labelled queries: both subject and object present')
    return _evaluate_observed(self, qs, np.arange(qs.n_quads), all_triplets if all_triplets is not None else qs.facts,
                              max_batch, relation, prior)


def _forecast_events(self, obs, ents, t, k=10, direction='ob', all_triplets=None, setting='raw', as_of=None, prior=None):
    """The k most probable events of the entities `ents` [n] at time(s) t (a scalar or [n]; it may lie past the stream's
    end): (rel int32 [n, k], ent int32 [n, k], logp [n, k], n_valid int32 [n]) as predict_events_observed gives per
    direction -- 'ob': the pairs (r, o) of ents as subjects, 'sub': the pairs (r, s) of ents as objects.  Runs
    predict_events_observed over a QueryStore whose relation column is 0 (history, RGCN rows and encoder_r's state do not
    depend on it) and whose other side is absent; the other direction is not computed.  prior: as in
    predict_events_observed; the as_of that cuts the histories cuts the prior -- a stale history gets a stale prior."""
    if direction not in ('ob', 'sub'):
        raise ValueError("direction must be 'ob' or 'sub'")
    if isinstance(ents, torch.Tensor) and ents.is_cuda:
        e = ents.to(torch.int32).reshape(-1)
        tt = torch.as_tensor(t).to(e.device).to(torch.int32).reshape(-1).expand(e.numel())
        none, zero = torch.full_like(e, -1), torch.zeros_like(e)
        quads = torch.stack((e, zero, none, tt) if direction == 'ob' else (none, zero, e, tt), dim=1).contiguous()
    else:
        e = np.asarray(ents.cpu() if isinstance(ents, torch.Tensor) else ents, dtype=np.int64).reshape(-1)
        tt = np.broadcast_to(np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, dtype=np.int64).reshape(-1), e.shape)
        none, zero = np.full_like(e, -1), np.zeros_like(e)
        quads = np.stack((e, zero, none, tt) if direction == 'ob' else (none, zero, e, tt), axis=1)
        if len(e) and e.min() < 0:
            raise ValueError('forecast_events: entity id outside [0, num_ent)')
    qs = _query_store(obs, quads, as_of)
    return _predict_events_observed(self, qs, np.arange(qs.n_quads), k, all_triplets if all_triplets is not None else qs.facts,
                                    setting, sides=(direction,), prior=prior)[direction]


# =================================================================================================
# Rollout horizon under the observed protocol (the reference's generate-in-between idea, model.py:222-328, on the resident
# stream): the truth is observed every h timestamps, and the steps in between see the model's own generated facts --
# ObservedStream.observe appends them to a chain that branches off the truth stream and is dropped after the block (the
# old store stays valid).  Three protocols, three sets of numbers: this one, the stale-history horizon
# (evaluate_forecast(as_of=horizon_as_of)) and the reference's multi-step state machine (evaluate_all_stream).
# =================================================================================================
def _generate_events_observed(self, obs, t, global_model, num_k=None, picks=None, block_floats=1 << 28):
    """The facts the model generates for timestamp t from the resident stream obs (everything the model knows: t must lie
    after its last timestamp, no as_of is taken): host int64 [m, 4], unique, sorted by (s, r, o), time column t, m <= 2 *
    num_k (default self.num_k; <= 1024).  Per direction -- 'ob': the picked entities as subjects, pairs (r, o); 'sub': as
    objects, pairs (r, s) -- prob = global_model.predict(t, obs.graph_dict, subject = direction is 'ob')[2]; the picked
    entities are picks(t, direction, prob) (an int array / tensor of draws, repeats counting) or self.sample_entities(prob);
    their joint blocks at t are forecast_events' (a QueryStore with relation column 0 and the other side absent: one encoder
    chunk, one merged batch graph), taken in sub-blocks of at most block_floats floats over ASCENDING entities; per sub-block
    renet_topk_rows gives every row's min(num_k, 1024) best (setting raw) and renet_select_events folds them into the
    direction's winners: the num_k best continuations by V = (score + row offset) + log prob[entity], an entity drawn m
    times counting m times (model.py:229-258), ties by (entity, relation, other entity) ascending.  Nothing is read back
    inside the loops; ONE device-to-host copy brings both directions' winners, and their union is taken on the host (observe()
    builds the facts' TimeGraph there anyway).  self.last_generate = {direction: {'entities', 'blocks', 'winners'}}."""
    store = _observed_store(obs)
    stream = getattr(store, 'obs', None)
    if stream is None or not hasattr(stream, 'graph_dict'):
        raise ValueError('generate_events_observed needs the resident ObservedStream (its graph_dict feeds the global model)')
    t = int(t)
    if len(stream.times) and t <= int(stream.times[-1]):
        raise ValueError('generate_events_observed: t = %d does not lie after the stream\'s last timestamp %d'
                         % (t, int(stream.times[-1])))
    num_k = int(self.num_k if num_k is None else num_k)
    R, dev = self.num_rels, self.ent_embeds.device
    if not 1 <= num_k <= K.SELECT_EVENTS_MAX:
        raise ValueError('generate_events_observed: num_k must lie in [1, %d]' % K.SELECT_EVENTS_MAX)
    if R > K.SELECT_EVENTS_MAX:
        raise ValueError('generate_events_observed takes at most %d relations' % K.SELECT_EVENTS_MAX)
    per = _event_groups_per_block(self, block_floats)
    sels, stats = {}, {}
    with torch.no_grad():
        q_rel = _event_q_rel(self)
        for name in ('ob', 'sub'):
            prob = global_model.predict(t, stream.graph_dict, subject=name == 'ob')[2]
            drawn = picks(t, name, prob) if picks is not None else self.sample_entities(prob)
            drawn = np.asarray(drawn.cpu() if isinstance(drawn, torch.Tensor) else drawn, dtype=np.int64).reshape(-1)
            ents, mult = np.unique(drawn, return_counts=True)
            if len(ents) == 0 or ents[0] < 0 or ents[-1] >= self.in_dim or len(ents) > K.SELECT_EVENTS_MAX:
                raise ValueError('generate_events_observed: picks must give 1 .. %d distinct entities of [0, num_ent)'
                                 % K.SELECT_EVENTS_MAX)
            none, zero = np.full_like(ents, -1), np.zeros_like(ents)
            quads = np.stack((ents, zero, none, np.full_like(ents, t)) if name == 'ob' else
                             (none, zero, ents, np.full_like(ents, t)), axis=1)
            qs = _query_store(store, quads)
            lprior = torch.log(prob[G.h2d(ents, dev)])
            mult_dev = G.h2d(mult.astype(np.int32), dev)
            sel = sels[name] = ops.EventSelection(num_k, dev)
            n_blocks = 0
            ch, = _event_chunks(self, qs, np.arange(qs.n_quads))                           # <= 1024 queries: one chunk
            d = ch.dirs[name]
            by_ent = np.argsort(d.ent, kind='stable')                                      # group indices, entity ascending
            assert np.array_equal(d.ent[by_ent], ents)
            for a in range(0, len(ents), per):
                groups = np.sort(by_ent[a:a + per])                                        # ascending group index: lengths descend
                block, off = _event_block(self, ch, name, q_rel[name], groups)
                idx, val, _, _ = K.topk_rows(block, min(num_k, 1024), want_logp=False)     # [m * R, k] each
                # the block's rows back into ascending entity order
                back = np.argsort(d.ent[groups], kind='stable')
                rows = G.h2d((back[:, None] * R + np.arange(R)[None, :]).reshape(-1), dev)
                sel.add(idx[rows].contiguous(), val[rows].contiguous(), off[rows].contiguous(),
                        G.h2d(ents[a:a + per].astype(np.int32), dev), lprior[a:a + per].contiguous(),
                        mult_dev[a:a + per].contiguous())
                n_blocks += 1
            stats[name] = {'entities': int(len(ents)), 'blocks': n_blocks}
    won = ops.EventSelection.results([sels['ob'], sels['sub']])
    facts = []
    for name, (given, rel, other, _, _) in zip(('ob', 'sub'), won):
        stats[name]['winners'] = int(len(given))
        facts.append(np.stack((given, rel, other) if name == 'ob' else (other, rel, given), axis=1).astype(np.int64))
    facts = np.unique(np.concatenate(facts), axis=0)
    self.last_generate = stats
    return np.concatenate((facts, np.full((len(facts), 1), t, dtype=np.int64)), axis=1)


def _evaluate_rollout(self, obs, quads, h, global_model, all_triplets=None, max_batch=4096, picks=None,
                      block_floats=1 << 28):
    """evaluate_forecast of the labelled, time-sorted quads under the ROLLOUT horizon h >= 1: the timestamps of quads are cut
    into blocks of h consecutive ones (horizon_as_of's rule); inside a block the first timestamp is forecast from the truth
    stream -- obs (resident, ending before quads[0, 3]) plus the true facts of the earlier blocks -- and every later one from
    that stream plus the facts generate_events_observed gave for the block's timestamps before it, appended with
    ObservedStream.observe; after the block its true facts are observed and the generated chain is dropped.  h = 1 is the
    forecast / observe loop.  all_triplets: what the filtered settings filter by (None: obs.allq and quads together);
    generated facts never enter a filter, and the filter index is built once and handed from store to store.  picks: as in
    generate_events_observed.  -> (ranks, loss) in evaluate_forecast's layout, in quads order; self.last_rollout lists, per
    generated timestamp, {'t', 'generated', 'true'}: the facts generated and how many of them are true facts of t."""
    h = int(h)
    if h < 1:
        raise ValueError('horizon must be >= 1')
    store = _observed_store(obs)
    truth = getattr(store, 'obs', None)
    if truth is None or not hasattr(truth, 'observe'):
        raise ValueError('evaluate_rollout needs the resident ObservedStream')
    quads = np.asarray(quads.cpu() if isinstance(quads, torch.Tensor) else quads, dtype=np.int64).reshape(-1, 4)
    if len(quads) == 0 or np.any(np.diff(quads[:, 3]) < 0):
        raise ValueError('evaluate_rollout takes labelled quadruples sorted by time')
    if len(truth.times) and int(truth.times[-1]) >= quads[0, 3]:
        raise ValueError('evaluate_rollout: the stream must end before the first evaluated timestamp')
    known = all_triplets if all_triplets is not None else np.concatenate((truth.allq, quads))

    def observed(stream, facts):
        index = getattr(stream.device, '_filter_index', None)
        new = stream.observe(facts, global_model)
        new.device._filter_index = index                                                   # (the index of `known`)
        return new

    times, first = np.unique(quads[:, 3], return_index=True)
    ends = list(first[1:]) + [len(quads)]
    ranks, loss, log = {}, [], []
    for b0 in range(0, len(times), h):
        b1 = min(b0 + h, len(times))
        cur = truth
        for j in range(b0, b1):
            q = quads[first[j]:ends[j]]
            r, l = _evaluate_forecast(self, cur, q, all_triplets=known, max_batch=max_batch)
            for name, v in r.items():
                ranks.setdefault(name, []).append(v)
            loss.append(l)
            if j + 1 < b1:
                gen = _generate_events_observed(self, cur, int(times[j]), global_model, picks=picks, block_floats=block_floats)
                true = {tuple(x) for x in q[:, :3].tolist()}
                log.append({'t': int(times[j]), 'generated': int(len(gen)),
                            'true': int(sum(tuple(x) in true for x in gen[:, :3].tolist()))})
                if len(gen):
                    cur = observed(cur, gen)
        if b1 < len(times):                                                                # (the chain `cur` is dropped here)
            truth = observed(truth, quads[first[b0]:ends[b1 - 1]])
    self.last_rollout = log
    return {name: np.concatenate(v) for name, v in ranks.items()}, np.concatenate(loss)


RENet.generate_events_observed = _moded(_generate_events_observed)
RENet.evaluate_rollout = _moded(_evaluate_rollout)
RENet.forecast_scores = _moded(_forecast_scores)
RENet.forecast_topk = _moded(_forecast_topk)
RENet.evaluate_forecast = _moded(_evaluate_forecast)
RENet.forecast_events = _moded(_forecast_events)
RENet.observed_event_scores = _moded(_observed_event_scores)
RENet.evaluate_events_observed = _moded(_evaluate_events_observed)
RENet.predict_events_observed = _moded(_predict_events_observed)
RENet.observed_scores = _moded(_observed_scores)
RENet.evaluate_observed = _moded(_evaluate_observed)
RENet.predict_topk_observed = _moded(_predict_topk_observed)
RENet.init_history = _init_history
RENet.update_cache = _update_cache
RENet.pred_r_rank2 = _moded(_pred_r_rank2)
RENet.sample_entities = _sample
RENet._joint_topk_many = _moded(_joint_topk_many)
RENet._advance_side = _advance_side
RENet._apply_winners = _apply_winners
RENet._winners_pruned = _moded(_winners_pruned)
RENet._roll_histories = _roll_histories
RENet._touched_sets = _touched_sets
RENet._cached_facts = _cached_facts
RENet._advance_time = _moded(_advance_time)
RENet.predict = _moded(_predict)
RENet.evaluate = _moded(_evaluate)
RENet.evaluate_filter = _moded(_evaluate_filter)
RENet._lookahead_filter = _lookahead_filter
RENet.predict_batch = _moded(_predict_batch)
RENet.evaluate_filter_batch = _moded(_evaluate_filter_batch)
RENet.evaluate_filter_stream = _moded(_evaluate_filter_stream)
RENet.evaluate_batch = _moded(_evaluate_batch)
RENet.evaluate_stream = _moded(_evaluate_stream)
RENet.evaluate_time_filter = _moded(_evaluate_time_filter)
RENet.evaluate_all_batch = _moded(_evaluate_all_batch)
RENet.evaluate_all_stream = _moded(_evaluate_all_stream)
RENet.predict_topk_batch = _moded(_predict_topk_batch)
RENet.predict_topk_stream = _moded(_predict_topk_stream)

import online  # noqa: E402,F401  (binds RENet.learn_observed / RENet.evaluate_online: the online-learning protocol)
