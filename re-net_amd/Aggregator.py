"""Neighbourhood aggregators with the reference's class names and call signatures
(reference Aggregator.py:9-237), rebuilt on the DGL-free batch builder (graph.py) and the HIP
kernels.  MeanAggregator / AttnAggregator (Aggregator.py:239-361; the paper's ablation encoders -- model.py:36 always
builds RGCNAggregator, and so does RENet here) need no graph: their neighbour id lists go through graph.NeighbourBatch
and the fused pooling kernels (csrc/nbr_pool.hip).

What differs from the reference internally (results are the same):
  * the batch graph is built by a few vectorised numpy passes instead of ~T_b DGL subgraph calls;
  * the per-sequence `# Slow!!!` scatter loop (Aggregator.py:148-155) and pack_padded_sequence are
    one kernel that writes the PackedSequence data directly (time-major), dropout fused;
  * the length sort is computed once (stable) and shared with the caller through `last_batch`.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import PackedSequence

import graph as G
import ops
from RGCN import RGCNBlockLayer as RGCNLayer


def _host_ints(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().astype(np.int64).reshape(-1)
    return np.asarray(x, dtype=np.int64).reshape(-1)


class GlobalEmbTable(object):
    """Device matrix view of the `global_emb` dict (t -> tensor[1,1,D], train.py:64-66): rows in
    ascending time + a searchsorted index.  Rebuilt when the dict's size changes or on invalidate()."""

    def __init__(self):
        self._key = None
        self.times = None
        self.mat = None

    def _signature(self, global_emb):
        return (id(global_emb), len(global_emb), tuple(id(v) for v in global_emb.values()))

    def get(self, global_emb, dim, device):
        key = (self._signature(global_emb), str(device))
        if key != self._key:
            ts = sorted(int(t) for t in global_emb.keys())
            self.times = np.asarray(ts, dtype=np.int64)
            if ts:
                # one stack per source device and ONE transfer (a .cpu() per row was a device sync per timestamp:
                # thousands per rebuild at GDELT scale, and the table is rebuilt at every new test timestamp)
                rows = [torch.as_tensor(global_emb[t]).detach().reshape(dim).float() for t in ts]
                devs = {r.device for r in rows}
                if len(devs) == 1:
                    self.mat = torch.stack(rows).to(device)
                else:
                    self.mat = torch.stack([r.to(device) for r in rows])
            else:
                self.mat = torch.zeros(1, dim, device=device)
            self._key = key
            # strong references: the signature is made of object identities, which a freed dict / tensor would
            # hand on to its successor
            self._alive = (global_emb, list(global_emb.values()))
        return self

    def invalidate(self):
        self._key = None
        self._host_key = None
        self._alive = None

    def get_host(self, global_emb):
        """Host-only view (sorted timestamps for `index`); no device access."""
        key = (id(global_emb), len(global_emb))
        if key != getattr(self, '_host_key', None):
            self.times = np.asarray(sorted(int(t) for t in global_emb.keys()), dtype=np.int64)
            self._host_key = key
            self._host_alive = global_emb
        return self

    def index(self, t):
        t = np.asarray(t, dtype=np.int64)
        p = np.searchsorted(self.times, t)
        if len(t) and (np.any(p >= len(self.times)) or np.any(self.times[np.minimum(p, len(self.times) - 1)] != t)):
            raise KeyError('timestamp without a global embedding')
        return p


class RGCNAggregator(nn.Module):
    def __init__(self, h_dim, dropout, num_nodes, num_rels, num_bases, model, seq_len=10):
        super().__init__()
        self.h_dim = h_dim
        self.drop_p = float(dropout or 0.0)
        self.dropout = nn.Dropout(dropout)       # kept for attribute compatibility; the mask is fused
        self.seq_len = seq_len
        self.num_rels = num_rels
        self.num_nodes = num_nodes
        self.model = model
        self.rgcn1 = RGCNLayer(h_dim, h_dim, 2 * num_rels, num_bases, activation=F.relu, self_loop=True,
                               dropout=dropout)
        self.rgcn2 = RGCNLayer(h_dim, h_dim, 2 * num_rels, num_bases, activation=None, self_loop=True,
                               dropout=dropout)
        self.glob_table = GlobalEmbTable()
        self.last_batch = None
        # forward_grouped builds its batch on the device (gpu_builder.GroupedDeviceBatch: the same arrays, bit for bit)
        # instead of graph.build_batch + the upload of graph.DeviceGraph; opt-in: RENET_GROUPED_DEVICE_BUILDER=1
        self.grouped_device_builder = os.environ.get('RENET_GROUPED_DEVICE_BUILDER', '0') == '1'

    # ------------------------------------------------------------------------------------------
    def build(self, s_hist, s, r, ent_embeds, graph_dict, global_emb, sort, group=None):
        """Host side of utils.py:209-283: returns the device batch graph (or None if every history
        is empty)."""
        s_np, r_np = _host_ints(s), _host_ints(r)
        fh = s_hist if isinstance(s_hist, G.FlatHistory) else G.FlatHistory.from_lists(s_hist[0], s_hist[1])
        if fh.seq_ptr[-1] == 0:
            return None
        table = self.glob_table.get(global_emb, self.h_dim, ent_embeds.device)
        hb = G.build_batch(G.store_for(graph_dict), self.num_nodes, self.num_rels, s_np, r_np, fh, sort=sort,
                           glob_index=table.index, group=group)
        if hb.L > self.seq_len:
            raise ValueError('history longer than seq_len (%d > %d)' % (hb.L, self.seq_len))
        g = G.DeviceGraph(hb, ent_embeds.device)
        g.glob = table.mat
        return g

    def build_grouped_device(self, fh, s, r, ent_embeds, graph_dict, global_emb, group):
        """build(..., sort=True, group=group) on the DEVICE builder, or None where that front does not apply (the caller then
        takes the host builder): tensors that are not on a HIP device, a batch beyond its limits, no history at all."""
        import gpu_builder
        if not ent_embeds.is_cuda or not 0 < len(fh) <= gpu_builder.MAX_GROUPED or fh.seq_ptr[-1] == 0 or \
                self.seq_len > gpu_builder.MAXL or 2 * self.num_rels > 1024:
            return None
        table = self.glob_table.get(global_emb, self.h_dim, ent_embeds.device)
        base = gpu_builder.graph_store_for(graph_dict, global_emb, self.num_nodes, self.num_rels, ent_embeds.device)
        for _ in range(16):                                 # (a capacity grew: rebuild; first batches only)
            if len(fh.step_t) + len(fh.nbr_o) >= 2 ** 30 or base.cap_nodes * 2 * self.num_rels >= 2 ** 31:
                return None                                 # (beyond the front's 32-bit sort keys: RENET_ERR_UNSUPPORTED)
            g = gpu_builder.GroupedDeviceBatch(gpu_builder.GroupedBatchStore(base, s, r, group, fh), self.seq_len)
            if g.finalize():
                g.glob = table.mat
                return g
        raise RuntimeError('device batch builder did not converge on its capacities')

    def encode(self, g, ent_embeds, rel_embeds, reverse, _lazy_bf16=False):
        """Device side: h0 gather, two RGCN layers, packed sequence assembly (Aggregator.py:136-165).
        _lazy_bf16 (PRIVATE: internal callers that hand X / Xr straight to ops.dual_gru / MultiGRUFn): in bf16-storage mode the
        GRU inputs are produced as bf16 operand matrices only (ops.SeqAssembleFn)."""
        g.ndata['h'] = ops.TableRows(ent_embeds, g.node_ent, g.plan_node_ent)               # utils.py:239, deferred
        self.rgcn1(g, reverse)
        g.out_rows = g.nA               # only the subject rows of layer 2 are ever read (Aggregator.py:139-140)
        self.rgcn2(g, reverse)
        g.out_rows = None
        h2 = g.ndata.pop('h')           # [nA, D]; subj_row < nA by construction
        p = self.drop_p if self.training else 0.0
        sx, sxr = (ops.next_seed(), ops.next_seed()) if p > 0 else (0, 0)
        return ops.SeqAssembleFn.apply(h2, ent_embeds, rel_embeds, g.glob, g, p, sx, sxr, bool(_lazy_bf16))

    def _run(self, s_hist, s, r, ent_embeds, rel_embeds, graph_dict, global_emb, reverse, sort, group=None):
        g = None
        if group is not None and sort and self.grouped_device_builder:
            s_hist = s_hist if isinstance(s_hist, G.FlatHistory) else G.FlatHistory.from_lists(s_hist[0], s_hist[1])
            g = self.build_grouped_device(s_hist, _host_ints(s), _host_ints(r), ent_embeds, graph_dict, global_emb,
                                          _host_ints(group))
        if g is None:
            g = self.build(s_hist, s, r, ent_embeds, graph_dict, global_emb, sort, group)
        self.last_batch = g
        if g is None:
            return None, None
        x, xr = self.encode(g, ent_embeds, rel_embeds, reverse)
        bs = torch.from_numpy(g.host.batch_sizes)
        return PackedSequence(x, bs), PackedSequence(xr, bs)

    def forward(self, s_hist, s, r, ent_embeds, rel_embeds, graph_dict, global_emb, reverse):
        """Aggregator.py:124-167.  Returns (PackedSequence[., 4h], PackedSequence[., 3h]) for the
        length-sorted non-empty sequences, or (None, None) when every history is empty."""
        return self._run(s_hist, s, r, ent_embeds, rel_embeds, graph_dict, global_emb, reverse, True)

    def forward_grouped(self, s_hist, s, r, ent_embeds, rel_embeds, graph_dict, global_emb, reverse, group):
        """Extension (not in the reference): forward() with SEPARATE member graphs for sequences of different
        `group` ids (graph.build_batch), i.e. the batch equals one reference call per group -- used to batch the
        reference's per-quadruple inference."""
        return self._run(s_hist, s, r, ent_embeds, rel_embeds, graph_dict, global_emb, reverse, True, group)

    def predict_batch(self, s_hist, s, r, ent_embeds, rel_embeds, graph_dict, global_emb, reverse):
        """Aggregator.py:169-214: same, sequences kept in the given order."""
        return self._run(s_hist, s, r, ent_embeds, rel_embeds, graph_dict, global_emb, reverse, False)

    def predict(self, s_history, s, r, ent_embeds, rel_embeds, graph_dict, global_emb, reverse):
        """Aggregator.py:218-237: one sequence -> (inp[len, 4h], inp_r[len, 3h])."""
        hist, hist_t = s_history
        px, pxr = self._run(([hist], [hist_t]), _host_ints(s)[:1], _host_ints(r)[:1], ent_embeds, rel_embeds,
                            graph_dict, global_emb, reverse, False)
        return px.data, pxr.data


class RGCNAggregator_global(nn.Module):
    def __init__(self, h_dim, dropout, num_nodes, num_rels, num_bases, model, seq_len=10, maxpool=1):
        super().__init__()
        self.h_dim = h_dim
        self.drop_p = float(dropout or 0.0)
        self.dropout = nn.Dropout(dropout)
        self.seq_len = seq_len
        self.num_rels = num_rels
        self.num_nodes = num_nodes
        self.model = model
        self.maxpool = maxpool
        self.rgcn1 = RGCNLayer(h_dim, h_dim, 2 * num_rels, num_bases, activation=F.relu, self_loop=True,
                               dropout=dropout)
        self.rgcn2 = RGCNLayer(h_dim, h_dim, 2 * num_rels, num_bases, activation=None, self_loop=True,
                               dropout=dropout)
        # build the full-graph batch on the device (gpu_builder.FullGraphBatch)?  None = follow RENET_GLOBAL_DEVICE_BUILDER
        # (default off); True / False = this model's own choice
        self.device_builder = None

    def _full_graphs(self, times, ent_embeds, graph_dict):
        """The batch graph of the full graphs of `times`: from the device builder when it is switched on and the model is on a
        GPU -- the same arrays, bit for bit -- else from the host builder.  The device builder takes 1 .. 1024 member graphs
        per batch; anything else stays with the host builder."""
        on = self.device_builder
        if on is None:
            on = os.environ.get('RENET_GLOBAL_DEVICE_BUILDER', '0') == '1'
        if on and ent_embeds.is_cuda:
            import gpu_builder
            if 0 < len(times) <= gpu_builder.MAX_FULL_GRAPHS:
                fs = gpu_builder.full_graph_store_for(graph_dict, self.num_rels, ent_embeds.device)
                g = gpu_builder.FullGraphBatch(fs, fs.store.index_of(np.asarray(times, dtype=np.int64)))
                g.finalize()
                return g
        return G.DeviceGraph(G.build_full_graphs(graph_dict, times), ent_embeds.device)

    def pooled(self, times, ent_embeds, graph_dict, reverse):
        """Batch the FULL graphs of `times`, two RGCN layers, per-graph max/mean readout
        (Aggregator.py:44-61 / 87-105) -> [len(times), h]."""
        g = self._full_graphs(times, ent_embeds, graph_dict)
        g.ndata['h'] = ops.TableRows(ent_embeds, g.node_ent, g.plan_node_ent)               # deferred gather
        self.rgcn1(g, reverse)
        self.rgcn2(g, reverse)
        h2 = g.ndata.pop('h')
        return ops.SegmentPoolFn.apply(h2, g.seg_ptr, g.G, 1 if self.maxpool == 1 else 0)

    def forward(self, t_list, ent_embeds, graph_dict, reverse):
        """Aggregator.py:27-73.  t_list: timestamps sorted descending (global_model.py:45); zeros (no
        history) are dropped.  Returns the PackedSequence of pooled graph embeddings [., h]."""
        times = np.asarray(list(graph_dict.keys()), dtype=np.int64)
        time_unit = int(times[1] - times[0])
        t_np = _host_ints(t_list)
        t_np = t_np[:int(np.count_nonzero(t_np))]
        length = t_np // time_unit
        lens = np.minimum(length, self.seq_len)
        starts = length - lens
        win = G.ragged_arange(starts, lens)                      # positions in the timeline, sequence-major
        uniq_pos, inv = np.unique(win, return_inverse=True)
        pooled = self.pooled(times[uniq_pos], ent_embeds, graph_dict, reverse)
        n = len(lens)
        L = int(lens[0]) if n else 0
        bs = (lens[None, :] > np.arange(L)[:, None]).sum(axis=1) if L else np.zeros(0, np.int64)
        off = np.concatenate(([0], np.cumsum(bs)))
        seq = np.repeat(np.arange(n), lens)
        j = np.arange(len(win)) - np.repeat(np.cumsum(lens) - lens, lens)
        packed_of_k = off[j] + seq
        rows = np.empty(len(win), dtype=np.int64)
        rows[packed_of_k] = inv
        plan = G.SegPlan.host(rows)
        dev = ent_embeds.device
        for f in ('order', 'seg_ptr', 'target'):
            setattr(plan, f, torch.from_numpy(getattr(plan, f)).to(dev))
        idx = torch.from_numpy(rows.astype(np.int32)).to(dev)
        x = ops.GatherRowsFn.apply(pooled, idx, plan)            # Aggregator.py:64-67
        if self.training and self.drop_p > 0:
            x = ops.DropoutFn.apply(x, self.drop_p, ops.next_seed())      # Aggregator.py:69
        return PackedSequence(x, torch.from_numpy(bs.astype(np.int64)))

    def predict(self, t, ent_embeds, graph_dict, reverse):
        """Aggregator.py:75-107: pooled embeddings of the <= seq_len graphs strictly before t."""
        times = list(graph_dict.keys())
        pos = 0
        for tt in times:
            if tt >= t:
                break
            pos += 1
        win = times[max(0, pos - self.seq_len):pos]
        return self.pooled(win, ent_embeds, graph_dict, reverse)


class _NeighbourAggregator(nn.Module):
    """What MeanAggregator and AttnAggregator share: the host batch of the neighbour id lists, the packed result with
    its dropout (Aggregator.py:281 / 342: the reference drops on the padded tensor before packing -- elementwise the same
    distribution), and predict() as a one-sequence batch."""

    def __init__(self, h_dim, dropout, seq_len):
        super().__init__()
        self.h_dim = h_dim
        self.drop_p = float(dropout or 0.0)
        self.dropout = nn.Dropout(dropout)       # kept for attribute compatibility; the mask is ops.DropoutFn's
        self.seq_len = seq_len
        self.last_batch = None

    def build(self, s_hist, s, r, ent_embeds, seq_len):
        """-> graph.DeviceNeighbourBatch, or None when every history is empty."""
        hb = G.NeighbourBatch(_host_ints(s), _host_ints(r), s_hist, seq_len=seq_len)
        return hb.to(ent_embeds.device) if hb.nseq else None

    def pooled(self, nb, ent_embeds, rel_embeds):
        raise NotImplementedError

    def forward(self, s_hist, s, r, ent_embeds, rel_embeds):
        """-> PackedSequence of the length-sorted non-empty sequences (`last_batch.host.perm` is the order), or None when
        every history is empty."""
        nb = self.last_batch = self.build(s_hist, s, r, ent_embeds, self.seq_len)
        if nb is None:
            return None
        x = self.pooled(nb, ent_embeds, rel_embeds)
        if self.training and self.drop_p > 0:
            x = ops.DropoutFn.apply(x, self.drop_p, ops.next_seed())
        return PackedSequence(x, torch.from_numpy(nb.host.batch_sizes.astype(np.int64)))

    def predict(self, s_history, s, r, ent_embeds, rel_embeds):
        """One sequence: s_history = list of 1-D id arrays -> one row per time step (no dropout, no length limit)."""
        if len(s_history) == 0:
            return self._empty(ent_embeds)
        nb = self.build([list(s_history)], _host_ints(s)[:1], _host_ints(r)[:1], ent_embeds, None)
        return self.pooled(nb, ent_embeds, rel_embeds)


class MeanAggregator(_NeighbourAggregator):
    """Aggregator.py:239-297: packed rows [ mean_j ent[nbr_j] | ent[s] ] (gcn=True: relu(gcn_layer(mean)) first)."""

    def __init__(self, h_dim, dropout, seq_len=10, gcn=False):
        super().__init__(h_dim, dropout, seq_len)
        self.gcn = gcn
        if gcn:
            self.gcn_layer = nn.Linear(h_dim, h_dim)

    def _empty(self, ent_embeds):
        return ent_embeds.new_zeros(0, 2 * self.h_dim)

    def pooled(self, nb, ent_embeds, rel_embeds):
        x = ops.NbrPoolFn.apply(ent_embeds, None, None, None, None, nb)
        if self.gcn:                                                              # Aggregator.py:269-271
            h = self.h_dim
            m = F.relu(ops.LinearFn.apply(x[:, :h], self.gcn_layer.weight, self.gcn_layer.bias))
            x = torch.cat((m, x[:, h:]), dim=1)
        return x


class AttnAggregator(_NeighbourAggregator):
    """Aggregator.py:306-361: packed rows [ sum_j w_j ent[nbr_j] | ent[s] | rel[r] ] with
    w = softmax_j( tanh(attn_s([ent[nbr_j] | ent[s] | rel[r]])) @ v_s )."""

    def __init__(self, h_dim, dropout, seq_len=10):
        super().__init__(h_dim, dropout, seq_len)
        self.attn_s = nn.Linear(3 * h_dim, h_dim)
        self.v_s = nn.Parameter(torch.Tensor(h_dim, 1))
        nn.init.xavier_uniform_(self.v_s, gain=nn.init.calculate_gain('relu'))

    def _empty(self, ent_embeds):
        return ent_embeds.new_zeros(0, 3 * self.h_dim)

    def pooled(self, nb, ent_embeds, rel_embeds):
        p, q = ops.NbrAttnProjFn.apply(ent_embeds, rel_embeds, self.attn_s.weight, self.attn_s.bias, nb)
        return ops.NbrPoolFn.apply(ent_embeds, rel_embeds, p, q, self.v_s, nb)
