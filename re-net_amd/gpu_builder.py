"""Device-side batch-graph builder for the merged training batch (csrc/builder_both.hip, renet_build_batch_both).

The host builder (graph.build_batch_both: numpy front + the native passes of csrc/host_builder.cpp) costs ~13 ms per
merged batch against a ~3.6 ms device step.  Here the dataset is resident in HBM -- the quadruples, the per-role
history index of preprocess.HistoryIndex and the per-timestamp fact lists of graph.GraphStore (`DeviceStore`) -- and a
batch is built from its B quadruple indices by kernels: 4 KB up, ~100 bytes of counts back, no synchronisation in
between.  `DeviceBatch` then carries the attributes of graph.BatchGraph, as graph.DeviceGraph does (the arrays are
bit-identical to the host builder's: tests/test_gpu_builder.py), so model.RENet.loss_prepared_both runs on it unchanged.
Replaces, for that case, utils.py:209-244 + 115-131 + dgl.batch of the reference.

The global model's full-graph batches (graph.build_full_graphs; Aggregator.py:44-55 / 87-98) are built the same way:
`FullGraphStore` keeps the per-timestamp node lists and local fact endpoints resident, `FullGraphBatch` is the union of the
full graphs of a list of timestamps (csrc/builder_full.hip: renet_build_full_graphs, the same tail kernels behind a three-kernel
front), again bit-identical to the host builder (tests/test_gpu_full_graph_builder.py).

Grouped inference batches (graph.build_batch(group=...), RGCNAggregator.forward_grouped) are the third front:
`GroupedBatchStore` uploads one call's s / r / group / FlatHistory, `GroupedDeviceBatch` is the batch of ONE direction with
a member graph per (group, timestamp) (renet_build_batch_grouped), bit-identical again (tests/test_gpu_grouped_builder.py).

Open queries of the observed pass (`QueryStore`, made by ObservedStore.queries): a store whose positions are arbitrary
(s, r, o, t) queries with histories as of a timestamp <= t, the windows from one renet_query_histories launch
(csrc/builder_query.hip) on the resident tables; DeviceBatch runs on it as on the stream itself.

Layout of this file: the ctypes mirrors of the structs and count slots of include/renet_hip.h (tests/test_host_cpu.py holds
them to the header); `_Store`, the base of the resident stores, and the per-graph_dict cache `_cached_store`; `_launch`,
the one place that lays out, allocates and calls a builder front; `_PendingBatch`, the life cycle of a batch from the
launch to finalize(), of which `DeviceBatch`, `GroupedDeviceBatch` and `FullGraphBatch` are a front plus the fields each adds."""
import ctypes
import weakref

import numpy as np
import torch

import graph as G
import renet_hip as K

_P = ctypes.c_void_p
NCOUNTS = 64
(C_NNZ, C_S, C_L, C_TB, C_FACTS, C_N, C_NA, C_E2, C_E, C_NHEAVY, C_NHEAVY_OUT, C_NCHUNKS, C_NCHUNKS2, C_NITEMS,
 C_NGROUPS, C_NGROUPS_OUT, C_NSEG0, C_NSEG1, C_NSEG2, C_NSEG3, C_ERR, C_EOUT) = range(22)
C_STEP_OFF = 24
MAXL = 32


class _StoreDev(ctypes.Structure):
    _fields_ = [('q_s', _P), ('q_r', _P), ('q_o', _P), ('h_first', _P * 2), ('h_count', _P * 2), ('snap_t', _P * 2),
                ('snap_ptr', _P * 2), ('nbr_o', _P * 2), ('times', _P), ('trip_ptr', _P), ('trip_s', _P), ('trip_r', _P),
                ('trip_o', _P), ('glob_times', _P), ('T', ctypes.c_int), ('n_glob', ctypes.c_int),
                ('n_facts', ctypes.c_int), ('num_ent', ctypes.c_int), ('num_rels', ctypes.c_int)]


class _BatchOut(ctypes.Structure):
    _fields_ = [(n, _P) for n in ('node_ent', 'node_slot', 'row_ptr', 'col', 'etype', 'norm', 'heavy_rows', 'e_src', 'e_dst',
                                  'chunk_ptr', 'chunk_type', 'type_chunk_ptr', 'e_src2', 'e_dst2', 'chunk_ptr2',
                                  'chunk_type2', 'type_chunk_ptr2', 'it_src', 'it_type', 'grp_ptr', 'subj_row', 'row_seq',
                                  'row_ent', 'row_rel', 'glob_row', 's_sorted', 'r_sorted', 'rel_label', 'ent_label', 'perm',
                                  'step_off')] + \
               [('plan_order', _P * 4), ('plan_seg', _P * 4), ('plan_target', _P * 4), ('counts', _P),
                ('cap_nodes', ctypes.c_int), ('cap_edges', ctypes.c_int), ('seg_ptr', _P)]


class _FullStoreDev(ctypes.Structure):
    _fields_ = [('node_ptr', _P), ('node_ent_all', _P), ('trip_ptr', _P), ('trip_ls', _P), ('trip_r', _P), ('trip_lo', _P),
                ('T', ctypes.c_int), ('n_nodes', ctypes.c_int), ('n_facts', ctypes.c_int), ('num_ent', ctypes.c_int),
                ('num_rels', ctypes.c_int)]


class _GroupedStoreDev(ctypes.Structure):
    _fields_ = [(n, _P) for n in ('s', 'r', 'group', 'h_first', 'h_count', 'step_t', 'nbr_ptr', 'nbr_o', 'times', 'trip_ptr',
                                  'trip_s', 'trip_r', 'trip_o', 'glob_times', 'by_subj', 'subj_sorted')] + \
               [(n, ctypes.c_int) for n in ('n_steps', 'n_nbr', 'T', 'n_glob', 'n_facts', 'num_ent', 'num_rels')]


def _bind():
    return K.lib()          # renet_build_batch_workspace / renet_build_batch_both are bound with the rest of the C ABI


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _check_int32(what, *arrays, limit=2 ** 31):
    """ValueError('<what> must fit int32') unless every value of `arrays` lies in [0, limit)."""
    for a in arrays:
        if len(a) and (int(a.max()) >= limit or int(a.min()) < 0):
            raise ValueError(what + ' must fit int32')


class _Store(object):
    """What every resident store shares: its device, num_ent / num_rels and the pinned 256-byte count buffers.  Those are a
    free-list, not a ring -- every pending batch OWNS its buffer from the async D2H copy until finalize() has read it
    (with a shared ring of 8, the ninth pending batch overwrote the counts of the first)."""

    def __init__(self, device, num_ent, num_rels):
        self.device = device
        self.num_ent, self.num_rels = int(num_ent), int(num_rels)
        self._pinned_free = []

    def _take_pinned(self):
        if self._pinned_free:
            return self._pinned_free.pop()
        return torch.empty(NCOUNTS, dtype=torch.int32, pin_memory=True)

    def _give_pinned(self, buf):
        if buf is not None and len(self._pinned_free) < 64:
            self._pinned_free.append(buf)


class GraphDeviceStore(_Store):
    """The part of a DeviceStore that a batch does NOT bring itself: the per-timestamp fact lists of the graph store and the
    timestamps of the global-embedding table.  Used by the reference's LIST API (RENet.forward with nested history lists,
    train.py:136-137): there the quadruples and their histories arrive with every call (ListBatchStore uploads them, ~160 KB),
    so no dataset has to be registered with the model.  Cached per (graph store, global_emb timestamps) in graph_store_for()."""

    def __init__(self, graph_dict, global_emb, num_ent, num_rels, device):
        _Store.__init__(self, device, num_ent, num_rels)
        store = G.store_for(graph_dict)
        times = np.asarray(store.times, dtype=np.int64)
        if len(times) > 1 and np.any(np.diff(times) <= 0):
            raise ValueError('graph_dict must be in ascending time order')
        _check_int32('ids / timestamps', store.trip_s, store.trip_o, times)
        self.n_quads = 0
        self.t = dict(times=_i32(times, device), trip_ptr=_i32(store.trip_ptr, device), trip_s=_i32(store.trip_s, device),
                      trip_r=_i32(store.trip_r, device), trip_o=_i32(store.trip_o, device),
                      glob_times=_i32(sorted(int(t) for t in global_emb.keys()), device))
        self.n_facts = int(len(store.trip_s))
        self.T, self.n_glob = len(times), int(self.t['glob_times'].numel())
        # capacities: grown on demand (an overflow is reported in the counts and the batch rebuilt)
        self.cap_nodes, self.cap_edges = 1 << 17, 1 << 19
        self.c = None                         # (a ListBatchStore fills a struct per batch)
        self._store = store

    def subject_index(self):
        """Device (by_subj, subj_sorted) of graph.GraphStore.subject_index(), uploaded on first use: the grouped front walks
        the facts of a node through it."""
        if 'by_subj' not in self.t:
            by_subj, subj_sorted = self._store.subject_index()
            _check_int32('fact indices', by_subj)
            self.t.update(by_subj=_i32(by_subj, self.device), subj_sorted=_i32(subj_sorted, self.device))
        return self.t['by_subj'], self.t['subj_sorted']


class DeviceStore(GraphDeviceStore):
    """The dataset, resident on the device: quadruples, both history indices, the graph store, the sorted timestamps of
    the global-embedding table."""

    def __init__(self, quads, hist_s, hist_o, graph_dict, global_emb, num_ent, num_rels, device):
        GraphDeviceStore.__init__(self, graph_dict, global_emb, num_ent, num_rels, device)
        quads = np.asarray(quads, dtype=np.int64)
        _check_int32('ids / timestamps', quads)
        self.n_quads = len(quads)
        self.t.update(q_s=_i32(quads[:, 0], device), q_r=_i32(quads[:, 1], device), q_o=_i32(quads[:, 2], device))
        for r, h in enumerate((hist_s, hist_o)):
            self.t['h_first%d' % r] = _i32(h.first, device)
            self.t['h_count%d' % r] = _i32(h.count, device)
            self.t['snap_t%d' % r] = _i32(h.snap_t, device)
            self.t['snap_ptr%d' % r] = _i32(h.snap_ptr, device)
            self.t['nbr_o%d' % r] = _i32(h.nbr_o, device)
            self.t['ent_ptr%d' % r] = _i32(h.ent_ptr, device)          # (renet_query_histories: QueryStore below)
        self.history_len = int(hist_s.history_len)
        self._fill_struct()

    def _fill_struct(self):
        """`c`, the RenetStoreDev of the tensors in `t`."""
        sd = _StoreDev()
        for n in ('q_s', 'q_r', 'q_o', 'times', 'trip_ptr', 'trip_s', 'trip_r', 'trip_o', 'glob_times'):
            setattr(sd, n, self.t[n].data_ptr())
        for n in ('h_first', 'h_count', 'snap_t', 'snap_ptr', 'nbr_o'):
            setattr(sd, n, (_P * 2)(self.t[n + '0'].data_ptr(), self.t[n + '1'].data_ptr()))
        sd.T, sd.n_glob, sd.n_facts = self.T, self.n_glob, self.n_facts
        sd.num_ent, sd.num_rels = self.num_ent, self.num_rels
        self.c = sd


class ObservedStore(DeviceStore):
    """The DeviceStore of a whole preprocess.ObservedStream (train, valid and test as one stream: true histories and graphs
    at every timestamp) with the global-embedding table that belongs to it: `glob` [timestamps, D], rows in ascending time
    -- the order of the store's glob_times, which glob_row of a batch indexes.  The observed evaluation pass hands `glob`
    to RENet.finish_prepare_device; the model's own global_emb / glob_table are not involved.  `quads` is the host copy of
    the stream (labels and filter keys are read from it)."""

    def __init__(self, obs, global_emb, h_dim, device):
        DeviceStore.__init__(self, obs.allq, obs.hist_s, obs.hist_o, obs.graph_dict, global_emb, obs.num_ent, obs.num_rels,
                             device)
        self.obs, self.quads = obs, obs.allq
        ts = sorted(int(t) for t in global_emb.keys())
        self._glob_times = np.asarray(ts, dtype=np.int64)               # (host copy of t['glob_times']: appended() cuts by it)
        self.glob = torch.stack([torch.as_tensor(global_emb[t]).detach().reshape(h_dim).float() for t in ts]).to(device)
        self._pair = {}                                                 # pair_tables(), once asked for

    def pair_tables(self):
        """The resident PAIR TABLES of the recurrence prior: per role (0: subject runs, 1: object runs) the int32 device
        tensors (p_rel, p_other, p_t) of preprocess.PairIndex over this store's facts -- the same fact runs as the history
        index of the role (snap_ptr[ent_ptr]), sorted inside a run by (relation, partner, time).  Built on first use from the
        host quadruples, uploaded once and cached; a store that appended() makes from one that has them gets them from
        renet_pair_append instead.  The holder is shared by the stores that share this store's tables (refresh_global's
        copy, QueryStore)."""
        if 'tables' not in self._pair:
            import preprocess
            _check_int32('relations', self.quads[:, 1])
            tabs = []
            for role in (0, 1):
                pi = preprocess.PairIndex(self.quads, role, self.num_ent)
                tabs.append(tuple(_i32(a, self.device) for a in (pi.p_rel, pi.p_other, pi.p_t)))
            self._pair['tables'] = tuple(tabs)
        return self._pair['tables']

    def queries(self, quads, as_of=None, stream=None):
        """The QueryStore of the queries `quads` [n, 4] = (s, r, o, t) on top of this store: histories as of `as_of` (None:
        each query's own t), -1 for an absent subject or object."""
        return QueryStore(self, quads, as_of, stream)

    # the host GraphStore behind subject_index(): an appended store makes it when first asked
    _store = property(lambda self: self._graph_store(), lambda self, v: setattr(self, '_gstore', v))

    def _graph_store(self):
        if self._gstore is None:
            self._gstore = G.store_for(self.obs.graph_dict)
        return self._gstore

    def appended(self, quads, global_emb_new, _obs=None):
        """A NEW ObservedStore: this one with the newly observed quadruples `quads` (host int [m, 4], validated as
        ObservedStream.extended validates them: the same ValueErrors) appended ON THE DEVICE -- equal, tensor for tensor and
        bit for bit, to ObservedStore(obs.extended(quads), ...).  Per role one renet_store_append over the resident history
        index (csrc/builder_append.hip; host statement preprocess.HistoryIndex.appended), renet_append_i32 for the arrays an
        append only lengthens; uploaded: the new facts, sorted per role by (entity, time, input order) on the host (m is
        small), and the tails of times / trip_ptr.  All on the current stream, into fresh tensors: this store, and any batch
        still pending on it, stays valid.

        global_emb_new: {t: row} for EVERY timestamp of the longer stream >= the first appended one (ValueError otherwise;
        empty for m = 0) -- `glob` is this store's rows of the earlier timestamps followed by them.  cap_nodes / cap_edges
        are carried over; no filter index is; `obs` / `quads` are the light stream of ObservedStream._appended."""
        old = self.obs
        quads = old._checked_new(quads)
        obs = _obs if _obs is not None else old._appended(quads)
        m, nq, dev = len(quads), self.n_quads, self.device
        _check_int32('ids / timestamps', quads)
        if max(nq + m, obs.num_ent + 1) >= 2 ** 31 - 1024:
            raise ValueError('fact count must fit int32')
        t0 = int(quads[0, 3]) if m else None
        want = [int(t) for t in obs.times if t >= t0] if m else []
        if sorted(int(t) for t in global_emb_new.keys()) != want:
            raise ValueError('global_emb_new must hold exactly the timestamps of the longer stream from the first appended one on')
        # host side, over the new facts and the old stream's LAST timestamp only: per role the sorted new facts and the
        # snapshot count of the longer index (a new (entity, time) group joins an old snapshot only at the old last time)
        joined = m and len(old.allq) and t0 == int(old.allq[-1, 3])
        tail = old.allq[np.searchsorted(old.allq[:, 3], t0):] if joined else np.zeros((0, 4), np.int64)
        packs, caps = [], []
        for c, oc in ((0, 2), (2, 0)):
            order = np.lexsort((np.arange(m), quads[:, 3], quads[:, c]))
            packs.append(np.stack((quads[order, c], quads[order, 3], quads[order, oc], order)))
            groups = np.unique(quads[:, [c, 3]], axis=0) if m else np.zeros((0, 2), np.int64)
            n_join = int(np.isin(groups[groups[:, 1] == t0, 0], tail[:, c]).sum()) if joined else 0
            caps.append(int(self.t['snap_t%d' % (c // 2)].numel()) + len(groups) - n_join)
        new_t = np.unique(quads[:, 3])
        if joined:
            new_t = new_t[1:]
        ends = self.n_facts + np.searchsorted(quads[:, 3], np.unique(quads[:, 3]), side='right')
        flat = np.concatenate([a.reshape(-1) for a in packs] + [quads[:, 0], quads[:, 1], quads[:, 2], new_t, ends,
                               np.asarray(want, dtype=np.int64)])
        up = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.int32)).to(dev, non_blocking=True)     # ONE upload
        role = [up[k * 4 * m:(k + 1) * 4 * m].view(4, m) for k in (0, 1)]
        o = 8 * m
        n_s, n_r, n_o = up[o:o + m], up[o + m:o + 2 * m], up[o + 2 * m:o + 3 * m]
        o += 3 * m
        n_times, n_ends = up[o:o + len(new_t)], up[o + len(new_t):o + len(new_t) + len(ends)]
        n_glob_t = up[o + len(new_t) + len(ends):]

        new = ObservedStore.__new__(ObservedStore)
        _Store.__init__(new, dev, self.num_ent, self.num_rels)
        t, ot = {}, self.t
        totals = []
        for r, q_ent in enumerate((ot['q_s'], ot['q_o'])):
            names = ['%s%d' % (f, r) for f in ('ent_ptr', 'snap_t', 'snap_ptr', 'nbr_o', 'h_first', 'h_count')]
            out, tot = K.store_append([ot[f] for f in names], q_ent, self.num_ent, self.history_len, role[r], caps[r])
            t.update(zip(names, out))
            totals.append(tot)
        new._pair = {}
        if 'tables' in self._pair:
            # the pair tables ride along: the new facts sorted per role by (entity, relation, partner, time), one more
            # upload, one renet_pair_append per role over the run pointers just made.  A store that never asked for a prior
            # has no tables and runs none of this.
            _check_int32('relations', quads[:, 1])
            keys = [np.stack((quads[:, c], quads[:, 1], quads[:, oc], quads[:, 3])) for c, oc in ((0, 2), (2, 0))]
            keys = [k[:, np.lexsort(k[::-1])] for k in keys]
            pk = torch.from_numpy(np.ascontiguousarray(np.stack(keys), dtype=np.int32)).to(dev, non_blocking=True)
            new._pair['tables'] = tuple(
                K.pair_append(self._pair['tables'][r], ot['ent_ptr%d' % r], ot['snap_ptr%d' % r], t['ent_ptr%d' % r],
                              t['snap_ptr%d' % r], self.num_ent, pk[r]) for r in (0, 1))
        t['q_s'], t['q_r'], t['q_o'] = K.append_i32(ot['q_s'], n_s), K.append_i32(ot['q_r'], n_r), K.append_i32(ot['q_o'], n_o)
        t['trip_s'], t['trip_r'], t['trip_o'] = (K.append_i32(ot['trip_s'], n_s), K.append_i32(ot['trip_r'], n_r),
                                                 K.append_i32(ot['trip_o'], n_o))
        t['times'] = K.append_i32(ot['times'], n_times)
        # (a timestamp equal to the old last one: its end moves, no entry is added)
        t['trip_ptr'] = K.append_i32(ot['trip_ptr'], n_ends, n_old=self.T + (0 if joined else 1))
        keep = int(np.searchsorted(self._glob_times, t0)) if m else self.n_glob
        rows = [torch.as_tensor(global_emb_new[tt]).detach().reshape(self.glob.shape[1]).float().to(dev) for tt in want]
        new.glob = torch.cat((self.glob[:keep], torch.stack(rows))) if rows else self.glob[:keep].clone()
        t['glob_times'] = K.append_i32(ot['glob_times'], n_glob_t, n_old=keep)
        new._glob_times = np.concatenate((self._glob_times[:keep], np.asarray(want, dtype=np.int64)))
        new.t = t
        new.n_quads = new.n_facts = nq + m
        new.T, new.n_glob = int(t['times'].numel()), int(t['glob_times'].numel())
        new.cap_nodes, new.cap_edges = self.cap_nodes, self.cap_edges
        new.history_len = self.history_len
        new._gstore = None
        new.obs, new.quads = obs, obs.allq
        new._fill_struct()
        # the snapshot outputs were sized from the host's count: the kernels report theirs (8 bytes per role, one read)
        got = torch.stack(totals).cpu().numpy()
        if [int(x) for x in got[:, 0]] != caps:
            raise K.RenetHipError('store append: %s snapshots on the device where the host counts %s' % (got[:, 0], caps))
        return new


def _cached_store(cache, graph_dict, device, stamp, make):
    """The entry of `cache` for graph_dict on `device`, made by make() when there is none, when the graph store object changed
    (graph.store_for re-creates it when the dict gained timestamps) or when `stamp` did.  Keyed on the dict's identity;
    entries die with their graph_dict (weak reference), at most 8 stay resident."""
    store = G.store_for(graph_dict)
    key = (id(graph_dict), str(device))
    ent = cache.get(key)
    if ent is None or ent[0] is not store or ent[1] != stamp:
        if len(cache) > 8:
            cache.clear()
        ent = cache[key] = (store, stamp, make())
        try:
            weakref.finalize(graph_dict, cache.pop, key, None)
        except TypeError:                    # (a plain dict cannot be weakly referenced: the size bound above applies)
            pass
    return ent[2]


_graph_stores = {}


def graph_store_for(graph_dict, global_emb, num_ent, num_rels, device):
    """The resident GraphDeviceStore of (graph_dict, global_emb) on `device`; rebuilt also when the global-embedding table's
    TIMESTAMPS changed (the store holds their sorted list: the same count with different keys must not reuse it)."""
    return _cached_store(_graph_stores, graph_dict, device, hash(tuple(sorted(int(t) for t in global_emb.keys()))),
                         lambda: GraphDeviceStore(graph_dict, global_emb, num_ent, num_rels, device))


class ListBatchStore(object):
    """What DeviceBatch needs of a store, for ONE batch that arrives through the reference's list API: the batch's own
    quadruples (s, r, o) and its two FlatHistory objects (graph.FlatHistory.from_lists of the nested lists) uploaded in ONE
    int32 copy, laid out like a DeviceStore's history index (first / count per sequence, snapshot timestamps, snapshot
    pointers, neighbours) on top of the resident GraphDeviceStore.  The batch's quadruple indices are 0..B-1."""

    def __init__(self, base, trip, fs, fo, stream=None):
        self.base = base
        self.device, self.num_ent, self.num_rels = base.device, base.num_ent, base.num_rels
        trip = np.asarray(trip, dtype=np.int64)
        B = len(trip)
        if len(fs) != B or len(fo) != B:
            raise ValueError('histories and quadruples differ in length')
        parts = [trip[:, 0], trip[:, 1], trip[:, 2]]
        for fh in (fs, fo):
            parts += [fh.seq_ptr[:-1], np.diff(fh.seq_ptr), fh.step_t, fh.nbr_ptr, fh.nbr_o]
        _check_int32('ids / timestamps', *parts)
        offs, tot = [], 0
        for a in parts:
            offs.append(tot)
            tot += (len(a) + 15) & ~15                       # 64-byte aligned slices
        flat = np.zeros(tot + 16, dtype=np.int32)
        for a, o in zip(parts, offs):
            flat[o:o + len(a)] = a
        st = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            self._buf = torch.from_numpy(flat).to(self.device, non_blocking=True)
        ptr = [self._buf.data_ptr() + 4 * o for o in offs]
        sd = _StoreDev()
        sd.q_s, sd.q_r, sd.q_o = ptr[0], ptr[1], ptr[2]
        for k, n in enumerate(('h_first', 'h_count', 'snap_t', 'snap_ptr', 'nbr_o')):
            setattr(sd, n, (_P * 2)(ptr[3 + k], ptr[8 + k]))
        for n in ('times', 'trip_ptr', 'trip_s', 'trip_r', 'trip_o', 'glob_times'):
            setattr(sd, n, base.t[n].data_ptr())
        sd.T, sd.n_glob, sd.n_facts = base.T, base.n_glob, base.n_facts
        sd.num_ent, sd.num_rels = self.num_ent, self.num_rels
        self.c = sd
        self.n_quads = B

    # capacities and the pinned count buffers live in the resident store (they outlast the batch)
    cap_nodes = property(lambda self: self.base.cap_nodes, lambda self, v: setattr(self.base, 'cap_nodes', v))
    cap_edges = property(lambda self: self.base.cap_edges, lambda self, v: setattr(self.base, 'cap_edges', v))

    def _take_pinned(self):
        return self.base._take_pinned()

    def _give_pinned(self, buf):
        self.base._give_pinned(buf)


class QueryStore(ListBatchStore):
    """An observed store whose positions are QUERIES (s, r, o, t) that need not be facts of the stream: its own q_s, q_r, q_o
    and history windows h_first / h_count on top of the resident tables of an ObservedStore (snapshot tables, graph store,
    glob_times, `glob`, capacities, pinned count buffers: the base's).  The windows come from renet_query_histories (ONE
    launch): per query and role the last <= history_len snapshots of its entity with snap_t < as_of; glob_row of a history
    step follows from the step's own timestamp, so a query past the end of the stream needs no new row of the global table.
    The encoder, score, rank and top-k path of the observed pass runs on it with idx = arange(n_quads), unmodified.

    quads: int [n, 4] -- a host array (validated here: ValueError for an id out of range or as_of > t) or a device int32
    tensor, which is NOT read back: there an entity id outside [0, num_ent) counts as absent and the relation is clamped
    into range, so that no kernel indexes out of bounds (with as_of given, one flag comes back for the as_of <= t check).
    as_of: None (the query's own t), a scalar or [n].  A subject or object of -1 is an ABSENT side: its sequence is empty
    (h_count = 0) and the builder gathers entity 0 in its place; `quads` (the host copy, read back on first use for a device
    tensor) keeps the -1, which addresses no filter list."""

    def __init__(self, base, quads, as_of=None, stream=None):
        self.base = base
        self.device, self.num_ent, self.num_rels = base.device, base.num_ent, base.num_rels
        self.glob, self.history_len, self.facts = base.glob, base.history_len, base.quads
        N, R = self.num_ent, self.num_rels
        st = stream if stream is not None else torch.cuda.current_stream()
        on_dev = isinstance(quads, torch.Tensor) and quads.is_cuda
        if on_dev:
            if quads.dtype != torch.int32 or quads.dim() != 2 or quads.shape[1] != 4:
                raise ValueError('device queries are an int32 [n, 4] tensor')
            n = int(quads.shape[0])
            self._host, self._quads_dev = None, quads
            with torch.cuda.stream(st):
                s, r, o, t = quads.t().contiguous()
                r = r.clamp(0, R - 1)
                a = t
                if as_of is not None:
                    a = torch.as_tensor(as_of).to(self.device).to(torch.int32).reshape(-1).expand(n).contiguous()
                    if n and bool((a > t).any()):
                        raise ValueError('as_of later than the query\'s own timestamp')
        else:
            q = np.asarray(quads.cpu() if isinstance(quads, torch.Tensor) else quads, dtype=np.int64).reshape(-1, 4)
            n = len(q)
            a = q[:, 3] if as_of is None else np.broadcast_to(
                np.asarray(as_of.cpu() if isinstance(as_of, torch.Tensor) else as_of, dtype=np.int64).reshape(-1), (n,))
            if n:
                if q[:, [0, 2]].min() < -1 or q[:, [0, 2]].max() >= N:
                    raise ValueError('query entity outside [0, num_ent) (-1: an absent side)')
                if q[:, 1].min() < 0 or q[:, 1].max() >= R:
                    raise ValueError('query relation outside [0, num_rels)')
                if np.any(a > q[:, 3]):
                    raise ValueError('as_of later than the query\'s own timestamp')
                _check_int32('timestamps', q[:, 3])
                if a.min() < -2 ** 31:
                    raise ValueError('as_of must fit int32')
            self._host, self._quads_dev = q, None
            with torch.cuda.stream(st):
                up = torch.from_numpy(np.ascontiguousarray(np.concatenate((q.T, a[None, :])), dtype=np.int32))
                up = up.to(self.device, non_blocking=True)              # [5, n]: ONE upload, rows contiguous
                s, r, o, t, a = up
        if n == 0:
            raise ValueError('no queries')
        with torch.cuda.stream(st):
            ent = torch.stack((s, o))                                   # [2, n]: the entity of role 0 / 1
            self.present = (ent >= 0) & (ent < N)
            gather = torch.where(self.present, ent, 0)                  # (an absent side gathers entity 0)
            win = K.query_histories((base.t['ent_ptr0'], base.t['ent_ptr1']), (base.t['snap_t0'], base.t['snap_t1']), N,
                                    self.history_len, ent, a)
        self.t = dict(q_s=gather[0], q_r=r.contiguous(), q_o=gather[1], h_first0=win[0, 0], h_first1=win[0, 1],
                      h_count0=win[1, 0], h_count1=win[1, 1], t=t, as_of=a)
        sd = _StoreDev()
        for f in ('q_s', 'q_r', 'q_o'):
            setattr(sd, f, self.t[f].data_ptr())
        for f in ('h_first', 'h_count'):
            setattr(sd, f, (_P * 2)(self.t[f + '0'].data_ptr(), self.t[f + '1'].data_ptr()))
        for f in ('snap_t', 'snap_ptr', 'nbr_o'):
            setattr(sd, f, (_P * 2)(base.t[f + '0'].data_ptr(), base.t[f + '1'].data_ptr()))
        for f in ('times', 'trip_ptr', 'trip_s', 'trip_r', 'trip_o', 'glob_times'):
            setattr(sd, f, base.t[f].data_ptr())
        sd.T, sd.n_glob, sd.n_facts = base.T, base.n_glob, base.n_facts
        sd.num_ent, sd.num_rels = N, R
        self.c = sd
        self.n_quads = n

    @property
    def quads(self):
        """The host copy of the queries, int64 [n, 4], absent sides as -1 (a device tensor is read back on first use)."""
        if self._host is None:
            self._host = self._quads_dev.cpu().numpy().astype(np.int64)
        return self._host

    def pair_tables(self):
        """The base store's pair tables (ObservedStore.pair_tables): the queries add no facts."""
        return self.base.pair_tables()

    def sides_present(self):
        """(any subject present, any object present): a side that no query has needs no rows at all."""
        if self._host is not None:
            return bool((self._host[:, 0] >= 0).any()), bool((self._host[:, 2] >= 0).any())
        return tuple(bool(x) for x in self.present.any(dim=1).cpu())

    # filter_index.filter_index_for caches on its owner: the index of the base stream's facts belongs to the base store
    _filter_index = property(lambda self: getattr(self.base, '_filter_index', None),
                             lambda self, v: setattr(self.base, '_filter_index', v))


MAX_GROUPED = 4096           # sequences per grouped batch (one workgroup sorts their lengths)
MAX_BOTH = MAX_GROUPED // 2  # quadruples per merged batch: two sequences each, the same sort


class GroupedBatchStore(ListBatchStore):
    """What GroupedDeviceBatch needs of a store, for ONE grouped batch of one direction: its s, r, group and FlatHistory
    (first / count per sequence, step timestamps, neighbour pointers, neighbours) uploaded in ONE int32 copy, on top of the
    resident GraphDeviceStore and its subject index.  The ranges the host builder checks are checked here: the kernels
    index with these ids."""

    def __init__(self, base, s, r, group, fh, stream=None):
        self.base = base
        self.device, self.num_ent, self.num_rels = base.device, base.num_ent, base.num_rels
        s, r, group = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (s, r, group))
        B = len(s)
        if len(fh) != B or len(r) != B or len(group) != B:
            raise ValueError('histories, subjects, relations and groups differ in length')
        if base._store.max_ent >= self.num_ent or base._store.max_rel >= self.num_rels:
            raise ValueError('graph_dict holds entity id %d / relation id %d but num_ent = %d, num_rels = %d'
                             % (base._store.max_ent, base._store.max_rel, self.num_ent, self.num_rels))
        parts = [s, r, group, fh.seq_ptr[:-1], np.diff(fh.seq_ptr), fh.step_t, fh.nbr_ptr, fh.nbr_o]
        _check_int32('ids / timestamps', *parts)
        if B and (s.max() >= self.num_ent or r.max() >= self.num_rels):
            raise ValueError('batch subject / relation id out of range')
        if len(fh.nbr_o) and fh.nbr_o.max() >= self.num_ent:
            raise ValueError('history neighbour id out of range')
        if len(fh.nbr_ptr) != len(fh.step_t) + 1 or fh.seq_ptr[-1] != len(fh.step_t) or fh.nbr_ptr[-1] != len(fh.nbr_o):
            raise ValueError('inconsistent FlatHistory')
        offs, tot = [], 0
        for a in parts:
            offs.append(tot)
            tot += (len(a) + 15) & ~15                       # 64-byte aligned slices
        flat = np.zeros(tot + 16, dtype=np.int32)
        for a, o in zip(parts, offs):
            flat[o:o + len(a)] = a
        st = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            self._buf = torch.from_numpy(flat).to(self.device, non_blocking=True)
            by_subj, subj_sorted = base.subject_index()
        sd = _GroupedStoreDev()
        for n, o in zip(('s', 'r', 'group', 'h_first', 'h_count', 'step_t', 'nbr_ptr', 'nbr_o'), offs):
            setattr(sd, n, self._buf.data_ptr() + 4 * o)
        for n in ('times', 'trip_ptr', 'trip_s', 'trip_r', 'trip_o', 'glob_times'):
            setattr(sd, n, base.t[n].data_ptr())
        sd.by_subj, sd.subj_sorted = by_subj.data_ptr(), subj_sorted.data_ptr()
        sd.n_steps, sd.n_nbr = len(fh.step_t), len(fh.nbr_o)
        sd.T, sd.n_glob, sd.n_facts = base.T, base.n_glob, base.n_facts
        sd.num_ent, sd.num_rels = self.num_ent, self.num_rels
        self.c = sd
        self.n_quads = B
        self.longest = int(np.diff(fh.seq_ptr).max()) if B else 0


class _Host(object):
    """Host-side view of a DeviceBatch (what graph._HostView offers for a host-built batch)."""

    def __init__(self, batch, c):
        self._batch = batch
        self.N, self.E, self.S, self.nnz, self.L, self.nA, self.B = batch.N, batch.E, batch.S, batch.nnz, batch.L, batch.nA, batch.B
        self.step_off = c[C_STEP_OFF:C_STEP_OFF + batch.L + 1].astype(np.int32)
        self.batch_sizes = np.diff(self.step_off).astype(np.int64)
        self._perm = None

    @property
    def perm(self):
        if self._perm is None:              # sorted position -> sequence of the merged batch (one small D2H, on demand)
            self._perm = self._batch._v['perm'].cpu().numpy().astype(np.int64)
        return self._perm


# the fronts of csrc/builder_both.hip, builder_grouped.hip and builder_full.hip: (workspace size, build) of the C ABI
_FRONT_BOTH = ('renet_build_batch_workspace', 'renet_build_batch_both')
_FRONT_GROUPED = ('renet_build_batch_grouped_workspace', 'renet_build_batch_grouped')
_FRONT_FULL = ('renet_build_full_graphs_workspace', 'renet_build_full_graphs')


def _launch(front, store, idx_dev, n, lead, own, cn, ce, stream):
    """One builder call on `stream`: lays the int32 outputs out as 64-int aligned slices of ONE buffer -- the graph part that
    every front fills for capacities (cn, ce), then the front's `own` {name: size} -- allocates buffer / norm / workspace on
    the stream, fills the _BatchOut (views by field name, the plans that have slices) and calls front(store, idx_dev, n,
    *lead, ...).  Returns (views, norm, keep): the int32 output views by name (incl. 'counts', still on the device), the fp32
    norm, and the objects that must stay alive until the kernels have run, the buffer first.  Nothing is synchronised or
    read back here."""
    L = _bind()
    T2 = 2 * store.num_rels
    cc = ce // G.CHUNK + T2 + 2
    sizes = dict(node_ent=cn, row_ptr=cn + 2, col=ce, etype=ce, heavy_rows=cn, e_src=ce, e_dst=ce, chunk_ptr=cc + 1,
                 chunk_type=cc, type_chunk_ptr=T2 + 1, it_src=ce + cn, it_type=ce + cn, grp_ptr=cn + 2, counts=NCOUNTS,
                 plan_order0=cn, plan_seg0=cn + 1, plan_target0=cn, **own)
    offs, tot = {}, 0
    for f, m in sizes.items():
        offs[f] = tot
        tot += (m + 63) & ~63
    nbytes = getattr(L, front[0])(ctypes.addressof(store.c), n, cn, ce)
    with torch.cuda.stream(stream):          # the buffers belong to the stream the builder runs on
        buf = torch.empty(tot, device=store.device, dtype=torch.int32)
        norm = torch.empty(cn, device=store.device, dtype=torch.float32)
        ws = torch.empty(nbytes // 4 + 64, device=store.device, dtype=torch.int32)
    v = {f: buf[o:o + sizes[f]] for f, o in offs.items()}
    out = _BatchOut()
    for f, _ in _BatchOut._fields_:
        if f in v:
            setattr(out, f, v[f].data_ptr())
    out.norm = norm.data_ptr()
    for f in ('plan_order', 'plan_seg', 'plan_target'):
        setattr(out, f, (_P * 4)(*[v[f + str(k)].data_ptr() if f + str(k) in v else None for k in range(4)]))
    out.cap_nodes, out.cap_edges = cn, ce
    rc = getattr(L, front[1])(ctypes.addressof(store.c), idx_dev.data_ptr() if idx_dev is not None else None, n, *lead, G.HEAVY, G.GROUP_ITEMS, G.CHUNK,
                              ctypes.addressof(out), ws.data_ptr(), nbytes, stream.cuda_stream)
    if rc != 0:
        raise K.RenetHipError('%s failed with code %d' % (front[1], rc))
    return v, norm, (buf, ws, out, idx_dev)


class _PendingBatch(G.BatchGraph):
    """A batch graph whose builder kernels have been enqueued: the index upload, one _launch, and the hand-over of the counts
    through a pinned buffer of the store (async copy + event).  finalize() waits for the counts and slices the graph part
    of graph.BatchGraph out of the views; a subclass names its front and its own slices, judges the counts (_accept) and
    slices what it adds (_own_part)."""

    def __init__(self, front, store, idx, lead, own, cn, ce, stream):
        G.BatchGraph.__init__(self)
        self.store = store
        st = stream if stream is not None else torch.cuda.current_stream()
        idx_dev = None                               # (idx = None: the front takes the store's own order, nothing to upload)
        if idx is not None:
            with torch.cuda.stream(st):
                idx_dev = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(store.device, non_blocking=True)
        n = len(idx) if idx is not None else store.n_quads
        self._v, self._norm, self._keep = _launch(front, store, idx_dev, n, lead, own, cn, ce, st)
        self._counts_host = store._take_pinned()     # owned by this batch until finalize() / release
        self._stream = st
        with torch.cuda.stream(st):
            self._counts_host.copy_(self._v['counts'], non_blocking=True)
            self._done = torch.cuda.Event()
            self._done.record(st)
        self._final = False

    def finalize(self):
        """Waits for the counts, slices the outputs to their sizes.  True when the batch is ready (and on every later call);
        False if the subclass turned the counts down (DeviceBatch: a capacity was exceeded, rebuild)."""
        if self._final:
            return True
        self._done.synchronize()
        c = self._counts_host.numpy().astype(np.int64)      # (a copy: the pinned buffer goes back to the free-list)
        self.store._give_pinned(self._counts_host)
        self._counts_host = None
        self._buf, self._keep = self._keep[0], None          # (workspace, struct and indices are done with)
        cur = torch.cuda.current_stream()
        if cur != self._stream:                  # built on a side stream, consumed on this one
            self._buf.record_stream(cur)
            self._norm.record_stream(cur)
        if not self._accept(c):
            return False
        self._graph_part(c)
        self._own_part(c)
        self._final = True
        return True

    def _plan(self, k, n_rows, c):
        v, u, p = self._v, int(c[C_NSEG0 + k]), G.SegPlan()
        p.order, p.seg_ptr, p.target = v['plan_order%d' % k][:n_rows], v['plan_seg%d' % k][:u + 1], v['plan_target%d' % k][:u]
        p.num_segments = u
        return p

    def _graph_part(self, c):
        """The graph part of graph.BatchGraph, for a batch without a row prefix (nA = N)."""
        v = self._v
        N, E = int(c[C_N]), int(c[C_E])
        self.N = self.nA = N
        self.E = self.E_out = E
        self.num_types = 2 * self.store.num_rels
        self.heavy_thresh = G.HEAVY
        self.node_ent = v['node_ent'][:N]
        self.row_ptr, self.col, self.etype = v['row_ptr'][:N + 1], v['col'][:E], v['etype'][:E]
        self.norm = self._norm[:N]
        nh = int(c[C_NHEAVY])
        self.heavy_rows = self.heavy_rows_out = v['heavy_rows'][:nh] if nh else None
        self.e_src, self.e_dst = v['e_src'][:E], v['e_dst'][:E]
        self.n_chunks = int(c[C_NCHUNKS])
        self.chunk_ptr, self.chunk_type = v['chunk_ptr'][:self.n_chunks + 1], v['chunk_type'][:self.n_chunks]
        self.type_chunk_ptr = v['type_chunk_ptr']
        ni = int(c[C_NITEMS])
        self.it_src, self.it_type = v['it_src'][:ni], v['it_type'][:ni]
        self.n_groups = self.n_groups_out = int(c[C_NGROUPS])
        self.grp_ptr = v['grp_ptr'][:self.n_groups + 1]
        self.plan_node_ent = self._plan(0, N, c)

    def __del__(self):
        # a batch dropped before finalize(): its copy may still be in flight -- wait for it before the buffer is reused
        try:
            if getattr(self, '_counts_host', None) is not None:
                self._done.synchronize()
                self.store._give_pinned(self._counts_host)
                self._counts_host = None
        except Exception:       # interpreter shutdown
            pass


class DeviceBatch(_PendingBatch):
    """A merged batch built on the device from the quadruple indices `idx` of `store`.  After finalize() it carries the
    attributes of graph.BatchGraph, graph and sequence part, with the row prefix [0, nA) of the subject rows."""

    _LABELS = ('rel_label', 'ent_label')

    def __init__(self, store, idx, seq_len, stream=None):
        self.n_quads = int(len(idx))
        self.B = B2 = 2 * self.n_quads              # sequences of the merged batch (graph.HostBatch.B)
        cn, ce = store.cap_nodes, store.cap_edges
        cs = B2 * MAXL
        T2 = 2 * store.num_rels
        cc = ce // G.CHUNK + T2 + 2
        own = dict(node_slot=cn, e_src2=ce, e_dst2=ce, chunk_ptr2=cc + 1, chunk_type2=cc, type_chunk_ptr2=T2 + 1,
                   subj_row=cs, row_seq=cs, row_ent=cs, row_rel=cs, glob_row=cs, s_sorted=B2, r_sorted=B2,
                   rel_label=B2, ent_label=B2, perm=B2, step_off=MAXL + 1,
                   plan_order1=cs, plan_seg1=cs + 1, plan_target1=cs,
                   plan_order2=B2, plan_seg2=B2 + 1, plan_target2=B2, plan_order3=B2, plan_seg3=B2 + 1, plan_target3=B2)
        _PendingBatch.__init__(self, _FRONT_BOTH, store, idx, (int(seq_len),), own, cn, ce, stream)

    def _accept(self, c):
        """False if a capacity was exceeded (the store's capacities are then doubled: rebuild)."""
        err = c[C_ERR]
        if err & 4:
            self.store.cap_nodes *= 2
        if err & 8:
            self.store.cap_edges *= 2
        if err & 3:
            raise KeyError('a history timestamp is missing from graph_dict / global_emb')
        return err == 0

    def _own_part(self, c):
        v = self._v
        N, S = self.N, int(c[C_S])
        self.nA, self.E_out, self.S, self.nnz, self.L = int(c[C_NA]), int(c[C_EOUT]), S, int(c[C_NNZ]), int(c[C_L])
        self.node_slot = v['node_slot'][:N]
        nho = int(c[C_NHEAVY_OUT])
        self.heavy_rows_out = v['heavy_rows'][:nho] if nho else None
        self.n_chunks2, self.n_groups_out = int(c[C_NCHUNKS2]), int(c[C_NGROUPS_OUT])
        self.type_chunk_ptr2 = v['type_chunk_ptr2']
        self.chunk_ptr2, self.chunk_type2 = v['chunk_ptr2'][:self.n_chunks2 + 1], v['chunk_type2'][:self.n_chunks2]
        self.e_src2, self.e_dst2 = v['e_src2'][:self.E_out], v['e_dst2'][:self.E_out]
        for n in ('subj_row', 'row_seq', 'row_ent', 'row_rel', 'glob_row'):
            setattr(self, n, v[n][:S])
        for n in ('s_sorted', 'r_sorted') + self._LABELS:
            setattr(self, n, v[n])
        self.step_off = v['step_off'][:self.L + 1]
        self.plan_subj_row, self.plan_s, self.plan_r = self._plan(1, S, c), self._plan(2, self.B, c), self._plan(3, self.B, c)
        # the few host-side values the model still needs (packing of the GRU launches, reporting)
        self.host = _Host(self, c)


class GroupedDeviceBatch(DeviceBatch):
    """The grouped batch of ONE direction (graph.build_batch(..., sort=True, group=...)) built on the device from a
    GroupedBatchStore: B sequences, a member graph per (group, timestamp).  After finalize() it carries what a DeviceBatch
    carries (it shares _accept and _own_part), without rel_label / ent_label; `host.perm` and `host.batch_sizes` are what
    forward_grouped's callers read."""
    _LABELS = ()

    def __init__(self, store, seq_len, stream=None):
        self.n_quads = self.B = B = int(store.n_quads)
        if not 0 < B <= MAX_GROUPED or not 0 < int(seq_len) <= MAXL:
            raise ValueError('a grouped device batch has 1 .. %d sequences of at most %d steps' % (MAX_GROUPED, MAXL))
        if store.longest > int(seq_len):
            raise ValueError('history longer than seq_len (%d > %d)' % (store.longest, int(seq_len)))
        cn, ce = store.cap_nodes, store.cap_edges
        cs = B * MAXL
        T2 = 2 * store.num_rels
        cc = ce // G.CHUNK + T2 + 2
        own = dict(node_slot=cn, e_src2=ce, e_dst2=ce, chunk_ptr2=cc + 1, chunk_type2=cc, type_chunk_ptr2=T2 + 1,
                   subj_row=cs, row_seq=cs, row_ent=cs, row_rel=cs, glob_row=cs, s_sorted=B, r_sorted=B, perm=B,
                   step_off=MAXL + 1, plan_order1=cs, plan_seg1=cs + 1, plan_target1=cs,
                   plan_order2=B, plan_seg2=B + 1, plan_target2=B, plan_order3=B, plan_seg3=B + 1, plan_target3=B)
        # (idx = None: the sequences in the order of the store's arrays -- the store's upload is the only one)
        _PendingBatch.__init__(self, _FRONT_GROUPED, store, None, (int(seq_len),), own, cn, ce, stream)


# ---- full-graph batches of the global model (csrc/builder_full.hip: renet_build_full_graphs) ------------------------------
MAX_FULL_GRAPHS = 1024       # member graphs per call (one workgroup scans their counts)


class FullGraphStore(_Store):
    """What a FULL-graph batch (graph.build_full_graphs: the global model, Aggregator.py:44-55 / 87-98) needs resident: per
    timestamp of graph_dict, in the dict's order, the node list `ent` and the facts with their LOCAL endpoints (ls, r, lo)
    of graph.TimeGraph.  `host` holds the int32 arrays; they are uploaded once when `device` is given (device=None: host
    arrays only, nothing touches a GPU)."""

    def __init__(self, graph_dict, num_rels, device=None):
        store = G.store_for(graph_dict)
        gs = store._graphs
        self.store = store                                              # (index_of maps timestamps to positions)
        self.T = len(gs)
        node_ptr = np.concatenate(([0], np.cumsum(store.node_cnt))).astype(np.int64)
        trip_ptr = np.asarray(store.trip_ptr, dtype=np.int64)
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
        ent, ls, lo = cat([g.ent for g in gs]), cat([g.ls for g in gs]), cat([g.lo for g in gs])
        r = np.asarray(store.trip_r, dtype=np.int64)
        _Store.__init__(self, device, int(ent.max()) + 1 if len(ent) else 1, num_rels)
        # the kernels index with these unchecked (a guard on the device reports, it does not repair): validate once, here
        if 2 * self.num_rels > 1024 or self.num_rels <= 0:
            raise ValueError('the device builder handles at most 512 relations')
        _check_int32('node / edge counts', node_ptr[-1:], 2 * trip_ptr[-1:])
        _check_int32('entity ids', ent, limit=2 ** 31 - 1)
        if len(r) and (r.min() < 0 or r.max() >= self.num_rels):
            raise ValueError('relation id outside [0, num_rels)')
        n_of_fact = np.repeat(store.node_cnt, np.diff(trip_ptr))
        if len(ls) and (min(ls.min(), lo.min()) < 0 or np.any(ls >= n_of_fact) or np.any(lo >= n_of_fact)):
            raise ValueError('local node id outside its graph')
        self.n_nodes, self.n_facts = int(node_ptr[-1]), int(trip_ptr[-1])
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        self.host = dict(node_ptr=i32(node_ptr), node_ent_all=i32(ent), trip_ptr=i32(trip_ptr), trip_ls=i32(ls),
                         trip_r=i32(r), trip_lo=i32(lo))
        self.t, self.c = None, None
        if device is not None:
            self.t = {n: torch.from_numpy(a).to(device) for n, a in self.host.items()}
            sd = _FullStoreDev()
            for n in self.host:
                setattr(sd, n, self.t[n].data_ptr())
            sd.T, sd.n_nodes, sd.n_facts, sd.num_ent, sd.num_rels = self.T, self.n_nodes, self.n_facts, self.num_ent, self.num_rels
            self.c = sd

    def sizes(self, tidx):
        """(node offsets [G + 1], fact offsets [G + 1]) of the member graphs tidx -- N and E / 2 are their last entries."""
        tidx = np.asarray(tidx, dtype=np.int64).reshape(-1)
        if len(tidx) and (tidx.min() < 0 or tidx.max() >= self.T):
            raise KeyError('timestamp index outside the store')
        npt, tpt = self.host['node_ptr'].astype(np.int64), self.host['trip_ptr'].astype(np.int64)
        return (np.concatenate(([0], np.cumsum(npt[tidx + 1] - npt[tidx]))),
                np.concatenate(([0], np.cumsum(tpt[tidx + 1] - tpt[tidx]))))

    def host_edges(self, tidx):
        """numpy specification of the device front (fg_edges_kernel): (node_ent, src, dst, et) of the batch of member graphs
        tidx.  Member graph k owns edge positions [2 fact_off[k], 2 fact_off[k + 1]): its facts forward (ls -> lo, type r),
        then reversed (lo -> ls, type r + R) -- the order of graph.build_full_graphs' concatenation, which decides every tie
        of the stable sorts behind it."""
        tidx = np.asarray(tidx, dtype=np.int64).reshape(-1)
        noff, foff = self.sizes(tidx)
        h = {n: a.astype(np.int64) for n, a in self.host.items()}
        nf = np.diff(foff)
        node_ent = h['node_ent_all'][G.ragged_arange(h['node_ptr'][tidx], np.diff(noff))]
        j = G.ragged_arange(h['trip_ptr'][tidx], nf)                    # store fact of every batch fact, graph-major
        k = np.repeat(np.arange(len(tidx), dtype=np.int64), nf)
        e = np.arange(len(j), dtype=np.int64) - foff[k]                 # fact number inside its graph
        a, b, r = h['trip_ls'][j] + noff[k], h['trip_lo'][j] + noff[k], h['trip_r'][j]
        E = 2 * int(foff[-1])
        src, dst, et = np.empty(E, np.int64), np.empty(E, np.int64), np.empty(E, np.int64)
        fwd, rev = 2 * foff[k] + e, 2 * foff[k] + nf[k] + e
        src[fwd], dst[fwd], et[fwd] = a, b, r
        src[rev], dst[rev], et[rev] = b, a, r + self.num_rels
        return node_ent, src, dst, et


_full_stores = {}


def full_graph_store_for(graph_dict, num_rels, device=None):
    """The resident FullGraphStore of graph_dict on `device`, rebuilt also when num_rels changed.  Validated by the IDENTITY
    of the dict's graph store -- no key is hashed per call."""
    return _cached_store(_full_stores, graph_dict, device, int(num_rels), lambda: FullGraphStore(graph_dict, num_rels, device))


def build_full_graphs_raw(store, tidx_dev, n_graphs, cap_nodes, cap_edges, stream=None):
    """The C call (renet_build_full_graphs) for the given capacities on `stream`, without a batch object: what _launch
    returns.  (FullGraphBatch sizes the buffers exactly; the capacity-guard test calls this with capacities one too small.)"""
    st = stream if stream is not None else torch.cuda.current_stream()
    return _launch(_FRONT_FULL, store, tidx_dev, int(n_graphs), (), dict(seg_ptr=int(n_graphs) + 1), int(cap_nodes),
                   int(cap_edges), st)


class _FullHost(object):
    """Host-side view of a FullGraphBatch: the scalars of the graph.HostBatch that graph.build_full_graphs returns."""

    def __init__(self, b):
        self.G, self.N, self.E, self.nA, self.num_types = b.G, b.N, b.E, b.nA, b.num_types
        self.n_chunks, self.n_groups, self.n_groups_out, self.heavy_thresh = b.n_chunks, b.n_groups, b.n_groups_out, b.heavy_thresh


class FullGraphBatch(_PendingBatch):
    """The disjoint union of the full graphs of store timestamps `tidx` (a repeated index = two member graphs), built on
    the device.  After finalize() it carries the graph part of graph.BatchGraph for a graph.build_full_graphs batch (no row
    prefix, no *2 arrays; G and seg_ptr), the arrays bit-identical (tests/test_gpu_full_graph_builder.py).  N and E are known
    on the host before the launch: the buffers are sized exactly, and the only data read back is the counts."""

    def __init__(self, store, tidx, stream=None):
        tidx = np.ascontiguousarray(tidx, dtype=np.int64).reshape(-1)
        if not 0 < len(tidx) <= MAX_FULL_GRAPHS:
            raise ValueError('a full-graph batch has 1 .. %d member graphs' % MAX_FULL_GRAPHS)
        noff, foff = store.sizes(tidx)
        self.G = int(len(tidx))
        self._sizes = (int(noff[-1]), 2 * int(foff[-1]))
        _PendingBatch.__init__(self, _FRONT_FULL, store, tidx, (), dict(seg_ptr=self.G + 1), max(self._sizes[0], 1),
                               max(self._sizes[1], 2), stream)

    def _accept(self, c):
        """The capacities are exact, so an error bit here is a store that does not describe its graphs: it raises."""
        N, E = int(c[C_N]), int(c[C_E])
        if c[C_ERR] != 0 or (N, E) != self._sizes:
            raise K.RenetHipError('full-graph builder: error bits %d, N %d E %d where the store gives %s'
                                  % (c[C_ERR], N, E, self._sizes))
        return True

    def _own_part(self, c):
        self.seg_ptr = self._v['seg_ptr']
        self.host = _FullHost(self)
