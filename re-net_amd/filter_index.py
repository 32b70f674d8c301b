"""Resident filter index of the time-agnostic filtered evaluation (model.py:392-401 of the reference).

evaluate_filter ranks the gold object of (s, r, o, t) among all entities EXCEPT the other objects o' for which (s, r, o') is a
known fact at any time, and the gold subject likewise against the known subjects of (o, r).  The known facts are the
`all_triplets` array that test.py / train.py hand to every call: the same object for a whole run.  `FilterIndex` is built from
it ONCE: two CSR tables

    (s, r) -> sorted unique o        (side 'o': the objects that filter an object ranking)
    (o, r) -> sorted unique s        (side 's')

with the sorted key codes on the host and the int32 column lists resident on the device.  A lookup of n query keys is two
`searchsorted` calls over the key codes, one upload of 2 (n + 1) int32 (row_ptr of the result and the position of every
row's list in the resident table) and one device gather: no per-call sort of all_triplets and no per-call upload of the
lists.  The same (s, r, o) appears at many timestamps; the index deduplicates, so every column is listed at most once per
row, which renet_rank_rows (csrc/rank.hip) relies on.

The TIME-AWARE filtered setting (RE-GCN, xERTE, TITer: only the completions that are true at the query's own timestamp are
removed) takes two more tables of the same form, built on first use from the four columns of all_triplets

    (s, r, t) -> sorted unique o     (side 'o', keys[n, 3])
    (o, r, t) -> sorted unique s     (side 's')

each with its own resident int32 column list.  The timestamps are rank-compressed before they enter the key code, so the code
is bounded by span * span * (number of distinct timestamps), which is checked against int64.  `ranges` answers a query
with (start, count) INTO the resident list -- one upload of 2 n int32, no device gather --, the form renet_rank_rows3 takes;
`ranges_both` answers the time-agnostic and the time-aware query of the same keys together (one sort, one upload).
"""
import numpy as np
import torch

import graph as G
from gpu_builder import _check_int32

SIDES = {'o': (0, 1, 2), 's': (2, 1, 0)}                 # side -> (key column, key column, value column) of all_triplets


class _Table(object):
    """One CSR table: `codes` (sorted unique key codes), `ptr` [len(codes) + 1], `cols` (int32; sorted, unique per key)."""
    __slots__ = ('codes', 'ptr', 'cols')

    def __init__(self, code, val):
        order = np.lexsort((val, code))
        code, val = code[order], val[order]
        keep = np.ones(len(code), dtype=bool)
        keep[1:] = (code[1:] != code[:-1]) | (val[1:] != val[:-1])
        code, val = code[keep], val[keep]
        first = np.ones(len(code), dtype=bool)
        first[1:] = code[1:] != code[:-1]
        self.codes = code[first]
        self.ptr = np.concatenate((np.nonzero(first)[0], [len(code)])).astype(np.int64)
        self.cols = val.astype(np.int32)


class FilterIndex(object):
    def __init__(self, all_triplets):
        at = all_triplets.detach().cpu().numpy() if isinstance(all_triplets, torch.Tensor) else np.asarray(all_triplets)
        full = at.astype(np.int64)
        at = full[:, :3]
        _check_int32('entity / relation ids', at)
        self.span = (int(at.max()) if len(at) else 0) + 2
        self.tables = {side: _Table(at[:, k0] * self.span + at[:, k1], at[:, v]) for side, (k0, k1, v) in SIDES.items()}
        _check_int32('filter list sizes', *(t.ptr[-1:] for t in self.tables.values()))
        self._dev = {}                                    # (side, timed, device) -> the resident int32 column list
        self._quads = full[:, :4] if full.shape[1] >= 4 else None      # kept for the timed tables (built on first use)
        self._times = None                                # sorted unique timestamps: a timestamp's rank is its key digit
        self._timed = {}                                  # side -> _Table keyed by (k0 * span + k1) * len(times) + rank(t)

    def timed_table(self, side):
        """The table (s, r, t) -> o (side 'o') / (o, r, t) -> s (side 's'), built at the first request."""
        tab = self._timed.get(side)
        if tab is None:
            at = self._quads
            if at is None:
                raise ValueError('the time-aware filter needs the timestamps: all_triplets has no fourth column')
            if self._times is None:
                self._times = np.unique(at[:, 3])
                # codes are < span * span * len(times); python integers, so the check itself cannot overflow
                if self.span * self.span * max(len(self._times), 1) >= 2 ** 63:
                    raise ValueError('time-aware filter keys do not fit int64: span %d, %d timestamps'
                                     % (self.span, len(self._times)))
            k0, k1, v = SIDES[side]
            code = (at[:, k0] * self.span + at[:, k1]) * max(len(self._times), 1) + np.searchsorted(self._times, at[:, 3])
            tab = self._timed[side] = _Table(code, at[:, v])
            _check_int32('filter list sizes', tab.ptr[-1:])
        return tab

    def _codes(self, keys):
        """(time-agnostic key code, time-aware key code or None) per query, -1 for a key that cannot have facts, for
        keys[n, 2] or keys[n, 3] (the last column a timestamp: the time-aware tables must exist)."""
        k0, k1 = keys[:, 0], keys[:, 1]
        inside = (k0 >= 0) & (k1 >= 0) & (k0 < self.span) & (k1 < self.span)
        code = k0 * self.span + k1
        want = np.where(inside, code, -1)
        if keys.shape[1] == 2:
            return want, None
        nt = len(self._times)
        rank = np.minimum(np.searchsorted(self._times, keys[:, 2]), max(nt - 1, 0))
        seen = inside & (self._times[rank] == keys[:, 2]) if nt else np.zeros(len(keys), dtype=bool)
        return want, np.where(seen, code * max(nt, 1) + rank, -1)

    @staticmethod
    def _find(tab, want, order):
        """(start [n], count [n]) of the key codes `want` in `tab`, searched in the order `order` (a permutation that sorts
        them, or nearly: a binary search over 10^5 - 10^6 codes is bound by cache misses, and neighbours in sorted order
        share most of their path -- less than half the time of the same searches in query order)."""
        pos = np.empty(len(want), dtype=np.int64)
        pos[order] = np.searchsorted(tab.codes, want[order])
        pos = np.minimum(pos, max(len(tab.codes) - 1, 0))
        hit = (tab.codes[pos] == want) if len(tab.codes) else np.zeros(len(want), dtype=bool)
        start = np.where(hit, tab.ptr[pos], 0)
        count = np.where(hit, tab.ptr[np.minimum(pos + 1, len(tab.ptr) - 1)] - start, 0)
        return start.astype(np.int64), count.astype(np.int64)

    def _keys(self, side, keys):
        """keys as int64 [n, 2] or [n, 3] -> (keys, the table they address)."""
        keys = np.asarray(keys, dtype=np.int64)
        keys = keys.reshape(-1, 3 if keys.ndim == 2 and keys.shape[1] == 3 else 2)
        return keys, self.timed_table(side) if keys.shape[1] == 3 else self.tables[side]

    def ranges_host(self, side, keys):
        """(start [n], count [n]) int64: the list of key i is cols[start[i] : start[i] + count[i]] of the table the keys
        address (keys[n, 2]: tables[side]; keys[n, 3]: timed_table(side)).  A key without facts -- an unseen timestamp, a
        negative id or one beyond the indexed range included -- gets count 0."""
        keys, tab = self._keys(side, keys)
        want, want_t = self._codes(keys)
        want = want if want_t is None else want_t
        return self._find(tab, want, np.argsort(want, kind='stable'))

    def ranges_both_host(self, side, keys):
        """ranges_host of keys[:, :2] and of keys (keys[n, 3]) -> (start_a, count_a, start_t, count_t), from ONE sort of the
        queries: the time-aware code is monotone in the time-agnostic one, so the order that sorts the latter sorts the
        former as well up to the timestamps of equal (k0, k1) -- which are equal within one evaluated group."""
        keys, tab_t = self._keys(side, np.asarray(keys, dtype=np.int64).reshape(-1, 3))
        want_a, want_t = self._codes(keys)
        order = np.argsort(want_a, kind='stable')
        return self._find(self.tables[side], want_a, order) + self._find(tab_t, want_t, order)

    def lookup_host(self, side, keys):
        """For the n query keys[n, 2] ((s, r) for side 'o', (o, r) for side 's'): (row_ptr [n + 1], start [n]) -- row i of
        the result is tables[side].cols[start[i] : start[i] + row_ptr[i + 1] - row_ptr[i]]; a key without facts (an id
        beyond the indexed range included) gets an empty row."""
        start, count = self.ranges_host(side, np.asarray(keys, dtype=np.int64).reshape(-1, 2))
        return np.concatenate(([0], np.cumsum(count))).astype(np.int64), start

    def lists_host(self, side, keys):
        """(row_ptr [n + 1], cols [nnz]) of the query on the host (tests, tools)."""
        row_ptr, start = self.lookup_host(side, keys)
        return row_ptr, self.tables[side].cols[G.ragged_arange(start, np.diff(row_ptr))]

    def resident(self, side, device, timed=False):
        key = (side, bool(timed), str(device))
        cols = self._dev.get(key)
        if cols is None:
            tab = self.timed_table(side) if timed else self.tables[side]
            cols = self._dev[key] = torch.from_numpy(tab.cols).to(device)
        return cols

    def ranges(self, side, keys, device):
        """-> (cols, start [n], count [n]): the resident int32 column list that the keys address and, per key, its range in
        it (int32 device tensors from ONE upload of 2 n int32): the operands of renet_hip.rank_rows3."""
        keys, _ = self._keys(side, keys)
        up = torch.from_numpy(np.stack(self.ranges_host(side, keys)).astype(np.int32)).to(device)
        return self.resident(side, device, timed=keys.shape[1] == 3), up[0], up[1]

    def ranges_both(self, side, keys, device):
        """-> (cols_a, start_a, count_a, cols_t, start_t, count_t) for keys[n, 3]: ranges(side, keys[:, :2]) + ranges(side,
        keys), the six list operands of renet_hip.rank_rows3, from one sort of the queries and ONE upload of 4 n int32."""
        up = torch.from_numpy(np.stack(self.ranges_both_host(side, keys)).astype(np.int32)).to(device)
        return (self.resident(side, device), up[0], up[1], self.resident(side, device, timed=True), up[2], up[3])

    def lookup(self, side, keys, device):
        """-> (filt_ptr [n + 1], filt_col [nnz]): int32 device tensors, the operands of renet_hip.rank_rows."""
        row_ptr, start = self.lookup_host(side, keys)
        n, nnz = len(start), int(row_ptr[-1])
        _check_int32('filter list sizes', row_ptr[-1:])
        up = np.zeros((2, n + 1), dtype=np.int32)
        up[0], up[1, :n] = row_ptr, start
        up = torch.from_numpy(up).to(device)
        if nnz == 0:
            return up[0], torch.zeros(1, device=device, dtype=torch.int32)
        # position in the resident list of result element k of row i: start[i] + (k - row_ptr[i])
        shift = torch.repeat_interleave(up[1, :n] - up[0, :n], up[0, 1:] - up[0, :n], output_size=nnz)
        return up[0], self.resident(side, device)[(shift + torch.arange(nnz, device=device, dtype=torch.int32)).long()]


def filter_index_for(owner, all_triplets):
    """The FilterIndex of `all_triplets`, cached on `owner` (attribute _filter_index) by the IDENTITY of the array, as
    RENet._la_at caches its host copy: the drivers pass the same object with every call.  A different object (or a tensor
    written in place since) releases the cached index and builds a new one."""
    version = getattr(all_triplets, '_version', None)
    ent = getattr(owner, '_filter_index', None)
    if ent is None or ent[0] is not all_triplets or ent[1] != version:
        ent = owner._filter_index = (all_triplets, version, FilterIndex(all_triplets))
    return ent[2]
