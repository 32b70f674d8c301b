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
"""
import numpy as np
import torch

import graph as G
from gpu_builder import _check_int32

SIDES = {'o': (0, 1, 2), 's': (2, 1, 0)}                 # side -> (key column, key column, value column) of all_triplets


class _Table(object):
    """One CSR table: `codes` (sorted unique key codes), `ptr` [len(codes) + 1], `cols` (int32; sorted, unique per key)."""
    __slots__ = ('codes', 'ptr', 'cols')

    def __init__(self, key0, key1, val, span):
        code = key0 * span + key1
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
        at = at.astype(np.int64)[:, :3]
        _check_int32('entity / relation ids', at)
        self.span = (int(at.max()) if len(at) else 0) + 2
        self.tables = {side: _Table(at[:, k0], at[:, k1], at[:, v], self.span) for side, (k0, k1, v) in SIDES.items()}
        _check_int32('filter list sizes', *(t.ptr[-1:] for t in self.tables.values()))
        self._dev = {}                                    # (side, device) -> the resident int32 column list

    def lookup_host(self, side, keys):
        """For the n query keys[n, 2] ((s, r) for side 'o', (o, r) for side 's'): (row_ptr [n + 1], start [n]) -- row i of
        the result is tables[side].cols[start[i] : start[i] + row_ptr[i + 1] - row_ptr[i]]; a key without facts (an id
        beyond the indexed range included) gets an empty row."""
        tab = self.tables[side]
        keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
        inside = (keys >= 0).all(axis=1) & (keys < self.span).all(axis=1)
        want = np.where(inside, keys[:, 0] * self.span + keys[:, 1], -1)
        pos = np.minimum(np.searchsorted(tab.codes, want), max(len(tab.codes) - 1, 0))
        hit = (tab.codes[pos] == want) if len(tab.codes) else np.zeros(len(want), dtype=bool)
        start = np.where(hit, tab.ptr[pos], 0)
        count = np.where(hit, tab.ptr[np.minimum(pos + 1, len(tab.ptr) - 1)] - start, 0)
        return np.concatenate(([0], np.cumsum(count))).astype(np.int64), start.astype(np.int64)

    def lists_host(self, side, keys):
        """(row_ptr [n + 1], cols [nnz]) of the query on the host (tests, tools)."""
        row_ptr, start = self.lookup_host(side, keys)
        return row_ptr, self.tables[side].cols[G.ragged_arange(start, np.diff(row_ptr))]

    def resident(self, side, device):
        key = (side, str(device))
        cols = self._dev.get(key)
        if cols is None:
            cols = self._dev[key] = torch.from_numpy(self.tables[side].cols).to(device)
        return cols

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
