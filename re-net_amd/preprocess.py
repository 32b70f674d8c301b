"""DGL-free, vectorised replacement of the offline preprocessing (reference
data/<DS>/get_history_graph.py:111-317): per-timestamp graphs + rolling per-entity histories.

The reference materialises, for every quadruple, a Python list of <= history_len numpy arrays (and
re-pickles them per split).  Here the stream is indexed ONCE into a snapshot table:

  snapshot = all facts of one (entity, timestamp) pair, in file order      (the s_his_cache rows)
  snapshots of one entity are contiguous and time-ordered

and the history of quadruple i is just a RANGE of snapshot ids
  [ max(first snapshot of its entity, sid_i - history_len), sid_i )
so nothing is duplicated, `history_len` is a parameter (the seq_len=15 config needs 15, the
reference hard-codes 10 at get_history_graph.py:118), and a batch's FlatHistory is two ragged
gathers.  Semantics match the reference's streaming loop: a history holds the last <= history_len
PREVIOUS timestamps (t' < t) in which the entity was active in that role, across train -> valid ->
test in file order (the rolling state carried at :206-317).
"""
import numpy as np

from graph import FlatHistory, ragged_arange, TimeGraph


class HistoryIndex(object):
    """Histories of every quadruple of a (time-sorted) stream for one role ('s': subject histories of
    (r, o) rows; 'o': object histories of (r, s) rows)."""

    def __init__(self, quads, role, history_len=10, num_ent=None):
        quads = np.asarray(quads, dtype=np.int64)
        if len(quads) > 1 and np.any(np.diff(quads[:, 3]) < 0):
            raise ValueError('quadruples must be sorted by time (as the dataset files are)')
        n = len(quads)
        ent = quads[:, 0] if role == 's' else quads[:, 2]
        other = quads[:, 2] if role == 's' else quads[:, 0]
        order = np.lexsort((np.arange(n), quads[:, 3], ent))          # entity, then time, then file order
        e_s, t_s = ent[order], quads[order, 3]
        new = np.ones(n, dtype=bool)
        if n:
            new[1:] = (e_s[1:] != e_s[:-1]) | (t_s[1:] != t_s[:-1])
        starts = np.nonzero(new)[0]
        self.snap_t = t_s[starts]
        self.snap_ent = e_s[starts]
        self.snap_ptr = np.concatenate((starts, [n])).astype(np.int64)
        self.nbr_r = quads[order, 1]
        self.nbr_o = other[order]
        sid_sorted = np.cumsum(new) - 1                                  # snapshot id of each sorted fact
        sid = np.empty(n, dtype=np.int64)
        sid[order] = sid_sorted
        # first snapshot of the entity owning each snapshot
        ent_new = np.ones(len(starts), dtype=bool)
        if len(starts):
            ent_new[1:] = self.snap_ent[1:] != self.snap_ent[:-1]
        first_of_ent = np.maximum.accumulate(np.where(ent_new, np.arange(len(starts)), 0))
        lo = np.maximum(first_of_ent[sid], sid - history_len)
        self.first = lo
        self.count = sid - lo
        self.history_len = history_len
        self.role = role
        # the snapshot range of every entity, [ent_ptr[e], ent_ptr[e + 1]) (empty for an entity without snapshots): what
        # lookup() and the device's renet_query_histories search
        self.num_ent = int(num_ent) if num_ent is not None else (int(ent.max()) + 1 if n else 0)
        if n and (int(ent.min()) < 0 or int(ent.max()) >= self.num_ent):
            raise ValueError('entity id outside [0, num_ent)')
        self.ent_ptr = np.searchsorted(self.snap_ent, np.arange(self.num_ent + 1)).astype(np.int64)

    def __len__(self):
        return len(self.first)

    def appended(self, ent_old, new_quads):
        """The index of the stream with new_quads [m, 4] APPENDED, from this index's six resident fields (first, count,
        snap_t, snap_ptr, nbr_o, ent_ptr), ent_old [n] (this role's entity of every old quadruple) and the new quadruples
        alone: no sort over the old facts.  The host statement of the device append (csrc/builder_append.hip,
        renet_store_append), array for array; equal to HistoryIndex(old ++ new) in those six fields (and in snap_ent, which
        follows from ent_ptr; nbr_r is not carried: to_lists() needs a full index).

        New facts have t >= every old fact (ValueError otherwise) and come later in file order, so in the (entity, time,
        file order) sort they land at the END of their entity's run.  With the new facts sorted the same way: add_fact[e]
        = new facts of e, add_snap[e] = distinct new times of e, minus one if the first of them is e's last old snap_t (those
        facts JOIN that snapshot); fshift / sshift = their exclusive scans over the entities.  Then ent_ptr' = ent_ptr +
        sshift, old snapshot k of e moves to k + sshift[e], the old fact run of e moves by fshift[e] and e's new facts follow
        it, snap_ptr' is the scan of the merged snapshot sizes; an old quadruple keeps count and has first + sshift[its
        entity]; a new one with snapshot id sid has first = max(ent_ptr'[e], sid - history_len), count = sid - first."""
        q = np.asarray(new_quads, dtype=np.int64).reshape(-1, 4)
        ent_old = np.asarray(ent_old, dtype=np.int64).reshape(-1)
        m, n, N, S = len(q), len(self.first), self.num_ent, len(self.snap_t)
        if len(ent_old) != n:
            raise ValueError('ent_old must hold the entity of every old quadruple')
        if m and (np.any(np.diff(q[:, 3]) < 0) or (S and q[0, 3] < self.snap_t.max())):
            raise ValueError('appended quadruples must be sorted by time and not earlier than the end of the stream')
        ent = q[:, 0] if self.role == 's' else q[:, 2]
        other = q[:, 2] if self.role == 's' else q[:, 0]
        if m and (int(ent.min()) < 0 or int(ent.max()) >= N):
            raise ValueError('entity id outside [0, num_ent)')
        order = np.lexsort((np.arange(m), q[:, 3], ent))              # entity, then time, then input order
        e_s, t_s = ent[order], q[order, 3]
        head_e = np.ones(m, dtype=bool)
        head_e[1:] = e_s[1:] != e_s[:-1]
        head_s = head_e.copy()
        head_s[1:] |= t_s[1:] != t_s[:-1]
        old_cnt = np.diff(self.ent_ptr)
        join = np.zeros(m, dtype=bool)
        cand = head_e & (old_cnt[e_s] > 0)                              # entity heads with an old snapshot to join
        join[cand] = self.snap_t[self.ent_ptr[e_s[cand] + 1] - 1] == t_s[cand]
        opens = head_s & ~join
        add_fact = np.bincount(e_s, minlength=N)
        add_snap = np.bincount(e_s[opens], minlength=N)
        fshift = np.concatenate(([0], np.cumsum(add_fact))).astype(np.int64)
        sshift = np.concatenate(([0], np.cumsum(add_snap))).astype(np.int64)
        ent_ptr2 = self.ent_ptr + sshift
        S2 = S + int(sshift[-1])
        snap_ent_old = np.repeat(np.arange(N, dtype=np.int64), old_cnt)
        # snapshot id of every sorted new fact: the snapshots its entity opened up to it, behind the entity's old ones
        oinc = np.cumsum(opens)
        rank = oinc - (oinc - opens)[fshift[e_s]] if m else oinc
        sid = ent_ptr2[e_s + 1] - add_snap[e_s] + rank - 1
        snap_t2 = np.empty(S2, dtype=np.int64)
        size2 = np.zeros(S2, dtype=np.int64)
        old_to = np.arange(S, dtype=np.int64) + sshift[snap_ent_old]
        snap_t2[old_to] = self.snap_t
        size2[old_to] = np.diff(self.snap_ptr)
        snap_t2[sid[opens]] = t_s[opens]
        np.add.at(size2, sid, 1)
        nbr2 = np.empty(n + m, dtype=np.int64)
        nbr2[np.arange(n, dtype=np.int64) + fshift[np.repeat(snap_ent_old, np.diff(self.snap_ptr))]] = self.nbr_o
        nbr2[self.snap_ptr[self.ent_ptr[e_s + 1]] + np.arange(m, dtype=np.int64)] = other[order]
        first2, count2 = np.empty(n + m, dtype=np.int64), np.empty(n + m, dtype=np.int64)
        first2[:n], count2[:n] = self.first + sshift[ent_old], self.count
        lo = np.maximum(ent_ptr2[e_s], sid - self.history_len)
        first2[n + order], count2[n + order] = lo, sid - lo
        out = HistoryIndex.__new__(HistoryIndex)
        out.first, out.count, out.snap_t, out.nbr_o, out.ent_ptr = first2, count2, snap_t2, nbr2, ent_ptr2
        out.snap_ptr = np.concatenate(([0], np.cumsum(size2))).astype(np.int64)
        out.snap_ent = np.repeat(np.arange(N, dtype=np.int64), np.diff(ent_ptr2))
        out.nbr_r = None
        out.history_len, out.role, out.num_ent = self.history_len, self.role, N
        return out

    def lookup(self, ent, as_of):
        """(first, count) int64 of the history window of ARBITRARY (entity, as_of) pairs: the last <= history_len snapshots
        of the entity in this role with snap_t < as_of, as the range [first, first + count) of the snapshot table.  With sid
        the first snapshot of the entity's range whose snap_t >= as_of: first = max(range start, sid - history_len), count =
        sid - first.  An entity id < 0 or >= num_ent gives (0, 0) -- how an absent side is expressed.  For the stream's own
        facts lookup(ent_i, t_i) = (first[i], count[i])."""
        ent = np.asarray(ent, dtype=np.int64).reshape(-1)
        as_of = np.broadcast_to(np.asarray(as_of, dtype=np.int64), ent.shape)
        ok = (ent >= 0) & (ent < self.num_ent)
        e = np.where(ok, ent, 0)
        # snapshots are sorted by (entity, time): ONE search over the combined key; as_of clipped into the key's time digit
        t0 = int(self.snap_t.min()) if len(self.snap_t) else 0
        span = (int(self.snap_t.max()) if len(self.snap_t) else 0) - t0 + 2
        sid = np.searchsorted(self.snap_ent * span + (self.snap_t - t0), e * span + np.clip(as_of - t0, 0, span - 1))
        lo = self.ent_ptr[e] if self.num_ent else np.zeros_like(e)
        first = np.maximum(lo, sid - self.history_len)
        return np.where(ok, first, 0), np.where(ok, sid - first, 0)

    def take(self, idx, max_len=None):
        """FlatHistory of the quadruples `idx` (optionally keeping only the newest max_len steps)."""
        idx = np.asarray(idx, dtype=np.int64)
        cnt = self.count[idx]
        first = self.first[idx]
        if max_len is not None:
            cut = np.maximum(cnt - max_len, 0)
            first, cnt = first + cut, cnt - cut
        steps = ragged_arange(first, cnt)
        ncnt = self.snap_ptr[steps + 1] - self.snap_ptr[steps]
        nb = ragged_arange(self.snap_ptr[steps], ncnt)
        return FlatHistory(np.concatenate(([0], np.cumsum(cnt))), self.snap_t[steps],
                           np.concatenate(([0], np.cumsum(ncnt))), self.nbr_o[nb])

    def to_lists(self, idx):
        """The reference's nested layout for quadruples `idx`: (hist, hist_t) with hist[i] a list of
        int arrays [k, 2] = (r, o) -- what train_history_sub.txt / *_ob.txt unpickle to."""
        hist, hist_t = [], []
        for i in np.asarray(idx, dtype=np.int64):
            h, ht = [], []
            for k in range(self.first[i], self.first[i] + self.count[i]):
                a, b = self.snap_ptr[k], self.snap_ptr[k + 1]
                h.append(np.stack((self.nbr_r[a:b], self.nbr_o[a:b]), axis=1))
                ht.append(int(self.snap_t[k]))
            hist.append(h)
            hist_t.append(ht)
        return hist, hist_t


def _role_index(role):
    """0 / 's': the entity is the subject, the partner the object; 1 / 'o': the other way round."""
    if role in (0, 's'):
        return 0
    if role in (1, 'o'):
        return 1
    raise ValueError("role must be 0 / 's' or 1 / 'o'")


class PairIndex(object):
    """The RELATION-KEYED view of one role's facts, for the recurrence prior ("what did (entity, relation) connect to
    before, how often, how recently"): p_rel, p_other (the partner: o for role 0 / 's', s for role 1 / 'o') and p_t over
    ALL facts, sorted by (entity, relation, partner, time).  The fact run of entity e is [run_ptr[e], run_ptr[e + 1]) --
    the same index range as in the HistoryIndex of that role, run_ptr = snap_ptr[ent_ptr]; the resident copy keeps no
    pointer array of its own.  Duplicate quadruples stay and count as facts.  Equal keys are indistinguishable in the three
    arrays, so the tables are a function of the MULTISET of facts: no file-order tie rule exists.  The host statement of
    the resident pair tables (gpu_builder.ObservedStore.pair_tables), of renet_pair_append (appended) and, with
    tests/recurrence_statement.py, of renet_recurrence_mix_rows (prior_rows)."""

    def __init__(self, quads, role, num_ent):
        q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
        self.role, self.num_ent = _role_index(role), int(num_ent)
        ent, other = (q[:, 0], q[:, 2]) if self.role == 0 else (q[:, 2], q[:, 0])
        if len(q) and (int(ent.min()) < 0 or int(ent.max()) >= self.num_ent):
            raise ValueError('entity id outside [0, num_ent)')
        order = np.lexsort((q[:, 3], other, q[:, 1], ent))
        self.p_rel, self.p_other, self.p_t = q[order, 1], other[order], q[order, 3]
        self.run_ptr = np.searchsorted(ent[order], np.arange(self.num_ent + 1)).astype(np.int64)

    def __len__(self):
        return len(self.p_rel)

    def _keys_of(self, q):
        ent, other = (q[:, 0], q[:, 2]) if self.role == 0 else (q[:, 2], q[:, 0])
        return ent, q[:, 1], other, q[:, 3]

    def sorted_new(self, new_quads):
        """int64 [4, m] = (entity, relation, partner, time) of new_quads sorted by that key: what renet_pair_append takes."""
        q = np.asarray(new_quads, dtype=np.int64).reshape(-1, 4)
        ent, rel, other, t = self._keys_of(q)
        if len(q) and (int(ent.min()) < 0 or int(ent.max()) >= self.num_ent):
            raise ValueError('entity id outside [0, num_ent)')
        order = np.lexsort((t, other, rel, ent))
        return np.stack((ent[order], rel[order], other[order], t[order]))

    def appended(self, new_quads):
        """The tables of the stream with new_quads [m, 4] appended, WITHOUT a sort of the old facts: the host statement of
        renet_pair_append (csrc/recurrence.hip), rank by rank.  With the new facts of entity e sorted by key:
          old fact j of e's run  -> (new run start of e) + (j - old run start) + #{new facts of e with key <  key_j}
          i-th new fact of e     -> (new run start of e) + i                   + #{old facts of e with key <= key_i}
        Equal to PairIndex(old ++ new) array for array (the new facts may carry any timestamps: the tables hold no order
        between facts but the key's)."""
        ne, nr, no, nt = self.sorted_new(new_quads)
        n, m, N = len(self), len(ne), self.num_ent
        add = np.bincount(ne, minlength=N) if m else np.zeros(N, dtype=np.int64)
        new_ptr = np.concatenate(([0], np.cumsum(add))).astype(np.int64)      # the new facts of e: [new_ptr[e], new_ptr[e + 1])
        run2 = self.run_ptr + new_ptr
        out = PairIndex.__new__(PairIndex)
        out.role, out.num_ent, out.run_ptr = self.role, N, run2
        rel2, other2, t2 = (np.empty(n + m, dtype=np.int64) for _ in range(3))
        key_lt = lambda a, b: (a[0] < b[0]) or (a[0] == b[0] and (a[1] < b[1] or (a[1] == b[1] and a[2] < b[2])))
        old_ent = np.repeat(np.arange(N, dtype=np.int64), np.diff(self.run_ptr))
        for j in range(n):
            e = old_ent[j]
            key = (self.p_rel[j], self.p_other[j], self.p_t[j])
            lo, hi = new_ptr[e], new_ptr[e + 1]
            while lo < hi:                                                      # first new fact of e with key >= key_j
                mid = (lo + hi) // 2
                if key_lt((nr[mid], no[mid], nt[mid]), key):
                    lo = mid + 1
                else:
                    hi = mid
            p = run2[e] + (j - self.run_ptr[e]) + (lo - new_ptr[e])
            rel2[p], other2[p], t2[p] = key
        for i in range(m):
            e = ne[i]
            key = (nr[i], no[i], nt[i])
            lo, hi = self.run_ptr[e], self.run_ptr[e + 1]
            while lo < hi:                                                      # first old fact of e with key > key_i
                mid = (lo + hi) // 2
                if key_lt(key, (self.p_rel[mid], self.p_other[mid], self.p_t[mid])):
                    hi = mid
                else:
                    lo = mid + 1
            p = run2[e] + (i - new_ptr[e]) + (lo - self.run_ptr[e])
            rel2[p], other2[p], t2[p] = key
        out.p_rel, out.p_other, out.p_t = rel2, other2, t2
        return out

    def sub_run(self, ent, rel):
        """[a, b) of the facts of (ent, rel): two searches over p_rel inside the entity's run; (0, 0) for an entity outside
        [0, num_ent)."""
        if ent < 0 or ent >= self.num_ent:
            return 0, 0
        lo, hi = int(self.run_ptr[ent]), int(self.run_ptr[ent + 1])
        a = lo + int(np.searchsorted(self.p_rel[lo:hi], rel, side='left'))
        b = lo + int(np.searchsorted(self.p_rel[lo:hi], rel, side='right'))
        return a, b

    def prior_rows(self, ent, rel, t, as_of, half_life=None, inv_half_life=None):
        """The recurrence statistic of the queries (ent, rel, t) [n] with histories as of as_of (<= t): CSR lists (ptr int64
        [n + 1], col int64, w float64), row i holding, in ascending partner order, every partner o of a fact (ent_i, rel_i,
        o, t') with t' < as_of_i and w[o] = sum over those facts of 2^(-(t_i - t') * inv_half_life).  half_life None (or
        inv_half_life 0): plain counts.  inv_half_life, when given, is used as it stands (the device takes it as fp32:
        recurrence.RecurrencePrior.inv_half_life); else it is 1 / half_life.  An ARRAY inv_half_life holds one decay per row
        (a learned per-relation half-life: the host statement of renet_recurrence_mix_rows_decay); row i then equals the
        scalar call with inv_half_life[i], list for list."""
        ent, rel, t = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (ent, rel, t))
        as_of = np.broadcast_to(np.asarray(as_of, dtype=np.int64).reshape(-1), ent.shape)
        if inv_half_life is not None and np.ndim(inv_half_life) > 0:
            rates = np.asarray(inv_half_life, dtype=np.float64).reshape(-1)
            if rates.shape != ent.shape:
                raise ValueError('prior_rows: an array inv_half_life holds one value per row')
        else:
            rates = None
            ihl = float(inv_half_life) if inv_half_life is not None else (0.0 if half_life is None else 1.0 / float(half_life))
        ptr, col, w = [0], [], []
        for i in range(len(ent)):
            a, b = self.sub_run(int(ent[i]), int(rel[i]))
            seen = self.p_t[a:b] < as_of[i]
            o, tp = self.p_other[a:b][seen], self.p_t[a:b][seen]
            if rates is not None:
                ihl = float(rates[i])
            if len(o):
                cols, inv = np.unique(o, return_inverse=True)
                col.append(cols)
                w.append(np.bincount(inv, weights=np.exp2(-(t[i] - tp).astype(np.float64) * ihl), minlength=len(cols)))
            ptr.append(ptr[-1] + (len(col[-1]) if len(o) else 0))
        return (np.asarray(ptr, dtype=np.int64), np.concatenate(col) if col else np.zeros(0, dtype=np.int64),
                np.concatenate(w) if w else np.zeros(0, dtype=np.float64))

    def event_rows(self, ent, t, as_of, half_life=None, inv_half_life=None):
        """The JOINT recurrence statistic of the histories (ent, t) [n] as of as_of (<= t), every relation at once: CSR lists
        (ptr int64 [n + 1], rel int64, col int64, w float64), row i holding, in ascending (relation, partner) order, every
        pair (r, o) of a fact (ent_i, r, o, t') with t' < as_of_i and w[r, o] = sum over those facts of 2^(-(t_i - t') *
        inv_half_life).  The row's sum of w is the entity-wide W of renet_joint_mix_rows; restricted to one relation r the
        row is prior_rows(ent, r, ...)'s, list for list.  half_life / inv_half_life and every other convention as in
        prior_rows; an entity outside [0, num_ent) has an empty row.  The host statement, with
        tests/event_prior_statement.py, of renet_joint_mix_rows."""
        ent, t = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (ent, t))
        as_of = np.broadcast_to(np.asarray(as_of, dtype=np.int64).reshape(-1), ent.shape)
        ihl = float(inv_half_life) if inv_half_life is not None else (0.0 if half_life is None else 1.0 / float(half_life))
        ptr, rel, col, w = [0], [], [], []
        for i in range(len(ent)):
            a, b = (int(self.run_ptr[ent[i]]), int(self.run_ptr[ent[i] + 1])) if 0 <= ent[i] < self.num_ent else (0, 0)
            seen = self.p_t[a:b] < as_of[i]
            r, o, tp = self.p_rel[a:b][seen], self.p_other[a:b][seen], self.p_t[a:b][seen]
            n = 0
            if len(o):
                pairs, inv = np.unique(np.stack((r, o), axis=1), axis=0, return_inverse=True)      # ascending (relation, partner)
                n = len(pairs)
                rel.append(pairs[:, 0])
                col.append(pairs[:, 1])
                w.append(np.bincount(inv.reshape(-1), weights=np.exp2(-(t[i] - tp).astype(np.float64) * ihl), minlength=n))
            ptr.append(ptr[-1] + n)
        cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)
        return np.asarray(ptr, dtype=np.int64), cat(rel, np.int64), cat(col, np.int64), cat(w, np.float64)

    def prior_stats(self, ent, rel, t, as_of):
        """int64 [n, 2] = (distinct partners seen before as_of, facts counted) of every query: the integers
        renet_recurrence_mix_rows reports."""
        ptr, col, w = self.prior_rows(ent, rel, t, as_of)
        facts = [int(round(w[a:b].sum())) for a, b in zip(ptr[:-1], ptr[1:])]
        return np.stack((np.diff(ptr), np.asarray(facts, dtype=np.int64)), axis=1).reshape(-1, 2)


def build_graph_dict(quads, num_rels):
    """get_history_graph.py:137-140: {t: TimeGraph}, ascending time."""
    quads = np.asarray(quads, dtype=np.int64)
    order = np.argsort(quads[:, 3], kind='stable')
    q = quads[order]
    times, starts = np.unique(q[:, 3], return_index=True)
    ends = np.concatenate((starts[1:], [len(q)]))
    return {int(t): TimeGraph.from_triples(q[a:b, :3], num_rels) for t, a, b in zip(times, starts, ends)}


class ObservedStream(object):
    """A whole dataset as ONE observed stream, for the single-step (ground-truth history) evaluation protocol: at query
    time t every fact before t is known, the evaluated split's own included (model.RENet.evaluate_observed).

    splits: the time-ordered quadruple arrays train, valid, test in file order; valid may be None or left out (ICEWS14 has
    none).  Holds `allq` (the concatenation), `ranges` (split name -> [a, b) of positions in allq), the history index of
    both roles over the WHOLE stream -- the history of a test quadruple at t is the last <= history_len timestamps t' < t at
    which its entity was active in that role, with the true neighbours at t', whichever split they come from: what
    get_history_graph.py:206-317 writes into test_history_*.txt -- and `graph_dict`, one graph per timestamp of the whole
    stream (the reference writes the training timestamps only).  Host arrays only; resident() puts them on a device, and
    observe() appends newly observed quadruples to the resident copy."""

    def __init__(self, splits, num_ent, num_rels, history_len=10):
        splits = [np.asarray(q, dtype=np.int64).reshape(-1, 4) for q in splits if q is not None]
        if len(splits) not in (2, 3):
            raise ValueError('an observed stream is (train, valid, test) or (train, test)')
        names = ('train', 'valid', 'test') if len(splits) == 3 else ('train', 'test')
        self.num_ent, self.num_rels, self.history_len = int(num_ent), int(num_rels), int(history_len)
        self.allq = np.concatenate(splits)
        ends = np.cumsum([len(q) for q in splits])
        self.ranges = {name: (int(b - len(q)), int(b)) for name, q, b in zip(names, splits, ends)}
        self._hist = {'s': HistoryIndex(self.allq, 's', history_len, self.num_ent),   # (raises unless the stream is sorted by time)
                      'o': HistoryIndex(self.allq, 'o', history_len, self.num_ent)}
        self.graph_dict = build_graph_dict(self.allq, num_rels)
        self.times = np.unique(self.allq[:, 3])
        self.device = None                                              # the ObservedStore of the last resident() call

    def __len__(self):
        return len(self.allq)

    def _history(self, role):
        # a stream made by observe() has no host index until somebody asks: the device path reads the resident tables
        if self._hist[role] is None:
            self._hist[role] = HistoryIndex(self.allq, role, self.history_len, self.num_ent)
        return self._hist[role]

    hist_s = property(lambda self: self._history('s'))
    hist_o = property(lambda self: self._history('o'))

    def positions(self, split):
        """The stream positions of a split ('train', 'valid', 'test'), in file order."""
        return np.arange(*self.ranges[split])

    def horizon_as_of(self, idx, h, start=None):
        """Per stream position of idx, the as-of timestamp under horizon h (int64 [len]): the timestamps of the stream from
        `start` on (default: the first timestamp of the split that holds the first of the positions) are cut into blocks of
        h consecutive timestamps, and a position at t gets the FIRST timestamp of its block -- the model forecasts t knowing
        only the facts before it, up to h - 1 timestamps stale (RENet.evaluate_forecast(..., as_of=...)).  h = 1 gives t
        itself; the result is never > t.  ValueError for h < 1 or a position before `start`."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        h = int(h)
        if h < 1:
            raise ValueError('horizon must be >= 1')
        if len(idx) == 0:
            return np.zeros(0, dtype=np.int64)
        if idx.min() < 0 or idx.max() >= len(self.allq):
            raise ValueError('positions outside the stream')
        if start is None:
            a = max(a for a, b in self.ranges.values() if a <= idx.min() and a < b)
            start = self.allq[a, 3]
        ts = self.times[self.times >= int(start)]
        t = self.allq[idx, 3]
        if t.min() < int(start):
            raise ValueError('a position lies before the start of the horizon blocks')
        return ts[(np.searchsorted(ts, t) // h) * h]

    def extended(self, quads):
        """A NEW stream with the newly observed quadruples `quads` [m, 4] appended to the last split (they must be sorted
        by time and not earlier than the stream's last timestamp: ValueError).  A host rebuild of both history indices and
        the graphs; resident() is called again by the user.  (observe() gives the same resident stream without the rebuild: the
        "observe" half of a forecast / observe loop.)"""
        quads = self._checked_new(quads)
        names = [n for n in ('train', 'valid', 'test') if n in self.ranges]
        splits = [self.allq[slice(*self.ranges[n])] for n in names]
        splits[-1] = np.concatenate((splits[-1], quads))
        return ObservedStream(splits, self.num_ent, self.num_rels, self.history_len)

    def _checked_new(self, quads):
        """quads as int64 [m, 4], or the ValueError of extended()."""
        quads = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
        if len(quads) and ((len(self.allq) and quads[0, 3] < self.allq[-1, 3]) or np.any(np.diff(quads[:, 3]) < 0)):
            raise ValueError('appended quadruples must be sorted by time and not earlier than the end of the stream')
        if len(quads) and (quads[:, [0, 2]].min() < 0 or quads[:, [0, 2]].max() >= self.num_ent or quads[:, 1].min() < 0
                           or quads[:, 1].max() >= self.num_rels):
            raise ValueError('appended quadruples hold an entity / relation id outside the stream\'s range')
        return quads

    def _appended(self, quads):
        """The LIGHT stream of extended(quads), for the device append (gpu_builder.ObservedStore.appended): allq, ranges and
        times by concatenation; graph_dict a new dict that shares this stream's TimeGraph objects and adds -- for a timestamp
        equal to the last one, replaces -- only the appended timestamps' graphs; no history index (hist_s / hist_o are built
        when first read: nothing on the device path reads them).  quads must have passed _checked_new."""
        new = ObservedStream.__new__(ObservedStream)
        new.num_ent, new.num_rels, new.history_len = self.num_ent, self.num_rels, self.history_len
        new.allq = np.concatenate((self.allq, quads))
        last = [n for n in ('train', 'valid', 'test') if n in self.ranges][-1]
        new.ranges = dict(self.ranges)
        new.ranges[last] = (self.ranges[last][0], self.ranges[last][1] + len(quads))
        new._hist = {'s': None, 'o': None}
        new.graph_dict = dict(self.graph_dict)
        t_all = new.allq[:, 3]
        for t in np.unique(quads[:, 3]):                              # (ascending: the dict stays in time order)
            a, b = np.searchsorted(t_all, [t, t + 1])
            new.graph_dict[int(t)] = TimeGraph.from_triples(new.allq[a:b, :3], self.num_rels)
        new.times = np.asarray(list(new.graph_dict.keys()), dtype=np.int64)
        new.device = None
        return new

    def observe(self, quads, global_model):
        """extended(quads) + resident() WITHOUT the host rebuild: a new stream whose `device` is the resident store of this
        one with the quadruples appended on the device (gpu_builder.ObservedStore.appended: kernels over the resident tables,
        nothing but the new facts is uploaded).  Of the global-embedding table only the rows that can have changed are
        computed -- those of the timestamps >= the first appended one: the row of t_k is global_model.predict(t_{k+1}), the
        last one predict(last + time unit) (get_global_emb's own rule), and a row of an earlier timestamp reads no appended
        graph.  Needs an earlier resident() (ValueError); the old stream and its store stay valid.  Equal to
        extended(quads).resident(model, global_model) bit for bit, PROVIDED the global model's weights have not changed since
        the rows of the earlier timestamps were computed -- after a weight update call refresh_global() (or resident()) first."""
        import torch
        if self.device is None:
            raise ValueError('observe() appends to a resident stream: call resident() first')
        quads = self._checked_new(quads)
        new = self._appended(quads)
        rows = {}
        if len(quads):
            ts = [int(t) for t in new.times]
            unit = ts[1] - ts[0] if len(ts) > 1 else 1
            with torch.no_grad():
                for k, t in enumerate(ts):
                    if t >= quads[0, 3]:
                        nxt = ts[k + 1] if k + 1 < len(ts) else t + unit
                        rows[t] = global_model.predict(nxt, new.graph_dict)[0].detach()
        new.device = self.device.appended(quads, rows, _obs=new)
        return new

    def refresh_global(self, global_model):
        """After an update of the global model's weights: a NEW stream whose resident store shares every table of this one's
        (quadruples, history indices, graph store, filter index) but carries a new `glob`, recomputed batched on the device
        (online.global_table_batched: the RGCN layers once per timestamp instead of once per window position, one packed
        encoder launch per <= 1024 windows instead of one predict() per timestamp).  Keys and rows are those of
        global_table(global_model) -- rows to GEMM rounding, the batched GEMMs see other M -- so the result stands for
        resident() without the host rebuild and the upload.  Needs an earlier resident(); this stream and its store stay valid."""
        import online
        return online.refresh_global(self, global_model)

    def global_table(self, global_model):
        """{t: embedding} over ALL timestamps of the stream, from the global model as it stands and this stream's own
        graphs (global_model.py:57-73; no entry depends on a model prediction)."""
        import torch
        with torch.no_grad():
            return global_model.get_global_emb(self.times, self.graph_dict)

    def resident(self, model, global_model):
        """The stream on the model's device: a gpu_builder.ObservedStore (the DeviceStore of the whole stream plus the
        global-embedding table of its own, as a matrix).  Built anew at every call -- the table follows the global model's
        weights -- and kept in `device`, where RENet.observed_scores / evaluate_observed find it."""
        import gpu_builder
        self.device = gpu_builder.ObservedStore(self, self.global_table(global_model), model.h_dim, model.ent_embeds.device)
        return self.device


def write_reference_pickles(data_dir, history_len=10):
    """Command-line equivalent of running data/<DS>/get_history_graph.py in `data_dir`: reads stat.txt,
    train.txt, valid.txt (optional), test.txt and writes train_graphs.txt and
    {train,dev,test}_history_{sub,ob}.txt in the layout train.py:78-110 / test.py unpickle
    ([histories, timestamps] nested lists; graphs as graph.TimeGraph instead of DGLGraph)."""
    import os
    import pickle
    from utils import get_total_number, load_quadruples
    num_e, num_r = get_total_number(data_dir, 'stat.txt')
    splits = []
    for name, out in (('train.txt', 'train'), ('valid.txt', 'dev'), ('test.txt', 'test')):
        if os.path.isfile(os.path.join(data_dir, name)):
            splits.append((out, load_quadruples(data_dir, name)[0]))
    allq = np.concatenate([q for _, q in splits])
    hs, ho = HistoryIndex(allq, 's', history_len), HistoryIndex(allq, 'o', history_len)
    with open(os.path.join(data_dir, 'train_graphs.txt'), 'wb') as f:
        pickle.dump(build_graph_dict(splits[0][1], num_r), f)
    off = 0
    for out, q in splits:
        idx = np.arange(off, off + len(q))
        off += len(q)
        for tag, h in (('sub', hs), ('ob', ho)):
            with open(os.path.join(data_dir, '%s_history_%s.txt' % (out, tag)), 'wb') as f:
                pickle.dump(list(h.to_lists(idx)), f)


if __name__ == '__main__':
    import sys
    write_reference_pickles(sys.argv[1] if len(sys.argv) > 1 else '.',
                            int(sys.argv[2]) if len(sys.argv) > 2 else 10)
