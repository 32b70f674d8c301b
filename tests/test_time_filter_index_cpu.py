"""CPU tests of the host side of the three-setting evaluation (raw, filtered, time-aware filtered): the time-aware tables of
filter_index.FilterIndex and its range lookups against a brute-force dictionary, the refusals, the C ABI entry of
renet_rank_rows3 in the header / binding / build list, and evaluate_time_filter's id selection."""
import os

import numpy as np
import pytest
import torch

from helpers import ROOT

TIMES = (0, 24, 48)
SIDE_COLS = {'o': (0, 1, 2), 's': (2, 1, 0)}


def _facts():
    """all_triplets [m, 4] over entities 0..8 / relations 0..2: 70 random (s, r, o), each at a random non-empty subset of
    TIMES (the same triple at several timestamps), exact duplicate quadruples inside one timestamp, and (7, 2, 8), the only
    fact of the keys (7, 2) / (8, 2), at t = 0 and 24 but not at 48 (a key present only at other times)."""
    rng = np.random.RandomState(11)
    base = np.stack((rng.randint(0, 6, 70), rng.randint(0, 2, 70), rng.randint(0, 6, 70)), axis=1)
    rows = []
    for f in base:
        when = [t for t in TIMES if rng.rand() < 0.5] or [TIMES[rng.randint(3)]]
        rows += [[f[0], f[1], f[2], t] for t in when]
    rows += rows[:12]                                                       # exact duplicates
    rows += [[7, 2, 8, 0], [7, 2, 8, 24]]
    at = np.asarray(rows, dtype=np.int64)
    return at[rng.permutation(len(at))]


def _brute(at, side):
    k0, k1, v = SIDE_COLS[side]
    timed, untimed = {}, {}
    for q in at.tolist():
        timed.setdefault((q[k0], q[k1], q[3]), set()).add(q[v])
        untimed.setdefault((q[k0], q[k1]), set()).add(q[v])
    return timed, untimed


def _queries():
    """Every (id, relation, time) of a grid that reaches past the facts on all sides: negative ids, ids >= span (span is
    10 here: 8 + 2), relations without facts, a negative and an unseen timestamp (72), and a far id."""
    grid = np.stack(np.meshgrid(np.arange(-1, 12), np.arange(-1, 4), np.array([-5, 0, 24, 48, 72, 12]), indexing='ij'),
                    axis=-1).reshape(-1, 3)
    return np.concatenate((grid, grid[:5], [[40, 1, 0], [7, 2, 48], [7, 2, 0], [8, 2, 24], [2 ** 40, 0, 0]])).astype(np.int64)


@pytest.mark.parametrize('as_tensor', [False, True])
def test_timed_tables_equal_a_brute_force_dictionary(as_tensor):
    import filter_index as FI
    at = _facts()
    assert len(np.unique(at, axis=0)) < len(at)                             # duplicates are in
    idx = FI.FilterIndex(torch.from_numpy(at) if as_tensor else at)
    assert idx.span == 10
    keys = _queries()
    for side in ('o', 's'):
        timed, _ = _brute(at, side)
        start, count = idx.ranges_host(side, keys)
        cols = idx.timed_table(side).cols
        assert cols.dtype == np.int32 and start.shape == count.shape == (len(keys),)
        got = [cols[a:a + c].tolist() for a, c in zip(start.tolist(), count.tolist())]
        want = [sorted(timed.get(tuple(k), ())) for k in keys.tolist()]
        assert got == want
        assert sum(len(w) > 1 for w in want) > 5 and sum(len(w) == 0 for w in want) > 5
        # every key of the dictionary was asked for, and every stored list belongs to one
        assert set(timed) <= set(map(tuple, keys.tolist()))
        assert len(cols) == sum(len(v) for v in timed.values())
    # present at t = 0 and 24 only
    a, c = idx.ranges_host('o', np.array([[7, 2, 0], [7, 2, 24], [7, 2, 48], [7, 2, 72]]))
    assert c.tolist() == [1, 1, 0, 0] and idx.timed_table('o').cols[a[0]] == 8
    a, c = idx.ranges_host('s', np.array([[8, 2, 24], [8, 2, 48]]))
    assert c.tolist() == [1, 0] and idx.timed_table('s').cols[a[0]] == 7
    # no query at all
    a, c = idx.ranges_host('o', np.zeros((0, 3), dtype=np.int64))
    assert len(a) == 0 and len(c) == 0


def test_time_aware_list_is_a_subset_of_the_time_agnostic_one():
    import filter_index as FI
    at = _facts()
    idx = FI.FilterIndex(at)
    strict = 0
    for side, (k0, k1, v) in SIDE_COLS.items():
        st, ct = idx.ranges_host(side, at[:, [k0, k1, 3]])
        sa, ca = idx.ranges_host(side, at[:, [k0, k1]])
        tcols, acols = idx.timed_table(side).cols, idx.tables[side].cols
        for i in range(len(at)):
            aware, agnostic = set(tcols[st[i]:st[i] + ct[i]].tolist()), set(acols[sa[i]:sa[i] + ca[i]].tolist())
            assert at[i, v] in aware and aware <= agnostic
            strict += aware < agnostic
    assert strict > 0


def test_two_column_ranges_address_the_lists_of_lists_host():
    import filter_index as FI
    at = _facts()
    idx = FI.FilterIndex(at)
    keys = np.unique(_queries()[:, :2], axis=0)
    for side in ('o', 's'):
        _, untimed = _brute(at, side)
        start, count = idx.ranges_host(side, keys)
        row_ptr, cols = idx.lists_host(side, keys)
        assert np.array_equal(np.diff(row_ptr), count)
        table = idx.tables[side].cols
        for i, k in enumerate(keys.tolist()):
            mine = table[start[i]:start[i] + count[i]].tolist()
            assert mine == cols[row_ptr[i]:row_ptr[i + 1]].tolist() == sorted(untimed.get(tuple(k), ()))
        # lookup_host keeps its result: (row_ptr, start)
        rp, st = idx.lookup_host(side, keys)
        assert np.array_equal(rp, row_ptr) and np.array_equal(st, start) and rp.dtype == st.dtype == np.int64


def test_combined_lookup_equals_the_two_lookups():
    """ranges_both_host (one sort of the queries for both tables) on queries of mixed timestamps in no order."""
    import filter_index as FI
    at = _facts()
    idx = FI.FilterIndex(at)
    keys = _queries()
    keys = keys[np.random.RandomState(2).permutation(len(keys))]
    for side in ('o', 's'):
        sa, ca, st, ct = idx.ranges_both_host(side, keys)
        for got, want in zip((sa, ca), idx.ranges_host(side, keys[:, :2])):
            assert np.array_equal(got, want) and got.dtype == np.int64
        for got, want in zip((st, ct), idx.ranges_host(side, keys)):
            assert np.array_equal(got, want) and got.dtype == np.int64
        assert ct.sum() > 0 and np.all(ct <= ca)
    assert all(len(x) == 0 for x in idx.ranges_both_host('o', np.zeros((0, 3), dtype=np.int64)))


def test_refusals_and_empty_facts():
    import filter_index as FI
    at3 = _facts()[:, :3]
    idx = FI.FilterIndex(at3)
    with pytest.raises(ValueError):
        idx.ranges_host('o', np.array([[7, 2, 0]]))
    with pytest.raises(ValueError):
        idx.timed_table('s')
    with pytest.raises(ValueError):
        idx.ranges_both_host('s', np.array([[8, 2, 0]]))
    assert idx.lists_host('o', np.array([[7, 2]]))[1].tolist() == [8]       # the untimed tables are still served
    assert idx.ranges_host('s', np.array([[8, 2]]))[1].tolist() == [1]
    empty = FI.FilterIndex(np.zeros((0, 4), dtype=np.int64))
    for keys in (np.array([[0, 0, 0], [3, 1, 24]]), np.array([[0, 0], [3, 1]])):
        start, count = empty.ranges_host('s', keys)
        assert start.tolist() == [0, 0] and count.tolist() == [0, 0]
    assert len(empty.timed_table('o').cols) == 0


def test_key_codes_that_would_not_fit_int64_are_refused():
    import filter_index as FI
    big = 2 ** 31 - 2                                                       # span 2^31: span^2 * 2 timestamps = 2^63
    idx = FI.FilterIndex(np.array([[big, 0, 1, 0], [big, 0, 2, 5]], dtype=np.int64))
    assert idx.lists_host('o', np.array([[big, 0]]))[1].tolist() == [1, 2]
    with pytest.raises(ValueError):
        idx.ranges_host('o', np.array([[big, 0, 5]]))
    one = FI.FilterIndex(np.array([[big, 0, 1, 7], [big, 0, 2, 7]], dtype=np.int64))      # one timestamp: 2^62 fits
    start, count = one.ranges_host('o', np.array([[big, 0, 7], [big, 0, 8], [big, big + 1, 7]]))
    assert count.tolist() == [2, 0, 0] and one.timed_table('o').cols[start[0]:start[0] + 2].tolist() == [1, 2]
    # timestamps far apart are rank-compressed, not multiplied in
    far = FI.FilterIndex(np.array([[3, 0, 1, -2 ** 40], [3, 0, 2, 2 ** 50]], dtype=np.int64))
    assert far.ranges_host('o', np.array([[3, 0, 2 ** 50], [3, 0, 0]]))[1].tolist() == [1, 0]


def test_rank3_entry_is_declared_bound_and_built():
    import build
    import renet_hip as K
    hdr = open(os.path.join(ROOT, 'include', 'renet_hip.h')).read()
    assert 'int renet_rank_rows3(const float* scores, int ld, int n, int C, const int32_t* label,' in hdr
    assert 'renet_rank_rows3' in K.EXPORTS
    restype, argtypes = K._SIGNATURES['renet_rank_rows3']
    assert len(argtypes) == 16                                              # full argtypes: the stream handle is the last
    src = [s for s in build.sources() if os.path.basename(s) == 'rank.hip']
    assert len(src) == 1 and 'int renet_rank_rows3(' in open(src[0]).read()
    assert callable(K.rank_rows3)


@pytest.mark.parametrize('as_tensor', [False, True])
def test_evaluate_time_filter_selects_the_ids_of_the_querys_own_timestamp(as_tensor):
    """(1, 0, ?) holds for objects {2, 3} at t = 0 and {3, 4} at t = 24; (?, 0, 3) for subjects {1, 5} at t = 0 and {1} at
    t = 24.  Another relation and another subject at the same times must not leak in."""
    import model as M
    at = np.array([[1, 0, 2, 0], [1, 0, 3, 0], [5, 0, 3, 0], [1, 1, 6, 0], [2, 0, 7, 0],
                   [1, 0, 3, 24], [1, 0, 4, 24], [1, 0, 4, 24], [6, 1, 3, 24]], dtype=np.int64)
    at = torch.from_numpy(at) if as_tensor else at
    ids = lambda x: sorted(np.asarray(x).tolist())
    ob, sub = M._time_aware_ids(at, 1, 0, 3, 0)
    assert ids(ob) == [2, 3] and ids(sub) == [1, 5]
    ob, sub = M._time_aware_ids(at, 1, 0, 3, 24)
    assert ids(ob) == [3, 4, 4] and ids(sub) == [1]
    ob, sub = M._time_aware_ids(at, 1, 0, 3, 48)                           # a timestamp without facts
    assert ids(ob) == [] and ids(sub) == []
    for name in ('evaluate_time_filter', 'evaluate_all_batch', 'evaluate_all_stream'):
        assert callable(getattr(M.RENet, name))
