"""CPU tests of the host side of the open-query forecasts: preprocess.HistoryIndex.lookup (the history window of an
arbitrary (entity, as_of) pair -- the host statement of renet_query_histories) against the index's own windows and against
a brute-force scan of the quadruple array, ObservedStream.horizon_as_of, ObservedStream.extended, and the binding."""
import numpy as np
import pytest

import observed_stream as S


@pytest.fixture(scope='module')
def obs():
    import preprocess as P
    splits = S.make()
    S.check_cases(*splits)
    return P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)


def _window(h, first, count):
    """The snapshots [first, first + count) of a history index as [(t, sorted neighbours)]."""
    return [(int(h.snap_t[k]), sorted(h.nbr_o[h.snap_ptr[k]:h.snap_ptr[k + 1]].tolist())) for k in range(first, first + count)]


def _brute(allq, ent_col, other_col, e, as_of, history_len):
    """The same by a scan of the quadruples: the last history_len active timestamps < as_of of entity e in that role."""
    m = (allq[:, ent_col] == e) & (allq[:, 3] < as_of)
    ts = np.unique(allq[m, 3])[-history_len:] if history_len else []
    return [(int(t), sorted(allq[m & (allq[:, 3] == t), other_col].tolist())) for t in ts]


@pytest.mark.parametrize('history_len', [S.SEQ_LEN, 10, 1])
def test_lookup_reproduces_the_index_and_a_brute_force_scan(history_len):
    import preprocess as P
    allq = np.concatenate(S.make())
    for role, ec, oc in (('s', 0, 2), ('o', 2, 0)):
        h = P.HistoryIndex(allq, role, history_len, S.NUM_ENT)
        assert h.ent_ptr.shape == (S.NUM_ENT + 1,) and h.ent_ptr[0] == 0 and h.ent_ptr[-1] == len(h.snap_t)
        assert np.all(np.diff(h.ent_ptr) >= 0)
        for e in range(S.NUM_ENT):
            assert np.all(h.snap_ent[h.ent_ptr[e]:h.ent_ptr[e + 1]] == e)
        # the stream's own facts
        first, count = h.lookup(allq[:, ec], allq[:, 3])
        assert first.dtype == count.dtype == np.int64
        assert np.array_equal(first, h.first) and np.array_equal(count, h.count)
        # every (entity, as_of), entities -1 and NUM_ENT included
        ents = np.repeat(np.arange(-1, S.NUM_ENT + 1), S.NUM_T + 3)
        as_of = np.tile(np.arange(-1, S.NUM_T + 2), S.NUM_ENT + 2)
        first, count = h.lookup(ents, as_of)
        for e, a, f, c in zip(ents.tolist(), as_of.tolist(), first.tolist(), count.tolist()):
            if e < 0 or e >= S.NUM_ENT:
                assert (f, c) == (0, 0)
                continue
            assert 0 <= c <= history_len and h.ent_ptr[e] <= f and f + c <= h.ent_ptr[e + 1]
            assert _window(h, f, c) == _brute(allq, ec, oc, e, a, history_len), (role, e, a)
        # (a): the entity that first appears at t = 21 has no history up to then
        late = h.lookup(np.full(23, S.NEW_ENT), np.arange(-1, 22))
        assert not late[1].any()
        # a scalar as_of broadcasts
        f1, c1 = h.lookup(np.arange(S.NUM_ENT), 12)
        f2, c2 = h.lookup(np.arange(S.NUM_ENT), np.full(S.NUM_ENT, 12))
        assert np.array_equal(f1, f2) and np.array_equal(c1, c2)


def test_lookup_on_an_index_without_num_ent_and_on_an_empty_one():
    import preprocess as P
    allq = np.concatenate(S.make())
    h = P.HistoryIndex(allq, 's', 3)                          # num_ent = max subject id + 1
    assert h.num_ent == int(allq[:, 0].max()) + 1 and len(h.ent_ptr) == h.num_ent + 1
    assert np.array_equal(h.lookup(allq[:, 0], allq[:, 3])[0], h.first)
    assert [x.tolist() for x in h.lookup([h.num_ent], [5])] == [[0], [0]]
    e = P.HistoryIndex(np.zeros((0, 4), dtype=np.int64), 's', 3, 4)
    f, c = e.lookup([0, 3, -1, 4], [0, 7, 1, 1])
    assert not f.any() and not c.any()
    with pytest.raises(ValueError):
        P.HistoryIndex(allq, 's', 3, num_ent=5)


def test_horizon_as_of(obs):
    test, valid = obs.positions('test'), obs.positions('valid')
    t = obs.allq[test, 3]
    assert sorted(set(t.tolist())) == [20, 21, 22, 23]
    assert np.array_equal(obs.horizon_as_of(test, 1), t)
    both = np.concatenate((valid, test))
    assert np.array_equal(obs.horizon_as_of(both, 1), obs.allq[both, 3])
    got = obs.horizon_as_of(test, 3)
    assert got.dtype == np.int64
    for tt, want in ((20, 20), (21, 20), (22, 20), (23, 23)):
        assert np.all(got[t == tt] == want)
    assert np.all(obs.horizon_as_of(test, 9) == 20)
    # valid + test from the valid split's first timestamp: blocks 16-18, 19-21, 22-23
    got = obs.horizon_as_of(both, 3)
    tb = obs.allq[both, 3]
    assert np.array_equal(got, 16 + 3 * ((tb - 16) // 3))
    # an explicit start
    got = obs.horizon_as_of(test, 2, start=19)
    assert np.array_equal(got, np.where(t == 20, 19, np.where(t <= 22, 21, 23)))
    for h in (1, 2, 3, 4, 9):
        assert np.all(obs.horizon_as_of(both, h) <= tb)
    with pytest.raises(ValueError):
        obs.horizon_as_of(test, 0)
    with pytest.raises(ValueError):
        obs.horizon_as_of(valid, 2, start=18)


def _same_index(a, b):
    for f in ('first', 'count', 'snap_t', 'snap_ent', 'snap_ptr', 'nbr_r', 'nbr_o', 'ent_ptr'):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.history_len == b.history_len and a.num_ent == b.num_ent


def test_extended_equals_the_stream_built_from_the_concatenation(obs):
    import preprocess as P
    tr, va, te = S.make()
    new = np.array([[0, 1, 2, 23], [S.NEW_ENT, 0, 3, 24], [4, 4, 4, 24], [0, 1, 9, 26]], dtype=np.int64)
    ext = obs.extended(new)
    want = P.ObservedStream((tr, va, np.concatenate((te, new))), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    assert ext is not obs and len(obs) == len(tr) + len(va) + len(te)            # the stream itself is unchanged
    assert np.array_equal(ext.allq, want.allq) and ext.ranges == want.ranges
    assert ext.ranges['test'] == (len(tr) + len(va), len(tr) + len(va) + len(te) + 4)
    assert np.array_equal(ext.times, want.times) and ext.times[-1] == 26
    _same_index(ext.hist_s, want.hist_s)
    _same_index(ext.hist_o, want.hist_o)
    assert list(ext.graph_dict.keys()) == list(want.graph_dict.keys())
    for k in want.graph_dict:
        for f in ('ent', 'ls', 'r', 'lo'):
            assert np.array_equal(getattr(ext.graph_dict[k], f), getattr(want.graph_dict[k], f))
    assert (ext.num_ent, ext.num_rels, ext.history_len) == (obs.num_ent, obs.num_rels, obs.history_len)
    # a stream without a valid split keeps its two splits
    two = P.ObservedStream((tr, None, te), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN).extended(new)
    assert sorted(two.ranges) == ['test', 'train'] and np.array_equal(two.allq, np.concatenate((tr, te, new)))
    with pytest.raises(ValueError):
        obs.extended(np.array([[0, 1, 2, 22]]))                                 # earlier than the stream's end
    with pytest.raises(ValueError):
        obs.extended(np.array([[0, 1, 2, 25], [0, 1, 2, 24]]))                  # not sorted
    with pytest.raises(ValueError):
        obs.extended(np.array([[S.NUM_ENT, 1, 2, 24]]))


def test_binding_and_entry_points_are_attached():
    import ctypes
    import gpu_builder as GB
    import model as M
    import renet_hip as K
    assert 'renet_query_histories' in K.EXPORTS
    restype, argtypes = K._SIGNATURES['renet_query_histories']
    assert restype is ctypes.c_int and len(argtypes) == 12
    for name in ('forecast_scores', 'forecast_topk', 'evaluate_forecast', 'forecast_events'):
        assert callable(getattr(M.RENet, name))
    assert issubclass(GB.QueryStore, GB.ListBatchStore) and callable(GB.ObservedStore.queries)
