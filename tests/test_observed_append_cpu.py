"""CPU tests of the host statement of the device append (preprocess.HistoryIndex.appended, ObservedStream._appended -- the
light stream behind ObservedStream.observe) against a full rebuild (HistoryIndex / ObservedStream.extended of the longer
stream) on the small stream of tests/observed_stream.py, both roles, and of the binding of renet_store_append."""
import ctypes

import numpy as np
import pytest

import observed_stream as S

FIELDS = ('first', 'count', 'snap_t', 'snap_ptr', 'nbr_o', 'ent_ptr', 'snap_ent')
ROLES = (('s', 0), ('o', 2))


@pytest.fixture(scope='module')
def allq():
    splits = S.make()
    S.check_cases(*splits)
    return np.concatenate(splits)


def cut_at(allq, n):
    """The stream of the first n facts as (train, test) -- train: what lies before SPLIT_T[0] -- as an ObservedStream."""
    import preprocess as P
    a = min(n, int(np.searchsorted(allq[:, 3], S.SPLIT_T[0])))
    return P.ObservedStream((allq[:a], allq[a:n]), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)


def before(allq, t):
    return int(np.searchsorted(allq[:, 3], t))


def cases(allq):
    """{name: (facts of the old stream, facts appended)} -- the cuts of the issue."""
    mid22 = before(allq, 22) + 7                                        # inside timestamp 22: the appended t == the last
    assert allq[mid22 - 1, 3] == 22 and allq[mid22, 3] == 22
    return {'t20..': (before(allq, 20), len(allq)), 't23': (before(allq, 23), len(allq)),
            'inside_t22': (mid22, len(allq)), 'inside_t22_only': (mid22, before(allq, 23)),
            'after_first': (before(allq, 1), len(allq)), 't21_new_entity': (before(allq, 21), before(allq, 22)),
            'nothing': (before(allq, 20), before(allq, 20))}


def assert_index_equal(got, want, what):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.shape == b.shape and np.array_equal(a, b), (what, f)


def check_append(allq, n_old, n_new, what):
    import preprocess as P
    for role, col in ROLES:
        old = P.HistoryIndex(allq[:n_old], role, S.SEQ_LEN, S.NUM_ENT)
        got = old.appended(allq[:n_old, col], allq[n_old:n_new])
        assert_index_equal(got, P.HistoryIndex(allq[:n_new], role, S.SEQ_LEN, S.NUM_ENT), (what, role))


@pytest.mark.parametrize('name', ['t20..', 't23', 'inside_t22', 'inside_t22_only', 'after_first', 't21_new_entity', 'nothing'])
def test_appended_index_equals_the_rebuilt_one(allq, name):
    n_old, n_new = cases(allq)[name]
    check_append(allq, n_old, n_new, name)
    if name == 't21_new_entity':                # NEW_ENT has no snapshot before: its facts join nothing, shift nothing old
        new = allq[n_old:n_new]
        assert S.NEW_ENT in new[:, 0] and S.NEW_ENT not in allq[:n_old, [0, 2]]
    if name == 'inside_t22':                    # both kinds at once: entities that join their last snapshot, entities that open one
        old_t22 = allq[before(allq, 22):n_old]
        new_t22 = allq[n_old:before(allq, 23)]
        assert np.isin(new_t22[:, 0], old_t22[:, 0]).any() and not np.isin(new_t22[:, 0], old_t22[:, 0]).all()


def test_chain_of_single_timestamp_appends(allq):
    """From the first timestamp alone, 23 appends of one timestamp each, every index made from the APPENDED one before it
    (never from a rebuild) and compared after every step."""
    import preprocess as P
    n = before(allq, 1)
    idx = {role: P.HistoryIndex(allq[:n], role, S.SEQ_LEN, S.NUM_ENT) for role, _ in ROLES}
    for t in range(1, S.NUM_T):
        n2 = before(allq, t + 1)
        for role, col in ROLES:
            idx[role] = idx[role].appended(allq[:n, col], allq[n:n2])
            assert_index_equal(idx[role], P.HistoryIndex(allq[:n2], role, S.SEQ_LEN, S.NUM_ENT), (t, role))
        n = n2
    assert n == len(allq)
    # an entity with more than SEQ_LEN snapshots: its windows are cut at SEQ_LEN, not at the entity's first snapshot
    for role, _ in ROLES:
        h = idx[role]
        assert np.diff(h.ent_ptr).max() > S.SEQ_LEN
        assert (h.first > h.ent_ptr[h.snap_ent[np.minimum(h.first, len(h.snap_ent) - 1)]]).any() and h.count.max() == S.SEQ_LEN
        fh, want = h.take(np.arange(len(allq))), P.HistoryIndex(allq, role, S.SEQ_LEN, S.NUM_ENT).take(np.arange(len(allq)))
        for f in ('seq_ptr', 'step_t', 'nbr_ptr', 'nbr_o'):
            assert np.array_equal(getattr(fh, f), getattr(want, f)), f


def test_appended_refuses_what_cannot_be_appended(allq):
    import preprocess as P
    n = before(allq, 22)
    h = P.HistoryIndex(allq[:n], 's', S.SEQ_LEN, S.NUM_ENT)
    with pytest.raises(ValueError):
        h.appended(allq[:n, 0], np.array([[0, 1, 2, 20]]))                      # earlier than the index's last snapshot
    with pytest.raises(ValueError):
        h.appended(allq[:n, 0], np.array([[0, 1, 2, 25], [0, 1, 2, 24]]))       # not sorted
    with pytest.raises(ValueError):
        h.appended(allq[:n, 0], np.array([[S.NUM_ENT, 1, 2, 24]]))
    with pytest.raises(ValueError):
        h.appended(allq[:n - 1, 0], allq[n:])                                    # not the old quadruples' entity column


def assert_stream_equal(got, want):
    assert np.array_equal(got.allq, want.allq) and got.ranges == want.ranges and len(got) == len(want)
    assert np.array_equal(got.times, want.times) and got.times.dtype == want.times.dtype
    assert (got.num_ent, got.num_rels, got.history_len) == (want.num_ent, want.num_rels, want.history_len)
    assert list(got.graph_dict.keys()) == list(want.graph_dict.keys())
    for t in want.graph_dict:
        for a, b in zip(got.graph_dict[t].global_triples(), want.graph_dict[t].global_triples()):
            assert np.array_equal(a, b), t
        assert np.array_equal(got.graph_dict[t].ent, want.graph_dict[t].ent)
    pos = got.positions('test')
    for h in (1, 2, 3):
        if len(pos):
            assert np.array_equal(got.horizon_as_of(pos, h), want.horizon_as_of(pos, h))


@pytest.mark.parametrize('name', ['t20..', 't23', 'inside_t22', 'after_first', 'nothing'])
def test_light_stream_equals_extended(allq, name):
    n_old, n_new = cases(allq)[name]
    old = cut_at(allq, n_old)
    quads = allq[n_old:n_new]
    got, want = old._appended(old._checked_new(quads)), old.extended(quads)
    assert got._hist == {'s': None, 'o': None}                         # no host index until it is asked for
    assert_stream_equal(got, want)
    shared = [t for t in old.graph_dict if got.graph_dict[t] is old.graph_dict[t]]
    assert len(shared) == len(old.graph_dict) - (1 if name == 'inside_t22' else 0)      # old graphs shared, t == last replaced
    assert len(old.graph_dict) == len(np.unique(allq[:n_old, 3]))                         # (the old stream's dict is untouched)
    for f in ('hist_s', 'hist_o'):
        assert_index_equal(getattr(got, f), getattr(want, f), f)
        assert np.array_equal(getattr(got, f).nbr_r, getattr(want, f).nbr_r)
    assert got.hist_s is got.hist_s


def test_light_stream_chain(allq):
    old = cut_at(allq, before(allq, 1))
    for t in range(1, S.NUM_T):
        old = old._appended(old._checked_new(allq[before(allq, t):before(allq, t + 1)]))
    import preprocess as P
    n1 = before(allq, 1)                                                 # (appends go to the last split)
    want = P.ObservedStream((allq[:n1], allq[n1:]), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    assert_stream_equal(old, want)
    assert_index_equal(old.hist_o, want.hist_o, 'chain')


def test_observe_refuses_as_extended_does(allq):
    import preprocess as P
    obs = P.ObservedStream(S.make(), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    for bad in (np.array([[0, 1, 2, 22]]), np.array([[0, 1, 2, 25], [0, 1, 2, 24]]), np.array([[S.NUM_ENT, 1, 2, 24]]),
                np.array([[0, S.NUM_RELS, 2, 24]])):
        with pytest.raises(ValueError) as a:
            obs.extended(bad)
        with pytest.raises(ValueError) as b:
            obs._checked_new(bad)
        assert str(a.value) == str(b.value)
    with pytest.raises(ValueError):
        obs.observe(allq[-1:], None)                                             # no resident() before


def test_binding_and_entry_points_are_attached():
    import gpu_builder as GB
    import preprocess as P
    import renet_hip as K
    assert {'renet_store_append', 'renet_store_append_workspace', 'renet_append_i32'} <= set(K.EXPORTS)
    restype, argtypes = K._SIGNATURES['renet_store_append']
    assert restype is ctypes.c_int and len(argtypes) == 27
    assert argtypes[7:11] == [ctypes.c_int] * 4 and argtypes[15:17] == [ctypes.c_int] * 2
    assert argtypes[25] is ctypes.c_size_t and argtypes[26] is ctypes.c_void_p
    assert [a for k, a in enumerate(argtypes) if k not in (7, 8, 9, 10, 15, 16, 25)] == [ctypes.c_void_p] * 20
    assert K._SIGNATURES['renet_store_append_workspace'] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    assert K._SIGNATURES['renet_append_i32'][0] is ctypes.c_int and len(K._SIGNATURES['renet_append_i32'][1]) == 6
    assert callable(K.store_append) and callable(K.append_i32)
    assert callable(GB.ObservedStore.appended) and callable(P.ObservedStream.observe) and callable(P.HistoryIndex.appended)
