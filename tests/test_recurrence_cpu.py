"""CPU tests of the host statements of the recurrence prior: preprocess.PairIndex (the pair tables), its appended() (the
statement of renet_pair_append), prior_rows (the statement of renet_recurrence_mix_rows with tests/recurrence_statement.py)
and the ordering guard that the exact-rank GPU test rests on."""
import numpy as np
import pytest

import recurrence_statement as RS


@pytest.fixture(scope='module')
def quads():
    q = RS.make_stream()
    assert 560 <= len(q) <= 640 and len(np.unique(q[:, 3])) == RS.NUM_T and set(np.diff(np.unique(q[:, 3]))) == {RS.STEP}
    hot = q[(q[:, 0] == RS.HOT_S) & (q[:, 1] == RS.HOT_R)]
    assert len(hot) > 300 and len(np.unique(hot[:, 2])) > 64
    assert set(hot[hot[:, 2] == RS.HOT_O][:, 3]) == set(np.unique(q[:, 3]))            # one group in every timestamp
    assert len(np.unique(q, axis=0)) < len(q)                                          # duplicate quadruples
    assert not set(q[:, 0]) & set(RS.NEVER_SUBJECT) and not set(q[:, 2]) & set(RS.NEVER_OBJECT)
    assert not np.any((q[:, 0] == RS.BARE_S) & (q[:, 1] == RS.BARE_R))
    assert not np.any((q[:, 2] == RS.BARE_O) & (q[:, 1] == RS.BARE_R))
    return q


def brute(quads, role):
    ent, other = (quads[:, 0], quads[:, 2]) if role == 0 else (quads[:, 2], quads[:, 0])
    order = np.lexsort((quads[:, 3], other, quads[:, 1], ent))
    return quads[order, 1], other[order], quads[order, 3], ent[order]


def assert_same(a, b):
    for f in ('p_rel', 'p_other', 'p_t', 'run_ptr'):
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and np.array_equal(x, y), f


@pytest.mark.parametrize('role', [0, 1])
def test_pair_index_equals_a_brute_force_lexsort(quads, role):
    import preprocess as P
    pi = P.PairIndex(quads, role, RS.NUM_ENT)
    rel, other, t, ent = brute(quads, role)
    assert np.array_equal(pi.p_rel, rel) and np.array_equal(pi.p_other, other) and np.array_equal(pi.p_t, t)
    # the fact run of an entity is the HistoryIndex's: no pointer array of its own is needed
    hi = P.HistoryIndex(quads, 's' if role == 0 else 'o', RS.SEQ_LEN, RS.NUM_ENT)
    assert np.array_equal(pi.run_ptr, hi.snap_ptr[hi.ent_ptr])
    assert np.array_equal(np.repeat(np.arange(RS.NUM_ENT), np.diff(pi.run_ptr)), ent)
    assert_same(P.PairIndex(quads, 'so'[role], RS.NUM_ENT), pi)
    # a function of the multiset of facts: file order does not matter
    assert_same(P.PairIndex(quads[np.random.RandomState(3).permutation(len(quads))], role, RS.NUM_ENT), pi)


def append_cases(quads):
    """name -> (n_old, the appended quadruples)."""
    t = quads[:, 3]
    last = int(t.max())
    a = int(np.searchsorted(t, last))                           # the first fact of the last timestamp
    mid = a + (len(quads) - a) // 2
    b = int(np.searchsorted(t, 5 * RS.STEP))
    early = quads[:b]
    fresh = sorted(set(range(RS.NUM_ENT)) - set(early[:, 0]) - set(early[:, 2]))
    assert mid > a and len(fresh) >= 2
    opens = np.asarray([[fresh[0], 0, fresh[1], 5 * RS.STEP], [fresh[1], 2, fresh[0], 5 * RS.STEP]], dtype=np.int64)
    return {
        'joins_last_timestamp': (mid, quads[mid:]),
        'whole_timestamps': (b, quads[b:a]),
        'opens_new_runs': (b, opens),
        'duplicates_of_old_facts': (a, np.concatenate((quads[a - 5:a], quads[a - 5:a]))),
        'm0': (a, quads[:0]),
        'm1': (a, quads[a:a + 1]),
    }


@pytest.mark.parametrize('role', [0, 1])
@pytest.mark.parametrize('name', ['joins_last_timestamp', 'whole_timestamps', 'opens_new_runs', 'duplicates_of_old_facts',
                                  'm0', 'm1'])
def test_appended_equals_the_index_of_the_longer_stream(quads, name, role):
    import preprocess as P
    n_old, new = append_cases(quads)[name]
    old = P.PairIndex(quads[:n_old], role, RS.NUM_ENT)
    keep = [a.copy() for a in (old.p_rel, old.p_other, old.p_t, old.run_ptr)]
    got = old.appended(new)
    assert_same(got, P.PairIndex(np.concatenate((quads[:n_old], new)), role, RS.NUM_ENT))
    assert all(np.array_equal(a, b) for a, b in zip(keep, (old.p_rel, old.p_other, old.p_t, old.run_ptr)))
    if name == 'opens_new_runs':
        e = int(new[0, 0] if role == 0 else new[0, 2])
        assert old.run_ptr[e] == old.run_ptr[e + 1] and got.run_ptr[e + 1] == got.run_ptr[e] + 1


def queries_of(quads, seed=5):
    """(ent, rel, t, as_of) of role-0 queries: stream facts, non-facts, stale as_of, t past the end, an absent side, a pair
    without history, an entity that never is a subject."""
    rng = np.random.RandomState(seed)
    pick = quads[rng.choice(len(quads), 40, replace=False)]
    ent, rel, t = list(pick[:, 0]), list(pick[:, 1]), list(pick[:, 3])
    as_of = list(pick[:, 3] - RS.STEP * rng.randint(0, 4, len(pick)))
    end = int(quads[:, 3].max())
    for e, r, tt, a in ((RS.HOT_S, RS.HOT_R, end + 3 * RS.STEP, end + 3 * RS.STEP), (RS.HOT_S, RS.HOT_R, end + RS.STEP, 100),
                        (RS.HOT_S, RS.HOT_R, 0, 0), (-1, 0, 48, 48), (RS.BARE_S, RS.BARE_R, 96, 96),
                        (RS.NEVER_SUBJECT[0], 1, 96, 96), (3, 2, 77, 50), (RS.NUM_ENT, 0, 48, 48)):
        ent.append(e), rel.append(r), t.append(tt), as_of.append(a)
    return tuple(np.asarray(x, dtype=np.int64) for x in (ent, rel, t, as_of))


@pytest.mark.parametrize('half_life', [None, 24.0, 100.0])
def test_prior_rows_equal_a_triple_loop_and_do_not_leak(quads, half_life):
    import preprocess as P
    pi = P.PairIndex(quads, 0, RS.NUM_ENT)
    ent, rel, t, as_of = queries_of(quads)
    ptr, col, w = pi.prior_rows(ent, rel, t, as_of, half_life)
    assert ptr[0] == 0 and ptr[-1] == len(col) == len(w) and w.dtype == np.float64
    for i in range(len(ent)):                                   # query, partner, quadruple
        want = {}
        mine = [f for f in quads.tolist() if f[0] == ent[i]]   # (the loops below see every quadruple of the entity)
        for o in range(RS.NUM_ENT):
            acc, seen = 0.0, False
            for s_, r_, o_, t_ in mine:
                if s_ == ent[i] and r_ == rel[i] and o_ == o and t_ < as_of[i]:
                    acc += 1.0 if half_life is None else 2.0 ** (-(t[i] - t_) / half_life)
                    seen = True
            if seen:
                want[o] = acc
        got = dict(zip(col[ptr[i]:ptr[i + 1]], w[ptr[i]:ptr[i + 1]]))
        assert sorted(got) == sorted(want) and list(col[ptr[i]:ptr[i + 1]]) == sorted(want)
        assert all(abs(got[o] - want[o]) <= 1e-12 * want[o] for o in want)
        # no leak: the facts at or after as_of change nothing
        cut = P.PairIndex(quads[quads[:, 3] < as_of[i]], 0, RS.NUM_ENT)
        p2, c2, w2 = cut.prior_rows(ent[i:i + 1], rel[i:i + 1], t[i:i + 1], as_of[i:i + 1], half_life)
        assert np.array_equal(c2, col[ptr[i]:ptr[i + 1]]) and np.array_equal(w2, w[ptr[i]:ptr[i + 1]])
    stats = pi.prior_stats(ent, rel, t, as_of)
    if half_life is None:
        assert np.array_equal(stats[:, 0], np.diff(ptr))
        assert np.array_equal(stats[:, 1], [int(round(w[a:b].sum())) for a, b in zip(ptr[:-1], ptr[1:])])
    assert np.diff(ptr)[-5] == 0 and np.diff(ptr)[-4] == 0 and np.diff(ptr)[-3] == 0 and np.diff(ptr)[-1] == 0


def test_inv_half_life_is_used_as_given(quads):
    import preprocess as P
    pi = P.PairIndex(quads, 0, RS.NUM_ENT)
    q = (np.asarray([RS.HOT_S]), np.asarray([RS.HOT_R]), np.asarray([400]), np.asarray([400]))
    a = pi.prior_rows(*q, half_life=24.0)[2]
    b = pi.prior_rows(*q, inv_half_life=1.0 / 24.0)[2]
    c = pi.prior_rows(*q, inv_half_life=float(np.float32(1.0 / 24.0)))[2]
    assert np.array_equal(a, b) and not np.array_equal(a, c) and np.allclose(a, c, rtol=1e-5)


def sigmoid32(x):
    """torch.sigmoid's fp32 formula, as csrc/rank.hip restates it."""
    x = np.asarray(x, dtype=np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def test_float32_mix_values_are_strictly_ordered_in_the_count(quads):
    """The guard of the exact-rank GPU test: with uniform logits and plain counts, for every (entity, relation, as_of) of
    the stream and both roles, the fp32 value of log((1 - a) / C + a c / W) -- and its fp32 sigmoid, which the filtered
    settings compare -- is strictly increasing in the integer count c over the counts that occur (0 for the unseen columns
    included), with more than two fp32 steps between neighbours: one rounding step of slack on either side for the device's
    own log / exp."""
    alpha = float(np.float32(0.5))
    times = list(np.unique(quads[:, 3])) + [int(quads[:, 3].max()) + RS.STEP]
    checked = 0
    for role in (0, 1):
        e_col = 0 if role == 0 else 2
        for e, r in {(int(f[e_col]), int(f[1])) for f in quads}:
            for as_of in times:
                c = RS.partner_counts(quads, role, e, r, as_of)
                W = float(c.sum())
                if W == 0:
                    continue
                counts = np.unique(c)                                    # ascending, 0 included (70 columns, <= 68 partners)
                assert counts[0] == 0
                v = np.log((1.0 - alpha) / RS.NUM_ENT + alpha * counts / W).astype(np.float32)
                for x in (v, sigmoid32(v)):
                    up2 = np.nextafter(np.nextafter(x[:-1], np.float32(np.inf)), np.float32(np.inf))
                    assert np.all(up2 < x[1:]), (role, e, r, as_of)
                assert sigmoid32(v)[0] > 0
                checked += 1
    assert checked > 500
