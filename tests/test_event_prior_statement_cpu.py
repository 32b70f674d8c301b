"""CPU tests of the host statement of the joint copy mix (renet_joint_mix_rows): preprocess.PairIndex.event_rows against a
brute-force mask over the quadruples and against prior_rows, tests/event_prior_statement.py's mix_block (alpha = 0, mass
conservation), the header / binding / public keywords, and the guard the exact-rank baseline test on the GPU rests on."""
import inspect

import numpy as np
import pytest

import event_prior_statement as ES
import recurrence_statement as RS
from test_recurrence_cpu import queries_of


@pytest.fixture(scope='module')
def quads():
    return RS.make_stream()


def histories(quads):
    """(ent, t, as_of) of role-0 histories: queries_of's, their relation dropped."""
    ent, rel, t, as_of = queries_of(quads)
    return ent, t, as_of


@pytest.mark.parametrize('role', [0, 1])
@pytest.mark.parametrize('half_life', [None, 24.0, 100.0])
def test_event_rows_equal_a_brute_force_mask(quads, role, half_life):
    import preprocess as P
    pi = P.PairIndex(quads, role, RS.NUM_ENT)
    ent, t, as_of = histories(quads)
    ptr, rel, col, w = pi.event_rows(ent, t, as_of, half_life)
    assert ptr[0] == 0 and ptr[-1] == len(rel) == len(col) == len(w) and w.dtype == np.float64
    e_col, p_col = (0, 2) if role == 0 else (2, 0)
    busy = 0
    for i in range(len(ent)):
        hit = (quads[:, e_col] == ent[i]) & (quads[:, 3] < as_of[i])
        want = {}
        for f in quads[hit].tolist():
            key = (f[1], f[p_col])
            want[key] = want.get(key, 0.0) + (1.0 if half_life is None else 2.0 ** (-(t[i] - f[3]) / half_life))
        keys = list(zip(rel[ptr[i]:ptr[i + 1]].tolist(), col[ptr[i]:ptr[i + 1]].tolist()))
        assert keys == sorted(want)                                          # ascending (relation, partner), each once
        got = w[ptr[i]:ptr[i + 1]]
        assert all(abs(g - want[k]) <= 1e-12 * want[k] for g, k in zip(got, keys))
        busy += len(keys) > 64
        # no leak: the facts at or after as_of change nothing
        cut = P.PairIndex(quads[quads[:, 3] < as_of[i]], role, RS.NUM_ENT)
        _, r2, c2, w2 = cut.event_rows(ent[i:i + 1], t[i:i + 1], as_of[i:i + 1], half_life)
        assert np.array_equal(r2, rel[ptr[i]:ptr[i + 1]]) and np.array_equal(c2, col[ptr[i]:ptr[i + 1]]) and np.array_equal(w2, got)
    assert role == 1 or busy >= 1
    empty = np.diff(ptr) == 0
    assert empty[ent == -1].all() and empty[ent == RS.NUM_ENT].all() and empty[as_of <= 0].all()


@pytest.mark.parametrize('half_life', [None, 24.0])
def test_event_rows_of_one_relation_are_prior_rows_and_the_masses_add_up(quads, half_life):
    import preprocess as P
    pi = P.PairIndex(quads, 0, RS.NUM_ENT)
    ent, t, as_of = histories(quads)
    ptr, rel, col, w = pi.event_rows(ent, t, as_of, half_life)
    W = ES.group_mass((ptr, rel, col, w))
    per_rel = np.zeros_like(W)
    for r in range(RS.NUM_RELS):
        p2, c2, w2 = pi.prior_rows(ent, np.full_like(ent, r), t, as_of, half_life)
        for i in range(len(ent)):
            mine = rel[ptr[i]:ptr[i + 1]] == r
            assert np.array_equal(col[ptr[i]:ptr[i + 1]][mine], c2[p2[i]:p2[i + 1]])
            assert np.array_equal(w[ptr[i]:ptr[i + 1]][mine], w2[p2[i]:p2[i + 1]])
            per_rel[i] += w2[p2[i]:p2[i + 1]].sum()
    assert set(rel.tolist()) <= set(range(RS.NUM_RELS))
    if half_life is None:
        assert np.array_equal(W, per_rel)
    else:
        assert np.all(np.abs(W - per_rel) <= 1e-12 * per_rel)
    # inv_half_life is used as given
    a = pi.event_rows(ent, t, as_of, half_life=24.0)[3]
    b = pi.event_rows(ent, t, as_of, inv_half_life=1.0 / 24.0)[3]
    c = pi.event_rows(ent, t, as_of, inv_half_life=float(np.float32(1.0 / 24.0)))[3]
    assert np.array_equal(a, b) and not np.array_equal(a, c) and np.allclose(a, c, rtol=1e-5)


def random_joint(G, R, C, seed):
    """fp32 [G, R, C]: log-probabilities of a random joint per group (exp sums to 1 up to fp32 rounding)."""
    x = 3.0 * np.random.RandomState(seed).randn(G, R * C)
    x -= np.asarray([ES.logsumexp64(row) for row in x])[:, None]
    return x.reshape(G, R, C).astype(np.float32)


def test_mix_block_alpha_zero_is_j_and_a_mixed_group_keeps_its_mass(quads):
    import preprocess as P
    pi = P.PairIndex(quads, 0, RS.NUM_ENT)
    ent, t, as_of = histories(quads)
    rows = pi.event_rows(ent, t, as_of, 100.0)
    G, R, C = len(ent), RS.NUM_RELS, RS.NUM_ENT
    J = random_joint(G, R, C, 11)
    assert np.array_equal(ES.mix_block(J, rows, 0.0), J.astype(np.float64))
    W = ES.group_mass(rows)
    assert np.any(W > 0) and np.any(W == 0)
    for alpha in (0.3, 0.9):
        M = ES.mix_block(J, rows, alpha)
        assert np.array_equal(M[W == 0], J[W == 0].astype(np.float64))       # the prior abstains: M is J
        assert not np.array_equal(M[W > 0], J[W > 0].astype(np.float64))
        for g in np.nonzero(W > 0)[0]:
            # (1 - a) sum exp(J) + a sum w / W = sum exp(J) when that sum is 1: the mixed joint is normalised as J is
            assert abs(ES.logsumexp64(M[g]) - ES.logsumexp64(J[g])) <= 1e-6
    # pairs outside the block count in W and are not addressed: with C = 64 the partners 64 .. 67 of the hot pair lose their mass
    small = ES.mix_block(np.ascontiguousarray(J[:, :, :64]), rows, 0.3)
    full = ES.mix_block(J, rows, 0.3)
    assert np.array_equal(small, full[:, :, :64])
    hot = int(np.nonzero((ent == RS.HOT_S) & (W > 100))[0][0])
    assert ES.logsumexp64(small[hot]) < ES.logsumexp64(J[hot, :, :64])


def test_header_binding_and_public_keywords():
    import model as M
    import recurrence as RC
    import renet_hip as K
    assert 'renet_joint_mix_rows' in K.EXPORTS
    for name in ('evaluate_events_observed', 'predict_events_observed', 'observed_event_scores', 'forecast_events'):
        assert inspect.signature(getattr(M.RENet, name)).parameters['prior'].default is None, name
    assert callable(RC.evaluate_events)
    import preprocess as P
    assert callable(P.PairIndex.event_rows)
    # a per-relation gate gives no normalised joint: refused before any use of the device
    with pytest.raises(ValueError, match='per-relation'):
        RC.event_alpha(RC.CopyGate(RS.NUM_RELS, 0.3, per_relation=True), 'ob')
    gate = RC.CopyGate(RS.NUM_RELS, 0.3, per_relation=False)
    a = RC.event_alpha(gate, 'sub')
    assert a == float(np.float32(a)) and abs(a - 0.3) < 1e-6
    assert RC.event_alpha(RC.RecurrencePrior(0.25), 'ob') == 0.25
    with pytest.raises(ValueError):
        RC.event_alpha(0.3, 'ob')


def test_baseline_fp32_values_are_strictly_ordered_in_the_count(quads):
    """The guard of the exact-rank baseline test on the GPU: with the uniform joint J = -log(R C) and plain counts, for every
    (entity, as_of) of the stream and both roles the fp32 value of log((1 - a) / (R C) + a c / W) is strictly increasing in
    the integer count c over the counts that occur (0, the unseen pairs, included), with more than two fp32 steps between
    neighbours, and the unseen pairs' dense form J + log1p(-a) is the smallest of them."""
    alpha = float(np.float32(0.5))
    R, C = RS.NUM_RELS, RS.NUM_ENT
    J = float(np.float32(-np.log(float(R * C))))
    times = list(np.unique(quads[:, 3])) + [int(quads[:, 3].max()) + RS.STEP]
    checked = 0
    for role in (0, 1):
        e_col = 0 if role == 0 else 2
        for e in sorted(set(quads[:, e_col].tolist())):
            for as_of in times:
                c = np.stack([RS.partner_counts(quads, role, e, r, as_of) for r in range(R)])
                W = float(c.sum())
                if W == 0:
                    continue
                counts = np.unique(c)
                assert counts[0] == 0
                v = np.log((1.0 - alpha) * np.exp(J) + alpha * counts / W).astype(np.float32)
                v[0] = np.float32(J + np.log1p(-alpha))
                up2 = np.nextafter(np.nextafter(v[:-1], np.float32(np.inf)), np.float32(np.inf))
                assert np.all(up2 < v[1:]), (role, e, as_of)
                checked += 1
    assert checked > 500
