"""CPU tests of the float64 statement of the learned half-life (tests/half_life_statement.py): the closed form of dq / d(decay)
against float64 autograd of q(decay), preprocess.PairIndex.prior_rows with one decay per row against its scalar calls, and the
parameters of recurrence.CopyGate(learn_half_life=True).

Bound of the closed form: every one of the four sums G, W, GD, WD carries a summation-order error of at most n 2^-53 of itself,
and dq is the difference GD W - G WD of two products of them over W^2: at most n_counted 2^-50 scale with scale = ln2 (GD W +
G WD) / W^2 (tests/half_life_statement.py).  Measured: under 5e-16 scale."""
import math

import numpy as np
import pytest
import torch

import half_life_statement as HS
import recurrence_statement as RS


def test_the_stream_has_the_long_groups():
    import preprocess as P
    facts = HS.make_stream()
    assert facts.shape == (754, 4) and int(facts[:, :3:2].max()) + 1 == RS.NUM_ENT and len(np.unique(facts[:, 1])) == RS.NUM_RELS
    assert np.all(np.diff(facts[:, 3]) >= 0) and len(np.unique(facts[:, 3])) == RS.NUM_T
    for role in (0, 1):
        e, r, g, t = HS.long_row(facts, role)
        o, tp = HS.counted(P.PairIndex(facts, role, RS.NUM_ENT), e, r, t)
        assert np.count_nonzero(o == g) > 150                            # beyond RC_LONG = 128: a whole wave sums the group
    assert np.count_nonzero((facts[:, 0] == RS.HOT_S) & (facts[:, 1] == RS.HOT_R)) > 256    # more facts than a workgroup has threads


@pytest.mark.parametrize('rate', HS.RATES)
@pytest.mark.parametrize('role', [0, 1])
def test_closed_form_dq_equals_float64_autograd(role, rate):
    import preprocess as P
    facts = HS.make_stream()
    pi = P.PairIndex(facts, role, RS.NUM_ENT)
    ent, rel, t, as_of, gold = HS.statement_queries(facts, role)
    assert len(ent) == 41
    q, W, dq, scale, cnt = HS.gold_rows_decay(pi, ent, rel, t, as_of, gold, rate, RS.NUM_ENT)
    q_ad, dq_ad = HS.q_autograd(pi, ent, rel, t, as_of, gold, rate, RS.NUM_ENT)
    err = np.abs(dq - dq_ad)
    rel_err = float(np.max(err[scale > 0] / scale[scale > 0]))
    print('dq closed form against autograd, role %d rate %.6g: %.3e of scale, %d rows with dq != 0'
          % (role, rate, rel_err, np.count_nonzero(dq)))
    assert np.all(err <= cnt * 2.0 ** -50 * scale)
    assert np.all(np.abs(q - q_ad) <= cnt * 2.0 ** -52 * q)
    assert np.count_nonzero(dq) >= 5                    # (autograd rounds where the closed form's difference is exactly 0)
    assert np.all(dq[(W == 0) | (q == 0)] == 0.0)
    # the second form: -ln2 q (E_gold[D] - E_all[D])
    i = len(ent) - 1                                                      # the long group's row
    o, tp = HS.counted(pi, ent[i], rel[i], as_of[i])
    lag, w = (t[i] - tp).astype(np.float64), np.exp2(-(t[i] - tp).astype(np.float64) * rate)
    hit = o == gold[i]
    want = -HS.LN2 * q[i] * ((lag * w)[hit].sum() / w[hit].sum() - (lag * w).sum() / w.sum())
    assert hit.sum() > 150 and abs(dq[i] - want) <= cnt[i] * 2.0 ** -50 * scale[i]


@pytest.mark.parametrize('role', [0, 1])
def test_prior_rows_with_an_array_decay_equals_the_scalar_calls(role):
    import preprocess as P
    facts = HS.make_stream()
    pi = P.PairIndex(facts, role, RS.NUM_ENT)
    ent, rel, t, as_of, _ = HS.statement_queries(facts, role, stale=1)
    rates = np.asarray(HS.RATES + (float(np.float32(1.0 / 3.0)),))[np.random.RandomState(8).randint(0, 4, len(ent))]
    ptr, col, w = pi.prior_rows(ent, rel, t, as_of, inv_half_life=rates)
    assert len(ptr) == len(ent) + 1 and ptr[-1] == len(col) == len(w) and len(col) > 40
    for i in range(len(ent)):
        p1, c1, w1 = pi.prior_rows(ent[i:i + 1], rel[i:i + 1], t[i:i + 1], as_of[i:i + 1], inv_half_life=float(rates[i]))
        assert np.array_equal(col[ptr[i]:ptr[i + 1]], c1) and np.array_equal(w[ptr[i]:ptr[i + 1]], w1)
    # the scalar behaviour is unchanged, and a constant array is the scalar
    for ihl in (None, HS.RATES[1]):
        a, b = pi.prior_rows(ent, rel, t, as_of, inv_half_life=ihl), pi.prior_rows(ent, rel, t, as_of, half_life=None if ihl is None else 1.0 / ihl)
        assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.allclose(a[2], b[2], rtol=1e-12, atol=0)
    c = pi.prior_rows(ent, rel, t, as_of, inv_half_life=np.full(len(ent), HS.RATES[1]))
    assert all(np.array_equal(x, y) for x, y in zip(c, pi.prior_rows(ent, rel, t, as_of, inv_half_life=HS.RATES[1])))
    with pytest.raises(ValueError):
        pi.prior_rows(ent, rel, t, as_of, inv_half_life=rates[:3])


def test_copy_gate_with_a_learned_half_life_has_a_second_parameter():
    import recurrence as RC
    gate = RC.CopyGate(RS.NUM_RELS, alpha=0.3, half_life=24, learn_half_life=True)
    assert sorted(gate.state_dict()) == ['log_rate', 'logit'] and [n for n, _ in gate.named_parameters()] == ['logit', 'log_rate']
    assert gate.log_rate.shape == gate.logit.shape == (2, RS.NUM_RELS) and gate.log_rate.dtype == torch.float32
    assert torch.equal(gate.log_rate.detach(), torch.full((2, RS.NUM_RELS), math.log(1.0 / 24.0), dtype=torch.float32))
    assert torch.equal(gate.rate_table(), torch.exp(gate.log_rate)) and gate.rate_table().requires_grad
    hl = gate.half_lives()
    assert isinstance(hl, np.ndarray) and hl.shape == (2, RS.NUM_RELS) and np.all(np.abs(hl - 24.0) <= 24.0 * 2.0 ** -21)
    assert gate.check() is gate
    one = RC.CopyGate(RS.NUM_RELS, half_life=7.0, per_relation=False, learn_half_life=True)
    assert one.log_rate.shape == (2, 1)
    # the rows of the table, with the gates' index: 'sub' rows come from the table's second row
    with torch.no_grad():
        gate.log_rate[1, 2] = math.log(0.5)
    rows = gate.rate_rows('sub', np.asarray([2, 0])).detach()
    assert rows.shape == (2,) and abs(float(rows[0]) - 0.5) <= 1e-7 and abs(float(rows[1]) - 1.0 / 24.0) <= 1e-8
    assert torch.equal(gate.rate_rows('ob', torch.tensor([2])), gate.rate_table().detach()[0, 2:3])
    # a state_dict round trip carries the decays
    again = RC.CopyGate(RS.NUM_RELS, half_life=1.0, learn_half_life=True)
    again.load_state_dict(gate.state_dict())
    assert torch.equal(again.log_rate, gate.log_rate) and torch.equal(again.logit, gate.logit)


def test_refusals_and_the_fixed_gate_is_unchanged():
    import recurrence as RC
    with pytest.raises(ValueError):
        RC.CopyGate(RS.NUM_RELS, learn_half_life=True)                    # no half_life to start from
    with pytest.raises(ValueError):
        RC.CopyGate(RS.NUM_RELS, half_life=0.0, learn_half_life=True)
    fixed = RC.CopyGate(RS.NUM_RELS, alpha=0.3, half_life=24)
    assert list(fixed.state_dict()) == ['logit'] and not fixed.learn_half_life and not hasattr(fixed, 'log_rate')
    assert fixed.inv_half_life == float(np.float32(1.0 / 24.0))
    with pytest.raises(ValueError):
        fixed.rate_table()
    gate = RC.CopyGate(RS.NUM_RELS, half_life=24, learn_half_life=True)
    for bad in (float('nan'), float('inf')):
        with torch.no_grad():
            gate.log_rate[0, 1] = bad
        with pytest.raises(ValueError):
            gate.check()
    with torch.no_grad():
        gate.log_rate[0, 1] = 0.0
    assert gate.check() is gate
