"""CPU tests of the float64 statement of training through the joint copy mix (tests/event_gate_statement.py) on the stream of
tests/recurrence_statement.py: dq against a central difference of q, every gradient of the loss against float64 autograd, W
against event_prior_statement.group_mass, and the new entries' names.

Bounds.  q(rate) is a ratio of sums of 2^(-D rate) with lags D <= Dmax = the query time: its k-th derivative is a cumulant-like
combination of moments of ln2 D, at most a small constant (taken as 8) times (ln2 Dmax)^k.  The central difference
(q(rate + h) - q(rate - h)) / 2h has the truncation error h^2 / 6 |q'''| <= 8 h^2 / 6 (ln2 Dmax)^3 and the rounding error of two
float64 quotients over 2h, 64 * 2^-52 / h with the sums' own roundings; h = 2^-20 balances them near 1.5e-5 for Dmax = 336,
against derivatives of 1e-2 to 1e2 (measured error: under 2e-8).  Autograd and the closed forms differ by roundings of float64
only: 1e-12 relative to the largest entry."""
import numpy as np
import pytest
import torch

import event_gate_statement as ES
import event_prior_statement as EP
import recurrence_statement as RS

RATES = (0.0, float(np.float32(1.0 / 24.0)))


def statement_queries(facts, role, stale=0):
    """40 facts of the stream asked for their own (relation, partner) at their own time, the hot pair one step behind the
    stream's end, and one row each with a relation of -1, a relation of R, a gold of -1 and an entity of -1."""
    e_col, p_col = (0, 2) if role == 0 else (2, 0)
    pick = facts[np.random.RandomState(71 + role).choice(len(facts), 40, replace=False)]
    ent, rel, gold, t = (list(pick[:, k]) for k in (e_col, 1, p_col, 3))
    end = int(facts[:, 3].max())
    hot = (RS.HOT_S, RS.HOT_R, RS.HOT_O) if role == 0 else (RS.HOT_O, RS.HOT_R, RS.HOT_S)
    for e, r, g in (hot, (hot[0], -1, hot[2]), (hot[0], RS.NUM_RELS, hot[2]), (hot[0], hot[1], -1), (-1, hot[1], hot[2])):
        ent.append(e), rel.append(r), gold.append(g), t.append(end + RS.STEP)
    ent, rel, gold, t = (np.asarray(x, dtype=np.int64) for x in (ent, rel, gold, t))
    return ent, rel, t, t - stale * RS.STEP, gold


@pytest.mark.parametrize('stale', [0, 2])
@pytest.mark.parametrize('rate', RATES)
@pytest.mark.parametrize('role', [0, 1])
def test_dq_equals_a_central_difference_and_w_is_the_group_mass(role, rate, stale):
    import preprocess as P
    facts = RS.make_stream()
    pi = P.PairIndex(facts, role, RS.NUM_ENT)
    ent, rel, t, as_of, gold = statement_queries(facts, role, stale)
    q, W, dq, G, GD, WD = ES.gold_rows(pi, ent, rel, t, as_of, gold, rate, RS.NUM_RELS, RS.NUM_ENT)
    assert np.array_equal(W, EP.group_mass(pi.event_rows(ent, t, as_of, inv_half_life=rate)))
    n = len(ent)
    assert q[n - 5] > 0 and W[n - 5] > (256 if (role, rate, stale) == (0, 0.0, 0) else 0)   # the hot entity: a run longer than a workgroup
    assert all(W[i] > 0 and q[i] == 0 and dq[i] == 0 for i in (n - 4, n - 3, n - 2)) and W[n - 1] == 0 and q[n - 1] == 0
    assert np.all((q >= 0) & (q <= 1)) and np.count_nonzero(q) >= 10 and np.all(dq[(W == 0) | (G == 0)] == 0)
    h = 2.0 ** -20
    base = max(rate, h)                                                    # (a decay is >= 0: at rate 0 the difference is taken at h)
    qp = ES.gold_rows(pi, ent, rel, t, as_of, gold, base + h, RS.NUM_RELS, RS.NUM_ENT)[0]
    qm = ES.gold_rows(pi, ent, rel, t, as_of, gold, base - h, RS.NUM_RELS, RS.NUM_ENT)[0]
    dq0 = ES.gold_rows(pi, ent, rel, t, as_of, gold, base, RS.NUM_RELS, RS.NUM_ENT)[2]
    err = np.abs((qp - qm) / (2 * h) - dq0)
    print('dq against the central difference, role %d rate %.4g stale %d: %.3e, %d rows with dq != 0'
          % (role, rate, stale, float(err.max()), np.count_nonzero(dq0)))
    bound = 8.0 * h * h / 6.0 * (ES.LN2 * t.astype(np.float64)) ** 3 + 64.0 * 2.0 ** -52 / h
    assert np.all(err <= bound) and np.count_nonzero(np.abs(dq0) > 100 * bound) >= 5
    if rate == 0.0:
        assert np.array_equal(G, np.round(G)) and np.array_equal(W, np.round(W))   # plain counts


def test_gradients_equal_float64_autograd():
    rng = np.random.RandomState(3)
    n, C, R = 24, 57, RS.NUM_RELS
    x, y = 3 * rng.standard_normal((n, C)), 2 * rng.standard_normal((n, R))
    gold, rel = rng.randint(0, C, n), rng.randint(0, R, n)
    a, q = rng.uniform(0.05, 0.95, n), rng.uniform(0.01, 0.9, n)
    kind = np.arange(n) % 4
    a[kind == 0] = 0.0
    q[kind == 1] = 0.0
    q[kind == 2] = 1.0
    L, dx, dy, d_a, d_q, s = ES.joint_mix_ce(x, gold, y, rel, a, q)
    xt, yt, at, qt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, y, a, q))
    rows = torch.arange(n)
    pj = torch.softmax(xt, 1)[rows, torch.from_numpy(gold)] * torch.softmax(yt, 1)[rows, torch.from_numpy(rel)]
    loss = -torch.log((1 - at) * pj + at * qt)
    loss.sum().backward()
    for got, want, name in ((L, loss.detach().numpy(), 'L'), (dx, xt.grad.numpy(), 'dx'), (dy, yt.grad.numpy(), 'dy'),
                            (d_a, at.grad.numpy(), 'd_a'), (d_q, qt.grad.numpy(), 'd_q')):
        assert np.all(np.abs(got - want) <= 1e-12 * max(1.0, float(np.abs(want).max()))), name
    assert np.all((s >= 0) & (s <= 1)) and np.all(s[(a == 0) | (q == 0)] == 1.0)
    # both heads receive their plain CE gradient times the same scalar
    plain = ES.joint_mix_ce(x, gold, y, rel, np.zeros(n), np.zeros(n))
    assert np.allclose(dx, s[:, None] * plain[1], rtol=1e-13, atol=0) and np.allclose(dy, s[:, None] * plain[2], rtol=1e-13, atol=0)
    # the product underflows: the statement stays finite where a == 0 or q == 0, and the copy term carries the row elsewhere
    lp = np.full(n, -800.0)
    L2, dx2, d_a2, d_q2, s2 = ES.joint_mix_ce_lp(x, gold, lp, a, q)
    assert np.all(np.isfinite(L2)) and np.all(s2[(a > 0) & (q > 0)] == 0.0)
    assert np.allclose(L2[(a > 0) & (q > 0)], -np.log((a * q)[(a > 0) & (q > 0)]), rtol=1e-14, atol=0)


def test_the_new_entries_are_exported():
    import renet_hip as K
    for name in ('renet_joint_gold_rows', 'renet_joint_gold_rows_decay', 'renet_joint_mix_ce', 'renet_joint_mix_ce_planes'):
        assert name in K.EXPORTS
    for name in ('joint_gold_rows', 'joint_gold_rows_decay', 'joint_mix_ce', 'joint_mix_ce_planes'):
        assert callable(getattr(K, name))
