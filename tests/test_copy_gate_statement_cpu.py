"""CPU tests of the float64 statement of training through the copy mix (tests/copy_gate_statement.py): the analytic
gradients against float64 autograd, and q / W of preprocess.PairIndex.prior_rows against brute-force partner counts on the
shared synthetic stream (tests/recurrence_statement.py), both roles, stale as_of."""
import numpy as np
import pytest
import torch

import copy_gate_statement as CS
import recurrence_statement as RS


def test_analytic_gradients_equal_float64_autograd():
    rng = np.random.RandomState(3)
    n, C = 24, 37
    z = 3.0 * rng.randn(n, C)
    gold = rng.randint(0, C, n)
    gold[:2] = (0, C - 1)
    u = 2.0 * rng.randn(n)
    q = rng.rand(n)
    q[3:6] = (0.0, 1.0, 0.0)
    z[6, gold[6]] -= 40.0                                                 # a small p_g
    a = 1.0 / (1.0 + np.exp(-u))
    loss, dz, da = CS.mix_ce(z, gold, a, q)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
    at = torch.sigmoid(ut)
    pg = torch.softmax(zt, dim=1)[torch.arange(n), torch.from_numpy(gold)]
    lt = -torch.log((1 - at) * pg + at * torch.tensor(q))
    lt.sum().backward()
    assert np.max(np.abs(loss - lt.detach().numpy())) <= 1e-12
    assert np.max(np.abs(dz - zt.grad.numpy())) <= 1e-12
    assert np.max(np.abs(da * a * (1 - a) - ut.grad.numpy())) <= 1e-12    # d/du = d/da * sigmoid'(u)
    s = -dz[np.arange(n), gold] / (1.0 - np.exp(RS.log_softmax64(z))[np.arange(n), gold])
    assert np.all(s >= 0.0) and np.all(s <= 1.0 + 1e-12)                  # the row scalar lies in [0, 1]


def test_gate_zero_or_no_prior_mass_is_the_cross_entropy():
    rng = np.random.RandomState(4)
    z = 3.0 * rng.randn(6, 11)
    gold = rng.randint(0, 11, 6)
    lp = RS.log_softmax64(z)
    ce = -lp[np.arange(6), gold]
    a = np.asarray([0.0, 0.0, 0.4, 0.9, 0.0, 0.25])
    q = np.asarray([0.0, 0.7, 0.0, 0.0, 1.0, 0.0])
    loss, dz, _ = CS.mix_ce(z, gold, a, q)
    onehot = np.eye(11)[gold]
    assert np.max(np.abs(loss - (ce - np.log1p(-a)))) <= 1e-12
    assert np.array_equal(dz, np.exp(lp) - onehot)
    # an underflowed p_g with prior mass: the copy term carries the row, the logits get no gradient
    z[0, gold[0]] = z[0].max() - 2000.0
    loss, dz, da = CS.mix_ce(z[:1], gold[:1], np.asarray([0.3]), np.asarray([0.5]))
    assert abs(loss[0] + np.log(0.15)) <= 1e-12 and np.all(dz == 0.0) and abs(da[0] + 1.0 / 0.3) <= 1e-12


@pytest.mark.parametrize('half_life', [None, 24.0])
@pytest.mark.parametrize('role', [0, 1])
def test_gold_rows_equal_brute_force_partner_counts(role, half_life):
    import preprocess as P
    quads = RS.make_stream()
    pi = P.PairIndex(quads, role, RS.NUM_ENT)
    rng = np.random.RandomState(8 + role)
    pick = quads[rng.choice(len(quads), 60, replace=False)]
    e_col, p_col = (0, 2) if role == 0 else (2, 0)
    ent, rel, gold, t = pick[:, e_col].copy(), pick[:, 1].copy(), pick[:, p_col].copy(), pick[:, 3].copy()
    as_of = t - RS.STEP * rng.randint(0, 3, len(pick))                    # at t, and one and two timestamps stale
    gold[:5] = (-1, RS.NUM_ENT, 3, 69, 0)
    ent[5] = -1
    q, W = CS.gold_rows(*pi.prior_rows(ent, rel, t, as_of, half_life), gold, RS.NUM_ENT)
    some = 0
    for i in range(len(pick)):
        if half_life is None:
            c = RS.partner_counts(quads, role, ent[i], rel[i], as_of[i]).astype(np.float64)
        else:                                                             # the weighted counts, by a mask over the quadruples
            hit = (quads[:, e_col] == ent[i]) & (quads[:, 1] == rel[i]) & (quads[:, 3] < as_of[i])
            c = np.bincount(quads[hit, p_col], weights=np.exp2(-(t[i] - quads[hit, 3]) / half_life), minlength=RS.NUM_ENT)
        Wi = c.sum()
        qi = c[gold[i]] / Wi if Wi > 0 and 0 <= gold[i] < RS.NUM_ENT else 0.0
        assert abs(W[i] - Wi) <= 1e-12 * max(Wi, 1.0) and abs(q[i] - qi) <= 1e-12, i
        some += int(qi > 0)
    assert some >= 10 and np.any(W == 0) and q[0] == q[1] == 0.0 and W[5] == 0.0
