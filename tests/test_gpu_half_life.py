"""GPU tests of the learned half-life of the recurrence prior (run with -m gpu on an MI355X): renet_recurrence_mix_rows_decay,
renet_recurrence_gold_rows_decay, the d_q output of the head Functions, recurrence.CopyGate(learn_half_life=True) through
CopyRows / fit_gate / learn_observed, the evaluation entries and the event entries.  The float64 statement is
tests/half_life_statement.py.

The kernel tests run on that statement's stream (tests/recurrence_statement.py's plus 150 facts of one partner of the hot
pair: a partner group of more than 128 counted facts in either role, which the mix kernel hands to a whole wave) with the
queries of tests/test_gpu_copy_gate.py and one row on the long group; the model tests on the world of
tests/test_gpu_recurrence.py (made once, shared, left unchanged; whatever trains does so on clones).

Bounds.  A constant decay gives the scalar entries' bits, and a row of a mixed launch the bits of the same row of a uniform
launch at its rate.  Against float64: W and q one fp32 rounding beside the fp64 sums (2^-23 relative), mixed rows ROW_BOUND of
tests/test_gpu_recurrence.py.  dq = -ln2 (GD W - G WD) / W^2 is one fp32 rounding of a difference of products of four fp64 sums,
each with a summation-order error of at most n 2^-53 of itself: |dq - dq64| <= 2^-23 |dq64| + n_counted 2^-50 scale, scale =
ln2 (GD W + G WD) / W^2.  The loss gradient d log_rate[k] = rate_k sum_i weight_i (-a_i / m_i) dq_i: -a / m = -a exp(L) carries
the relative error of m, at most that of the parent's loss -log p_g (ROW_ERR, measured in the test as
tests/test_gpu_copy_gate.py measures it, four times as there), every factor and every partial sum of the n_k rows one fp32
rounding: (4 ROW_ERR + (n_k + 4) 2^-24) sum_i |term_i| per (side, relation)."""
import numpy as np
import pytest
import torch

import copy_gate_statement as CS
import half_life_statement as HS
import recurrence_statement as RS
from test_gpu_copy_gate import _Capture, gold_queries, hip_adam, late_positions, role_args
from test_gpu_online_learning import clone_of, same_parameters
from test_gpu_recurrence import ROW_BOUND, SETTINGS, i32, model_queries, stream_of, world

pytestmark = pytest.mark.gpu

RATES4 = HS.RATES + (float(np.float32(1.0 / 3.0)),)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _to(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


_LONG = {}


def long_world(dev):
    """The statement's stream of 754 facts, resident: made once, shared, only read."""
    if not _LONG:
        w = world(dev)
        facts = HS.make_stream()
        _LONG.update(facts=facts, store=stream_of(facts).resident(w['net'], w['gnet']))
    return _LONG


def queries(facts, role, stale):
    """gold_queries of tests/test_gpu_copy_gate.py and, last, the row on the long partner group."""
    ent, rel, t, as_of, gold = gold_queries(facts, role, stale)
    e, r, g, tt = HS.long_row(facts, role)
    cat = lambda x, v: np.concatenate((x, [v])).astype(np.int64)
    return cat(ent, e), cat(rel, r), cat(t, tt), cat(as_of, tt - stale * RS.STEP), cat(gold, g)


def case(dev, role, stale):
    lw = long_world(dev)
    ent, rel, t, as_of, gold = queries(lw['facts'], role, stale)
    args = [i32(x, dev) for x in (ent, rel, t, as_of)]
    return lw['facts'], lw['store'], (ent, rel, t, as_of, gold), args, i32(gold, dev)


def gates(n, dev):
    alpha = np.random.RandomState(5).uniform(0.0, 0.95, n).astype(np.float32)
    alpha[1] = 0.0
    return alpha, _to(alpha, dev)


# ---- 1. a uniform decay is the scalar entries, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize('stale', [0, 2])
@pytest.mark.parametrize('role', [0, 1])
def test_a_uniform_decay_equals_the_scalar_entries_bit_for_bit(dev, role, stale):
    import renet_hip as K
    facts, store, q, args, gold = case(dev, role, stale)
    n, C = len(q[0]), RS.NUM_ENT
    _, alpha = gates(n, dev)
    x = _to((3.0 * np.random.RandomState(17 + role).randn(n, C)).astype(np.float32), dev)
    for h in (0.0, float(np.float32(1.0 / 24.0))):
        ihl = torch.full((n,), h, device=dev)
        for logits in (None, x):
            want = K.recurrence_mix_rows_gated(*args, *role_args(store, role), logits, alpha, h, num_cols=C, want_stats=True)
            got = K.recurrence_mix_rows_decay(*args, *role_args(store, role), logits, alpha, ihl, num_cols=C, want_stats=True)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (h, logits is None)
            assert got[1][-1, 1] > 128 and bool(torch.isfinite(got[0]).all())           # the long group's row counts its facts
        qs, Ws = K.recurrence_gold_rows(*args, gold, *role_args(store, role), C, h)
        qd, Wd, dq = K.recurrence_gold_rows_decay(*args, gold, *role_args(store, role), C, ihl)
        assert torch.equal(qs, qd) and torch.equal(Ws, Wd) and bool(torch.isfinite(dq).all())
        assert float(qd[-1]) > 0 and torch.equal(Wd, got[2])


# ---- 2. mixed decays in one launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('stale', [0, 2])
@pytest.mark.parametrize('role', [0, 1])
def test_mixed_decays_in_one_launch(dev, role, stale):
    import preprocess as P
    import renet_hip as K
    facts, store, q, args, gold = case(dev, role, stale)
    ent, rel, t, as_of, gold_h = q
    n, C = len(ent), RS.NUM_ENT
    alpha_h, alpha = gates(n, dev)
    pick = np.random.RandomState(23 + role).randint(0, 4, n)
    pick[-1], pick[-9] = 3, 2                                            # the long group at 1/3, the hot pair at 1/240
    rate = np.asarray(RATES4, dtype=np.float32)[pick]
    assert all(np.count_nonzero(pick == k) >= 5 for k in range(4))
    x_h = (3.0 * np.random.RandomState(29 + role).randn(n, C)).astype(np.float32)
    x = _to(x_h, dev)
    out, stats, W = K.recurrence_mix_rows_decay(*args, *role_args(store, role), x, alpha, _to(rate, dev), want_stats=True)
    flat = K.recurrence_mix_rows_decay(*args, *role_args(store, role), None, alpha, _to(rate, dev), num_cols=C)
    qd, Wd, dq = K.recurrence_gold_rows_decay(*args, gold, *role_args(store, role), C, _to(rate, dev))
    assert torch.equal(W, Wd)
    # rows of one launch do not leak into each other: each is the row of a uniform launch at its own rate
    for k, h in enumerate(RATES4):
        ihl = torch.full((n,), h, device=dev)
        rows = _to(np.nonzero(pick == k)[0], dev)
        u_out, u_stats, u_W = K.recurrence_mix_rows_decay(*args, *role_args(store, role), x, alpha, ihl, want_stats=True)
        u_flat = K.recurrence_mix_rows_decay(*args, *role_args(store, role), None, alpha, ihl, num_cols=C)
        u_q, u_Wd, u_dq = K.recurrence_gold_rows_decay(*args, gold, *role_args(store, role), C, ihl)
        for a, b in ((out, u_out), (stats, u_stats), (W, u_W), (flat, u_flat), (qd, u_q), (Wd, u_Wd), (dq, u_dq)):
            assert torch.equal(a[rows], b[rows]), h
    # against float64
    pi = P.PairIndex(facts, role, RS.NUM_ENT)
    q64, W64, _, _, cnt = HS.gold_rows_decay(pi, ent, rel, t, as_of, gold_h, rate.astype(np.float64), C)
    Wg, qg = W.double().cpu().numpy(), qd.double().cpu().numpy()
    assert np.all(np.abs(Wg - W64) <= 2.0 ** -23 * W64) and np.array_equal(Wg == 0, W64 == 0)
    assert np.all(np.abs(qg - q64) <= 2.0 ** -23 * q64) and np.array_equal(qg == 0, q64 == 0)
    assert np.array_equal(stats.cpu().numpy()[:, 1], cnt) and cnt[-1] > 128 and np.count_nonzero(q64) >= 10
    for logits_h, got in ((x_h, out), (None, flat)):
        ref = HS.mix_rows_decay(pi, logits_h, C, ent, rel, t, as_of, alpha_h, rate.astype(np.float64))
        o = got.double().cpu().numpy()
        err = float(np.max(np.abs(np.expm1(o - ref))))
        print('mix_rows_decay role %d stale %d %s: rel err %.3e' % (role, stale, 'uniform' if logits_h is None else 'logits', err))
        assert np.all(np.isfinite(o)) and err <= ROW_BOUND
    assert torch.equal(x.cpu(), torch.from_numpy(x_h))                                   # the logits are never written


# ---- 3. dq ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stale', [0, 2])
@pytest.mark.parametrize('role', [0, 1])
def test_dq_against_float64(dev, role, stale):
    """Measured on the MI355X: see profiles/learned_half_life.md."""
    import preprocess as P
    import renet_hip as K
    facts, store, q, args, gold = case(dev, role, stale)
    ent, rel, t, as_of, gold_h = q
    n, C = len(ent), RS.NUM_ENT
    pi = P.PairIndex(facts, role, RS.NUM_ENT)
    bare, absent, beyond, late, long_ = n - 7, (n - 6, n - 5), (n - 4, n - 3), n - 2, n - 1
    for h in HS.RATES:
        ihl = torch.full((n,), h, device=dev)
        qd, Wd, dq = K.recurrence_gold_rows_decay(*args, gold, *role_args(store, role), C, ihl)
        q64, W64, dq64, scale, cnt = HS.gold_rows_decay(pi, ent, rel, t, as_of, gold_h, h, C)
        got = dq.double().cpu().numpy()
        err = np.abs(got - dq64)
        bound = 2.0 ** -23 * np.abs(dq64) + cnt * 2.0 ** -50 * scale
        nz = dq64 != 0
        print('dq role %d stale %d rate %.6g: %d non-zero rows, largest error %.3e of the bound, %.3e relative'
              % (role, stale, h, np.count_nonzero(nz), float(np.max(err[nz] / bound[nz])), float(np.max(err[nz] / np.abs(dq64[nz])))))
        assert np.all(np.isfinite(got)) and np.all(err <= bound)
        assert np.count_nonzero(nz) >= 5
        # exactly 0: the bare pair, the absent sides, a gold outside [0, C), gold's facts at or after as_of
        zero = (bare,) + absent + beyond + (late,)
        assert all(got[i] == 0.0 and dq64[i] == 0.0 for i in zero)
        assert W64[bare] == 0 and all(W64[i] == 0 for i in absent) and all(W64[i] > 0 for i in beyond) and W64[late] > 0
        assert cnt[long_] > 128 and dq64[long_] != 0
        if h == 0.0:                                                      # all four sums are integers: one rounding
            want = dq64.astype(np.float32)
            assert np.all(np.abs(dq.cpu().numpy().astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
        again = K.recurrence_gold_rows_decay(*args, gold, *role_args(store, role), C, ihl)
        assert all(torch.equal(a, b) for a, b in zip(again, (qd, Wd, dq)))               # run to run


# ---- 4. the loss gradient ------------------------------------------------------------------------------------------------
def learned_gate(dev, **kw):
    import recurrence as RC
    return RC.CopyGate(RS.NUM_RELS, alpha=0.3, half_life=24, learn_half_life=True, **kw).to(dev)


def log_rate_gradient_float64(net, obs, facts, idx, gate, weight, dev):
    """(grad, magnitude, rows) [2, R] of the statement on observed_scores' logits, and ROW_ERR: the largest error of the
    parent's renet_softmax_ce against float64 on the same logits."""
    import preprocess as P
    import renet_hip as K
    sub_pred, ob_pred = net.observed_scores(obs, idx)
    s, r, o, t = facts[idx].T
    rate = gate.rate_table().detach().double().cpu().numpy()
    tab = gate.table().detach().double().cpu().numpy()
    R = RS.NUM_RELS
    grad, mag, rows, row_err = np.zeros((2, R)), np.zeros((2, R)), np.zeros((2, R), dtype=np.int64), 0.0
    for side, ent, gold, pred in ((0, s, o, ob_pred), (1, o, s, sub_pred)):
        pi = P.PairIndex(facts, side, RS.NUM_ENT)
        q, W, dq, _, _ = HS.gold_rows_decay(pi, ent, r, t, t, gold, rate[side, r], RS.NUM_ENT)
        a = np.where(W > 0, tab[side, r], 0.0)
        x = pred.double().cpu().numpy()
        ce64 = -RS.log_softmax64(x)[np.arange(len(idx)), gold]
        ce32 = K.softmax_ce(pred.clone(), i32(gold, dev), 1.0, False).double().cpu().numpy()
        row_err = max(row_err, float(np.abs(ce32 - ce64).max()))
        m = (1.0 - a) * np.exp(-ce64) + a * q
        grad[side], mag[side], rows[side] = HS.log_rate_gradient(rate[side], r, np.full(len(idx), weight), a, m, dq)
    return grad, mag, rows, row_err


def check_log_rate_gradient(name, got, want):
    grad, mag, rows, row_err = want
    got = got.double().cpu().numpy()
    bound = (4 * row_err + (rows + 4) * 2.0 ** -24) * mag
    err = np.abs(got - grad)
    live = mag > 0
    print('%s: ROW_ERR %.3e; d log_rate error / bound per (side, relation): %s; relative: %s'
          % (name, row_err, np.array2string(err[live] / bound[live], precision=3), np.array2string(err[live] / mag[live], precision=3)))
    assert row_err > 0 and np.count_nonzero(live) >= 3 and np.all(np.isfinite(got))
    assert np.all(err <= bound), (err, bound)
    assert np.all(got[~live] == 0.0)


def test_fit_gate_gradient_of_the_decay(dev):
    """Measured on the MI355X: see profiles/learned_half_life.md."""
    import recurrence as RC
    w = world(dev)
    facts, obs = w['facts'], w['obs']
    idx = late_positions(facts)
    frozen = clone_of(w['net'], dev)
    runs = []
    for learn in (True, True, False):
        gate = learned_gate(dev)
        gate.log_rate.requires_grad_(learn)
        cap = _Capture([p for p in gate.parameters() if p.requires_grad])
        losses = RC.fit_gate(frozen, obs, idx, gate, cap, steps=1)
        runs.append((losses, cap.grads[0]))
    assert len(runs[0][1]) == 2 and len(runs[2][1]) == 1 and runs[0][0] == runs[1][0] == runs[2][0]
    assert torch.equal(runs[0][1][0], runs[1][1][0]) and torch.equal(runs[0][1][1], runs[1][1][1])      # run to run
    assert torch.equal(runs[0][1][0], runs[2][1][0])                     # the gates' gradient does not see the decay's
    assert same_parameters(frozen, w['net'])
    want = log_rate_gradient_float64(w['net'], obs, facts, idx, learned_gate(dev), 1.0 / (2 * len(idx)), dev)
    check_log_rate_gradient('fit_gate', runs[0][1][1], want)
    # a gate with a fixed half-life at the same value: the same losses, the same gate gradient
    fixed = RC.CopyGate(RS.NUM_RELS, alpha=0.3, half_life=24).to(dev)
    fixed.inv_half_life = float(learned_gate(dev).rate_table().detach()[0, 0])
    cap = _Capture(fixed.parameters())
    assert RC.fit_gate(frozen, obs, idx, fixed, cap, steps=1) == runs[0][0] and torch.equal(cap.grads[0][0], runs[0][1][0])
    # one SGD step moves the decays against the gradient
    gate = learned_gate(dev)
    before = gate.log_rate.detach().clone()
    RC.fit_gate(frozen, obs, idx, gate, torch.optim.SGD(gate.parameters(), lr=0.5), steps=1)
    moved = (gate.log_rate.detach() - before).cpu().numpy()
    live = want[1] > 0
    assert np.all(np.sign(moved[live]) == -np.sign(want[0][live])) and np.all(moved[~live] == 0)


def test_learn_observed_gradient_of_the_decay(dev):
    """Measured on the MI355X: see profiles/learned_half_life.md."""
    w = world(dev)
    facts, obs = w['facts'], w['obs']
    idx = late_positions(facts)
    runs = []
    for learn in (True, True, False):
        net = clone_of(w['net'], dev)
        gate = learned_gate(dev)
        gate.log_rate.requires_grad_(learn)
        cap = _Capture([p for p in gate.parameters() if p.requires_grad])
        losses = net.learn_observed(obs, idx, hip_adam(net), prior=gate, gate_optimizer=cap)
        assert len(losses) == 1 and len(cap.grads) == 1
        runs.append((losses, cap.grads[0], net))
    assert runs[0][0] == runs[1][0] and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))   # run to run
    assert same_parameters(runs[0][2], runs[1][2]) and not same_parameters(runs[0][2], w['net'])
    # with the decay frozen: the same losses, the same model after the step, the same gate gradient -- d_q reaches the decay only
    assert runs[0][0] == runs[2][0] and same_parameters(runs[0][2], runs[2][2]) and torch.equal(runs[0][1][0], runs[2][1][0])
    want = log_rate_gradient_float64(w['net'], obs, facts, idx, learned_gate(dev), 1.0 / len(idx), dev)
    check_log_rate_gradient('learn_observed', runs[0][1][1], want)
    # the decay is a gate parameter: an SGD step of the gate optimizer moves it, the model's step is the same
    net = clone_of(w['net'], dev)
    gate = learned_gate(dev)
    net.learn_observed(obs, idx, hip_adam(net), prior=gate, gate_optimizer=torch.optim.SGD(gate.parameters(), lr=0.5))
    moved = (gate.log_rate.detach().cpu() - learned_gate(dev).log_rate.detach().cpu()).numpy()
    live = want[1] > 0
    assert np.all(np.sign(moved[live]) == -np.sign(want[0][live])) and same_parameters(net, runs[0][2])


def test_head_function_returns_the_gradient_of_q(dev):
    """HeadCEFn with copy_q requiring grad: d_q = -up * grad_scale * a / m against float64 autograd; None's place otherwise."""
    import graph as G
    import ops
    from test_gpu_copy_gate import head_case
    p, ia, ic, tgt, a, q, kind = head_case()
    t64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}
    q64 = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    feat = torch.cat((t64['ent'][ia.astype(np.int64)], t64['h'], t64['rel'][ic.astype(np.int64)]), dim=1)
    pg = torch.softmax(feat @ t64['w'].t() + t64['bias'], dim=1)[torch.arange(len(tgt)), torch.from_numpy(tgt.astype(np.int64))]
    a64 = torch.tensor(a, dtype=torch.float64)
    m = (1 - a64) * pg + a64 * q64
    live = (m > 1e-30).detach()
    (-torch.log(m[live])).sum().div(len(tgt)).mul(0.7).backward()
    want = q64.grad.numpy()

    def plan(idx):
        sp = G.SegPlan.host(idx.astype(np.int64))
        for f in ('order', 'seg_ptr', 'target'):
            setattr(sp, f, torch.from_numpy(getattr(sp, f)).to(dev))
        return sp
    t = {k: torch.nn.Parameter(_to(v, dev)) for k, v in p.items()}
    qt = _to(q, dev).requires_grad_(True)
    loss = ops.HeadCEFn.apply(t['ent'], _to(ia, dev), t['h'], t['rel'], _to(ic, dev), t['w'], t['bias'], _to(tgt, dev),
                              plan(ia), plan(ic), 0.0, 12345, 1.0, _to(a, dev), qt)
    (loss * 0.7).backward()
    got = qt.grad.double().cpu().numpy()
    underflow = (kind == 3) & (q == 0)                                  # p_g = 0 in fp32 and no prior mass: m = 0 is not divided by
    live = live.numpy() & ~underflow
    assert np.all(np.isfinite(got)) and np.all(got[a == 0] == 0.0) and np.all(got[underflow] == 0.0) and underflow.any()
    assert np.count_nonzero(got) > len(tgt) // 2
    np.testing.assert_allclose(got[live], want[live], rtol=1e-4, atol=0)


# ---- 5. evaluation and events --------------------------------------------------------------------------------------------
def test_a_frozen_learned_decay_equals_the_fixed_gate(dev):
    import recurrence as RC
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    gate = learned_gate(dev)
    gate.log_rate.requires_grad_(False)
    fixed = RC.CopyGate(RS.NUM_RELS, alpha=0.3, half_life=24).to(dev)
    rate = gate.rate_table().cpu().numpy()
    assert rate.dtype == np.float32 and np.all(rate == rate[0, 0])
    fixed.inv_half_life = float(rate[0, 0])
    pos = late_positions(facts)[:40]
    qs = model_queries(facts)

    def results(p):
        return net.evaluate_observed(obs, pos, prior=p), RC.evaluate(obs, qs, p), net.forecast_topk(obs, qs, k=7, prior=p)

    x, y = results(gate), results(fixed)
    assert all(np.array_equal(x[k][0][name], y[k][0][name]) for k in (0, 1) for name in SETTINGS)
    assert all(np.array_equal(x[k][1], y[k][1]) for k in (0, 1))
    assert all(torch.equal(u, v) for name in ('sub', 'ob') for u, v in zip(x[2][name], y[2][name]))
    # another decay per relation does move the numbers
    with torch.no_grad():
        gate.log_rate[:, RS.HOT_R] = float(np.log(1.0 / 3.0))
    z = net.evaluate_observed(obs, pos, prior=gate)
    assert not np.array_equal(z[1], x[0][1])


def test_events_take_one_learned_decay_per_direction(dev):
    import recurrence as RC
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    idx = late_positions(facts)[:16]
    gate = RC.CopyGate(RS.NUM_RELS, alpha=0.3, half_life=24, per_relation=False, learn_half_life=True).to(dev)
    with torch.no_grad():
        gate.log_rate[1, 0] = float(np.log(1.0 / 100.0))
        gate.logit[1, 0] = 1.5
    alpha, rate = RC.event_scalars(gate)
    assert rate['ob'] != rate['sub'] and alpha['ob'] != alpha['sub']
    tab = gate.rate_table().detach().cpu().numpy()
    assert rate == {'ob': float(tab[0, 0]), 'sub': float(tab[1, 0])} and RC.event_alphas(gate) == alpha
    got = net.evaluate_events_observed(obs, idx, prior=gate)
    for col, name in ((1, 'ob'), (0, 'sub')):
        prior = RC.RecurrencePrior(alpha[name], 24)
        prior.inv_half_life = rate[name]
        want = net.evaluate_events_observed(obs, idx, prior=prior)
        for kind in ('pair', 'relation'):
            assert all(np.array_equal(got[kind][s][:, col], want[kind][s][:, col]) for s in SETTINGS), (kind, name)
        assert np.array_equal(got['logp'][:, col], want['logp'][:, col])
        base = RC.evaluate_events(obs, idx, gate), RC.evaluate_events(obs, idx, prior)
        assert np.array_equal(base[0]['logp'][:, col], base[1]['logp'][:, col])
    per_rel = learned_gate(dev)
    with pytest.raises(ValueError, match='per-relation'):
        net.evaluate_events_observed(obs, idx, prior=per_rel)
    with pytest.raises(ValueError, match='per-relation'):
        RC.evaluate_events(obs, idx, per_rel)


# ---- 6. today's path -----------------------------------------------------------------------------------------------------
def test_a_fixed_half_life_makes_todays_launches(dev, monkeypatch):
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    facts, obs = w['facts'], w['obs']
    idx = late_positions(facts)
    calls = []
    for name in ('recurrence_gold_rows', 'recurrence_gold_rows_decay', 'recurrence_mix_rows_gated', 'recurrence_mix_rows_decay'):
        monkeypatch.setattr(K, name, (lambda fn, name: lambda *x, **k: (calls.append(name), fn(*x, **k))[1])(getattr(K, name), name))
    net = clone_of(w['net'], dev)
    gate = RC.CopyGate(RS.NUM_RELS, alpha=0.3, half_life=24).to(dev)
    assert list(gate.state_dict()) == ['logit']
    net.learn_observed(obs, idx, hip_adam(net), prior=gate, gate_optimizer=torch.optim.SGD(gate.parameters(), lr=0.1))
    RC.fit_gate(net, obs, idx, gate, torch.optim.SGD(gate.parameters(), lr=0.1), steps=1)
    net.evaluate_observed(obs, idx[:16], prior=gate)
    assert calls.count('recurrence_gold_rows') == 4 and calls.count('recurrence_mix_rows_gated') == 2
    assert 'recurrence_gold_rows_decay' not in calls and 'recurrence_mix_rows_decay' not in calls
    del calls[:]
    learned = learned_gate(dev)
    net.learn_observed(obs, idx, hip_adam(net), prior=learned, gate_optimizer=torch.optim.SGD(learned.parameters(), lr=0.1))
    net.evaluate_observed(obs, idx[:16], prior=learned)
    assert calls == ['recurrence_gold_rows_decay'] * 2 + ['recurrence_mix_rows_decay'] * 2


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(dev, monkeypatch):
    import model as M
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    with pytest.raises(ValueError, match='half_life'):
        RC.CopyGate(RS.NUM_RELS, alpha=0.3, learn_half_life=True)
    # the C entries: a missing array, C beyond the limit -- nothing is written
    n, C = 8, RS.NUM_ENT
    ent, rel, t = (i32(facts[:n, k], dev) for k in (0, 1, 3))
    (p_rel, p_other, p_t), ent_ptr, snap_ptr, num_ent = role_args(store, 0)
    ihl, a = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    outs = [torch.full((n,), 7.0, device=dev) for _ in range(3)]
    rows = torch.full((n, C), 7.0, device=dev)
    ptr = lambda v: None if v is None else v.data_ptr()
    L, st = K.lib(), K._stream()
    front = (ptr(p_rel), ptr(p_other), ptr(p_t), int(p_rel.numel()), ptr(ent_ptr), ptr(snap_ptr), int(snap_ptr.numel()) - 1, num_ent)

    def gold(ihl_, dq_, C_):
        return L.renet_recurrence_gold_rows_decay(ptr(ent), ptr(rel), ptr(t), ptr(t), ptr(ent), n, *front, C_, ptr(ihl_),
                                                  ptr(outs[0]), ptr(outs[1]), ptr(dq_), st)

    def mix(a_, ihl_, C_, ld):
        return L.renet_recurrence_mix_rows_decay(ptr(ent), ptr(rel), ptr(t), ptr(t), n, *front, None, ld, C_, ptr(a_), ptr(ihl_),
                                                 ptr(rows), None, None, st)
    assert gold(None, outs[2], C) != 0 and gold(ihl, None, C) != 0 and gold(ihl, outs[2], K.RECURRENCE_MAX_C + 1) != 0
    assert gold(ihl, outs[2], 0) != 0
    assert mix(a, None, C, C) != 0 and mix(None, ihl, C, C) != 0 and mix(a, ihl, K.RECURRENCE_MAX_C + 1, C) != 0
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((rows == 7.0).all())
    # the wrappers: a decay per row, float32, finite and >= 0
    for bad in (ihl[:3], ihl.double(), None):
        with pytest.raises(K.RenetHipError):
            K.recurrence_gold_rows_decay(ent, rel, t, t, ent, (p_rel, p_other, p_t), ent_ptr, snap_ptr, num_ent, C, bad)
        with pytest.raises(K.RenetHipError):
            K.recurrence_mix_rows_decay(ent, rel, t, t, (p_rel, p_other, p_t), ent_ptr, snap_ptr, num_ent, None, a, bad, num_cols=C)
    for bad in (-0.5, float('nan'), float('inf')):
        with pytest.raises(K.RenetHipError):
            K.recurrence_mix_rows_decay(ent, rel, t, t, (p_rel, p_other, p_t), ent_ptr, snap_ptr, num_ent, None, a,
                                        torch.full((n,), bad, device=dev), num_cols=C)
    # a NaN log_rate is refused by check(), wherever the gate is used
    idx = late_positions(facts)[:16]
    net = clone_of(w['net'], dev)
    gate = learned_gate(dev)
    good = RC.CopyRows(store, idx, gate)
    _, prep = M._observed_prepared(net, store, (idx, net.prepare_both_device(idx, store)))
    calls = []
    for name in ('recurrence_gold_rows_decay', 'recurrence_mix_rows_decay', 'recurrence_gold_rows', 'recurrence_mix_rows_gated',
                 'mix_ce', 'mix_ce_planes'):
        monkeypatch.setattr(K, name, lambda *x, **k: calls.append(1))
    with torch.no_grad():
        gate.log_rate[1, 2] = float('nan')
    one = RC.CopyGate(RS.NUM_RELS, half_life=24, per_relation=False, learn_half_life=True).to(dev)
    with torch.no_grad():
        one.log_rate[0, 0] = float('inf')
    for call in (lambda: net.evaluate_observed(w['obs'], idx, prior=gate), lambda: RC.CopyRows(store, idx, gate),
                 lambda: net.learn_observed(w['obs'], idx, hip_adam(net), prior=gate,
                                            gate_optimizer=torch.optim.SGD(gate.parameters(), lr=0.1)),
                 lambda: RC.fit_gate(net, w['obs'], idx, gate, torch.optim.SGD(gate.parameters(), lr=0.1)),
                 lambda: RC.event_scalars(one), lambda: net.evaluate_events_observed(w['obs'], idx, prior=one)):
        with pytest.raises(ValueError):
            call()
    # a sharded batch, and bf16-storage mode
    monkeypatch.setattr(K, 'concat3_fwd', lambda *x, **k: calls.append(1))
    prep.sharded = True
    with pytest.raises(ValueError):
        net.loss_prepared_both(prep, copy=good)
    prep.sharded = False
    monkeypatch.setattr(K, 'GEMM_MODE', 'bf16s')
    with pytest.raises(ValueError):
        net.loss_prepared_both(prep, copy=good)
    with pytest.raises(ValueError):
        net.learn_observed(w['obs'], idx, hip_adam(net), prior=learned_gate(dev))
    assert calls == []
