"""GPU tests of training through the JOINT copy mix (run with -m gpu on an MI355X): renet_joint_gold_rows(_decay),
renet_joint_mix_ce(_planes), the event_a / event_q inputs of ops.DualHeadCEFn, RENet.loss_prepared_both(event_copy=),
recurrence.EventCopyRows / fit_event_gate and the event_prior= keyword of learn_observed.  The stream, the models and the
resident store are those of tests/test_gpu_recurrence.py (made once, shared, left unchanged; whatever trains does so on
clones); the float64 statement is tests/event_gate_statement.py.

Bounds.  W is exact (the mass kernel's bits, rounded once); q is one fp64-to-fp32 rounding of G / W, whose fp64 sums differ
from the statement's by summation order only; dq = -ln2 (GD W - G WD) / W^2 is a difference of two products of such sums:
one rounding of the result, 2^-24 |dq|, and the order errors of a few hundred terms, n 2^-53 of ln2 (GD W + G WD) / W^2 <=
2 ln2 Dmax q -- far below 2^-24 q for the lags of this stream: 2^-22 (|dq| + |q|) holds both with room.
The joint loss, its gradient and s are held to FOUR times the largest error of the parent's renet_softmax_ce against float64
on the same logits, measured in the same test (the convention of tests/test_gpu_copy_gate.py); d_a as there, relative to
|d_a| + grad_scale.  With a = 0 the kernel computes fl(A - fl(x_g + lp)) where the parent computes fl(A - x_g): the parent's
error plus one rounding of the sum x_g + lp and one of the result."""
import numpy as np
import pytest
import torch

import event_gate_statement as ES
import recurrence_statement as RS
from test_gpu_copy_gate import (SHAPES, _Capture, _to, ce_case, gold_queries, head_case, hip_adam, late_positions, mixed_rows,
                                role_args, strided)
from test_gpu_event_prior import mix_store
from test_gpu_online_learning import clone_of, same_parameters
from test_gpu_parity import ATOL, RTOL
from test_gpu_recurrence import i32, world

pytestmark = pytest.mark.gpu

R, N = RS.NUM_RELS, RS.NUM_ENT


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


# ---- 1. gold rows ------------------------------------------------------------------------------------------------------
def event_gold_queries(facts, role, stale):
    """gold_queries of tests/test_gpu_copy_gate.py and, behind them, the hot pair with a relation of -1 and of R and a BARE
    ENTITY (gold_queries' bare row is a bare PAIR: its entity has facts under other relations, so W > 0 here)."""
    ent, rel, t, as_of, gold = gold_queries(facts, role, stale)
    hot = (RS.HOT_S, RS.HOT_O) if role == 0 else (RS.HOT_O, RS.HOT_S)
    end = int(facts[:, 3].max())
    add = lambda x, v: np.concatenate((x, np.asarray(v, dtype=np.int64)))
    never = RS.NEVER_SUBJECT[0] if role == 0 else RS.NEVER_OBJECT[0]
    return (add(ent, [hot[0]] * 2 + [never]), add(rel, [-1, R, 0]), add(t, [end] * 3), add(as_of, [end - stale * RS.STEP] * 3),
            add(gold, [hot[1]] * 2 + [3]))


@pytest.mark.parametrize('stale', [0, 2])
@pytest.mark.parametrize('half_life', [None, 24])
@pytest.mark.parametrize('role', [0, 1])
def test_gold_rows_equal_the_mass_kernels_w_and_the_float64_q(dev, role, half_life, stale):
    import preprocess as P
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    ihl = RC.RecurrencePrior(0.5, half_life).inv_half_life
    ent, rel, t, as_of, gold = event_gold_queries(facts, role, stale)
    n = len(ent)
    args = [i32(x, dev) for x in (ent, rel, t, as_of, gold)]
    q, W = K.joint_gold_rows(*args, *role_args(store, role), R, N, ihl)
    # W: fp32(mass) of a renet_joint_mix_rows call on the same groups, bit for bit
    C = 64
    _, _, mass = mix_store(store, role, (ent, t, as_of), torch.zeros(n * R, C, device=dev), torch.zeros(n * R, device=dev), 0.0, ihl)
    assert torch.equal(W, mass.float())
    pi = P.PairIndex(facts, role, N)
    q64, W64, dq64, G64, _, _ = ES.gold_rows(pi, ent, rel, t, as_of, gold, ihl, R, N)
    got = q.double().cpu().numpy()
    assert np.all(np.abs(got - q64) <= 2.0 ** -23 * q64) and np.array_equal(got == 0, q64 == 0)
    assert np.array_equal(W.cpu().numpy() == 0, W64 == 0)
    if half_life is None:
        assert np.array_equal(q.cpu().numpy(), np.where(W64 > 0, G64 / np.maximum(W64, 1), 0).astype(np.float32))   # fp32(G / W)
        assert np.array_equal(W.cpu().numpy(), W64.astype(np.float32))
    # the census
    m = n - 3
    hot_row, bare_pair, absent, beyond, late, bad_rel, bare_row = m - 8, m - 6, (m - 5, m - 4), (m - 3, m - 2), m - 1, (n - 3, n - 2), n - 1
    assert W64[hot_row] > (256 if (role, half_life) == (0, None) else 0) and q64[hot_row] > 0   # a run longer than a workgroup
    assert W64[bare_row] == 0 and got[bare_row] == 0 and q64[bare_pair] == 0 and got[bare_pair] == 0
    assert all(W64[i] == 0 and got[i] == 0 for i in absent)
    assert all(W64[i] > 0 and got[i] == 0 for i in beyond + bad_rel)
    assert W64[late] > 0 and got[late] == 0
    assert np.count_nonzero(q64) >= 10
    # the decay entry with a constant ihl_row: the scalar entry's bits, and dq
    q2, W2, dq = K.joint_gold_rows_decay(*args, *role_args(store, role), R, N, torch.full((n,), ihl, device=dev))
    assert torch.equal(q, q2) and torch.equal(W, W2)
    dqg = dq.double().cpu().numpy()
    err = np.abs(dqg - dq64)
    print('joint_gold_rows role %d half_life %r stale %d: q err %.3e of q, dq err %.3e of |dq| + |q| (%d rows with dq != 0)'
          % (role, half_life, stale, float(np.max(np.abs(got - q64)[q64 > 0] / q64[q64 > 0])),
             float(np.max(err[q64 > 0] / (np.abs(dq64) + q64)[q64 > 0])), np.count_nonzero(dqg)))
    assert np.all(err <= 2.0 ** -22 * (np.abs(dq64) + np.abs(q64)))
    assert np.all(dqg[(G64 == 0) | (W64 == 0) | (got == 1)] == 0.0) and np.count_nonzero(dqg) >= 5
    # run to run
    q3, W3, dq3 = K.joint_gold_rows_decay(*args, *role_args(store, role), R, N, torch.full((n,), ihl, device=dev))
    q4, W4 = K.joint_gold_rows(*args, *role_args(store, role), R, N, ihl)
    assert torch.equal(q, q3) and torch.equal(W, W3) and torch.equal(dq, dq3) and torch.equal(q, q4) and torch.equal(W, W4)


# ---- 2. the writers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,c', SHAPES)
def test_a_zero_lp_is_the_copy_mix_and_a_zero_gate_the_cross_entropy(dev, b, c):
    import renet_hip as K
    rng, x, t = ce_case(dev, b, c)
    x, a, q, kind = mixed_rows(rng, x, t)
    gs = 2.0 / b
    r16 = (b + 15) & ~15
    tt, at, qt = _to(t, dev), _to(a, dev), _to(q, dev)
    zero = torch.zeros(b, device=dev)
    logits = strided(x, dev)
    # lp_row = 0: renet_mix_ce(_planes), bit for bit
    loss_m, dl_m, da_m = K.mix_ce_planes(logits, tt, at, qt, gs)
    loss_j, dl_j, da_j, s_j = K.joint_mix_ce_planes(logits, tt, at, qt, zero, gs)
    assert torch.equal(loss_m.view(torch.int32), loss_j.view(torch.int32)) and torch.equal(da_m.view(torch.int32), da_j.view(torch.int32))
    pm, pj = K.planes_to_dense(dl_m), K.planes_to_dense(dl_j)
    assert torch.equal(pm[:, :r16].view(torch.int32), pj[:, :r16].view(torch.int32))
    f_m, f_j = _to(x, dev).clone(), _to(x, dev).clone()
    l_m, d_m = K.mix_ce(f_m, tt, at, qt, gs, True)
    l_j, d_j, s_f = K.joint_mix_ce(f_j, tt, at, qt, zero, gs, True)
    assert torch.equal(l_m.view(torch.int32), l_j.view(torch.int32)) and torch.equal(d_m.view(torch.int32), d_j.view(torch.int32))
    assert torch.equal(f_m.view(torch.int32), f_j.view(torch.int32))                     # (s_j and s_f come from two writers' sums)
    assert np.array_equal(logits.cpu().numpy(), x)
    # the existing entries keep their bits next to the parent's CE where a = 0 (checked, not assumed)
    loss_c, dl_c = K.softmax_ce_planes(logits, tt, gs)
    loss_0, dl_0, _ = K.mix_ce_planes(logits, tt, zero, qt, gs)
    assert torch.equal(loss_c, loss_0)
    assert torch.equal(K.planes_to_dense(dl_c)[:, :r16].view(torch.int32), K.planes_to_dense(dl_0)[:, :r16].view(torch.int32))
    # a_row = 0: the CE's gradient bits, L = CE - lp
    lp = rng.uniform(-8.0, 0.0, b).astype(np.float32)
    lpt = _to(lp, dev)
    f_c = _to(x, dev).clone()
    ce32 = K.softmax_ce(f_c, tt, gs, True).double().cpu().numpy()
    ce64, _, _, _, _ = ES.joint_mix_ce_lp(x, t, np.zeros(b), np.zeros(b), np.zeros(b))
    err_loss = float(np.abs(ce32 - ce64).max())
    loss_a, dl_a, da_a, s_a = K.joint_mix_ce_planes(logits, tt, zero, qt, lpt, gs)
    assert torch.equal(K.planes_to_dense(dl_c)[:, :r16].view(torch.int32), K.planes_to_dense(dl_a)[:, :r16].view(torch.int32))
    f_a = _to(x, dev).clone()
    loss_f, _, s_fa = K.joint_mix_ce(f_a, tt, zero, qt, lpt, gs, True)
    assert torch.equal(f_a.view(torch.int32), f_c.view(torch.int32))
    assert bool((s_a == 1).all()) and bool((s_fa == 1).all())
    want = ce64 - lp.astype(np.float64)
    xg = x[np.arange(b), t].astype(np.float64)
    bound = err_loss + 2.0 ** -24 * (np.abs(xg + lp) + np.abs(want))
    for name, loss in (('planes', loss_a), ('fp32', loss_f)):
        e = np.abs(loss.double().cpu().numpy() - want)
        print('joint_mix_ce a = 0 %s %dx%d: |L - (CE - lp)| %.3e (parent %.3e)' % (name, b, c, float(e.max()), err_loss))
        assert np.all(e <= bound), name


def joint_rows(rng, x, t):
    """mixed_rows() with lp drawn from [-8, 0], and lp = -120 (the product p_g pr underflows in fp32) in the rows i with i % 8
    == 6 (kind 2: q = 1) and i % 16 == 5 (kind 1: q = 0).  The rows i % 8 == 2 are BALANCED: the gold logit is put within 1 of
    the logsumexp of the others (p_g in 0.27 .. 0.73), lp in [-1, 0], q in [0.1, 0.3] and a in [0.4, 0.8], so that both terms of m count and s
    lies in 0.07 .. 0.92 -- in the other mixed rows s is 1e-4 and below, and an absolute bound says little about it.
    -> (x, a, q, lp, kind, under): under marks a product that is 0 in fp32."""
    x, a, q, kind = mixed_rows(rng, x, t)
    b = x.shape[0]
    i = np.arange(b)
    lp = rng.uniform(-8.0, 0.0, b).astype(np.float32)
    low = (i % 8 == 6) | (i % 16 == 5)
    lp[low] = -120.0
    for k in np.nonzero(i % 8 == 2)[0]:
        others = np.delete(x[k], t[k]).astype(np.float64)
        x[k, t[k]] = np.float32(others.max() + np.log(np.exp(others - others.max()).sum()) + rng.uniform(-1.0, 1.0))
        lp[k], q[k], a[k] = rng.uniform(-1.0, 0.0), rng.uniform(0.1, 0.3), rng.uniform(0.4, 0.8)
    return x, a, q, lp, kind, low | (kind == 3)


@pytest.mark.parametrize('b,c', SHAPES)
def test_joint_rows_in_one_group_against_float64(dev, b, c):
    """Measured on the MI355X: see profiles/event_gate.md (the figures are printed by this test)."""
    import renet_hip as K
    rng, x, t = ce_case(dev, b, c)
    x, a, q, lp, kind, under = joint_rows(rng, x, t)
    gs = 2.0 / b
    tt, at, qt, lpt = _to(t, dev), _to(a, dev), _to(q, dev), _to(lp, dev)
    f_c = _to(x, dev).clone()
    ce32 = K.softmax_ce(f_c, tt, gs, True).double().cpu().numpy()
    grad32 = f_c.double().cpu().numpy()
    zeros = np.zeros(b)
    ce64, grad64, _, _, _ = ES.joint_mix_ce_lp(x, t, zeros, zeros, zeros)
    err_loss, err_grad = float(np.abs(ce32 - ce64).max()), float(np.abs(grad32 - gs * grad64).max())
    assert err_loss > 0 and err_grad > 0
    logits = strided(x, dev)
    loss_c, dl_c = K.softmax_ce_planes(logits, tt, gs)
    loss_p, dl_p, da_p, s_p = K.joint_mix_ce_planes(logits, tt, at, qt, lpt, gs)
    f_m = _to(x, dev).clone()
    loss_f, da_f, s_f = K.joint_mix_ce(f_m, tt, at, qt, lpt, gs, True)
    assert np.array_equal(logits.cpu().numpy(), x)                                      # the logits are untouched
    r16 = (b + 15) & ~15
    pc, pm = K.planes_to_dense(dl_c).cpu().numpy(), K.planes_to_dense(dl_p).cpu().numpy()
    assert np.all(np.isfinite(pm[:, :r16]))
    assert np.all(pm[:, :b, c:] == 0.0) and np.all(pm[:, b:r16, :] == 0.0)               # column and row padding
    rec = pm[0, :b, :c].astype(np.float64) + pm[1, :b, :c] + pm[2, :b, :c]
    ref_loss, ref_grad, ref_da, _, ref_s = ES.joint_mix_ce_lp(x, t, lp, a, q)
    a64, lp64 = a.astype(np.float64), lp.astype(np.float64)
    xg = x[np.arange(b), t].astype(np.float64)
    for name, loss, grad, da, s, ce in (('planes', loss_p, rec, da_p, s_p, loss_c.double().cpu().numpy()),
                                        ('fp32', loss_f, f_m.double().cpu().numpy(), da_f, s_f, ce32)):
        loss, da, s = (v.double().cpu().numpy() for v in (loss, da, s))
        assert all(np.all(np.isfinite(v)) for v in (loss, da, s, grad)), name
        # a = 0 or q = 0: s = 1 exactly, the CE gradient bit for bit, L = (CE - lp) - log1p(-a)
        plain = (q == 0) | (a == 0)
        assert np.all(s[plain] == 1.0), name
        if name == 'planes':
            assert np.array_equal(pm[:, :b][:, plain].view(np.int32), pc[:, :b][:, plain].view(np.int32))
        else:
            assert np.array_equal(grad[plain], grad32[plain])
        l1p = np.log1p(-a64[plain])
        want = ce64[plain] - lp64[plain] - l1p
        bound = err_loss + 2.0 ** -24 * (np.abs(xg + lp64)[plain] + np.abs(ce64 - lp64)[plain]) + 2.0 ** -23 * np.abs(l1p) + \
            2.0 ** -24 * np.abs(want)
        assert np.all(np.abs(loss[plain] - want) <= bound), name
        assert np.all(da[plain & under] == 0.0), name                                    # a product of 0 is not divided by
        # the product is 0 with prior mass: the copy term carries the row
        dead = under & ~plain
        if dead.any():
            want = -np.log(a64[dead] * q[dead].astype(np.float64))
            assert np.all(grad[dead] == 0.0) and np.all(s[dead] == 0.0), name
            assert np.all(np.abs(loss[dead] - want) <= 2.0 ** -23 * (np.abs(want) + 1.0)), name
        # the remaining rows: four times the parent's own error
        rest = ~plain & ~dead
        e_s = float(np.abs(s - ref_s).max())
        assert e_s <= 4 * err_loss, (name, e_s)
        balanced = np.arange(b) % 8 == 2
        assert np.all((ref_s[balanced] > 0.05) & (ref_s[balanced] < 0.95)) and np.all(rest[balanced]), name
        if rest.any():
            e_l = float(np.abs(loss[rest] - ref_loss[rest]).max())
            e_g = float(np.abs(grad[rest] - gs * ref_grad[rest]).max())
            e_a = float((np.abs(da[rest] - gs * ref_da[rest]) / (np.abs(gs * ref_da[rest]) + gs)).max())
            print('joint_mix_ce %s %dx%d: parent loss %.3e grad %.3e | joint loss %.3e grad %.3e d_a (rel) %.3e s %.3e'
                  % (name, b, c, err_loss, err_grad, e_l, e_g, e_a, e_s))
            assert e_l <= 4 * err_loss and e_g <= 4 * err_grad and e_a <= 4 * err_loss, name


# ---- 3. the head Function ----------------------------------------------------------------------------------------------
def dual_case():
    p, ia, ic, tgt, a, q, kind = head_case()
    rng = np.random.RandomState(9)
    b, d = p['h'].shape
    p = dict(p, h2=rng.uniform(-1, 1, (b, d)).astype(np.float32), w2=rng.uniform(-.3, .3, (R, 2 * d)).astype(np.float32),
             b2=rng.uniform(-.1, .1, R).astype(np.float32))
    q[kind == 4] = rng.uniform(2e-6, 2e-5, int((kind == 4).sum())).astype(np.float32)   # near p_g pr of a general row: s mid-range
    return p, ia, ic, tgt, rng.randint(0, R, b).astype(np.int32), a, q, kind


NAMES = ('ent', 'rel', 'w', 'bias', 'h', 'h2', 'w2', 'b2')


def dual_float64(p, ia, ic, tgt, tgt2, a, q, up):
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    at, qt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (a, q))
    e = t['ent'][ia.astype(np.int64)]
    rows = torch.arange(len(tgt))
    lp1 = torch.log_softmax(torch.cat((e, t['h'], t['rel'][ic.astype(np.int64)]), dim=1) @ t['w'].t() + t['bias'], dim=1)
    lp2 = torch.log_softmax(torch.cat((e, t['h2']), dim=1) @ t['w2'].t() + t['b2'], dim=1)
    pj = torch.exp(lp1[rows, torch.from_numpy(tgt.astype(np.int64))] + lp2[rows, torch.from_numpy(tgt2.astype(np.int64))])
    loss = (-torch.log((1 - at) * pj + at * qt)).mean()
    (loss * up).backward()
    return [loss.item()] + [t[k].grad.numpy() for k in NAMES] + [at.grad.numpy(), qt.grad.numpy()]


def dual_apply(dev, p, ia, ic, tgt, tgt2, up, **kw):
    import graph as G
    import ops
    t = {k: torch.nn.Parameter(_to(v, dev)) for k, v in p.items()}

    def plan(idx):
        sp = G.SegPlan.host(idx.astype(np.int64))
        for f in ('order', 'seg_ptr', 'target'):
            setattr(sp, f, torch.from_numpy(getattr(sp, f)).to(dev))
        return sp
    extra = {'loss_scale': 1.0, 'rel_weight': 0.1, 'row_tap': None, 'copy_a': None, 'copy_q': None, 'event_a': None, 'event_q': None}
    extra.update(kw)
    loss = ops.DualHeadCEFn.apply(t['ent'], _to(ia, dev), t['h'], t['rel'], _to(ic, dev), t['w'], t['bias'], _to(tgt, dev),
                                  t['h2'], t['w2'], t['b2'], _to(tgt2, dev), plan(ia), plan(ic), 0.0, 12345, 12346,
                                  *[extra[k] for k in ('loss_scale', 'rel_weight', 'row_tap', 'copy_a', 'copy_q', 'event_a', 'event_q')])
    (loss * up).backward()
    torch.cuda.synchronize()
    return loss, t


@pytest.mark.parametrize('planes', [True, False], ids=['planes', 'in-loop'])
def test_dual_head_function_with_event_arrays_against_float64(dev, planes):
    import renet_hip as K
    p, ia, ic, tgt, tgt2, a, q, kind = dual_case()
    want = dual_float64(p, ia, ic, tgt, tgt2, a, q, 0.7)
    old = K.PLANES
    K.PLANES = planes
    try:
        at, qt = _to(a, dev).requires_grad_(True), _to(q, dev).requires_grad_(True)
        tap = []
        loss, t = dual_apply(dev, p, ia, ic, tgt, tgt2, 0.7, event_a=at, event_q=qt, row_tap=tap)
        got = [loss.item()] + [t[k].grad.cpu().numpy() for k in NAMES] + [at.grad.cpu().numpy(), qt.grad.cpu().numpy()]
        # event_a = 0: the parameter gradients of DualHeadCEFn(rel_weight=1.0), bit for bit
        _, t0 = dual_apply(dev, p, ia, ic, tgt, tgt2, 0.7, event_a=torch.zeros(len(a), device=dev), event_q=_to(q, dev))
        _, t1 = dual_apply(dev, p, ia, ic, tgt, tgt2, 0.7, rel_weight=1.0)
        for k in NAMES:
            assert torch.equal(t0[k].grad.view(torch.int32), t1[k].grad.view(torch.int32)), k
    finally:
        K.PLANES = old
    assert abs(got[0] - want[0]) <= 1e-4 * abs(want[0]) + 1e-6
    rows, s1, s2 = tap[0]
    b = len(a)
    assert s2 == 0.0 and bool((rows[b:] == 0).all()) and abs(float(rows[:b].sum()) * s1 - got[0]) <= 1e-5 * abs(got[0])
    underflow = (kind == 3) & (q == 0)                                  # p_g = 0 in fp32: d_a and d_q are written as 0, not divided
    for k in (9, 10):
        assert np.all(got[k][underflow] == 0.0) and np.all(np.isfinite(got[k]))
        got[k], want[k] = got[k][~underflow], want[k][~underflow]
    for x, y, name in zip(got[1:], want[1:], NAMES + ('d_a', 'd_q')):
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(y).max()) * 10), err_msg=name)


# ---- 4. consistency with evaluation ------------------------------------------------------------------------------------
def test_the_training_loss_is_the_evaluated_joint_log_probability(dev):
    import model as M
    import recurrence as RC
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    store = obs.device
    idx = late_positions(facts)
    idx = idx[np.random.RandomState(12).choice(len(idx), 40, replace=False)]
    prior = RC.RecurrencePrior(0.3, 100)
    ev = net.evaluate_events_observed(obs, idx, prior=prior)
    assert not net.training
    with torch.no_grad():
        _, prep = M._observed_prepared(net, store, (idx, net.prepare_both_device(idx, store)))
        rows = RC.EventCopyRows(store, idx, prior)
        tap = []
        loss = net.loss_prepared_both(prep, event_copy=rows, row_tap=tap)
    n = len(idx)
    L_rows = tap[0][0][:2 * n]
    perm = prep.g._v['perm'][:2 * n].long()
    L_seq = torch.empty_like(L_rows)
    L_seq[perm] = L_rows                                                 # sequence i: 'ob' of position i; n + i: its 'sub'
    L = L_seq.cpu().numpy()
    assert abs(float(loss) - L.sum() / n) <= 1e-5 * abs(float(loss))
    assert np.count_nonzero(rows.q_seq.cpu().numpy()) >= 10
    for name, col, part in (('ob', 1, L[:n]), ('sub', 0, L[n:])):
        print(name, 'max |L + logp|', float(np.abs(part + ev['logp'][:, col]).max()))
        np.testing.assert_allclose(part, -ev['logp'][:, col], rtol=RTOL, atol=ATOL, err_msg=name)


# ---- 5. learning -------------------------------------------------------------------------------------------------------
def test_no_event_prior_is_todays_path(dev, monkeypatch):
    import renet_hip as K
    w = world(dev)
    facts, obs = w['facts'], w['obs']
    idx = late_positions(facts)
    a, b = clone_of(w['net'], dev), clone_of(w['net'], dev)
    calls = []
    for name in ('joint_gold_rows', 'joint_gold_rows_decay', 'joint_mix_ce', 'joint_mix_ce_planes', 'recurrence_gold_rows'):
        monkeypatch.setattr(K, name, (lambda fn, name: lambda *x, **k: (calls.append(name), fn(*x, **k))[1])(getattr(K, name), name))
    la = a.learn_observed(obs, idx, hip_adam(a), steps=2)
    lb = b.learn_observed(obs, idx, hip_adam(b), steps=2, event_prior=None)
    assert calls == [] and la == lb and same_parameters(a, b) and not same_parameters(a, w['net'])


def event_gate_gradient_float64(net, obs, facts, idx, alpha):
    """d loss / d logit [2] in float64 from the eval pass's own row losses (entity and relation head, both directions): loss =
    the two directions' mean joint losses; -> (grad, mean joint loss)."""
    import preprocess as P
    _, _, rel = net.evaluate_observed(obs, idx, relation=True)
    s, r, o, t = facts[idx].T
    n = len(idx)
    grad, total = np.zeros(2), 0.0
    for side, role, col, ent, gold in ((0, 0, 1, s, o), (1, 1, 0, o, s)):
        q, W = ES.gold_rows(P.PairIndex(facts, role, N), ent, r, t, t, gold, 0.0, R, N)[:2]
        a = np.where(W > 0, alpha, 0.0)
        pj = np.exp(-(rel['entity_loss'][:, col].astype(np.float64) + rel['loss'][:, col].astype(np.float64)))
        m = (1.0 - a) * pj + a * q
        grad[side] = float(np.sum(np.where(W > 0, (pj - q) / m * a * (1.0 - a) / n, 0.0)))
        total += float(np.sum(-np.log(m))) / n
    return grad, total


def test_learning_with_an_event_gate(dev):
    import recurrence as RC
    w = world(dev)
    facts, obs = w['facts'], w['obs']
    idx = late_positions(facts)
    runs = []
    for _ in range(2):
        net = clone_of(w['net'], dev)
        gate = RC.CopyGate(R, alpha=0.3, per_relation=False).to(dev)
        cap = _Capture(gate.parameters())
        losses = net.learn_observed(obs, idx, hip_adam(net), event_prior=gate, gate_optimizer=cap)
        assert len(losses) == 1 and len(cap.grads) == 1
        runs.append((losses, cap.grads[0][0], net))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])             # bit-identical run to run
    assert same_parameters(runs[0][2], runs[1][2]) and not same_parameters(runs[0][2], w['net'])
    got = runs[0][1].double().cpu().numpy().reshape(-1)
    want, total = event_gate_gradient_float64(w['net'], obs, facts, idx, float(np.float32(0.3)))
    print('event gate gradient', got, 'float64', want, 'loss', runs[0][0][0], total)
    assert got.shape == (2,) and abs(runs[0][0][0] - total) <= 1e-4 * total
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(want).max()) * 10))
    assert list(gate.state_dict()) == ['logit']
    # a gate that learns its decay: log_rate moves
    net = clone_of(w['net'], dev)
    gate = RC.CopyGate(R, alpha=0.3, half_life=24, per_relation=False, learn_half_life=True).to(dev)
    before = gate.log_rate.detach().clone()
    net.learn_observed(obs, idx, hip_adam(net), event_prior=gate, gate_optimizer=torch.optim.Adam(gate.parameters(), lr=0.05))
    assert sorted(gate.state_dict()) == ['log_rate', 'logit'] and bool((gate.log_rate.detach() != before).all())
    assert bool(torch.isfinite(gate.log_rate).all()) and bool(torch.isfinite(gate.logit).all())


def test_fit_event_gate_lowers_the_joint_loss_and_leaves_the_model(dev):
    import recurrence as RC
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    idx = late_positions(facts)
    frozen = clone_of(net, dev)
    fit = RC.CopyGate(R, alpha=0.3, half_life=24, per_relation=False).to(dev)
    losses = RC.fit_event_gate(frozen, obs, idx, fit, torch.optim.Adam(fit.parameters(), lr=0.1), steps=20)
    print('fit_event_gate: mean joint loss %.4f -> %.4f, alpha %s' % (losses[0], losses[-1], RC.event_alphas(fit)))
    assert len(losses) == 20 and losses[-1] < losses[0] and same_parameters(frozen, net) and not frozen.training
    assert not torch.equal(fit.logit.detach(), torch.full((2, 1), float(np.log(0.3 / 0.7)), device=dev))
    # the first loss is the evaluation's: the mean of -logp of evaluate_events_observed under the initial gate
    ev = net.evaluate_events_observed(obs, idx, prior=RC.RecurrencePrior(0.3, 24))
    want = float(-ev['logp'].astype(np.float64).sum() / (2 * len(idx)))
    assert abs(losses[0] - want) <= ATOL + RTOL * abs(want)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(dev, monkeypatch):
    import model as M
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    n, C = 8, 64
    x = torch.zeros(n, C, device=dev)
    tgt, a, q, lp = torch.zeros(n, device=dev, dtype=torch.int32), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    loss, da, s = (torch.full((n,), 7.0, device=dev) for _ in range(3))
    L = K.lib()
    ptr = lambda v: v.data_ptr()
    st = K._stream()
    planes = K.planes_empty(n, C, dev)
    pl = (ptr(planes.p), planes.plane, planes.p.shape[2], planes.p.shape[1])
    # a missing lp_row (and the parent's refusals: a missing array, ld < C)
    assert L.renet_joint_mix_ce(ptr(x), ptr(tgt), ptr(a), ptr(q), None, n, C, C, 1.0, ptr(loss), None, ptr(da), ptr(s), st) != 0
    assert L.renet_joint_mix_ce(ptr(x), ptr(tgt), None, ptr(q), ptr(lp), n, C, C, 1.0, ptr(loss), None, ptr(da), ptr(s), st) != 0
    assert L.renet_joint_mix_ce(ptr(x), ptr(tgt), ptr(a), ptr(q), ptr(lp), n, C, C - 1, 1.0, ptr(loss), None, ptr(da), ptr(s), st) != 0
    assert L.renet_joint_mix_ce_planes(ptr(x), ptr(tgt), ptr(a), ptr(q), None, n, C, C, 1.0, ptr(loss), *pl, ptr(da), ptr(s), st) != 0
    assert L.renet_joint_mix_ce_planes(ptr(x), ptr(tgt), ptr(a), ptr(q), ptr(lp), n, C, C, 1.0, ptr(loss), None, *pl[1:], ptr(da),
                                       ptr(s), st) != 0
    with pytest.raises(K.RenetHipError):
        K.joint_mix_ce(x, tgt, a, q, None, 1.0, False)
    with pytest.raises(K.RenetHipError):
        K.joint_mix_ce_planes(x, tgt, a, q, None, 1.0)
    # R = 0 and R = 1025
    ent, rel, t = (i32(facts[:n, k], dev) for k in (0, 1, 3))
    tables, ent_ptr, snap_ptr, num_ent = role_args(store, 0)
    qo, Wo = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    for bad in (0, 1025):
        with pytest.raises(K.RenetHipError):
            K.joint_gold_rows(ent, rel, t, t, tgt, tables, ent_ptr, snap_ptr, num_ent, bad, N)
        assert L.renet_joint_gold_rows(ptr(ent), ptr(rel), ptr(t), ptr(t), ptr(tgt), n, *(ptr(v) for v in tables), int(tables[0].numel()),
                                       ptr(ent_ptr), ptr(snap_ptr), int(snap_ptr.numel()) - 1, num_ent, bad, N, 0.0, ptr(qo), ptr(Wo),
                                       st) != 0
        assert L.renet_joint_gold_rows_decay(ptr(ent), ptr(rel), ptr(t), ptr(t), ptr(tgt), n, *(ptr(v) for v in tables),
                                             int(tables[0].numel()), ptr(ent_ptr), ptr(snap_ptr), int(snap_ptr.numel()) - 1, num_ent,
                                             bad, N, ptr(lp), ptr(qo), ptr(Wo), ptr(da), st) != 0
    with pytest.raises(K.RenetHipError):
        K.joint_gold_rows(ent, rel, t, t, tgt[:3], tables, ent_ptr, snap_ptr, num_ent, R, N)
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in (loss, da, s, qo, Wo))    # nothing ran
    # a per-relation gate; both copy= and event_copy=; a sharded batch; bf16-storage mode
    net = clone_of(w['net'], dev)
    idx = late_positions(facts)[:16]
    per_rel = RC.CopyGate(R).to(dev)
    calls = []
    for name in ('joint_gold_rows', 'joint_gold_rows_decay', 'concat3_fwd'):
        monkeypatch.setattr(K, name, lambda *x, **k: calls.append(1))
    for fn in (lambda: RC.EventCopyRows(store, idx, per_rel),
               lambda: RC.fit_event_gate(net, w['obs'], idx, per_rel, torch.optim.SGD(per_rel.parameters(), lr=0.1)),
               lambda: net.learn_observed(w['obs'], idx, hip_adam(net), event_prior=per_rel),
               lambda: net.learn_observed(w['obs'], idx, hip_adam(net), prior=RC.RecurrencePrior(0.3), event_prior=RC.RecurrencePrior(0.3))):
        with pytest.raises(ValueError):
            fn()
    _, prep = M._observed_prepared(net, store, (idx, net.prepare_both_device(idx, store)))
    pair = (torch.zeros(2 * len(idx), device=dev), torch.zeros(2 * len(idx), device=dev))
    with pytest.raises(ValueError):
        net.loss_prepared_both(prep, copy=pair, event_copy=pair)
    prep.sharded = True
    with pytest.raises(ValueError):
        net.loss_prepared_both(prep, event_copy=pair)
    prep.sharded = False
    monkeypatch.setattr(K, 'GEMM_MODE', 'bf16s')
    with pytest.raises(ValueError):
        net.loss_prepared_both(prep, event_copy=pair)
    with pytest.raises(ValueError):
        net.learn_observed(w['obs'], idx, hip_adam(net), event_prior=RC.RecurrencePrior(0.3))
    assert calls == []


# ---- 7. the tool -------------------------------------------------------------------------------------------------------
def test_the_eval_tool_fits_and_reports_the_event_gate(dev, tmp_path):
    """tools/run_observed_eval.py --events --recurrence --half-life --fit-gate --learn-half-life on the test stream written out
    as a dataset directory (train / valid / test cut at timestamp borders) with the world's weights as checkpoints: one child
    process, which is what this test is about."""
    import json
    import os
    import subprocess
    import sys
    w = world(dev)
    facts = w['facts']
    data, models = tmp_path / 'SYN', tmp_path / 'models'
    data.mkdir(), models.mkdir()
    (data / 'stat.txt').write_text('%d %d\n' % (N, R))
    t = facts[:, 3]
    for name, part in (('train.txt', facts[t < 8 * RS.STEP]), ('valid.txt', facts[(t >= 8 * RS.STEP) & (t < 11 * RS.STEP)]),
                       ('test.txt', facts[t >= 11 * RS.STEP])):
        np.savetxt(str(data / name), part, fmt='%d', delimiter='\t')
    cpu = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
    torch.save({'state_dict': cpu(w['net'])}, str(models / 'rgcn.pth'))
    torch.save({'state_dict': cpu(w['gnet'])}, str(models / 'max1rgcn_global2.pth'))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'run_observed_eval.py'), str(data), '--n-hidden', '100',
                          '--seq-len', str(RS.SEQ_LEN), '--model-dir', str(models), '--split', 'test', '--events', '0',
                          '--recurrence', '0.3', '--half-life', '24', '--fit-gate', '3', '--learn-half-life', '--gate-lr', '0.1'],
                         capture_output=True, text=True, timeout=170)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0
    line, = [l for l in out.stdout.splitlines() if l.startswith('EVENT GATE fitted on the valid split')]
    assert '3 Adam steps at lr 0.1 from alpha 0.3, half-life 24' in line
    rec = [json.loads(l) for l in out.stdout.splitlines() if l.startswith('{') and '"task": "events"' in l][-1]
    fg = rec['fitted_gate']
    assert fg['fit_steps'] == 3 and fg['initial_alpha'] == 0.3 and fg['initial_half_life'] == 24.0 and fg['learn_half_life']
    assert all(0.0 < fg['alpha'][k] < 1.0 and fg['alpha'][k] != 0.3 and fg['half_life'][k] > 0 and fg['half_life'][k] != 24.0
               for k in ('ob', 'sub'))
    assert all(set(rec[k]) == {'pair', 'relation'} for k in ('mixed_fitted_gate', 'mixed', 'baseline', 'metrics'))
    assert 'LEARNED GATE per side and relation' not in out.stdout        # one invocation fits one gate
