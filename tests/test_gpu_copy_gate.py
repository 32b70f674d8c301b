"""GPU tests of training through the copy mix (run with -m gpu on an MI355X): renet_recurrence_gold_rows,
renet_recurrence_mix_rows_gated, renet_mix_ce / renet_mix_ce_planes, the copy= input of the head Functions,
recurrence.CopyGate / CopyRows / fit_gate and the prior= keyword of learn_observed and evaluate_online.  The stream, the
models and the resident store are those of tests/test_gpu_recurrence.py (made once, shared, left unchanged; whatever trains
does so on clones); the float64 statement is tests/copy_gate_statement.py.

Bounds.  W is exact (the mix kernel's bits); q is one fp64-to-fp32 rounding.  The mixed loss and gradient are held to FOUR
times the largest error of the PARENT's renet_softmax_ce against float64 on the same logits, measured in the same test (the
convention of ROW_BOUND = 4 * ROW_ERR in tests/test_gpu_recurrence.py; the values measured are in profiles/copy_gate.md).
d_a = grad_scale (p_g - q) / m has no parent: p_g and m carry the relative error of p_g, which IS the absolute error of the
parent's loss -log p_g, so d_a is held to 4 x that error, relative to |d_a| + grad_scale."""
import numpy as np
import pytest
import torch

import copy_gate_statement as CS
import recurrence_statement as RS
from test_gpu_online_learning import clone_of, same_parameters
from test_gpu_recurrence import ROW_BOUND, SETTINGS, i32, model_queries, stream_of_resident, world

pytestmark = pytest.mark.gpu

SHAPES = [(64, 23033), (33, 4100), (17, 2048), (9, 24576), (5, 1000), (3, 30000)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _to(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def role_args(store, role):
    return store.pair_tables()[role], store.t['ent_ptr%d' % role], store.t['snap_ptr%d' % role], store.num_ent


# ---- 1. gold rows ------------------------------------------------------------------------------------------------------
def late_gold(facts, role):
    """(ent, rel, gold, first): a pair (ent, rel) with facts before `first`, the time of gold's FIRST fact with it."""
    e_col, p_col = (0, 2) if role == 0 else (2, 0)
    first, start = {}, {}
    for f in facts.tolist():
        key = (f[e_col], f[1])
        first.setdefault(key + (f[p_col],), f[3])
        start.setdefault(key, f[3])
    for (e, r, g), t in sorted(first.items()):
        if t > start[(e, r)]:
            return e, r, g, t
    raise AssertionError('the stream has no partner that appears late in its pair')


def gold_queries(facts, role, stale):
    e_col, p_col = (0, 2) if role == 0 else (2, 0)
    rng = np.random.RandomState(31 + role)
    pick = facts[rng.choice(len(facts), 40, replace=False)]
    ent, rel, gold, t = (list(pick[:, k]) for k in (e_col, 1, p_col, 3))
    end = int(facts[:, 3].max())
    hot = (RS.HOT_S, RS.HOT_R, RS.HOT_O) if role == 0 else (RS.HOT_O, RS.HOT_R, RS.HOT_S)
    bare = (RS.BARE_S, RS.BARE_R, 3) if role == 0 else (RS.BARE_O, RS.BARE_R, 3)
    le, lr, lg, lt = late_gold(facts, role)
    for e, r, g, tt in (hot + (end + RS.STEP,), hot + (end,), bare + (end,), (-1, 0, 3, 48), (RS.NUM_ENT, 0, 3, 48),
                        (hot[0], hot[1], RS.NUM_ENT, end), (hot[0], hot[1], -1, end), (le, lr, lg, lt + stale * RS.STEP)):
        ent.append(e), rel.append(r), gold.append(g), t.append(tt)
    ent, rel, gold, t = (np.asarray(x, dtype=np.int64) for x in (ent, rel, gold, t))
    return ent, rel, t, t - stale * RS.STEP, gold


@pytest.mark.parametrize('stale', [0, 2])
@pytest.mark.parametrize('half_life', [None, 24])
@pytest.mark.parametrize('role', [0, 1])
def test_gold_rows_equal_the_mix_kernels_w_and_the_float64_q(dev, role, half_life, stale):
    import preprocess as P
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    prior = RC.RecurrencePrior(0.5, half_life)
    ent, rel, t, as_of, gold = gold_queries(facts, role, stale)
    args = [i32(x, dev) for x in (ent, rel, t, as_of)]
    q, W = K.recurrence_gold_rows(*args, i32(gold, dev), *role_args(store, role), RS.NUM_ENT, prior.inv_half_life)
    _, _, stats_w = K.recurrence_mix_rows(*args, *role_args(store, role), None, prior.alpha, prior.inv_half_life,
                                          num_cols=RS.NUM_ENT, want_stats=True)
    assert torch.equal(W, stats_w)                                                      # bit for bit
    pi = P.PairIndex(facts, role, RS.NUM_ENT)
    q64, W64 = CS.gold_rows(*pi.prior_rows(ent, rel, t, as_of, inv_half_life=prior.inv_half_life), gold, RS.NUM_ENT)
    got = q.double().cpu().numpy()
    assert np.all(np.abs(got - q64) <= 2.0 ** -23 * q64) and np.array_equal(got == 0, q64 == 0)
    assert np.array_equal(W.cpu().numpy() == 0, W64 == 0)
    n = len(ent)
    hot_row, bare_row, absent, beyond, late = n - 8, n - 6, (n - 5, n - 4), (n - 3, n - 2), n - 1
    assert W64[hot_row] > (256 if (role, half_life) == (0, None) else 0) and q64[hot_row] > 0   # the hot pair: > a workgroup
    assert W64[bare_row] == 0 and q64[bare_row] == 0                                     # a bare pair
    assert all(W64[i] == 0 and got[i] == 0 for i in absent)                              # an open side
    assert all(W64[i] > 0 and got[i] == 0 for i in beyond)                               # a gold outside [0, C)
    assert W64[late] > 0 and got[late] == 0                                              # gold's facts lie at or after as_of
    assert np.count_nonzero(q64) >= 10
    q2, W2 = K.recurrence_gold_rows(*args, i32(gold, dev), *role_args(store, role), RS.NUM_ENT, prior.inv_half_life)
    assert torch.equal(q, q2) and torch.equal(W, W2)                                     # run to run


# ---- 2. / 3. the loss through the mix ----------------------------------------------------------------------------------
def ce_case(dev, b, c):
    rng = np.random.RandomState(b * 7 + c)
    x = (rng.standard_normal((b, c)) * 3).astype(np.float32)
    t = rng.randint(0, c, b).astype(np.int32)
    t[0], t[-1] = 0, c - 1
    return rng, x, t


def strided(x, dev):
    b, c = x.shape
    buf = torch.zeros(b, (c + 3) & ~3, device=dev)
    buf[:, :c] = _to(x, dev)
    return buf[:, :c]


@pytest.mark.parametrize('b,c', SHAPES)
def test_a_zero_gate_is_the_cross_entropy_bit_for_bit(dev, b, c):
    import renet_hip as K
    rng, x, t = ce_case(dev, b, c)
    gs = 2.0 / b
    a = torch.zeros(b, device=dev)
    q = _to(rng.rand(b).astype(np.float32), dev)
    logits = strided(x, dev)
    loss_c, dl_c = K.softmax_ce_planes(logits, _to(t, dev), gs)
    loss_m, dl_m, d_a = K.mix_ce_planes(logits, _to(t, dev), a, q, gs)
    assert torch.equal(loss_c, loss_m)
    pc, pm = K.planes_to_dense(dl_c), K.planes_to_dense(dl_m)
    r16 = (b + 15) & ~15
    assert torch.equal(pc[:, :r16].view(torch.int32), pm[:, :r16].view(torch.int32))    # rows, column and row padding
    assert np.array_equal(logits.cpu().numpy(), x) and bool(torch.isfinite(d_a).all())
    f_c, f_m = _to(x, dev).clone(), _to(x, dev).clone()
    l_c = K.softmax_ce(f_c, _to(t, dev), gs, True)
    l_m, _ = K.mix_ce(f_m, _to(t, dev), a, q, gs, True)
    assert torch.equal(l_c, l_m) and torch.equal(f_c.view(torch.int32), f_m.view(torch.int32))


def mixed_rows(rng, x, t):
    """The row kinds inside every group of four rows: 0: a = 0; 1: q = 0, a > 0; 2: q = 1; 3: the gold logit 120 below the
    row's maximum (p_g = 0 in fp32), with q > 0 in the even groups and q = 0 in the odd ones.  -> (x, a, q, kind)."""
    b = x.shape[0]
    kind = np.arange(b) % 4
    a = rng.uniform(0.05, 0.95, b).astype(np.float32)
    q = rng.uniform(0.05, 0.95, b).astype(np.float32)
    a[kind == 0] = 0.0
    q[kind == 1] = 0.0
    q[kind == 2] = 1.0
    q[(kind == 3) & ((np.arange(b) // 4) % 2 == 1)] = 0.0
    x = x.copy()
    for i in np.nonzero(kind == 3)[0]:
        x[i, t[i]] = np.float32(np.delete(x[i], t[i]).max() - 120.0)
    return x, a, q, kind


@pytest.mark.parametrize('b,c', SHAPES)
def test_mixed_rows_in_one_group_against_float64(dev, b, c):
    """Measured on the MI355X (largest over the six shapes; profiles/copy_gate.md has them per shape): the parent's
    renet_softmax_ce against float64 -- loss 4.3e-6, gradient 4.2e-8; the mix over its `remaining` rows -- loss 1.0e-6,
    gradient 4.2e-8, d_a 1.2e-6 relative to |d_a| + grad_scale."""
    import renet_hip as K
    rng, x, t = ce_case(dev, b, c)
    x, a, q, kind = mixed_rows(rng, x, t)
    gs = 2.0 / b
    rows = np.arange(b)
    tt, at, qt = _to(t, dev), _to(a, dev), _to(q, dev)
    # the parent, and its error against float64 on these logits
    f_c = _to(x, dev).clone()
    ce32 = K.softmax_ce(f_c, tt, gs, True).double().cpu().numpy()
    grad32 = f_c.double().cpu().numpy()
    ce64, grad64, _ = CS.mix_ce(x, t, np.zeros(b), np.zeros(b))
    err_loss, err_grad = float(np.abs(ce32 - ce64).max()), float(np.abs(grad32 - gs * grad64).max())
    assert err_loss > 0 and err_grad > 0
    logits = strided(x, dev)
    loss_c, dl_c = K.softmax_ce_planes(logits, tt, gs)
    loss_m, dl_m, d_a = K.mix_ce_planes(logits, tt, at, qt, gs)
    f_m = _to(x, dev).clone()
    loss_f, d_a_f = K.mix_ce(f_m, tt, at, qt, gs, True)
    assert np.array_equal(logits.cpu().numpy(), x)                                      # the logits are untouched
    pc, pm = K.planes_to_dense(dl_c).cpu().numpy(), K.planes_to_dense(dl_m).cpu().numpy()
    assert np.all(np.isfinite(pm[:, :((b + 15) & ~15)]))
    assert np.all(pm[:, :b, c:] == 0.0) and np.all(pm[:, b:((b + 15) & ~15), :] == 0.0)  # column and row padding
    rec = pm[0, :b, :c].astype(np.float64) + pm[1, :b, :c] + pm[2, :b, :c]
    ref_loss, ref_grad, ref_da = CS.mix_ce(x, t, a, q)
    a64 = a.astype(np.float64)
    for name, loss, grad, da, ce in (('planes', loss_m, rec, d_a, loss_c.double().cpu().numpy()),
                                     ('fp32', loss_f, f_m.double().cpu().numpy(), d_a_f, ce32)):
        loss, da = loss.double().cpu().numpy(), da.double().cpu().numpy()
        assert np.all(np.isfinite(loss)) and np.all(np.isfinite(da)) and np.all(np.isfinite(grad)), name
        # q = 0: the CE gradient bit for bit, the CE loss minus log1p(-a) (one rounding of the difference, log1pf's own ulp)
        plain = q == 0
        if name == 'planes':
            assert np.array_equal(pm[:, :b][:, plain].view(np.int32), pc[:, :b][:, plain].view(np.int32))
        else:
            assert np.array_equal(grad[plain], grad32[plain])
        l1p = np.log1p(-a64[plain])
        want = ce[plain] - l1p                                             # (the CE loss of the same writer)
        assert np.all(np.abs(loss[plain] - want) <= 2.0 ** -24 * np.abs(want) + 2.0 ** -23 * np.abs(l1p)), name
        # p_g = 0 with prior mass: the copy term carries the row
        dead = (kind == 3) & (q > 0)
        if dead.any():
            want = -np.log(a64[dead] * q[dead].astype(np.float64))
            assert np.all(grad[dead] == 0.0) and np.all(np.abs(loss[dead] - want) <= 2.0 ** -23 * (np.abs(want) + 1.0)), name
        # the remaining rows (a = 0 with prior mass; q = 1): four times the parent's own error
        rest = ~plain & ~dead
        e_l = float(np.abs(loss[rest] - ref_loss[rest]).max())
        e_g = float(np.abs(grad[rest] - gs * ref_grad[rest]).max())
        e_a = float((np.abs(da[rest] - gs * ref_da[rest]) / (np.abs(gs * ref_da[rest]) + gs)).max())
        print('mix_ce %s %dx%d: parent loss %.3e grad %.3e | mix loss %.3e grad %.3e d_a (rel) %.3e'
              % (name, b, c, err_loss, err_grad, e_l, e_g, e_a))
        assert e_l <= 4 * err_loss and e_g <= 4 * err_grad and e_a <= 4 * err_loss, name
        assert np.all(da[(kind == 3) & plain] == 0.0), name                              # p_g = 0 is not divided by


# ---- 4. the gated mix --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C, n', [(RS.NUM_ENT, 24), (40000, 4)])
def test_gated_rows_equal_the_scalar_entry_and_the_float64_statement(dev, C, n):
    import preprocess as P
    import renet_hip as K
    from test_gpu_recurrence import row_queries
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    qr = row_queries(facts, n)
    args = [i32(a, dev) for a in qr]
    x = (3.0 * np.random.RandomState(C + 11).randn(n, C)).astype(np.float32)
    logits = _to(x, dev)
    ihl = float(np.float32(1.0 / 24.0))
    const = K.recurrence_mix_rows_gated(*args, *role_args(store, 0), logits, torch.full((n,), 0.3, device=dev), ihl)
    assert torch.equal(const, K.recurrence_mix_rows(*args, *role_args(store, 0), logits, 0.3, ihl))
    alpha = np.random.RandomState(5).uniform(0.0, 0.95, n).astype(np.float32)
    alpha[1] = 0.0
    out, _, W = K.recurrence_mix_rows_gated(*args, *role_args(store, 0), logits, _to(alpha, dev), ihl, want_stats=True)
    pi = P.PairIndex(facts, 0, RS.NUM_ENT)
    ptr, col, wts = pi.prior_rows(*qr, inv_half_life=ihl)
    ref = np.concatenate([RS.mix_rows(x[i:i + 1], C, np.asarray([0, ptr[i + 1] - ptr[i]]), col[ptr[i]:ptr[i + 1]],
                                      wts[ptr[i]:ptr[i + 1]], float(alpha[i])) for i in range(n)])
    o = out.double().cpu().numpy()
    assert np.all(np.isfinite(o)) and float(np.max(np.abs(np.expm1(o - ref)))) <= ROW_BOUND
    # the gold column agrees with what the loss is built from: (1 - a) p_g + a q, q from gold_rows
    gold = np.asarray([col[ptr[i]] if ptr[i + 1] > ptr[i] else 3 for i in range(n)], dtype=np.int64)
    q, W2 = K.recurrence_gold_rows(*args, i32(gold, dev), *role_args(store, 0), C, ihl)
    assert torch.equal(W, W2)
    a_eff = np.where(W.cpu().numpy() > 0, alpha, 0.0).astype(np.float64)
    p_g = np.exp(RS.log_softmax64(x))[np.arange(n), gold]
    m = (1.0 - a_eff) * p_g + a_eff * q.double().cpu().numpy()
    assert np.all(np.abs(np.exp(o[np.arange(n), gold]) - m) <= ROW_BOUND * m) and np.count_nonzero(q.cpu().numpy()) >= 2
    # a row without history abstains whatever its gate
    bare = 2
    assert W.cpu().numpy()[bare] == 0 and float(np.max(np.abs(np.expm1(o[bare] - RS.log_softmax64(x)[bare])))) <= ROW_BOUND


# ---- 5. the head Function ----------------------------------------------------------------------------------------------
LOW = (11, 4999)                                                        # gold columns whose bias puts them far below the rest


def head_case(b=300, d=100, n_ent=5000, seed=4):
    rng = np.random.RandomState(seed)
    p = {'ent': rng.uniform(-.5, .5, (n_ent, d)), 'rel': rng.uniform(-.5, .5, (40, d)), 'w': rng.uniform(-.1, .1, (n_ent, 3 * d)),
         'bias': rng.uniform(-.1, .1, n_ent), 'h': rng.uniform(-1, 1, (b, d))}
    p = {k: v.astype(np.float32) for k, v in p.items()}
    p['bias'][list(LOW)] = -150.0
    ia, ic = rng.randint(0, n_ent, b).astype(np.int32), rng.randint(0, 40, b).astype(np.int32)
    tgt = rng.randint(12, n_ent - 1, b).astype(np.int32)
    kind = np.arange(b) % 5                                             # the kinds of mixed_rows, and 4: a general row
    a = rng.uniform(0.05, 0.95, b).astype(np.float32)
    q = rng.uniform(0.0005, 0.05, b).astype(np.float32)
    a[kind == 0] = 0.0
    q[kind == 1] = 0.0
    q[kind == 2] = 1.0
    q[(kind == 3) & ((np.arange(b) // 5) % 2 == 1)] = 0.0
    tgt[kind == 3] = np.where((np.arange(b) // 5) % 2 == 1, LOW[0], LOW[1])[kind == 3]
    return p, ia, ic, tgt, a, q, kind


def head_float64(p, ia, ic, tgt, a, q, up):
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    at = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    feat = torch.cat((t['ent'][ia.astype(np.int64)], t['h'], t['rel'][ic.astype(np.int64)]), dim=1)
    lp = torch.log_softmax(feat @ t['w'].t() + t['bias'], dim=1)
    pg = torch.exp(lp[torch.arange(len(tgt)), torch.from_numpy(tgt.astype(np.int64))])
    loss = (-torch.log((1 - at) * pg + at * torch.tensor(q, dtype=torch.float64))).mean()
    (loss * up).backward()
    return [loss.item()] + [t[k].grad.numpy() for k in ('ent', 'rel', 'w', 'bias', 'h')] + [at.grad.numpy()]


@pytest.mark.parametrize('planes', [True, False], ids=['planes', 'in-loop'])
def test_head_function_with_copy_against_float64(dev, planes):
    import graph as G
    import ops
    import renet_hip as K
    p, ia, ic, tgt, a, q, kind = head_case()
    want = head_float64(p, ia, ic, tgt, a, q, 0.7)
    old = K.PLANES
    K.PLANES = planes
    try:
        t = {k: torch.nn.Parameter(_to(v, dev)) for k, v in p.items()}
        at = _to(a, dev).requires_grad_(True)

        def plan(idx):
            sp = G.SegPlan.host(idx.astype(np.int64))
            for f in ('order', 'seg_ptr', 'target'):
                setattr(sp, f, torch.from_numpy(getattr(sp, f)).to(dev))
            return sp
        loss = ops.HeadCEFn.apply(t['ent'], _to(ia, dev), t['h'], t['rel'], _to(ic, dev), t['w'], t['bias'], _to(tgt, dev),
                                  plan(ia), plan(ic), 0.0, 12345, 1.0, at, _to(q, dev))
        (loss * 0.7).backward()
        torch.cuda.synchronize()
        got = [loss.item()] + [t[k].grad.cpu().numpy() for k in ('ent', 'rel', 'w', 'bias', 'h')] + [at.grad.cpu().numpy()]
    finally:
        K.PLANES = old
    assert abs(got[0] - want[0]) <= 1e-4 * abs(want[0]) + 1e-6
    underflow = (kind == 3) & (q == 0)                                  # p_g = 0 in fp32: d_a is written as 0, not divided
    assert np.all(got[6][underflow] == 0.0) and np.all(np.isfinite(got[6]))
    got[6], want[6] = got[6][~underflow], want[6][~underflow]
    for x, y, name in zip(got[1:], want[1:], ('ent', 'rel', 'weight', 'bias', 'h', 'd_a')):
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(y).max()) * 10), err_msg=name)


# ---- 6. / 7. learn_observed --------------------------------------------------------------------------------------------
def late_positions(facts):
    return np.nonzero(facts[:, 3] >= 10 * RS.STEP)[0]


def hip_adam(net, lr=1e-3):
    import parallel
    return parallel.HipAdam(net, lr=lr, weight_decay=1e-5, max_norm=1.0)


def test_a_zero_prior_learns_as_no_prior_and_no_prior_is_todays_path(dev, monkeypatch):
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    facts = w['facts']
    idx = late_positions(facts)
    a, b = clone_of(w['net'], dev), clone_of(w['net'], dev)
    obs = stream_of_resident(facts, w['net'], w['gnet'])
    calls = []
    for name in ('recurrence_gold_rows', 'mix_ce', 'mix_ce_planes', 'recurrence_mix_rows_gated', 'recurrence_mix_rows'):
        monkeypatch.setattr(K, name, (lambda fn, name: lambda *x, **k: (calls.append(name), fn(*x, **k))[1])(getattr(K, name), name))
    la = a.learn_observed(obs, idx, hip_adam(a), steps=2)
    assert calls == [] and obs.device._pair == {}                       # prior=None: no tables, today's launches
    lb = b.learn_observed(obs, idx, hip_adam(b), steps=2, prior=RC.RecurrencePrior(0.0))
    assert calls.count('recurrence_gold_rows') == 4 and 'tables' in obs.device._pair
    assert len(la) == 2 and la == lb and same_parameters(a, b) and not same_parameters(a, w['net'])


class _Capture(torch.optim.SGD):
    """lr 0: step() only keeps a copy of every gradient."""

    def __init__(self, params):
        super(_Capture, self).__init__(params, lr=0.0)
        self.grads = []

    def step(self, closure=None):
        self.grads.append([p.grad.detach().clone() for g in self.param_groups for p in g['params']])


def gate_gradient_float64(net, obs, facts, idx, logit):
    """d loss / d logit [2, R] in float64 on observed_scores' logits: loss = the two directions' mean mixed losses."""
    import preprocess as P
    sub_pred, ob_pred = net.observed_scores(obs, idx)
    s, r, o, t = facts[idx].T
    n = len(idx)
    grad = np.zeros((2, RS.NUM_RELS))
    for side, role, ent, gold, pred in ((0, 0, s, o, ob_pred), (1, 1, o, s, sub_pred)):
        pi = P.PairIndex(facts, role, RS.NUM_ENT)
        q, W = CS.gold_rows(*pi.prior_rows(ent, r, t, t), gold, RS.NUM_ENT)
        a = np.where(W > 0, 1.0 / (1.0 + np.exp(-logit[side, r])), 0.0)
        _, _, d_a = CS.mix_ce(pred.double().cpu().numpy(), gold, a, q)
        np.add.at(grad[side], r, np.where(W > 0, d_a * a * (1.0 - a) / n, 0.0))
    return grad


def test_learning_with_a_copy_gate(dev):
    import recurrence as RC
    w = world(dev)
    facts, obs = w['facts'], w['obs']
    idx = late_positions(facts)
    assert np.any((facts[idx, 0] == RS.HOT_S) & (facts[idx, 1] == RS.HOT_R))
    runs = []
    for _ in range(2):
        net = clone_of(w['net'], dev)
        gate = RC.CopyGate(RS.NUM_RELS, alpha=0.3).to(dev)
        cap = _Capture(gate.parameters())
        losses = net.learn_observed(obs, idx, hip_adam(net), prior=gate, gate_optimizer=cap)
        assert len(losses) == 1 and len(cap.grads) == 1
        runs.append((losses, cap.grads[0][0], net))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])             # bit-identical run to run
    assert same_parameters(runs[0][2], runs[1][2]) and not same_parameters(runs[0][2], w['net'])   # the model's parameters move
    got = runs[0][1].double().cpu().numpy()
    want = gate_gradient_float64(w['net'], obs, facts, idx, np.full((2, RS.NUM_RELS), np.log(0.3 / 0.7)))
    assert got.shape == (2, RS.NUM_RELS)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(want).max()) * 10))
    # the hot relation's 'ob' side: the statement's sign, and one Adam step moves the logit against it
    assert want[0, RS.HOT_R] != 0 and np.sign(got[0, RS.HOT_R]) == np.sign(want[0, RS.HOT_R])
    net = clone_of(w['net'], dev)
    gate = RC.CopyGate(RS.NUM_RELS, alpha=0.3).to(dev)
    before = gate.logit.detach().clone()
    net.learn_observed(obs, idx, hip_adam(net), prior=gate, gate_optimizer=torch.optim.Adam(gate.parameters(), lr=0.05))
    moved = (gate.logit.detach() - before).cpu().numpy()
    assert np.sign(moved[0, RS.HOT_R]) == -np.sign(want[0, RS.HOT_R]) and np.all(np.sign(moved) == -np.sign(want))
    with pytest.raises(ValueError):
        net.learn_observed(obs, idx, hip_adam(net), prior=RC.RecurrencePrior(0.3), gate_optimizer=cap)


# ---- 8. a gate wherever a prior is accepted; fit_gate ------------------------------------------------------------------
def test_a_gate_of_one_half_equals_the_scalar_prior_and_fit_gate_fits(dev):
    import recurrence as RC
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    gate = RC.CopyGate(RS.NUM_RELS, alpha=0.5, half_life=24).to(dev)
    assert torch.equal(gate.logit, torch.zeros(2, RS.NUM_RELS, device=dev))
    prior = RC.RecurrencePrior(0.5, 24)
    pos = late_positions(facts)[:40]
    queries = model_queries(facts)

    def results(p):
        a, b = net.evaluate_observed(obs, pos, prior=p), RC.evaluate(obs, queries, p)
        top = net.forecast_topk(obs, queries, k=7, prior=p)
        return a, b, top

    def same(x, y):
        return all(np.array_equal(x[k][0][name], y[k][0][name]) for k in (0, 1) for name in SETTINGS) and \
            all(np.array_equal(x[k][1], y[k][1]) for k in (0, 1)) and \
            all(torch.equal(u, v) for name in ('sub', 'ob') for u, v in zip(x[2][name], y[2][name]))
    assert same(results(gate), results(prior))
    # fit_gate: the model frozen, the mean mixed loss of the fitted stream lower after 20 steps
    frozen = clone_of(net, dev)
    fit = RC.CopyGate(RS.NUM_RELS, alpha=0.3, half_life=24).to(dev)
    idx = late_positions(facts)
    losses = RC.fit_gate(frozen, obs, idx, fit, torch.optim.Adam(fit.parameters(), lr=0.1), steps=20)
    print('fit_gate: mean mixed loss %.4f -> %.4f' % (losses[0], losses[-1]))
    assert len(losses) == 20 and losses[-1] < losses[0] and same_parameters(frozen, net) and not frozen.training
    assert not torch.equal(fit.logit.detach(), torch.full((2, RS.NUM_RELS), float(np.log(0.3 / 0.7)), device=dev))
    # the first loss is the statement's mean mixed loss
    sub_pred, ob_pred = net.observed_scores(obs, idx)
    import preprocess as P
    s, r, o, t = facts[idx].T
    total = 0.0
    for role, ent, gold, pred in ((0, s, o, ob_pred), (1, o, s, sub_pred)):
        q, W = CS.gold_rows(*P.PairIndex(facts, role, RS.NUM_ENT).prior_rows(ent, r, t, t, inv_half_life=fit.inv_half_life),
                            gold, RS.NUM_ENT)
        total += CS.mix_ce(pred.double().cpu().numpy(), gold, np.where(W > 0, 0.3, 0.0), q)[0].sum()
    assert abs(losses[0] - total / (2 * len(idx))) <= 1e-5 * total / (2 * len(idx))
    # state_dict round trip
    again = RC.CopyGate(RS.NUM_RELS, half_life=24).to(dev)
    again.load_state_dict(fit.state_dict())
    x, y = net.evaluate_observed(obs, pos, prior=fit), net.evaluate_observed(obs, pos, prior=again)
    assert all(np.array_equal(x[0][name], y[0][name]) for name in SETTINGS) and np.array_equal(x[1], y[1])
    one = RC.CopyGate(RS.NUM_RELS, alpha=0.5, half_life=24, per_relation=False).to(dev)
    assert one.logit.shape == (2, 1)
    z = net.evaluate_observed(obs, pos, prior=one)
    ref = net.evaluate_observed(obs, pos, prior=prior)
    assert all(np.array_equal(z[0][name], ref[0][name]) for name in SETTINGS) and np.array_equal(z[1], ref[1])


# ---- 9. the online loop ------------------------------------------------------------------------------------------------
def test_online_loop_with_a_gate(dev):
    import recurrence as RC
    from test_gpu_recurrence import stream_of
    w = world(dev)
    gnet, facts = w['gnet'], w['facts']
    n = int(np.searchsorted(facts[:, 3], 11 * RS.STEP))
    head, quads = facts[:n], facts[n:]
    out = []
    for prior, kw in ((RC.RecurrencePrior(0.5, 24), {}), (RC.CopyGate(RS.NUM_RELS, alpha=0.5, half_life=24).to(dev), {})):
        net = clone_of(w['net'], dev)
        obs = stream_of(head)
        obs.resident(net, gnet)
        out.append(net.evaluate_online(obs, quads, gnet, hip_adam(net), steps=1, all_triplets=facts, prior=prior, **kw) + (net,))
    for name in SETTINGS:
        assert np.array_equal(out[0][0][name], out[1][0][name]), name
    assert np.array_equal(out[0][1], out[1][1]) and same_parameters(out[0][3], out[1][3])
    assert [e['losses'] for e in out[0][2]] == [e['losses'] for e in out[1][2]]
    net = clone_of(w['net'], dev)
    gate = RC.CopyGate(RS.NUM_RELS, alpha=0.5, half_life=24).to(dev)
    obs = stream_of(head)
    obs.resident(net, gnet)
    ranks, loss, log = net.evaluate_online(obs, quads, gnet, hip_adam(net), steps=1, all_triplets=facts, prior=gate,
                                           learn_prior=True, gate_optimizer=torch.optim.Adam(gate.parameters(), lr=0.05))
    assert len(net.last_online) == len(facts) and ranks['raw'].shape == (len(quads), 2) and np.all(np.isfinite(loss))
    assert all(len(e['losses']) == 1 for e in log) and bool((gate.logit.detach() != 0).any())
    with pytest.raises(ValueError):
        net.evaluate_online(obs, quads, gnet, hip_adam(net), steps=1, learn_prior=True)


# ---- 10. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(dev, monkeypatch):
    import ops
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    n, C = 8, 64
    x = torch.zeros(n, C, device=dev)
    tgt, a, q = torch.zeros(n, device=dev, dtype=torch.int32), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    loss, da = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    L = K.lib()
    ptr = lambda v: v.data_ptr()
    st = K._stream()
    planes = K.planes_empty(n, C, dev)
    pl = (ptr(planes.p), planes.plane, planes.p.shape[2], planes.p.shape[1])
    # a missing array, ld < C
    assert L.renet_mix_ce(ptr(x), ptr(tgt), None, ptr(q), n, C, C, 1.0, ptr(loss), None, ptr(da), st) != 0
    assert L.renet_mix_ce(ptr(x), ptr(tgt), ptr(a), None, n, C, C, 1.0, ptr(loss), None, ptr(da), st) != 0
    assert L.renet_mix_ce(ptr(x), ptr(tgt), ptr(a), ptr(q), n, C, C - 1, 1.0, ptr(loss), None, ptr(da), st) != 0
    assert L.renet_mix_ce_planes(ptr(x), ptr(tgt), None, ptr(q), n, C, C, 1.0, ptr(loss), *pl, ptr(da), st) != 0
    assert L.renet_mix_ce_planes(ptr(x), ptr(tgt), ptr(a), ptr(q), n, C, C - 1, 1.0, ptr(loss), *pl, ptr(da), st) != 0
    assert L.renet_mix_ce_planes(ptr(x), ptr(tgt), ptr(a), ptr(q), n, C, C, 1.0, ptr(loss), None, *pl[1:], ptr(da), st) != 0
    torch.cuda.synchronize()
    assert bool((loss == 7.0).all()) and bool((da == 7.0).all())         # nothing ran
    ent, rel, t = (i32(facts[:n, k], dev) for k in (0, 1, 3))
    tables, ent_ptr, snap_ptr, num_ent = role_args(store, 0)
    for bad in (1.0, -0.25, float('nan')):
        with pytest.raises(K.RenetHipError):
            K.recurrence_mix_rows_gated(ent, rel, t, t, tables, ent_ptr, snap_ptr, num_ent, None,
                                        torch.full((n,), bad, device=dev), num_cols=RS.NUM_ENT)
    with pytest.raises(K.RenetHipError):
        K.recurrence_mix_rows_gated(ent, rel, t, t, tables, ent_ptr, snap_ptr, num_ent, None, None, num_cols=RS.NUM_ENT)
    with pytest.raises(K.RenetHipError):
        K.recurrence_mix_rows_gated(ent, rel, t, t, tables, ent_ptr, snap_ptr, num_ent, x, a, num_cols=RS.NUM_ENT)   # ld < C
    with pytest.raises(K.RenetHipError):
        K.recurrence_gold_rows(ent, rel, t, t, tgt[:3], tables, ent_ptr, snap_ptr, num_ent, RS.NUM_ENT)
    gate = RC.CopyGate(RS.NUM_RELS).to(dev)
    with torch.no_grad():
        gate.logit[0, 0] = float('nan')
    with pytest.raises(ValueError):
        w['net'].evaluate_observed(w['obs'], late_positions(facts)[:8], prior=gate)
    with pytest.raises(ValueError):
        RC.CopyGate(RS.NUM_RELS, alpha=1.0)
    # a sharded batch, and bf16-storage mode
    net = clone_of(w['net'], dev)
    idx = late_positions(facts)[:16]
    import model as M
    _, prep = M._observed_prepared(net, store, (idx, net.prepare_both_device(idx, store)))
    rows = RC.CopyRows(store, idx, RC.RecurrencePrior(0.3))
    prep.sharded = True
    with pytest.raises(ValueError):
        net.loss_prepared_both(prep, copy=rows)
    prep.sharded = False
    calls = []
    monkeypatch.setattr(K, 'concat3_fwd', lambda *x, **k: calls.append(1))
    monkeypatch.setattr(K, 'GEMM_MODE', 'bf16s')
    with pytest.raises(ValueError):
        net.loss_prepared_both(prep, copy=rows)
    with pytest.raises(ValueError):
        ops._head_forward(None, None, None, None, None, None, None, None, 0.0, 0, 1.0, True, copy=(a, q))
    with pytest.raises(ValueError):
        net.learn_observed(w['obs'], idx, hip_adam(net), prior=RC.RecurrencePrior(0.3))
    assert calls == []
