"""GPU tests of the recurrence prior for event forecasts (run with -m gpu on an MI355X): renet_joint_mix_rows through direct
C-ABI calls against the float64 statement (preprocess.PairIndex.event_rows + tests/event_prior_statement.py), its walks on
hand-built pair tables, its refusals, the `prior=` keyword of the four event entries against a hand composition of the same
launches, recurrence.evaluate_events against the prediction from brute-force counts, and the observe loop.  The stream and
the world are those of tests/test_gpu_recurrence.py (70 entities, 3 relations, 14 timestamps; made once, left unchanged).

Bound of the rows: every element within one fp32 ulp of the statement, |out - ref| <= 2^-23 |ref| -- the device computes a
correctly rounded fp32 of an fp64 value, and its libm may differ from numpy's by a few fp64 ulps, which moves a value across at
most one rounding boundary.  Ranks, abstaining groups, alpha = 0 and plain-count masses are exact."""
import numpy as np
import pytest
import torch

import event_prior_statement as ES
import recurrence_statement as RS
from test_gpu_recurrence import SETTINGS, i32, stream_of, world

pytestmark = pytest.mark.gpu

R, N = RS.NUM_RELS, RS.NUM_ENT
ULP = 2.0 ** -23
RC_LONG, RC_TILE, JM_WIN = 128, 1 << 15, 1 << 16          # csrc/recurrence_common.h, csrc/joint_mix.hip
DIRECTIONS = (('sub', 0, 's', 2, 0, 1), ('ob', 1, 'o', 0, 2, 0))      # name, result column, filter side, given, ranked, role


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def mix_call(tables, ent_ptr, snap_ptr, num_ent, q, scores, off, num_rels, alpha, inv_half_life):
    """One renet_joint_mix_rows call on CLONES of scores [G * R, C] and off [G * R] -> (scores, off, mass)."""
    import renet_hip as K
    dev = scores.device
    s, o = scores.clone(), off.clone()
    mass = K.joint_mix_rows(s, num_rels, o, *(i32(a, dev) for a in q), tables, ent_ptr, snap_ptr, num_ent, alpha, inv_half_life)
    return s, o, mass


def mix_store(store, role, q, scores, off, prior_alpha, inv_half_life, num_rels=R):
    base = getattr(store, 'base', store)
    return mix_call(base.pair_tables()[role], base.t['ent_ptr%d' % role], base.t['snap_ptr%d' % role], base.num_ent, q, scores,
                    off, num_rels, prior_alpha, inv_half_life)


def assert_rows(out, ref, what):
    out = out.astype(np.float64)
    assert np.all(np.isfinite(out)), what
    err = np.abs(out - ref)
    worst = float(np.max(err / np.maximum(np.abs(ref), 1e-300)))
    print('%s: largest |out - ref| / |ref| = %.3e (bound %.3e)' % (what, worst, ULP))
    assert np.all(err <= ULP * np.abs(ref)), (what, worst)


# ---- 1. the kernel against the float64 statement ------------------------------------------------------------------------
def kernel_groups(facts):
    """(ent, t, as_of) of role-0 groups: the hot entity, an entity without facts in the role, -1 and num_ent, as_of at the
    first timestamp, as_of mid-stream with a later t, and two ordinary entities."""
    end = int(facts[:, 3].max())
    g = [(RS.HOT_S, end + RS.STEP, end + RS.STEP), (RS.NEVER_SUBJECT[0], end, end), (-1, end, end), (RS.NUM_ENT, end, end),
         (RS.HOT_S, 3 * RS.STEP, 0), (RS.HOT_S, end + 2 * RS.STEP, 6 * RS.STEP), (2, end, end), (17, end, end - RS.STEP)]
    return tuple(np.asarray(x, dtype=np.int64) for x in zip(*g))


@pytest.mark.parametrize('C, pick', [(RS.NUM_ENT, None), (64, None), (40000, (0, 5))])
@pytest.mark.parametrize('half_life', [None, 24, 100])
@pytest.mark.parametrize('alpha', [0.0, 0.3, 0.9])
def test_rows_against_float64(dev, alpha, half_life, C, pick):
    import preprocess as P
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    prior = RC.RecurrencePrior(alpha, half_life)
    q = kernel_groups(facts)
    if pick is not None:
        q = tuple(x[list(pick)] for x in q)
    G = len(q[0])
    rng = np.random.RandomState(C + 13)
    x = (3.0 * rng.randn(G * R, C)).astype(np.float32)
    o = (rng.randn(G * R) - 8.0).astype(np.float32)
    pi = P.PairIndex(facts, 0, RS.NUM_ENT)
    rows = pi.event_rows(*q, inv_half_life=prior.inv_half_life)
    counts = ES.group_mass(pi.event_rows(*q))                                          # facts counted, exact
    assert counts[0] > 256 and (pick is not None or (np.all(counts[1:5] == 0) and 0 < counts[5] < counts[0]))
    J32 = x + o[:, None]
    assert J32.dtype == np.float32
    ref = ES.mix_block(J32.reshape(G, R, C), rows, prior.alpha).reshape(G * R, C)
    got, off, mass = (a.cpu().numpy() for a in mix_store(store, 0, q, torch.from_numpy(x).to(dev), torch.from_numpy(o).to(dev),
                                                          prior.alpha, prior.inv_half_life))
    mixed = np.repeat(counts > 0, R)
    # abstaining groups: rows and off bit for bit; mixed groups: off = 0 and the rows within one ulp
    assert np.array_equal(got[~mixed], x[~mixed]) and np.array_equal(off[~mixed], o[~mixed])
    assert np.all(off[mixed] == 0) and not np.any(np.signbit(off[mixed]))
    assert_rows(got[mixed], ref[mixed], 'joint mix C %d alpha %.1f half_life %s' % (C, alpha, half_life))
    if alpha == 0.0:
        assert np.array_equal(got[mixed], J32[mixed])                                  # M == J bit for bit
    else:
        assert not np.array_equal(got[mixed], J32[mixed])
    # mass: exact for plain counts, a reordered sum of n positive terms otherwise
    Wref = ES.group_mass(rows)
    if half_life is None:
        assert np.array_equal(mass, counts)
    else:
        assert np.all(np.abs(mass - Wref) <= (counts + 4) * 2.0 ** -52 * Wref)
    # the same bits from a second launch
    again = mix_store(store, 0, q, torch.from_numpy(x).to(dev), torch.from_numpy(o).to(dev), prior.alpha, prior.inv_half_life)
    assert np.array_equal(again[0].cpu().numpy(), got) and np.array_equal(again[2].cpu().numpy(), mass)
    if C == RS.NUM_ENT and half_life == 100:
        # rows that start at every alignment, behind a row stride: the same values
        wide = torch.zeros(G * R, C + 5, device=dev)
        for shift in (1, 2, 3):
            wide.zero_()
            wide[:, shift:shift + C] = torch.from_numpy(x).to(dev)
            view = wide[:, shift:shift + C]
            o2 = torch.from_numpy(o).to(dev)
            K.joint_mix_rows(view, R, o2, *(i32(a, dev) for a in q), store.pair_tables()[0], store.t['ent_ptr0'],
                             store.t['snap_ptr0'], store.num_ent, prior.alpha, prior.inv_half_life)
            assert np.array_equal(view.cpu().numpy(), got) and np.array_equal(o2.cpu().numpy(), off), shift
            assert float(wide[:, :shift].abs().max()) == 0 and float(wide[:, shift + C:].abs().max()) == 0


# ---- 2. the walks, on hand-built tables ---------------------------------------------------------------------------------
def hand_tables(quads, num_ent, dev):
    """(tables, ent_ptr, snap_ptr, PairIndex) of role 0 for hand-built facts: one snapshot slot per entity, so that
    snap_ptr[ent_ptr[e]] is the entity's run start."""
    import preprocess as P
    pi = P.PairIndex(quads, 0, num_ent)
    tables = tuple(i32(a, dev) for a in (pi.p_rel, pi.p_other, pi.p_t))
    return tables, i32(np.arange(num_ent + 1), dev), i32(pi.run_ptr, dev), pi


def facts_of(groups):
    """[(relation, partner, counted, later)] -> facts of entity 0: `counted` facts at t' = 0 .. 9, `later` at t' = 50."""
    out = []
    for r, c, counted, later in groups:
        out += [(0, r, c, k % 10) for k in range(counted)] + [(0, r, c, 50)] * later
    out.append((1, 0, 2, 3))                                                           # another entity's run behind it
    return np.asarray(out, dtype=np.int64)


WALKS = {
    # a group of exactly RC_LONG counted facts (the head's thread), one of RC_LONG + 1 (a wave), both longer than that in all
    'long_threshold': (9, 2, [(0, 3, RC_LONG, 5), (0, 4, RC_LONG + 1, 0), (1, 3, RC_LONG + 1, 7), (1, 8, 1, 0), (1, 9, 4, 0)]),
    # a sub-run longer than RC_TILE: the third partner's head lies in the second tile; partner 12 lies outside the row
    'two_tiles': (11, 2, [(1, 1, 16500, 0), (1, 6, 16500, 3), (1, 7, 5, 0), (1, 12, 2, 0), (0, 0, 3, 0)]),
    # two windows of the column bitmap, the row starting one float behind a 16-byte border; partner 70000 outside the row
    'two_windows': (JM_WIN + 70, 1, [(0, 1, 2, 0), (0, JM_WIN - 1, 3, 0), (0, JM_WIN, 1, 1), (0, JM_WIN + 2, 300, 0),
                                      (0, JM_WIN + 3, 1, 0), (0, JM_WIN + 4, 1, 0), (0, JM_WIN + 69, 7, 0), (0, 70000, 9, 0)]),
}


@pytest.mark.parametrize('name', sorted(WALKS))
def test_walks_on_hand_built_tables(dev, name):
    import renet_hip as K
    C, nrel, groups = WALKS[name]
    quads = facts_of(groups)
    tables, ent_ptr, snap_ptr, pi = hand_tables(quads, 2, dev)
    q = (np.asarray([0]), np.asarray([40]), np.asarray([40]))
    rows = pi.event_rows(*q)
    counted = sum(g[2] for g in groups)
    assert counted > 256                                                               # longer than the mass launch's stride
    rng = np.random.RandomState(len(name))
    buf = np.zeros((nrel, C + 4), dtype=np.float32)
    buf[:, 1:C + 1] = (2.0 * rng.randn(nrel, C)).astype(np.float32)
    o = (rng.randn(nrel) - 6.0).astype(np.float32)
    J32 = buf[:, 1:C + 1] + o[:, None]
    alpha = float(np.float32(0.4))
    ref = ES.mix_block(J32.reshape(1, nrel, C), rows, alpha).reshape(nrel, C)
    assert np.count_nonzero(ref != J32.astype(np.float64) + np.log1p(-alpha)) == sum(1 for g in groups if g[1] < C and g[0] < nrel)
    whole = torch.from_numpy(buf).to(dev)
    view = whole[:, 1:C + 1]                                                           # (rows one float behind the buffer's alignment)
    off = torch.from_numpy(o).to(dev)
    mass = K.joint_mix_rows(view, nrel, off, *(i32(a, dev) for a in q), tables, ent_ptr, snap_ptr, 2, alpha, 0.0)
    assert float(mass.cpu()[0]) == counted
    assert_rows(view.cpu().numpy(), ref, 'joint mix walk %s' % name)
    assert np.all(off.cpu().numpy() == 0)
    got = whole.cpu().numpy()
    assert np.all(got[:, 0] == 0) and np.all(got[:, C + 1:] == 0)                      # nothing outside the rows is written


# ---- 3. refusals and G == 0 ---------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_no_groups_are_a_no_op(dev):
    import renet_hip as K
    w = world(dev)
    store = w['obs'].device
    tables, ent_ptr, snap_ptr = store.pair_tables()[0], store.t['ent_ptr0'], store.t['snap_ptr0']
    q = tuple(i32(a, dev) for a in kernel_groups(w['facts']))
    G = int(q[0].numel())
    x = torch.randn(G * R, N, device=dev)
    o = torch.randn(G * R, device=dev)
    keep_x, keep_o = x.clone(), o.clone()
    for alpha, ihl in ((1.0, 0.0), (-0.1, 0.0), (float('nan'), 0.0), (0.3, -1.0), (0.3, float('inf')), (0.3, float('nan'))):
        with pytest.raises(K.RenetHipError):
            K.joint_mix_rows(x, R, o, *q, tables, ent_ptr, snap_ptr, store.num_ent, alpha, ihl)
    mass = torch.empty(G, device=dev, dtype=torch.float64)
    nf, ns = int(tables[0].numel()), int(snap_ptr.numel()) - 1

    def raw(**kw):
        a = dict(ent=q[0].data_ptr(), t=q[1].data_ptr(), as_of=q[2].data_ptr(), G=G, p_rel=tables[0].data_ptr(),
                 p_other=tables[1].data_ptr(), p_t=tables[2].data_ptr(), n_facts=nf, ent_ptr=ent_ptr.data_ptr(),
                 snap_ptr=snap_ptr.data_ptr(), n_snaps=ns, num_ent=store.num_ent, scores=x.data_ptr(), ld=N, R=R, C=N,
                 off=o.data_ptr(), alpha=0.3, ihl=0.0, mass=mass.data_ptr(), stream=None)
        a.update(kw)
        return K.lib().renet_joint_mix_rows(*a.values())

    for kw in (dict(ld=N - 1), dict(R=0), dict(R=1025), dict(C=0), dict(C=(1 << 20) + 1, ld=(1 << 20) + 1), dict(G=-1),
               dict(mass=None), dict(scores=None), dict(off=None), dict(ent=None), dict(t=None), dict(as_of=None),
               dict(p_other=None), dict(ent_ptr=None), dict(snap_ptr=None)):
        assert raw(**kw) == -1, kw                                                     # RENET_ERR_BADARG, before any launch
    assert raw(G=0, mass=None, scores=None) == 0                                       # G == 0: a no-op
    torch.cuda.synchronize()
    assert torch.equal(x, keep_x) and torch.equal(o, keep_o)
    empty = K.joint_mix_rows(x[:0], R, o[:0], *(a[:0] for a in q), tables, ent_ptr, snap_ptr, store.num_ent, 0.3, 0.0)
    assert empty.shape == (0,) and empty.dtype == torch.float64


# ---- 4. the model path --------------------------------------------------------------------------------------------------
def event_positions(facts):
    pos = np.nonzero(facts[:, 3] >= 10 * RS.STEP)[0]
    return pos[np.random.RandomState(12).choice(len(pos), 40, replace=False)]


def same_events(a, b):
    return all(np.array_equal(a[kind][name], b[kind][name]) for kind in ('pair', 'relation') for name in SETTINGS) and \
        np.array_equal(a['logp'], b['logp'])


def hand_mixed(net, store, idx, quads, as_of, prior):
    """{direction: (M [n, R, N], off [n, R])}: observed_event_scores without a prior, then ONE direct mix call per direction,
    every position a group of its own."""
    ev = net.observed_event_scores(store, idx)
    out = {}
    for name, col, side, given, ranked, role in DIRECTIONS:
        B, off = ev[name]
        n = B.shape[0]
        m, o, _ = mix_store(store, role, (quads[:, given], quads[:, 3], as_of), B.reshape(n * R, N), off.reshape(-1),
                            prior.alpha, prior.inv_half_life)
        out[name] = (m.view(n, R, N), o.view(n, R))
    return out


def test_prior_none_is_todays_path_and_a_prior_is_one_mix_call(dev):
    import filter_index as FI
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    store = obs.device
    idx = event_positions(facts)
    quads = facts[idx]
    base = net.evaluate_events_observed(obs, idx)
    assert same_events(base, net.evaluate_events_observed(obs, idx, prior=None))
    assert same_events(base, net.evaluate_events_observed(obs, idx, prior=RC.RecurrencePrior(0.0, 100)))
    prior = RC.RecurrencePrior(0.3, 100)
    got = net.evaluate_events_observed(obs, idx, prior=prior)
    mixed = hand_mixed(net, store, idx, quads, quads[:, 3], prior)
    index = FI.filter_index_for(store, store.quads)
    n = len(idx)
    group = i32(np.arange(n), dev)
    for name, col, side, given, ranked, role in DIRECTIONS:
        keys = np.stack((np.repeat(quads[:, given], R), np.tile(np.arange(R), n), np.repeat(quads[:, 3], R)), axis=1)
        M, off = mixed[name]
        cnt, at_gold, _, _ = K.joint_rank_rows(M.reshape(n * R, N), R, off.reshape(-1), group, i32(quads[:, 1], dev),
                                               i32(quads[:, ranked], dev), *index.ranges_both(side, keys, dev))
        cnt = cnt.cpu().numpy().astype(np.float64)
        for k, setting in enumerate(SETTINGS):
            assert np.array_equal(got['pair'][setting][:, col], cnt[2 * k] + (cnt[2 * k + 1] - 1.0) / 2 + 1), (name, setting)
        assert np.array_equal(got['logp'][:, col], at_gold.cpu().numpy()[np.arange(n), quads[:, 1]])
    assert any(not np.array_equal(got['pair'][name], base['pair'][name]) for name in SETTINGS)     # the prior does move ranks
    # observed_event_scores(prior=): the hand-mixed blocks
    ev = net.observed_event_scores(obs, idx, prior=prior)
    plain = net.observed_event_scores(obs, idx)
    again = net.observed_event_scores(obs, idx, prior=None)
    for name in ('sub', 'ob'):
        assert torch.equal(ev[name][0], mixed[name][0]) and torch.equal(ev[name][1], mixed[name][1]), name
        assert torch.equal(plain[name][0], again[name][0]) and torch.equal(plain[name][1], again[name][1])
    # predict_events_observed(prior=): J descending, then relation, then entity, taken on the host from that block
    k = 9
    top = net.predict_events_observed(obs, idx, k=k, prior=prior)
    for name in ('sub', 'ob'):
        J = (ev[name][0] + ev[name][1][:, :, None]).cpu().numpy().reshape(n, R * N)
        rel, ent, logp, n_valid = (x.cpu().numpy() for x in top[name])
        for i in range(n):
            order = np.lexsort((np.arange(R * N), -J[i].astype(np.float64)))[:k]       # flat index = relation-major, then entity
            assert np.array_equal(rel[i], order // N) and np.array_equal(ent[i], order % N), (name, i)
            assert np.array_equal(logp[i], J[i][order])
        assert np.all(n_valid == k)
    none = net.predict_events_observed(obs, idx, k=k, prior=None)
    unmixed = net.predict_events_observed(obs, idx, k=k)
    assert all(torch.equal(x, y) for name in ('sub', 'ob') for x, y in zip(none[name], unmixed[name]))
    assert any(not torch.equal(x, y) for name in ('sub', 'ob') for x, y in zip(top[name], unmixed[name]))


def test_forecast_events_cuts_the_prior_at_the_histories_as_of(dev):
    import recurrence as RC
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    store = obs.device
    end = int(facts[:, 3].max())
    prior = RC.RecurrencePrior(0.3, 100)
    ents = np.asarray([RS.HOT_S, 2, 17, RS.NEVER_SUBJECT[0], RS.HOT_S, 33])
    t = np.asarray([end + RS.STEP, end, end, end, end, end + RS.STEP])
    as_of = np.asarray([end + RS.STEP, end - 2 * RS.STEP, end, end, 5 * RS.STEP, 0])
    got = net.forecast_events(obs, ents, t, k=6, direction='ob', as_of=as_of, prior=prior)
    quads = np.stack((ents, np.zeros_like(ents), np.full_like(ents, -1), t), axis=1)
    qs = store.queries(quads, as_of)
    pos = np.arange(len(ents))
    want = net.predict_events_observed(qs, pos, k=6, all_triplets=qs.facts, sides=('ob',), prior=prior)['ob']
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    fresh = net.forecast_events(obs, ents, t, k=6, direction='ob', prior=prior)            # as_of = t: another prior for the stale rows
    assert not torch.equal(fresh[2][1], got[2][1])
    # the block behind it: the model's own block of the same QueryStore through a direct mix call with THAT as_of
    ev = net.observed_event_scores(qs, pos, prior=prior)['ob']
    B, off = net.observed_event_scores(qs, pos)['ob']
    m, o, mass = mix_store(store, 0, (ents, t, as_of), B.reshape(len(ents) * R, N), off.reshape(-1), prior.alpha,
                           prior.inv_half_life)
    assert torch.equal(ev[0].reshape(-1, N), m) and torch.equal(ev[1].reshape(-1), o)
    mass = mass.cpu().numpy()
    assert mass[3] == 0 and mass[5] == 0 and np.all(mass[[0, 1, 2, 4]] > 0)
    assert torch.equal(ev[1][3], off[3]) and torch.equal(ev[0][3], B[3])                   # no history: untouched
    J = (ev[0] + ev[1][:, :, None]).cpu().numpy().reshape(len(ents), R * N)
    for i in range(len(ents)):
        order = np.lexsort((np.arange(R * N), -J[i].astype(np.float64)))[:6]
        assert np.array_equal(got[0][i].cpu().numpy(), order // N) and np.array_equal(got[1][i].cpu().numpy(), order % N)


def test_a_single_gate_is_its_alpha_and_a_gate_per_relation_is_refused(dev):
    import recurrence as RC
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    idx = event_positions(facts)[:16]
    gate = RC.CopyGate(R, 0.3, 100, per_relation=False).to(dev)
    a = RC.event_alpha(gate, 'ob')
    assert a == RC.event_alpha(gate, 'sub') == float(np.float32(a)) and abs(a - 0.3) < 1e-6
    want = net.evaluate_events_observed(obs, idx, prior=RC.RecurrencePrior(a, 100))
    assert same_events(net.evaluate_events_observed(obs, idx, prior=gate), want)
    with torch.no_grad():
        gate.logit[1, 0] = 1.5                                                         # the 'sub' side's own gate
    b = RC.event_alpha(gate, 'sub')
    assert b != a and RC.event_alpha(gate, 'ob') == a
    got = net.evaluate_events_observed(obs, idx, prior=gate)
    other = net.evaluate_events_observed(obs, idx, prior=RC.RecurrencePrior(b, 100))
    for name in SETTINGS:
        assert np.array_equal(got['pair'][name][:, 1], want['pair'][name][:, 1])       # ob: a
        assert np.array_equal(got['pair'][name][:, 0], other['pair'][name][:, 0])      # sub: b
    assert np.array_equal(got['logp'][:, 1], want['logp'][:, 1]) and np.array_equal(got['logp'][:, 0], other['logp'][:, 0])
    per_rel = RC.CopyGate(R, 0.3, 100, per_relation=True).to(dev)
    for call in (lambda: net.evaluate_events_observed(obs, idx, prior=per_rel),
                 lambda: net.predict_events_observed(obs, idx, k=3, prior=per_rel),
                 lambda: net.observed_event_scores(obs, idx, prior=per_rel),
                 lambda: net.forecast_events(obs, [2], int(facts[:, 3].max()), k=3, prior=per_rel),
                 lambda: RC.evaluate_events(obs, idx, per_rel)):
        with pytest.raises(ValueError, match='per-relation'):
            call()
    with pytest.raises(ValueError):
        net.evaluate_events_observed(obs, idx, prior=0.3)


# ---- 5. the baseline ----------------------------------------------------------------------------------------------------
def predicted_event_ranks(facts, quads):
    """({setting: pair ranks [n, 2]}, raw relation ranks [n, 2]) from the integer (relation, partner) counts alone; a known
    pair other than the gold one is no candidate under the filtered settings."""
    n = len(quads)
    pair = {name: np.zeros((n, 2)) for name in SETTINGS}
    rel = np.zeros((n, 2))
    for i, f in enumerate(quads.tolist()):
        for name, col, side, given, ranked, role in DIRECTIONS:
            e, t, gr, gc = f[given], f[3], f[1], f[ranked]
            c = np.stack([RS.partner_counts(facts, role, e, r, t) for r in range(R)])
            mine = facts[facts[:, given] == e]
            for setting in SETTINGS:
                live = np.ones((R, N), dtype=bool)
                known = mine if setting == 'filtered' else mine[mine[:, 3] == t] if setting == 'time_filtered' else mine[:0]
                live[known[:, 1], known[:, ranked]] = False
                live[gr, gc] = True
                pair[setting][i, col] = np.sum(live & (c > c[gr, gc])) + (np.sum(live & (c == c[gr, gc])) - 1) / 2 + 1
            rel[i, col] = np.sum(c[:, gc] > c[gr, gc]) + (np.sum(c[:, gc] == c[gr, gc]) - 1) / 2 + 1
    return pair, rel


def test_baseline_ranks_equal_the_counts_prediction(dev):
    """With half_life = None the mixed uniform joint is strictly increasing in the integer count (guarded on the CPU by
    tests/test_event_prior_statement_cpu.py), so the baseline's ranks follow from brute-force counts; a group without history
    is one R * N-way tie."""
    import recurrence as RC
    w = world(dev)
    obs, facts = w['obs'], w['facts']
    rng = np.random.RandomState(31)
    idx = np.concatenate((rng.choice(len(facts), 48, replace=False), np.nonzero(facts[:, 3] == 0)[0][:4]))
    quads = facts[idx]
    prior = RC.RecurrencePrior(0.5)
    got = RC.evaluate_events(obs, idx, prior)
    pair, rel = predicted_event_ranks(facts, quads)
    for name in SETTINGS:
        assert got['pair'][name].dtype == np.float64 and got['pair'][name].shape == (len(idx), 2)
        assert np.array_equal(got['pair'][name], pair[name]), (name, np.argwhere(got['pair'][name] != pair[name])[:5])
    assert np.array_equal(got['relation']['raw'], rel)
    first = len(idx) - 1                                                               # a fact of the first timestamp: no history
    assert got['pair']['raw'][first, 0] == got['pair']['raw'][first, 1] == (R * N + 1) / 2
    flat = np.float32(-np.log(float(R * N)))
    assert abs(got['logp'][first, 0] - flat) <= 2e-7 * abs(flat)
    # the same numbers whatever the cut of the sub-blocks
    again = RC.evaluate_events(obs, idx, prior, block_floats=5 * R * N)
    assert same_events(got, again)
    # topk_events: the most frequent pairs first, then the unseen ones by relation and entity
    top = RC.topk_events(obs, idx[:12], prior, k=6, sides=('ob',))
    assert sorted(top) == ['ob']
    rel_k, ent_k, logp_k, n_valid = (x.cpu().numpy() for x in top['ob'])
    for i, f in enumerate(quads[:12].tolist()):
        c = np.stack([RS.partner_counts(facts, 0, f[0], r, f[3]) for r in range(R)]).reshape(-1)
        order = np.lexsort((np.arange(R * N), -c))[:6]
        assert np.array_equal(rel_k[i], order // N) and np.array_equal(ent_k[i], order % N), i
        if c.sum() > 0:
            p = 0.5 / (R * N) + 0.5 * c[order] / c.sum()
            assert np.all(np.abs(np.exp(logp_k[i].astype(np.float64)) - p) <= 4e-6 * p)
    assert np.all(n_valid == 6)


# ---- 6. the observe loop ------------------------------------------------------------------------------------------------
def test_mixed_event_ranks_ride_through_observe(dev):
    import recurrence as RC
    w = world(dev)
    net, gnet, facts = w['net'], w['gnet'], w['facts']
    t = facts[:, 3]
    n0, n1 = int(np.searchsorted(t, 10 * RS.STEP)), int(np.searchsorted(t, 12 * RS.STEP))
    prior = RC.RecurrencePrior(0.3, 24)
    cur = stream_of(facts[:n0])
    cur.resident(net, gnet).pair_tables()                                              # asked for: observe() carries them
    cur = cur.observe(facts[n0:n1], gnet)
    assert 'tables' in cur.device._pair
    idx = np.arange(n0, n1)[::3]
    got = net.evaluate_events_observed(cur, idx, prior=prior)
    base = RC.evaluate_events(cur, idx, prior)
    ref = stream_of(facts[:n0]).extended(facts[n0:n1])
    ref.resident(net, gnet)
    assert same_events(got, net.evaluate_events_observed(ref, idx, prior=prior))
    assert same_events(base, RC.evaluate_events(ref, idx, prior))
    assert not same_events(got, net.evaluate_events_observed(ref, idx))
