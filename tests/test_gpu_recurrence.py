"""GPU tests of the recurrence prior (run with -m gpu on an MI355X): renet_pair_append behind ObservedStream.observe,
renet_recurrence_mix_rows directly, through recurrence.evaluate / topk and behind the prior= keyword of the observed family.
One synthetic stream (tests/recurrence_statement.py: 70 entities, 3 relations, 14 timestamps with step 24, about 600 facts,
a pair with 350 facts over 68 partners, duplicates, entities without facts in one role), n_hidden 100, seq_len 4.

Tables, integer statistics and ranks are exact.  The rows are compared with the float64 statement in PROBABILITY space; the
bound is 4 x the largest relative error measured over the cases of test_rows_against_float64 (ROW_ERR below, recorded in
profiles/recurrence_prior.md): an output is one fp32 rounding of a log-probability l, which is a relative error of |l| *
2^-24 in the probability."""
import numpy as np
import pytest
import torch

from helpers import fixtures, global_shapes, renet_shapes
import recurrence_statement as RS
from test_recurrence_cpu import queries_of

pytestmark = pytest.mark.gpu

D = 100
SETTINGS = ('raw', 'filtered', 'time_filtered')
ROW_ERR = 9.54e-7         # measured: the largest relative error of exp(out) over the 18 cases below (at l = -16: 16 * 2^-24)
ROW_BOUND = 4 * ROW_ERR


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def stream_of(facts):
    import preprocess as P
    cut = int(np.searchsorted(facts[:, 3], facts[len(facts) // 2, 3]))              # (a split border at a timestamp border)
    return P.ObservedStream((facts[:cut], facts[cut:]), RS.NUM_ENT, RS.NUM_RELS, RS.SEQ_LEN)


_WORLD = {}


def world(dev):
    """The facts, the models and the resident stream of all 14 timestamps: made once, shared, left unchanged."""
    if not _WORLD:
        import global_model as GM
        import model as M
        facts = RS.make_stream()
        net = M.RENet(RS.NUM_ENT, D, RS.NUM_RELS, dropout=0.0, seq_len=RS.SEQ_LEN)
        gnet = GM.RENet_global(RS.NUM_ENT, D, RS.NUM_RELS, dropout=0.0, seq_len=RS.SEQ_LEN, maxpool=1)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in
                             fixtures.make_params(71, renet_shapes(RS.NUM_ENT, RS.NUM_RELS, D)).items()})
        gnet.load_state_dict({k: torch.from_numpy(v) for k, v in
                              fixtures.make_params(72, global_shapes(RS.NUM_ENT, RS.NUM_RELS, D)).items()})
        net, gnet = net.to(dev).eval(), gnet.to(dev).eval()
        obs = stream_of(facts)
        obs.resident(net, gnet)
        _WORLD.update(facts=facts, net=net, gnet=gnet, obs=obs)
    return _WORLD


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def mix_direct(store, role, q, logits, prior, want_stats=False, num_cols=None):
    """One renet_recurrence_mix_rows launch on the store's resident tables for the queries q = (ent, rel, t, as_of)."""
    import renet_hip as K
    dev = store.device
    return K.recurrence_mix_rows(*(i32(a, dev) for a in q), store.pair_tables()[role], store.t['ent_ptr%d' % role],
                                 store.t['snap_ptr%d' % role], store.num_ent, logits, prior.alpha, prior.inv_half_life,
                                 num_cols=num_cols, want_stats=want_stats)


# ---- 1. pair append ----------------------------------------------------------------------------------------------------
def test_pair_tables_ride_through_observe(dev):
    import preprocess as P
    w = world(dev)
    facts, net, gnet = w['facts'], w['net'], w['gnet']
    t = facts[:, 3]
    a = int(np.searchsorted(t, 9 * RS.STEP))
    b = int(np.searchsorted(t, 10 * RS.STEP))
    cuts = [a + (b - a) // 2, b, int(np.searchsorted(t, 12 * RS.STEP)), len(facts)]    # the first append JOINS timestamp 9
    assert cuts[0] > a and facts[cuts[0] - 1, 3] == facts[cuts[0], 3]
    cur = stream_of(facts[:cuts[0]])
    first = cur.resident(net, gnet)
    old = [[x.clone() for x in tab] for tab in first.pair_tables()]
    for n0, n1 in zip(cuts[:-1], cuts[1:]):
        cur = cur.observe(facts[n0:n1], gnet)
        got = cur.device._pair['tables']
        want = stream_of(facts[:cuts[0]]).extended(facts[cuts[0]:n1]).resident(net, gnet).pair_tables()
        for role in (0, 1):
            host = P.PairIndex(facts[:n1], role, RS.NUM_ENT)
            for x, y, h in zip(got[role], want[role], (host.p_rel, host.p_other, host.p_t)):
                assert x.dtype == y.dtype == torch.int32 and x.shape == y.shape == (n1,) and torch.equal(x, y), (n1, role)
                assert np.array_equal(x.cpu().numpy(), h)
        assert cur.device.pair_tables() is got                                          # cached, not rebuilt
    for tab, keep in zip(first.pair_tables(), old):                                     # the old tables are never written
        assert all(torch.equal(x, y) for x, y in zip(tab, keep))
    # a store that never asked for pair tables has none after observe()
    plain = stream_of(facts[:cuts[0]])
    plain.resident(net, gnet)
    assert plain.observe(facts[cuts[0]:cuts[1]], gnet).device._pair == {} and plain.device._pair == {}
    # refresh_global's store and a QueryStore share the base store's tables
    shared = cur.refresh_global(gnet)
    assert shared.device.pair_tables() is got
    assert cur.device.queries(facts[:3]).pair_tables() is got


# ---- 2. exact integers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('role', [0, 1])
def test_stats_equal_the_host_statement(dev, role):
    import preprocess as P
    import recurrence as RC
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    q = queries_of(facts)
    assert np.any(q[3] < q[2]) and q[2].max() > facts[:, 3].max() and q[0].min() == -1
    pi = P.PairIndex(facts, role, RS.NUM_ENT)
    want = pi.prior_stats(*q)
    assert np.any(want[:, 1] == 0) and (role == 1 or (want[:, 1].max() > 300 and want[:, 0].max() > 64))
    out, stats, W = mix_direct(store, role, q, None, RC.RecurrencePrior(0.5), want_stats=True, num_cols=RS.NUM_ENT)
    assert np.array_equal(stats.cpu().numpy(), want)
    assert np.array_equal(W.cpu().numpy(), want[:, 1].astype(np.float32))               # plain counts: W is the integer
    # a row without history is uniform, whatever alpha
    flat = np.float32(-np.log(float(RS.NUM_ENT)))
    rows = out.cpu().numpy()[want[:, 1] == 0]
    assert len(rows) >= 4 and np.all(rows == rows[:, :1]) and np.all(np.abs(rows - flat) <= 2e-7 * abs(flat))


# ---- 3. exact ranks through the whole path -----------------------------------------------------------------------------
def labelled_queries(facts):
    rng = np.random.RandomState(9)
    end = int(facts[:, 3].max())
    hot = facts[(facts[:, 0] == RS.HOT_S) & (facts[:, 1] == RS.HOT_R) & (facts[:, 3] >= 4 * RS.STEP)]
    q = [facts[rng.choice(len(facts), 40, replace=False)], hot[rng.choice(len(hot), 12, replace=False)],
         np.asarray([[RS.HOT_S, RS.HOT_R, 69, end], [RS.HOT_S, RS.HOT_R, 68, end + RS.STEP],        # gold never seen
                     [RS.HOT_S, RS.HOT_R, RS.HOT_O, end + 2 * RS.STEP], [RS.BARE_S, RS.BARE_R, RS.BARE_O, 96],
                     [RS.BARE_S, RS.BARE_R, 3, end], [60, 0, 69, 48], [2, 1, 2, 0]])]
    return np.concatenate(q).astype(np.int64)


def predicted_ranks(facts, queries, as_of):
    """{setting: float64 [n, 2]} from the integer partner counts alone: greater = #{c > c_gold}, equal = #{c == c_gold} over
    the columns that are not filtered (a filtered column other than the gold one falls below everything)."""
    n, N = len(queries), RS.NUM_ENT
    out = {name: np.zeros((n, 2)) for name in SETTINGS}
    for i, (s, r, o, t) in enumerate(queries.tolist()):
        for col, role, ent, gold, e_col, p_col in ((0, 1, o, s, 2, 0), (1, 0, s, o, 0, 2)):
            c = RS.partner_counts(facts, role, ent, r, as_of[i])
            same = (facts[:, e_col] == ent) & (facts[:, 1] == r)
            known = {'raw': set(), 'filtered': set(facts[same, p_col].tolist()),
                     'time_filtered': set(facts[same & (facts[:, 3] == t), p_col].tolist())}
            for name in SETTINGS:
                live = np.ones(N, dtype=bool)
                live[sorted(known[name] - {gold})] = False
                greater, equal = int(np.sum(live & (c > c[gold]))), int(np.sum(live & (c == c[gold])))
                out[name][i, col] = greater + (equal - 1) / 2 + 1
    return out


@pytest.mark.parametrize('stale', [0, 2])
def test_baseline_ranks_equal_the_counts_prediction(dev, stale):
    import recurrence as RC
    w = world(dev)
    facts, obs = w['facts'], w['obs']
    queries = labelled_queries(facts)
    as_of = queries[:, 3] - stale * RS.STEP
    ranks, loss = RC.evaluate(obs, queries, RC.RecurrencePrior(0.5), as_of=None if stale == 0 else as_of, max_batch=32)
    want = predicted_ranks(facts, queries, as_of)
    for name in SETTINGS:
        assert ranks[name].dtype == np.float64 and ranks[name].shape == (len(queries), 2)
        assert np.array_equal(ranks[name], want[name]), (name, np.argwhere(ranks[name] != want[name])[:5])
    bare = len(queries) - 4                                                            # (BARE_S, BARE_R, BARE_O): no history on either side
    assert ranks['raw'][bare, 0] == ranks['raw'][bare, 1] == (RS.NUM_ENT + 1) / 2       # one N-way tie
    assert loss.shape == (len(queries),) and abs(loss[bare] - 2 * np.log(RS.NUM_ENT)) <= 1e-6 * loss[bare]
    # the same numbers whatever the cut of the scoring batches
    again, loss2 = RC.evaluate(obs, queries, RC.RecurrencePrior(0.5), as_of=None if stale == 0 else as_of)
    assert all(np.array_equal(again[name], ranks[name]) for name in SETTINGS) and np.array_equal(loss, loss2)


def test_baseline_topk_lists_the_most_frequent_partners(dev):
    import recurrence as RC
    w = world(dev)
    facts, obs = w['facts'], w['obs']
    end = int(facts[:, 3].max())
    q = np.asarray([[RS.HOT_S, RS.HOT_R, -1, end + RS.STEP], [RS.BARE_S, RS.BARE_R, -1, end]])
    got = RC.topk(obs, q, RC.RecurrencePrior(0.5), k=5, sides=('ob',))
    assert sorted(got) == ['ob']
    idx, score, logp, n_valid = (x.cpu().numpy() for x in got['ob'])
    c = RS.partner_counts(facts, 0, RS.HOT_S, RS.HOT_R, end + RS.STEP)
    order = np.lexsort((np.arange(RS.NUM_ENT), -c))[:5]                                # count descending, column ascending
    assert list(idx[0]) == list(order) and list(idx[1]) == [0, 1, 2, 3, 4] and list(n_valid) == [5, 5]
    p = 0.5 / RS.NUM_ENT + 0.5 * c[order] / c.sum()
    assert np.all(np.abs(np.exp(logp[0].astype(np.float64)) - p) <= ROW_BOUND * p) and np.array_equal(score, logp)


# ---- 4. rows against float64, 5. run to run ----------------------------------------------------------------------------
def row_queries(facts, n):
    end = int(facts[:, 3].max())
    q = [(RS.HOT_S, RS.HOT_R, end + RS.STEP, end + RS.STEP), (RS.HOT_S, RS.HOT_R, end, end - 3 * RS.STEP),
         (RS.BARE_S, RS.BARE_R, end, end), (2, 1, end, end)]
    rng = np.random.RandomState(4)
    for f in facts[rng.choice(len(facts), max(0, n - len(q)), replace=False)]:
        q.append((int(f[0]), int(f[1]), int(f[3]), int(f[3]) - RS.STEP * int(rng.randint(0, 3))))
    return tuple(np.asarray(x, dtype=np.int64) for x in zip(*q[:n]))


def row_errors(out, ref):
    """(largest relative error of exp(out) against the statement, largest |logsumexp(out)|), float64."""
    o = out.double().cpu().numpy()
    assert np.all(np.isfinite(o))
    m = o.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(o - m).sum(axis=1, keepdims=True)))[:, 0]
    return float(np.max(np.abs(np.expm1(o - ref)))), float(np.max(np.abs(lse)))


@pytest.mark.parametrize('C, n', [(RS.NUM_ENT, 24), (40000, 4)])
@pytest.mark.parametrize('half_life', [None, 24, 100])
@pytest.mark.parametrize('alpha', [0.0, 0.3, 0.9])
def test_rows_against_float64(dev, alpha, half_life, C, n):
    import preprocess as P
    import recurrence as RC
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    prior = RC.RecurrencePrior(alpha, half_life)
    q = row_queries(facts, n)
    x = (3.0 * np.random.RandomState(C + 7).randn(n, C)).astype(np.float32)
    logits = torch.from_numpy(x).to(dev)
    pi = P.PairIndex(facts, 0, RS.NUM_ENT)
    ref = RS.mix_rows(x, C, *pi.prior_rows(*q, inv_half_life=prior.inv_half_life), prior.alpha)
    out, stats, W = mix_direct(store, 0, q, logits, prior, want_stats=True)
    assert torch.equal(logits.cpu(), torch.from_numpy(x))                              # the logits are never written
    err, lse = row_errors(out, ref)
    print('recurrence rows: C %d alpha %.1f half_life %s: rel err %.3e, |logsumexp| %.3e' % (C, alpha, half_life, err, lse))
    assert err <= ROW_BOUND and lse <= ROW_BOUND
    if alpha == 0.0:                                                                   # log_softmax of the logits
        assert np.max(np.abs(np.expm1(out.double().cpu().numpy() - RS.log_softmax64(x)))) <= ROW_BOUND
    ptr, col, wts = pi.prior_rows(*q, inv_half_life=prior.inv_half_life)
    Wref = np.asarray([wts[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])])
    assert np.all(np.abs(W.double().cpu().numpy() - Wref) <= 1.2e-7 * Wref)
    # 5. run to run: the same bits from a second launch
    again = mix_direct(store, 0, q, logits, prior)
    assert torch.equal(out, again)
    # a row stride that puts the logits and the output rows at different alignments takes the scalar stores: the same bound
    # (the logsumexp is summed in another order there, so the bits may differ)
    if C == RS.NUM_ENT:
        wide = torch.zeros(n, C + 3, device=dev)
        wide[:, 1:C + 1] = logits
        err, lse = row_errors(mix_direct(store, 0, q, wide[:, 1:C + 1], prior), ref)
        assert err <= ROW_BOUND and lse <= ROW_BOUND


@pytest.mark.parametrize('half_life', [None, 24])
def test_long_partner_groups_are_summed_by_a_wave(dev, half_life):
    """A partner group of more than 128 counted facts leaves the head's thread for a whole wave (csrc/recurrence.hip, step
    5): the stream plus 500 / 129 / 128 facts of three objects of the hot pair, spread over the timestamps -- one group on
    either side of the threshold and one far beyond it, cut by as_of in the stale rows."""
    import preprocess as P
    import recurrence as RC
    w = world(dev)
    rng = np.random.RandomState(21)
    times = np.unique(w['facts'][:, 3])
    extra = [(RS.HOT_S, RS.HOT_R, o, int(t)) for o, k in ((11, 500), (12, 129), (13, 128)) for t in rng.choice(times, k)]
    facts = np.concatenate((w['facts'], np.asarray(extra, dtype=np.int64)))
    facts = facts[np.argsort(facts[:, 3], kind='stable')]
    store = stream_of(facts).resident(w['net'], w['gnet'])
    prior = RC.RecurrencePrior(0.3, half_life)
    q = row_queries(facts, 8)
    x = (3.0 * np.random.RandomState(3).randn(8, RS.NUM_ENT)).astype(np.float32)
    pi = P.PairIndex(facts, 0, RS.NUM_ENT)
    lists = pi.prior_rows(*q, inv_half_life=prior.inv_half_life)
    assert pi.prior_stats(*q)[0, 1] > 1000
    out, stats, W = mix_direct(store, 0, q, torch.from_numpy(x).to(dev), prior, want_stats=True)
    assert np.array_equal(stats.cpu().numpy(), pi.prior_stats(*q))
    err, lse = row_errors(out, RS.mix_rows(x, RS.NUM_ENT, *lists, prior.alpha))
    assert err <= ROW_BOUND and lse <= ROW_BOUND
    assert torch.equal(out, mix_direct(store, 0, q, torch.from_numpy(x).to(dev), prior))


def test_uniform_rows_equal_zero_logits_and_bad_arguments_are_refused(dev):
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    store, facts = w['obs'].device, w['facts']
    q = row_queries(facts, 16)
    prior = RC.RecurrencePrior(0.3, 24)
    a = mix_direct(store, 0, q, None, prior, num_cols=RS.NUM_ENT)
    b = mix_direct(store, 0, q, torch.zeros(16, RS.NUM_ENT, device=dev), prior)
    assert np.max(np.abs(np.expm1((a - b).double().cpu().numpy()))) <= ROW_BOUND
    for bad in (1.0, -0.1, float('nan')):
        with pytest.raises(K.RenetHipError):
            K.recurrence_mix_rows(*(i32(x, dev) for x in q), store.pair_tables()[0], store.t['ent_ptr0'], store.t['snap_ptr0'],
                                  store.num_ent, None, bad, 0.0, num_cols=RS.NUM_ENT)
    with pytest.raises(ValueError):
        RC.RecurrencePrior(1.0)
    with pytest.raises(ValueError):
        RC.RecurrencePrior(0.5, half_life=0)
    empty = tuple(x[:0] for x in q)
    assert mix_direct(store, 0, empty, None, prior, num_cols=RS.NUM_ENT).shape == (0, RS.NUM_ENT)      # n == 0: a no-op


# ---- 6. the model path -------------------------------------------------------------------------------------------------
def model_queries(facts):
    t = facts[:, 3]
    late = facts[t >= 10 * RS.STEP]
    return late[np.random.RandomState(12).choice(len(late), 48, replace=False)].copy()


def hand_mixed(w, queries, prior, dev):
    """{side: the mixed matrix} computed by hand: forecast_scores, then one mix launch per direction."""
    net, obs = w['net'], w['obs']
    sub_pred, ob_pred = net.forecast_scores(obs, queries)
    s, r, o, t = queries.T
    store = obs.device
    return {'sub': mix_direct(store, 1, (o, r, t, t), sub_pred, prior), 'ob': mix_direct(store, 0, (s, r, t, t), ob_pred, prior)}


def test_prior_none_is_todays_path_and_a_prior_is_one_mix_launch(dev):
    import filter_index as FI
    import recurrence as RC
    import renet_hip as K
    w = world(dev)
    net, obs, facts = w['net'], w['obs'], w['facts']
    queries = model_queries(facts)
    base = net.evaluate_forecast(obs, queries)
    none = net.evaluate_forecast(obs, queries, prior=None)
    for name in SETTINGS:
        assert np.array_equal(base[0][name], none[0][name])
    assert np.array_equal(base[1], none[1])
    prior = RC.RecurrencePrior(0.3, 100)
    got_ranks, got_loss = net.evaluate_forecast(obs, queries, prior=prior)
    mixed = hand_mixed(w, queries, prior, dev)
    s, r, o, t = queries.T
    index = FI.filter_index_for(obs.device, obs.device.quads)
    losses = []
    for col, side, name, key, gold in ((0, 's', 'sub', o, s), (1, 'o', 'ob', s, o)):
        cnt, ls = K.rank_rows3(mixed[name], i32(gold, dev), *index.ranges_both(side, np.stack((key, r, t), axis=1), dev))
        cnt = cnt.cpu().numpy().astype(np.float64)
        for k, setting in enumerate(SETTINGS):
            assert np.array_equal(got_ranks[setting][:, col], cnt[2 * k] + (cnt[2 * k + 1] - 1.0) / 2 + 1), (setting, name)
        losses.append(ls)
    assert np.array_equal(got_loss, torch.stack(losses, dim=1).sum(dim=1).cpu().numpy())
    assert any(not np.array_equal(got_ranks[name], base[0][name]) for name in SETTINGS)    # the prior does move ranks
    # evaluate_observed on the stream's own positions: the same keyword, the same numbers
    pos = np.arange(len(facts))[facts[:, 3] >= 10 * RS.STEP][:40]
    a = net.evaluate_forecast(obs, facts[pos], prior=prior)
    b = net.evaluate_observed(obs, pos, prior=prior)
    assert all(np.array_equal(a[0][name], b[0][name]) for name in SETTINGS) and np.array_equal(a[1], b[1])
    # forecast_scores and forecast_topk
    fs = net.forecast_scores(obs, queries, prior=prior)
    assert torch.equal(fs[0], mixed['sub']) and torch.equal(fs[1], mixed['ob'])
    top = net.forecast_topk(obs, queries, k=7, prior=prior)
    for name in ('sub', 'ob'):
        want = K.topk_rows(mixed[name], 7)
        assert all(torch.equal(x, y) for x, y in zip(top[name], want)), name
    plain = net.forecast_topk(obs, queries, k=7)
    again = net.forecast_topk(obs, queries, k=7, prior=None)
    assert all(torch.equal(x, y) for name in ('sub', 'ob') for x, y in zip(plain[name], again[name]))


def test_online_loop_with_a_prior_equals_the_host_rebuilt_streams(dev):
    import recurrence as RC
    w = world(dev)
    net, gnet, facts = w['net'], w['gnet'], w['facts']
    n = int(np.searchsorted(facts[:, 3], 10 * RS.STEP))
    head, quads = facts[:n], facts[n:]
    prior = RC.RecurrencePrior(0.3, 24)
    obs = stream_of(head)
    obs.resident(net, gnet)
    ranks, loss, log = net.evaluate_online(obs, quads, gnet, None, steps=0, all_triplets=facts, prior=prior)
    assert 'tables' in net.last_online.device._pair and len(net.last_online) == len(facts)
    cur, want_ranks, want_loss = stream_of(head), {name: [] for name in SETTINGS}, []
    for t in np.unique(quads[:, 3]):
        q = quads[quads[:, 3] == t]
        cur.resident(net, gnet)
        r, l = net.evaluate_forecast(cur, q, all_triplets=facts, prior=prior)
        for name in SETTINGS:
            want_ranks[name].append(r[name])
        want_loss.append(l)
        cur = cur.extended(q)
    for name in SETTINGS:
        assert np.array_equal(ranks[name], np.concatenate(want_ranks[name])), name
    assert np.array_equal(loss, np.concatenate(want_loss))
    plain = net.evaluate_online(stream_of_resident(head, net, gnet), quads, gnet, None, steps=0, all_triplets=facts)
    assert any(not np.array_equal(plain[0][name], ranks[name]) for name in SETTINGS)
    assert net.last_online.device._pair == {}                                          # no prior: no tables, today's launches


def stream_of_resident(facts, net, gnet):
    obs = stream_of(facts)
    obs.resident(net, gnet)
    return obs
