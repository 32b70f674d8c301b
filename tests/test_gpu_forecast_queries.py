"""GPU tests of the open-query forecasts under the observed protocol (run with -m gpu on an MI355X): the lookup kernel
renet_query_histories against its host statement preprocess.HistoryIndex.lookup, gpu_builder.QueryStore, and
RENet.forecast_scores / forecast_topk / evaluate_forecast / forecast_events on the small stream of tests/observed_stream.py.
What pins the MEANING: queries that are stream facts give the observed pass bit for bit (test 3); queries that are no facts
give what the observed pass gives on a COMPARISON stream that holds them as facts, and what the oracle's restatement of the
reference forward gives on that stream's histories (tests 4, 5, 7).  A comparison store shares the base store's global table
row by timestamp, so that the histories are the only thing that could differ."""
import copy

import numpy as np
import pytest
import torch

from helpers import O, fixtures, global_shapes, renet_shapes
from test_gpu_parity import ATOL, RTOL            # the tolerance of logits against the reference golden, same GEMM mode

import observed_stream as S

pytestmark = pytest.mark.gpu

SETTINGS = ('raw', 'filtered', 'time_filtered')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _models(dev, d):
    import global_model as GM
    import model as M
    params = fixtures.make_params(41, renet_shapes(S.NUM_ENT, S.NUM_RELS, d))
    net = M.RENet(S.NUM_ENT, d, S.NUM_RELS, dropout=0.0, seq_len=S.SEQ_LEN)
    gnet = GM.RENet_global(S.NUM_ENT, d, S.NUM_RELS, dropout=0.0, seq_len=S.SEQ_LEN, num_k=10, maxpool=1)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    gnet.load_state_dict({k: torch.from_numpy(v) for k, v in
                          fixtures.make_params(42, global_shapes(S.NUM_ENT, S.NUM_RELS, d)).items()})
    return net.to(dev).eval(), gnet.to(dev).eval(), params


_WORLDS = {}


def _world(dev, d):
    """Model and resident stream per hidden size (made once, shared and left unchanged)."""
    if d not in _WORLDS:
        import preprocess as P
        splits = S.make()
        S.check_cases(*splits)
        obs = P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
        net, gnet, params = _models(dev, d)
        store = obs.resident(net, gnet)
        idx = np.concatenate((obs.positions('valid'), obs.positions('test')))
        _WORLDS[d] = dict(obs=obs, net=net, gnet=gnet, params=params, store=store, idx=idx, quads=obs.allq[idx], d=d)
    return _WORLDS[d]


def _comparison(w, dev, allq2):
    """The resident ObservedStream of the fact array allq2 with the SAME global table as w's store: the base rows by timestamp,
    a zero row for a timestamp the base does not have (no history step reads it) -> (stream, store, {t: row on the CPU})."""
    import gpu_builder
    import preprocess as P
    t = allq2[:, 3]
    obs2 = P.ObservedStream((allq2[t < S.SPLIT_T[0]], allq2[t >= S.SPLIT_T[0]]), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    row = {int(tt): w['store'].glob[k] for k, tt in enumerate(w['obs'].times)}
    ge = {int(tt): row.get(int(tt), torch.zeros(w['d'], device=dev)) for tt in obs2.times}
    return obs2, gpu_builder.ObservedStore(obs2, ge, w['d'], dev), {tt: v.cpu() for tt, v in ge.items()}


def _oracle_scores(w, allq2, pos, ge):
    """{'ob': [n, N_ent], 'sub': ...} float64: the oracle's restatement of the reference forward (model.py:64-104) for the rows
    pos of allq2 on that array's own histories and graphs, un-permuted (as tests/test_gpu_observed_eval.py does it)."""
    op = {k: torch.from_numpy(v) for k, v in w['params'].items()}
    ogd = O.build_graph_dict(allq2, S.NUM_RELS)
    sh, oh, _ = O.build_histories(allq2, S.NUM_ENT, history_len=S.SEQ_LEN)
    ref = {}
    with torch.no_grad():
        for name, subject, h in (('ob', True, sh), ('sub', False, oh)):
            _, parts = O.renet_forward_loss(op, allq2[pos], [h[0][i] for i in pos], [h[1][i] for i in pos], ogd, ge, S.NUM_RELS,
                                            S.SEQ_LEN, subject=subject, return_parts=True)
            full = np.empty((len(pos), S.NUM_ENT), dtype=np.float64)
            full[parts['bg'].perm] = parts['ob_pred'].double().numpy()
            ref[name] = full
    return ref


def _queries_at(allq, t_star, seed=7, n=40):
    """n queries (s, r, o, t*) from a fixed seed that are (mostly) no facts: (0, 1, ., t*), a query on NEW_ENT, a duplicate
    pair and (s, r) pairs the stream never holds; asserted here."""
    rng = np.random.RandomState(seed + t_star)
    q = np.stack((rng.randint(0, S.NUM_ENT - 1, n), rng.randint(0, S.NUM_RELS, n), rng.randint(0, S.NUM_ENT - 1, n),
                  np.full(n, t_star)), axis=1).astype(np.int64)
    q[0] = (0, 1, 11, t_star)
    q[1] = (S.NEW_ENT, 2, 5, t_star)
    q[2] = (6, 0, S.NEW_ENT, t_star)
    q[4] = q[3]
    known = set(map(tuple, allq[:, :2].tolist()))
    assert sum(tuple(x) not in known for x in q[:, :2].tolist()) >= 3
    facts = set(map(tuple, allq.tolist()))
    assert sum(tuple(x) not in facts for x in q.tolist()) >= n - 3
    return q


def _inserted(allq, q, t_star):
    """allq with q inserted as facts at the end of timestamp t* -> (the array, the positions of the inserted rows)."""
    at = int(np.searchsorted(allq[:, 3], t_star, side='right'))
    return np.concatenate((allq[:at], q, allq[at:])), np.arange(at, at + len(q))


def _filter_sets(allq, quads):
    """Per query, by brute force over the fact array: {'ob': [(agnostic, aware)], 'sub': [...]} -- the entities that complete
    (s, r, ?) / (?, r, o) at any time and at the query's own."""
    out = {'ob': [], 'sub': []}
    for s, r, o, t in quads.tolist():
        for name, key, kc, vc in (('ob', s, 0, 2), ('sub', o, 2, 0)):
            m = (allq[:, kc] == key) & (allq[:, 1] == r)
            out[name].append((set(allq[m, vc].tolist()), set(allq[m & (allq[:, 3] == t), vc].tolist())))
    return out


# ---- 2. the lookup kernel against the host statement -----------------------------------------------------------------
def _synthetic_index(history_len):
    """Quadruples with a time unit of 24 in which entity e has, per role, a chosen number of snapshots: 0, 1, history_len,
    history_len + 1 and 70 (a search deeper than six steps) as subject, the same numbers in another order as object."""
    counts = [0, 1, history_len, history_len + 1, 70]
    rows = []
    for e, (cs, co) in enumerate(zip(counts, counts[::-1])):
        for j in range(cs):                                  # subject e active at steps 2 + e, 2 + e + 1, ... (two facts each)
            rows += [(e, 0, 5, 24 * (2 + e + j)), (e, 1, 6, 24 * (2 + e + j))]
        for j in range(co):                                  # object e active at every other step
            rows.append((6, 2, e, 24 * (1 + 2 * j)))
    quads = np.asarray(sorted(rows, key=lambda x: x[3]), dtype=np.int64)
    return quads, 7, counts


@pytest.mark.parametrize('history_len', [1, 3, 10])
def test_lookup_kernel_equals_the_host_statement(dev, history_len):
    import preprocess as P
    import renet_hip as K
    quads, num_ent, counts = _synthetic_index(history_len)
    hist = [P.HistoryIndex(quads, role, history_len, num_ent) for role in ('s', 'o')]
    assert [int(np.diff(hist[0].ent_ptr)[e]) for e in range(5)] == counts
    assert [int(np.diff(hist[1].ent_ptr)[e]) for e in range(5)] == counts[::-1]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    ent_ptr, snap_t = [i32(h.ent_ptr) for h in hist], [i32(h.snap_t) for h in hist]
    # every entity id from -1 to num_ent against as_of: negative, before the first snapshot, every snapshot time, strictly
    # between two (no multiple of 24), after the last
    t_max = int(quads[:, 3].max())
    as_of = np.concatenate(([-5, -1, 0, 1, 23], np.arange(24, t_max + 25, 24), np.arange(24, t_max + 25, 24) + 7, [t_max + 1000]))
    grid = np.stack(np.meshgrid(np.arange(-1, num_ent + 1), as_of, indexing='ij'), axis=-1).reshape(-1, 2)
    rng = np.random.RandomState(history_len)
    for n in (1, 63, 64, 65, 1025, len(grid)):
        pick = grid[rng.permutation(len(grid))[:n]] if n <= len(grid) else grid[rng.randint(0, len(grid), n)]
        if n == 1:
            pick = np.asarray([[4, 24 * 40 + 7]])            # the 70-snapshot entity, between two snapshots
        ent = np.stack((pick[:, 0], pick[rng.permutation(n), 0]))               # subjects, objects
        a = pick[:, 1]
        win = K.query_histories(ent_ptr, snap_t, num_ent, history_len, i32(ent), i32(a))
        assert win.shape == (2, 2, n) and win.dtype == torch.int32
        got = win.cpu().numpy()
        for role in (0, 1):
            first, count = hist[role].lookup(ent[role], a)
            assert np.array_equal(got[0, role], first) and np.array_equal(got[1, role], count), (n, role)
    # the full grid holds every case the kernel distinguishes
    f, c = hist[0].lookup(grid[:, 0], grid[:, 1])
    assert c.max() == min(history_len, 70) and (c == 0).any() and ((c > 0) & (c < history_len)).any() == (history_len > 1)
    assert (f[grid[:, 0] == 4] > hist[0].ent_ptr[4]).any()   # a window that does not start at the entity's first snapshot


# ---- 3. queries that are the stream's own facts ----------------------------------------------------------------------
def _same_topk(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('on_device', [False, True])
def test_stream_facts_as_queries_give_the_observed_pass_bit_for_bit(dev, on_device, monkeypatch):
    w = _world(dev, 100)
    net, obs, idx = w['net'], w['obs'], w['idx']
    q = torch.from_numpy(w['quads'].astype(np.int32)).to(dev) if on_device else w['quads']
    want = net.observed_scores(obs, idx)
    got = net.forecast_scores(obs, q)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for relation in (False, True):
        a, b = net.evaluate_forecast(obs, q, relation=relation), net.evaluate_observed(obs, idx, relation=relation)
        for name in SETTINGS:
            assert np.array_equal(a[0][name], b[0][name]), name
        assert np.array_equal(a[1], b[1])
        if relation:
            assert all(np.array_equal(a[2][f], b[2][f]) for f in ('rank', 'loss', 'entity_loss'))
    a = net.evaluate_forecast(obs, q, max_batch=50)[0]
    b = net.evaluate_observed(obs, idx, max_batch=50)[0]
    assert all(np.array_equal(a[name], b[name]) for name in SETTINGS)
    for setting in SETTINGS:
        ref = net.predict_topk_observed(obs, idx, k=10, setting=setting, keep_gold=False)
        if on_device and setting == 'raw':
            # no query content may come back to the host: any device-to-host copy of a tensor fails the call
            def refuse(self, *a, **k):
                raise AssertionError('forecast_topk read a tensor back to the host')
            with monkeypatch.context() as m:
                m.setattr(torch.Tensor, 'cpu', refuse)
                m.setattr(torch.Tensor, 'tolist', refuse)
                m.setattr(torch.Tensor, 'item', refuse)
                got = net.forecast_topk(obs, q, k=10, setting=setting)
        else:
            got = net.forecast_topk(obs, q, k=10, setting=setting)
        assert sorted(got) == ['ob', 'sub']
        for name in ('sub', 'ob'):
            assert len(got[name]) == 4 and _same_topk(got[name], ref[name]), (setting, name)
    # the resident store is accepted in place of the stream
    again = net.forecast_scores(w['store'], q)
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])


def test_query_store_windows_equal_the_stream_index_and_validate(dev):
    import gpu_builder
    w = _world(dev, 100)
    obs, store = w['obs'], w['store']
    qs = store.queries(obs.allq)
    assert isinstance(qs, gpu_builder.QueryStore) and qs.n_quads == len(obs.allq) and qs.quads is not obs.allq
    for r, h in enumerate((obs.hist_s, obs.hist_o)):
        assert np.array_equal(qs.t['h_first%d' % r].cpu().numpy(), h.first)
        assert np.array_equal(qs.t['h_count%d' % r].cpu().numpy(), h.count)
    for col, name in enumerate(('q_s', 'q_r', 'q_o')):
        assert np.array_equal(qs.t[name].cpu().numpy(), obs.allq[:, col])
    assert qs.glob is store.glob and qs.facts is store.quads
    # an absent side: an empty window and entity 0 where the builder gathers; the host copy keeps the -1
    qs = store.queries(np.asarray([[3, 1, -1, 12], [-1, 0, 4, 12]]))
    assert qs.t['q_o'].tolist() == [0, 4] and qs.t['q_s'].tolist() == [3, 0]
    assert qs.t['h_count1'].tolist()[0] == 0 and qs.t['h_count0'].tolist()[1] == 0
    assert qs.quads[0, 2] == -1 and qs.quads[1, 0] == -1 and qs.sides_present() == (True, True)
    for bad in ([[0, S.NUM_RELS, 1, 5]], [[0, -1, 1, 5]], [[S.NUM_ENT, 0, 1, 5]], [[0, 0, -2, 5]]):
        with pytest.raises(ValueError):
            store.queries(np.asarray(bad))
    with pytest.raises(ValueError):
        store.queries(np.zeros((0, 4), dtype=np.int64))


# ---- 4. queries that are no facts, against a stream that holds them ---------------------------------------------------
@pytest.mark.parametrize('d', [100, 200])
@pytest.mark.parametrize('t_star', [10, 21, 24])
def test_queries_that_are_no_facts_equal_the_observed_pass_on_an_appended_stream(dev, d, t_star):
    """Bit-identical to the observed pass on the comparison stream on the MI355X (profiles/forecast_queries.md); asserted
    within the score tolerance, as the issue of this feature sets it."""
    w = _world(dev, d)
    net, obs = w['net'], w['obs']
    q = _queries_at(obs.allq, t_star)
    allq2, pos = _inserted(obs.allq, q, t_star)
    assert np.array_equal(allq2[pos], q)
    obs2, store2, ge = _comparison(w, dev, allq2)
    # facts at t* enter no history of a query at t*: the windows are those of the base index
    for h, h2, col in ((obs.hist_s, obs2.hist_s, 0), (obs.hist_o, obs2.hist_o, 2)):
        assert np.array_equal(h.lookup(q[:, col], q[:, 3])[1], h2.count[pos])
    got = net.forecast_scores(obs, q)
    want = net.observed_scores(store2, pos)
    ref = _oracle_scores(w, allq2, pos, ge)
    for name, g, x in (('sub', got[0], want[0]), ('ob', got[1], want[1])):
        print('d', d, 't*', t_star, name, 'bit-identical to the appended stream:', bool(torch.equal(g, x)),
              'max |diff|', float((g - x).abs().max()), 'max |score - oracle|', float(np.abs(g.cpu().numpy() - ref[name]).max()))
        np.testing.assert_allclose(g.cpu().numpy(), x.cpu().numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g.cpu().numpy(), ref[name], rtol=RTOL, atol=ATOL)
    if t_star > obs.times[-1]:
        assert t_star not in obs.graph_dict and w['store'].glob.shape[0] == len(obs.times)     # no new row was needed


# ---- 5. as-of --------------------------------------------------------------------------------------------------------
def test_histories_as_of_an_earlier_timestamp(dev):
    """The comparison stream holds the facts with t < 18 followed by the test quadruples AT 18 (with their own later
    timestamps they would enter each other's histories): the inserted rows' histories are exactly the stale ones."""
    w = _world(dev, 100)
    net, obs = w['net'], w['obs']
    test = obs.positions('test')
    q = obs.allq[test]
    assert q[:, 3].min() >= 20
    q18 = q.copy()
    q18[:, 3] = 18
    allq2 = np.concatenate((obs.allq[obs.allq[:, 3] < 18], q18))
    pos = np.arange(len(allq2) - len(q), len(allq2))
    obs2, store2, _ = _comparison(w, dev, allq2)
    got = net.forecast_scores(obs, q, as_of=18)
    want = net.observed_scores(store2, pos)
    fresh = net.observed_scores(obs, test)
    for g, x, f in zip(got, want, fresh):
        print('as of 18: bit-identical', bool(torch.equal(g, x)), 'max |diff|', float((g - x).abs().max()),
              'max |stale - fresh|', float((g - f).abs().max()))
        np.testing.assert_allclose(g.cpu().numpy(), x.cpu().numpy(), rtol=RTOL, atol=ATOL)
        assert float((g - f).abs().max()) > 100 * ATOL                          # the stale histories are other histories
    # a per-query as_of: the array form of the same scalar, and horizon 1 = the observed pass exactly
    again = net.forecast_scores(obs, q, as_of=np.full(len(q), 18))
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    a = net.evaluate_forecast(obs, q, as_of=obs.horizon_as_of(test, 1))
    b = net.evaluate_observed(obs, test)
    assert all(np.array_equal(a[0][name], b[0][name]) for name in SETTINGS) and np.array_equal(a[1], b[1])
    # horizon 3: t = 20 and 23 open a block, 21 and 22 forecast from the facts before 20 -- other numbers than horizon 1
    h3 = obs.horizon_as_of(test, 3)
    c = net.evaluate_forecast(obs, q, as_of=h3)
    stale = h3 < q[:, 3]
    assert stale.any() and not stale.all() and np.all(np.isfinite(c[1])) and not np.array_equal(c[1][stale], b[1][stale])
    with pytest.raises(ValueError):
        net.forecast_scores(obs, q, as_of=q[:, 3] + 1)
    with pytest.raises(ValueError):
        net.forecast_scores(obs, torch.from_numpy(q.astype(np.int32)).to(dev), as_of=24)


# ---- 6. an absent side -----------------------------------------------------------------------------------------------
def test_absent_side_equals_a_twin_with_an_empty_history(dev, monkeypatch):
    import model as M
    w = _world(dev, 100)
    net, obs = w['net'], w['obs']
    assert not obs.hist_o.lookup(np.full(22, S.NEW_ENT), np.arange(22))[1].any()          # NEW_ENT has no history up to 21
    rng = np.random.RandomState(3)
    n = 12
    open_ = np.stack((rng.randint(0, S.NUM_ENT - 1, n), rng.randint(0, S.NUM_RELS, n), np.full(n, -1),
                      rng.randint(1, 22, n)), axis=1).astype(np.int64)
    twin = open_.copy()
    twin[:, 2] = S.NEW_ENT
    sub_a, ob_a = net.forecast_scores(obs, open_)
    sub_b, ob_b = net.forecast_scores(obs, twin)
    assert sub_a is None and sub_b is not None and torch.equal(ob_a, ob_b)
    # the same with the subject absent
    mirror = open_[:, [2, 1, 0, 3]]
    sub_c, ob_c = net.forecast_scores(obs, mirror)
    assert ob_c is None and sub_c.shape == (n, S.NUM_ENT)
    # in an otherwise identical MIXED batch (stream facts around the open query)
    facts = obs.allq[(obs.allq[:, 3] >= 5) & (obs.allq[:, 3] <= 21)][::7]
    mixed_a, mixed_b = np.concatenate((facts, open_[:3])), np.concatenate((facts, twin[:3]))
    sa, oa = net.forecast_scores(obs, mixed_a)
    sb, ob = net.forecast_scores(obs, mixed_b)
    assert torch.equal(oa, ob) and sa is not None and torch.equal(sa[:len(facts)], sb[:len(facts)])
    # forecast_topk: one side asked for is one score GEMM, and the twins agree
    calls = []
    real = M._linear_eval
    monkeypatch.setattr(M, '_linear_eval', lambda lin, x: calls.append(1) or real(lin, x))
    for setting in SETTINGS:
        del calls[:]
        ta = net.forecast_topk(obs, mixed_a, k=5, setting=setting, sides=('ob',))
        assert len(calls) == 1 and sorted(ta) == ['ob']
        tb = net.forecast_topk(obs, mixed_b, k=5, setting=setting, sides=('ob',))
        assert _same_topk(ta['ob'], tb['ob']), setting
    with pytest.raises(ValueError):
        net.forecast_topk(obs, mixed_a, sides=('both',))
    with pytest.raises(ValueError):
        net.evaluate_forecast(obs, mixed_a)                                       # labelled queries only


def test_a_batch_of_empty_histories_takes_the_zero_state_rows(dev, monkeypatch):
    w = _world(dev, 100)
    net, obs = w['net'], w['obs']
    rng = np.random.RandomState(4)
    n = 9
    q = np.stack((rng.randint(0, S.NUM_ENT, n), rng.randint(0, S.NUM_RELS, n), rng.randint(0, S.NUM_ENT, n),
                  np.zeros(n, dtype=np.int64)), axis=1).astype(np.int64)

    def refuse(*a, **k):
        raise AssertionError('the encoder was launched for a batch without a history step')
    monkeypatch.setattr(net.aggregator, 'encode', refuse)
    sub_pred, ob_pred = net.forecast_scores(obs, q)
    qd = torch.from_numpy(q).to(dev)
    with torch.no_grad():
        ent, rel, zero = net.ent_embeds.double(), net.rel_embeds.double(), torch.zeros(n, 100, device=dev).double()
        lin = lambda f: f @ net.linear.weight.double().t() + net.linear.bias.double()
        want_ob = lin(torch.cat((ent[qd[:, 0]], zero, rel[qd[:, 1]]), dim=1))
        want_sub = lin(torch.cat((ent[qd[:, 2]], zero, rel[S.NUM_RELS + qd[:, 1]]), dim=1))
    np.testing.assert_allclose(ob_pred.cpu().numpy(), want_ob.cpu().numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(sub_pred.cpu().numpy(), want_sub.cpu().numpy(), rtol=RTOL, atol=ATOL)
    # the stream's own first timestamp: the S == 0 branch of the observed pass, bit for bit
    first = np.nonzero(obs.allq[:, 3] == obs.times[0])[0]
    a, b = net.forecast_scores(obs, obs.allq[first]), net.observed_scores(obs, first)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 7. top-k and events without gold --------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 10, S.NUM_ENT + 5])
def test_topk_equals_numpy_sorting_of_the_forecast_scores(dev, k):
    w = _world(dev, 100)
    net, obs = w['net'], w['obs']
    q = np.concatenate((_queries_at(obs.allq, 21), _queries_at(obs.allq, 24)[:8], obs.allq[obs.positions('test')][:20]))
    sets = _filter_sets(obs.allq, q)
    assert any(a - b for a, b in sets['ob']) and any(len(b) >= 2 for a, b in sets['ob'])
    sub_pred, ob_pred = (x.cpu().numpy() for x in net.forecast_scores(obs, q))
    lse = {name: torch.logsumexp(torch.from_numpy(p).double(), dim=1).numpy() for name, p in (('sub', sub_pred), ('ob', ob_pred))}
    for setting in SETTINGS:
        got = net.forecast_topk(obs, q, k=k, setting=setting)
        for name, pred in (('sub', sub_pred), ('ob', ob_pred)):
            gi, gv, gl, gn = (x.cpu().numpy() for x in got[name])
            assert gi.shape == gv.shape == gl.shape == (len(q), k) and gn.shape == (len(q),)
            for i in range(len(q)):
                agnostic, aware = sets[name][i]
                out = set() if setting == 'raw' else set(agnostic if setting == 'filtered' else aware)
                cand = np.asarray([c for c in range(S.NUM_ENT) if c not in out], dtype=np.int64)
                order = cand[np.lexsort((cand, -pred[i, cand]))][:k]
                m = len(order)
                assert gn[i] == m and gi[i, :m].tolist() == order.tolist() and np.all(gi[i, m:] == -1), (setting, name, i)
                assert np.array_equal(gv[i, :m], pred[i, order]) and np.all(np.isneginf(gv[i, m:]))
                np.testing.assert_allclose(gl[i, :m], pred[i, order] - lse[name][i], rtol=1e-5, atol=1e-5)
    # the queries themselves are never the known facts: an explicit all_triplets = the stream is the default
    a = net.forecast_topk(obs, q, k=k, setting='filtered', all_triplets=obs.allq)
    b = net.forecast_topk(obs, q, k=k, setting='filtered')
    assert _same_topk(a['ob'], b['ob']) and _same_topk(a['sub'], b['sub'])
    with pytest.raises(ValueError):
        net.forecast_topk(obs, q, k=k, setting='best')


@pytest.mark.parametrize('direction', ['ob', 'sub'])
def test_events_past_the_end_equal_the_event_pass_on_an_appended_stream(dev, direction):
    w = _world(dev, 100)
    net, obs = w['net'], w['obs']
    k = 7
    q = _queries_at(obs.allq, 24)
    allq2, pos = _inserted(obs.allq, q, 24)
    obs2, store2, _ = _comparison(w, dev, allq2)
    ents = q[:, 0] if direction == 'ob' else q[:, 2]
    got = [x.cpu().numpy() for x in net.forecast_events(obs, ents, t=24, k=k, direction=direction)]
    # one more than k from the comparison: the gap behind the k-th place is needed too
    ref = [x.cpu().numpy() for x in net.predict_events_observed(store2, pos, k=k + 1)[direction]]
    assert got[0].shape == got[1].shape == got[2].shape == (len(q), k) and np.all(got[3] == k)
    np.testing.assert_allclose(got[2], ref[2][:, :k], rtol=RTOL, atol=ATOL)
    tol = ATOL + RTOL * np.abs(ref[2])
    gap = np.minimum(np.concatenate((np.full((len(q), 1), np.inf), ref[2][:, :-1] - ref[2][:, 1:]), axis=1)[:, :k],
                     (ref[2][:, :-1] - ref[2][:, 1:])[:, :k])
    clear = gap > 2 * tol[:, :k]
    print(direction, 'slots separated by more than the tolerance', float(clear.mean()), 'lists bit-identical',
          bool(np.array_equal(got[0], ref[0][:, :k]) and np.array_equal(got[1], ref[1][:, :k]) and np.array_equal(got[2], ref[2][:, :k])))
    assert clear.mean() > 0.5                                  # (a property of the comparison's scores: the index check is not vacuous)
    assert np.array_equal(got[0][clear], ref[0][:, :k][clear]) and np.array_equal(got[1][clear], ref[1][:, :k][clear])
    # a device tensor of entities and a per-entity time give the same lists
    again = net.forecast_events(obs, torch.from_numpy(ents.astype(np.int32)).to(dev), t=np.full(len(ents), 24), k=k,
                                direction=direction)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(again, got))
    # filtered: no pair that is a known fact (at any time / at the query's own) is listed, and such pairs exist
    ec, oc = (0, 2) if direction == 'ob' else (2, 0)
    for setting, t in (('filtered', 24), ('time_filtered', 21)):
        raw = [x.cpu().numpy() for x in net.forecast_events(obs, ents, t=t, k=S.NUM_RELS * S.NUM_ENT, direction=direction)]
        flt = [x.cpu().numpy() for x in net.forecast_events(obs, ents, t=t, k=S.NUM_RELS * S.NUM_ENT, direction=direction,
                                                            setting=setting)]
        dropped = 0
        for i, e in enumerate(ents.tolist()):
            m = (obs.allq[:, ec] == e) & ((obs.allq[:, 3] == t) if setting == 'time_filtered' else True)
            known = set(zip(obs.allq[m, 1].tolist(), obs.allq[m, oc].tolist()))
            listed = set(zip(flt[0][i, :flt[3][i]].tolist(), flt[1][i, :flt[3][i]].tolist()))
            assert not (listed & known) and len(listed) == S.NUM_RELS * S.NUM_ENT - len(known), (setting, i)
            assert raw[3][i] == S.NUM_RELS * S.NUM_ENT
            dropped += len(known)
        assert dropped > 0
    with pytest.raises(ValueError):
        net.forecast_events(obs, ents, t=24, direction='both')


# ---- 8. state --------------------------------------------------------------------------------------------------------
STATE = ('s_hist_test', 'o_hist_test', 's_hist_test_t', 'o_hist_test_t', 's_his_cache', 'o_his_cache', 's_his_cache_t',
         'o_his_cache_t', 'graph_dict', 'global_emb', 'preds_list_s', 'preds_ind_s', 'preds_list_o', 'preds_ind_o', 'data')


def _same_content(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    if isinstance(a, dict):
        return list(a.keys()) == list(b.keys()) and all(_same_content(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_content(x, y) for x, y in zip(a, b))
    if hasattr(a, '__slots__') and not isinstance(a, (int, float)):                  # graph.TimeGraph
        return all(_same_content(getattr(a, f), getattr(b, f)) for f in ('ent', 'ls', 'r', 'lo'))
    return a == b


def test_forecasts_leave_model_state_and_resident_tables_untouched(dev):
    import model as M
    import utils as U
    w = _world(dev, 100)
    obs = w['obs']
    # a model in the state test.py has before its multi-step evaluation loop, with a store of its own
    net, gnet, _ = _models(dev, 100)
    tr, va, te = (obs.allq[obs.positions(k)] for k in ('train', 'valid', 'test'))
    H = {k: (obs.hist_s.to_lists(obs.positions(k)), obs.hist_o.to_lists(obs.positions(k))) for k in ('train', 'valid', 'test')}
    gd = U.build_graph_dict(tr, S.NUM_RELS)
    valid = torch.from_numpy(va)
    with torch.no_grad():
        net.global_emb = gnet.get_global_emb(np.unique(tr[:, 3]), gd)
        net.graph_dict = gd
        net.init_history(tr, H['train'][0], H['train'][1], valid, H['valid'][0], H['valid'][1], te, H['test'][0], H['test'][1])
        net.latest_time = valid[0][3]
    held = {k: getattr(net, k) for k in STATE}
    snap = copy.deepcopy({k: (dict(v) if k.startswith('preds_') else v) for k, v in held.items() if k != 'graph_dict'})
    latest, last_batch, glob_key = copy.deepcopy(net.latest_time), net.aggregator.last_batch, net.aggregator.glob_table._key
    store = obs.resident(net, gnet)
    obs.device = w['store']                                     # (the shared world's store stays the stream's)
    resident = {k: v.clone() for k, v in store.t.items()}
    glob, caps = store.glob.clone(), (store.cap_nodes, store.cap_edges)
    q21, q24 = _queries_at(obs.allq, 21), _queries_at(obs.allq, 24)

    def every_entry_point():
        return (net.forecast_scores(store, q21), net.forecast_scores(store, q24, as_of=20),
                net.forecast_topk(store, q24, k=3, setting='time_filtered'),
                net.evaluate_forecast(store, q21, relation=True, max_batch=16),
                net.forecast_events(store, q24[:9, 0], t=24, k=3, setting='filtered'))
    first = every_entry_point()
    second = every_entry_point()                                # repeatable in place
    assert _same_content(first, second)
    assert sorted(store.t) == sorted(resident) and all(torch.equal(store.t[k], resident[k]) for k in resident)
    assert torch.equal(store.glob, glob) and (store.cap_nodes, store.cap_edges) == caps
    for k in STATE:
        assert getattr(net, k) is held[k], k
        if k != 'graph_dict':
            now = getattr(net, k)
            assert _same_content(dict(now) if k.startswith('preds_') else now, snap[k]), k
    assert list(net.graph_dict.keys()) == list(gd.keys())
    assert _same_content(net.latest_time, latest) and net.aggregator.last_batch is last_batch
    assert net.aggregator.glob_table._key == glob_key
    # two QueryStores of one base pending at once: the second built and launched before the first is finalized
    qs1, qs2 = store.queries(q21), store.queries(q24, as_of=20)
    with torch.no_grad():
        p1 = M._observed_launch(net, qs1, np.arange(qs1.n_quads))
        p2 = M._observed_launch(net, qs2, np.arange(qs2.n_quads))
        f1, f2 = M._observed_features(net, qs1, p1), M._observed_features(net, qs2, p2)
        for (feat_ob, feat_sub, _, _), (sub_pred, ob_pred) in ((f1, first[0]), (f2, first[1])):
            assert torch.equal(M._linear_eval(net.linear, feat_sub), sub_pred)
            assert torch.equal(M._linear_eval(net.linear, feat_ob), ob_pred)
