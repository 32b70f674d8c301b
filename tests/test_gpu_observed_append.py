"""GPU tests of the device-side append of observed facts to a resident stream (run with -m gpu on an MI355X):
renet_store_append / renet_append_i32 behind gpu_builder.ObservedStore.appended and preprocess.ObservedStream.observe.  The
statement is exact: the appended store equals ObservedStore(extended(quads), ...) tensor for tensor under torch.equal, so
nothing here carries a tolerance.  Streams: the small one of tests/observed_stream.py, cut as in test_observed_append_cpu.py;
a 70 000-entity stream (ids beyond 16 bits, more entities than one workgroup covers); and one append of 270 000 facts (the
scan over the new facts carries across more block sums than its second pass takes at once)."""
import numpy as np
import pytest
import torch

import observed_stream as S
from test_observed_append_cpu import before, cases

pytestmark = pytest.mark.gpu

D = 100
SETTINGS = ('raw', 'filtered', 'time_filtered')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def allq():
    splits = S.make()
    S.check_cases(*splits)
    return np.concatenate(splits)


def cut3(allq, n, num_ent=S.NUM_ENT, num_rels=S.NUM_RELS, split_t=S.SPLIT_T):
    """The first n facts as (train, valid, test) at the stream's own split times (a split may be empty): appends go to test,
    so that the full stream's ranges come back."""
    import preprocess as P
    a, b = (min(n, int(np.searchsorted(allq[:, 3], t))) for t in split_t)
    return P.ObservedStream((allq[:a], allq[a:b], allq[b:n]), num_ent, num_rels, S.SEQ_LEN)


def rows_for(times, seed, d):
    """{t: row} on the CPU from a fixed seed per (seed, t): rows given explicitly, no global model involved."""
    return {int(t): torch.from_numpy(np.random.RandomState(1000 * seed + int(t)).randn(d).astype(np.float32)) for t in times}


def assert_stores_equal(got, want, what=''):
    assert sorted(got.t) == sorted(want.t), what
    for name in want.t:
        a, b = got.t[name], want.t[name]
        assert a.dtype == b.dtype == torch.int32 and a.shape == b.shape and torch.equal(a, b), (what, name)
    assert (got.T, got.n_glob, got.n_facts, got.n_quads) == (want.T, want.n_glob, want.n_facts, want.n_quads), what
    assert (got.num_ent, got.num_rels, got.history_len) == (want.num_ent, want.num_rels, want.history_len)
    assert got.glob.shape == want.glob.shape and torch.equal(got.glob, want.glob), what
    assert np.array_equal(got.quads, want.quads)
    for f in ('T', 'n_glob', 'n_facts', 'num_ent', 'num_rels'):
        assert getattr(got.c, f) == getattr(want.c, f), (what, f)
    for f in ('q_s', 'q_r', 'q_o', 'times', 'trip_ptr', 'trip_s', 'trip_r', 'trip_o', 'glob_times'):
        assert getattr(got.c, f) == got.t[f].data_ptr(), f                 # the struct names the NEW tensors
    for f in ('h_first', 'h_count', 'snap_t', 'snap_ptr', 'nbr_o'):
        assert list(getattr(got.c, f)) == [got.t[f + '0'].data_ptr(), got.t[f + '1'].data_ptr()], f


def append_and_rebuild(old, quads, dev, d, store=None, seeds=(1, 2)):
    """(appended store, rebuilt store): rows of the timestamps before the first appended one from seeds[0] on both sides,
    the later ones -- a replaced row of the old last timestamp among them -- from seeds[1]."""
    import gpu_builder as GB
    if store is None:
        store = GB.ObservedStore(old, rows_for(old.times, seeds[0], d), d, dev)
    ext = old.extended(quads)
    t0 = quads[0, 3] if len(quads) else None
    new_rows = rows_for([t for t in ext.times if len(quads) and t >= t0], seeds[1], d)
    table = rows_for(ext.times, seeds[0], d)
    table.update(new_rows)
    before_t = {n: v.clone() for n, v in store.t.items()}
    got = store.appended(quads, new_rows)
    torch.cuda.synchronize()
    for n, v in before_t.items():                                           # the old store's tensors are never written
        assert torch.equal(store.t[n], v), n
    return got, GB.ObservedStore(ext, table, d, dev)


# ---- 1. tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['t20..', 't23', 'inside_t22', 'inside_t22_only', 'after_first', 't21_new_entity', 'nothing'])
def test_appended_tables_equal_the_rebuilt_store(dev, allq, name):
    n_old, n_new = cases(allq)[name]
    old = cut3(allq, n_old)
    got, want = append_and_rebuild(old, allq[n_old:n_new], dev, 8)
    assert_stores_equal(got, want, name)
    assert got.obs._hist == {'s': None, 'o': None} and got._gstore is None           # nothing of the host side was rebuilt
    assert (got.cap_nodes, got.cap_edges) == (want.cap_nodes, want.cap_edges)
    for a, b in zip(got.subject_index(), want.subject_index()):                       # the host graph store, on first use
        assert torch.equal(a, b)


def test_chain_of_single_timestamp_appends(dev, allq):
    """23 appends of one timestamp each from the first timestamp alone, every store made from the appended one before it."""
    import gpu_builder as GB
    n = before(allq, 1)
    old = cut3(allq, n)
    store = GB.ObservedStore(old, rows_for(old.times, 1, 8), 8, dev)
    for t in range(1, S.NUM_T):
        n2 = before(allq, t + 1)
        got, want = append_and_rebuild(store.obs, allq[n:n2], dev, 8, store=store, seeds=(1, 1))
        assert_stores_equal(got, want, t)
        store, n = got, n2
    assert store.n_quads == len(allq)


def test_appended_validates_as_extended_does(dev, allq):
    import gpu_builder as GB
    old = cut3(allq, before(allq, 23))
    store = GB.ObservedStore(old, rows_for(old.times, 1, 8), 8, dev)
    rows = rows_for([24], 2, 8)
    for bad in (np.array([[0, 1, 2, 21]]), np.array([[0, 1, 2, 25], [0, 1, 2, 24]]), np.array([[S.NUM_ENT, 1, 2, 24]]),
                np.array([[0, S.NUM_RELS, 2, 24]])):
        with pytest.raises(ValueError) as a:
            old.extended(bad)
        with pytest.raises(ValueError) as b:
            store.appended(bad, rows)
        assert str(a.value) == str(b.value)
    with pytest.raises(ValueError):
        store.appended(np.array([[0, 1, 2, 24]]), {})                                  # the appended timestamp's row is missing
    with pytest.raises(ValueError):
        store.appended(np.array([[0, 1, 2, 24]]), rows_for([22, 24], 2, 8))            # 22 is not among the rows to replace


# ---- 2 - 5: with the models --------------------------------------------------------------------------------------------
_WORLD = {}


def world(dev, allq):
    """Models, the full resident stream, and the chain: cut before t = 20, resident(), then observe() 20, 21, 22, 23 one at
    a time (made once; every stream of the chain is kept, none is changed afterwards)."""
    if not _WORLD:
        import preprocess as P
        from test_gpu_forecast_queries import _models
        net, gnet, _ = _models(dev, D)
        full = P.ObservedStream(S.make(), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
        full.resident(net, gnet)
        chain = {20: cut3(allq, before(allq, 20))}
        chain[20].resident(net, gnet)
        for t in range(20, 24):
            chain[t + 1] = chain[t].observe(allq[before(allq, t):before(allq, t + 1)], gnet)
        _WORLD.update(net=net, gnet=gnet, full=full, chain=chain)
    return _WORLD


def test_observe_chain_equals_resident_of_the_full_stream(dev, allq):
    w = world(dev, allq)
    got, want = w['chain'][24], w['full']
    assert got.device is not None and got.device.obs is got and got.ranges == want.ranges
    bad = [int(t) for k, t in enumerate(want.times) if not torch.equal(got.device.glob[k], want.device.glob[k])]
    assert not bad, 'global rows that differ, by timestamp: %s' % bad
    assert_stores_equal(got.device, want.device, 'chain')
    # every link: the store of the stream cut before t, made resident from scratch
    for t in (21, 22, 23):
        ref = cut3(allq, before(allq, t))
        ref.resident(w['net'], w['gnet'])
        assert_stores_equal(w['chain'][t].device, ref.device, t)
    assert w['chain'][20].device is not w['chain'][21].device and w['chain'][20].device.n_quads == before(allq, 20)


def test_results_on_the_appended_store_equal_the_rebuilt_one(dev, allq):
    from test_gpu_forecast_queries import _queries_at
    w = world(dev, allq)
    net, got, want = w['net'], w['chain'][24], w['full']
    idx = want.positions('test')
    assert np.array_equal(idx, got.positions('test')) and len(idx) > 60
    a, b = net.observed_scores(got, idx), net.observed_scores(want, idx)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = net.evaluate_observed(got, idx, relation=True), net.evaluate_observed(want, idx, relation=True)
    for name in SETTINGS:
        assert np.array_equal(a[0][name], b[0][name]), name
    assert np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][f], b[2][f]) for f in ('rank', 'loss', 'entity_loss'))
    q = _queries_at(want.allq, 24)
    assert len(q) == 40
    for setting in SETTINGS:
        ta, tb = net.forecast_topk(got, q, k=10, setting=setting), net.forecast_topk(want, q, k=10, setting=setting)
        for side in ('sub', 'ob'):
            assert len(ta[side]) == 4 and all(torch.equal(x, y) for x, y in zip(ta[side], tb[side])), (setting, side)


def test_no_leak_from_the_future(dev, allq):
    """The store that knows only t < 22 (reached by observe) forecasts the facts of t = 22 as the full store scores them
    under observed histories: nothing of t >= 22 is in the full store's answer, nothing is missing from the short one's."""
    w = world(dev, allq)
    net, short, full = w['net'], w['chain'][22], w['full']
    assert short.times[-1] == 21 and len(short) == before(allq, 22)
    pos = np.arange(before(allq, 22), before(allq, 23))
    q = full.allq[pos]
    assert len(q) >= 15 and np.all(q[:, 3] == 22)
    got, want = net.forecast_scores(short, q), net.observed_scores(full, pos)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_a_batch_pending_on_the_old_store_survives_the_append(dev, allq):
    import model as M
    w = world(dev, allq)
    net, gnet = w['net'], w['gnet']
    old = cut3(allq, before(allq, 23))
    store = old.resident(net, gnet)
    idx = old.positions('test')
    with torch.no_grad():
        want = [x.clone() for x in M._observed_features(net, store, M._observed_launch(net, store, idx))[:2]]
        pending = M._observed_launch(net, store, idx)                      # enqueued on the old store, not finalized
        new = old.observe(allq[before(allq, 23):], gnet)
        got = M._observed_features(net, store, pending)[:2]
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(M._linear_eval(net.linear, got[0]), M._linear_eval(net.linear, want[0]))
    assert old.device is store and new.device is not store and new.device.n_quads == len(allq)
    a, b = net.observed_scores(store, idx), net.observed_scores(new, idx)  # both stores answer, alike: same histories
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 6. wide entity set, tables only -----------------------------------------------------------------------------------
def random_stream(num_ent, num_rels, per_t, seed):
    rng = np.random.RandomState(seed)
    parts = []
    for t, m in enumerate(per_t):
        parts.append(np.stack((rng.randint(0, num_ent, m), rng.randint(0, num_rels, m), rng.randint(0, num_ent, m),
                               np.full(m, t)), axis=1))
    return np.concatenate(parts).astype(np.int64)


def test_wide_entity_set(dev):
    num_ent = 70000
    allq = random_stream(num_ent, 7, (3000, 2900, 3100, 3000), 11)
    n_old = before(allq, 3)
    oldq, newq = allq[:n_old], allq[n_old:]
    for col in (0, 2):
        assert (oldq[:, col] > 65535).sum() > 100 and (newq[:, col] > 65535).sum() > 30
        fresh = ~np.isin(newq[:, col], oldq[:, col])                        # appended entities without an old snapshot
        assert fresh.any() and not fresh.all()
        assert len(np.unique(newq[:, col])) < len(newq)                     # and entities with several new facts
    old = cut3(allq, n_old, num_ent, 7, (2, 3))
    got, want = append_and_rebuild(old, newq, dev, 4)
    assert_stores_equal(got, want, 'wide')
    # the cut inside the last timestamp: joins and openings among 70 000 entities
    n_mid = n_old + 1500
    got, want = append_and_rebuild(cut3(allq, n_mid, num_ent, 7, (2, 3)), allq[n_mid:], dev, 4)
    assert_stores_equal(got, want, 'wide, inside t = 3')


def test_one_append_of_more_facts_than_the_block_sums_take_at_once(dev):
    """270 000 new facts: 264 block sums of 1024 flags, scanned 256 at a time with a carry."""
    num_ent = 1000
    allq = random_stream(num_ent, 3, (1000, 1000, 270000), 12)
    n_old = before(allq, 2) + 400                                           # (inside t = 2: joins as well)
    assert (len(allq) - n_old + 1 + 1023) // 1024 > 256
    old = cut3(allq, n_old, num_ent, 3, (1, 1))
    got, want = append_and_rebuild(old, allq[n_old:], dev, 4)
    assert_stores_equal(got, want, 'long append')
