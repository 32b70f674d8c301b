"""GPU tests of the rollout horizon under the observed protocol (run with -m gpu on an MI355X):
RENet.generate_events_observed and RENet.evaluate_rollout on the small stream of tests/observed_stream.py.  What pins the
meaning: the generated facts equal a brute-force restatement (observed_event_scores' blocks, every row's 16 best, V in
fp32, the reference's multiset rule); h = 1 is the forecast / observe loop bit for bit; at h > 1 the first timestamp of a
block is the loop's and every other one equals evaluate_forecast on a stream REBUILT ON THE HOST from the truth before the
block plus the generated facts.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from helpers import fixtures, global_shapes, renet_shapes

import event_select_statement as E
import observed_stream as S
from test_observed_append_cpu import before

pytestmark = pytest.mark.gpu

D, NUM_K = 100, 16
SEEDS = (124, 125)                        # model, global model (seeded random weights); chosen so that some generated fact is
                                          # true: test_the_seed_gives_a_rollout_worth_testing holds the choice to that
MULT = (5, 4, 3, 2, 1, 1)                 # the picks: the 6 most probable entities, 16 draws
BLOCK_FLOATS = 3 * S.NUM_RELS * S.NUM_ENT  # 3 entities per sub-block: 2 sub-blocks per direction
SETTINGS = ('raw', 'filtered', 'time_filtered')
TIMES = (20, 21, 22, 23)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def picks(t, side, prob):
    top = torch.topk(prob, len(MULT)).indices.cpu().numpy()
    return np.repeat(top, MULT)


def stream_of(facts):
    """The ObservedStream of a time-sorted fact array, cut at the small stream's own split times."""
    import preprocess as P
    a, b = (int(np.searchsorted(facts[:, 3], t)) for t in S.SPLIT_T)
    return P.ObservedStream((facts[:a], facts[a:b], facts[b:]), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)


_WORLD = {}


def world(dev):
    """Models, the stream before the test split (resident), the known facts, and the forecast / observe loop over the test
    split -- made once, shared, left unchanged."""
    if not _WORLD:
        import global_model as GM
        import model as M
        splits = S.make()
        S.check_cases(*splits)
        allq = np.concatenate(splits)
        net = M.RENet(S.NUM_ENT, D, S.NUM_RELS, dropout=0.0, seq_len=S.SEQ_LEN, num_k=NUM_K)
        gnet = GM.RENet_global(S.NUM_ENT, D, S.NUM_RELS, dropout=0.0, seq_len=S.SEQ_LEN, num_k=NUM_K, maxpool=1)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in
                             fixtures.make_params(SEEDS[0], renet_shapes(S.NUM_ENT, S.NUM_RELS, D)).items()})
        gnet.load_state_dict({k: torch.from_numpy(v) for k, v in
                              fixtures.make_params(SEEDS[1], global_shapes(S.NUM_ENT, S.NUM_RELS, D)).items()})
        net, gnet = net.to(dev).eval(), gnet.to(dev).eval()
        n20 = before(allq, 20)
        obs = stream_of(allq[:n20])
        obs.resident(net, gnet)
        test = allq[n20:]
        known = allq
        loop, cur = {}, obs
        for t in TIMES:
            q = test[test[:, 3] == t]
            loop[t] = net.evaluate_forecast(cur, q, all_triplets=known)
            index = cur.device._filter_index
            cur = cur.observe(q, gnet)
            cur.device._filter_index = index
        _WORLD.update(net=net, gnet=gnet, allq=allq, n20=n20, obs=obs, test=test, known=known, loop=loop)
    return _WORLD


def rows_equal(got, want, what):
    for name in SETTINGS:
        assert got[0][name].dtype == want[0][name].dtype and np.array_equal(got[0][name], want[0][name]), (what, name)
    assert np.array_equal(got[1], want[1]), (what, 'loss')


def cut_rows(res, sel):
    return {name: v[sel] for name, v in res[0].items()}, res[1][sel]


def brute_generate(w, obs, t):
    """The facts of timestamp t by brute force: observed_event_scores on the same QueryStore, every row's NUM_K best by
    (score descending, column ascending), V in fp32 in the stated order, the multiset rule."""
    import model as M
    net, gnet = w['net'], w['gnet']
    R, N = S.NUM_RELS, S.NUM_ENT
    facts = []
    for name in ('ob', 'sub'):
        with torch.no_grad():
            prob = gnet.predict(t, obs.graph_dict, subject=name == 'ob')[2]
        ents, mult = np.unique(picks(t, name, prob), return_counts=True)
        lprior = torch.log(prob[torch.from_numpy(ents).to(prob.device)]).cpu().numpy()
        none, zero, tt = np.full_like(ents, -1), np.zeros_like(ents), np.full_like(ents, t)
        quads = np.stack((ents, zero, none, tt) if name == 'ob' else (none, zero, ents, tt), axis=1)
        qs = M._query_store(obs, quads)
        B, off = (x.cpu().numpy() for x in net.observed_event_scores(qs, np.arange(len(ents)))[name])
        B = B.reshape(len(ents) * R, N)
        cols = np.argsort(-B, axis=1, kind='stable')[:, :NUM_K]
        block = (cols.astype(np.int32), np.take_along_axis(B, cols, axis=1), off.reshape(-1), ents.astype(np.int32),
                 lprior.astype(np.float32), mult.astype(np.int32))
        given, rel, other, _, _, n = E.select_events_brute(block, None, NUM_K)
        n = int(n[0])
        given, rel, other = given[:n], rel[:n], other[:n]
        facts.append(np.stack((given, rel, other) if name == 'ob' else (other, rel, given), axis=1).astype(np.int64))
    facts = np.unique(np.concatenate(facts), axis=0)
    return np.concatenate((facts, np.full((len(facts), 1), t, dtype=np.int64)), axis=1)


def test_generated_facts_equal_the_brute_force_rule(dev):
    w = world(dev)
    net = w['net']
    got = net.generate_events_observed(w['obs'], 20, w['gnet'], picks=picks, block_floats=BLOCK_FLOATS)
    stats = net.last_generate
    assert got.dtype == np.int64 and got.shape[1] == 4 and 0 < len(got) <= 2 * NUM_K and np.all(got[:, 3] == 20)
    assert np.array_equal(np.unique(got, axis=0), got)                                   # unique, sorted by (s, r, o)
    for name in ('ob', 'sub'):
        assert stats[name]['entities'] == len(MULT) and stats[name]['blocks'] == 2 and 0 < stats[name]['winners'] <= NUM_K
    assert np.array_equal(got, brute_generate(w, w['obs'], 20))
    one = net.generate_events_observed(w['obs'], 20, w['gnet'], picks=picks)            # one sub-block: the same facts
    assert net.last_generate['ob']['blocks'] == 1 and np.array_equal(one, got)
    few = net.generate_events_observed(w['obs'], 25, w['gnet'], num_k=3, picks=picks, block_floats=BLOCK_FLOATS)
    assert 0 < len(few) <= 6 and np.all(few[:, 3] == 25)


def test_horizon_one_is_the_forecast_observe_loop(dev):
    w = world(dev)
    got = w['net'].evaluate_rollout(w['obs'], w['test'], 1, w['gnet'], all_triplets=w['known'], picks=picks)
    want = ({name: np.concatenate([w['loop'][t][0][name] for t in TIMES]) for name in SETTINGS},
            np.concatenate([w['loop'][t][1] for t in TIMES]))
    rows_equal(got, want, 'h = 1')
    assert w['net'].last_rollout == []


_ROLLOUTS = {}


def rollout(dev, h):
    w = world(dev)
    if h not in _ROLLOUTS:
        before_t = {n: v.clone() for n, v in w['obs'].device.t.items()}
        glob = w['obs'].device.glob.clone()
        res = w['net'].evaluate_rollout(w['obs'], w['test'], h, w['gnet'], all_triplets=w['known'], picks=picks,
                                        block_floats=BLOCK_FLOATS)
        torch.cuda.synchronize()
        for n, v in before_t.items():                                                    # the old store survives
            assert torch.equal(w['obs'].device.t[n], v), n
        assert torch.equal(w['obs'].device.glob, glob) and w['obs'].device.n_quads == w['n20']
        _ROLLOUTS[h] = (res, list(w['net'].last_rollout))
    return _ROLLOUTS[h]


@pytest.mark.parametrize('h', [2, 4])
def test_rollout_equals_forecasts_on_host_rebuilt_streams(dev, h):
    w = world(dev)
    net, gnet, allq, test = w['net'], w['gnet'], w['allq'], w['test']
    (ranks, loss), log = rollout(dev, h)
    assert len(loss) == len(test) and [e['t'] for e in log] == [t for k, t in enumerate(TIMES) if (k + 1) % h]
    n_gen = n_true = 0
    for b0 in range(0, len(TIMES), h):
        block = TIMES[b0:b0 + h]
        facts = allq[:before(allq, block[0])]                                            # the truth before the block
        for j, t in enumerate(block):
            sel = test[:, 3] == t
            q = test[sel]
            got = cut_rows((ranks, loss), sel)
            if j == 0:
                rows_equal(got, w['loop'][t], (h, t, 'first of its block'))
            else:
                rows_equal(got, net.evaluate_forecast(host, q, all_triplets=w['known']), (h, t, 'host-rebuilt stream'))
            if j + 1 < len(block):
                if j == 0:
                    host = stream_of(facts)
                    host.resident(net, gnet)
                gen = net.generate_events_observed(host, t, gnet, picks=picks, block_floats=BLOCK_FLOATS)
                entry = log[n_gen]
                true = {tuple(x) for x in q[:, :3].tolist()}
                assert entry == {'t': t, 'generated': len(gen), 'true': sum(tuple(x) in true for x in gen[:, :3].tolist())}
                n_gen, n_true = n_gen + 1, n_true + entry['true']
                facts = np.concatenate((facts, gen))
                host = stream_of(facts)
                host.resident(net, gnet)
    assert n_gen == len(log)


def test_the_seed_gives_a_rollout_worth_testing(dev):
    """Guards against a hollow test: some generated fact is true, some is not, and the generated facts change a rank."""
    w = world(dev)
    import preprocess as P
    full = P.ObservedStream(S.make(), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    full.resident(w['net'], w['gnet'])
    idx = full.positions('test')
    assert np.array_equal(full.allq[idx], w['test'])
    differs = False
    for h in (2, 4):
        (ranks, loss), log = rollout(dev, h)
        assert sum(e['true'] for e in log) > 0, 'no generated fact is a true fact'
        assert sum(e['generated'] - e['true'] for e in log) > 0, 'every generated fact is a true fact'
        as_of = full.horizon_as_of(idx, h)
        stale = w['net'].evaluate_forecast(full, w['test'], as_of=as_of, all_triplets=w['known'])
        later = as_of < w['test'][:, 3]                                                  # rows of the non-first timestamps
        assert later.any()
        differs = differs or any(np.any(ranks[name][later] != stale[0][name][later]) for name in SETTINGS)
    assert differs, 'the rollout ranks of the non-first timestamps equal the stale-history ranks'


def test_argument_checks(dev):
    w = world(dev)
    net, gnet, obs, test = w['net'], w['gnet'], w['obs'], w['test']
    for t in (19, 5):
        with pytest.raises(ValueError):
            net.generate_events_observed(obs, t, gnet, picks=picks)
    with pytest.raises(ValueError):
        net.generate_events_observed(obs, 20, gnet, num_k=1025, picks=picks)
    with pytest.raises(ValueError):
        net.generate_events_observed(obs, 20, gnet, num_k=0, picks=picks)
    for h in (0, -1):
        with pytest.raises(ValueError):
            net.evaluate_rollout(obs, test, h, gnet, picks=picks)
    with pytest.raises(ValueError):
        net.evaluate_rollout(obs, w['allq'][w['n20'] - 5:], 2, gnet, picks=picks)       # the stream reaches into quads
    with pytest.raises(ValueError):
        net.evaluate_rollout(obs, test[::-1], 2, gnet, picks=picks)                      # not sorted by time
