"""GPU tests of the event forecasts under observed history (run with -m gpu on an MI355X): RENet.observed_event_scores /
evaluate_events_observed / predict_events_observed on the small stream of tests/observed_stream.py, in the world of
test_gpu_observed_eval.py (same model, resident stream and oracle scores, computed once).  What pins the MEANING are tests
1 and 3: the blocks against the oracle's restatement of the reference forward called once per relation, and the pair and
relation ranks of all three settings against the intervals those oracle values allow.  The rest is consistency: the existing
observed pass, a numpy restatement on the returned blocks (exact), sub-blocking, top-k, the all-empty first timestamp, the
untouched multi-step state."""
import numpy as np
import pytest
import torch

from helpers import O
from test_gpu_parity import ATOL, RTOL            # the tolerance of logits against the reference golden, same GEMM mode
from test_gpu_observed_eval import STATE, SETTINGS, _multi_step_setup, _same_content, _world

import observed_stream as S

pytestmark = pytest.mark.gpu

R, N = S.NUM_RELS, S.NUM_ENT
DIRECTIONS = (('sub', 0, 2, 0), ('ob', 1, 0, 2))          # name, result column, given column, ranked column of a quadruple


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _lse64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def _offsets64(B, Lr):
    """fp64: logsoftmax(Lr[i])[r] - logsumexp(B[i, r, :]) for B [n, R, N], Lr [n, R]."""
    Lr = np.asarray(Lr, dtype=np.float64)
    return (Lr - _lse64(Lr)[:, None]) - _lse64(B)


def _known_masks(allq, quads):
    """Per direction, by brute force over the fact array: (any [n, R, N], at [n, R, N]) bool -- the pairs (r', e') that
    complete the given entity of the quadruple to a known fact at any time / at the quadruple's own."""
    out = {}
    for name, col, given, ranked in DIRECTIONS:
        anyt, at = np.zeros((len(quads), R, N), dtype=bool), np.zeros((len(quads), R, N), dtype=bool)
        for i, q in enumerate(quads.tolist()):
            m = allq[:, given] == q[given]
            anyt[i, allq[m, 1], allq[m, ranked]] = True
            m &= allq[:, 3] == q[3]
            at[i, allq[m, 1], allq[m, ranked]] = True
        out[name] = (anyt, at)
    return out


def _candidates(masks, name, setting, i, gr, gc):
    """bool [R, N]: the pairs that are candidates of position i (the gold pair always among them)."""
    keep = np.ones((R, N), dtype=bool)
    if setting != 'raw':
        keep = ~masks[name][0 if setting == 'filtered' else 1][i]
        keep[gr, gc] = True
    return keep


def _restated_ranks(B, off, quads, masks):
    """The definitions on fp32 J = B + off (one addition): ({'pair': ..., 'relation': ...} of {setting: [n, 2]}, logp [n, 2])."""
    n = len(quads)
    out = {kind: {name: np.zeros((n, 2)) for name in SETTINGS} for kind in ('pair', 'relation')}
    logp = np.zeros((n, 2), dtype=np.float32)
    for name, col, given, ranked in DIRECTIONS:
        J = B[name] + off[name][:, :, None]
        assert J.dtype == np.float32
        for i in range(n):
            gr, gc = int(quads[i, 1]), int(quads[i, ranked])
            v = logp[i, col] = J[i, gr, gc]
            for setting in SETTINGS:
                keep = _candidates(masks, name, setting, i, gr, gc)
                out['pair'][setting][i, col] = np.count_nonzero(J[i][keep] > v) + (np.count_nonzero(J[i][keep] == v) - 1) / 2 + 1
                line = J[i, keep[:, gc], gc]
                out['relation'][setting][i, col] = np.count_nonzero(line > v) + (np.count_nonzero(line == v) - 1) / 2 + 1
    return out, logp


def _oracle_intervals(ref_B, ref_Lr, quads, masks):
    """{kind: {setting: (lo [n, 2], hi [n, 2])}} from the ORACLE's values alone, by the rule of test_gpu_observed_eval: with
    tol = 2 (ATOL + RTOL max|B_i|) + 2 (ATOL + RTOL max|Lr_i|) the tolerance of a joint log-probability, lo counts only the
    candidates above gold + tol, hi all candidates at or above gold - tol."""
    n = len(quads)
    out = {kind: {name: (np.zeros((n, 2)), np.zeros((n, 2))) for name in SETTINGS} for kind in ('pair', 'relation')}
    tols = np.zeros((n, 2))
    for name, col, given, ranked in DIRECTIONS:
        J = ref_B[name] + _offsets64(ref_B[name], ref_Lr[name])[:, :, None]
        for i in range(n):
            gr, gc = int(quads[i, 1]), int(quads[i, ranked])
            tol = tols[i, col] = 2 * (ATOL + RTOL * float(np.abs(ref_B[name][i]).max())) + \
                2 * (ATOL + RTOL * float(np.abs(ref_Lr[name][i]).max()))
            v = J[i, gr, gc]
            for setting in SETTINGS:
                keep = _candidates(masks, name, setting, i, gr, gc)
                keep[gr, gc] = False                                  # the others
                for kind, vals in (('pair', J[i][keep]), ('relation', J[i, keep[:, gc], gc])):
                    out[kind][setting][0][i, col] = 1 + np.count_nonzero(vals > v + tol)
                    out[kind][setting][1][i, col] = 1 + np.count_nonzero(vals >= v - tol)
    return out, tols


_EVENTS = {}


def _events(dev, d):
    """The world of test_gpu_observed_eval plus the ORACLE's blocks: renet_forward_loss once per relation r' with the relation
    column overwritten by r', un-permuted with bg.perm (computed once per hidden size, shared and left unchanged)."""
    if d in _EVENTS:
        return _EVENTS[d]
    w = _world(dev, d)
    obs, store, idx, quads = w['obs'], w['store'], w['idx'], w['quads']
    allq = obs.allq
    op = {k: torch.from_numpy(v) for k, v in w['params'].items()}
    ge = {int(t): store.glob[k].cpu() for k, t in enumerate(obs.times)}
    ogd = O.build_graph_dict(allq, R)
    sh, oh, _ = O.build_histories(allq, S.NUM_ENT, history_len=S.SEQ_LEN)
    ref_B = {}
    with torch.no_grad():
        for name, subject, h in (('ob', True, sh), ('sub', False, oh)):
            full = np.empty((len(idx), R, N), dtype=np.float64)
            for rr in range(R):
                q = quads.copy()
                q[:, 1] = rr
                _, parts = O.renet_forward_loss(op, q, [h[0][i] for i in idx], [h[1][i] for i in idx], ogd, ge, R, S.SEQ_LEN,
                                                subject=subject, return_parts=True)
                full[parts['bg'].perm, rr] = parts['ob_pred'].double().numpy()
            ref_B[name] = full
    e = dict(w=w, ref_B=ref_B, ref_Lr=w['ref_r'], masks=_known_masks(allq, quads))
    # the oracle's own row of the quadruple's relation is the row the existing pass is checked against
    for name in ('ob', 'sub'):
        np.testing.assert_allclose(ref_B[name][np.arange(len(idx)), quads[:, 1]], w['ref'][name], rtol=1e-5, atol=1e-6)
    if d == 100:
        e['intervals'], e['tols'] = _oracle_intervals(ref_B, w['ref_r'], quads, e['masks'])
    _EVENTS[d] = e
    return e


_CALLS = {}


def _default_pass(dev):
    """evaluate_events_observed and observed_event_scores of the d = 100 world with the default block size, run once."""
    if not _CALLS:
        e = _events(dev, 100)
        w = e['w']
        _CALLS['ranks'] = w['net'].evaluate_events_observed(w['obs'], w['idx'])
        got = w['net'].observed_event_scores(w['obs'], w['idx'])
        _CALLS['B'] = {name: got[name][0].cpu().numpy() for name in got}
        _CALLS['off'] = {name: got[name][1].cpu().numpy() for name in got}
    return _CALLS


def _inside(kind, got, intervals, what):
    for name in SETTINGS:
        lo, hi = intervals[kind][name]
        bad = (got[name] < lo) | (got[name] > hi)
        print(what, kind, name, 'ranks outside the oracle intervals', int(bad.sum()), 'of', bad.size)
        assert not bad.any(), (what, kind, name, np.argwhere(bad)[:5])


# ---- 1. meaning: the blocks against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize('d', [100, 300])
def test_blocks_equal_the_oracle_forward_called_once_per_relation(dev, d):
    e = _events(dev, d)
    w = e['w']
    got = w['net'].observed_event_scores(w['obs'], w['idx'])
    assert sorted(got) == ['ob', 'sub']
    for name in ('ob', 'sub'):
        B, off = (x.cpu().numpy() for x in got[name])
        assert B.shape == (len(w['idx']), R, N) and off.shape == (len(w['idx']), R) and B.dtype == off.dtype == np.float32
        print('d', d, name, 'max |B - oracle|', float(np.abs(B - e['ref_B'][name]).max()), 'scale', float(np.abs(e['ref_B'][name]).max()))
        np.testing.assert_allclose(B, e['ref_B'][name], rtol=RTOL, atol=ATOL)
        want = _offsets64(e['ref_B'][name], e['ref_Lr'][name])
        print('d', d, name, 'max |off - oracle formula|', float(np.abs(off - want).max()), 'scale', float(np.abs(want).max()))
        np.testing.assert_allclose(off, want, rtol=2 * RTOL, atol=2 * ATOL)
    with pytest.raises(ValueError):
        w['net'].observed_event_scores(w['obs'], w['idx'], block_floats=len(w['idx']) * R * N - 1)


# ---- 2. consistency with the existing pass -----------------------------------------------------------------------------
def test_the_quadruples_own_rows_are_the_observed_scores(dev):
    """B[i, r_i, :] against observed_scores: the two differ only in how the GRU input projection is associated."""
    e = _events(dev, 100)
    w, calls = e['w'], _default_pass(dev)
    sub_pred, ob_pred = w['net'].observed_scores(w['obs'], w['idx'])
    rows = np.arange(len(w['idx']))
    for name, pred in (('ob', ob_pred), ('sub', sub_pred)):
        mine, theirs = calls['B'][name][rows, w['quads'][:, 1]], pred.cpu().numpy()
        print(name, 'max |B[i, r_i] - observed_scores|', float(np.abs(mine - theirs).max()))
        np.testing.assert_allclose(mine, theirs, rtol=RTOL, atol=ATOL)


# ---- 3. ranks against the oracle ---------------------------------------------------------------------------------------
def test_ranks_lie_in_the_intervals_the_oracle_allows(dev):
    e = _events(dev, 100)
    w, got = e['w'], _default_pass(dev)['ranks']
    n = len(w['idx'])
    assert sorted(got) == ['logp', 'pair', 'relation'] and got['logp'].shape == (n, 2) and got['logp'].dtype == np.float32
    for kind, need in (('pair', 0.7), ('relation', 0.95)):
        assert sorted(got[kind]) == sorted(SETTINGS)
        for name in SETTINGS:
            lo, hi = e['intervals'][kind][name]
            assert got[kind][name].shape == (n, 2) and got[kind][name].dtype == np.float64
            sharp = float(np.mean(lo == hi))
            print(kind, name, 'rows with lo == hi under the oracle alone', sharp)
            assert sharp >= need                                   # otherwise the intervals prove nothing
        _inside(kind, got[kind], e['intervals'], 'default blocks')
        assert np.all(got[kind]['filtered'] <= got[kind]['time_filtered'])
        assert np.all(got[kind]['time_filtered'] <= got[kind]['raw'])
    assert got['pair']['raw'].min() >= 1 and got['pair']['raw'].max() <= R * N
    assert got['relation']['raw'].min() >= 1 and got['relation']['raw'].max() <= R
    # the planted case (c): three objects of (0, 1) at t = 20 -- whichever of them the model likes least has the other two
    # above it, and only the time-aware filter (and the time-agnostic one) takes them out
    q = w['quads']
    planted = np.nonzero((q[:, 0] == 0) & (q[:, 1] == 1) & (q[:, 3] == 20))[0]
    assert len(planted) == 3 and all(len(w['sets']['ob'][i][1]) >= 3 for i in planted)
    print('planted (c): raw', got['pair']['raw'][planted, 1], 'time_filtered', got['pair']['time_filtered'][planted, 1])
    assert np.any(got['pair']['raw'][planted, 1] > got['pair']['time_filtered'][planted, 1])


# ---- 4. exact self-consistency -----------------------------------------------------------------------------------------
def test_ranks_equal_the_numpy_restatement_on_the_returned_blocks(dev):
    e = _events(dev, 100)
    w, calls = e['w'], _default_pass(dev)
    want, logp = _restated_ranks(calls['B'], calls['off'], w['quads'], e['masks'])
    got = calls['ranks']
    for kind in ('pair', 'relation'):
        for name in SETTINGS:
            print(kind, name, 'rows differing from the restatement', int((got[kind][name] != want[kind][name]).sum()))
            assert np.array_equal(got[kind][name], want[kind][name]), (kind, name)
    assert np.array_equal(got['logp'], logp)
    # all_triplets given explicitly (the stream itself, as a tensor) is the default
    again = w['net'].evaluate_events_observed(w['obs'], w['idx'], all_triplets=torch.from_numpy(w['obs'].allq))
    assert all(np.array_equal(again[kind][name], got[kind][name]) for kind in ('pair', 'relation') for name in SETTINGS)
    assert np.array_equal(again['logp'], got['logp'])


# ---- 5. sub-blocking ---------------------------------------------------------------------------------------------------
def test_two_groups_per_sub_block_agree_with_the_default(dev):
    e = _events(dev, 100)
    w, one = e['w'], _default_pass(dev)['ranks']
    cut = w['net'].evaluate_events_observed(w['obs'], w['idx'], block_floats=2 * R * N)
    print('largest |logp difference| between the block sizes', float(np.abs(cut['logp'] - one['logp']).max()),
          'smallest tolerance', float(e['tols'].min()))
    assert np.all(np.abs(cut['logp'].astype(np.float64) - one['logp']) <= e['tols'])
    for kind in ('pair', 'relation'):
        print(kind, 'ranks differing between the block sizes', {name: int((cut[kind][name] != one[kind][name]).sum()) for name in SETTINGS})
        _inside(kind, cut[kind], e['intervals'], 'two groups per sub-block')
        _inside(kind, one[kind], e['intervals'], 'default blocks')


# ---- 6. top-k ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 10, R * N + 5])
def test_topk_equals_a_numpy_lexsort_of_the_candidates(dev, k):
    e = _events(dev, 100)
    w, calls = e['w'], _default_pass(dev)
    net, obs, idx, quads = w['net'], w['obs'], w['idx'], w['quads']
    n = len(idx)
    rel_of, ent_of = np.divmod(np.arange(R * N), N)
    for setting in SETTINGS:
        got = net.predict_events_observed(obs, idx, k=k, setting=setting)
        assert sorted(got) == ['ob', 'sub']
        for name, col, given, ranked in DIRECTIONS:
            gr, ge, gl, gn = (x.cpu().numpy() for x in got[name])
            assert gr.shape == ge.shape == gl.shape == (n, k) and gn.shape == (n,)
            assert gr.dtype == ge.dtype == gn.dtype == np.int32 and gl.dtype == np.float32
            J = (calls['B'][name] + calls['off'][name][:, :, None]).reshape(n, R * N)
            for i in range(n):
                keep = np.ones(R * N, dtype=bool)
                if setting != 'raw':
                    keep = ~e['masks'][name][0 if setting == 'filtered' else 1][i].reshape(-1)
                cand = np.nonzero(keep)[0]
                order = cand[np.lexsort((ent_of[cand], rel_of[cand], -J[i, cand]))][:k]
                m = len(order)
                assert gn[i] == m, (setting, name, i)
                assert gr[i, :m].tolist() == rel_of[order].tolist() and ge[i, :m].tolist() == ent_of[order].tolist(), (setting, name, i)
                assert np.all(gr[i, m:] == -1) and np.all(ge[i, m:] == -1) and np.all(np.isneginf(gl[i, m:]))
                assert np.array_equal(gl[i, :m], J[i, order])                       # bit-equal to B + off in fp32
            if setting == 'raw' and k >= R * N:
                # the place of the gold pair in the full list is its raw pair rank where it has no ties
                gold = quads[:, 1] * N + quads[:, ranked]
                place = np.asarray([int(np.nonzero(gr[i].astype(np.int64) * N + ge[i] == gold[i])[0][0]) + 1 for i in range(n)])
                alone = (J == J[np.arange(n), gold][:, None]).sum(axis=1) == 1
                assert alone.any() and np.array_equal(place[alone], calls['ranks']['pair']['raw'][alone, col])
    with pytest.raises(ValueError):
        net.predict_events_observed(obs, idx, k=k, setting='best')


# ---- 7. the first timestamp alone --------------------------------------------------------------------------------------
def test_first_timestamp_takes_the_zero_state_blocks(dev):
    w = _events(dev, 100)['w']
    net, obs = w['net'], w['obs']
    idx = np.nonzero(obs.allq[:, 3] == obs.times[0])[0]
    assert len(idx) >= 15 and obs.hist_s.count[idx].max() == 0 and obs.hist_o.count[idx].max() == 0
    got = net.observed_event_scores(obs, idx)
    q = torch.from_numpy(obs.allq[idx]).to(dev)
    with torch.no_grad():
        ent, rel = net.ent_embeds.double(), net.rel_embeds.double()
        zero = torch.zeros(len(idx), R, 100, device=dev).double()
        lin = lambda f: f @ net.linear.weight.double().t() + net.linear.bias.double()
        fold = lambda x: x.view(len(idx), 1, 100).expand(len(idx), R, 100)
        want = {'ob': lin(torch.cat((fold(ent[q[:, 0]]), zero, rel[:R].view(1, R, 100).expand(len(idx), R, 100)), dim=2)),
                'sub': lin(torch.cat((fold(ent[q[:, 2]]), zero, rel[R:].view(1, R, 100).expand(len(idx), R, 100)), dim=2))}
    for name in ('ob', 'sub'):
        np.testing.assert_allclose(got[name][0].cpu().numpy(), want[name].cpu().numpy(), rtol=RTOL, atol=ATOL)
        assert np.all(np.isfinite(got[name][1].cpu().numpy()))
    ranks = net.evaluate_events_observed(obs, idx)
    B = {name: got[name][0].cpu().numpy() for name in got}
    off = {name: got[name][1].cpu().numpy() for name in got}
    want_ranks, logp = _restated_ranks(B, off, obs.allq[idx], _known_masks(obs.allq, obs.allq[idx]))
    assert all(np.array_equal(ranks[kind][name], want_ranks[kind][name]) for kind in ('pair', 'relation') for name in SETTINGS)
    assert np.array_equal(ranks['logp'], logp)


# ---- 8. state untouched ------------------------------------------------------------------------------------------------
def test_the_three_calls_leave_the_multi_step_state_untouched_and_are_repeatable(dev):
    import copy
    w = _events(dev, 100)['w']
    obs = w['obs']
    net, gnet, H, valid = _multi_step_setup(dev, obs)
    held = {k: getattr(net, k) for k in STATE}
    graphs = dict(net.graph_dict)
    snap = copy.deepcopy({k: (dict(v) if k.startswith('preds_') else v) for k, v in held.items() if k != 'graph_dict'})
    latest, last_batch = copy.deepcopy(net.latest_time), net.aggregator.last_batch
    glob_key = net.aggregator.glob_table._key
    store = obs.resident(net, gnet)                             # a store of its own for this model
    idx = obs.positions('valid')
    try:
        first = net.evaluate_events_observed(store, idx, block_floats=5 * R * N)
        second = net.evaluate_events_observed(store, idx, block_floats=5 * R * N)
        for kind in ('pair', 'relation'):
            for name in SETTINGS:
                assert np.array_equal(first[kind][name], second[kind][name])
        assert np.array_equal(first['logp'], second['logp'])
        top = [net.predict_events_observed(store, idx[:9], k=3, setting='time_filtered') for _ in range(2)]
        blocks = [net.observed_event_scores(store, idx[:9]) for _ in range(2)]
        for name in ('ob', 'sub'):
            assert all(torch.equal(a, b) for a, b in zip(top[0][name], top[1][name]))
            assert all(torch.equal(a, b) for a, b in zip(blocks[0][name], blocks[1][name]))
    finally:
        obs.device = w['store']                                 # (the shared world's store stays the stream's)
    for k in STATE:
        assert getattr(net, k) is held[k], k
        if k != 'graph_dict':
            now = getattr(net, k)
            assert _same_content(dict(now) if k.startswith('preds_') else now, snap[k]), k
    assert list(net.graph_dict.keys()) == list(graphs.keys()) and all(net.graph_dict[t] is graphs[t] for t in graphs)
    assert _same_content(net.latest_time, latest) and net.aggregator.last_batch is last_batch
    assert net.aggregator.glob_table._key == glob_key
