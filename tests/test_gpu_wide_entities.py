"""GPU tests of the public prediction paths on a model with more entities than one CU's LDS holds as a row (run with -m gpu
on an MI355X): N_ent = 40 000, a tiny time-sorted stream whose entities lie on both sides of column 32768, set up through
preprocess.ObservedStream and resident() as tests/test_gpu_observed_eval.py does.  predict_topk_observed against the numpy
reference of tests/test_gpu_topk_rows.py on the rows of observed_scores, predict_events_observed against a host sort of the
observed_event_scores blocks, and the lists against the ranks of evaluate_observed.  (Before renet_topk_rows_wide the first
two raised RenetHipError: renet_topk_rows refuses C > 32768.)"""
import numpy as np
import pytest
import torch

from helpers import fixtures, global_shapes, renet_shapes
from test_gpu_observed_eval import _filter_sets
from test_gpu_topk_rows import _assert_logp, _lse64, _reference

pytestmark = pytest.mark.gpu

NUM_ENT, NUM_RELS, D, SEQ_LEN = 40000, 4, 100, 3
NUM_T, PER_T, K = 6, 40, 10
SETTINGS = ('raw', 'filtered', 'time_filtered')
DIRECTIONS = (('sub', 0, 2, 0), ('ob', 1, 0, 2))          # name, result column, given column, ranked column of a quadruple


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _stream():
    """6 timestamps of 40 distinct quadruples over 24 entities below column 32768 and 24 at or above it (the seam's two
    neighbours and the last column among them), few enough that histories and filter lists fill."""
    rng = np.random.RandomState(3)
    pool = np.concatenate((np.sort(rng.choice(32768, 22, replace=False)), [0, 32767, 32768, 32769, NUM_ENT - 1],
                           np.sort(32770 + rng.choice(NUM_ENT - 32771, 21, replace=False))))
    parts = []
    for t in range(NUM_T):
        q = np.stack((rng.choice(pool, 3 * PER_T), rng.randint(0, NUM_RELS, 3 * PER_T), rng.choice(pool, 3 * PER_T)), axis=1)
        _, first = np.unique(q, axis=0, return_index=True)
        q = q[np.sort(first)[:PER_T]]
        assert len(q) == PER_T
        parts.append(np.c_[q, np.full(PER_T, t)])
    return np.concatenate(parts).astype(np.int64), pool


@pytest.fixture(scope='module')
def world(dev):
    """Model (seeded weights), resident stream, the last two timestamps' positions, their observed_scores rows on the host and
    the brute-force filter sets: computed once, shared and left unchanged."""
    import global_model as GM
    import model as M
    import preprocess as P
    allq, pool = _stream()
    cut = (NUM_T - 2) * PER_T
    obs = P.ObservedStream((allq[:cut], allq[cut:]), NUM_ENT, NUM_RELS, SEQ_LEN)
    net = M.RENet(NUM_ENT, D, NUM_RELS, dropout=0.0, seq_len=SEQ_LEN, num_k=10)
    gnet = GM.RENet_global(NUM_ENT, D, NUM_RELS, dropout=0.0, seq_len=SEQ_LEN, num_k=10, maxpool=1)
    params = fixtures.make_params(41, renet_shapes(NUM_ENT, NUM_RELS, D))
    params['linear.bias'][pool] += 3.0                       # the stream's entities lead every row: gold ranks reach the lists
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    gnet.load_state_dict({k: torch.from_numpy(v) for k, v in
                          fixtures.make_params(42, global_shapes(NUM_ENT, NUM_RELS, D)).items()})
    net, gnet = net.to(dev).eval(), gnet.to(dev).eval()
    obs.resident(net, gnet)
    idx = obs.positions('test')
    quads = allq[idx]
    ids = np.concatenate((allq[:, 0], allq[:, 2]))
    assert np.mean(ids >= 32768) >= 1 / 3 and np.mean(quads[:, 2] >= 32768) >= 1 / 3 and np.mean(quads[:, 0] >= 32768) >= 1 / 3
    assert len(idx) == 2 * PER_T and obs.hist_s.count[idx].max() > 0 and obs.hist_o.count[idx].max() > 0
    sub_pred, ob_pred = (x.cpu().numpy() for x in net.observed_scores(obs, idx))
    assert ob_pred.shape == (len(idx), NUM_ENT)
    return dict(net=net, obs=obs, idx=idx, quads=quads, allq=allq, pred={'sub': sub_pred, 'ob': ob_pred},
                sets=_filter_sets(allq, quads))


def _lists(world, name, setting):
    if setting == 'raw':
        return None
    return [np.asarray(sorted(a if setting == 'filtered' else b), dtype=np.int64) for a, b in world['sets'][name]]


@pytest.mark.parametrize('keep_gold', [False, True])
@pytest.mark.parametrize('setting', SETTINGS)
def test_predict_topk_observed_equals_the_reference_on_the_observed_scores(world, setting, keep_gold):
    got = world['net'].predict_topk_observed(world['obs'], world['idx'], k=K, setting=setting, keep_gold=keep_gold)
    assert sorted(got) == ['ob', 'sub']
    for name, _, _, ranked in DIRECTIONS:
        pred, gold = world['pred'][name], world['quads'][:, ranked]
        lists = _lists(world, name, setting)
        want = _reference(pred, K, lists, gold if keep_gold else None)
        idx, val, logp, nv = (x.cpu().numpy() for x in got[name])
        assert idx.dtype == np.int32 and nv.dtype == np.int32 and idx.shape == val.shape == logp.shape == (len(gold), K)
        print(setting, 'keep_gold', keep_gold, name, 'rows differing in idx / val / n_valid',
              int((idx != want[0]).any(axis=1).sum()), int((val != want[1]).any(axis=1).sum()), int((nv != want[2]).sum()),
              '; entries at or above column 32768:', int((idx >= 32768).sum()), 'of', idx.size)
        assert np.array_equal(idx, want[0]) and np.array_equal(val, want[1]) and np.array_equal(nv, want[2])
        _assert_logp(logp, val, nv, _lse64(pred))
        assert (idx >= 32768).any() and ((idx >= 0) & (idx < 32768)).any()
        if lists is not None:
            assert sum(len(x) for x in lists) > len(lists)           # the lists do remove something
            hit = (idx == gold[:, None]).any(axis=1)
            assert keep_gold or not hit.any()                        # the gold entity is a known fact of its own timestamp


@pytest.mark.parametrize('setting', SETTINGS)
def test_predict_events_observed_equals_a_host_sort_of_the_blocks(world, setting):
    """The k = 5 best (relation, entity) pairs: J = B + off of observed_event_scores in fp32, the known pairs of the given
    entity taken out, by J descending, then relation, then entity ascending."""
    net, obs, idx, quads, allq = (world[x] for x in ('net', 'obs', 'idx', 'quads', 'allq'))
    k, n, R, N = 5, len(world['idx']), NUM_RELS, NUM_ENT
    if 'blocks' not in world:                                    # once for the three settings
        world['blocks'] = {name: tuple(x.cpu().numpy() for x in b) for name, b in net.observed_event_scores(obs, idx).items()}
    got = net.predict_events_observed(obs, idx, k=k, setting=setting)
    assert sorted(got) == ['ob', 'sub']
    rel_of, ent_of = np.divmod(np.arange(R * N), N)
    for name, _, given, ranked in DIRECTIONS:
        B, off = world['blocks'][name]
        J = (B + off[:, :, None]).reshape(n, R * N)
        assert J.dtype == np.float32
        gr, ge, gl, gn = (x.cpu().numpy() for x in got[name])
        assert gr.shape == ge.shape == gl.shape == (n, k) and gr.dtype == ge.dtype == gn.dtype == np.int32
        removed = 0
        for i, q in enumerate(quads.tolist()):
            keep = np.ones(R * N, dtype=bool)
            if setting != 'raw':
                m = allq[:, given] == q[given]
                if setting == 'time_filtered':
                    m &= allq[:, 3] == q[3]
                keep[allq[m, 1] * N + allq[m, ranked]] = False
                removed += int((~keep).sum())
            cand = np.nonzero(keep)[0]
            v = J[i, cand]
            sel = cand[v >= np.partition(v, len(v) - k)[len(v) - k]]          # everything from the k-th value up, then ordered
            order = sel[np.lexsort((ent_of[sel], rel_of[sel], -J[i, sel]))][:k]
            assert gn[i] == k and gr[i].tolist() == rel_of[order].tolist() and ge[i].tolist() == ent_of[order].tolist(), \
                (setting, name, i)
            assert np.array_equal(gl[i], J[i, order])                          # bit-equal to B + off in fp32
        assert (removed > 0) == (setting != 'raw')
        assert (ge >= 32768).any() and (ge < 32768).any()


def test_lists_are_consistent_with_the_ranks_of_evaluate_observed(dev, world):
    """With keep_gold, per setting: a gold entity whose rank is r <= k stands at place r of the list, one with a higher rank
    stands nowhere.  The ranks average ties, and the filtered settings compare sigmoid(score), which collapses distinct
    scores: where the gold value is tied among the candidates the place may lie anywhere inside the tie."""
    net, obs, idx, quads = (world[x] for x in ('net', 'obs', 'idx', 'quads'))
    ranks, _ = net.evaluate_observed(obs, idx)
    for s, setting in enumerate(SETTINGS):
        got = net.predict_topk_observed(obs, idx, k=K, setting=setting, keep_gold=True)
        for name, col, _, ranked in DIRECTIONS:
            pred, gold = world['pred'][name], quads[:, ranked]
            lists = _lists(world, name, setting)
            top = got[name][0].cpu().numpy()
            vals = pred if setting == 'raw' else torch.sigmoid(torch.from_numpy(pred).to(dev)).cpu().numpy()   # (the device's rounding)
            exact = 0
            for i in range(len(gold)):
                cand = np.ones(NUM_ENT, dtype=bool)
                if lists is not None:
                    cand[lists[i]] = False
                    cand[gold[i]] = True
                greater = int((vals[i, cand] > vals[i, gold[i]]).sum())
                equal = int((vals[i, cand] == vals[i, gold[i]]).sum())
                assert ranks[setting][i, col] == greater + (equal - 1) / 2 + 1, (setting, name, i)
                at = np.nonzero(top[i] == gold[i])[0]
                if greater + equal - 1 < K:
                    assert len(at) == 1 and greater <= at[0] <= greater + equal - 1, (setting, name, i)
                if greater >= K:
                    assert len(at) == 0, (setting, name, i)
                exact += equal == 1
            listed = int((top == gold[:, None]).any(axis=1).sum())
            print(setting, name, 'gold listed in', listed, 'of', len(gold), 'rows; untied gold value in', exact)
            assert exact >= 0.9 * len(gold)                          # otherwise the places prove little
            assert listed > 0
