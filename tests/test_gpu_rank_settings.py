"""GPU tests of the three-setting evaluation (run with -m gpu on an MI355X): renet_rank_rows3 (csrc/rank.hip: raw, filtered and
time-aware filtered counts from one read of a score row) against the kernel it stands beside (renet_rank_rows, one setting
per launch) and against the torch formulation (model._rank_rows) -- exact --, its loss against renet_softmax_ce, and the public
paths (RENet.evaluate_all_stream / evaluate_all_batch / evaluate_time_filter) on the evaluation fixture."""
import numpy as np
import pytest
import torch

from helpers import load_golden
from test_gpu_rank import LOGITS, SHAPES, _facts_for, _scores

pytestmark = pytest.mark.gpu

QUERY_TIMES = (0, 48, 72)        # _facts_for: every fact at t = 0 and 24, a third at 48 -> equal, strict subset, empty
SETTINGS = ('raw', 'filtered', 'time_filtered')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _brute_lists(at, n, qt):
    """Per row i (key s = i, r = 0): (sorted unique objects at any time, those at time qt[i]) -- by sorting the facts by
    subject and cutting, not through filter_index."""
    order = np.argsort(at[:, 0], kind='stable')
    srt = at[order]
    lo, hi = np.searchsorted(srt[:, 0], np.arange(n), 'left'), np.searchsorted(srt[:, 0], np.arange(n), 'right')
    agnostic, aware = [], []
    for i in range(n):
        chunk = srt[lo[i]:hi[i]]
        assert np.all(chunk[:, 1] == 0)
        agnostic.append(np.unique(chunk[:, 2]))
        aware.append(np.unique(chunk[chunk[:, 3] == qt[i], 2]))
    return agnostic, aware


def _table(lists, C, seed):
    """The lists laid out in one column table in a shuffled row order, with distractors (valid columns, -1, C + 5) before,
    between and after them -> (cols, start [n], count [n]) as int32 numpy arrays."""
    rng = np.random.RandomState(seed)
    junk = lambda: np.concatenate((rng.randint(0, C, 3), [-1, C + 5]))
    parts, start, pos = [junk()], np.zeros(len(lists), dtype=np.int32), 5
    for i in rng.permutation(len(lists)):
        start[i] = pos
        parts += [lists[i], junk()]
        pos += len(lists[i]) + 5
    count = np.asarray([len(x) for x in lists], dtype=np.int32)
    return np.concatenate(parts).astype(np.int32), start, count


def _csr(lists, dev):
    ptr = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int32)
    col = np.concatenate(lists + [np.zeros(1, dtype=np.int64)]).astype(np.int32)        # (never an empty tensor)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(col).to(dev)


def _pairs(lists, dev):
    rows = np.repeat(np.arange(len(lists)), [len(x) for x in lists])
    cols = np.concatenate(lists + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)


def _ranks(cnt2):
    return (cnt2[0].double() + (cnt2[1].double() - 1.0) / 2 + 1).cpu().numpy()


@pytest.mark.parametrize('logits', LOGITS)
@pytest.mark.parametrize('n,C,ld', SHAPES)
def test_three_settings_equal_the_one_setting_kernel_and_the_torch_path(dev, n, C, ld, logits):
    import model as M
    import renet_hip as K
    scores, label = _scores(dev, n, C, ld, logits)
    lab32 = label.int()
    before = scores.clone()
    raw_cnt, _ = K.rank_rows(scores, lab32, filtered=False, want_loss=False)
    raw_ranks = M._rank_rows(scores, label)
    qt = np.asarray(QUERY_TIMES)[np.arange(n) % 3]
    plans = [np.arange(n) % 4] if n >= 8 else [np.full(n, k) for k in range(4)]
    seen = set()
    for p, plan in enumerate(plans):
        at = _facts_for(n, C, label.cpu().numpy(), plan, seed=n + C + p)
        agnostic, aware = _brute_lists(at, n, qt) if len(at) else ([np.zeros(0, dtype=np.int64)] * n,) * 2
        for a, b in zip(agnostic, aware):
            assert set(b.tolist()) <= set(a.tolist())
            seen.add('empty' if len(b) == 0 and len(a) else 'equal' if len(b) == len(a) else 'subset')
        ta = [torch.from_numpy(x).to(dev) for x in _table(agnostic, C, 1 + p)]
        tt = [torch.from_numpy(x).to(dev) for x in _table(aware, C, 101 + p)]
        cnt, loss = K.rank_rows3(scores, lab32, *ta, *tt, want_loss=False)
        assert loss is None and cnt.shape == (6, n) and cnt.dtype == torch.int32
        want_a, _ = K.rank_rows(scores, lab32, *_csr(agnostic, dev), filtered=True, want_loss=False)
        want_t, _ = K.rank_rows(scores, lab32, *_csr(aware, dev), filtered=True, want_loss=False)
        for name, got, want in (('raw', cnt[0:2], raw_cnt), ('filtered', cnt[2:4], want_a), ('time_filtered', cnt[4:6], want_t)):
            print(name, n, C, ld, logits, 'plan', p, 'greater', int((got[0] != want[0]).sum()), 'equal',
                  int((got[1] != want[1]).sum()), 'rows differ from rank_rows')
            assert torch.equal(got, want)
        assert np.array_equal(_ranks(cnt[0:2]), raw_ranks)
        assert np.array_equal(_ranks(cnt[2:4]), M._rank_rows(scores, label, *_pairs(agnostic, dev)))
        assert np.array_equal(_ranks(cnt[4:6]), M._rank_rows(scores, label, *_pairs(aware, dev)))
        assert np.all(_ranks(cnt[2:4]) <= _ranks(cnt[4:6]))
    if n >= 3:
        assert seen == {'empty', 'equal', 'subset'}
    assert torch.equal(scores, before)


def test_null_lists_and_scores_untouched(dev):
    import renet_hip as K
    n, C = 9, 1031
    scores, label = _scores(dev, n, C, C, 'blocks')
    lab32 = label.int()
    before = scores.clone()
    raw, _ = K.rank_rows(scores, lab32, filtered=False, want_loss=False)
    plain, _ = K.rank_rows(scores, lab32, filtered=True, want_loss=False)           # sigmoid counts, no lists
    at = _facts_for(n, C, label.cpu().numpy(), np.arange(n) % 4, seed=3)
    agnostic, _ = _brute_lists(at, n, np.zeros(n, dtype=np.int64))
    tab = [torch.from_numpy(x).to(dev) for x in _table(agnostic, C, 9)]
    listed, _ = K.rank_rows(scores, lab32, *_csr(agnostic, dev), filtered=True, want_loss=False)
    assert not torch.equal(listed, plain)                                           # the lists do change the counts
    none = (None, None, None)
    for la, lt, want_a, want_t in ((none, none, plain, plain), (tab, none, listed, plain), (none, tab, plain, listed)):
        cnt, _ = K.rank_rows3(scores, lab32, *la, *lt, want_loss=False)
        assert torch.equal(cnt[0:2], raw) and torch.equal(cnt[2:4], want_a) and torch.equal(cnt[4:6], want_t)
    # an empty column table is no list
    e = torch.zeros(0, device=dev, dtype=torch.int32)
    z = torch.zeros(n, device=dev, dtype=torch.int32)
    cnt, _ = K.rank_rows3(scores, lab32, e, z, z, *tab, want_loss=False)
    assert torch.equal(cnt[2:4], plain) and torch.equal(cnt[4:6], listed)
    assert torch.equal(scores, before)


@pytest.mark.parametrize('logits', LOGITS)
@pytest.mark.parametrize('n,C,ld', SHAPES)
def test_row_loss_is_as_accurate_as_softmax_ce(dev, n, C, ld, logits):
    """The statement of test_gpu_rank.test_row_loss_is_as_accurate_as_softmax_ce for renet_rank_rows3: its error against a
    float64 logsumexp is at most the error renet_softmax_ce has on THIS matrix against the same reference, measured here.
    (The sweep takes an element exactly as rank_rows_kernel does, so the loss is expected to be bit-equal to rank_rows';
    printed, not asserted.)"""
    import renet_hip as K
    scores, label = _scores(dev, n, C, ld, logits)
    rows = torch.arange(n, device=dev)
    ref = torch.logsumexp(scores.double(), dim=1) - scores.double()[rows, label]
    old = K.softmax_ce(scores, label.int(), 1.0, False)
    assert bool(torch.isfinite(old).all())
    bound = float((old.double() - ref).abs().max())
    _, new = K.rank_rows3(scores, label.int(), None, None, None, None, None, None, want_loss=True)
    _, one = K.rank_rows(scores, label.int(), filtered=False, want_loss=True)
    err = float((new.double() - ref).abs().max())
    print('loss', n, C, ld, logits, 'softmax_ce error', bound, 'rank_rows3 error', err, 'between the kernels',
          float((new - old).abs().max()), 'bit-equal to rank_rows', bool(torch.equal(new, one)))
    assert err <= bound
    assert float((new.double() - old.double()).abs().max()) <= 2 * bound


def test_argument_checks(dev):
    import renet_hip as K
    L = K.lib()
    s = torch.zeros(4, 8, device=dev)
    lab = torch.tensor([0, 7, -5, 99], device=dev, dtype=torch.int32)
    out = torch.full((6, 4), 7, device=dev, dtype=torch.int32)
    cols = torch.arange(16, device=dev, dtype=torch.int32) % 8
    rng = torch.zeros(4, device=dev, dtype=torch.int32)
    p = lambda t: None if t is None else t.data_ptr()

    def call(n=4, C=8, ld=8, a=(None, None, None, 0), t=(None, None, None, 0)):
        return L.renet_rank_rows3(p(s), ld, n, C, p(lab), p(a[0]), p(a[1]), p(a[2]), a[3], p(t[0]), p(t[1]), p(t[2]), t[3],
                                  p(out), None, K._stream())
    assert call(n=-1) == -1 and call(C=0) == -1 and call(ld=7) == -1
    for bad in ((None, rng, None, 0), (cols, rng, None, 16), (None, rng, rng, 0), (cols, None, rng, 16), (cols, None, None, 16),
                (cols, rng, rng, -1)):
        assert call(a=bad) == -1 and call(t=bad) == -1
    assert call(n=0) == 0                                                      # no-op: nothing launched, nothing written
    torch.cuda.synchronize()
    assert out.eq(7).all()
    # labels outside [0, C) are clamped into the row: the all-zero rows tie in every column whatever the label
    cnt, loss = K.rank_rows3(s, lab, None, None, None, None, None, None)
    assert cnt[[0, 2, 4]].eq(0).all() and cnt[[1, 3, 5]].eq(8).all()
    np.testing.assert_allclose(loss.cpu().numpy(), np.log(8.0), rtol=1e-6)
    # a range is cut to the length given for its table: with columns 0 at 5.0 (sigmoid > the gold's 0.5) and label 1, a listed
    # column 0 stops counting as greater.  cols = 0 1 2 ... : [2, 2 + 100) cut to len 4 lists columns 2 and 3 only; the
    # entries behind the given length (8 -> column 0 at index 8) are not read.
    s2 = s.clone()
    s2[:, 0] = 5.0
    lab2 = torch.ones(4, device=dev, dtype=torch.int32)
    start = torch.tensor([0, 2, 2, -3], device=dev, dtype=torch.int32)
    count = torch.tensor([1, 100, 0, 4], device=dev, dtype=torch.int32)
    assert L.renet_rank_rows3(p(s2), 8, 4, 8, p(lab2), p(cols), p(start), p(count), 4, None, None, None, 0, p(out), None,
                              K._stream()) == 0
    # greater: row 0 lists column 0 -> 0; row 1 lists 2, 3 -> 1; row 2 nothing -> 1; row 3: [-3, 1) cut to [0, 1) -> 0
    assert out[2].tolist() == [0, 1, 1, 0] and out[4].tolist() == [1, 1, 1, 1] and out[0].tolist() == [1, 1, 1, 1]
    # equal (gold sigmoid 0.5, a zeroed column is 0): 7 unless listed columns among 2..7 leave
    assert out[3].tolist() == [7, 5, 7, 7] and out[5].tolist() == [7, 7, 7, 7]
    with pytest.raises(K.RenetHipError):
        K.rank_rows3(s.double(), lab, None, None, None, None, None, None)
    with pytest.raises(K.RenetHipError):
        K.rank_rows3(s, lab, cols, rng, None, None, None, None)


# ---------------------------------------------------------------------------------------------
# the public paths on the evaluation fixture (set up as tests/test_gpu_parity.py sets up its stream test)
# ---------------------------------------------------------------------------------------------
def _recorded(net):
    """Keeps the quadruples and score matrices of every predict_batch call of `net`."""
    seen, inner = [], net.predict_batch

    def predict_batch(tr, *a, **k):
        out = inner(tr, *a, **k)
        seen.append((np.asarray(tr).copy(), out[1], out[2]))
        return out
    net.predict_batch = predict_batch
    return seen


def _loss64(seen, dev):
    """float64 losses of the recorded batches: lse(ob_pred) - ob_pred[o] + lse(sub_pred) - sub_pred[s] per row."""
    out = []
    for tr, sub_pred, ob_pred in seen:
        s, o = (torch.from_numpy(tr[:, k]).to(dev) for k in (0, 2))
        rows = torch.arange(len(tr), device=dev)
        out.append((torch.logsumexp(ob_pred.double(), 1) - ob_pred.double()[rows, o] +
                    torch.logsumexp(sub_pred.double(), 1) - sub_pred.double()[rows, s]).cpu().numpy())
    return np.concatenate(out)


def _fact_sets(facts, quads):
    """Per quadruple and side, by brute force over the fact array: (time-agnostic set, time-aware set) of the values that
    complete its key -> {'o': [(agnostic, aware)], 's': [...]}."""
    out = {'o': [], 's': []}
    for s, r, o, t in quads.tolist():
        for side, key, kc, vc in (('o', s, 0, 2), ('s', o, 2, 0)):
            m = (facts[:, kc] == key) & (facts[:, 1] == r)
            out[side].append((set(facts[m, vc].tolist()), set(facts[m & (facts[:, 3] == t), vc].tolist())))
    return out


def _time_aware_torch(seen, facts, dev):
    """model._rank_rows on the recorded score matrices with brute-force time-aware sets -> ranks [len, 2]."""
    import model as M
    out = []
    for tr, sub_pred, ob_pred in seen:
        sets = _fact_sets(facts, tr)
        res = []
        for side, pred, lab in (('s', sub_pred, tr[:, 0]), ('o', ob_pred, tr[:, 2])):
            lists = [np.asarray(sorted(aware), dtype=np.int64) for _, aware in sets[side]]
            res.append(M._rank_rows(pred, torch.from_numpy(lab).to(dev), *_pairs(lists, dev)))
        out.append(np.stack(res, axis=1))
    return np.concatenate(out)


@pytest.fixture(scope='module')
def passes(dev):
    """One pass per entry point over valid[:n_eval] of eval_small_100, each on a freshly set-up model (a pass advances the
    inference state): the parent's raw and filtered streams (device_rank off and on) and the new one-pass stream."""
    import test_gpu_parity as P
    gold = load_golden('eval_small_100.npz')
    n_eval = int(gold['n_eval'])
    res = {'n_eval': n_eval}

    def one(name, run, device_rank=False):
        net, gnet, H, gd, samples, total, valid, va = P._eval_setup(dev, gold)
        net.device_rank = device_rank
        seen = _recorded(net)
        (vs, vst), (vo, vot) = H['valid']
        out = run(net, valid[:n_eval], (vs[:n_eval], vst[:n_eval]), (vo[:n_eval], vot[:n_eval]), gnet, total)
        assert len(samples) == 0
        res[name] = out + (seen,)
        res['facts'], res['quads'] = total.cpu().numpy(), va[:n_eval]

    one('raw', lambda net, q, sh, oh, g, total: net.evaluate_stream(q, sh, oh, g))
    one('filter_off', lambda net, q, sh, oh, g, total: net.evaluate_filter_stream(q, sh, oh, g, total))
    one('filter_on', lambda net, q, sh, oh, g, total: net.evaluate_filter_stream(q, sh, oh, g, total), device_rank=True)
    one('all', lambda net, q, sh, oh, g, total: net.evaluate_all_stream(q, sh, oh, g, total))
    return res


def test_fixture_separates_the_three_settings(passes):
    """On the fact arrays alone: rows with a time-aware competitor other than the gold entity, and rows whose time-agnostic
    set is strictly larger than the time-aware one, exist on both sides (180 quadruples: 10 / 11 and 126 / 124 rows)."""
    sets = _fact_sets(passes['facts'], passes['quads'])
    for side, gold_col in (('o', 2), ('s', 0)):
        gold = passes['quads'][:, gold_col].tolist()
        competitor = sum(len(aware - {g}) > 0 for (_, aware), g in zip(sets[side], gold))
        larger = sum(aware < agnostic for agnostic, aware in sets[side])
        print('side', side, 'rows with a time-aware competitor', competitor, 'rows with a larger time-agnostic set', larger)
        assert competitor >= 1 and larger >= 1
        assert all(g in aware for (_, aware), g in zip(sets[side], gold))


def test_one_pass_stream_equals_the_one_setting_streams(dev, passes):
    import utils as U
    n_eval = passes['n_eval']
    ranks, loss, seen = passes['all']
    assert sorted(ranks) == sorted(SETTINGS)
    for name in SETTINGS:
        assert ranks[name].shape == (n_eval, 2) and ranks[name].dtype == np.float64
        assert sorted(U.rank_metrics(ranks[name])) == ['hits@1', 'hits@10', 'hits@3', 'mr', 'mrr']
    assert loss.shape == (n_eval,)
    print('rows differing: raw', int((ranks['raw'] != passes['raw'][0]).sum()),
          'filtered vs torch tail', int((ranks['filtered'] != passes['filter_off'][0]).sum()),
          'filtered vs device tail', int((ranks['filtered'] != passes['filter_on'][0]).sum()))
    assert np.array_equal(ranks['raw'], passes['raw'][0])
    assert np.array_equal(ranks['filtered'], passes['filter_off'][0])
    assert np.array_equal(ranks['filtered'], passes['filter_on'][0])
    want = _time_aware_torch(seen, passes['facts'], dev)
    print('time_filtered rows differing from the torch formulation', int((ranks['time_filtered'] != want).sum()),
          'rows where time_filtered > filtered', int((ranks['time_filtered'] > ranks['filtered']).sum()))
    assert np.array_equal(ranks['time_filtered'], want)
    assert np.all(ranks['filtered'] <= ranks['time_filtered'])
    assert U.rank_metrics(ranks['filtered']) == U.rank_metrics(passes['filter_on'][0])
    # the losses: the bound of test_gpu_rank.test_filtered_stream_with_device_rank_equals_the_torch_tail -- the error of the
    # softmax_ce path against float64 on these very score matrices
    l0, seen0 = passes['filter_off'][1:]
    ref0, ref = _loss64(seen0, dev), _loss64(seen, dev)
    print('loss: softmax_ce error', np.abs(l0 - ref0).max(), 'rank_rows3 error', np.abs(loss - ref).max())
    assert np.array_equal(ref0, ref)                                       # identical score matrices on both sides
    assert np.abs(loss - ref).max() <= np.abs(l0 - ref0).max()


def test_time_filter_sequential_calls_equal_the_one_pass_stream(dev):
    """evaluate_time_filter, one call per quadruple, vs evaluate_all_stream on an identical model, by the criterion of
    test_raw_stream_equals_sequential_evaluate_calls for batched against one-row scoring."""
    import test_gpu_parity as P
    gold = load_golden('eval_small_100.npz')
    n = 48
    net, gnet, H, gd, samples, total, valid, va = P._eval_setup(dev, gold)
    (vs, vst), (vo, vot) = H['valid']
    with torch.no_grad():
        seq = [net.evaluate_time_filter(valid[i], (vs[i], vst[i]), (vo[i], vot[i]), gnet, total) for i in range(n)]
    ranks_seq = np.asarray([r for r, _ in seq])
    loss_seq = np.asarray([float(l) for _, l in seq])
    net2, gnet2, H2, gd2, samples2, total2, valid2, _ = P._eval_setup(dev, gold)
    ranks, loss = net2.evaluate_all_stream(valid2[:n], (vs[:n], vst[:n]), (vo[:n], vot[:n]), gnet2, total2)
    ranks = ranks['time_filtered']
    assert len(samples) == len(samples2) and ranks.shape == (n, 2)
    print('time-aware stream: ranks identical', float(np.mean(ranks == ranks_seq)), 'largest difference',
          np.abs(ranks - ranks_seq).max(), 'loss difference', np.abs(loss - loss_seq).max())
    np.testing.assert_allclose(loss, loss_seq, rtol=1e-5, atol=1e-5)
    assert float(np.mean(ranks == ranks_seq)) >= 0.99 and np.abs(ranks - ranks_seq).max() <= 1
