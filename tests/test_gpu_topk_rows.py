"""GPU tests of the ranked top-k predictions (run with -m gpu on an MI355X): renet_topk_rows (csrc/topk_rows.hip: the k best
candidates of every score row -- filtered, sorted by score then column, with log-probabilities -- from one read of the row)
against a numpy reference -- exact in index, value and count --, its logp against a float64 logsumexp, and the public paths
(RENet.predict_topk_batch / predict_topk_stream) on the evaluation fixture, against the same reference on the recorded score
matrices and against the counts of renet_rank_rows3."""
import functools

import numpy as np
import pytest
import torch

from helpers import load_golden
from test_gpu_rank import LOGITS, SHAPES, _facts_for, _scores
from test_gpu_rank_settings import _brute_lists, _fact_sets, _recorded, _table

pytestmark = pytest.mark.gpu

KS = (1, 10, 1000)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _lse64(x):
    """float64 logsumexp of every row of x [n, C]."""
    x = x.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def _reference(x, k, lists=None, keep=None):
    """The contract of renet_topk_rows on the host matrix x [n, C]: per row the candidates by boolean mask (all columns minus
    the listed ones inside [0, C), the keep column put back), ordered by np.lexsort((column, -score)) -- -0.0 and +0.0 equal
    --, the first k -> (idx int32 [n, k], val float32 [n, k], n_valid int32 [n]) with the padding -1 / -inf."""
    n, C = x.shape
    idx, val = np.full((n, k), -1, dtype=np.int32), np.full((n, k), -np.inf, dtype=np.float32)
    nv = np.zeros(n, dtype=np.int32)
    for i in range(n):
        cand = np.ones(C, dtype=bool)
        if lists is not None:
            li = np.asarray(lists[i], dtype=np.int64)
            cand[li[(li >= 0) & (li < C)]] = False
            if keep is not None and 0 <= keep[i] < C:
                cand[keep[i]] = True
        col = np.nonzero(cand)[0]
        sc = x[i, col]
        order = np.lexsort((col, -sc))[:k]
        nv[i] = len(order)
        idx[i, :len(order)], val[i, :len(order)] = col[order], sc[order]
    return idx, val, nv


def _assert_logp(logp, val, nv, lse):
    """Finite entries: |logp - (val - lse)| <= spacing(|lse|) + spacing(|logp|) in fp32 (one rounding of the logsumexp, one
    of the subtraction); -inf scores and the padding: -inf."""
    ref = val.astype(np.float64) - lse[:, None]
    fin = np.isfinite(val) & (np.arange(val.shape[1])[None, :] < nv[:, None])
    bound = np.spacing(np.abs(lse).astype(np.float32)).astype(np.float64)[:, None] + \
        np.spacing(np.abs(np.where(fin, ref, 1.0)).astype(np.float32)).astype(np.float64)
    err = np.abs(logp.astype(np.float64) - np.where(fin, ref, 0.0))
    worst = float((err / bound)[fin].max()) if fin.any() else 0.0
    print('logp: largest error / bound', worst)
    assert np.all(err[fin] <= bound[fin])
    assert np.all(logp[~fin] == -np.inf)


def _assert_same(got, want, where):
    idx, val, nv = got[0].cpu().numpy(), got[1].cpu().numpy(), got[3].cpu().numpy()
    bad = int((idx != want[0]).any(axis=1).sum()), int((val != want[1]).any(axis=1).sum()), int((nv != want[2]).sum())
    print(where, 'rows differing in idx / val / n_valid', bad)
    assert idx.dtype == np.int32 and nv.dtype == np.int32 and val.dtype == np.float32
    assert np.array_equal(nv, want[2]) and np.array_equal(idx, want[0]) and np.array_equal(val, want[1])
    assert not np.any(val == np.float32(3e38))                    # the row padding of _scores was never read as a column
    return idx, val, nv


@functools.lru_cache(maxsize=None)
def _case(n, C, ld, logits):
    """One score matrix of test_gpu_rank._scores with everything the tests share, computed once: (scores, label) on the
    device, the host copy, its float64 logsumexp and the list plans (no list, then the four KINDS dealt as test_gpu_rank
    deals them) as (host lists or None, device (cols, start, count) or three Nones)."""
    dev = torch.device('cuda:0')
    scores, label = _scores(dev, n, C, ld, logits)
    x = scores.cpu().numpy()
    lab = label.cpu().numpy()
    plans = [(None, (None, None, None))]
    for p, plan in enumerate([np.arange(n) % 4] if n >= 8 else [np.full(n, q) for q in range(4)]):
        at = _facts_for(n, C, lab, plan, seed=n + C + p)
        lists = _brute_lists(at, n, np.zeros(n, dtype=np.int64))[0] if len(at) else [np.zeros(0, dtype=np.int64)] * n
        plans.append((lists, tuple(torch.from_numpy(t).to(dev) for t in _table(lists, C, 1 + p))))
    return scores, label, x, lab, _lse64(x), plans


@pytest.mark.parametrize('logits', LOGITS)
@pytest.mark.parametrize('n,C,ld', SHAPES)
def test_topk_rows_equals_the_reference_exactly(dev, n, C, ld, logits):
    import renet_hip as K
    scores, label, x, lab, lse, plans = _case(n, C, ld, logits)
    before = scores.clone()
    lab32 = label.int()
    for p, (lists, table) in enumerate(plans):
        for keep in (None, lab32):
            want_all = _reference(x, max(KS), lists, None if keep is None else lab)
            for k in KS:
                got = K.topk_rows(scores, k, *table, keep=keep)
                want = (want_all[0][:, :k], want_all[1][:, :k], np.minimum(want_all[2], k))
                idx, val, nv = _assert_same(got, want, '%d x %d (ld %d) %s plan %d keep %s k %d:' %
                                            (n, C, ld, logits, p, keep is not None, k))
                _assert_logp(got[2].cpu().numpy(), val, nv, lse)
            if lists is not None and n >= 8:                  # the plan does deal every_column: nothing left, or the label
                assert int(want_all[2].min()) == (0 if keep is None else 1)
    assert torch.equal(scores, before)


def test_largest_served_row(dev):
    """C = 32768, the bound the header states: the largest LDS request the kernel makes."""
    import renet_hip as K
    n, C = 2, 32768
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, C, generator=g) * 8
    lists = [np.arange(0, C, 3), np.zeros(0, dtype=np.int64)]
    table = tuple(torch.from_numpy(t).to(dev) for t in _table(lists, C, 3))
    for k in (10, 1024):
        got = K.topk_rows(x.to(dev), k, *table)
        idx, val, nv = _assert_same(got, _reference(x.numpy(), k, lists), 'C = 32768 k %d:' % k)
        _assert_logp(got[2].cpu().numpy(), val, nv, _lse64(x.numpy()))


def test_special_values(dev):
    """A hand-made 4 x 37 matrix: signed zeros, -inf scores, a list with entries outside the row and the keep column, and an
    empty range that starts beyond the table."""
    import renet_hip as K
    n, C = 4, 37
    rng = np.random.RandomState(7)
    x = (rng.randn(n, C) * 3).astype(np.float32)
    zeros = [3, 4, 9, 20, 21, 36]
    x[0, zeros] = [0.0, -0.0, -0.0, 0.0, -0.0, 0.0]           # tie, and order by column
    minus_inf = [0, 5, 6, 17, 36]
    x[1, minus_inf] = -np.inf
    best = int(np.argsort(-x[2])[0])
    lists = [np.array([3, 20, 30]),                           # two of the zeros and another column
             np.array([5, 8]),                                # one of the -inf columns: filtered, the others are not
             np.array([-1, C + 5, best, 11, 12]),             # outside the row twice, the keep column, two ordinary ones
             np.zeros(0, dtype=np.int64)]
    cols = np.concatenate(lists + [np.array([1, 2])]).astype(np.int32)
    count = np.array([3, 2, 5, 0], dtype=np.int32)
    start = np.array([0, 3, 5, len(cols) + 7], dtype=np.int32)
    keep = np.array([-1, C + 3, best, 0], dtype=np.int32)     # nothing exempt in rows 0, 1 (outside the row), 3 (not listed)
    table = tuple(torch.from_numpy(t).to(dev) for t in (cols, start, count))
    xd = torch.from_numpy(x).to(dev)
    assert best not in (11, 12)
    for k in (5, 35, 40):
        for kp in (None, keep):
            got = K.topk_rows(xd, k, *table, keep=None if kp is None else torch.from_numpy(kp).to(dev))
            idx, val, nv = _assert_same(got, _reference(x, k, lists, kp), 'special values k %d keep %s:' % (k, kp is not None))
            _assert_logp(got[2].cpu().numpy(), val, nv, _lse64(x))
            logp = got[2].cpu().numpy()
            assert nv.tolist() == [min(k, 34), min(k, 35), min(k, 34 + (kp is not None)), min(k, 37)]
            # the padding is distinct from everything real, a -inf score from a filtered column
            assert np.all((idx >= 0) == (np.arange(k)[None, :] < nv[:, None])) and np.all(idx < C)
            if k >= 35:
                real_inf = (val[1] == -np.inf) & (idx[1] >= 0)
                assert sorted(idx[1][real_inf].tolist()) == [0, 6, 17, 36] and np.all(logp[1][real_inf] == -np.inf)
                assert 5 not in idx[1] and 8 not in idx[1]
                z = [c for c in idx[0].tolist() if c in zeros]
                assert z == [4, 9, 21, 36]                    # the unlisted zeros, by column whatever their sign
                assert np.all(val[0][np.isin(idx[0], zeros)] == 0.0)
            assert (idx[2, 0] == best) == (kp is not None)


@pytest.mark.parametrize('logits', LOGITS)
@pytest.mark.parametrize('n,C,ld', SHAPES)
def test_logp_of_the_label_equals_the_row_loss(dev, n, C, ld, logits):
    """Where the label is among the top k, -logp there and row_loss of renet_rank_rows are two roundings of the same number:
    within spacing(|lse|) + spacing(|logp|).  want_logp=False changes nothing else."""
    import renet_hip as K
    scores, label, x, lab, lse, plans = _case(n, C, ld, logits)
    _, loss = K.rank_rows(scores, label.int(), filtered=False, want_loss=True)
    loss = loss.cpu().numpy()
    k = 10
    idx, val, logp, nv = K.topk_rows(scores, k)
    plain = K.topk_rows(scores, k, want_logp=False)
    assert plain[2] is None
    assert torch.equal(plain[0], idx) and torch.equal(plain[1], val) and torch.equal(plain[3], nv)
    idx, logp = idx.cpu().numpy(), logp.cpu().numpy()
    rows, pos = np.nonzero(idx == lab[:, None])
    bound = np.spacing(np.abs(lse[rows]).astype(np.float32)) + np.spacing(np.abs(logp[rows, pos]))
    err = np.abs(-logp[rows, pos].astype(np.float64) - loss[rows])
    print('label among the top', k, 'in', len(rows), 'of', n, 'rows; largest |(-logp) - row_loss| / bound',
          float((err / bound).max()) if len(rows) else 0.0)
    assert np.all(err <= bound)
    if logits == 'normal8' and n >= 3:
        assert len(rows) >= 1                                 # every other row's label is its third largest


def test_argument_checks(dev):
    import renet_hip as K
    L = K.lib()
    s = torch.zeros(4, 8, device=dev)
    idx = torch.full((4, 3), 7, device=dev, dtype=torch.int32)
    val = torch.full((4, 3), 7.0, device=dev)
    logp = torch.full((4, 3), 7.0, device=dev)
    nv = torch.full((4,), 7, device=dev, dtype=torch.int32)
    cols = torch.arange(16, device=dev, dtype=torch.int32) % 8
    rng = torch.zeros(4, device=dev, dtype=torch.int32)
    p = lambda t: None if t is None else t.data_ptr()

    def call(n=4, C=8, ld=8, k=3, lst=(None, None, None, 0)):
        return L.renet_topk_rows(p(s), ld, n, C, k, p(lst[0]), p(lst[1]), p(lst[2]), lst[3], None, p(idx), p(val), p(logp),
                                 p(nv), K._stream())
    assert call(k=0) == -1 and call(k=1025) == -1 and call(ld=7) == -1 and call(n=-1) == -1 and call(C=0) == -1
    for bad in ((cols, rng, None, 16), (None, rng, rng, 0), (cols, None, rng, 16), (cols, rng, rng, -1)):
        assert call(lst=bad) == -1
    assert L.renet_topk_rows(p(s), 8, 4, 8, 3, None, None, None, 0, None, None, p(val), p(logp), p(nv), K._stream()) == -1
    assert call(n=0) == 0                                                      # no-op: nothing launched, nothing written
    # a C the kernel's design does not serve is refused before any launch (n = 0: nothing could be read anyway)
    assert call(n=0, C=1 << 20, ld=1 << 20) == -2 and call(n=0, C=32769, ld=32769) == -2
    torch.cuda.synchronize()
    assert idx.eq(7).all() and val.eq(7).all() and logp.eq(7).all() and nv.eq(7).all()
    # the all-zero rows tie in every column: the lowest columns, each with probability 1 / 8
    assert call() == 0
    assert idx.tolist() == [[0, 1, 2]] * 4 and val.eq(0).all() and nv.tolist() == [3] * 4
    np.testing.assert_allclose(logp.cpu().numpy(), -np.log(8.0), rtol=1e-6)
    # a range is cut to the length given for its table: cols = 0 1 2 ...: [0, 100) cut to len 2 lists columns 0 and 1 only
    start = torch.tensor([0, 0, 1, -3], device=dev, dtype=torch.int32)
    count = torch.tensor([100, 0, 100, 4], device=dev, dtype=torch.int32)
    assert call(lst=(cols, start, count, 2)) == 0
    assert idx.tolist() == [[2, 3, 4], [0, 1, 2], [0, 2, 3], [1, 2, 3]]        # row 3: [-3, 1) cut to [0, 1)
    with pytest.raises(K.RenetHipError):
        K.topk_rows(s.double(), 3)
    with pytest.raises(K.RenetHipError):
        K.topk_rows(s, 3, cols, rng, None)
    with pytest.raises(K.RenetHipError):
        K.topk_rows(s, 0)


# ---------------------------------------------------------------------------------------------
# the public paths on the evaluation fixture (set up as the `passes` fixture of tests/test_gpu_rank_settings.py)
# ---------------------------------------------------------------------------------------------
K_PUBLIC = 10


def _recorded_counts():
    """Keeps the counts of every renet_hip.rank_rows3 call -> (list, undo)."""
    import renet_hip as K
    seen, inner = [], K.rank_rows3

    def rank_rows3(*a, **k):
        out = inner(*a, **k)
        seen.append(out[0].cpu().numpy())
        return out
    K.rank_rows3 = rank_rows3

    def undo():
        K.rank_rows3 = inner
    return seen, undo


@pytest.fixture(scope='module')
def passes(dev):
    """One predict_topk_stream pass over valid[:n_eval] of eval_small_100 per (setting, keep_gold), each on a freshly set-up
    model with predict_batch recorded, and one evaluate_all_stream pass with the counts of rank_rows3 recorded."""
    import model as M
    import test_gpu_parity as P
    gold = load_golden('eval_small_100.npz')
    n_eval = int(gold['n_eval'])
    res = {'n_eval': n_eval}

    def fresh():
        net, gnet, H, gd, samples, total, valid, va = P._eval_setup(dev, gold)
        (vs, vst), (vo, vot) = H['valid']
        res['facts'], res['quads'] = total.cpu().numpy(), va[:n_eval]
        return net, samples, (valid[:n_eval], (vs[:n_eval], vst[:n_eval]), (vo[:n_eval], vot[:n_eval]), gnet), total

    for setting in M.SETTINGS:
        for keep_gold in (False, True):
            net, samples, args, total = fresh()
            seen = _recorded(net)
            out = net.predict_topk_stream(*args, k=K_PUBLIC, all_triplets=total, setting=setting, keep_gold=keep_gold)
            assert len(samples) == 0
            res[setting, keep_gold] = (out, seen)
    net, samples, args, total = fresh()
    counts, undo = _recorded_counts()
    try:
        net.evaluate_all_stream(*args, total)
    finally:
        undo()
    assert len(samples) == 0
    # one call per side ('s' first) and group -> {'sub': [6, n_eval], 'ob': [6, n_eval]}
    res['counts'] = {'sub': np.concatenate(counts[0::2], axis=1), 'ob': np.concatenate(counts[1::2], axis=1)}
    res['spent'] = (net, args, total)                         # (its stream is used up; the refusals come before any use)
    res['fresh'] = fresh
    return res


SIDES = (('sub', 's', 0, 1), ('ob', 'o', 2, 2))              # result name, _fact_sets side, gold column, position in `seen`


@pytest.mark.parametrize('keep_gold', [False, True])
@pytest.mark.parametrize('setting', ['raw', 'filtered', 'time_filtered'])
def test_stream_equals_the_reference_on_the_recorded_scores(passes, setting, keep_gold):
    out, seen = passes[setting, keep_gold]
    n_eval = passes['n_eval']
    assert sum(len(g[0]) for g in seen) == n_eval and len(seen) > 1
    for name, side, gold_col, pred_at in SIDES:
        idx, val, logp, nv = out[name]
        assert idx.shape == val.shape == logp.shape == (n_eval, K_PUBLIC) and nv.shape == (n_eval,)
        assert idx.dtype == np.int32 and nv.dtype == np.int32
        at, removed = 0, 0
        for group in seen:
            tr, pred = group[0], group[pred_at].cpu().numpy()
            sets = _fact_sets(passes['facts'], tr)[side]
            lists = None if setting == 'raw' else \
                [np.asarray(sorted(ag if setting == 'filtered' else aw), dtype=np.int64) for ag, aw in sets]
            want = _reference(pred, K_PUBLIC, lists, tr[:, gold_col] if keep_gold else None)
            rows = slice(at, at + len(tr))
            assert np.array_equal(idx[rows], want[0]) and np.array_equal(val[rows], want[1])
            assert np.array_equal(nv[rows], want[2])
            _assert_logp(logp[rows], val[rows], nv[rows], _lse64(pred))
            removed += 0 if lists is None else sum(len(x) for x in lists)
            at += len(tr)
        assert (removed > 0) == (setting != 'raw')
        gold = passes['quads'][:, gold_col]
        hit = (idx == gold[:, None]).any(axis=1)
        print(setting, 'keep_gold', keep_gold, name, 'gold entity listed in', int(hit.sum()), 'of', n_eval, 'rows')
        if setting != 'raw' and not keep_gold:                # the gold entity is a known fact of its own timestamp
            assert not hit.any()


def test_one_group_through_predict_topk_batch_equals_its_stream_rows(passes):
    setting, keep_gold = 'time_filtered', False
    out, seen = passes[setting, keep_gold]
    net, samples, (quads, sh, oh, gnet), total = passes['fresh']()
    m = len(seen[0][0])                                       # the quadruples of the first timestamp
    assert 0 < m < passes['n_eval']
    got = net.predict_topk_batch(quads[:m], (sh[0][:m], sh[1][:m]), (oh[0][:m], oh[1][:m]), gnet, k=K_PUBLIC,
                                 all_triplets=total, setting=setting, keep_gold=keep_gold)
    assert sorted(got) == ['ob', 'sub']
    for name in got:
        assert all(t.is_cuda for t in got[name])
        for a, b in zip(got[name], out[name]):
            assert np.array_equal(a.cpu().numpy(), b[:m])


@pytest.mark.parametrize('s', range(3))
def test_lists_are_consistent_with_the_ranks(passes, s):
    """With keep_gold the gold entity's place in the list and the (greater, equal) counts of renet_rank_rows3 bound each
    other.  The counts of the filtered settings compare sigmoid(score), which is monotone but collapses distinct scores, so:
    greater <= position (rank - (equal - 1) / 2 - 1 = greater), position <= greater + equal - 1."""
    import model as M
    setting = M.SETTINGS[s]
    out, _ = passes[setting, True]
    for name, side, gold_col, _ in SIDES:
        idx = out[name][0]
        greater, equal = passes['counts'][name][2 * s], passes['counts'][name][2 * s + 1]
        rank = greater + (equal - 1.0) / 2 + 1
        gold = passes['quads'][:, gold_col]
        hit = idx == gold[:, None]
        listed, pos = hit.any(axis=1), hit.argmax(axis=1)
        print(setting, name, 'listed', int(listed.sum()), 'must be listed', int((greater + equal - 1 < K_PUBLIC).sum()))
        assert np.all((rank - (equal - 1.0) / 2 - 1)[listed] <= pos[listed])
        assert np.all(listed[greater + equal - 1 < K_PUBLIC])
        if setting == 'raw':
            print('raw greater >= k in', int((greater >= K_PUBLIC).sum()), 'rows')
            assert not np.any(listed[greater >= K_PUBLIC])


def test_refusals(passes):
    net, (quads, sh, oh, gnet), total = passes['spent']
    m = len(passes[('raw', False)][1][0][0])
    one = (quads[:m], (sh[0][:m], sh[1][:m]), (oh[0][:m], oh[1][:m]), gnet)
    for setting in ('filtered', 'time_filtered'):
        with pytest.raises(ValueError):
            net.predict_topk_batch(*one, k=K_PUBLIC, setting=setting)
        with pytest.raises(ValueError):
            net.predict_topk_stream(quads, sh, oh, gnet, k=K_PUBLIC, setting=setting)
    with pytest.raises(ValueError):
        net.predict_topk_batch(*one, k=K_PUBLIC, all_triplets=total, setting='time')
    two = m + 1                                               # quadruples of two timestamps, as predict_batch refuses them
    assert len(np.unique(passes['quads'][:two, 3])) == 2
    with pytest.raises(ValueError, match='ONE timestamp'):
        net.predict_topk_batch(quads[:two], (sh[0][:two], sh[1][:two]), (oh[0][:two], oh[1][:two]), gnet, k=K_PUBLIC)
