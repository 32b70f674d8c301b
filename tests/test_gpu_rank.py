"""GPU tests of the device-ranked evaluation (run with -m gpu on an MI355X): the one-pass rank kernel (csrc/rank.hip,
renet_rank_rows) against the torch formulation it replaces (model._rank_rows) on the SAME device score matrix -- exact --,
its loss against renet_softmax_ce, the resident filter index (filter_index.FilterIndex) against model._known_pairs, and
the public paths (RENet.device_rank, evaluate_batch / evaluate_stream) on the evaluation fixture."""
import numpy as np
import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu

# (n, C, ld): one element rows up; C % 4 != 0 with aligned and unaligned row starts (ld % 4 != 0: rows start at every
# 16-byte phase); more rows than one wave of workgroups; the ICEWS18 entity count; fewer float4 groups than threads
SHAPES = [(1, 5, 5), (3, 257, 257), (65, 1000, 1024), (130, 23033, 23040), (7, 4099, 4100)]
LOGITS = ['normal8', 'blocks', 'equal']
KINDS = ('empty', 'with_label', 'every_column', 'random')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _scores(dev, n, C, ld, logits):
    """(scores [n, C] as a view of an [n, ld] buffer whose padding holds 3e38 -- a read past C would count --, label [n])."""
    g = torch.Generator().manual_seed(n * 1000003 + C * 17 + len(logits))
    buf = torch.full((n, ld), 3e38)
    label = torch.randint(0, C, (n,), generator=g)
    if logits == 'normal8':              # N(0, 1) * 8: fp32 sigmoid maps many of these onto one value (real ties);
        buf[:, :C] = torch.randn(n, C, generator=g) * 8
        top = buf[:, :C].topk(min(3, C), dim=1).indices[:, -1]             # every other row's gold column is its third
        label = torch.where(torch.arange(n) % 2 == 0, top, label)          # largest, as for a well-ranked quadruple
    elif logits == 'blocks':             # sigmoid saturated to 1.0 / exactly 0 in blocks, the label inside a block
        buf[:, :C] = torch.randn(n, C, generator=g) * 8
        a, b = max(C // 3, 1), max(2 * C // 3, 2)
        buf[:, :a], buf[:, a:b] = 120.0, -120.0
        lo = torch.tensor([0, a, b])[torch.arange(n) % 3]
        hi = torch.tensor([a, b, C])[torch.arange(n) % 3]
        label = lo + (label % torch.clamp(hi - lo, min=1))
        label = torch.clamp(label, max=C - 1)
    else:                                # every row all-equal (another constant per row, a zero row among them)
        buf[:, :C] = (torch.arange(n).float().view(-1, 1) - 1.0) * 0.37
    return buf.to(dev)[:, :C], label.to(dev)


def _facts_for(n, C, label, plan, seed):
    """all_triplets whose objects of the key (s = i, r = 0) are row i's filter list of kind plan[i]; every fact once more at a
    second timestamp and a third of them at a third one (the index must deduplicate)."""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        kind = KINDS[plan[i]]
        if kind == 'empty':
            continue
        if kind == 'with_label':
            cols = np.union1d(rng.randint(0, C, min(C, 6)), [label[i]])
        elif kind == 'every_column':
            cols = np.arange(C)
        else:
            cols = np.unique(rng.randint(0, C, max(C // 100, 1)))
        rows.append(np.stack((np.full(len(cols), i), np.zeros(len(cols), dtype=np.int64), cols), axis=1))
    if not rows:
        return np.zeros((0, 4), dtype=np.int64)
    f = np.concatenate(rows).astype(np.int64)
    at = np.concatenate((np.c_[f, np.zeros(len(f), dtype=np.int64)], np.c_[f, np.full(len(f), 24)],
                         np.c_[f[::3], np.full(len(f[::3]), 48)]))
    return at[rng.permutation(len(at))]


def _torch_counts(scores, label, filt_rows=None, filt_cols=None):
    """The steps of model._rank_rows, returning the two counts."""
    rows = torch.arange(scores.shape[0], device=scores.device)
    if filt_rows is not None:
        scores = torch.sigmoid(scores)
        ground = scores[rows, label].clone()
        scores[filt_rows, filt_cols] = 0
        scores[rows, label] = ground
    else:
        ground = scores[rows, label]
    return (scores > ground[:, None]).sum(dim=1), (scores == ground[:, None]).sum(dim=1)


@pytest.mark.parametrize('logits', LOGITS)
@pytest.mark.parametrize('n,C,ld', SHAPES)
def test_rank_kernel_equals_the_torch_path_exactly(dev, n, C, ld, logits):
    import filter_index as FI
    import model as M
    import renet_hip as K
    scores, label = _scores(dev, n, C, ld, logits)
    lab32 = label.int()
    # raw
    cnt, _ = K.rank_rows(scores, lab32, filtered=False, want_loss=False)
    g, e = _torch_counts(scores, label)
    print('raw', n, C, ld, logits, 'greater', int((cnt[0] != g).sum()), 'equal', int((cnt[1] != e).sum()), 'rows differ')
    assert torch.equal(cnt[0].long(), g) and torch.equal(cnt[1].long(), e)
    ranks = (cnt[0].double() + (cnt[1].double() - 1.0) / 2 + 1).cpu().numpy()
    assert np.array_equal(ranks, M._rank_rows(scores, label))
    # filtered: every kind of list on every row (small n), or the kinds dealt round-robin over the rows
    plans = [np.arange(n) % 4] if n >= 8 else [np.full(n, k) for k in range(4)]
    keys = np.stack((np.arange(n), np.zeros(n, dtype=np.int64)), axis=1)
    ties = 0
    for p, plan in enumerate(plans):
        at = _facts_for(n, C, label.cpu().numpy(), plan, seed=n + C + p)
        ptr, col = FI.FilterIndex(at).lookup('o', keys, dev)
        cnt, _ = K.rank_rows(scores, lab32, ptr, col, filtered=True, want_loss=False)
        fr, fc = (torch.from_numpy(x).to(dev) for x in M._known_pairs(at, (0, 1), 2, keys)) if len(at) else \
            (torch.zeros(0, dtype=torch.long, device=dev),) * 2
        g, e = _torch_counts(scores, label, fr, fc)
        print('filtered', n, C, ld, logits, 'plan', p, 'greater', int((cnt[0] != g).sum()), 'equal',
              int((cnt[1] != e).sum()), 'rows differ; ties max', int(e.max()))
        assert torch.equal(cnt[0].long(), g) and torch.equal(cnt[1].long(), e)
        ranks = (cnt[0].double() + (cnt[1].double() - 1.0) / 2 + 1).cpu().numpy()
        assert np.array_equal(ranks, M._rank_rows(scores, label, fr, fc))
        ties = max(ties, int(e.max()))
    if logits == 'normal8' and C >= 1000:
        assert ties > 1                      # the matrix does produce sigmoid ties with the gold column


def test_filtered_without_lists_and_scores_untouched(dev):
    import renet_hip as K
    scores, label = _scores(dev, 9, 1031, 1031, 'blocks')
    before = scores.clone()
    cnt, _ = K.rank_rows(scores, label.int(), filtered=True, want_loss=False)
    g, e = _torch_counts(scores, label, torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.long, device=dev))
    assert torch.equal(cnt[0].long(), g) and torch.equal(cnt[1].long(), e)
    assert torch.equal(scores, before)


@pytest.mark.parametrize('logits', LOGITS)
@pytest.mark.parametrize('n,C,ld', SHAPES)
def test_row_loss_is_as_accurate_as_softmax_ce(dev, n, C, ld, logits):
    """row_loss against renet_softmax_ce (no gradient) on the same matrix.  The two kernels sum in different orders, so
    this is a tolerance: the largest error renet_softmax_ce itself has on THIS matrix against a float64 logsumexp, measured
    here, is the bound the new kernel has to keep against the same float64 reference; the two kernels then differ by at most
    twice that (triangle inequality).  renet_softmax_ce is finite on the +-120 matrices (the row maximum is subtracted), so
    they take part."""
    import renet_hip as K
    scores, label = _scores(dev, n, C, ld, logits)
    rows = torch.arange(n, device=dev)
    ref = torch.logsumexp(scores.double(), dim=1) - scores.double()[rows, label]
    old = K.softmax_ce(scores, label.int(), 1.0, False)
    assert bool(torch.isfinite(old).all())
    bound = float((old.double() - ref).abs().max())
    for filtered in (False, True):
        _, new = K.rank_rows(scores, label.int(), filtered=filtered, want_loss=True)
        err = float((new.double() - ref).abs().max())
        print('loss', n, C, ld, logits, 'filtered' if filtered else 'raw', 'softmax_ce error', bound, 'rank_rows error', err,
              'between the kernels', float((new - old).abs().max()))
        assert err <= bound
        assert float((new.double() - old.double()).abs().max()) <= 2 * bound


def test_argument_checks(dev):
    import renet_hip as K
    L = K.lib()
    s = torch.zeros(4, 8, device=dev)
    lab = torch.tensor([0, 7, -5, 99], device=dev, dtype=torch.int32)
    out = torch.zeros(2, 4, device=dev, dtype=torch.int32)
    p = lambda t: t.data_ptr()
    args = lambda n, C, ld: (p(s), ld, n, C, p(lab), None, None, 0, p(out[0]), p(out[1]), None, K._stream())
    assert L.renet_rank_rows(*args(-1, 8, 8)) == -1 and L.renet_rank_rows(*args(4, 0, 8)) == -1
    assert L.renet_rank_rows(*args(4, 8, 7)) == -1
    assert L.renet_rank_rows(*args(0, 8, 8)) == 0                              # no-op
    ptr = torch.zeros(5, device=dev, dtype=torch.int32)
    assert L.renet_rank_rows(p(s), 8, 4, 8, p(lab), p(ptr), p(ptr), 0, p(out[0]), p(out[1]), None, K._stream()) == -1
    # labels outside [0, C) are clamped into the row: the all-zero rows tie in every column whatever the label
    cnt, loss = K.rank_rows(s, lab, filtered=False)
    assert cnt[0].tolist() == [0] * 4 and cnt[1].tolist() == [8] * 4
    np.testing.assert_allclose(loss.cpu().numpy(), np.log(8.0), rtol=1e-6)
    with pytest.raises(K.RenetHipError):
        K.rank_rows(s.double(), lab)


# ---------------------------------------------------------------------------------------------
# the public paths on the evaluation fixture (set up as tests/test_gpu_parity.py sets up its stream test)
# ---------------------------------------------------------------------------------------------
def _recorded(net):
    """Keeps the score matrices of every predict_batch call of `net` (for a float64 reference of its losses)."""
    seen, inner = [], net.predict_batch

    def predict_batch(tr, *a, **k):
        out = inner(tr, *a, **k)
        seen.append((np.asarray(tr)[:, [0, 2]].copy(), out[1], out[2]))
        return out
    net.predict_batch = predict_batch
    return seen


def _loss64(seen, dev):
    """float64 losses of the recorded batches: lse(ob_pred) - ob_pred[o] + lse(sub_pred) - sub_pred[s] per row."""
    out = []
    for so, sub_pred, ob_pred in seen:
        s, o = (torch.from_numpy(so[:, k]).to(dev) for k in (0, 1))
        rows = torch.arange(len(so), device=dev)
        out.append((torch.logsumexp(ob_pred.double(), 1) - ob_pred.double()[rows, o] +
                    torch.logsumexp(sub_pred.double(), 1) - sub_pred.double()[rows, s]).cpu().numpy())
    return np.concatenate(out)


def test_filtered_stream_with_device_rank_equals_the_torch_tail(dev):
    """evaluate_filter_stream with device_rank on vs off on the same model and stream: the scores come from the same GEMM,
    so every rank is identical; the losses keep the bound of test_row_loss_is_as_accurate_as_softmax_ce (the error of the
    softmax_ce path against float64 on these very score matrices)."""
    import test_gpu_parity as P
    import utils as U
    gold = load_golden('eval_small_100.npz')
    n_eval = int(gold['n_eval'])
    res = {}
    for on in (False, True):
        net, gnet, H, gd, samples, total, valid, va = P._eval_setup(dev, gold)
        net.device_rank = on
        seen = _recorded(net)
        (vs, vst), (vo, vot) = H['valid']
        ranks, loss = net.evaluate_filter_stream(valid[:n_eval], (vs[:n_eval], vst[:n_eval]), (vo[:n_eval], vot[:n_eval]),
                                                 gnet, total)
        assert len(samples) == 0 and (net._filter_index is not None) == on
        res[on] = (ranks, loss, _loss64(seen, dev))
    (r0, l0, ref0), (r1, l1, ref1) = res[False], res[True]
    assert r1.shape == (n_eval, 2) and r1.dtype == np.float64
    print('ranks differing', int((r0 != r1).sum()), 'loss: softmax_ce error', np.abs(l0 - ref0).max(), 'rank_rows error',
          np.abs(l1 - ref1).max())
    assert np.array_equal(r0, r1)
    assert np.array_equal(ref0, ref1)                                      # identical score matrices on both sides
    assert np.abs(l1 - ref1).max() <= np.abs(l0 - ref0).max()
    assert U.rank_metrics(r0) == U.rank_metrics(r1)


def test_lookahead_evaluation_with_device_rank_returns_the_same_ranks(dev):
    """test.py's loop (one evaluate_filter call per quadruple) with lookahead_eval on, device_rank on vs off."""
    import test_gpu_parity as P
    gold = load_golden('eval_small_100.npz')
    n_eval = int(gold['n_eval'])
    out = []
    for on in (False, True):
        net, gnet, H, gd, samples, total, valid, va = P._eval_setup(dev, gold)
        net.lookahead_eval, net.device_rank = True, on
        (vs, vst), (vo, vot) = H['valid']
        with torch.no_grad():
            res = [net.evaluate_filter(valid[i].to(dev), (vs[i], vst[i]), (vo[i], vot[i]), gnet, total) for i in range(n_eval)]
        assert len(samples) == 0 and net._la is not None
        out.append((np.asarray([r for r, _ in res]), np.asarray([float(l) for _, l in res])))
    assert np.array_equal(out[0][0], out[1][0])
    np.testing.assert_allclose(out[1][1], out[0][1], rtol=1e-5, atol=1e-5)


def test_raw_stream_equals_sequential_evaluate_calls(dev):
    """evaluate_stream / evaluate_batch (raw ranks, one batch per timestamp) vs one evaluate() call per quadruple, by the
    criterion of test_evaluate_filter_stream_equals_sequential_calls for batched against one-row scoring."""
    import test_gpu_parity as P
    gold = load_golden('eval_small_100.npz')
    n = 48
    net, gnet, H, gd, samples, total, valid, va = P._eval_setup(dev, gold)
    (vs, vst), (vo, vot) = H['valid']
    with torch.no_grad():
        seq = [net.evaluate(valid[i], (vs[i], vst[i]), (vo[i], vot[i]), gnet) for i in range(n)]
    ranks_seq = np.asarray([r for r, _ in seq])
    loss_seq = np.asarray([float(l) for _, l in seq])
    net2, gnet2, H2, gd2, samples2, total2, valid2, _ = P._eval_setup(dev, gold)
    ranks, loss = net2.evaluate_stream(valid2[:n], (vs[:n], vst[:n]), (vo[:n], vot[:n]), gnet2)
    assert len(samples) == len(samples2) and ranks.shape == (n, 2)
    print('raw stream: ranks identical', float(np.mean(ranks == ranks_seq)), 'largest difference',
          np.abs(ranks - ranks_seq).max(), 'loss difference', np.abs(loss - loss_seq).max())
    np.testing.assert_allclose(loss, loss_seq, rtol=1e-5, atol=1e-5)
    assert float(np.mean(ranks == ranks_seq)) >= 0.99 and np.abs(ranks - ranks_seq).max() <= 1
