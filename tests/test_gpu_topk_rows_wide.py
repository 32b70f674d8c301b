"""GPU tests of renet_topk_rows_wide (run with -m gpu on an MI355X; csrc/topk_rows.hip: the ranked, filtered top-k of rows
that do not fit one CU's LDS, taken in pieces of stage_cols columns and merged per row) against the numpy reference of
tests/test_gpu_topk_rows.py -- exact in index, value and count, logp against a float64 logsumexp: small widths with small
pieces (every seam: ties, lists and k across pieces), constructed rows, real widths with the library's own pieces, the
refusals, and renet_hip.topk_rows' dispatch on the width."""
import numpy as np
import pytest
import torch

from test_gpu_rank_settings import _table
from test_gpu_topk_rows import _assert_logp, _assert_same, _case, _lse64, _reference

pytestmark = pytest.mark.gpu

KS = (1, 10, 1000)
STAGES = (64, 1000, 4096)
# (n, C, ld): the ld of test_gpu_rank.SHAPES where it has the width, else C and C + 5
SEAM_SHAPES = [(3, 70, 70), (3, 70, 75), (8, 257, 257), (8, 4099, 4100), (4, 23033, 23040)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _dev_table(lists, C, seed, dev):
    return tuple(torch.from_numpy(t).to(dev) for t in _table(lists, C, seed))


@pytest.mark.parametrize('logits', ['normal8', 'blocks', 'equal'])
@pytest.mark.parametrize('n,C,ld', SEAM_SHAPES)
def test_small_pieces_equal_the_reference_exactly(dev, n, C, ld, logits):
    """Every list plan, keep, k (1000 > stage_cols = 64: no single piece can supply the answer) and piece width."""
    import renet_hip as K
    scores, label, x, lab, lse, plans = _case(n, C, ld, logits)
    before = scores.clone()
    lab32 = label.int()
    for p, (lists, table) in enumerate(plans):
        for keep in (None, lab32):
            want_all = _reference(x, max(KS), lists, None if keep is None else lab)
            for stage in STAGES:
                for k in KS:
                    got = K.topk_rows_wide(scores, k, *table, keep=keep, stage_cols=stage)
                    want = (want_all[0][:, :k], want_all[1][:, :k], np.minimum(want_all[2], k))
                    idx, val, nv = _assert_same(got, want, '%d x %d (ld %d) %s plan %d keep %s pieces of %d k %d:' %
                                                (n, C, ld, logits, p, keep is not None, stage, k))
                    _assert_logp(got[2].cpu().numpy(), val, nv, lse)
    assert torch.equal(scores, before)


def _run(K, dev, x, k, lists=None, keep=None, stage=64, seed=1, logp=True):
    """The wide entry on the host matrix x against the reference -> (idx, val, n_valid)."""
    table = (None, None, None) if lists is None else _dev_table(lists, x.shape[1], seed, dev)
    got = K.topk_rows_wide(torch.from_numpy(x).to(dev), k, *table, stage_cols=stage,
                           keep=None if keep is None else torch.from_numpy(np.asarray(keep, dtype=np.int32)).to(dev))
    idx, val, nv = _assert_same(got, _reference(x, k, lists, keep), 'constructed k %d:' % k)
    if logp:
        _assert_logp(got[2].cpu().numpy(), val, nv, _lse64(x))
    return idx, val, nv


def test_constructed_rows(dev):
    """C = 300 in pieces of 64 columns (seams at 64, 128, 192, 256)."""
    import renet_hip as K
    C = 300
    rng = np.random.RandomState(11)
    none = np.zeros(0, dtype=np.int64)
    # an all-zero row: the ties cross four seams
    idx, _, _ = _run(K, dev, np.zeros((1, C), dtype=np.float32), 290)
    assert idx[0].tolist() == list(range(290))
    # the k-th value shared by the columns 60..70, across the first seam: the lowest of them
    x = (rng.randn(2, C) * 3).astype(np.float32)
    x[0, 60:71] = 50.0
    x[0, [5, 200, 299]] = 60.0
    idx, _, _ = _run(K, dev, x, 8)
    assert idx[0].tolist() == [5, 200, 299, 60, 61, 62, 63, 64]
    # a list removes the pieces 1 and 2 entirely; keep names a column inside them
    gone = [np.arange(64, 192), none]
    idx, _, nv = _run(K, dev, x, 250, gone)
    assert nv.tolist() == [C - 128, 250] and not np.any((idx[0] >= 64) & (idx[0] < 192))
    x[0, 100] = 70.0
    idx, _, nv = _run(K, dev, x, 250, gone, keep=[100, 100])
    assert nv[0] == C - 127 and idx[0, 0] == 100 and int(((idx[0] >= 64) & (idx[0] < 192)).sum()) == 1
    # fewer than k candidates in all: n_valid and the padding
    few = [np.setdiff1d(np.arange(C), [3, 64, 130, 299]), np.arange(C)]
    idx, val, nv = _run(K, dev, x, 10, few)
    assert nv.tolist() == [4, 0] and sorted(idx[0, :4].tolist()) == [3, 64, 130, 299]
    assert np.all(idx[0, 4:] == -1) and np.all(val[0, 4:] == -np.inf) and np.all(idx[1] == -1)
    # a column listed twice (and a third time in another place) is removed once: the table is built by hand
    cols = torch.tensor([70, 7, 70, 190, 70], dtype=torch.int32, device=dev)
    start = torch.tensor([0, 0], dtype=torch.int32, device=dev)
    count = torch.tensor([5, 0], dtype=torch.int32, device=dev)
    got = K.topk_rows_wide(torch.from_numpy(x).to(dev), 299, cols, start, count, stage_cols=64)
    _assert_same(got, _reference(x, 299, [np.array([70, 7, 190]), none]), 'listed twice:')
    assert got[3].tolist() == [297, 299]
    # a NaN ranks below every number whichever piece holds it (no logp: the row's logsumexp is a NaN)
    x[1, [2, 63, 64, 250]] = np.nan
    x[1, [10, 191]] = -np.inf
    idx, _, _ = _run(K, dev, x, 296, logp=False)
    assert idx[1, 294] == 10 and idx[1, 295] == 191 and not np.isin([2, 63, 64, 250], idx[1, :296]).any()


def test_special_values(dev):
    """The hand-made 4 x 37 matrix of test_gpu_topk_rows.test_special_values, built the same way: signed zeros, -inf
    scores, a list with entries outside the row and the keep column, and an empty range that starts beyond the table."""
    import renet_hip as K
    n, C = 4, 37
    rng = np.random.RandomState(7)
    x = (rng.randn(n, C) * 3).astype(np.float32)
    zeros = [3, 4, 9, 20, 21, 36]
    x[0, zeros] = [0.0, -0.0, -0.0, 0.0, -0.0, 0.0]
    x[1, [0, 5, 6, 17, 36]] = -np.inf
    best = int(np.argsort(-x[2])[0])
    lists = [np.array([3, 20, 30]), np.array([5, 8]), np.array([-1, C + 5, best, 11, 12]), np.zeros(0, dtype=np.int64)]
    cols = np.concatenate(lists + [np.array([1, 2])]).astype(np.int32)
    count = np.array([3, 2, 5, 0], dtype=np.int32)
    start = np.array([0, 3, 5, len(cols) + 7], dtype=np.int32)
    keep = np.array([-1, C + 3, best, 0], dtype=np.int32)
    table = tuple(torch.from_numpy(t).to(dev) for t in (cols, start, count))
    xd = torch.from_numpy(x).to(dev)
    for k in (5, 35, 40):
        for kp in (None, keep):
            got = K.topk_rows_wide(xd, k, *table, keep=None if kp is None else torch.from_numpy(kp).to(dev), stage_cols=64)
            idx, val, nv = _assert_same(got, _reference(x, k, lists, kp), 'special values k %d keep %s:' % (k, kp is not None))
            _assert_logp(got[2].cpu().numpy(), val, nv, _lse64(x))
            assert nv.tolist() == [min(k, 34), min(k, 35), min(k, 34 + (kp is not None)), min(k, 37)]
            assert np.all((idx >= 0) == (np.arange(k)[None, :] < nv[:, None])) and np.all(idx < C)
            if k >= 35:
                assert [c for c in idx[0].tolist() if c in zeros] == [4, 9, 21, 36]
                assert np.all(val[0][np.isin(idx[0], zeros)] == 0.0) and not np.any(np.signbit(val[0][np.isin(idx[0], zeros)]))


@pytest.mark.parametrize('pad', [0, 5])
@pytest.mark.parametrize('C', [32769, 65537, 100003])
def test_real_widths(dev, C, pad):
    """The library's own pieces; ld = C is odd, so the rows -- and the pieces -- start at every 4-byte alignment."""
    import renet_hip as K
    n = 3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, C, generator=g) * 8
    buf = torch.full((n, C + pad), 3e38)
    buf[:, :C] = x
    xd = buf.to(dev)[:, :C]
    before = xd.clone()
    x = x.numpy()
    lists = [np.arange(0, C, 3), np.arange(32768, C), np.zeros(0, dtype=np.int64)]
    table = _dev_table(lists, C, 3, dev)
    want_all = _reference(x, 1024, lists)
    for k in (1, 10, 1024):
        got = K.topk_rows_wide(xd, k, *table)
        want = (want_all[0][:, :k], want_all[1][:, :k], np.minimum(want_all[2], k))
        idx, val, nv = _assert_same(got, want, 'C = %d ld %d k %d:' % (C, C + pad, k))
        _assert_logp(got[2].cpu().numpy(), val, nv, _lse64(x))
    assert torch.equal(xd, before)


@pytest.mark.parametrize('stage', [0, 32768])
def test_equal_maxima_across_column_32768(dev, stage):
    """40 equal maxima in the columns 32750..32789: the ten lowest, also where a seam lies at 32768."""
    import renet_hip as K
    C = 65537
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(1, C, generator=g) * 8).numpy()
    x[0, 32750:32790] = 100.0
    idx, _, _ = _run(K, dev, x, 10, stage=stage)
    assert idx[0].tolist() == list(range(32750, 32760))


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
    need = L.renet_topk_rows_wide_workspace(4, 8, 3, 0)
    assert need == 4 * (3 * 8 + 24)
    ws = torch.zeros(need // 8, device=dev, dtype=torch.int64)

    def call(n=4, C=8, ld=8, k=3, lst=(None, None, None, 0), stage=0, out=idx, w=ws, wbytes=need):
        return L.renet_topk_rows_wide(p(s), ld, n, C, k, p(lst[0]), p(lst[1]), p(lst[2]), lst[3], None, p(out), p(val),
                                      p(logp), p(nv), stage, p(w), wbytes, K._stream())
    assert call(k=0) == -1 and call(k=1025) == -1 and call(ld=7) == -1 and call(n=-1) == -1 and call(C=0) == -1
    for bad in ((cols, rng, None, 16), (None, rng, rng, 0), (cols, None, rng, 16), (cols, rng, rng, -1)):
        assert call(lst=bad) == -1
    assert call(out=None) == -1
    assert call(stage=63) == -1 and call(stage=32769) == -1 and call(stage=-1) == -1
    assert call(wbytes=need - 1) == -3 and call(w=None) == -3                   # RENET_ERR_WORKSPACE
    assert call(n=0) == 0 and call(n=0, w=None, wbytes=0) == 0                  # no-op: nothing launched, nothing written
    wide = K.TOPK_ROWS_WIDE_MAX_C
    assert wide >= 1 << 20
    assert call(n=0, C=wide + 1, ld=wide + 1) == -2 and call(n=0, C=wide, ld=wide) == 0
    assert L.renet_topk_rows_wide_workspace(4, wide + 1, 3, 0) == 0 and L.renet_topk_rows_wide_workspace(4, 8, 3, 63) == 0
    torch.cuda.synchronize()
    assert idx.eq(7).all() and val.eq(7).all() and logp.eq(7).all() and nv.eq(7).all()
    # the all-zero rows tie in every column: the lowest columns, each with probability 1 / 8 (stage_cols 0 and 64 alike)
    for stage in (0, 64):
        idx.fill_(7)
        assert call(stage=stage) == 0
        assert idx.tolist() == [[0, 1, 2]] * 4 and val.eq(0).all() and nv.tolist() == [3] * 4
        np.testing.assert_allclose(logp.cpu().numpy(), -np.log(8.0), rtol=1e-6)
    # a range is cut to the length given for its table, as the narrow entry cuts it
    start = torch.tensor([0, 0, 1, -3], device=dev, dtype=torch.int32)
    count = torch.tensor([100, 0, 100, 4], device=dev, dtype=torch.int32)
    assert call(lst=(cols, start, count, 2)) == 0
    assert idx.tolist() == [[2, 3, 4], [0, 1, 2], [0, 2, 3], [1, 2, 3]]
    with pytest.raises(K.RenetHipError):
        K.topk_rows_wide(s.double(), 3)
    with pytest.raises(K.RenetHipError):
        K.topk_rows_wide(s, 3, cols, rng, None)
    with pytest.raises(K.RenetHipError):
        K.topk_rows_wide(s, 3, stage_cols=63)


def test_topk_rows_serves_a_row_of_40000_columns(dev):
    """renet_hip.topk_rows dispatches on the width (before the wide entry: RenetHipError, RENET_ERR_UNSUPPORTED)."""
    import renet_hip as K
    n, C = 3, 40000
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, C, generator=g) * 8
    lists = [np.arange(0, C, 3), np.arange(32768, C), np.zeros(0, dtype=np.int64)]
    got = K.topk_rows(x.to(dev), 10, *_dev_table(lists, C, 3, dev))
    idx, val, nv = _assert_same(got, _reference(x.numpy(), 10, lists), 'C = 40000 through topk_rows:')
    _assert_logp(got[2].cpu().numpy(), val, nv, _lse64(x.numpy()))
