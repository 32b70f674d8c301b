"""GPU tests of renet_soft_ce_sparse (csrc/soft_ce.hip; renet_hip.soft_ce_sparse) against a numpy float64 statement written
here, with error bounds derived from the kernel's arithmetic the way test_gpu_rowwise._softmax_fp64 derives its own.

Per row, with W = sum_k w_k, p = softmax(x), m = max x, lse = m + ln sum exp(x - m), n = the row's target count and
d = ceil(n / 256) + 9 (the additions on the path of one term of a target sum -- a thread's serial terms, six butterfly
steps, two adds of the four partials -- plus the rounding of its product):

  loss = W lse - sum_k w_k x_k.  lse is computed exactly as renet_softmax_ce computes it, so its error is at most
    (|m| + ln C + 32) 2^-23 (that test's bound without the target logit); W and the weighted sum each carry a relative error
    of at most d 2^-24 of their absolute sums; the product and the difference round once each.  Bound:
    ( W (|m| + ln C + 32) + (d + 1) / 2 (W |lse| + sum_k w_k |x_k|) ) 2^-23.

  grad_c = grad_scale (W p_c - w_c).  p_c is renet_softmax_ce's (error p (|x - m| + 32) 2^-23, which already holds the
    roundings of the products around it), W adds d 2^-24 relative, the difference and the scaling round once each
    (<= (W p + w_c) 2^-23 together), and a p flushed to zero costs less than W 2^-126.  Bound:
    grad_scale ( W p_c (|x_c - m| + 32 + d / 2) 2^-23 + w_c 2^-23 + max(W, 1) 2^-126 ).

With a single target of weight 1 the kernel must ALSO meet renet_softmax_ce's own bounds (_softmax_fp64) on the same row.
Every test prints the worst observed error-to-bound ratio (`pytest -s`; recorded in profiles/online_learning.md)."""
import math

import numpy as np
import pytest
import torch

from test_gpu_rowwise import U23, _assert_bits, _np, _report, _softmax_fp64, _to

pytestmark = pytest.mark.gpu

B_ROWS = 6
WIDTHS = (1, 2, 63, 257, 4097, 23033, 40000)
FAMILIES = ('plain', 'neginf', 'strided')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _edges(c):
    return sorted({j for j in (0, 511, 512, c - 2, c - 1) if 0 <= j < c})


def _csr(rows):
    """rows: list of (ascending int columns, float32 weights) -> ptr int32 [B + 1], col int32, w float32."""
    ptr = np.concatenate(([0], np.cumsum([len(c) for c, _ in rows]))).astype(np.int32)
    col = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows]) if rows else np.zeros(0, np.int32)
    w = np.concatenate([np.asarray(v, dtype=np.float32) for _, v in rows]) if rows else np.zeros(0, np.float32)
    return ptr, col, w


def _weights(rng, n, counts):
    """n weights: raw integer counts (W >> 1), or normalised to sum 1 (to fp32 rounding)."""
    if counts:
        return rng.randint(1, 60, n).astype(np.float32)
    v = rng.rand(n) + 0.05
    return (v / v.sum()).astype(np.float32)


def _patterns(c, rng, counts):
    """Two batches of B_ROWS target rows: (1) empty, then ONE column per row at the edge columns 0, 511, 512, C - 2, C - 1
    (those the row has, repeated cyclically); (2) every column (C <= 257) or ~1000 random columns that include the edge
    columns (C >= 4097), an empty row in the middle."""
    e = _edges(c)
    single = [((), ())] + [((e[k % len(e)],), _weights(rng, 1, counts)) for k in range(B_ROWS - 1)]
    many = []
    for k in range(B_ROWS):
        if k == 3:
            many.append(((), ()))
            continue
        if c <= 257:
            cols = np.arange(c)
        else:
            cols = np.union1d(rng.choice(c, 1000 - 7 * k, replace=False), e if k % 2 == 0 else e[:1])
        many.append((cols, _weights(rng, len(cols), counts)))
    return [single, many]


def _logits(c, rng, family, rows):
    """2 randn with +12 on one edge column per row; neginf: two -inf per row outside the row's targets (as far as the row has
    columns left)."""
    x = (2.0 * rng.randn(B_ROWS, c)).astype(np.float32)
    e = _edges(c)
    for b in range(B_ROWS):
        x[b, e[b % len(e)]] += np.float32(12.0)
    if family == 'neginf':
        for b in range(B_ROWS):
            free = np.setdiff1d(np.arange(c), np.asarray(rows[b][0], dtype=np.int64))
            x[b, free[np.linspace(0, len(free) - 1, 2).astype(np.int64)] if len(free) >= 2 else free] = -np.inf
            if not np.isfinite(x[b]).any():                  # (C <= 2 with no target: keep the row's maximum finite)
                x[b, 0] = np.float32(0.5)
    return x


def _fp64(x, rows, grad_scale):
    """float64 statement -> loss, gradient and the bounds of the module docstring."""
    x64 = x.astype(np.float64)
    b, c = x64.shape
    m = x64.max(axis=1, keepdims=True)
    with np.errstate(invalid='ignore'):
        z = x64 - m
    e = np.exp(z)
    ssum = e.sum(axis=1, keepdims=True)
    p = e / ssum
    lse = np.log(ssum[:, 0]) + m[:, 0]
    absz = np.where(p > 0, np.abs(z), 0.0)
    loss, loss_tol = np.zeros(b), np.zeros(b)
    grad, grad_tol = np.zeros((b, c)), np.zeros((b, c))
    for i, (cols, w) in enumerate(rows):
        cols, w = np.asarray(cols, dtype=np.int64), np.asarray(w, dtype=np.float64)
        if len(cols) == 0:
            continue                                         # loss 0, gradient 0, both exact
        d = math.ceil(len(cols) / 256.0) + 9
        W, xk = w.sum(), x64[i, cols]
        loss[i] = W * lse[i] - (w * xk).sum()
        loss_tol[i] = (W * (abs(m[i, 0]) + math.log(c) + 32.0) + (d + 1) / 2.0 * (W * abs(lse[i]) + (w * np.abs(xk)).sum())) * U23
        wd = np.zeros(c)
        wd[cols] = w
        grad[i] = grad_scale * (W * p[i] - wd)
        grad_tol[i] = grad_scale * (W * p[i] * (absz[i] + 32.0 + d / 2.0) * U23 + wd * U23 + max(W, 1.0) * 2.0 ** -126)
    return loss, grad, loss_tol, grad_tol


def _device_targets(rows, dev):
    ptr, col, w = _csr(rows)
    return _to(ptr, dev), _to(col, dev), _to(w, dev)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('c', WIDTHS)
def test_soft_ce_sparse_matches_fp64(dev, c, family):
    import renet_hip as K
    rng = np.random.RandomState(c * 13 + len(family))
    worst_loss = worst_grad = 0.0
    n_inf = 0
    for counts in (False, True):
        for rows in _patterns(c, rng, counts):
            x = _logits(c, rng, family, rows)
            ptr, col, w = _device_targets(rows, dev)
            empty = np.asarray([len(r[0]) == 0 for r in rows])
            for gs in (1.0, 1.0 / 2048):
                loss_ref, grad_ref, loss_tol, grad_tol = _fp64(x, rows, gs)
                assert np.isfinite(loss_ref).all()
                if family == 'strided':                      # a view of a buffer with ld = C + 5, +inf beside every row
                    buf = torch.full((B_ROWS, c + 5), float('inf'), device=dev)
                    lg = buf[:, :c]
                    lg.copy_(_to(x, dev))
                    assert lg.stride(0) == c + 5
                else:
                    lg = _to(x, dev)
                # loss only: the logits stay as they are
                loss0 = K.soft_ce_sparse(lg, ptr, col, w, gs, False)
                _assert_bits(_np(lg), x, 'logits after a loss-only call')
                # in place: the same loss bits
                loss = K.soft_ce_sparse(lg, ptr, col, w, gs, True)
                assert torch.equal(loss, loss0)
                got_loss, got = _np(loss).astype(np.float64), _np(lg).astype(np.float64)
                assert np.isfinite(got_loss).all() and np.isfinite(got).all()
                # an empty row: loss 0 and a zero gradient, exactly
                assert (got_loss[empty] == 0).all() and not got[empty].any()
                if family == 'neginf':
                    n_inf += int(np.isneginf(x).sum())
                    assert (got[np.isneginf(x)] == 0).all()
                if family == 'strided':
                    assert bool(torch.isposinf(buf[:, c:]).all())
                # a second run, on a contiguous copy: identical bits
                again = _to(x, dev)
                assert torch.equal(K.soft_ce_sparse(again, ptr, col, w, gs, True), loss) and torch.equal(again, lg)
                live = ~empty
                le = np.abs(got_loss - loss_ref)[live] / loss_tol[live]
                ge = np.abs(got - grad_ref)[live] / grad_tol[live]
                worst_loss, worst_grad = max(worst_loss, float(le.max())), max(worst_grad, float(ge.max()))
                assert (le <= 1).all(), ('loss', c, family, counts, gs, got_loss, loss_ref, float(le.max()))
                assert (ge <= 1).all(), ('gradient', c, family, counts, gs, float(ge.max()),
                                         np.unravel_index(ge.argmax(), ge.shape))
    assert family != 'neginf' or c <= 2 or n_inf >= 8 * B_ROWS       # (two per row wherever a row has columns left)
    _report('soft_ce_sparse C=%d %s: loss' % (c, family), worst_loss)
    _report('soft_ce_sparse C=%d %s: gradient' % (c, family), worst_grad)


@pytest.mark.parametrize('c', WIDTHS)
def test_one_target_of_weight_one_meets_the_bounds_of_softmax_ce(dev, c):
    """A single target of weight 1 is the hard-target cross-entropy: loss and gradient within renet_softmax_ce's OWN float64
    bounds (test_gpu_rowwise._softmax_fp64) on the same rows, the targets running over the edge columns."""
    import renet_hip as K
    rng = np.random.RandomState(c + 5)
    e = _edges(c)
    t = np.asarray([e[k % len(e)] for k in range(B_ROWS)], dtype=np.int32)
    rows = [((int(j),), (1.0,)) for j in t]
    x = _logits(c, rng, 'plain', rows)
    ptr, col, w = _device_targets(rows, dev)
    worst_loss = worst_grad = 0.0
    for gs in (1.0, 1.0 / 2048):
        loss_ref, grad_ref, loss_tol, grad_tol, _ = _softmax_fp64(x, t, gs)
        lg = _to(x, dev)
        loss = K.soft_ce_sparse(lg, ptr, col, w, gs, True)
        le = np.abs(_np(loss).astype(np.float64) - loss_ref) / loss_tol
        ge = np.abs(_np(lg).astype(np.float64) - grad_ref) / grad_tol
        worst_loss, worst_grad = max(worst_loss, float(le.max())), max(worst_grad, float(ge.max()))
        assert (le <= 1).all() and (ge <= 1).all(), (c, gs, float(le.max()), float(ge.max()))
    _report('soft_ce_sparse C=%d one target: loss' % c, worst_loss)
    _report('soft_ce_sparse C=%d one target: gradient' % c, worst_grad)


def test_autograd_function_hands_the_gradient_to_linear(dev):
    """ops.SoftCESparseFn behind ops.LinearFn: the loss is scale * sum(row losses) and the parameter gradients are LinearFn's
    products of the kernel's dlogits -- against torch autograd in float64 on the dense targets, relative L2 <= 4e-5 (the
    fp32-class GEMM parity figure of the step tests), loss <= 1e-5."""
    import ops
    rng = np.random.RandomState(3)
    b, h, c = 5, 100, 300
    xs = rng.randn(b, h).astype(np.float32)
    wt, bias = (0.1 * rng.randn(c, h)).astype(np.float32), (0.1 * rng.randn(c)).astype(np.float32)
    rows = [(np.sort(rng.choice(c, 20, replace=False)), _weights(rng, 20, False)) for _ in range(b)]
    rows[2] = ((), ())
    ptr, col, w = _csr(rows)
    tg = ops.SparseTargets(ptr, col, w, c, dev)
    leaves = [_to(a, dev).requires_grad_(True) for a in (xs, wt, bias)]
    loss = ops.SoftCESparseFn.apply(ops.LinearFn.apply(*leaves), tg, 1.0 / b)
    (2.0 * loss).backward()
    ref = [torch.from_numpy(a).double().requires_grad_(True) for a in (xs, wt, bias)]
    dense = np.zeros((b, c))
    for i, (cols, v) in enumerate(rows):
        dense[i, np.asarray(cols, dtype=np.int64)] = np.asarray(v, dtype=np.float64)
    logp = torch.log_softmax(ref[0] @ ref[1].t() + ref[2], dim=1)
    want = torch.mean(torch.sum(-torch.from_numpy(dense) * logp, 1))
    (2.0 * want).backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    for got, r in zip(leaves, ref):
        err = float((got.grad.double().cpu() - r.grad).norm() / r.grad.norm())
        print('  relative L2 of a gradient', tuple(r.shape), err)
        assert err <= 4e-5
    with pytest.raises(ValueError):
        ops.SparseTargets([0, 2], [3, 3], [0.5, 0.5], c, dev)               # a repeated column
