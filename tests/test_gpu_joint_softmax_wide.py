"""GPU tests of renet_joint_softmax on rows that do not fit LDS (run with -m gpu on an MI355X; csrc/topk.hip,
joint_softmax_stream_kernel: an online max / sum sweep, then a second sweep that writes) and of the fused paths of model.py
that it now serves at every width.  The bound is measured: the kernel may be 4 times as far from the float64 expression as
the reference's own fp32 torch ops on the CPU are (the margin this project gives a different reduction order, as
tests/test_gpu_nbr_aggregators.py states it), plus one fp32 rounding."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_TOP = 100


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _rel_err(got, want):
    return float((np.abs(got.astype(np.float64) - want) / want).max())


@functools.lru_cache(maxsize=None)
def _expression(n, R, N):
    """Seeded inputs -> (logits [n * R, N], logits_r [n, R], prob [n]) as CPU tensors, the joint [n, R * N] in float64 numpy,
    and e_ref: the largest relative error of the reference's fp32 torch ops on the CPU against it."""
    g = torch.Generator().manual_seed(4 + N)
    logits = torch.randn(n * R, N, generator=g) * 3
    lr = torch.randn(n, R, generator=g) * 2
    prob = torch.rand(n, generator=g) * 1e-3 + 1e-5
    joint = (_softmax64(logits.numpy()) * _softmax64(lr.numpy()).reshape(n * R, 1)).reshape(n, R * N) * \
        prob.numpy().astype(np.float64).reshape(n, 1)
    cpu = (torch.softmax(logits, dim=1) * torch.softmax(lr, dim=1).reshape(n * R, 1)).view(n, R * N) * prob.view(n, 1)
    return logits, lr, prob, joint, _rel_err(cpu.numpy(), joint)


@pytest.mark.parametrize('n,R,N', [(2, 3, 32769), (2, 3, 50001)])
def test_streamed_rows_match_the_float64_expression(dev, n, R, N):
    import renet_hip as K
    logits, lr, prob, joint, e_ref = _expression(n, R, N)
    mine = logits.to(dev)
    assert K.joint_softmax(mine, R, lr.to(dev), prob.to(dev)) is mine
    e_mine = _rel_err(mine.cpu().numpy().reshape(n, R * N), joint)
    bound = 4 * e_ref + 2.0 ** -23
    print('joint_softmax N = %d: fp32 CPU reference error %.3e, kernel error %.3e, allowed %.3e' % (N, e_ref, e_mine, bound))
    assert e_mine <= bound
    vals, idx = K.topk_positive(mine.view(n, R * N), K_TOP)
    ri = torch.topk(torch.from_numpy(joint), K_TOP, dim=1).indices
    same = [len(set(idx[i].tolist()) & set(ri[i].tolist())) for i in range(n)]
    assert min(same) >= K_TOP - 1, same                          # identical sets up to a near-tie at the boundary
    assert torch.equal(vals, mine.view(n, R * N).gather(1, idx))


def test_scaled_softmax_topk_on_a_wide_block(dev, monkeypatch):
    """model._scaled_softmax_topk on a [5, 40000] block: the fused branch (before: the torch expression, as the row exceeds
    LDS) against the float64 expression within the same bound, and against the torch branch on the same GPU."""
    import model as M
    rows, N, k = 5, 40000, K_TOP
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(rows, N, generator=g) * 3
    scale = torch.rand(rows, generator=g) * 1e-2 + 1e-4
    joint = (_softmax64(logits.numpy()) * scale.numpy().astype(np.float64).reshape(rows, 1)).reshape(-1)
    e_ref = _rel_err((torch.softmax(logits, dim=1) * scale.view(rows, 1)).numpy().reshape(-1), joint)
    bound = 4 * e_ref + 2.0 ** -23
    called = []
    import renet_hip as K
    inner = K.joint_softmax
    monkeypatch.setattr(K, 'joint_softmax', lambda *a: called.append(1) or inner(*a))
    monkeypatch.delenv('RENET_TOPK', raising=False)
    vals, idx = M._scaled_softmax_topk(logits.to(dev), scale.to(dev), k)
    assert called == [1]                                         # the fused branch
    monkeypatch.setenv('RENET_TOPK', 'torch')
    tv, ti = M._scaled_softmax_topk(logits.to(dev), scale.to(dev), k)
    assert called == [1]
    vals, idx, tv, ti = vals.cpu().numpy(), idx.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy()
    e_mine, e_torch = _rel_err(vals, joint[idx]), _rel_err(tv, joint[ti])
    print('scaled softmax top-k: fp32 CPU reference error %.3e, fused %.3e, torch branch %.3e, allowed %.3e'
          % (e_ref, e_mine, e_torch, bound))
    assert e_mine <= bound
    want = np.argsort(-joint, kind='stable')[:k]
    assert len(set(idx.tolist()) & set(want.tolist())) >= k - 1 and len(set(idx.tolist()) & set(ti.tolist())) >= k - 1
    # the entries both branches chose, value by value: each branch within its own error of the float64 value
    mine, theirs = dict(zip(idx.tolist(), vals.astype(np.float64))), dict(zip(ti.tolist(), tv.astype(np.float64)))
    both = sorted(set(mine) & set(theirs))
    assert all(abs(mine[c] - theirs[c]) <= (bound + e_torch) * joint[c] for c in both)
