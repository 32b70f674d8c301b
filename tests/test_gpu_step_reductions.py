"""The part RENET_STEP_BATCH bit 16 adds to the C launch list (csrc/step.cpp) against what it replaces, bit for bit:

  the head's weight planes  packed by the list == renet_hip.pack_planes byte for byte; a step without an optimizer update
                            in front of it packs nothing
  the whole step            child processes: RENET_STEP_BATCH = 6 against 22 (= 6 + 16, the default): losses equal, flat
                            gradients and parameters of 2 optimizer steps torch.equal
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


# ---------------------------------------------------------------------------------------------
# the head's weight planes, packed by the list
# ---------------------------------------------------------------------------------------------
def test_list_packs_stale_weight_planes_and_only_those(dev):
    """Three steps on one batch: the first two follow an optimizer update (the first the registration), the third none.
    With bit 16 of RENET_STEP_BATCH (the default) the forward list of a step behind an update counts one launch more -- its own
    renet_pack_planes -- and the planes it leaves in the cache equal renet_hip.pack_planes(weight) byte for byte; the step
    without an update in front of it packs nothing."""
    import model as M
    import parallel
    import renet_hip as K
    import step_plan
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import step_reductions_run as C
    packs = 1 if K.lib().renet_step_batch_mask() & 16 else 0          # (a process started with the bit off: Python packs)
    quads, num_ent, num_rels, gd, hs, ho = C.small_stream()
    old = K.PLANES_MIN_CLASSES
    K.PLANES_MIN_CLASSES = 256
    try:
        torch.manual_seed(7)
        net = M.RENet(num_ent, 100, num_rels, dropout=0.0, seq_len=10, num_k=10)
        gen = torch.Generator().manual_seed(3)
        net.global_emb = {int(t): torch.randn(1, 1, 100, generator=gen) * 0.1 for t in gd}
        net.to(dev).train()
        opt = parallel.HipAdam(net, lr=1e-3, weight_decay=1e-5, max_norm=1.0)
        idx = np.random.RandomState(1).permutation(len(quads))[:48]
        prep = net.prepare_both(quads[idx], hs.take(idx), ho.take(idx), gd)
        w = net.linear.weight
        assert K.use_planes(w, w.shape[0])
        fwd = []
        for update in (True, False, True):                                # (the third step follows no update)
            with opt.step_scope(head_passes=1):
                loss = net.loss_prepared_both(prep)
                assert 'StepFn' in type(loss.grad_fn).__name__
                fwd.append(step_plan.StepFn.last_launches[0])
                mine, stale = K.weight_planes_or_buffer(w.detach())
                assert not stale, 'the list must leave the cache current'
                torch.cuda.synchronize()
                assert torch.equal(mine.p.view(torch.int16), K.pack_planes(w.detach()).p.view(torch.int16))
                loss.backward()
                if update:
                    opt.step()
                else:
                    opt.sync_grads()
        torch.cuda.synchronize()
        assert fwd[0] == fwd[1] == fwd[2] + packs, fwd
        opt.close()
    finally:
        K.PLANES_MIN_CLASSES = old


# ---------------------------------------------------------------------------------------------
# the whole step: RENET_STEP_BATCH = 6 against 22
# ---------------------------------------------------------------------------------------------
CONFIGS = ['%d:%d:%d' % (h, s, p) for h in (100, 200) for s in (2, 1) for p in (0, 50)]       # hidden:streams:dropout %
_runs = {}


def _step_run(mask, tmp_path_factory):
    if mask not in _runs:
        out = str(tmp_path_factory.mktemp('step_reductions') / ('mask%d.pt' % mask))
        env = dict(os.environ, RENET_STEP_BATCH=str(mask))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'step_reductions_run.py'), out] + CONFIGS, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (mask, r.stdout[-2000:], r.stderr[-4000:])
        _runs[mask] = torch.load(out)
    return _runs[mask]


@pytest.mark.parametrize('mask', [6 | 16])
def test_whole_step_is_bit_identical_to_the_list_without_the_new_parts(dev, mask, tmp_path_factory):
    """300 entities, 48 quadruples, 2 optimizer steps; n_hidden 100 and 200, dropout 0 and 0.5, two streams and one.  The new
    part really ran, by the launch counts of the last step: bit 16 adds the pack to the forward list (every step follows an
    optimizer update); the backward list is the same."""
    base, new = _step_run(6, tmp_path_factory), _step_run(mask, tmp_path_factory)
    assert set(new) == set(base) == set(CONFIGS)
    for c in CONFIGS:
        (l0, f0, p0, n0), (l1, f1, p1, n1) = base[c], new[c]
        assert l0 == l1, (c, l0, l1)
        assert len(f0) == len(f1) == 2
        for x, y in zip(f0, f1):
            assert float(x.abs().max()) > 0
            assert torch.equal(x, y), c
        assert torch.equal(p0, p1), c
        assert n1[0] == n0[0] + (1 if mask & 16 else 0), (c, n0, n1)
        assert n1[1] == n0[1], (c, n0, n1)
