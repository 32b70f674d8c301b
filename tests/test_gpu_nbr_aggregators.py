"""MeanAggregator / AttnAggregator on the device (csrc/nbr_pool.hip behind ops.NbrPoolFn) against
  (a) a float64 restatement of Aggregator.py:249-285 / 316-346, with a tolerance MEASURED here: 4 x the error that the
      reference's own float32 arithmetic (the same restatement run by torch on the CPU in float32) has against float64 on
      the same inputs -- a different but equally valid summation order may land anywhere within a small multiple of it.
      The bound is the error of fp32 arithmetic, so these tests put the GEMM front in its exact-fp32 mode ('f32'); the
      error in the process default mode is printed next to it;
  (b) the fixtures the unmodified reference classes produced (tests/golden/nbr_agg_*.npz, tools/make_golden_nbr.py), with
      the tolerances tests/test_gpu_parity.py uses for the RGCN encoder against its fixtures.
"""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import fixtures, load_golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 2e-5                      # tests/test_gpu_parity.py: encoder internals against the fixtures
GRAD_RTOL, GRAD_ATOL = 2e-3, 3e-5            # ... and its gradients
NUM_ENT, NUM_RELS, NAMED = 500, 7, 480       # entities >= NAMED appear in no list and as no subject
SEG_LENS = [1, 2, 63, 64, 65, 256, 257, 1000]
KINDS = ('mean', 'gcn', 'attn')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _make(kind, d, dropout=0.0, seq_len=4):
    from Aggregator import MeanAggregator, AttnAggregator
    if kind == 'attn':
        return AttnAggregator(d, dropout, seq_len=seq_len)
    return MeanAggregator(d, dropout, seq_len=seq_len, gcn=(kind == 'gcn'))


_cases = {}


def _case(d):
    """One batch per D, shared by the tests: 10 sequences x 4 steps = 40 segments; the lengths of SEG_LENS (every path
    of the kernel: one / two 64-neighbour rounds, the split threshold 256 | 257, a long list) and 32 short random ones;
    ids repeat inside and across segments (1000 draws from 480 ids)."""
    if d not in _cases:
        rng = np.random.RandomState(4000 + d)
        lens = SEG_LENS + rng.randint(1, 13, size=32).tolist()
        rng.shuffle(lens)
        steps = [rng.randint(0, NAMED, size=n).astype(np.int64) for n in lens]
        hist = [steps[4 * i:4 * i + 4] for i in range(10)]
        s = rng.randint(0, NAMED, size=10).astype(np.int64)
        r = rng.randint(0, NUM_RELS, size=10).astype(np.int64)
        emb = fixtures.make_params(5000 + d, {'ent': (NUM_ENT, d), 'rel': (NUM_RELS, d), 'C': (40, 3 * d)}, scale=0.5)
        _cases[d] = dict(hist=hist, s=s, r=r, ent=emb['ent'], rel=emb['rel'], C=emb['C'])
    return _cases[d]


def _restated(kind, params, hist, s, r, ent, rel, nb):
    """Aggregator.py:249-285 / 316-346 (eval mode) in the dtype of `ent`, rows in the packed order of `nb`."""
    rows = []
    for i in range(nb.nseq):
        o = int(nb.perm[i])
        es = ent[int(s[o])]
        for ids in hist[o]:
            em = ent[torch.as_tensor(ids)]
            n = len(ids)
            if kind == 'attn':
                rr = rel[int(r[o])]
                x = torch.cat((em, es.repeat(n, 1), rr.repeat(n, 1)), dim=1)                       # :333
                w = F.softmax(torch.tanh(x @ params['attn_s.weight'].t() + params['attn_s.bias']) @ params['v_s'], dim=0)
                rows.append(torch.cat((torch.sum(w * em, dim=0), es, rr)))                       # :337-340
            else:
                m = em.sum(0) / n                                                                 # :266-267
                if kind == 'gcn':
                    m = F.relu(params['gcn_layer.weight'] @ m + params['gcn_layer.bias'])         # :270-271
                rows.append(torch.cat((m, es)))
    seq_major = torch.stack(rows)
    return seq_major[torch.as_tensor(np.argsort(nb.out_row))]


def _reference_run(kind, agg, c, nb, dtype, width):
    """-> (packed data, {name: gradient of sum(data * C)}) of the restatement on the CPU in `dtype`."""
    params = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in agg.named_parameters()}
    ent = torch.from_numpy(c['ent']).to(dtype).requires_grad_(True)
    rel = torch.from_numpy(c['rel']).to(dtype).requires_grad_(True)
    out = _restated(kind, params, c['hist'], c['s'], c['r'], ent, rel, nb)
    (out * torch.from_numpy(c['C'][:, :width]).to(dtype)).sum().backward()
    grads = {k: p.grad for k, p in params.items()}
    grads['ent'] = ent.grad
    if kind == 'attn':
        grads['rel'] = rel.grad
    return out.detach(), grads


def _device_run(agg, c, dev, width, mode):
    import renet_hip as K
    ent = torch.from_numpy(c['ent']).to(dev).requires_grad_(True)
    rel = torch.from_numpy(c['rel']).to(dev).requires_grad_(True)
    for p in agg.parameters():
        p.grad = None
    with K.gemm_mode(mode):
        packed = agg(c['hist'], torch.from_numpy(c['s']), torch.from_numpy(c['r']), ent, rel)
        (packed.data * torch.from_numpy(c['C'][:, :width]).to(dev)).sum().backward()
    grads = {k: p.grad.detach().cpu() for k, p in agg.named_parameters()}
    grads['ent'] = ent.grad.cpu()
    if rel.grad is not None:
        grads['rel'] = rel.grad.cpu()
    return packed, grads


_runs = {}


def _runs_of(kind, d, dev, v_scale=1.0):
    """The device result (exact-fp32 GEMM mode and process default) and the float64 / float32 references, computed once
    per (kind, D) and shared by the forward and the backward test."""
    key = (kind, d, v_scale)
    if key not in _runs:
        torch.manual_seed(100 + d)
        agg = _make(kind, d)
        if v_scale != 1.0:
            with torch.no_grad():
                agg.v_s.mul_(v_scale)
        agg.to(dev).eval()
        c = _case(d)
        width = (3 if kind == 'attn' else 2) * d
        packed, grads = _device_run(agg, c, dev, width, 'f32')
        nb = agg.last_batch.host
        packed_dflt, _ = _device_run(agg, c, dev, width, None)
        assert packed.batch_sizes.tolist() == [10, 10, 10, 10]
        ref64 = _reference_run(kind, agg, c, nb, torch.float64, width)
        ref32 = _reference_run(kind, agg, c, nb, torch.float32, width)
        _runs[key] = dict(out=packed.data.detach().cpu(), out_dflt=packed_dflt.data.detach().cpu(), grads=grads,
                          ref64=ref64, ref32=ref32, nb=nb, d=d)
    return _runs[key]


def _err(a, ref64):
    return float((a.double() - ref64).abs().max())


def _check_forward(kind, d, run):
    out64 = run['ref64'][0]
    e_ref, e_mine, e_dflt = _err(run['ref32'][0], out64), _err(run['out'], out64), _err(run['out_dflt'], out64)
    print('%s D=%d forward: fp32 reference error %.3e, kernel error %.3e (default GEMM mode %.3e), allowed %.3e'
          % (kind, d, e_ref, e_mine, e_dflt, 4 * e_ref))
    assert e_ref > 0
    assert e_mine <= 4 * e_ref
    # the copied column blocks E[s] (| R[r]) are exact
    assert torch.equal(run['out'][:, d:], out64[:, d:].float())


@pytest.mark.parametrize('d', [100, 200, 300, 400])
@pytest.mark.parametrize('kind', ['mean', 'attn'])
def test_forward_against_float64(dev, kind, d):
    _check_forward(kind, d, _runs_of(kind, d, dev))


def _largest_score(params, c, d, v_scale):
    """max |a_j| over the batch, in float64."""
    ent, rel = torch.from_numpy(c['ent']).double(), torch.from_numpy(c['rel']).double()
    w, b, v = (params[k].detach().cpu().double() for k in ('attn_s.weight', 'attn_s.bias', 'v_s'))
    top = 0.0
    for o in range(len(c['s'])):
        q = w[:, d:2 * d] @ ent[int(c['s'][o])] + w[:, 2 * d:] @ rel[int(c['r'][o])] + b
        for ids in c['hist'][o]:
            a = torch.tanh(ent[torch.as_tensor(ids)] @ w[:, :d].t() + q) @ (v * v_scale)
            top = max(top, float(a.abs().max()))
    return top


def test_forward_running_maximum_with_large_scores(dev):
    """v scaled so that |a_j| reaches about 60: sums of exp(a_j) would overflow fp32 (e^60 x 1000 neighbours is fine,
    but e^a grows past fp32 at a = 88 and loses all small terms long before); the online softmax subtracts the running
    maximum, which here moves many times inside one list."""
    d = 200
    torch.manual_seed(100 + d)
    probe = dict(_make('attn', d).named_parameters())                  # the parameters _runs_of builds from this seed
    v_scale = 60.0 / _largest_score(probe, _case(d), d, 1.0)
    run = _runs_of('attn', d, dev, v_scale=v_scale)
    top = _largest_score(probe, _case(d), d, v_scale)
    print('v scaled by %.1f: largest |a_j| = %.2f' % (v_scale, top))
    assert 59.0 <= top <= 61.0
    assert torch.isfinite(run['out']).all()
    _check_forward('attn', d, run)


@pytest.mark.parametrize('d', [100, 200, 300, 400])
@pytest.mark.parametrize('kind', KINDS)
def test_backward_against_float64_autograd(dev, kind, d):
    run = _runs_of(kind, d, dev)
    g64, g32, mine = run['ref64'][1], run['ref32'][1], run['grads']
    want = {'mean': ['ent'], 'gcn': ['ent', 'gcn_layer.weight', 'gcn_layer.bias'],
            'attn': ['ent', 'rel', 'attn_s.weight', 'attn_s.bias', 'v_s']}[kind]
    assert sorted(mine) == sorted(want)
    bad = []
    for k in want:
        e_ref, e_mine = _err(g32[k], g64[k]), _err(mine[k], g64[k])
        print('%s D=%d d%s: fp32 reference error %.3e, kernel error %.3e, allowed %.3e' % (kind, d, k, e_ref, e_mine, 4 * e_ref))
        if not e_mine <= 4 * e_ref:
            bad.append((k, e_mine, e_ref))
    assert not bad, bad
    # an entity that no list names and that is nobody's subject: an exactly zero row
    assert float(g64['ent'][NAMED:].abs().max()) == 0.0
    assert torch.count_nonzero(mine['ent'][NAMED:]) == 0
    assert torch.count_nonzero(mine['ent'][:NAMED]) > 0


@pytest.mark.parametrize('kind,d', [('mean', 300), ('gcn', 100), ('attn', 200), ('attn', 400)])
def test_two_runs_are_bit_identical(dev, kind, d):
    torch.manual_seed(7)
    agg = _make(kind, d).to(dev).eval()
    c = _case(d)
    width = (3 if kind == 'attn' else 2) * d
    p1, g1 = _device_run(agg, c, dev, width, None)
    p2, g2 = _device_run(agg, c, dev, width, None)
    assert torch.equal(p1.data, p2.data)
    assert sorted(g1) == sorted(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def _rows_by_sequence(data, order, lens, batch_sizes):
    """packed rows -> {(original sequence, step): row}; order[i] = original index of sorted sequence i."""
    off = np.concatenate(([0], np.cumsum(batch_sizes)))
    return {(int(order[i]), j): data[off[j] + i] for i in range(len(lens)) for j in range(int(lens[i]))}


@pytest.mark.parametrize('d', [100, 200])
@pytest.mark.parametrize('kind', KINDS)
def test_matches_the_reference_fixture(dev, kind, d):
    import model as M
    gold = load_golden('nbr_agg_%s_%d.npz' % (kind, d))
    seq_ptr, nbr_ptr, nbr_o = gold['seq_ptr'], gold['nbr_ptr'], gold['nbr_o']
    hist = [[nbr_o[nbr_ptr[k]:nbr_ptr[k + 1]] for k in range(seq_ptr[i], seq_ptr[i + 1])] for i in range(len(seq_ptr) - 1)]
    shapes = {k: tuple(v) for k, v in json.loads(str(gold['param_shapes'])).items()}
    params = fixtures.make_params(int(gold['param_seed']), shapes)
    for k in shapes:
        if 'param.' + k in gold:
            np.testing.assert_array_equal(params[k], gold['param.' + k])
    agg = _make(kind, d, dropout=0.2, seq_len=int(gold['seq_len']))
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    agg.to(dev).eval()
    ent = torch.from_numpy(gold['ent_embeds']).to(dev).requires_grad_(True)
    rel = torch.from_numpy(gold['rel_embeds']).to(dev).requires_grad_(True)
    s, r = torch.from_numpy(gold['s']), torch.from_numpy(gold['r'])
    packed = agg(hist, s, r, ent, rel)
    nb = agg.last_batch.host
    np.testing.assert_array_equal(packed.batch_sizes.numpy(), gold['batch_sizes'])
    lens_all = np.diff(seq_ptr)
    ref_lens = lens_all[gold['s_idx']][:nb.nseq]
    mine = _rows_by_sequence(packed.data.detach().cpu().numpy(), nb.perm, nb.lens, nb.batch_sizes)
    ref = _rows_by_sequence(gold['packed_data'], gold['s_idx'], ref_lens, gold['batch_sizes'])
    assert mine.keys() == ref.keys()
    for key in ref:
        np.testing.assert_allclose(mine[key], ref[key], rtol=RTOL, atol=ATOL, err_msg=str(key))
    # the same rows again through the FlatHistory input
    import graph as G
    fh = G.FlatHistory(seq_ptr, np.zeros(int(seq_ptr[-1]), np.int64), nbr_ptr, nbr_o)
    with torch.no_grad():
        assert torch.equal(agg(fh, s, r, ent, rel).data, packed.data)
    # predict() of one history
    i = int(gold['pred_index'])
    with torch.no_grad():
        pred = agg.predict(hist[i], s[i], r[i], ent, rel)
    np.testing.assert_allclose(pred.cpu().numpy(), gold['pred_out'], rtol=RTOL, atol=ATOL)
    # h_n of the package's GRU on the packed input, per original sequence
    width = packed.data.shape[1]
    gw = fixtures.make_params(int(gold['gru_seed']), {'weight_ih_l0': (3 * d, width), 'weight_hh_l0': (3 * d, d),
                                                      'bias_ih_l0': (3 * d,), 'bias_hh_l0': (3 * d,)},
                              scale=1.0 / np.sqrt(d))
    gru = M.GRU(width, d)
    gru.load_state_dict({k: torch.from_numpy(v) for k, v in gw.items()})
    gru.to(dev)
    with torch.no_grad():
        _, hn = gru(packed, total_rows=nb.nseq)
    hn = hn[0].cpu().numpy()
    for i_ref in range(nb.nseq):
        i_mine = int(np.nonzero(nb.perm[:nb.nseq] == gold['s_idx'][i_ref])[0][0])
        np.testing.assert_allclose(hn[i_mine], gold['h_n'][i_ref], rtol=RTOL, atol=ATOL)
    # gradients of sum(packed.data * C): C is stored in the reference's row order
    off_m = np.concatenate(([0], np.cumsum(nb.batch_sizes)))
    c_mine = np.empty_like(gold['C'])
    c_ref = _rows_by_sequence(gold['C'], gold['s_idx'], ref_lens, gold['batch_sizes'])
    for i_s in range(nb.nseq):
        for j in range(int(nb.lens[i_s])):
            c_mine[off_m[j] + i_s] = c_ref[(int(nb.perm[i_s]), j)]
    (packed.data * torch.from_numpy(c_mine).to(dev)).sum().backward()
    grads = {k: p.grad for k, p in agg.named_parameters()}
    grads['ent_embeds'], grads['rel_embeds'] = ent.grad, rel.grad
    for k, g in grads.items():
        g = g.cpu().numpy() if g is not None else np.zeros(tuple(gold['rel_embeds'].shape), np.float32)
        ok, err, how = fixtures.check_packed(gold, 'grad.' + k, g, GRAD_RTOL, GRAD_ATOL)
        assert ok, (k, err, how)


@pytest.mark.parametrize('kind', ['mean', 'attn'])
def test_train_mode_dropout(dev, kind):
    d = 200
    torch.manual_seed(11)
    agg = _make(kind, d, dropout=0.5).to(dev)
    c = _case(d)
    width = (3 if kind == 'attn' else 2) * d
    agg.eval()
    p_eval, _ = _device_run(agg, c, dev, width, None)
    x = p_eval.data.detach()
    assert torch.count_nonzero(x) == x.numel()
    agg.train()
    p_train, g_train = _device_run(agg, c, dev, width, None)
    y = p_train.data.detach()
    dropped = y == 0
    assert torch.equal(y[~dropped], (2.0 * x)[~dropped])               # every element: 0 or the eval value x 2
    n = y.numel()
    frac = float(dropped.sum()) / n
    print('%s: dropped fraction %.5f of %d elements (5 sigma = %.5f)' % (kind, frac, n, 2.5 / np.sqrt(n)))
    assert abs(frac - 0.5) <= 5 * 0.5 / np.sqrt(n)
    # the backward pass masks the same elements: eval mode with the upstream gradient C * mask * 2 gives the same bits
    c2 = dict(c)
    c2['C'] = c['C'].copy()
    c2['C'][:, :width] = c['C'][:, :width] * (2.0 * (~dropped).float().cpu().numpy())
    agg.eval()
    _, g_eval = _device_run(agg, c2, dev, width, None)
    assert sorted(g_eval) == sorted(g_train)
    for k in g_eval:
        assert torch.equal(g_eval[k], g_train[k]), k


def test_edge_cases(dev):
    import renet_hip as K
    ent, rel = torch.zeros(8, 100, device=dev), torch.zeros(2, 100, device=dev)
    for kind in KINDS:
        agg = _make(kind, 100).to(dev)
        assert agg([[], []], torch.tensor([0, 1]), torch.tensor([0, 1]), ent, rel) is None
        assert tuple(agg.predict([], torch.tensor(0), torch.tensor(0), ent, rel).shape) == (0, (3 if kind == 'attn' else 2) * 100)
    # D outside renet_dim_ok: refused at the entry, before anything is read
    L = K.lib()
    assert L.renet_nbr_pool_fwd(*([None] * 12), 1, 500, 1, None, None, None, None) == -2
    assert L.renet_nbr_pool_bwd(*([None] * 12), 1, 500, 1, *([None] * 7)) == -2
    # a segment of length 0: RENET_ERR_BADARG, nothing launched
    z = torch.zeros(64, 100, device=dev)
    iz = torch.zeros(8, dtype=torch.int32, device=dev)
    host = (ctypes.c_int32 * 2)(0, 0)
    rc = L.renet_nbr_pool_fwd(z.data_ptr(), None, None, None, None, iz.data_ptr(), iz.data_ptr(),
                              ctypes.cast(host, ctypes.c_void_p), iz.data_ptr(), None, None, iz.data_ptr(), 1, 100, 0,
                              z.data_ptr(), None, None, None)
    assert rc == -1
    # an id beyond the table is refused on the host
    agg = _make('mean', 100).to(dev)
    with pytest.raises(ValueError, match='beyond the embedding table'):
        agg([[np.asarray([9])]], torch.tensor([0]), torch.tensor([0]), ent, rel)
