"""GPU tests of the DEVICE builder for the global model's full-graph batches (csrc/builder_full.hip: renet_build_full_graphs;
gpu_builder.FullGraphStore / FullGraphBatch; RGCNAggregator_global.device_builder): every array it produces is compared BIT
FOR BIT with graph.build_full_graphs uploaded through graph.DeviceGraph, the capacity guard reports instead of faulting, a
RENet_global computes exactly the same numbers with the switch on as with it off, and with the switch on it still matches
the unmodified reference's recorded outputs."""
import numpy as np
import pytest
import torch

from helpers import fixtures, global_shapes, load_golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 2e-5            # tests/test_gpu_parity.py


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


_streams = {}


def _setup(shape, num_t, dev):
    """graph_dict of a synth stream (the shapes of tests/test_gpu_builder.py::_setup) + its resident full-graph store."""
    import gpu_builder
    import preprocess as P
    import synth
    key = (shape, num_t)
    if key not in _streams:
        quads, ne, nr, _ = synth.make_stream(shape, seed=999, num_t=num_t)
        _streams[key] = (P.build_graph_dict(quads, nr), ne, nr)
    gd, ne, nr = _streams[key]
    return gd, ne, nr, gpu_builder.full_graph_store_for(gd, nr, dev)


def _same(name, a, b):
    if a is None or b is None:
        assert a is None and b is None, (name, a, b)
        return
    assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
    assert torch.equal(a, b), (name, torch.nonzero(a.reshape(-1) != b.reshape(-1)).reshape(-1)[:10].tolist())


def _assert_same_full_batch(fb, dg):
    """fb: gpu_builder.FullGraphBatch (finalized); dg: graph.DeviceGraph of graph.build_full_graphs on the same timestamps."""
    for f in ('N', 'E', 'G', 'nA', 'n_chunks', 'n_groups', 'n_groups_out', 'num_types', 'heavy_thresh'):
        assert int(getattr(fb, f)) == int(getattr(dg, f)), (f, getattr(fb, f), getattr(dg, f))
        if hasattr(dg.host, f):                                 # (the host batch itself: what the model reads as g.host)
            assert int(getattr(fb.host, f)) == int(getattr(dg.host, f)), ('host.' + f,)
    assert fb.nA == fb.N and fb.n_groups_out == fb.n_groups
    for f in ('seg_ptr', 'node_ent', 'row_ptr', 'col', 'etype', 'norm', 'heavy_rows', 'e_src', 'e_dst', 'type_chunk_ptr',
              'chunk_type', 'chunk_ptr', 'it_src', 'it_type', 'grp_ptr'):
        _same(f, getattr(fb, f), getattr(dg, f))
    _same('heavy_rows_out', fb.heavy_rows_out, fb.heavy_rows)
    a, b = fb.plan_node_ent, dg.plan_node_ent
    assert a.num_segments == b.num_segments
    for sub in ('order', 'seg_ptr', 'target'):
        _same('plan_node_ent.' + sub, getattr(a, sub), getattr(b, sub))
    for f in ('e_src2', 'e_dst2', 'chunk_ptr2', 'chunk_type2', 'type_chunk_ptr2'):
        assert not hasattr(fb, f), f


def _subsets(T):
    rng = np.random.RandomState(7)
    some = rng.permutation(T)[:max(2, T // 3)]                              # a random subset in random order
    twice = np.concatenate((some[:3], some[1:2], some[3:]))                 # ... with one timestamp twice
    return [('one', np.array([T // 2])), ('all', np.arange(T)), ('some', some), ('twice', twice)]


@pytest.mark.parametrize('shape,num_t', [('ICEWS18', None), ('YAGO', None), ('ICEWS18', 40), ('WIKI', 60)])
def test_device_built_full_graph_batch_is_bit_identical_to_the_host_builder(dev, shape, num_t):
    import gpu_builder
    import graph as G
    gd, ne, nr, fs = _setup(shape, num_t, dev)
    times = np.asarray(list(gd.keys()), dtype=np.int64)
    assert len(times) <= gpu_builder.MAX_FULL_GRAPHS
    for what, tidx in _subsets(len(times)):
        hb = G.build_full_graphs(gd, times[tidx])
        if what == 'all':
            # every shape has hub rows (in-degree > graph.HEAVY: a workgroup each) ...
            assert len(hb.heavy_rows) > 0, (shape, num_t)
            if shape == 'ICEWS18':
                # ... and this one a relation with more than graph.CHUNK edges (several dW work items of one type)
                assert int(np.diff(hb.type_chunk_ptr).max()) > 1 and int(np.bincount(hb.etype).max()) > G.CHUNK
        assert np.array_equal(fs.store.index_of(times[tidx]), tidx)
        fb = gpu_builder.FullGraphBatch(fs, tidx)
        assert fb.finalize() and fb.finalize()
        _assert_same_full_batch(fb, G.DeviceGraph(hb, dev))
        assert fb.table_items() is fb.table_items()


def test_full_graph_batch_built_on_a_side_stream(dev):
    import gpu_builder
    import graph as G
    gd, ne, nr, fs = _setup('WIKI', 60, dev)
    times = np.asarray(list(gd.keys()), dtype=np.int64)
    side = torch.cuda.Stream()
    tidx = np.arange(5, 25)
    fb = gpu_builder.FullGraphBatch(fs, tidx, stream=side)
    fb.finalize()
    _assert_same_full_batch(fb, G.DeviceGraph(G.build_full_graphs(gd, times[tidx]), dev))


def test_edge_capacity_one_below_E_sets_the_error_bit_and_nothing_faults(dev):
    """The raw C call with cap_edges = E - 1: it returns normally, counts[C_ERR] has the edge bit, and the batch is EMPTY on
    the device (every later stage is guarded by the counts) -- no output array is read here."""
    import gpu_builder
    gd, ne, nr, fs = _setup('ICEWS18', 40, dev)
    tidx = np.arange(len(gd))
    noff, foff = fs.sizes(tidx)
    N, E = int(noff[-1]), 2 * int(foff[-1])
    idx_dev = torch.from_numpy(tidx.astype(np.int32)).to(dev)
    v, norm, keep = gpu_builder.build_full_graphs_raw(fs, idx_dev, len(tidx), N, E - 1)
    torch.cuda.synchronize()
    c = v['counts'].cpu().numpy()
    assert c[gpu_builder.C_ERR] & 8, c[gpu_builder.C_ERR]
    assert c[gpu_builder.C_N] == 0 and c[gpu_builder.C_E] == 0 and c[gpu_builder.C_NITEMS] == 0
    # and the node guard, the same way
    v, norm, keep = gpu_builder.build_full_graphs_raw(fs, idx_dev, len(tidx), N - 1, E)
    torch.cuda.synchronize()
    c = v['counts'].cpu().numpy()
    assert c[gpu_builder.C_ERR] & 4 and c[gpu_builder.C_N] == 0 and c[gpu_builder.C_E] == 0
    # exact capacities: no bit
    v, norm, keep = gpu_builder.build_full_graphs_raw(fs, idx_dev, len(tidx), N, E)
    torch.cuda.synchronize()
    c = v['counts'].cpu().numpy()
    assert c[gpu_builder.C_ERR] == 0 and c[gpu_builder.C_N] == N and c[gpu_builder.C_E] == E


def _soft_targets(n_t, ne, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(n_t, ne, generator=g) * 3, dim=1)


@pytest.mark.parametrize('dropout', [0.0, 0.5])
def test_global_model_is_bit_identical_with_the_device_builder_on(dev, dropout):
    """Same seed, switch off then on: loss, pooled, every parameter gradient (both heads) and predict() are torch.equal --
    the graph arrays are identical and the kernels are the same, so any difference is a bug, not rounding."""
    import global_model as GM
    import ops
    gd, ne, nr, _ = _setup('ICEWS18', 40, dev)
    times = np.asarray(list(gd.keys()), dtype=np.int64)
    true_s, true_o = _soft_targets(len(times), ne, 1).to(dev), _soft_targets(len(times), ne, 2).to(dev)
    torch.manual_seed(11)
    net = GM.RENet_global(ne, 200, nr, dropout=dropout, seq_len=10, maxpool=1).to(dev)
    net.train()
    assert net.aggregator.device_builder is None
    res = []
    for on in (False, True):
        net.aggregator.device_builder = on
        out = {}
        for subj in (True, False):
            torch.manual_seed(999)
            ops.reset_seed_counter()
            net.zero_grad(set_to_none=True)
            loss = net(torch.from_numpy(times), true_s, true_o, gd, subject=subj)
            loss.backward()
            torch.cuda.synchronize()
            out['loss%d' % subj] = loss.detach().clone()
            for k, p in net.named_parameters():
                if p.grad is not None:
                    out['grad%d.%s' % (subj, k)] = p.grad.clone()
        torch.manual_seed(999)
        ops.reset_seed_counter()
        with torch.no_grad():
            out['pooled'] = net.aggregator.pooled(times[3:17], net.ent_embeds, gd, False)
            for t in (times[1], times[12], times[-1]):                   # times[1]: the first timestamp with a history
                for subj in (True, False):
                    emb, logits, prob = net.predict(int(t), gd, subject=subj)
                    out['predict%d_%d' % (t, subj)] = torch.cat((emb.view(-1), logits.view(-1), prob.view(-1)))
        res.append(out)
    assert res[0].keys() == res[1].keys() and any(k.startswith('grad1.aggregator') for k in res[0])
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    assert bool(torch.isfinite(res[1]['loss1'])) and float(res[1]['pooled'].abs().max()) > 0


def test_switch_follows_the_environment_when_the_attribute_is_none(dev, monkeypatch):
    import gpu_builder
    import Aggregator
    gd, ne, nr, _ = _setup('WIKI', 60, dev)
    times = list(gd.keys())[:4]
    agg = Aggregator.RGCNAggregator_global(200, 0.0, ne, nr, 100, 0, 10, 1)
    emb = torch.zeros(ne, 200, device=dev)
    monkeypatch.delenv('RENET_GLOBAL_DEVICE_BUILDER', raising=False)
    assert not isinstance(agg._full_graphs(times, emb, gd), gpu_builder.FullGraphBatch)           # default: off
    monkeypatch.setenv('RENET_GLOBAL_DEVICE_BUILDER', '1')
    assert isinstance(agg._full_graphs(times, emb, gd), gpu_builder.FullGraphBatch)
    assert not isinstance(agg._full_graphs(times, emb.cpu(), gd), gpu_builder.FullGraphBatch)     # not on a GPU: host path
    agg.device_builder = False
    assert not isinstance(agg._full_graphs(times, emb, gd), gpu_builder.FullGraphBatch)


@pytest.mark.parametrize('name,d,maxpool', [('tiny', 100, 1), ('tiny', 200, 0), ('small', 200, 1)])
def test_global_model_on_the_device_builder_matches_reference_golden(dev, name, d, maxpool):
    """tests/test_gpu_parity.py::test_global_model_matches_reference_golden with device_builder = True (same tolerances)."""
    import global_model as GM
    import utils as U
    gold = load_golden('global_%s_%d_max%d.npz' % (name, d, maxpool))
    cfg, tr, va, te = fixtures.split_dataset(name)
    seq_len = int(gold['seq_len'])
    p = fixtures.make_params(int(gold['param_seed']), global_shapes(cfg['num_ent'], cfg['num_rels'], d))
    net = GM.RENet_global(cfg['num_ent'], d, cfg['num_rels'], dropout=0.0, seq_len=seq_len, maxpool=maxpool)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    net.to(dev)
    net.aggregator.device_builder = True
    gd = U.build_graph_dict(tr, cfg['num_rels'])
    times = np.unique(tr[:, 3])
    loss = net(torch.from_numpy(times), torch.from_numpy(gold['true_s']).to(dev),
               torch.from_numpy(gold['true_o']).to(dev), gd, subject=True)
    assert abs(loss.item() - float(gold['loss'])) < 2e-4 * max(1.0, abs(float(gold['loss'])))
    loss.backward()
    for k, prm in net.named_parameters():
        if ('grad.' + k) in gold or ('grad.' + k + '__samp') in gold:
            ok, err, how = fixtures.check_packed(gold, 'grad.' + k, prm.grad.cpu().numpy(), 2e-3, 3e-5)
            assert ok, (k, err, how)
    with torch.no_grad():
        for k, t in enumerate(gold['predict_t']):
            for subj in (True, False):
                emb, logits, prob = net.predict(int(t), gd, subject=subj)
                tag = 'predict%d_%s_' % (k, 's' if subj else 'o')
                np.testing.assert_allclose(emb.view(-1).cpu().numpy(), gold[tag + 'emb'], rtol=RTOL, atol=ATOL)
                np.testing.assert_allclose(logits.view(-1).cpu().numpy(), gold[tag + 'logits'], rtol=RTOL, atol=ATOL)
        ge = net.get_global_emb(times, gd)
        assert [int(x) for x in ge.keys()] == gold['global_emb_keys'].tolist()
        vals = np.stack([ge[x].view(-1).cpu().numpy() for x in ge.keys()])
        np.testing.assert_allclose(vals, gold['global_emb_vals'], rtol=RTOL, atol=ATOL)


def test_global_model_at_pretrain_scale_on_the_device_builder_matches_reference(dev):
    """The reference part of tests/test_gpu_config.py::test_global_model_at_pretrain_scale_matches_reference_and_oracle (240
    full graphs in one RGCN pass, then get_global_emb over the whole timeline) with device_builder = True, against
    config_global_icews18_d200.npz, same tolerances."""
    import global_model as GM
    import preprocess as P
    from oracle import config_cases as C
    gold = load_golden('config_global_icews18_d200.npz')
    case = C.build_global_case('global_icews18_d200')
    spec = case['spec']
    d = spec['hidden']
    net = GM.RENet_global(case['num_ent'], d, case['num_rels'], dropout=0.0, seq_len=spec['seq_len'],
                          maxpool=spec['maxpool'])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in case['params'].items()})
    net.to(dev)
    net.eval()
    net.aggregator.device_builder = True
    gd = P.build_graph_dict(case['quads'], case['num_rels'])
    times = case['times']
    loss = net(torch.from_numpy(times.copy()), torch.from_numpy(case['true_s']).to(dev),
               torch.from_numpy(case['true_o']).to(dev), gd, subject=True)
    loss.backward()
    torch.cuda.synchronize()
    ref = float(gold['loss'])
    assert abs(loss.item() - ref) < 1e-4 * abs(ref), (loss.item(), ref)
    for k, p in net.named_parameters():
        if ('grad.' + k) in gold or ('grad.' + k + '__samp') in gold:
            ok, err, scale = C.compare_packed(gold, 'grad.' + k, p.grad.cpu().numpy(), rel=2e-3)
            assert ok, ('reference', k, err, scale)
    with torch.no_grad():
        ge = net.get_global_emb(times, gd)
    assert [int(x) for x in ge.keys()] == gold['global_emb_keys'].tolist()
    vals = np.stack([ge[x].view(-1).cpu().numpy() for x in ge.keys()])
    ok, err, scale = C.compare_packed(gold, 'global_emb_vals', vals, rel=5e-4)
    assert ok, ('global_emb', err, scale)
