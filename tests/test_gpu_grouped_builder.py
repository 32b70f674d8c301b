"""GPU tests of the DEVICE builder for grouped inference batches (csrc/builder_grouped.hip: renet_build_batch_grouped;
gpu_builder.GroupedBatchStore / GroupedDeviceBatch; RGCNAggregator.grouped_device_builder): every array it produces is
compared BIT FOR BIT with the host builder's graph.build_batch(..., sort=True, group=s), the capacities grow from 256, the
guarded error paths raise, and forward_grouped / evaluate_filter_stream give the same results with the switch on and off."""
import numpy as np
import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu

# (stream shape, seq_len, sequences, timestamps of the synthetic stream)
CASES = {'icews18': ('ICEWS18', 10, 96, 40), 'wiki': ('WIKI', 10, 777, 60), 'yago': ('YAGO', 15, 300, 50)}
_streams = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _stream(name):
    """(quads, ne, nr, graph_dict, subject HistoryIndex, global_emb stand-in, its sorted timestamps), made once per shape."""
    if name not in _streams:
        import preprocess as P
        import synth
        shape, seq_len, _, num_t = CASES[name]
        quads, ne, nr, _ = synth.make_stream(shape, seed=999, num_t=num_t)
        gd = P.build_graph_dict(quads, nr)
        g = torch.Generator().manual_seed(3)
        glob = {int(t): torch.randn(1, 1, 8, generator=g) for t in gd}
        _streams[name] = (quads, ne, nr, gd, P.HistoryIndex(quads, 's', seq_len), glob,
                          np.asarray(sorted(glob.keys()), dtype=np.int64))
    return _streams[name]


def _late(quads, back=2):
    """Indices of the quadruples of one late timestamp."""
    times = np.unique(quads[:, 3])
    return np.nonzero(quads[:, 3] == times[-back])[0]


def _case_idx(name):
    quads = _stream(name)[0]
    n, late = CASES[name][2], _late(_stream(name)[0])
    if name == 'icews18':                # a quarter as many quadruples, each four times: duplicate (group, t, entity) keys
        return np.resize(late[:n // 4], n)
    assert len(late) >= n
    return late[:n]


def _host(name, idx, fh=None):
    import graph as G
    quads, ne, nr, gd, hs, glob, gtimes = _stream(name)
    fh = hs.take(idx) if fh is None else fh
    s, r = quads[idx, 0], quads[idx, 1]
    hb = G.build_batch(G.store_for(gd), ne, nr, s, r, fh, sort=True, glob_index=lambda t: np.searchsorted(gtimes, t), group=s)
    return hb, s, r, fh


def _device(base, s, r, group, fh, seq_len, attempts):
    import gpu_builder
    for attempt in range(attempts):                         # capacities grow on overflow, one doubling per attempt
        db = gpu_builder.GroupedDeviceBatch(gpu_builder.GroupedBatchStore(base, s, r, group, fh), seq_len)
        if db.finalize():
            return db, attempt + 1
    raise AssertionError('device builder did not converge on its capacities in %d attempts' % attempts)


def _cmp(name, dev_t, host_a):
    a = dev_t.cpu().numpy() if dev_t is not None else np.zeros(0, np.int64)
    b = np.asarray(host_a) if host_a is not None else np.zeros(0, np.int64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if a.dtype != np.float32:
        a, b = a.astype(np.int64), b.astype(np.int64)
    assert np.array_equal(a, b), (name, np.nonzero(a.reshape(-1) != b.reshape(-1))[0][:10])


def _assert_same_batch(db, hb):
    for f in ('N', 'E', 'S', 'nnz', 'L', 'nA', 'E_out', 'n_chunks', 'n_chunks2', 'n_groups', 'n_groups_out', 'B', 'num_types'):
        assert int(getattr(db, f)) == int(getattr(hb, f)), (f, getattr(db, f), getattr(hb, f))
    for f in ('node_ent', 'node_slot', 'row_ptr', 'col', 'etype', 'norm', 'e_src', 'e_dst', 'chunk_ptr', 'chunk_type',
              'type_chunk_ptr', 'e_src2', 'e_dst2', 'chunk_ptr2', 'chunk_type2', 'type_chunk_ptr2', 'it_src', 'it_type',
              'grp_ptr', 'subj_row', 'row_seq', 'row_ent', 'row_rel', 'glob_row', 's_sorted', 'r_sorted', 'heavy_rows',
              'heavy_rows_out', 'step_off'):
        _cmp(f, getattr(db, f), getattr(hb, f))
    assert not hasattr(db, 'rel_label') and not hasattr(db, 'ent_label')
    assert np.array_equal(db.host.step_off, hb.step_off) and np.array_equal(db.host.batch_sizes, hb.batch_sizes)
    assert db.host.batch_sizes.dtype == hb.batch_sizes.dtype
    assert np.array_equal(db.host.perm, hb.perm)
    for pn in ('plan_node_ent', 'plan_subj_row', 'plan_s', 'plan_r'):
        a, b = getattr(db, pn), getattr(hb, pn)
        assert a.num_segments == b.num_segments, pn
        for sub in ('order', 'seg_ptr', 'target'):
            _cmp(pn + '.' + sub, getattr(a, sub), getattr(b, sub))


def _fresh_store(name, dev, cap=None):
    import gpu_builder
    quads, ne, nr, gd, hs, glob, gtimes = _stream(name)
    base = gpu_builder.GraphDeviceStore(gd, glob, ne, nr, dev)
    if cap is not None:
        base.cap_nodes = base.cap_edges = cap
    return base


@pytest.mark.parametrize('name', sorted(CASES))
def test_grouped_batch_is_bit_identical_to_the_host_builder(dev, name):
    import graph as G
    idx = _case_idx(name)
    hb, s, r, fh = _host(name, idx)
    deg = np.diff(hb.row_ptr)
    slot, ent, gt = np.asarray(hb.node_slot), np.asarray(hb.node_ent), np.asarray(hb.graph_t)
    sets = {}
    for c in range(len(gt)):
        sets.setdefault(int(gt[c]), set()).add(frozenset(ent[slot == c].tolist()))
    print(name, 'B', hb.B, 'nnz', hb.nnz, 'S', hb.S, 'slots', len(gt), 'N', hb.N, 'nA', hb.nA, 'E', hb.E, 'max in-degree',
          int(deg.max()), 'timestamps with several node sets', sum(len(v) > 1 for v in sets.values()))
    # not vacuous: hub rows, groups that share a timestamp with different node sets, several sequences per member graph,
    # empty histories behind the non-empty ones
    assert deg.max() > G.HEAVY and hb.heavy_rows is not None and len(hb.heavy_rows) > 0
    assert any(len(v) > 1 for v in sets.values())
    assert len(gt) > len(np.unique(gt)) and hb.S > hb.nA
    assert 0 < hb.nnz < hb.B
    db, _ = _device(_fresh_store(name, dev), s, r, s, fh, CASES[name][1], 6)
    _assert_same_batch(db, hb)


def test_empty_histories_among_the_others_sort_last(dev):
    """The first quadruples of the stream (no history yet) interleaved with late ones."""
    quads = _stream('icews18')[0]
    late = _late(quads)[:40]
    idx = np.stack((np.arange(40), late), axis=1).reshape(-1)[3:]
    hb, s, r, fh = _host('icews18', idx)
    lens = np.diff(fh.seq_ptr)
    assert 0 < hb.nnz < hb.B and lens[0] > 0 and np.count_nonzero(lens == 0) >= 20
    db, _ = _device(_fresh_store('icews18', dev), s, r, s, fh, 10, 6)
    _assert_same_batch(db, hb)
    assert np.all(lens[db.host.perm[hb.nnz:]] == 0)


def test_one_sequence_with_one_step(dev):
    import graph as G
    quads, ne, nr, gd, hs, glob, gtimes = _stream('icews18')
    idx = _late(quads)[:200]
    full = hs.take(idx)
    i = int(np.nonzero(np.diff(full.seq_ptr) > 0)[0][0])
    k = int(full.seq_ptr[i + 1] - 1)                                       # its newest step only
    fh = G.FlatHistory([0, 1], full.step_t[k:k + 1], [0, full.nbr_ptr[k + 1] - full.nbr_ptr[k]],
                       full.nbr_o[full.nbr_ptr[k]:full.nbr_ptr[k + 1]])
    hb, s, r, fh = _host('icews18', idx[i:i + 1], fh)
    assert hb.B == hb.nnz == hb.S == hb.L == 1 and hb.N >= 1
    db, _ = _device(_fresh_store('icews18', dev), s, r, s, fh, 10, 6)
    _assert_same_batch(db, hb)


@pytest.mark.parametrize('name', ['icews18', 'yago'])
def test_capacities_grow_from_256(dev, name):
    """cap_nodes = cap_edges = 256: every attempt doubles ONE capacity (a node overflow hides the edge count), so the
    builder needs log2 steps for the nodes, then for the edges (E, and the item stream E + N is sized with both), plus the
    attempt that fits -- at most 12 for these cases, checked on the host batch."""
    hb, s, r, fh = _host(name, _case_idx(name))
    need = lambda n: max(int(np.ceil(np.log2(max(n, 256) / 256.0))), 0)
    most = need(hb.N) + need(hb.E) + 1
    print(name, 'N', hb.N, 'E', hb.E, 'attempts at most', most)
    assert hb.N > 256 and hb.E > 256 and most <= 12
    base = _fresh_store(name, dev, 256)
    db, attempts = _device(base, s, r, s, fh, CASES[name][1], 12)
    print(name, 'attempts', attempts, 'cap_nodes', base.cap_nodes, 'cap_edges', base.cap_edges)
    assert attempts <= most and base.cap_nodes >= hb.N and base.cap_edges >= hb.E
    assert base.cap_nodes < 2 * max(hb.N, 256) and base.cap_edges < 2 * max(hb.E, 256)      # nothing doubled needlessly
    _assert_same_batch(db, hb)


def test_missing_timestamp_and_long_history_raise(dev):
    import gpu_builder
    import preprocess as P
    quads, ne, nr, gd, hs, glob, gtimes = _stream('icews18')
    idx = _case_idx('icews18')
    fh = hs.take(idx)
    s, r = quads[idx, 0], quads[idx, 1]
    gone = int(np.unique(fh.step_t)[-2])                                   # a timestamp the histories do hold
    gd_less = P.build_graph_dict(quads[quads[:, 3] != gone], nr)
    assert gone not in gd_less and gone in glob
    base = gpu_builder.GraphDeviceStore(gd_less, glob, ne, nr, dev)
    with pytest.raises(KeyError):
        _device(base, s, r, s, fh, 10, 6)
    glob_less = {t: v for t, v in glob.items() if t != gone}
    with pytest.raises(KeyError):
        _device(gpu_builder.GraphDeviceStore(gd, glob_less, ne, nr, dev), s, r, s, fh, 10, 6)
    assert int(np.diff(fh.seq_ptr).max()) == 10
    with pytest.raises(ValueError):
        gpu_builder.GroupedDeviceBatch(gpu_builder.GroupedBatchStore(_fresh_store('icews18', dev), s, r, s, fh), 9)
    torch.cuda.synchronize()
    # the store still builds: the guarded paths left nothing behind
    hb = _host('icews18', idx)[0]
    db, _ = _device(_fresh_store('icews18', dev), s, r, s, fh, 10, 6)
    _assert_same_batch(db, hb)


# ---- the consumers: forward_grouped and the filtered evaluation ---------------------------------------------------------
def _net(dev, name='icews18'):
    import model as M
    quads, ne, nr, gd, hs, glob, gtimes = _stream(name)
    torch.manual_seed(1)
    net = M.RENet(ne, 100, nr, dropout=0.0, seq_len=CASES[name][1])
    g = torch.Generator().manual_seed(4)
    net.global_emb = {int(t): torch.randn(1, 1, 100, generator=g) * 0.1 for t in gd}
    return net.to(dev).eval()


def _forward_grouped(net, on, name, idx, reverse):
    import graph as G
    quads, ne, nr, gd, hs, glob, gtimes = _stream(name)
    agg = net.aggregator
    agg.grouped_device_builder = on
    rel = net.rel_embeds[nr:] if reverse else net.rel_embeds[:nr]
    with torch.no_grad():
        px, pxr = agg.forward_grouped(hs.take(idx), quads[idx, 0], quads[idx, 1], net.ent_embeds, rel, gd, net.global_emb,
                                      reverse, quads[idx, 0])
    torch.cuda.synchronize()
    return px, pxr, agg.last_batch


@pytest.mark.parametrize('reverse', [False, True])
def test_forward_grouped_is_bit_equal_between_the_builders(dev, reverse):
    import gpu_builder
    import graph as G
    net = _net(dev)
    assert net.aggregator.grouped_device_builder is False                  # opt-in
    idx = _case_idx('icews18')
    (px0, pxr0, g0), (px1, pxr1, g1) = (_forward_grouped(net, on, 'icews18', idx, reverse) for on in (False, True))
    assert isinstance(g0, G.DeviceGraph) and isinstance(g1, gpu_builder.GroupedDeviceBatch)
    assert torch.equal(px0.batch_sizes, px1.batch_sizes) and torch.equal(pxr0.batch_sizes, pxr1.batch_sizes)
    assert torch.equal(px0.data, px1.data) and torch.equal(pxr0.data, pxr1.data)
    assert np.array_equal(g0.host.perm, g1.host.perm) and np.array_equal(g0.host.batch_sizes, g1.host.batch_sizes)


def test_switch_falls_back_to_the_host_builder(dev):
    """Above the front's sequence limit, and without any history, forward_grouped with the switch on is the host path."""
    import gpu_builder
    import graph as G
    net = _net(dev)
    quads = _stream('icews18')[0]
    idx = np.resize(_late(quads), gpu_builder.MAX_GROUPED + 1)
    (px0, pxr0, g0), (px1, pxr1, g1) = (_forward_grouped(net, on, 'icews18', idx, False) for on in (False, True))
    assert isinstance(g0, G.DeviceGraph) and isinstance(g1, G.DeviceGraph)
    assert torch.equal(px0.batch_sizes, px1.batch_sizes) and torch.equal(px0.data, px1.data) and torch.equal(pxr0.data, pxr1.data)
    first = np.nonzero(quads[:, 3] == quads[0, 3])[0][:50]                # the first timestamp: no history at all
    for on in (False, True):
        px, pxr, g = _forward_grouped(net, on, 'icews18', first, False)
        assert px is None and pxr is None and g is None


def test_filtered_evaluation_is_the_same_with_the_switch_on(dev):
    """evaluate_filter_stream (one evaluate_filter_batch per timestamp) on the evaluation fixture, h 100, over its first two
    validation timestamps: identical ranks, losses within the tolerance tests/test_gpu_rank.py uses for them."""
    import gpu_builder
    import test_gpu_parity as P
    gold = load_golden('eval_small_100.npz')
    assert int(gold['d']) == 100
    res = {}
    for on in (False, True):
        net, gnet, H, gd, samples, total, valid, va = P._eval_setup(dev, gold)
        t2 = np.unique(va[:, 3])[:2]
        n = min(int(np.count_nonzero(np.isin(va[:, 3], t2))), int(gold['n_eval']))
        assert len(np.unique(va[:n, 3])) == 2
        net.aggregator.grouped_device_builder = on
        built = []
        inner = net.aggregator.encode
        net.aggregator.encode = lambda g, *a, **k: (built.append(type(g)), inner(g, *a, **k))[1]
        (vs, vst), (vo, vot) = H['valid']
        ranks, loss = net.evaluate_filter_stream(valid[:n], (vs[:n], vst[:n]), (vo[:n], vot[:n]), gnet, total)
        assert built and any(b is gpu_builder.GroupedDeviceBatch for b in built) == on, built
        res[on] = (ranks, np.asarray(loss, dtype=np.float64))
    print('ranks differing', int((res[False][0] != res[True][0]).sum()), 'largest loss difference',
          np.abs(res[False][1] - res[True][1]).max())
    assert res[True][0].shape == (n, 2) and np.array_equal(res[False][0], res[True][0])
    np.testing.assert_allclose(res[True][1], res[False][1], rtol=1e-5, atol=1e-5)
