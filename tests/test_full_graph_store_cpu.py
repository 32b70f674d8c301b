"""CPU tests of the resident store behind the device builder of the global model's full-graph batches
(gpu_builder.FullGraphStore; csrc/builder_full.hip: renet_build_full_graphs).  No GPU is needed or initialised here: the store
is built with device=None (host arrays only), and its numpy statement of the device front (host_edges) is pinned against
graph.build_full_graphs, whose arrays the device builder must reproduce bit for bit (tests/test_gpu_full_graph_builder.py)."""
import numpy as np
import pytest
import torch


def _graph_dict(shape, num_t):
    import preprocess as P
    import synth
    quads, ne, nr, _ = synth.make_stream(shape, seed=999, num_t=num_t)
    return P.build_graph_dict(quads, nr), ne, nr


def _subsets(T):
    rng = np.random.RandomState(7)
    some = rng.permutation(T)[:max(2, T // 3)]
    return [np.array([T // 2]), np.arange(T), some, np.concatenate((some[:3], some[1:2], some[3:]))]


@pytest.mark.parametrize('shape,num_t', [('ICEWS18', 40), ('WIKI', 60), ('YAGO', 30)])
def test_host_arrays_rebuild_every_time_graph(shape, num_t):
    import gpu_builder
    gd, ne, nr = _graph_dict(shape, num_t)
    fs = gpu_builder.FullGraphStore(gd, nr, device=None)
    h = fs.host
    assert fs.t is None and fs.c is None
    assert fs.T == len(gd) and len(h['node_ptr']) == fs.T + 1 and len(h['trip_ptr']) == fs.T + 1
    assert all(a.dtype == np.int32 for a in h.values())
    for k, t in enumerate(gd):
        g = gd[t]
        n0, n1 = h['node_ptr'][k], h['node_ptr'][k + 1]
        f0, f1 = h['trip_ptr'][k], h['trip_ptr'][k + 1]
        assert np.array_equal(h['node_ent_all'][n0:n1], g.ent)
        assert np.array_equal(h['trip_ls'][f0:f1], g.ls)
        assert np.array_equal(h['trip_r'][f0:f1], g.r)
        assert np.array_equal(h['trip_lo'][f0:f1], g.lo)
    assert h['node_ptr'][-1] == len(h['node_ent_all']) and h['trip_ptr'][-1] == len(h['trip_ls'])
    assert not torch.cuda.is_initialized()


@pytest.mark.parametrize('shape,num_t', [('ICEWS18', 40), ('WIKI', 60)])
def test_edge_positions_give_the_order_of_build_full_graphs(shape, num_t):
    """Edge e of member graph k sits at 2 * trip_off_k + e: forward facts, then reversed facts, PER GRAPH.  The order decides
    every tie of the stable sorts behind it, so both the raw lists and the layouts derived from them must match."""
    import gpu_builder
    import graph as G
    gd, ne, nr = _graph_dict(shape, num_t)
    fs = gpu_builder.FullGraphStore(gd, nr, device=None)
    times = np.asarray(list(gd.keys()), dtype=np.int64)
    for tidx in _subsets(len(times)):
        node_ent, src, dst, et = fs.host_edges(tidx)
        gs = [gd[int(t)] for t in times[tidx]]
        off = np.concatenate(([0], np.cumsum([g.number_of_nodes() for g in gs])))
        parts = [g.edges(False) for g in gs]
        assert np.array_equal(src, np.concatenate([p[0] + o for p, o in zip(parts, off)]))
        assert np.array_equal(dst, np.concatenate([p[1] + o for p, o in zip(parts, off)]))
        assert np.array_equal(et, np.concatenate([p[2] for p in parts]))
        noff, foff = fs.sizes(tidx)
        assert np.array_equal(noff, off) and 2 * foff[-1] == len(src)
        # the same edge list through the host layouts = graph.build_full_graphs
        hb = G.build_full_graphs(gd, times[tidx])
        mine = G.HostBatch().set_edges(int(noff[-1]), src, dst, et, 2 * nr).set_gather_plan()
        assert np.array_equal(node_ent, hb.node_ent) and np.array_equal(noff, hb.seg_ptr)
        for f in ('row_ptr', 'col', 'etype', 'norm', 'heavy_rows', 'e_src', 'e_dst', 'chunk_ptr', 'chunk_type',
                  'type_chunk_ptr', 'it_src', 'it_type', 'grp_ptr'):
            assert np.array_equal(getattr(mine, f), getattr(hb, f)), f
        assert (mine.n_chunks, mine.n_groups, mine.n_groups_out) == (hb.n_chunks, hb.n_groups, hb.n_groups_out)
        assert hb.n_groups_out == hb.n_groups                  # no row prefix in a full-graph batch
    assert not torch.cuda.is_initialized()


def test_store_checks_its_ranges():
    import gpu_builder
    gd, ne, nr = _graph_dict('YAGO', 20)
    with pytest.raises(ValueError):
        gpu_builder.FullGraphStore(gd, nr - 1, device=None)            # a relation id outside [0, num_rels)
    fs = gpu_builder.FullGraphStore(gd, nr, device=None)
    with pytest.raises(KeyError):
        fs.sizes([len(gd)])
    with pytest.raises(KeyError):
        fs.store.index_of(np.array([10 ** 9]))


def test_cache_returns_the_same_store_until_the_dict_gains_a_timestamp():
    import gpu_builder
    import graph as G
    gd, ne, nr = _graph_dict('YAGO', 20)
    a = gpu_builder.full_graph_store_for(gd, nr, None)
    assert gpu_builder.full_graph_store_for(gd, nr, None) is a
    assert a.store is G.store_for(gd)
    ts = list(gd.keys())
    t_new = ts[-1] + (ts[1] - ts[0])
    gd[t_new] = G.TimeGraph.from_triples(np.array([[1, 0, 2], [2, 1, 3]]), nr)
    b = gpu_builder.full_graph_store_for(gd, nr, None)
    assert b is not a and b.T == a.T + 1
    assert gpu_builder.full_graph_store_for(gd, nr, None) is b
    assert np.array_equal(b.host['node_ent_all'][b.host['node_ptr'][-2]:], [1, 2, 3])
    assert len(gpu_builder._full_stores) <= 9
    assert not torch.cuda.is_initialized()
