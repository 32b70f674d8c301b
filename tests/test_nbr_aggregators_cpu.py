"""Host side of MeanAggregator / AttnAggregator (no GPU): the public names, the parameter layout, graph.NeighbourBatch
against the reference's sorted batch stored in tests/golden/nbr_agg_*.npz, and the C ABI declarations."""
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, load_golden

import graph as G

KINDS = ('mean', 'gcn', 'attn')
DIMS = (100, 200)


def _hist_lists(gold):
    seq_ptr, nbr_ptr, nbr_o = gold['seq_ptr'], gold['nbr_ptr'], gold['nbr_o']
    return [[nbr_o[nbr_ptr[k]:nbr_ptr[k + 1]] for k in range(seq_ptr[i], seq_ptr[i + 1])]
            for i in range(len(seq_ptr) - 1)]


def _make(kind, d, dropout=0.0, seq_len=4):
    from Aggregator import MeanAggregator, AttnAggregator
    if kind == 'attn':
        return AttnAggregator(d, dropout, seq_len=seq_len)
    return MeanAggregator(d, dropout, seq_len=seq_len, gcn=(kind == 'gcn'))


def test_public_names_import():
    from Aggregator import MeanAggregator, AttnAggregator, RGCNAggregator     # the reference's model.py:5
    assert MeanAggregator(100, 0.2).seq_len == 10 and AttnAggregator(100, 0.2).seq_len == 10
    assert RGCNAggregator is not None


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', DIMS)
def test_state_dict_matches_the_reference_names(kind, d):
    gold = load_golden('nbr_agg_%s_%d.npz' % (kind, d))
    shapes = {k: tuple(v) for k, v in json.loads(str(gold['param_shapes'])).items()}
    sd = _make(kind, d).state_dict()
    assert sorted(sd) == json.loads(str(gold['param_names'])) == sorted(shapes)
    for k, v in sd.items():
        assert tuple(v.shape) == shapes[k], k
    if kind == 'attn':
        assert shapes['v_s'] == (d, 1) and shapes['attn_s.weight'] == (d, 3 * d)


def test_initialisers_are_the_reference_ones():
    torch.manual_seed(0)
    a = _make('attn', 100)
    bound = np.sqrt(2.0) * np.sqrt(6.0 / (100 + 1))                  # xavier_uniform_, gain of relu, on [h, 1]
    assert float(a.v_s.detach().abs().max()) <= bound and float(a.v_s.detach().abs().max()) > 0.5 * bound
    assert float(a.attn_s.weight.detach().abs().max()) <= 1.0 / np.sqrt(300.0)    # nn.Linear(3h, h)
    g = _make('gcn', 100)
    assert float(g.gcn_layer.weight.detach().abs().max()) <= 1.0 / np.sqrt(100.0)


@pytest.mark.parametrize('kind,d', [('mean', 100), ('attn', 200)])
def test_neighbour_batch_reproduces_the_reference_batch(kind, d):
    gold = load_golden('nbr_agg_%s_%d.npz' % (kind, d))
    hist = _hist_lists(gold)
    nb = G.NeighbourBatch(gold['s'], gold['r'], hist, seq_len=int(gold['seq_len']))
    lens = np.diff(gold['seq_ptr'])
    assert np.all(np.diff(lens[nb.perm]) <= 0)                       # perm sorts lengths descending
    assert sorted(nb.perm.tolist()) == list(range(len(lens)))
    assert nb.nseq == int(np.count_nonzero(lens)) and nb.B == len(lens)
    np.testing.assert_array_equal(nb.batch_sizes, gold['batch_sizes'])
    assert nb.batch_sizes.dtype == np.int32 and nb.nbr.dtype == np.int32 and nb.out_row.dtype == np.int32
    # rows through each side's own permutation: per ORIGINAL sequence, its per-step list lengths and ids
    ref_len = np.split(gold['len_s'], np.cumsum(lens[gold['s_idx']][:nb.nseq])[:-1])
    ref_ids = np.split(gold['flat_s'], np.cumsum(gold['len_s'])[:-1])
    mine_len = np.split(np.diff(nb.seg_ptr), np.cumsum(nb.lens)[:-1])
    mine_ids = np.split(nb.nbr, nb.seg_ptr[1:-1])
    k_ref = k_mine = 0
    by_ref, by_mine = {}, {}
    for i in range(nb.nseq):
        n = len(ref_len[i])
        by_ref[int(gold['s_idx'][i])] = (ref_len[i].tolist(), [a.tolist() for a in ref_ids[k_ref:k_ref + n]])
        k_ref += n
        n = len(mine_len[i])
        by_mine[int(nb.perm[i])] = (mine_len[i].tolist(), [a.tolist() for a in mine_ids[k_mine:k_mine + n]])
        k_mine += n
    assert by_ref == by_mine
    # segment bookkeeping: sequence-major segments, packed rows time-major
    off = np.concatenate(([0], np.cumsum(nb.batch_sizes)))
    k = 0
    for i in range(nb.nseq):
        for j in range(int(nb.lens[i])):
            assert nb.out_row[k] == off[j] + i and nb.seg_q[k] == i
            assert nb.seg_s[k] == gold['s'][nb.perm[i]] and nb.seg_r[k] == gold['r'][nb.perm[i]]
            k += 1
    assert k == nb.S == len(nb.seg_ptr) - 1 and nb.nnz == len(nb.nbr) == nb.seg_ptr[-1]
    assert sorted(nb.out_row.tolist()) == list(range(nb.S))
    # the plans list every row once, grouped by target
    for plan, idx in ((nb.plan_nbr, nb.nbr), (nb.plan_seq, nb.seg_q), (nb.plan_s, nb.s_sorted), (nb.plan_r, nb.r_sorted)):
        assert sorted(plan.order.tolist()) == list(range(len(idx)))
        for u in range(plan.num_segments):
            assert np.all(idx[plan.order[plan.seg_ptr[u]:plan.seg_ptr[u + 1]]] == plan.target[u])


def test_flat_history_gives_the_same_batch():
    gold = load_golden('nbr_agg_mean_100.npz')
    fh = G.FlatHistory(gold['seq_ptr'], np.zeros(int(gold['seq_ptr'][-1]), np.int64), gold['nbr_ptr'], gold['nbr_o'])
    a = G.NeighbourBatch(gold['s'], gold['r'], _hist_lists(gold), seq_len=4)
    b = G.NeighbourBatch(gold['s'], gold['r'], fh, seq_len=4)
    for f in ('perm', 'batch_sizes') + G.NeighbourBatch.INT_FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    for pn in G.NeighbourBatch.PLANS:
        for f in ('order', 'seg_ptr', 'target'):
            np.testing.assert_array_equal(getattr(getattr(a, pn), f), getattr(getattr(b, pn), f))


def test_same_order_as_build_batch():
    lens = np.asarray([2, 0, 3, 2, 3, 1, 0, 2])
    np.testing.assert_array_equal(G.length_order(lens), np.argsort(-lens, kind='stable'))
    hist = [[np.asarray([1, 2])] * n for n in lens]
    nb = G.NeighbourBatch(np.arange(8), np.zeros(8, np.int64), hist, seq_len=3)
    np.testing.assert_array_equal(nb.perm, G.length_order(lens))
    assert nb.nseq == 6


def test_history_longer_than_seq_len_raises():
    hist = [[np.asarray([1, 2]), np.asarray([3]), np.asarray([4])], [np.asarray([5])]]
    with pytest.raises(ValueError, match='longer than seq_len'):
        G.NeighbourBatch([0, 1], [0, 0], hist, seq_len=2)
    assert G.NeighbourBatch([0, 1], [0, 0], hist, seq_len=3).L == 3
    agg = _make('mean', 100, seq_len=2)
    with pytest.raises(ValueError, match='longer than seq_len'):
        agg(hist, torch.tensor([0, 1]), torch.tensor([0, 0]), torch.zeros(8, 100), torch.zeros(2, 100))


def test_ids_must_fit_int32_and_steps_must_not_be_empty():
    with pytest.raises(ValueError, match='int32'):
        G.NeighbourBatch([0], [0], [[np.asarray([2 ** 31])]])
    with pytest.raises(ValueError, match='int32'):
        G.NeighbourBatch([0], [0], [[np.asarray([-1])]])
    with pytest.raises(ValueError, match='without neighbours'):
        G.NeighbourBatch([0], [0], [[np.asarray([], np.int64)]])


def test_all_empty_histories_give_none_without_a_device():
    for kind in KINDS:
        agg = _make(kind, 100)
        out = agg([[], [], []], torch.tensor([0, 1, 2]), torch.tensor([0, 0, 1]), torch.zeros(8, 100), torch.zeros(2, 100))
        assert out is None and agg.last_batch is None


def test_new_entries_are_declared_and_bound():
    import renet_hip as K
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'renet_hip.h')).read(), flags=re.S)
    for name, nargs in (('renet_nbr_pool_fwd', 19), ('renet_nbr_pool_bwd', 22)):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name + ' is not declared in include/renet_hip.h'
        assert len(m.group(1).split(',')) == nargs == len(K._SIGNATURES[name][1])
        assert name in K.EXPORTS
    assert callable(K.nbr_pool_fwd) and callable(K.nbr_pool_bwd)
