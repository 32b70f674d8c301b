"""CPU tests of the host side of the device-ranked evaluation: the resident filter index (filter_index.FilterIndex) against
the per-call formulation it replaces (model._known_pairs), its cache, the C ABI entry of the rank kernel in the header and
the build list, and utils.rank_metrics against hand-computed figures."""
import os
import types

import numpy as np
import pytest
import torch

from helpers import ROOT


def _facts():
    """Synthetic all_triplets [m, 4] over 9 entities / 3 relations: random facts, every one of them repeated at later
    timestamps, plus hand-placed ones: (7, 2, 8) is the ONLY fact of the keys (7, 2) and (8, 2)."""
    rng = np.random.RandomState(5)
    base = np.stack((rng.randint(0, 6, 60), rng.randint(0, 2, 60), rng.randint(0, 6, 60)), axis=1)
    rows = [np.concatenate((base, np.full((60, 1), t)), axis=1) for t in (0, 24, 48)]
    rows.append(np.array([[7, 2, 8, 0], [7, 2, 8, 24]]))
    at = np.concatenate(rows).astype(np.int64)
    return at[rng.permutation(len(at))]


def _expected(at, key_cols, val_col, keys):
    """model._known_pairs, deduplicated and sorted per row -> list of n int lists."""
    import model as M
    rows, vals = M._known_pairs(at, key_cols, val_col, keys)
    return [sorted(set(vals[rows == i].tolist())) for i in range(len(keys))]


@pytest.mark.parametrize('as_tensor', [False, True])
def test_lookups_equal_known_pairs_deduplicated(as_tensor):
    import filter_index as FI
    at = _facts()
    idx = FI.FilterIndex(torch.from_numpy(at) if as_tensor else at)
    # queries: every (s, r) / (o, r) combination of the id range (many without a single fact), repeated keys, the key whose
    # only match is the query's own label, and an entity beyond anything the index has seen (a RELATION beyond the indexed
    # range has no list here either, but _known_pairs' key code aliases it onto another key: not a comparison)
    grid = np.stack(np.meshgrid(np.arange(9), np.arange(3), indexing='ij'), axis=-1).reshape(-1, 2)
    keys = np.concatenate((grid, grid[:4], [[7, 2], [8, 2], [40, 1]])).astype(np.int64)
    for side, key_cols, val_col in (('o', (0, 1), 2), ('s', (2, 1), 0)):
        row_ptr, cols = idx.lists_host(side, keys)
        want = _expected(at, key_cols, val_col, keys)
        assert row_ptr.shape == (len(keys) + 1,) and row_ptr[0] == 0 and row_ptr[-1] == len(cols)
        assert cols.dtype == np.int32
        got = [cols[row_ptr[i]:row_ptr[i + 1]].tolist() for i in range(len(keys))]
        assert got == want
        assert any(len(g) == 0 for g in got) and any(len(g) > 1 for g in got)
        # repeated (s, r, o) at three timestamps: the raw lists are longer than the deduplicated ones
        import model as M
        assert len(M._known_pairs(at, key_cols, val_col, keys)[1]) > len(cols)
    # the key whose only match is the label itself: one listed column, the label
    i = len(grid) + 4
    assert idx.lists_host('o', keys[i:i + 1])[1].tolist() == [8]           # objects of (7, 2)
    assert idx.lists_host('s', keys[i + 1:i + 2])[1].tolist() == [7]       # subjects of (8, 2)
    assert idx.lists_host('o', np.array([[3, 11], [-1, 0]]))[0].tolist() == [0, 0, 0]
    # no query at all
    row_ptr, cols = idx.lists_host('o', np.zeros((0, 2), dtype=np.int64))
    assert row_ptr.tolist() == [0] and len(cols) == 0


def test_empty_fact_array_gives_empty_lists():
    import filter_index as FI
    idx = FI.FilterIndex(np.zeros((0, 4), dtype=np.int64))
    row_ptr, cols = idx.lists_host('s', np.array([[0, 0], [3, 1]]))
    assert row_ptr.tolist() == [0, 0, 0] and len(cols) == 0


def test_ids_must_fit_int32():
    import filter_index as FI
    with pytest.raises(ValueError):
        FI.FilterIndex(np.array([[0, 0, 2 ** 31, 0]], dtype=np.int64))
    with pytest.raises(ValueError):
        FI.FilterIndex(np.array([[0, -1, 3, 0]], dtype=np.int64))


def test_index_is_cached_by_identity():
    import filter_index as FI
    owner = types.SimpleNamespace()
    at = torch.from_numpy(_facts())
    a = FI.filter_index_for(owner, at)
    assert FI.filter_index_for(owner, at) is a                            # the same object: the cached index
    other = at.clone()                                                     # equal content, a different object: rebuilt,
    b = FI.filter_index_for(owner, other)                                  # and the first one is released
    assert b is not a and owner._filter_index[0] is other
    assert FI.filter_index_for(owner, other) is b
    other[0, 2] = 5                                                        # written in place: not the facts it indexed
    assert FI.filter_index_for(owner, other) is not b
    arr = _facts()                                                         # numpy arrays are keyed the same way
    c = FI.filter_index_for(owner, arr)
    assert FI.filter_index_for(owner, arr) is c and FI.filter_index_for(owner, arr.copy()) is not c


def test_model_carries_the_switch_default_off(monkeypatch):
    import model as M
    monkeypatch.delenv('RENET_DEVICE_RANK', raising=False)
    net = M.RENet(7, 100, 3, dropout=0.0, seq_len=3, num_k=2)
    assert net.device_rank is False
    monkeypatch.setenv('RENET_DEVICE_RANK', '1')
    assert M.RENet(7, 100, 3, dropout=0.0, seq_len=3, num_k=2).device_rank is True
    for name in ('evaluate_batch', 'evaluate_stream'):
        assert callable(getattr(net, name))


def test_rank_entry_is_declared_bound_and_built():
    import build
    import renet_hip as K
    hdr = open(os.path.join(ROOT, 'include', 'renet_hip.h')).read()
    assert 'int renet_rank_rows(const float* scores, int ld, int n, int C, const int32_t* label,' in hdr
    assert 'renet_rank_rows' in K.EXPORTS
    assert 'rank.hip' in [os.path.basename(s) for s in build.sources()]


def test_rank_metrics_on_a_hand_written_array():
    import utils as U
    ranks = np.array([[1.0, 2.0], [4.0, 10.0], [1.5, 20.0]])              # (rank_sub, rank_ob) of three quadruples
    m = U.rank_metrics(ranks)
    assert m['mrr'] == pytest.approx((1 + 1 / 2 + 1 / 4 + 1 / 10 + 1 / 1.5 + 1 / 20) / 6, rel=1e-12)
    assert m['mr'] == pytest.approx(38.5 / 6, rel=1e-12)
    assert m['hits@1'] == pytest.approx(1 / 6) and m['hits@3'] == pytest.approx(3 / 6)
    assert m['hits@10'] == pytest.approx(5 / 6)
    assert sorted(m) == ['hits@1', 'hits@10', 'hits@3', 'mr', 'mrr']
