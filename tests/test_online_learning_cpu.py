"""Host tests of the online-learning protocol (re-net_amd/online.py): the CSR targets of the global model's learn step are
the CLEAN per-timestamp distributions of the stream, and they differ from utils.get_true_distribution exactly in that
function's documented off-by-one.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 're-net_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import observed_stream as S


def _stream():
    import preprocess as P
    splits = S.make()
    return P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)


def _counts(allq, col):
    out = np.zeros((S.NUM_T, S.NUM_ENT))
    np.add.at(out, (allq[:, 3], allq[:, col]), 1.0)
    return out


def test_csr_targets_are_the_clean_per_timestamp_distributions():
    import online
    obs = _stream()
    times = obs.times[::-1]                                  # any order: rows follow `times`
    csr = online.stream_targets(obs.graph_dict, times, S.NUM_ENT)
    for role, col in (('s', 0), ('o', 2)):
        ptr, cols, w = csr[role]
        assert ptr.dtype == np.int64 and w.dtype == np.float32 and ptr[0] == 0 and ptr[-1] == len(cols) == len(w)
        for a, b in zip(ptr[:-1], ptr[1:]):
            assert b > a and np.all(np.diff(cols[a:b]) > 0)   # distinct, ascending
        counts = _counts(obs.allq, col)[times]
        want = (counts / counts.sum(axis=1, keepdims=True)).astype(np.float32)
        got = online.dense_targets(csr[role], S.NUM_ENT)
        assert np.array_equal(got, want.astype(np.float64))
        assert np.allclose(got.sum(axis=1), 1.0, atol=1e-6)
    # a repeated timestamp gives a repeated row; an unknown one is an error
    twice = online.stream_targets(obs.graph_dict, [3, 3], S.NUM_ENT)['s']
    d = online.dense_targets(twice, S.NUM_ENT)
    assert np.array_equal(d[0], d[1])
    with pytest.raises(KeyError):
        online.stream_targets(obs.graph_dict, [S.NUM_T + 5], S.NUM_ENT)


def test_they_differ_from_get_true_distribution_exactly_in_its_off_by_one():
    """utils.get_true_distribution counts a fact BEFORE it tests for a new timestamp: the first fact of timestamp k + 1 lands
    in row k (and is missing from row k + 1), and the last row stays un-normalised.  Rebuilding that from the clean counts
    gives its rows bit for bit -- and the clean rows are not its rows."""
    import online
    import utils as U
    obs = _stream()
    allq = obs.allq
    ref_s, ref_o = U.get_true_distribution(allq, S.NUM_ENT)
    assert ref_s.shape == (S.NUM_T, S.NUM_ENT)
    first = np.searchsorted(allq[:, 3], np.arange(S.NUM_T))            # position of every timestamp's first fact
    csr = online.stream_targets(obs.graph_dict, obs.times, S.NUM_ENT)
    for role, col, ref in (('s', 0, ref_s), ('o', 2, ref_o)):
        counts = _counts(allq, col)
        shifted = counts.copy()
        for k in range(1, S.NUM_T):
            e = allq[first[k], col]
            shifted[k, e] -= 1.0
            shifted[k - 1, e] += 1.0
        shifted[:-1] /= shifted[:-1].sum(axis=1, keepdims=True)
        assert np.array_equal(shifted, ref)
        clean = online.dense_targets(csr[role], S.NUM_ENT)
        assert abs(ref[-1].sum() - 1.0) > 1.0 and abs(clean[-1].sum() - 1.0) < 1e-6
        differing = [k for k in range(S.NUM_T) if not np.allclose(clean[k], ref[k], atol=1e-6)]
        assert len(differing) >= S.NUM_T - 2, differing


def test_the_protocol_is_bound_where_the_issue_places_it():
    import global_model as GM
    import model as M
    import preprocess as P
    import renet_hip as K
    assert callable(M.RENet.learn_observed) and callable(M.RENet.evaluate_online)
    assert callable(GM.RENet_global.learn_observed) and callable(P.ObservedStream.refresh_global)
    assert 'renet_soft_ce_sparse' in K._SIGNATURES and len(K._SIGNATURES['renet_soft_ce_sparse'][1]) == 11
    hdr = open(os.path.join(ROOT, 'include', 'renet_hip.h')).read()
    assert 'int renet_soft_ce_sparse(' in hdr
    with pytest.raises(ValueError):
        _stream().refresh_global(None)                       # not resident
