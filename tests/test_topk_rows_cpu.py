"""CPU tests of the host side of the ranked top-k predictions: the C ABI entry of renet_topk_rows in the header / binding / build
list, the public entry points on RENet and the setting names they accept (the kernel itself: tests/test_gpu_topk_rows.py)."""
import os
import types

import numpy as np
import pytest

from helpers import ROOT


def test_topk_rows_entry_is_declared_bound_and_built():
    import build
    import model as M
    import renet_hip as K
    from ctypes import c_int, c_void_p
    hdr = open(os.path.join(ROOT, 'include', 'renet_hip.h')).read()
    assert 'int renet_topk_rows(const float* scores, int ld, int n, int C, int k,' in hdr
    assert 'renet_topk_rows' in K.EXPORTS
    restype, argtypes = K._SIGNATURES['renet_topk_rows']
    # scores, ld, n, C, k | cols, start, count, len | keep | out_idx, out_val, out_logp, out_n | the stream handle, last
    assert restype is c_int and argtypes == [c_void_p] + [c_int] * 4 + [c_void_p] * 3 + [c_int] + [c_void_p] * 6
    defining = [s for s in build.sources() if 'int renet_topk_rows(' in open(s).read()]
    assert len(defining) == 1
    assert callable(K.topk_rows)
    for name in ('predict_topk_batch', 'predict_topk_stream'):
        assert callable(getattr(M.RENet, name))


class _Reached(Exception):
    pass


def _stub():
    """Stands in for a RENet up to the first use of the device: predict_batch raises _Reached."""
    def predict_batch(*a, **k):
        raise _Reached()
    return types.SimpleNamespace(predict_batch=predict_batch)


def test_setting_names_are_exactly_model_settings():
    import model as M
    quads = np.array([[0, 0, 1, 24], [1, 0, 2, 24]], dtype=np.int64)
    facts = np.array([[0, 0, 1, 0], [0, 0, 2, 24], [1, 0, 2, 24]], dtype=np.int64)
    hist = ([[], []], [[], []])
    assert M.SETTINGS == ('raw', 'filtered', 'time_filtered')
    for name in M.SETTINGS:                                  # accepted: the call gets as far as the scores
        with pytest.raises(_Reached):
            M._predict_topk_batch(_stub(), quads, hist, hist, None, 3, facts, name)
    for name in ('time', 'filter', 'RAW', '', None):
        with pytest.raises(ValueError, match='setting must be one of'):
            M._predict_topk_batch(_stub(), quads, hist, hist, None, 3, facts, name)
    # a filtered setting needs the known facts; the raw one does not
    for name in ('filtered', 'time_filtered'):
        with pytest.raises(ValueError, match='all_triplets'):
            M._predict_topk_batch(_stub(), quads, hist, hist, None, 3, None, name)
    with pytest.raises(_Reached):
        M._predict_topk_batch(_stub(), quads, hist, hist, None, 3, None, 'raw')
