"""CPU tests of the host side of the event forecasts under observed history: the C ABI entries of csrc/joint_rank.hip in the
header / binding / build list, the public entry points on RENet, and the errors they raise before any use of the device (the
kernels: tests/test_gpu_joint_rank.py; the passes: tests/test_gpu_event_forecast.py)."""
import os
import types

import numpy as np
import pytest

from helpers import ROOT


def test_joint_rank_entries_are_declared_bound_and_built():
    import build
    import renet_hip as K
    from ctypes import c_int, c_void_p
    hdr = open(os.path.join(ROOT, 'include', 'renet_hip.h')).read()
    assert 'int renet_joint_row_offsets(const float* scores, int ld, int G, int R, int C, const float* logits_r, int ld_r,' in hdr
    assert 'int renet_joint_rank_rows(const float* scores, int ld, int G, int C, int R, const float* off, int Q,' in hdr
    assert 'renet_joint_row_offsets' in K.EXPORTS and 'renet_joint_rank_rows' in K.EXPORTS
    restype, argtypes = K._SIGNATURES['renet_joint_row_offsets']
    # scores, ld, G, R, C | logits_r, ld_r | off_out | the stream handle, last
    assert restype is c_int and argtypes == [c_void_p] + [c_int] * 4 + [c_void_p, c_int] + [c_void_p] * 2
    restype, argtypes = K._SIGNATURES['renet_joint_rank_rows']
    # scores, ld, G, C, R | off, Q | group, gold_r, gold_c | list a: cols, start, count, len | list t | counts, at_gold,
    # listed | the stream handle
    assert restype is c_int and argtypes == [c_void_p] + [c_int] * 4 + [c_void_p, c_int] + [c_void_p] * 3 + \
        ([c_void_p] * 3 + [c_int]) * 2 + [c_void_p] * 4
    for name in ('renet_joint_row_offsets', 'renet_joint_rank_rows'):
        defining = [s for s in build.sources() if 'int %s(' % name in open(s).read()]
        assert len(defining) == 1 and os.path.basename(defining[0]) == 'joint_rank.hip', (name, defining)
    assert callable(K.joint_row_offsets) and callable(K.joint_rank_rows)


def test_the_three_entry_points_exist_on_renet():
    import model as M
    for name in ('observed_event_scores', 'evaluate_events_observed', 'predict_events_observed'):
        assert callable(getattr(M.RENet, name)), name


class _Reached(Exception):
    pass


class _Store(object):
    """Stands in for a resident store up to the first use of the device: reading the quadruples raises _Reached."""
    glob, n_quads = None, 4

    @property
    def quads(self):
        raise _Reached()


def _stub():
    class Params(object):
        @property
        def device(self):
            raise _Reached()
    return types.SimpleNamespace(num_rels=5, in_dim=50, h_dim=100, ent_embeds=Params(), training=False, drop_p=0.0)


def test_setting_names_are_exactly_model_settings():
    import model as M
    idx = np.arange(3)
    for name in M.SETTINGS:                                  # accepted: the call gets as far as the device
        with pytest.raises(_Reached):
            M._predict_events_observed(_stub(), _Store(), idx, 3, None, name)
    for name in ('time', 'filter', 'RAW', '', None):
        with pytest.raises(ValueError, match='setting must be one of'):
            M._predict_events_observed(_stub(), _Store(), idx, 3, None, name)
    # the same text as predict_topk_observed
    with pytest.raises(ValueError) as mine:
        M._predict_events_observed(_stub(), _Store(), idx, 3, None, 'best')
    with pytest.raises(ValueError) as theirs:
        M._predict_topk_observed(_stub(), _Store(), idx, 3, None, 'best')
    assert str(mine.value) == str(theirs.value)


def test_a_stream_that_is_not_resident_is_refused_before_any_device_use():
    import model as M
    stream = types.SimpleNamespace(device=None)              # a preprocess.ObservedStream before resident()
    with pytest.raises(ValueError) as want:
        M._observed_store(stream)
    for call in (lambda: M._observed_event_scores(_stub(), stream, np.arange(3)),
                 lambda: M._evaluate_events_observed(_stub(), stream, np.arange(3)),
                 lambda: M._predict_events_observed(_stub(), stream, np.arange(3))):
        with pytest.raises(ValueError) as got:
            call()
        assert str(got.value) == str(want.value) and 'not resident' in str(got.value)


def test_positions_and_block_size_are_checked_on_the_host():
    import model as M
    with pytest.raises(ValueError, match='positions outside the stream'):
        M._evaluate_events_observed(_stub(), _Store(), np.array([0, 4]))
    with pytest.raises(ValueError, match='positions outside the stream'):
        M._observed_event_scores(_stub(), _Store(), np.array([], dtype=np.int64))
    # 3 positions x 5 relations x 50 entities = 750 floats per direction
    with pytest.raises(ValueError, match='exceed block_floats'):
        M._observed_event_scores(_stub(), _Store(), np.arange(3), block_floats=749)
