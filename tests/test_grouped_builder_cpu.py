"""CPU tests of the grouped device builder's host side: the ctypes mirror of RenetGroupedStoreDev against the header, the
switch and its fall-back when the tensors are not on a HIP device."""
import os
import re

import numpy as np
import torch

from test_host_cpu import ROOT, _header_struct


def test_grouped_store_mirror_matches_the_header():
    import ctypes
    import gpu_builder as GB
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'renet_hip.h')).read(), flags=re.S)
    want = _header_struct(hdr, 'RenetGroupedStoreDev')
    assert len(want) == 23
    got = [(f, 'ptr' if t is ctypes.c_void_p else 'int', 0) for f, t in GB._GroupedStoreDev._fields_]
    assert all(t in (ctypes.c_void_p, ctypes.c_int) for _, t in GB._GroupedStoreDev._fields_)
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b]
    import renet_hip as K
    for name in GB._FRONT_GROUPED:
        assert name in K._SIGNATURES
    assert K._SIGNATURES[GB._FRONT_GROUPED[1]] == K._SIGNATURES[GB._FRONT_BOTH[1]]       # _launch calls both alike


def test_switch_follows_the_environment_and_leaves_cpu_tensors_to_the_host_builder(monkeypatch):
    import Aggregator as A
    import graph as G
    import preprocess as P
    import synth
    make = lambda: A.RGCNAggregator(100, 0.0, 50, 4, 100, 'RGCN', seq_len=10)
    monkeypatch.delenv('RENET_GROUPED_DEVICE_BUILDER', raising=False)
    assert make().grouped_device_builder is False
    monkeypatch.setenv('RENET_GROUPED_DEVICE_BUILDER', '1')
    agg = make()
    assert agg.grouped_device_builder is True
    quads, ne, nr, _ = synth.make_stream('YAGO', seed=999, num_t=12)
    gd = P.build_graph_dict(quads, nr)
    idx = np.nonzero(quads[:, 3] == quads[-1, 3])[0][:20]
    fh = P.HistoryIndex(quads, 's', 10).take(idx)
    assert fh.seq_ptr[-1] > 0
    glob = {int(t): torch.zeros(1, 1, 100) for t in gd}
    assert agg.build_grouped_device(fh, quads[idx, 0], quads[idx, 1], torch.zeros(ne, 100), gd, glob, quads[idx, 0]) is None
