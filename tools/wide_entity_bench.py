#!/usr/bin/env python
"""The kernels that serve entity sets beyond 32768 (csrc/topk_rows.hip: renet_topk_rows_wide; csrc/topk.hip: the streaming
renet_joint_softmax) against the torch formulation on the same device and against one read of the matrix at copy bandwidth.
GPU only; every figure the median of five after a warm-up, with min and max; one JSON line (profiles/wide_entity_sets.md).

    python tools/wide_entity_bench.py [rows]        rows of the top-k matrices (default 4096)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))

COPY_TBS = 6.29                 # what a float4 copy reaches on the device, TB/s (profiles/topk_rows.md)
REPS = 5
LISTED = 64                     # listed columns per row


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _times(fn):
    fn()                                                        # warm-up
    t = [_wall(fn) for _ in range(REPS)]
    return {'median_ms': 1e3 * float(np.median(t)), 'min_ms': 1e3 * min(t), 'max_ms': 1e3 * max(t)}


def _lists(n, C, dev):
    """LISTED random columns per row (a repeat is harmless to both sides) as one resident table -> (cols, start, count), and
    the (row, column) pairs of it."""
    g = torch.Generator().manual_seed(1)
    cols = torch.randint(0, C, (n, LISTED), generator=g).int()
    start = (torch.arange(n) * LISTED).int()
    count = torch.full((n,), LISTED, dtype=torch.int32)
    rows = torch.arange(n).repeat_interleave(LISTED)
    return tuple(t.to(dev) for t in (cols.view(-1), start, count)), (rows.to(dev), cols.view(-1).long().to(dev))


def topk_case(K, fn, n, C, k, dev, with_lists):
    x = torch.randn(n, C, device=dev) * 8
    table, (rows, cols) = _lists(n, C, dev) if with_lists else ((None, None, None), (None, None))

    def torch_way():
        s = x
        if with_lists:
            s = x.clone()
            s[rows, cols] = -np.inf
        lp = torch.log_softmax(x, dim=1)
        v, i = torch.topk(s, k, dim=1)
        return i, v, lp.gather(1, i)
    got = fn(x, k, *table)
    want = torch_way()
    same = bool(torch.equal(got[1], want[1]))                  # values (torch leaves the order among ties open)
    res = {'n': n, 'C': C, 'k': k, 'lists': with_lists, 'values_equal_torch': same, 'kernel': _times(lambda: fn(x, k, *table)),
           'torch': _times(torch_way), 'one_read_at_copy_bandwidth_ms': 1e3 * n * C * 4.0 / (COPY_TBS * 1e12)}
    res['kernel_over_one_read'] = res['kernel']['median_ms'] / res['one_read_at_copy_bandwidth_ms']
    res['torch_over_kernel'] = res['torch']['median_ms'] / res['kernel']['median_ms']
    return res


def joint_case(K, n, R, N, dev):
    logits = torch.randn(n * R, N, device=dev) * 3
    lr = torch.randn(n, R, device=dev) * 2
    prob = torch.rand(n, device=dev) * 1e-3 + 1e-5
    work = logits.clone()

    def torch_way():
        return (torch.softmax(logits, dim=1) * torch.softmax(lr, dim=1).reshape(n * R, 1)).view(n, R * N) * prob.view(n, 1)
    want = torch_way()
    got = K.joint_softmax(logits.clone(), R, lr, prob).view(n, R * N)
    res = {'n': n, 'R': R, 'N': N, 'largest_relative_difference_to_torch': float(((got - want).abs() / want).max()),
           'kernel_in_place': _times(lambda: K.joint_softmax(work, R, lr, prob)), 'torch': _times(torch_way),
           'one_read_one_write_at_copy_bandwidth_ms': 1e3 * 2.0 * n * R * N * 4.0 / (COPY_TBS * 1e12)}
    res['torch_over_kernel'] = res['torch']['median_ms'] / res['kernel_in_place']['median_ms']
    return res


def main():
    import renet_hip as K
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    dev = torch.device('cuda:0')
    out = {'reps': REPS, 'listed_per_row': LISTED, 'wide': [], 'at_23033': {}}
    for C in (65536, 262144):
        for k in (10, 1000):
            for with_lists in (False, True):
                out['wide'].append(topk_case(K, K.topk_rows_wide, n, C, k, dev, with_lists))
                torch.cuda.empty_cache()
    for k in (10, 1000):
        for name, fn in (('narrow', K.topk_rows), ('wide', K.topk_rows_wide)):
            out['at_23033']['%s k %d' % (name, k)] = topk_case(K, fn, n, 23033, k, dev, True)
    out['joint_softmax'] = joint_case(K, 32, 8, 65536, dev)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
