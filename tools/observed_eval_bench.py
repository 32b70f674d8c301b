#!/usr/bin/env python
"""Rate of the observed-history evaluation pass (RENet.evaluate_observed) and of the multi-step pass
(RENet.evaluate_all_stream) over the SAME ICEWS18-shaped synthetic test stream (tools/infer_bench.py's setup: 40 training
timestamps + n_t evaluated ones, hidden 200, seq_len 10).  GPU only; one JSON line per mode (profiles/observed_eval.md).

    python tools/observed_eval_bench.py multistep [n_t] [reps]   evaluate_all_stream, a fresh model per pass (a pass advances
                                                                 the inference state); uses no API younger than that pass
    python tools/observed_eval_bench.py observed [n_t] [reps]    evaluate_observed, repeated in place, + the stage split"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import infer_bench

SHAPE, HIDDEN = 'ICEWS18', 200


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _spread(n, times):
    return {'median_s': float(np.median(times)), 'min_s': float(np.min(times)), 'max_s': float(np.max(times)),
            'quadruples_per_s': n / float(np.median(times)), 'passes_s': [round(x, 4) for x in times]}


def multistep(n_t=24, reps=3):
    dev = torch.device('cuda:0')
    times = []
    for rep in range(reps + 1):                                 # pass 0 warms up
        net, gnet, te, tes, teo, total = infer_bench.setup(SHAPE, n_t, HIDDEN, dev)
        with torch.no_grad():
            dt, (ranks, _) = _wall(lambda: net.evaluate_all_stream(te, tes, teo, gnet, total))
        if rep:
            times.append(dt)
    print(json.dumps(dict(mode='multistep evaluate_all_stream', shape=SHAPE, timestamps=n_t, quadruples=len(te), reps=reps,
                          mrr_time_filtered=float(np.mean(1.0 / ranks['time_filtered'])), **_spread(len(te), times))))


def _observed_setup(n_t, dev):
    import preprocess as P
    net, gnet, te, tes, teo, total = infer_bench.setup(SHAPE, n_t, HIDDEN, dev)      # the same weights and stream
    quads = total.cpu().numpy()
    tr = quads[:len(quads) - len(te)]
    dt, obs = _wall(lambda: P.ObservedStream((tr, te), net.in_dim, net.num_rels, net.seq_len))
    dt2, _ = _wall(lambda: obs.resident(net, gnet))
    return net, obs, obs.positions('test'), {'index_s': dt, 'resident_s': dt2}


def _stages(net, obs, idx, max_batch):
    """One pass with a device synchronisation after every stage (slower than the pass itself: the stages do not overlap
    here): seconds per stage, summed over the batches."""
    import filter_index as FI
    import model as M
    import renet_hip as K
    store, dev = obs.device, net.ent_embeds.device
    t = {'host lookups + upload': 0.0, 'builder': 0.0, 'encoder (RGCN x2, assembly, GRU x2)': 0.0, 'row assembly': 0.0,
         'score GEMMs': 0.0, 'rank (rank_rows3 x2)': 0.0}

    def timed(key, fn):
        dt, out = _wall(fn)
        t[key] += dt
        return out
    tr = store.quads[idx]
    s, r, o, tt = tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3]

    def lookups():
        index = FI.filter_index_for(store, store.quads)
        lists = np.stack(index.ranges_both_host('s', np.stack((o, r, tt), axis=1)) +
                         index.ranges_both_host('o', np.stack((s, r, tt), axis=1)) + (s, o)).astype(np.int32)
        return index, torch.from_numpy(lists).to(dev)
    index, up = timed('host lookups + upload', lookups)
    cols = {side: (index.resident(side, dev), index.resident(side, dev, timed=True)) for side in ('s', 'o')}
    real_encode, real_gru, real_rows = net.aggregator.encode, M.ops.dual_gru, M._eval_rows_torch
    import gpu_builder
    net.aggregator.encode = lambda *a, **k: timed('encoder (RGCN x2, assembly, GRU x2)', lambda: real_encode(*a, **k))
    M.ops.dual_gru = lambda *a, **k: timed('encoder (RGCN x2, assembly, GRU x2)', lambda: real_gru(*a, **k))
    M._eval_rows_torch = lambda *a, **k: timed('row assembly', lambda: real_rows(*a, **k))

    def chunks():                                               # (the capacities are settled: finalize() accepts)
        for c in range(0, len(idx), gpu_builder.MAX_BOTH):
            def build():
                pending = M._observed_launch(net, store, idx[c:c + gpu_builder.MAX_BOTH])
                assert pending[1].finalize()
                return pending
            yield M._observed_features(net, store, timed('builder', build))
    try:
        with torch.no_grad():
            for c, d, (feat_ob, feat_sub, _, _) in M._observed_cuts(chunks(), max_batch):
                preds = timed('score GEMMs', lambda: (M._linear_eval(net.linear, feat_sub), M._linear_eval(net.linear, feat_ob)))
                timed('rank (rank_rows3 x2)', lambda: [
                    K.rank_rows3(pred, up[8 + k][c:d], cols[side][0], up[b][c:d], up[b + 1][c:d], cols[side][1], up[b + 2][c:d],
                                 up[b + 3][c:d]) for k, (side, pred, b) in enumerate((('s', preds[0], 0), ('o', preds[1], 4)))])
    finally:
        net.aggregator.encode, M.ops.dual_gru, M._eval_rows_torch = real_encode, real_gru, real_rows
    return {k: round(v, 5) for k, v in t.items()}


def observed(n_t=24, reps=3, max_batch=4096):
    dev = torch.device('cuda:0')
    net, obs, idx, setup_s = _observed_setup(n_t, dev)
    times = []
    for rep in range(reps + 1):                                 # pass 0 warms up (and raises the builder's capacities)
        dt, (ranks, _) = _wall(lambda: net.evaluate_observed(obs, idx, max_batch=max_batch))
        if rep:
            times.append(dt)
    _stages(net, obs, idx, max_batch)
    print(json.dumps(dict(mode='observed evaluate_observed', shape=SHAPE, timestamps=n_t, quadruples=len(idx), reps=reps,
                          max_batch=max_batch, setup=setup_s, mrr_time_filtered=float(np.mean(1.0 / ranks['time_filtered'])),
                          stages_synchronised_s=_stages(net, obs, idx, max_batch), **_spread(len(idx), times))))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'observed'
    args = [int(x) for x in sys.argv[2:]]
    {'multistep': multistep, 'observed': observed}[mode](*args)
