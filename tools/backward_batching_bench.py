#!/usr/bin/env python
"""The small reductions of the encoder backward on the bench workload's merged batch (ICEWS18-shaped, batch 1024 per
direction, n_hidden 200): the call sequences of the unbatched launch list against the batched calls of RENET_STEP_BATCH
(csrc/step.cpp), us per sequence by device events, and the time the bytes alone would take at the chip's achievable
bandwidth (6.3 TB/s, a float4 copy).

  segmented adds   add_inplace, 2 x segment_add (head), zero, 3 x segment_add (sequence side)
                                                                    vs  ONE renet_segment_add_multi of 3 jobs
  W_hh splits      renet_gru_split_weights forward / backward (2 launches each; what leaves the main stream)

   python tools/backward_batching_bench.py [iterations, default 200]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))
import graph as G            # noqa: E402
import preprocess as P       # noqa: E402
import renet_hip as K        # noqa: E402
import synth                 # noqa: E402

ACHIEVABLE_TBS = 6.3


def timed(fn, iters):
    """us per call by device events; warns where the host needed as long to enqueue (the figure is then the host's)"""
    import time
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = (time.perf_counter() - t0) * 1e6 / iters
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    if host > 0.9 * us:
        print('   (host-bound: %.1f us to enqueue, %.1f us by events)' % (host, us), flush=True)
    return us


def report(name, us_old, us_new, nbytes):
    floor = nbytes / (ACHIEVABLE_TBS * 1e6)
    print('%-16s unbatched %7.1f us   batched %7.1f us   %6.1f MB -> %5.1f us at %.1f TB/s   (batched = %.1fx the bytes'' time)'
          % (name, us_old, us_new, nbytes / 1e6, floor, ACHIEVABLE_TBS, us_new / floor), flush=True)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    K.lib()
    dev = torch.device('cuda:0')
    quads, ne, nr, _ = synth.make_stream('ICEWS18', seed=999)
    gd = P.build_graph_dict(quads, nr)
    hs, ho = P.HistoryIndex(quads, 's', 10), P.HistoryIndex(quads, 'o', 10)
    idx = np.random.RandomState(999).permutation(len(quads))[3 * 1024:4 * 1024]
    hb = G.build_batch_both(G.store_for(gd), ne, nr, quads[idx, 0], quads[idx, 1], quads[idx, 2], hs.take(idx), ho.take(idx))
    g = G.DeviceGraph(G.PackedBatch(hb), dev)
    d, S, B, nA = 200, hb.S, hb.B, g.nA
    print('S %d packed rows, B %d sequences, nA %d rows of layer 2; segments: subj_row %d, s %d, r %d'
          % (S, B, nA, g.plan_subj_row.num_segments, g.plan_s.num_segments, g.plan_r.num_segments), flush=True)
    rn = lambda *s: torch.randn(*s, device=dev)

    # ---- segmented adds
    da1, da2, dc1 = rn(B, d), rn(B, d), rn(B, d)
    d_rows, d_ent_seq, d_rel_seq = rn(S, d), rn(B, d), rn(B, d)
    cover = g.plan_subj_row.num_segments == nA

    def seg_old(g_ent, g_rel, d_h2, scratch):
        scratch.copy_(da1)                                          # (the step's da1 is fresh every step; keep ours)
        K.lib().renet_add_inplace(scratch.data_ptr(), da2.data_ptr(), scratch.numel(), K._stream())
        K.segment_add(scratch, g.plan_s, g_ent)
        K.segment_add(dc1, g.plan_r, g_rel)
        K.lib().renet_zero(d_h2.data_ptr(), d_h2.numel(), K._stream())
        K.segment_add(d_rows, g.plan_subj_row, d_h2)
        K.segment_add(d_ent_seq, g.plan_s, g_ent)
        K.segment_add(d_rel_seq, g.plan_r, g_rel)

    def seg_new(g_ent, g_rel, d_h2):
        if not cover:
            K.lib().renet_zero(d_h2.data_ptr(), d_h2.numel(), K._stream())
        rc = K.segment_add_multi([(g.plan_r, g_rel, dc1, None, d_rel_seq, False), (g.plan_s, g_ent, da1, da2, d_ent_seq, False),
                                  (g.plan_subj_row, d_h2, d_rows, None, None, cover)])
        assert rc == 0, rc
    ge0, gr0 = rn(ne, d), rn(2 * nr, d)
    bufs = [(ge0.clone(), gr0.clone(), torch.full((nA, d), float('nan'), device=dev)) for _ in range(2)]
    scratch = torch.empty_like(da1)
    seg_old(*bufs[0], scratch), seg_new(*bufs[1])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*bufs)), 'segment_add_multi differs from the calls it replaces'
    nbytes = (S + 5 * B) * d * 4 + 2 * (2 * g.plan_s.num_segments + 2 * g.plan_r.num_segments) * d * 4 \
        + g.plan_subj_row.num_segments * d * 4
    us_copy = timed(lambda: scratch.copy_(da1), iters)
    us_old = timed(lambda: seg_old(*bufs[0], scratch), iters) - us_copy
    report('segmented adds', us_old, timed(lambda: seg_new(*bufs[1]), iters), nbytes)
    print('                 (d_h2 %s; the unbatched time excludes the %.1f us copy that restores da1)'
          % ('overwritten: the plan names all its rows' if cover else 'zeroed first: the plan does not name all its rows', us_copy))

    # ---- the W_hh splits
    whh = [rn(3 * d, d) * 0.1, rn(3 * d, d) * 0.1]
    nb = 2 * K.lib().renet_gru_workspace(0, d)
    gws = torch.empty(nb // 4, device=dev)
    for back in (False, True):
        us = timed(lambda: K.gru_split_weights(whh, d, back, gws, nb), iters)
        print('W_hh splits %-8s 2 launches %5.1f us (leave the main stream)' % ('backward' if back else 'forward', us), flush=True)


if __name__ == '__main__':
    main()
