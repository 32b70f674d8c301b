#!/usr/bin/env python
"""Micro-benchmark of the neighbour pooling kernels (csrc/nbr_pool.hip) of MeanAggregator / AttnAggregator on an
ICEWS18-shaped synthetic batch (synth.py, seed 999: 1024 sequences, seq_len 10, D = 200), GPU only.

    timeout -k 10 600 python tools/nbr_pool_bench.py [--md profiles/nbr_aggregators.md] [--json out.json]

Baseline: the same mathematics in torch ops on the same GPU (index_select, segment_reduce, index_put) -- all a user of
the package had before these kernels.  Both sides are warmed up, then timed per call with device events, the two sides
alternating; the medians are reported.  Bytes are the ALGORITHMIC bytes: nnz * D * 4 for the gathered rows (x 2 in
attention mode: E and P rows) plus the output (forward) / plus the contribution rows written and the gradient read
(backward); the fraction is of 8 TB/s HBM bandwidth -- an upper bound on what HBM delivers, the tables themselves
(N_ent * D * 4 = 18 MB) sit in the caches.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))
import graph as G            # noqa: E402
import ops                   # noqa: E402
import preprocess as P       # noqa: E402
import renet_hip as K        # noqa: E402
import synth                 # noqa: E402

HBM = 8000.0                 # GB/s, MI355X
B, SEQ, DIM = 1024, 10, 200


def workload(dev):
    quads, ne, nr, _ = synth.make_stream('ICEWS18', seed=999)
    hs = P.HistoryIndex(quads, 's', SEQ)
    idx = np.random.RandomState(999).permutation(len(quads))[3 * B:4 * B]          # bench.py's first timed batch
    nb = G.NeighbourBatch(quads[idx, 0], quads[idx, 1], hs.take(idx), seq_len=SEQ).to(dev)
    return nb, ne, nr


def medians(fns, warmup, reps):
    """fns: {name: callable}; per-call device-event times, the callables alternating -> {name: median microseconds}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in v])) * 1e3 for k, v in ev.items()}


def torch_mean(ent, nb, seg_id, lengths, d):
    rows = ent.index_select(0, nb.nbr.long())
    m = torch.segment_reduce(rows, 'mean', lengths=lengths)
    out = torch.empty(nb.S, 2 * d, device=ent.device)
    out[nb.out_row.long()] = torch.cat((m, ent.index_select(0, nb.seg_s.long())), dim=1)
    return out


def torch_attn(ent, rel, p, q, v, nb, seg_id, lengths, d):
    nbr = nb.nbr.long()
    rows = ent.index_select(0, nbr)
    a = (torch.tanh(p.index_select(0, nbr) + q.index_select(0, nb.seg_q.long()).index_select(0, seg_id)) @ v).view(-1)
    mx = torch.segment_reduce(a.detach(), 'max', lengths=lengths)
    ex = torch.exp(a - mx.index_select(0, seg_id))
    w = ex / torch.segment_reduce(ex, 'sum', lengths=lengths).index_select(0, seg_id)
    pooled = torch.segment_reduce(w.view(-1, 1) * rows, 'sum', lengths=lengths)
    out = torch.empty(nb.S, 3 * d, device=ent.device)
    out[nb.out_row.long()] = torch.cat((pooled, ent.index_select(0, nb.seg_s.long()), rel.index_select(0, nb.seg_r.long())),
                                       dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--json')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nbr_pool_bench needs a HIP device: nothing is measured without one')
    dev = torch.device('cuda:0')
    K.lib()
    nb, ne, nr = workload(dev)
    d = DIM
    torch.manual_seed(0)
    ent = (torch.randn(ne, d, device=dev) * 0.3).requires_grad_(True)
    rel = (torch.randn(2 * nr, d, device=dev) * 0.3).requires_grad_(True)
    p = (torch.randn(ne, d, device=dev) * 0.3).requires_grad_(True)
    q = (torch.randn(nb.nseq, d, device=dev) * 0.3).requires_grad_(True)
    v = (torch.randn(d, 1, device=dev) * 0.2).requires_grad_(True)
    lens_h = np.diff(nb.host.seg_ptr)
    lengths = torch.from_numpy(lens_h.astype(np.int64)).to(dev)
    seg_id = torch.repeat_interleave(torch.arange(nb.S, device=dev), lengths)
    res = {'sequences': B, 'kept': nb.nseq, 'segments': nb.S, 'neighbours': nb.nnz, 'D': d, 'entities': ne,
           'longest_segment': int(lens_h.max()), 'mean_segment': float(lens_h.mean()), 'modes': {}}
    for mode in ('mean', 'attn'):
        attn = mode == 'attn'
        width = (3 if attn else 2) * d
        args_f = (ent, rel, p, q, v) if attn else (ent, None, None, None, None)
        g_out = torch.randn(nb.S, width, device=dev)

        def tfwd():
            return torch_attn(ent, rel, p, q, v, nb, seg_id, lengths, d) if attn else torch_mean(ent, nb, seg_id, lengths, d)

        with torch.no_grad():
            e_d, r_d, p_d, q_d, v_d = (t.detach() if t is not None else None for t in args_f)
            out, stats, w = K.nbr_pool_fwd(e_d, r_d, p_d, q_d, v_d, nb)
            ref = tfwd()
            err = float((out - ref).abs().max())

        def fused_fwd():
            K.nbr_pool_fwd(e_d, r_d, p_d, q_d, v_d, nb)

        def fused_bwd():
            K.nbr_pool_bwd(g_out, out if attn else None, e_d, p_d, q_d, v_d, w, nb)

        def fused_step():
            for t in (ent, rel, p, q, v):
                t.grad = None
            ops.NbrPoolFn.apply(*args_f, nb).backward(g_out)

        def torch_fwd():
            with torch.no_grad():
                tfwd()

        def torch_step():
            for t in (ent, rel, p, q, v):
                t.grad = None
            tfwd().backward(g_out)

        t = medians({'fused_fwd': fused_fwd, 'torch_fwd': torch_fwd, 'fused_bwd': fused_bwd, 'fused_step': fused_step,
                     'torch_step': torch_step}, args.warmup, args.reps)
        gathered = nb.nnz * d * 4 * (2 if attn else 1)
        bytes_fwd = gathered + nb.S * width * 4
        bytes_bwd = gathered * (1 if attn else 0) + nb.nnz * d * 4 * (2 if attn else 1) + nb.S * width * 4
        res['modes'][mode] = dict(us=t, max_abs_diff_to_torch=err, bytes_fwd=bytes_fwd, bytes_bwd=bytes_bwd,
                                  frac_hbm_fwd=bytes_fwd / (t['fused_fwd'] * 1e-6) / 1e9 / HBM,
                                  frac_hbm_bwd=bytes_bwd / (t['fused_bwd'] * 1e-6) / 1e9 / HBM,
                                  fwd_speedup=t['torch_fwd'] / t['fused_fwd'],
                                  step_speedup=t['torch_step'] / t['fused_step'])
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, 'w') as f:
            f.write(markdown(res, args))
    return 0


def markdown(res, args):
    lines = ['# Neighbour pooling kernels (MeanAggregator / AttnAggregator)', '',
             'Measured by `tools/nbr_pool_bench.py` on one MI355X: ICEWS18-shaped synthetic batch (synth.py, seed 999), '
             '%d sequences (%d with history), seq_len %d, D = %d: %d segments, %d neighbour rows (mean list %.1f, longest %d), '
             '%d entities.' % (res['sequences'], res['kept'], SEQ, res['D'], res['segments'], res['neighbours'],
                               res['mean_segment'], res['longest_segment'], res['entities']),
             'Medians of %d calls after %d warm-up calls, device events per call, fused and torch calls alternating.'
             % (args.reps, args.warmup), '',
             'What was measured: the two kernels alone (`fused fwd`, `fused bwd`), the torch-op baseline of the forward '
             '(`index_select` + `segment_reduce` + row scatter), and a whole forward + backward through `ops.NbrPoolFn` '
             '(kernels + the segmented adds + column sum) next to torch autograd over the baseline.',
             'What was NOT measured: kernel times from a profiler trace (these are event times around the call, launch '
             'overhead included), HBM traffic counters (the byte counts are algorithmic), the projection GEMMs of '
             'attention mode (P, q are inputs here), any size other than this one.', '',
             '| mode | fused fwd us | torch fwd us | ratio | fwd bytes | of 8 TB/s | fused bwd us | bwd bytes | of 8 TB/s | '
             'fused fwd+bwd us | torch fwd+bwd us | ratio |', '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for mode, m in res['modes'].items():
        t = m['us']
        lines.append('| %s | %.1f | %.1f | %.2fx | %.1f MB | %.1f %% | %.1f | %.1f MB | %.1f %% | %.1f | %.1f | %.2fx |'
                     % (mode, t['fused_fwd'], t['torch_fwd'], m['fwd_speedup'], m['bytes_fwd'] / 1e6,
                        100 * m['frac_hbm_fwd'], t['fused_bwd'], m['bytes_bwd'] / 1e6, 100 * m['frac_hbm_bwd'],
                        t['fused_step'], t['torch_step'], m['step_speedup']))
    lines += ['', 'Largest difference between the fused forward and the torch baseline on this batch: '
              + ', '.join('%s %.2e' % (k, m['max_abs_diff_to_torch']) for k, m in res['modes'].items()) + '.',
              'A ratio above 1 means the fused path is faster than torch; below 1 it is slower.', '']
    return '\n'.join(lines)


if __name__ == '__main__':
    sys.exit(main())
