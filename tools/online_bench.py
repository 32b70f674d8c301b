#!/usr/bin/env python
"""Cost of ONE timestamp of the online loop (RENet.evaluate_online) on a resident stream, split into its parts, with the
paths it replaces timed beside it in the same process on the same device:

  forecast      RENet.evaluate_forecast of the timestamp's facts on the stream as it stands
  observe       ObservedStream.observe (device append + the changed rows of the global table)
  learn         RENet.learn_observed, steps = 1, on the new positions (batches of --batch-size)
  global step   RENet_global.learn_observed on the timestamp
  refresh       ObservedStream.refresh_global: the whole table, batched on the device
  baseline      obs.global_table() (one predict() per timestamp) and resident() (host rebuild + upload + that table):
                what a weight update of the global model cost before refresh_global

The stream is the ICEWS18-shaped synthetic one of re-net_amd/synth.py (240 timestamps, ~1 550 facts each); the timestamp is
its last.  Every part is a host clock around work that ends in a device synchronise.  Per repetition the parts run once
each, in the order above (the new path and the baseline alternate); medians over --reps repetitions after --warmup, with
minimum, quartiles and maximum as the run-to-run spread.  The weights move from repetition to repetition (that is the
loop); the shapes do not.  Before timing, refresh_global is compared with global_table() on the same weights.

    python tools/online_bench.py [--shape ICEWS18] [--n-hidden 200] [--seq-len 10] [--reps 7] [--warmup 2] [--out FILE.md]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shape', default='ICEWS18')
    ap.add_argument('--n-hidden', type=int, default=200)
    ap.add_argument('--seq-len', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch-size', type=int, default=1024)
    ap.add_argument('--num-t', type=int, default=None, help='timestamps of the stream (default: the shape\'s own)')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit('online_bench.py reports medians of at least 5 repetitions')

    import numpy as np
    import torch
    import parallel
    import synth
    from global_model import RENet_global
    from model import RENet
    from preprocess import ObservedStream
    if not torch.cuda.is_available():
        raise SystemExit('online_bench.py measures on a HIP device: none found')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    allq, num_ent, num_rels, unit = synth.make_stream(args.shape, num_t=args.num_t)
    model = RENet(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len).to(dev).eval()
    gnet = RENet_global(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len, maxpool=1).to(dev).eval()
    opt = parallel.HipAdam(model, lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    gopt = parallel.HipAdam(gnet, lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    times = np.unique(allq[:, 3])
    n_old = int(np.searchsorted(allq[:, 3], times[-1]))
    cut = int(np.searchsorted(allq[:, 3], times[int(len(times) * 0.8)]))
    old = ObservedStream((allq[:cut], allq[cut:n_old]), num_ent, num_rels, args.seq_len)
    quads = allq[n_old:]
    t_new = int(times[-1])
    old.resident(model, gnet)
    sync = torch.cuda.synchronize

    def clock(fn):
        sync()
        t = time.perf_counter()
        r = fn()
        sync()
        return r, 1e3 * (time.perf_counter() - t)

    # the two tables on the same weights, at the size that is timed
    probe = old.observe(quads, gnet)
    table = probe.global_table(gnet)
    fresh = probe.refresh_global(gnet).device.glob
    want = torch.stack([table[int(t)].reshape(-1) for t in probe.device._glob_times])
    dev_max, scale = float((fresh - want).abs().max()), float(want.abs().max())
    del probe, table, fresh, want

    names = ['forecast', 'observe', 'learn (steps = 1)', 'global step', 'refresh_global', 'online timestamp, total',
             'baseline: global_table()', 'baseline: resident()']
    rec = {n: [] for n in names}
    known = allq
    for rep in range(args.warmup + args.reps):
        _, t_fc = clock(lambda: model.evaluate_forecast(old, quads, all_triplets=known))
        new, t_obs = clock(lambda: old.observe(quads, gnet))
        pos = np.arange(n_old, len(new))
        _, t_learn = clock(lambda: model.learn_observed(new, pos, opt, steps=1, batch_size=args.batch_size))
        _, t_gstep = clock(lambda: gnet.learn_observed(new, [t_new], gopt))
        ref, t_ref = clock(lambda: new.refresh_global(gnet))
        _, t_table = clock(lambda: new.global_table(gnet))
        _, t_res = clock(lambda: new.resident(model, gnet))
        if rep >= args.warmup:
            for n, v in zip(names, (t_fc, t_obs, t_learn, t_gstep, t_ref, t_fc + t_obs + t_learn + t_gstep + t_ref, t_table, t_res)):
                rec[n].append(v)
        del new, ref

    lines = ['%s-shaped stream: %d entities, %d facts at %d timestamps resident, timestamp %d with %d facts; n_hidden %d, '
             'seq_len %d, batch size %d; %d repetitions after %d warm-ups, ms per timestamp'
             % (args.shape, num_ent, n_old, len(times) - 1, t_new, len(quads), args.n_hidden, args.seq_len, args.batch_size,
                args.reps, args.warmup),
             'refresh_global against global_table() on the same weights: max |difference| %.3e at table scale %.3f'
             % (dev_max, scale), '',
             '| part | median | min | 25 % | 75 % | max |', '|---|---|---|---|---|---|']
    for n in names:
        v = np.asarray(rec[n])
        lines.append('| %s | %.3f | %.3f | %.3f | %.3f | %.3f |' % (n, np.median(v), v.min(), np.percentile(v, 25),
                                                                  np.percentile(v, 75), v.max()))
    a, b = np.asarray(rec['baseline: global_table()']), np.asarray(rec['refresh_global'])
    c = np.asarray(rec['baseline: resident()'])
    lines += ['', 'global_table() / refresh_global of the medians: %.1f; the slowest refresh_global (%.3f ms) against the fastest '
              'global_table() (%.3f ms): %.1f; resident() / refresh_global of the medians: %.1f'
              % (np.median(a) / np.median(b), b.max(), a.min(), a.min() / b.max(), np.median(c) / np.median(b))]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
