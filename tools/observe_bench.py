#!/usr/bin/env python
"""Cost of OBSERVING one timestamp on a resident stream, two ways in one process on one device:

  (a) rebuild:  ObservedStream.extended(quads) + resident(model, global_model) -- host lexsorts over every fact, one
                TimeGraph per timestamp, a full upload, the whole global-embedding table;
  (b) append:   ObservedStream.observe(quads, global_model) -- renet_store_append / renet_append_i32 over the resident
                tables, the new facts uploaded, the rows of the global table that can have changed.

The stream is the ICEWS18-shaped synthetic one of re-net_amd/synth.py (240 timestamps, ~1 550 facts each); the appended
quadruples are its last timestamp.  Each path is split into its index / table part and its global-row part, every part a
host clock around work that ends in a device synchronise.  Per repetition the parts run in the order a-parts, b-parts (the
paths alternate); medians over --reps repetitions after --warmup, with minimum, maximum and quartiles as the run-to-run
spread.  Before timing, the stores of the two paths are compared tensor for tensor.

    python tools/observe_bench.py [--shape ICEWS18] [--n-hidden 200] [--seq-len 10] [--reps 20] [--warmup 3] [--out FILE.md]
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--num-t', type=int, default=None, help='timestamps of the stream (default: the shape\'s own)')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    args = ap.parse_args()

    import numpy as np
    import torch
    import gpu_builder
    import synth
    from global_model import RENet_global
    from model import RENet
    from preprocess import ObservedStream
    if not torch.cuda.is_available():
        raise SystemExit('observe_bench.py measures on a HIP device: none found')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    allq, num_ent, num_rels, unit = synth.make_stream(args.shape, num_t=args.num_t)
    model = RENet(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len).to(dev).eval()
    gnet = RENet_global(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len, maxpool=1).to(dev).eval()
    times = np.unique(allq[:, 3])
    n_old = int(np.searchsorted(allq[:, 3], times[-1]))
    cut = int(np.searchsorted(allq[:, 3], times[int(len(times) * 0.8)]))
    old = ObservedStream((allq[:cut], allq[cut:n_old]), num_ent, num_rels, args.seq_len)
    quads = allq[n_old:]
    old.resident(model, gnet)
    sync = torch.cuda.synchronize

    def clock(fn):
        sync()
        t = time.perf_counter()
        r = fn()
        sync()
        return r, 1e3 * (time.perf_counter() - t)

    def rows_of(light):
        ts = [int(t) for t in light.times]
        with torch.no_grad():
            return {ts[-1]: gnet.predict(ts[-1] + (ts[1] - ts[0]), light.graph_dict)[0].detach()}

    # the two paths give the same store (at the size that is timed)
    want = old.extended(quads)
    want.resident(model, gnet)
    got = old.observe(quads, gnet)
    same = all(torch.equal(got.device.t[k], want.device.t[k]) for k in want.device.t) and \
        torch.equal(got.device.glob, want.device.glob) and sorted(got.device.t) == sorted(want.device.t)
    if not same:
        raise SystemExit('observe() and extended() + resident() disagree: nothing timed')
    del want, got

    names = ['a: extended() (host index, graphs)', 'a: ObservedStore (upload)', 'a: global table (all rows)', 'a: total',
             'b: light stream + new graph', 'b: device append (tables)', 'b: global rows (changed ones)', 'b: total observe()']
    rec = {n: [] for n in names}
    for rep in range(args.warmup + args.reps):
        ext, t_ext = clock(lambda: old.extended(quads))
        table, t_glob = clock(lambda: ext.global_table(gnet))
        _, t_up = clock(lambda: gpu_builder.ObservedStore(ext, table, model.h_dim, dev))
        light, t_light = clock(lambda: old._appended(old._checked_new(quads)))
        rows, t_rows = clock(lambda: rows_of(light))
        _, t_app = clock(lambda: old.device.appended(quads, rows, _obs=light))
        _, t_obs = clock(lambda: old.observe(quads, gnet))
        if rep >= args.warmup:
            for n, v in zip(names, (t_ext, t_up, t_glob, t_ext + t_up + t_glob, t_light, t_app, t_rows, t_obs)):
                rec[n].append(v)
        del ext, table, light, rows

    lines = ['%s-shaped stream: %d entities, %d facts at %d timestamps resident, %d facts appended (timestamp %d); '
             'n_hidden %d, seq_len %d; %d repetitions after %d warm-ups, ms per call, stores equal: %s'
             % (args.shape, num_ent, n_old, len(times) - 1, len(quads), int(times[-1]), args.n_hidden, args.seq_len, args.reps,
                args.warmup, same), '',
             '| part | median | min | 25 % | 75 % | max |', '|---|---|---|---|---|---|']
    for n in names:
        v = np.asarray(rec[n])
        lines.append('| %s | %.3f | %.3f | %.3f | %.3f | %.3f |' % (n, np.median(v), v.min(), np.percentile(v, 25),
                                                                  np.percentile(v, 75), v.max()))
    a, b = np.asarray(rec['a: total']), np.asarray(rec['b: total observe()'])
    lines += ['', 'a / b of the medians: %.1f; the slowest b (%.3f ms) against the fastest a (%.3f ms): %.1f'
              % (np.median(a) / np.median(b), b.max(), a.min(), a.min() / b.max())]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
