#!/usr/bin/env python
"""Cost of training through the copy mix (re-net_amd/recurrence.py CopyGate / CopyRows, csrc/seq.hip renet_mix_ce_planes,
csrc/recurrence.hip renet_recurrence_gold_rows) on one device, on the ICEWS18-shaped synthetic stream of re-net_amd/synth.py.
Medians of --reps repetitions after --warmup, with minimum and maximum; the two sides of every comparison alternate inside
one repetition.

  1. renet_mix_ce_planes beside renet_softmax_ce_planes on one [--rows, N_ent] logits matrix (2048 x 23033): device events;
  2. the two renet_recurrence_gold_rows launches of a --batch-position batch (recurrence.CopyRows without its gather): device
     events around the pair;
  3. RENet.learn_observed, ms per step of --batch positions, with prior=None (the C launch list), with a RecurrencePrior
     and with a CopyGate and its optimizer (both on the autograd path): host clocks around a device synchronise;
  4. RENet.evaluate_observed over --positions positions with a scalar prior and with a CopyGate: quadruples per second.

    python tools/copy_gate_bench.py [--shape ICEWS18] [--n-hidden 200] [--seq-len 10] [--rows 2048] [--batch 1024]
                                    [--positions 8192] [--reps 7] [--warmup 2] [--out FILE.md]
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
    ap.add_argument('--rows', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--positions', type=int, default=8192)
    ap.add_argument('--alpha', type=float, default=0.3)
    ap.add_argument('--half-life', type=float, default=72.0)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--num-t', type=int, default=None, help='timestamps of the stream (default: the shape\'s own)')
    ap.add_argument('--out', default=None, help='also write the tables to this file')
    args = ap.parse_args()

    import numpy as np
    import torch
    import model as M
    import parallel
    import preprocess as P
    import recurrence
    import renet_hip as K
    import synth
    from global_model import RENet_global
    if not torch.cuda.is_available():
        raise SystemExit('copy_gate_bench.py measures on a HIP device: none found')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    allq, num_ent, num_rels, unit = synth.make_stream(args.shape, num_t=args.num_t)
    model = M.RENet(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len).to(dev).eval()
    gnet = RENet_global(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len, maxpool=1).to(dev).eval()
    times = np.unique(allq[:, 3])
    cut = int(np.searchsorted(allq[:, 3], times[int(len(times) * 0.8)]))
    obs = P.ObservedStream((allq[:cut], allq[cut:]), num_ent, num_rels, args.seq_len)
    store = obs.resident(model, gnet)
    prior = recurrence.RecurrencePrior(args.alpha, args.half_life)
    gate = recurrence.CopyGate(num_rels, alpha=args.alpha, half_life=args.half_life).to(dev)
    sync = torch.cuda.synchronize
    stat = lambda v: (np.median(v), np.min(v), np.max(v))
    lines = ['%s-shaped stream: %d entities, %d relations, %d facts at %d timestamps; n_hidden %d, seq_len %d; alpha %g, '
             'half-life %g; %d repetitions after %d warm-ups'
             % (args.shape, num_ent, num_rels, len(allq), len(times), args.n_hidden, args.seq_len, prior.alpha, prior.half_life,
                args.reps, args.warmup), '']

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return out, a.elapsed_time(b)

    def clock(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return out, 1e3 * (time.perf_counter() - t0)

    # ---- 1. the CE planes writer with and without the mix --------------------------------------------------------------
    n = args.rows
    rng = np.random.RandomState(1)
    logits = torch.empty(n, (num_ent + 3) & ~3, device=dev)[:, :num_ent]
    logits.copy_(torch.from_numpy((3.0 * rng.standard_normal((n, num_ent))).astype(np.float32)))
    gold = torch.from_numpy(rng.randint(0, num_ent, n).astype(np.int32)).to(dev)
    a_np = rng.uniform(0.05, 0.9, n).astype(np.float32)
    q_np = rng.uniform(0.0, 0.5, n).astype(np.float32)
    a_np[::3], q_np[::3] = 0.0, 0.0                                         # a third of the rows abstain
    a_row, q_row = torch.from_numpy(a_np).to(dev), torch.from_numpy(q_np).to(dev)
    rec = {'softmax_ce_planes': [], 'mix_ce_planes': []}
    for rep in range(args.warmup + args.reps):
        _, t_ce = timed(lambda: K.softmax_ce_planes(logits, gold, 1.0 / n))
        _, t_mix = timed(lambda: K.mix_ce_planes(logits, gold, a_row, q_row, 1.0 / n))
        if rep >= args.warmup:
            rec['softmax_ce_planes'].append(t_ce)
            rec['mix_ce_planes'].append(t_mix)
    lines += ['1. the CE gradient planes of one [%d, %d] logits matrix, device events, ms per call (each with its output '
              'allocation)' % (n, num_ent), '', '| writer | median | min | max |', '|---|---|---|---|']
    for k, v in rec.items():
        lines.append('| %s | %.4f | %.4f | %.4f |' % ((k,) + stat(v)))
    lines.append('')

    # ---- 2. the gold rows of one training batch ------------------------------------------------------------------------
    idx = np.arange(len(allq) - args.batch, len(allq))
    rows = recurrence.QueryRows(store, idx)
    base = rows.base

    def gold_pair():
        return [K.recurrence_gold_rows(rows.ent[role], rows.rel, rows.t, rows.as_of, rows.ent[1 - role], rows.tables[role],
                                       base.t['ent_ptr%d' % role], base.t['snap_ptr%d' % role], base.num_ent, base.num_ent,
                                       prior.inv_half_life) for role in (0, 1)]
    rec2 = {'2 x recurrence_gold_rows': [], 'recurrence.CopyRows (QueryRows, 2 launches, gate rows), host clock': []}
    for rep in range(args.warmup + args.reps):
        got, ms = timed(gold_pair)
        _, ms2 = clock(lambda: recurrence.CopyRows(store, idx, gate))
        if rep >= args.warmup:
            rec2['2 x recurrence_gold_rows'].append(ms)
            rec2['recurrence.CopyRows (QueryRows, 2 launches, gate rows), host clock'].append(ms2)
    hist = int(sum(int((w > 0).sum()) for _, w in got))
    lines += ['2. one batch of %d positions (2 x %d rows, %d with history), ms' % (len(idx), len(idx), hist), '',
              '| step | median | min | max |', '|---|---|---|---|']
    for k, v in rec2.items():
        lines.append('| %s | %.4f | %.4f | %.4f |' % ((k,) + stat(v)))
    lines.append('')

    # ---- 3. learn_observed ---------------------------------------------------------------------------------------------
    opt = parallel.HipAdam(model, lr=1e-4, weight_decay=1e-5, max_norm=1.0)
    gopt = torch.optim.Adam(gate.parameters(), lr=1e-3)
    runs = {'prior=None (C launch list)': lambda: model.learn_observed(obs, idx, opt),
            'RecurrencePrior (autograd path)': lambda: model.learn_observed(obs, idx, opt, prior=prior),
            'CopyGate + gate optimizer (autograd path)': lambda: model.learn_observed(obs, idx, opt, prior=gate, gate_optimizer=gopt)}
    rec3 = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for k, fn in runs.items():
            _, ms = clock(fn)
            if rep >= args.warmup:
                rec3[k].append(ms)
    lines += ['3. learn_observed, one step of %d positions (builder, step, optimizer, loss read-back), host clocks around a '
              'device synchronise, ms' % len(idx), '', '| step | median | min | max |', '|---|---|---|---|']
    for k, v in rec3.items():
        lines.append('| %s | %.3f | %.3f | %.3f |' % ((k,) + stat(v)))
    lines.append('')
    model.eval()

    # ---- 4. evaluate_observed ------------------------------------------------------------------------------------------
    pos = np.arange(len(allq) - min(args.positions, len(allq) - cut), len(allq))
    runs = {'evaluate_observed, RecurrencePrior': lambda: model.evaluate_observed(obs, pos, prior=prior),
            'evaluate_observed, CopyGate': lambda: model.evaluate_observed(obs, pos, prior=gate)}
    rec4 = {k: [] for k in runs}
    for rep in range(1 + args.reps):
        for k, fn in runs.items():
            _, ms = clock(fn)
            if rep >= 1:
                rec4[k].append(ms)
    lines += ['4. %d positions at the end of the stream, max_batch 4096, host clocks around a device synchronise, %d repetitions '
              'after 1 warm-up' % (len(pos), args.reps), '', '| pass | median ms | min | max | quadruples/s (median) |',
              '|---|---|---|---|---|']
    for k, v in rec4.items():
        med, lo, hi = stat(v)
        lines.append('| %s | %.1f | %.1f | %.1f | %.0f |' % (k, med, lo, hi, len(pos) / med * 1e3))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
