#!/usr/bin/env python
"""Cost of ONE generated timestamp of the rollout horizon (RENet.generate_events_observed + ObservedStream.observe) on the
ICEWS18-shaped synthetic stream of re-net_amd/synth.py, split into four parts:

  global predict    the two RENet_global.predict calls (host clock around a device synchronise, measured on their own);
  selection         the renet_select_events calls of the timestamp (HIP events around every call, summed);
  blocks + top-k    the rest of generate_events_observed: QueryStore, encoder chunk, per sub-block the recurrence, the
                    score GEMM, renet_joint_row_offsets and renet_topk_rows, the host glue and the one copy back
                    (total generate - global predict - selection);
  observe()         appending the generated facts to the resident stream.

The selection step is also timed against a TORCH STATEMENT of the same step on the same candidates -- V formed with the
same two additions, the carry concatenated in front, one stable torch.sort, a cumulative sum of the multiplicities; no
compaction and no read-back -- in a pass of its own (HIP events around every statement call, summed); the winners' values
of the two are compared once at the end.  The models are untrained (seeded random weights), so the global model's
distribution is nearly flat and the num_k draws are nearly all distinct: the number of distinct entities, the cost driver,
is printed.  Medians over --reps repetitions after --warmup, with minimum and maximum as the run-to-run spread.

    python tools/rollout_bench.py [--shape ICEWS18] [--n-hidden 200] [--num-k 1000] [--seq-len 10] [--reps 3] [--warmup 1]
                                  [--num-t T] [--out FILE.md]
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
    ap.add_argument('--num-k', type=int, default=1000)
    ap.add_argument('--seq-len', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--num-t', type=int, default=None, help='timestamps of the stream (default: the shape\'s own)')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    args = ap.parse_args()

    import numpy as np
    import torch
    import renet_hip as K
    import synth
    from global_model import RENet_global
    from model import RENet
    from preprocess import ObservedStream
    if not torch.cuda.is_available():
        raise SystemExit('rollout_bench.py measures on a HIP device: none found')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    allq, num_ent, num_rels, unit = synth.make_stream(args.shape, num_t=args.num_t)
    model = RENet(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len, num_k=args.num_k).to(dev).eval()
    gnet = RENet_global(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len, maxpool=1).to(dev).eval()
    times = np.unique(allq[:, 3])
    cut = int(np.searchsorted(allq[:, 3], times[int(len(times) * 0.8)]))
    obs = ObservedStream((allq[:cut], allq[cut:]), num_ent, num_rels, args.seq_len)
    obs.resident(model, gnet)
    t_next = int(times[-1]) + int(unit)
    sync = torch.cuda.synchronize
    R = num_rels

    def clock(fn):
        sync()
        t = time.perf_counter()
        r = fn()
        sync()
        return r, 1e3 * (time.perf_counter() - t)

    kernel = K.select_events
    events, agree = [], []
    mode = {'torch': False}

    def torch_statement(ent, val, off, g_ent, g_lprior, g_mult, num_k, carry):
        kk = min(ent.shape[1], num_k)
        v = (val[:, :kk] + off[:, None]) + g_lprior.repeat_interleave(R)[:, None]
        keep = ent[:, :kk] >= 0
        v = torch.where(keep, v, -np.inf).reshape(-1)
        w = torch.where(keep, g_mult.repeat_interleave(R)[:, None], 0).reshape(-1)
        if carry is not None:
            v, w = torch.cat((carry[3], v)), torch.cat((carry[4], w))
        sv, order = torch.sort(v, descending=True, stable=True)
        cw = torch.cumsum(w[order[:num_k]], 0)
        return sv[:num_k], (cw < num_k).sum() + 1

    def timed_select(ent, val, off, g_ent, g_lprior, g_mult, num_k, carry=None, workspace=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if mode['torch']:
            a.record()
            sv, n = torch_statement(ent, val, off, g_ent, g_lprior, g_mult, num_k, carry)
            b.record()
            out = kernel(ent, val, off, g_ent, g_lprior, g_mult, num_k, carry, workspace)
            live = torch.arange(num_k, device=dev) < out[5][0]
            agree.append((n.clamp(max=num_k) == out[5][0]) & (torch.where(live, sv, 0) == torch.where(live, out[3], 0)).all())
        else:
            a.record()
            out = kernel(ent, val, off, g_ent, g_lprior, g_mult, num_k, carry, workspace)
            b.record()
        events.append((a, b))
        return out

    K.select_events = timed_select

    def predicts():
        with torch.no_grad():
            return [gnet.predict(t_next, obs.graph_dict, subject=s)[2] for s in (True, False)]

    names = ['generate_events_observed, total', 'global predict (2 calls)', 'selection (renet_select_events, all calls)',
             'blocks + top-k (the rest)', 'observe() of the generated facts', 'selection as a torch statement (all calls)']
    rec = {n: [] for n in names}
    info = None
    for rep in range(args.warmup + args.reps):
        torch.manual_seed(100 + rep)
        del events[:]
        gen, t_gen = clock(lambda: model.generate_events_observed(obs, t_next, gnet))
        t_sel = sum(a.elapsed_time(b) for a, b in events)
        n_calls = len(events)
        info = (dict(model.last_generate), len(gen), n_calls)
        _, t_pred = clock(predicts)
        new, t_obs = clock(lambda: obs.observe(gen, gnet))
        del new
        mode['torch'] = True
        torch.manual_seed(100 + rep)
        del events[:]
        clock(lambda: model.generate_events_observed(obs, t_next, gnet))
        t_torch = sum(a.elapsed_time(b) for a, b in events)
        mode['torch'] = False
        if rep >= args.warmup:
            for n, v in zip(names, (t_gen, t_pred, t_sel, t_gen - t_pred - t_sel, t_obs, t_torch)):
                rec[n].append(v)
    same = bool(torch.stack([torch.as_tensor(x, device=dev) for x in agree]).all().item())
    K.select_events = kernel

    stats, n_gen, n_calls = info
    lines = ['%s-shaped stream: %d entities, %d relations, %d facts at %d timestamps resident; n_hidden %d, seq_len %d, num_k %d; '
             'one generated timestamp: %d / %d distinct entities (ob / sub) in %d / %d sub-blocks, %d select calls, %d facts '
             'generated; %d repetitions after %d warm-ups, ms per generated timestamp; winners of the torch statement equal '
             'the kernel\'s: %s'
             % (args.shape, num_ent, num_rels, len(allq), len(times), args.n_hidden, args.seq_len, args.num_k,
                stats['ob']['entities'], stats['sub']['entities'], stats['ob']['blocks'], stats['sub']['blocks'], n_calls, n_gen,
                args.reps, args.warmup, same), '',
             '| part | median | min | max |', '|---|---|---|---|']
    for n in names:
        v = np.asarray(rec[n])
        lines.append('| %s | %.3f | %.3f | %.3f |' % (n, np.median(v), v.min(), v.max()))
    a, b = np.asarray(rec[names[5]]), np.asarray(rec[names[2]])
    lines += ['', 'torch statement / kernel, medians: %.2f (per call: %.3f ms against %.3f ms)'
              % (np.median(a) / np.median(b), np.median(a) / n_calls, np.median(b) / n_calls)]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
