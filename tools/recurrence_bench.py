#!/usr/bin/env python
"""Cost of the recurrence prior (re-net_amd/recurrence.py, csrc/recurrence.hip) on one device, on the ICEWS18-shaped synthetic
stream of re-net_amd/synth.py:

  1. the mix kernel beside the score GEMM and renet_rank_rows3 on one [--rows, N_ent] score matrix (2048 x 23033): device
     events around each launch, medians over --reps repetitions after --warmup, with minimum and maximum;
  2. keeping the pair tables under observe(): renet_pair_append for both roles (with the host sort and upload of the new
     facts) beside the host rebuild (two preprocess.PairIndex lexsorts over every fact) plus upload, for the stream's last
     timestamp: host clocks around work that ends in a device synchronise, the two alternating per repetition;
  3. RENet.evaluate_observed over --positions positions of the stream's end with and without a prior, and the model-free
     baseline recurrence.evaluate over the same positions: host clocks, quadruples per second.

    python tools/recurrence_bench.py [--shape ICEWS18] [--n-hidden 200] [--seq-len 10] [--rows 2048] [--positions 8192]
                                     [--alpha 0.3] [--half-life 72] [--reps 20] [--warmup 3] [--out FILE.md]
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
    ap.add_argument('--positions', type=int, default=8192)
    ap.add_argument('--alpha', type=float, default=0.3)
    ap.add_argument('--half-life', type=float, default=72.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--num-t', type=int, default=None, help='timestamps of the stream (default: the shape\'s own)')
    ap.add_argument('--out', default=None, help='also write the tables to this file')
    args = ap.parse_args()

    import numpy as np
    import torch
    import filter_index as FI
    import gpu_builder
    import model as M
    import preprocess as P
    import recurrence
    import renet_hip as K
    import synth
    from global_model import RENet_global
    if not torch.cuda.is_available():
        raise SystemExit('recurrence_bench.py measures on a HIP device: none found')
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
    sync = torch.cuda.synchronize
    stat = lambda v: (np.median(v), np.min(v), np.max(v))
    lines = ['%s-shaped stream: %d entities, %d relations, %d facts at %d timestamps; n_hidden %d, seq_len %d; prior alpha %g, '
             'half-life %g; %d repetitions after %d warm-ups'
             % (args.shape, num_ent, num_rels, len(allq), len(times), args.n_hidden, args.seq_len, prior.alpha, prior.half_life,
                args.reps, args.warmup), '']

    # ---- 1. the kernels on one score matrix ----------------------------------------------------------------------------
    n = args.rows
    idx = np.arange(len(allq) - n, len(allq))
    tr = allq[idx]
    s, r, o, t = tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3]
    with torch.no_grad():
        (_, _, (feat_ob, _, _, _)), = M._observed_cuts(M._observed_chunks(model, store, idx), n)
    rows = recurrence.QueryRows(store, idx)
    index = FI.filter_index_for(store, store.quads)
    lists = index.ranges_both('o', np.stack((s, r, t), axis=1), dev)
    gold = torch.from_numpy(o.astype(np.int32)).to(dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return out, a.elapsed_time(b)

    rec = {k: [] for k in ('score GEMM', 'recurrence_mix_rows', 'recurrence_mix_rows (uniform logits)', 'rank_rows3',
                           'rank_rows3 on the mixed rows')}
    with torch.no_grad():
        for rep in range(args.warmup + args.reps):
            pred, t_gemm = timed(lambda: M._linear_eval(model.linear, feat_ob))
            mixed, t_mix = timed(lambda: rows.mix(prior, 'ob', pred))
            _, t_uni = timed(lambda: rows.mix(prior, 'ob', None))
            _, t_rank = timed(lambda: K.rank_rows3(pred, gold, *lists))
            _, t_rank2 = timed(lambda: K.rank_rows3(mixed, gold, *lists))
            if rep >= args.warmup:
                for k, v in zip(rec, (t_gemm, t_mix, t_uni, t_rank, t_rank2)):
                    rec[k].append(v)
        _, stats, _ = rows.mix(prior, 'ob', pred, want_stats=True)
    st = stats.cpu().numpy()
    nbytes = n * num_ent * 4
    lines += ['1. one [%d, %d] score matrix (%.1f MB), direction ob, device events, ms per launch; rows with history: %d of %d, '
              'facts counted per row: mean %.1f, max %d' % (n, num_ent, nbytes / 1e6, int((st[:, 1] > 0).sum()), n,
                                                           st[:, 1].mean(), st[:, 1].max()), '',
              '| launch | median | min | max | matrix passes per second (median) |', '|---|---|---|---|---|']
    for k, v in rec.items():
        med, lo, hi = stat(v)
        lines.append('| %s | %.4f | %.4f | %.4f | %.0f GB/s per pass |' % (k, med, lo, hi, nbytes / med / 1e6))
    lines.append('')

    # ---- 2. pair tables under observe() --------------------------------------------------------------------------------
    n_old = int(np.searchsorted(allq[:, 3], times[-1]))
    old = P.ObservedStream((allq[:cut], allq[cut:n_old]), num_ent, num_rels, args.seq_len)
    quads = allq[n_old:]
    old.resident(model, gnet)
    old.device.pair_tables()
    new = old.observe(quads, gnet)
    want = new.extended(quads[:0]).resident(model, gnet).pair_tables()                # (a host rebuild of the longer stream)
    same = all(torch.equal(x, y) for a, b in zip(new.device.pair_tables(), want) for x, y in zip(a, b))
    if not same:
        raise SystemExit('the appended pair tables differ from the rebuilt ones: nothing timed')

    def clock(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return out, 1e3 * (time.perf_counter() - t0)

    def rebuild():
        return [tuple(gpu_builder._i32(a, dev) for a in (pi.p_rel, pi.p_other, pi.p_t))
                for pi in (P.PairIndex(new.allq, role, num_ent) for role in (0, 1))]

    def append():
        keys = [np.stack((quads[:, c], quads[:, 1], quads[:, oc], quads[:, 3])) for c, oc in ((0, 2), (2, 0))]
        keys = [k[:, np.lexsort(k[::-1])] for k in keys]
        pk = torch.from_numpy(np.ascontiguousarray(np.stack(keys), dtype=np.int32)).to(dev)
        ot, nt = old.device.t, new.device.t
        return [K.pair_append(old.device.pair_tables()[role], ot['ent_ptr%d' % role], ot['snap_ptr%d' % role],
                              nt['ent_ptr%d' % role], nt['snap_ptr%d' % role], num_ent, pk[role]) for role in (0, 1)]

    rec2 = {'host rebuild (2 lexsorts) + upload': [], 'device append (sort of the new facts, upload, 2 x 2 launches)': [],
            'observe() without pair tables': [], 'observe() with pair tables': []}
    plain = P.ObservedStream((allq[:cut], allq[cut:n_old]), num_ent, num_rels, args.seq_len)
    plain.resident(model, gnet)
    for rep in range(args.warmup + args.reps):
        vals = (clock(rebuild)[1], clock(append)[1], clock(lambda: plain.observe(quads, gnet))[1],
                clock(lambda: old.observe(quads, gnet))[1])
        if rep >= args.warmup:
            for k, v in zip(rec2, vals):
                rec2[k].append(v)
    lines += ['2. pair tables of both roles after one observed timestamp (%d facts onto %d; tables equal: %s), host clocks '
              'around a device synchronise, ms' % (len(quads), n_old, same), '', '| path | median | min | max |', '|---|---|---|---|']
    for k, v in rec2.items():
        lines.append('| %s | %.3f | %.3f | %.3f |' % ((k,) + stat(v)))
    lines.append('')

    # ---- 3. evaluate_observed with and without a prior -----------------------------------------------------------------
    pos = np.arange(len(allq) - min(args.positions, len(allq) - cut), len(allq))
    runs = {'evaluate_observed, prior=None': lambda: model.evaluate_observed(obs, pos),
            'evaluate_observed, with the prior': lambda: model.evaluate_observed(obs, pos, prior=prior),
            'recurrence.evaluate (baseline alone)': lambda: recurrence.evaluate(obs, allq[pos], prior)}
    rec3 = {k: [] for k in runs}
    reps3 = max(3, args.reps // 4)
    for rep in range(1 + reps3):
        for k, fn in runs.items():
            _, ms = clock(fn)
            if rep >= 1:
                rec3[k].append(ms)
    lines += ['3. %d positions at the end of the stream, max_batch 4096, host clocks around a device synchronise, %d repetitions '
              'after 1 warm-up' % (len(pos), reps3), '', '| pass | median ms | min | max | quadruples/s (median) |',
              '|---|---|---|---|---|']
    for k, v in rec3.items():
        med, lo, hi = stat(v)
        lines.append('| %s | %.1f | %.1f | %.1f | %.0f |' % (k, med, lo, hi, len(pos) / med * 1e3))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
