#!/usr/bin/env python
"""The last stage of the filtered evaluation -- scores to ranks and loss -- on a score matrix of evaluation size: the torch
tail (model._known_pairs x 2, uploads, model._rank_rows x 2, softmax_ce x 2) against the device tail
(filter_index.FilterIndex lookups + renet_rank_rows x 2), and evaluate_filter_stream with RENet.device_rank off and on.
GPU only.

    python tools/rank_bench.py tail [n] [C] [n_facts] [reps]        medians of `reps` alternating repetitions, JSON line
    python tools/rank_bench.py tail3 [n] [C] [n_facts] [reps]       the same matrix: one renet_rank_rows3 launch per direction
                                                                     with range lookups (raw + filtered + time-aware) against
                                                                     the two one-setting device tails run back to back
    python tools/rank_bench.py topk [n] [C] [k] [reps]              renet_topk_rows with the filter lists of the same matrix
                                                                     (one launch: filtered, sorted top-k and logp) against
                                                                     the torch formulation (clone, scatter of -inf,
                                                                     log_softmax, topk), device events, alternating
    python tools/rank_bench.py stream [shape] [n_timestamps] [reps]
    python tools/rank_bench.py stream3 [shape] [n_timestamps] [reps]   evaluate_all_stream against evaluate_stream and
                                                                     evaluate_filter_stream (device_rank on), each timed alone
    python tools/rank_bench.py grouped [shape] [n_timestamps] [reps]   evaluate_filter_stream (device_rank on) with
                                                                     RGCNAggregator.grouped_device_builder off and on
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import filter_index as FI
import model as M
import renet_hip as K

PEAK_HBM = 8.0e12                 # bytes/s, MI355X
MEASURED_HBM = 6.29e12            # bytes/s a float4 copy reaches: the floor of a one-pass kernel is its bytes over this


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _tail_matrix(n, C, n_facts, dev):
    """The score matrices, facts and quadruples of the tail modes -> (facts, quads, sub_pred, ob_pred, total)."""
    rng = np.random.RandomState(3)
    num_rels = 256
    facts = np.stack((rng.randint(0, C, n_facts), rng.randint(0, num_rels, n_facts), rng.randint(0, C, n_facts),
                      rng.randint(0, 300, n_facts) * 24), axis=1).astype(np.int64)
    facts = np.concatenate((facts, facts[: n_facts // 2] + np.array([0, 0, 0, 24])))     # repeated at another time
    quads = facts[rng.choice(len(facts), n, replace=False)]
    g = torch.Generator().manual_seed(1)
    ob_pred = (torch.randn(n, C, generator=g) * 4).to(dev)
    sub_pred = (torch.randn(n, C, generator=g) * 4).to(dev)
    return facts, quads, sub_pred, ob_pred, torch.from_numpy(facts).to(dev)


def tail(n=4096, C=23033, n_facts=400000, reps=7):
    dev = torch.device('cuda:0')
    facts, quads, sub_pred, ob_pred, total = _tail_matrix(n, C, n_facts, dev)
    s, r, o = quads[:, 0], quads[:, 1], quads[:, 2]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def old_tail():
        ro, co = M._known_pairs(total, (0, 1), 2, np.stack((s, r), axis=1))
        rs, cs = M._known_pairs(total, (2, 1), 0, np.stack((o, r), axis=1))
        rank_ob = M._rank_rows(ob_pred, t(o), t(ro), t(co))
        rank_sub = M._rank_rows(sub_pred, t(s), t(rs), t(cs))
        loss = K.softmax_ce(ob_pred, t(o).int(), 1.0, False) + K.softmax_ce(sub_pred, t(s).int(), 1.0, False)
        return np.stack((rank_sub, rank_ob), axis=1), loss

    t_build, index = _wall(lambda: FI.FilterIndex(total))

    def new_tail():
        label = torch.from_numpy(np.stack((s, o)).astype(np.int32)).to(dev)
        counts, loss = [], None
        for side, pred, lab, keys in (('s', sub_pred, label[0], (o, r)), ('o', ob_pred, label[1], (s, r))):
            ptr, col = index.lookup(side, np.stack(keys, axis=1), dev)
            cnt, ls = K.rank_rows(pred, lab, ptr, col, filtered=True)
            counts.append(cnt)
            loss = ls if loss is None else loss + ls
        gr, eq = torch.stack(counts, dim=2).cpu().numpy().astype(np.float64)
        return gr + (eq - 1.0) / 2 + 1, loss

    (ra, la), (rb, lb) = old_tail(), new_tail()                 # warm-up of every shape, and the two tails must agree
    same = bool(np.array_equal(ra, rb))
    loss_diff = float((la - lb).abs().max())
    told, tnew = [], []
    for _ in range(reps):                                       # alternating: both sides see the same machine state
        told.append(_wall(old_tail)[0])
        tnew.append(_wall(new_tail)[0])
    # the kernel alone (device events), filtered with lists and loss: one read of the matrix
    ptr, col = index.lookup('o', np.stack((s, r), axis=1), dev)
    lab = t(o).int()
    ev = []
    for _ in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.rank_rows(ob_pred, lab, ptr, col, filtered=True)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3)
    t_k = float(np.median(ev[3:]))
    nbytes = float(n) * C * 4
    print(json.dumps({'n': n, 'C': C, 'facts': int(len(facts)), 'filter_nnz_per_side': int(ptr[-1]), 'reps': reps,
                      'ranks_identical': same, 'loss_max_abs_diff': loss_diff,
                      'old_tail_ms': [round(x * 1e3, 3) for x in sorted(told)], 'old_tail_median_ms': float(np.median(told)) * 1e3,
                      'new_tail_ms': [round(x * 1e3, 3) for x in sorted(tnew)], 'new_tail_median_ms': float(np.median(tnew)) * 1e3,
                      'index_build_once_ms': t_build * 1e3, 'kernel_median_ms': t_k * 1e3,
                      'kernel_bytes_per_s': nbytes / t_k, 'kernel_share_of_hbm_peak': nbytes / t_k / PEAK_HBM}))


def _event_ms(fn, reps):
    """Median device time of fn (events) over reps launches after 3 warm-up ones, in ms."""
    ev = []
    for _ in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    return float(np.median(ev[3:]))


def tail3(n=4096, C=23033, n_facts=400000, reps=7):
    """After the scores of one group, both directions: the two one-setting device tails back to back (what
    evaluate_stream + evaluate_filter_stream with device_rank on run per group: raw counts, then lookup + filtered counts,
    each with its label upload, loss and copy of the counts) against the one three-setting tail of evaluate_all_batch."""
    dev = torch.device('cuda:0')
    facts, quads, sub_pred, ob_pred, total = _tail_matrix(n, C, n_facts, dev)
    s, r, o, tq = quads[:, 0], quads[:, 1], quads[:, 2], quads[:, 3]
    index = FI.FilterIndex(total)
    sides = (('s', sub_pred, 0, o), ('o', ob_pred, 1, s))
    rank = lambda counts: (lambda c: c[0] + (c[1] - 1.0) / 2 + 1)(torch.stack(counts, dim=2).cpu().numpy().astype(np.float64))

    def one_setting(filtered):
        label = torch.from_numpy(np.stack((s, o)).astype(np.int32)).to(dev)
        counts, loss = [], None
        for side, pred, k, key in sides:
            ptr, col = index.lookup(side, np.stack((key, r), axis=1), dev) if filtered else (None, None)
            cnt, ls = K.rank_rows(pred, label[k], ptr, col, filtered=filtered)
            counts.append(cnt)
            loss = ls if loss is None else loss + ls
        return rank(counts), loss

    def two_tails():
        return one_setting(False), one_setting(True)

    def one_tail():
        label = torch.from_numpy(np.stack((s, o)).astype(np.int32)).to(dev)
        counts, loss = [], None
        for side, pred, k, key in sides:
            lists = index.ranges_both(side, np.stack((key, r, tq), axis=1), dev)
            cnt, ls = K.rank_rows3(pred, label[k], *lists)
            counts.append(cnt)
            loss = ls if loss is None else loss + ls
        c = torch.stack(counts, dim=2).cpu().numpy().astype(np.float64)
        return [c[2 * k] + (c[2 * k + 1] - 1.0) / 2 + 1 for k in range(3)], loss

    ((raw, l_raw), (filt, _)), (three, l3) = two_tails(), one_tail()       # warm-up (the timed tables are built here)
    told, tnew = [], []
    for _ in range(reps):                                       # alternating: both sides see the same machine state
        told.append(_wall(two_tails)[0])
        tnew.append(_wall(one_tail)[0])
    lab = torch.from_numpy(o.astype(np.int32)).to(dev)
    ptr, col = index.lookup('o', np.stack((s, r), axis=1), dev)
    lists = index.ranges_both('o', np.stack((s, r, tq), axis=1), dev)
    k_raw = _event_ms(lambda: K.rank_rows(ob_pred, lab, filtered=False), reps)
    k_filt = _event_ms(lambda: K.rank_rows(ob_pred, lab, ptr, col, filtered=True), reps)
    k_three = _event_ms(lambda: K.rank_rows3(ob_pred, lab, *lists), reps)
    nbytes = float(n) * C * 4
    print(json.dumps({'n': n, 'C': C, 'facts': int(len(facts)), 'reps': reps,
                      'filter_nnz_per_side': int(ptr[-1]), 'time_aware_nnz_per_side': int(lists[5].sum()),
                      'raw_identical': bool(np.array_equal(raw, three[0])), 'filtered_identical': bool(np.array_equal(filt, three[1])),
                      'filtered_le_time_filtered': bool(np.all(three[1] <= three[2])),
                      'rows_time_filtered_differs': int((three[1] != three[2]).any(axis=1).sum()),
                      'loss_bit_equal': bool(torch.equal(l_raw, l3)),
                      'two_tails_ms': [round(x * 1e3, 3) for x in sorted(told)], 'two_tails_median_ms': float(np.median(told)) * 1e3,
                      'one_tail_ms': [round(x * 1e3, 3) for x in sorted(tnew)], 'one_tail_median_ms': float(np.median(tnew)) * 1e3,
                      'kernel_raw_ms': k_raw, 'kernel_filtered_ms': k_filt, 'kernel_three_ms': k_three,
                      'kernel_three_bytes_per_s': nbytes / (k_three * 1e-3),
                      'kernel_three_share_of_hbm_peak': nbytes / (k_three * 1e-3) / PEAK_HBM}))


def topk(n=4096, C=23033, k=10, reps=20, n_facts=400000, inner=10):
    """The k best objects of (s, r, ?, t) outside the known ones, for every row of the tail modes' object score matrix:
    K.topk_rows with the time-agnostic lists addressed in the resident table, against what a user writes in torch on the
    same device matrix (the listed pairs already on the device).  Every repetition times `inner` back-to-back calls of one
    side with device events, then of the other; 3 warm-up repetitions; median, minimum and maximum per call."""
    dev = torch.device('cuda:0')
    facts, quads, _, ob_pred, total = _tail_matrix(n, C, n_facts, dev)
    s, r = quads[:, 0], quads[:, 1]
    keys = np.stack((s, r), axis=1)
    lists = FI.FilterIndex(total).ranges('o', keys, dev)
    rows, cols = (torch.from_numpy(x).to(dev) for x in M._known_pairs(total, (0, 1), 2, keys))

    def kernel():
        return K.topk_rows(ob_pred, k, *lists)

    def kernel_no_logp():                                       # what the fp64 logsumexp of the sweep costs
        return K.topk_rows(ob_pred, k, *lists, want_logp=False)

    lab = torch.from_numpy(quads[:, 2].astype(np.int32)).to(dev)

    def rank_kernel():                                          # renet_rank_rows with its loss: the same sweep and logsumexp
        return K.rank_rows(ob_pred, lab, filtered=False, want_loss=True)

    def torch_path():
        x = ob_pred.clone()
        x[rows, cols] = float('-inf')
        val, idx = torch.topk(torch.log_softmax(x, dim=1), k, dim=1, sorted=True)
        return idx, val

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    (idx, val, logp, nv), (tidx, _) = kernel(), torch_path()
    # the same entities wherever the scores are distinct (torch leaves the order of ties open; its logp is renormalised
    # over the candidates, so only the indices are compared)
    same_rows = int((idx.long() == tidx).all(dim=1).sum())
    tk, tt, tn, tr = [], [], [], []
    for rep in range(3 + reps):                                 # alternating: every side sees the same machine state
        a, b, c, d = timed(kernel), timed(torch_path), timed(kernel_no_logp), timed(rank_kernel)
        if rep >= 3:
            tk.append(a)
            tt.append(b)
            tn.append(c)
            tr.append(d)
    nbytes = float(n) * C * 4
    floor_ms = nbytes / MEASURED_HBM * 1e3
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v)), 'max_ms': float(np.max(v))}
    print(json.dumps({'n': n, 'C': C, 'k': k, 'reps': reps, 'calls_per_rep': inner, 'facts': int(len(facts)),
                      'filter_nnz': int(lists[2].sum()), 'n_valid_min': int(nv.min()),
                      'rows_with_torch_indices': same_rows, 'kernel': stat(tk), 'torch': stat(tt),
                      'kernel_without_logp': stat(tn), 'rank_rows_with_loss': stat(tr),
                      'torch_over_kernel': float(np.median(tt) / np.median(tk)),
                      'matrix_bytes': nbytes, 'one_hbm_read_ms_at_6.29TBps': floor_ms,
                      'kernel_over_one_hbm_read': float(np.median(tk) / floor_ms),
                      'kernel_bytes_per_s': nbytes / (float(np.median(tk)) * 1e-3)}))


def stream3(shape='ICEWS18', n_t=3, reps=3):
    """evaluate_stream, evaluate_filter_stream (device_rank on) and evaluate_all_stream over the same stream, a fresh model
    per pass, the three alternating; repetition 0 warms up all of them."""
    import infer_bench
    dev = torch.device('cuda:0')
    runs = {'raw': lambda net, te, tes, teo, gnet, total: net.evaluate_stream(te, tes, teo, gnet),
            'filtered': lambda net, te, tes, teo, gnet, total: net.evaluate_filter_stream(te, tes, teo, gnet, total),
            'all': lambda net, te, tes, teo, gnet, total: net.evaluate_all_stream(te, tes, teo, gnet, total)}
    times, ranks = {k: [] for k in runs}, {}
    for rep in range(reps + 1):
        for name, run in runs.items():
            net, gnet, te, tes, teo, total = infer_bench.setup(shape, n_t, 200, dev)
            net.device_rank = True
            with torch.no_grad():
                dt, (rk, _) = _wall(lambda: run(net, te, tes, teo, gnet, total))
            if rep:
                times[name].append(dt)
            ranks[name] = rk
    n = len(ranks['raw'])
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({'shape': shape, 'timestamps': n_t, 'quadruples': n, 'reps': reps,
                      'raw_identical': bool(np.array_equal(ranks['raw'], ranks['all']['raw'])),
                      'filtered_identical': bool(np.array_equal(ranks['filtered'], ranks['all']['filtered'])),
                      'rows_time_filtered_differs': int((ranks['all']['filtered'] != ranks['all']['time_filtered']).any(axis=1).sum()),
                      'raw_s': [round(x, 4) for x in times['raw']], 'filtered_s': [round(x, 4) for x in times['filtered']],
                      'all_s': [round(x, 4) for x in times['all']],
                      'raw_median_s': med['raw'], 'filtered_median_s': med['filtered'],
                      'two_passes_median_s': med['raw'] + med['filtered'], 'all_median_s': med['all']}))


def stream(shape='ICEWS18', n_t=3, reps=2):
    import infer_bench
    dev = torch.device('cuda:0')
    times = {False: [], True: []}
    ranks = {}
    for rep in range(reps + 1):                                 # repetition 0 warms up both sides
        for on in (False, True):
            net, gnet, te, tes, teo, total = infer_bench.setup(shape, n_t, 200, dev)
            net.device_rank = on
            with torch.no_grad():
                dt, (rk, _) = _wall(lambda: net.evaluate_filter_stream(te, tes, teo, gnet, total))
            if rep:
                times[on].append(dt)
            ranks[on] = rk
    n = len(ranks[True])
    print(json.dumps({'shape': shape, 'timestamps': n_t, 'quadruples': n, 'reps': reps,
                      'ranks_identical': bool(np.array_equal(ranks[False], ranks[True])),
                      'off_s': [round(x, 4) for x in times[False]], 'on_s': [round(x, 4) for x in times[True]],
                      'off_quadruples_per_s': n / float(np.median(times[False])),
                      'on_quadruples_per_s': n / float(np.median(times[True]))}))


def grouped(shape='ICEWS18', n_t=3, reps=2):
    """evaluate_filter_stream with the grouped batches from the host builder (off) and the device builder (on), device_rank
    on in both: alternating repetitions after a warm-up of each, then ONE profiled pass per side that synchronises around
    every forward_grouped stage -- builder (graph.build_batch + upload / GroupedDeviceBatch to finalize) and encoder (host
    timer and device events) per call; `rest` is what remains of the pass (score GEMMs, ranks, the host loop)."""
    import infer_bench
    dev = torch.device('cuda:0')
    times = {False: [], True: []}
    ranks, split = {}, {}

    def one(on, profile=False):
        net, gnet, te, tes, teo, total = infer_bench.setup(shape, n_t, 200, dev)
        net.device_rank = True
        agg = net.aggregator
        agg.grouped_device_builder = on
        rec = {'build': [], 'encode': [], 'encode_dev': [], 'rows': []}
        if profile:
            build, build_dev, encode = agg.build, agg.build_grouped_device, agg.encode

            def timed(fn, key):
                def run(*a, **k):
                    dt, out = _wall(lambda: fn(*a, **k))
                    if out is not None or key != 'build_dev':
                        rec['build'].append(dt)
                    return out
                return run

            def enc(g, *a, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                out = encode(g, *a, **k)
                e1.record()
                torch.cuda.synchronize()
                rec['encode'].append(time.perf_counter() - t0)
                rec['encode_dev'].append(e0.elapsed_time(e1) * 1e-3)
                rec['rows'].append(int(g.S))
                return out
            agg.build, agg.build_grouped_device, agg.encode = timed(build, 'build'), timed(build_dev, 'build_dev'), enc
        with torch.no_grad():
            dt, (rk, _) = _wall(lambda: net.evaluate_filter_stream(te, tes, teo, gnet, total))
        return dt, rk, rec

    for rep_ in range(reps + 1):                                # repetition 0 warms up both sides
        for on in (False, True):
            dt, rk, _ = one(on)
            if rep_:
                times[on].append(dt)
            ranks[on] = rk
    for on in (False, True):
        dt, _, rec = one(on, profile=True)
        ms = lambda xs: round(float(np.median(xs)) * 1e3, 3) if xs else None
        split[on] = {'groups': len(rec['encode']), 'pass_s': round(dt, 4), 'build_ms_median': ms(rec['build']),
                     'build_ms_sum': round(sum(rec['build']) * 1e3, 2), 'encode_ms_median': ms(rec['encode']),
                     'encode_device_ms_median': ms(rec['encode_dev']), 'encode_ms_sum': round(sum(rec['encode']) * 1e3, 2),
                     'rest_ms_sum': round((dt - sum(rec['build']) - sum(rec['encode'])) * 1e3, 2),
                     'steps_median': int(np.median(rec['rows'])) if rec['rows'] else 0}
    n = len(ranks[True])
    print(json.dumps({'shape': shape, 'timestamps': n_t, 'quadruples': n, 'reps': reps,
                      'ranks_identical': bool(np.array_equal(ranks[False], ranks[True])),
                      'off_s': [round(x, 4) for x in times[False]], 'on_s': [round(x, 4) for x in times[True]],
                      'off_quadruples_per_s': n / float(np.median(times[False])),
                      'on_quadruples_per_s': n / float(np.median(times[True])),
                      'split_off': split[False], 'split_on': split[True]}))


if __name__ == '__main__':
    a = sys.argv[1:]
    if a and a[0] == 'grouped':
        grouped(a[1] if len(a) > 1 else 'ICEWS18', int(a[2]) if len(a) > 2 else 3, int(a[3]) if len(a) > 3 else 2)
    elif a and a[0] == 'stream3':
        stream3(a[1] if len(a) > 1 else 'ICEWS18', int(a[2]) if len(a) > 2 else 3, int(a[3]) if len(a) > 3 else 3)
    elif a and a[0] == 'tail3':
        tail3(*[int(x) for x in a[1:5]])
    elif a and a[0] == 'topk':
        topk(*[int(x) for x in a[1:5]])
    elif a and a[0] == 'stream':
        stream(a[1] if len(a) > 1 else 'ICEWS18', int(a[2]) if len(a) > 2 else 3, int(a[3]) if len(a) > 3 else 2)
    else:
        tail(*[int(x) for x in a[1:5]])
