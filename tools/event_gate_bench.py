#!/usr/bin/env python
"""What training through the JOINT copy mix costs, on the ICEWS18-shaped synthetic stream of tools/event_bench.py (40 training
timestamps + n_t evaluated ones, hidden 200, seq_len 10).  GPU only; medians of REPS repetitions after WARMUP warm-ups, the
two sides of every comparison alternating; one JSON line (profiles/event_gate.md).

  gold     device events around the two renet_joint_gold_rows launches of one batch and around the two
           renet_recurrence_gold_rows launches of the SAME positions (both directions each);
  step     host clocks, ending in a synchronise, around one RENet.learn_observed step with event_prior= and one with prior=
           (the nearest existing path: same batch, same autograd route), a RecurrencePrior each, on two clones of the model;
  join     device events at the join of the side stream before the entity head's CE writer -- the first join made INSIDE
           ops.DualHeadCEFn's event path (an earlier join of the step, that of the GRU input projections, is not it): one
           recorded on the main stream and one on the side stream as the join is enqueued.  main -> side elapsed > 0: the
           main stream reached the join first and WAITS that long (a stall of the entity head); < 0: the relation head had
           ended that long before (an event wait already satisfied).

THE EXPECTATION, written down before anything was measured (profiles/event_gate.md has the reasoning): the joint gold kernel
walks the entity's whole run where the entity-side one walks one (entity, relation) sub-run, one workgroup per row in both, so
beyond the launch floor its time scales with the facts the BUSIEST rows walk, not with the total: expected ratio =
max(1, (FLOOR_FACTS + joint facts of the busiest row) / (FLOOR_FACTS + pair facts of the busiest row)) with FLOOR_FACTS the
facts a workgroup walks in the time of an empty launch (taken as 256 * 8: eight strided loads per thread).  The tool prints
both fact counts (total and busiest row).  The step: expected extra cost = the gold launches' difference plus the join of the
side stream before the entity head's CE writer (an event wait: the relation head ends long before the entity logits GEMM),
plus one [B, R] row scale.

    python tools/event_gate_bench.py [positions] [n_t] [alpha] [half_life] [first|last]      defaults 1024, 2, 0.3, 24 * 7, first

`last` takes the positions from the END of the evaluated timestamps: with a large n_t their histories are as long as the
stream (tools/event_prior_bench.py's convention)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import observed_eval_bench as OB

REPS, WARMUP = 9, 2
FLOOR_FACTS = 256 * 8


def _device_seconds(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternating(fns, clock):
    times = {name: [] for name in fns}
    for rep in range(WARMUP + REPS):
        for name, fn in fns.items():
            dt = clock(fn)
            if rep >= WARMUP:
                times[name].append(dt)
    return {name: float(np.median(v)) for name, v in times.items()}


def gold(store, idx, prior):
    import recurrence
    import renet_hip as K
    rows = recurrence.QueryRows(store, idx)
    base = rows.base

    def args(role):
        return (rows.ent[role], rows.rel, rows.t, rows.as_of, rows.ent[1 - role], rows.tables[role],
                base.t['ent_ptr%d' % role], base.t['snap_ptr%d' % role], base.num_ent)

    def joint():
        return [K.joint_gold_rows(*args(role), base.num_rels, base.num_ent, prior.inv_half_life) for role in (0, 1)]

    def pair():
        return [K.recurrence_gold_rows(*args(role), base.num_ent, prior.inv_half_life) for role in (0, 1)]
    med = _alternating({'joint': joint, 'pair': pair}, _device_seconds)
    # the facts walked: W at inv_half_life 0 is the count
    counts = {}
    for name, fn in (('joint', lambda role: K.joint_gold_rows(*args(role), base.num_rels, base.num_ent, 0.0)),
                     ('pair', lambda role: K.recurrence_gold_rows(*args(role), base.num_ent, 0.0))):
        w = torch.cat([fn(role)[1] for role in (0, 1)]).double().cpu().numpy()
        counts[name] = {'total': float(w.sum()), 'median': float(np.median(w)), 'max': float(w.max())}
    expected = max(1.0, (FLOOR_FACTS + counts['joint']['max']) / (FLOOR_FACTS + counts['pair']['max']))
    ratio = med['joint'] / med['pair']
    return {'rows': 2 * len(idx), 'seconds': med, 'facts_counted': counts, 'ratio': ratio, 'ratio_expected': expected,
            'ratio_of_totals': counts['joint']['total'] / max(counts['pair']['total'], 1.0),
            'expectation_held': bool(ratio <= 1.5 * expected and ratio >= expected / 1.5)}


def step(net, obs, idx, prior, dev):
    import copy
    import ops
    import parallel
    nets = {name: copy.deepcopy(net).to(dev) for name in ('event_prior', 'prior')}
    opts = {name: parallel.HipAdam(n, lr=1e-4, weight_decay=1e-5, max_norm=1.0) for name, n in nets.items()}
    fns = {'event_prior': lambda: nets['event_prior'].learn_observed(obs, idx, opts['event_prior'], event_prior=prior,
                                                                     batch_size=len(idx)),
           'prior': lambda: nets['prior'].learn_observed(obs, idx, opts['prior'], prior=prior, batch_size=len(idx))}
    med = _alternating(fns, _wall)
    # the join before the entity head's writer: the first join made after DualHeadCEFn's event path is entered (the step
    # joins the GRU input projections' side stream earlier, in MultiGRUFn.forward: that join is passed over)
    real_join, real_event, log, armed = ops._Side.join, ops.DualHeadCEFn.__dict__['_forward_event'], [], [False]

    def forward_event(*a, **k):
        armed[0] = True
        try:
            return real_event.__func__(*a, **k)
        finally:
            armed[0] = False

    def join(self):
        if self.on and armed[0]:
            armed[0] = False
            e_main, e_side = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e_main.record(self.main)
            e_side.record(self.side)
            log[-1].append((e_main, e_side))
        return real_join(self)
    ops._Side.join, ops.DualHeadCEFn._forward_event = join, staticmethod(forward_event)
    try:
        for _ in range(REPS):
            log.append([])
            fns['event_prior']()
    finally:
        ops._Side.join, ops.DualHeadCEFn._forward_event = real_join, real_event
    assert all(len(pair) == 1 for pair in log), 'one join before the entity head\'s writer per event step'
    torch.cuda.synchronize()
    lead = [pair[0][0].elapsed_time(pair[0][1]) * 1e-3 for pair in log if pair]       # > 0: main waits for the side stream
    return {'positions': int(len(idx)), 'seconds': med, 'extra_s': med['event_prior'] - med['prior'],
            'join_main_to_side_s': {'median': float(np.median(lead)), 'min': float(np.min(lead)), 'max': float(np.max(lead))} if lead else None,
            'join_stalled': bool(lead and np.median(lead) > 0.0)}


def main():
    import recurrence
    limit = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    n_t = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    alpha = float(sys.argv[3]) if len(sys.argv) > 3 else 0.3
    half_life = float(sys.argv[4]) if len(sys.argv) > 4 else 24.0 * 7
    dev = torch.device('cuda:0')
    net, obs, idx, setup_s = OB._observed_setup(n_t, dev)
    which = sys.argv[5] if len(sys.argv) > 5 else 'first'
    idx = idx[:limit] if which == 'first' else idx[-limit:]
    prior = recurrence.RecurrencePrior(alpha, half_life)
    store = obs.device
    store.pair_tables()                                         # built once, outside every timed region
    g = gold(store, idx, prior)
    s = step(net, obs, idx, prior, dev)
    s['extra_expected_s'] = g['seconds']['joint'] - g['seconds']['pair']
    print(json.dumps(dict(shape=OB.SHAPE, hidden=net.h_dim, relations=net.num_rels, entities=net.in_dim, timestamps=n_t, which=which,
                          reps=REPS, warmup=WARMUP, alpha=prior.alpha, half_life=prior.half_life, facts=int(len(obs.allq)),
                          gold=g, step=s)))


if __name__ == '__main__':
    main()
