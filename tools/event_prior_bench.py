#!/usr/bin/env python
"""What the recurrence prior costs the event forecasts, on the ICEWS18-shaped synthetic stream of tools/event_bench.py (40
training timestamps + n_t evaluated ones, hidden 200, seq_len 10).  GPU only; medians of REPS repetitions after WARMUP
warm-ups, the two sides of every comparison alternating; one JSON line (profiles/event_prior.md).

  kernels   device events around renet_joint_row_offsets, renet_joint_mix_rows (both launches) and renet_joint_rank_rows on the
            operands of the pass's FIRST sub-block (the mix on a fresh copy of the block every time: it works in place);
  passes    host clocks, ending in a synchronise, around RENet.evaluate_events_observed with and without a prior and around
            recurrence.evaluate_events.

THE EXPECTATION, written down before anything was measured: the mix moves one read and one write of the block, twice the
bytes of renet_joint_row_offsets, so at copy bandwidth it costs 2 * rows * C * 4 bytes / COPY_TBS and about twice the offsets
kernel.  profiles/recurrence_prior.md shows the ENTITY mix missing that kind of expectation by 4 x because of its sub-run
walks; the same walks run here.  The line reports both ratios and says whether the expectation held.

    python tools/event_prior_bench.py [positions] [n_t] [alpha] [half_life] [first|last]      defaults 256, 2, 0.3, 24 * 7, first

`last` takes the positions from the END of the evaluated timestamps: with a large n_t their histories are as long as the
stream (tools/event_bench.py's own choice is `first`: histories of 40 timestamps)."""
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

COPY_TBS = 6.29                 # what a float4 copy reaches on the device, TB/s (profiles/topk_rows.md)
REPS, WARMUP = 9, 2


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternating(fns):
    """{name: median seconds}: WARMUP + REPS rounds, every round running each side once, in turn."""
    times = {name: [] for name in fns}
    for rep in range(WARMUP + REPS):
        for name, fn in fns.items():
            dt = _wall(fn)
            if rep >= WARMUP:
                times[name].append(dt)
    return {name: float(np.median(v)) for name, v in times.items()}


def _device_seconds(prepare, fn):
    """fn between two device events, after prepare (not timed)."""
    prepare()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def first_sub_block(net, obs, idx, prior):
    """The operands of the first mix call and the first rank call of one pass with the prior (the same sub-block): the block
    and its offsets as they were BEFORE the mix."""
    import renet_hip as K
    real_mix, real_rank = K.joint_mix_rows, K.joint_rank_rows
    got = {}

    def mix(scores, num_rels, off, *rest, **kw):
        if 'mix' not in got:
            got['mix'] = (scores.clone(), num_rels, off.clone()) + rest
        return real_mix(scores, num_rels, off, *rest, **kw)

    def rank(*a):
        if 'rank' not in got:
            got['rank'] = a
        return real_rank(*a)
    K.joint_mix_rows, K.joint_rank_rows = mix, rank
    try:
        net.evaluate_events_observed(obs, idx, prior=prior)
    finally:
        K.joint_mix_rows, K.joint_rank_rows = real_mix, real_rank
    return got


def kernels(got):
    import renet_hip as K
    block0, R, off0 = got['mix'][:3]
    rest = got['mix'][3:]
    rank_rest = got['rank'][3:]
    rows, C = block0.shape
    g = rows // R
    logits_r = torch.randn(g, R, device=block0.device)
    block, off = block0.clone(), off0.clone()
    mass = torch.empty(g, device=block0.device, dtype=torch.float64)

    def fresh():
        block.copy_(block0)
        off.copy_(off0)
    sides = {
        'offsets': (lambda: None, lambda: K.joint_row_offsets(block0, R, logits_r)),
        'mix': (fresh, lambda: K.joint_mix_rows(block, R, off, *rest, mass=mass)),
        'rank': (lambda: None, lambda: K.joint_rank_rows(block, R, off, *rank_rest)),
    }
    times = {name: [] for name in sides}
    for rep in range(WARMUP + REPS):
        for name, (prepare, fn) in sides.items():
            dt = _device_seconds(prepare, fn)
            if rep >= WARMUP:
                times[name].append(dt)
    med = {name: float(np.median(v)) for name, v in times.items()}
    weights = mass.cpu().numpy()
    fresh()
    facts = K.joint_mix_rows(block, R, off, *rest[:-1], 0.0).cpu().numpy()             # inv_half_life 0: the facts counted
    b_block = rows * C * 4.0
    expected = 2.0 * b_block / (COPY_TBS * 1e12)
    res = {'block': [rows, C], 'groups': g, 'groups_with_history': int((facts > 0).sum()), 'facts_counted_median': float(np.median(facts)),
           'facts_counted_max': float(facts.max()), 'mass_median': float(np.median(weights)), 'mass_max': float(weights.max()),
           'seconds': med,
           'offsets_TB_per_s': b_block / med['offsets'] / 1e12, 'mix_TB_per_s': 2.0 * b_block / med['mix'] / 1e12,
           'rank_TB_per_s': got['rank'][3].numel() * R * C * 4.0 / med['rank'] / 1e12,
           'mix_expected_s_at_copy_bandwidth': expected, 'mix_over_expected': med['mix'] / expected,
           'mix_over_offsets': med['mix'] / med['offsets'], 'mix_over_offsets_expected': 2.0}
    res['expectation_held'] = bool(res['mix_over_expected'] <= 1.5 and res['mix_over_offsets'] <= 3.0)
    return res


def main():
    import recurrence
    limit = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    n_t = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    alpha = float(sys.argv[3]) if len(sys.argv) > 3 else 0.3
    half_life = float(sys.argv[4]) if len(sys.argv) > 4 else 24.0 * 7
    dev = torch.device('cuda:0')
    net, obs, idx, setup_s = OB._observed_setup(n_t, dev)
    which = sys.argv[5] if len(sys.argv) > 5 else 'first'
    idx = idx[:limit] if which == 'first' else idx[-limit:]
    prior = recurrence.RecurrencePrior(alpha, half_life)
    obs.device.pair_tables()                                    # built once, outside every timed region
    got = first_sub_block(net, obs, idx, prior)
    passes = _alternating({'model': lambda: net.evaluate_events_observed(obs, idx),
                           'model_with_prior': lambda: net.evaluate_events_observed(obs, idx, prior=prior),
                           'baseline': lambda: recurrence.evaluate_events(obs, idx, prior)})
    out = dict(shape=OB.SHAPE, hidden=net.h_dim, relations=net.num_rels, entities=net.in_dim, positions=int(len(idx)),
               timestamps=n_t, which=which, reps=REPS, warmup=WARMUP, alpha=prior.alpha, half_life=prior.half_life,
               facts=int(len(obs.allq)), pass_median_s=passes,
               prior_costs_the_pass=passes['model_with_prior'] / passes['model'] - 1.0,
               kernels_first_sub_block=kernels(got))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
