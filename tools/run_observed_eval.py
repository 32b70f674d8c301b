#!/usr/bin/env python
"""Observed-history (single-step, ground-truth history) evaluation of a trained model: raw, filtered and time-aware filtered
MRR / Hits of a split, every query at time t seeing all facts before t (the evaluated split's own included) -- the
protocol under which RE-GCN, xERTE and TITer report the time-aware filter.  NOT the reference's multi-step protocol
(test.py; RENet.evaluate_all_stream): the two answer different questions, their numbers must not be mixed.

    python tools/run_observed_eval.py DATA_DIR --n-hidden H --seq-len L [--split valid|test] [--topk K] [--events [K]]
                                      [--model-dir models/<DS>] [--maxpool 1] [--max-batch 4096] [--gpu 0]
                                      [--horizon H] [--queries FILE [--k K]] [--observe-loop]
                                      [--rollout H [--num-k K]]
                                      [--online [STEPS] [--replay N] [--online-global] [--lr LR]]
                                      [--recurrence ALPHA [--half-life H] [--fit-gate STEPS] [--learn-copy] [--gate-lr LR]]

--horizon H evaluates with STALE histories (RENet.evaluate_forecast with ObservedStream.horizon_as_of): the split's timestamps
are cut into blocks of H, and every query forecasts from the facts before the first timestamp of its block; nothing is
generated in between.  H is printed with the metrics: numbers of different H (H = 1 is the plain observed protocol) must not
be mixed.  --queries FILE forecasts open queries instead of a split: a TSV of `s r o t` lines with -1 for an absent side
(RENet.forecast_topk, time-aware filtered); prints the K best objects of (s, r, ?, t) and subjects of (?, r, o, t).

--observe-loop evaluates the split as a FORECAST / OBSERVE loop: the stream starts with the facts before the split; per
timestamp t of the split, the facts of t are forecast on the resident store as it stands (RENet.evaluate_forecast: nothing
of t or later is in it), then observed (ObservedStream.observe: appended on the device, one new row of the global table).
The filtered settings filter by the whole dataset, as the plain pass does.  Every timestamp is a batch graph of its own
here, and a row depends on what shares its batch graph: the metrics are those of the plain pass asked timestamp by timestamp,
close to but not bit for bit those of the plain pass over the whole split.  The times of the two halves are printed apart.

--rollout H evaluates under the ROLLOUT horizon (RENet.evaluate_rollout): the stream starts with the facts before the split,
as --observe-loop; the split's timestamps are cut into blocks of H; the first timestamp of a block is forecast from the true
facts before it, every later one from those plus the facts the model GENERATED for the block's earlier timestamps
(RENet.generate_events_observed, appended with ObservedStream.observe); the truth is observed after every block.  Its
numbers are neither those of --horizon H (nothing generated) nor the reference's multi-step numbers (test.py: per-entity
caches, no observed truth at all): three protocols, three sets of numbers.  Exclusive with --horizon, --observe-loop,
--queries and --events.

--online [STEPS] evaluates with ONLINE LEARNING (RENet.evaluate_online): the forecast / observe loop of --observe-loop, and
after every observed timestamp STEPS training steps (default 1; parallel.HipAdam, --lr) on that timestamp's facts plus those
of the --replay timestamps before it; with --online-global the global model takes a step on the timestamp as well and the
resident global table is recomputed (ObservedStream.refresh_global).  The weights that rank timestamp t have seen every
evaluated timestamp before t: a FOURTH protocol, whose numbers must not be mixed with the static observed ones, --horizon,
--rollout or the reference's multi-step numbers.  The checkpoints are not written back.

--recurrence ALPHA [--half-life H] adds the RECURRENCE PRIOR (re-net_amd/recurrence.py) to the plain pass (and to --horizon):
after the model's own metrics it prints the model-free BASELINE alone -- how often, and with --half-life how recently, (s, r)
connected to each object before the query's as-of time, ranked under the same histories, filters and tie rule -- and the
model MIXED with the prior at weight ALPHA, each labelled as such.  The baseline is a protocol-matched yardstick: report it
with its ALPHA and half-life (in the dataset's raw timestamp units), beside model numbers of the same protocol only.

--events [K] --recurrence ALPHA [--half-life H] --fit-gate STEPS [--learn-half-life] fits the EVENT gate INSTEAD of the
per-relation entity gate (one invocation fits one gate; the entity blocks above it are those of the initial prior): a
recurrence.CopyGate(per_relation=False) -- one gate, and with --learn-half-life one decay, per side -- through the joint mix
(recurrence.fit_event_gate) on the VALID split, the model frozen; it prints the fitted alpha and half-life per side, then the
event numbers with the fitted gate, with the initial prior and without a prior.  WARNING: numbers with a fitted event gate are a
protocol of their own: report them with the initial ALPHA and H, the fitting split, STEPS and --gate-lr.
--fit-gate STEPS (with --recurrence) LEARNS the weight of the prior: a recurrence.CopyGate -- one gate per side and relation,
initialised to ALPHA -- is fitted with the model frozen (recurrence.fit_gate, STEPS Adam steps at --gate-lr) on the VALID
split under observed histories, and the chosen split is then evaluated mixed with the learned gates.  --online --recurrence
ALPHA mixes the prior into the forecast half of the online loop; with --learn-copy the learn steps train THROUGH the mix
(RENet.learn_observed(prior=, gate_optimizer=)) and the gates learn along the stream.  Numbers with a LEARNED gate are a
protocol of their own -- the gate has seen the fitting data: every line printed says so, and such numbers are comparable only
with numbers of the same protocol and the same fitting data.  A learn step through the mix is not in the C launch list
(csrc/step.cpp): it runs the autograd path and pays its host enqueue.

--learn-half-life (with --recurrence ALPHA --half-life H and one of --fit-gate / --online --learn-copy) LEARNS the decay too:
the gate carries one half-life per side and relation (recurrence.CopyGate(learn_half_life=True)), initialised to H and trained
by the same optimizer through q's derivative by the decay (renet_recurrence_gold_rows_decay).  The lines printed give the min,
median and max of the learned half-lives per side beside the gate range, and the JSON record holds them.  Numbers with learned
parameters are a protocol of their own: report the INITIAL alpha and half-life, the fitting split, steps and learning rate.
With --events --fit-gate the EVENT gate carries ONE half-life per side (renet_joint_gold_rows_decay); both are printed.

--events adds the EVENT forecasts (RENet.evaluate_events_observed): MRR / Hits of the gold (relation, entity) pair among all
pairs of the given entity, and of the gold relation given both endpoints, in the three settings; with K also the K most
probable (relation, object) pairs of the first few queries (RENet.predict_events_observed, time-aware filtered).
--events with --recurrence ALPHA [--half-life H] prints three event blocks of one protocol, each labelled with ALPHA and the
half-life: the model-free recurrence baseline (recurrence.evaluate_events), the model mixed with the JOINT prior
(evaluate_events_observed(prior=)) and the model alone; the JSON record gains `recurrence`, `baseline` and `mixed`.  The
histories (and the prior) are as of each query's own timestamp, as for --events alone.

DATA_DIR holds stat.txt, train.txt, valid.txt (optional) and test.txt.  From the model directory (default: models/<name of
DATA_DIR>, where the reference's drivers write) only the weights are read: `rgcn.pth` (train.py:189) and the global model's
`max<M>rgcn_global2.pth` (train.py:196) or, without it, `max<M>rgcn_global.pth` (pretrain.py:98); the multi-step state saved
beside them (histories, caches, graph_dict, global_emb) is ignored -- the pass builds what it needs from the text files."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 're-net_amd'))


def observe_loop(args, model, global_model, splits, num_ent, num_rels, data_dir):
    """--observe-loop: forecast t on the store as it stands, then observe t, for every timestamp of the split."""
    import numpy as np
    import torch
    import utils as U
    from model import SETTINGS
    from preprocess import ObservedStream
    known = np.concatenate([q for q in splits if q is not None])       # what the filtered settings filter by, as the plain pass
    names = [n for n, q in zip(('train', 'valid', 'test'), splits) if q is not None]
    k = names.index(args.split)
    evaluated = splits[[i for i, q in enumerate(splits) if q is not None][k]]
    start = [q for q in splits if q is not None][:k] + [np.zeros((0, 4), dtype=np.int64)]
    if len(start) < 2:
        raise SystemExit('nothing lies before the %s split' % args.split)
    t0 = time.perf_counter()
    obs = ObservedStream(start, num_ent, num_rels, args.seq_len)
    obs.resident(model, global_model)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ranks, loss, t_forecast, t_observe = {name: [] for name in SETTINGS}, [], 0.0, 0.0
    times, first = np.unique(evaluated[:, 3], return_index=True)
    for a, b in zip(first, list(first[1:]) + [len(evaluated)]):
        q = evaluated[a:b]
        ta = time.perf_counter()
        r, l = model.evaluate_forecast(obs, q, all_triplets=known, max_batch=args.max_batch)
        torch.cuda.synchronize()
        tb = time.perf_counter()
        index = getattr(obs.device, '_filter_index', None)
        obs = obs.observe(q, global_model)
        obs.device._filter_index = index                               # (the index of `known`, not of the store's own facts)
        torch.cuda.synchronize()
        t_forecast, t_observe = t_forecast + tb - ta, t_observe + time.perf_counter() - tb
        for name in SETTINGS:
            ranks[name].append(r[name])
        loss.append(l)
    ranks, loss = {name: np.concatenate(v) for name, v in ranks.items()}, np.concatenate(loss)
    print('observed-history protocol as a forecast / observe loop, %s split of %s: %d quadruples at %d timestamps; setup %.2f s, '
          'forecasts %.2f s, observes %.2f s (%.1f ms per timestamp)'
          % (args.split, data_dir, len(evaluated), len(times), t1 - t0, t_forecast, t_observe, 1e3 * t_observe / max(len(times), 1)))
    print('mean loss %.6f' % float(np.mean(loss)))
    for name in SETTINGS:
        m = U.rank_metrics(ranks[name])
        print('%-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
              % (name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
    print(json.dumps({'protocol': 'observed', 'loop': 'forecast/observe', 'split': args.split, 'n': int(len(evaluated)),
                      'metrics': {name: U.rank_metrics(ranks[name]) for name in SETTINGS}}))


def rollout_loop(args, model, global_model, splits, num_ent, num_rels, data_dir):
    """--rollout H: RENet.evaluate_rollout over the split, from the facts before it."""
    import numpy as np
    import torch
    import utils as U
    from model import SETTINGS
    from preprocess import ObservedStream
    present = [q for q in splits if q is not None]
    known = np.concatenate(present)                                    # what the filtered settings filter by, as the plain pass
    k = [n for n, q in zip(('train', 'valid', 'test'), splits) if q is not None].index(args.split)
    evaluated = present[k]
    start = present[:k] + [np.zeros((0, 4), dtype=np.int64)]
    if len(start) < 2:
        raise SystemExit('nothing lies before the %s split' % args.split)
    t0 = time.perf_counter()
    obs = ObservedStream(start, num_ent, num_rels, args.seq_len)
    obs.resident(model, global_model)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    model.num_k = args.num_k
    ranks, loss = model.evaluate_rollout(obs, evaluated, args.rollout, global_model, all_triplets=known, max_batch=args.max_batch)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    log = model.last_rollout
    print('observed-history protocol, ROLLOUT horizon H = %d, %s split of %s: %d quadruples at %d timestamps; setup %.2f s, '
          'pass %.2f s; %d generated timestamps, %d generated facts of which %d true'
          % (args.rollout, args.split, data_dir, len(evaluated), len(np.unique(evaluated[:, 3])), t1 - t0, t2 - t1, len(log),
             sum(e['generated'] for e in log), sum(e['true'] for e in log)))
    print('mean loss %.6f' % float(np.mean(loss)))
    for name in SETTINGS:
        m = U.rank_metrics(ranks[name])
        print('%-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
              % (name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
    print(json.dumps({'horizon': args.rollout, 'protocol': 'observed', 'loop': 'rollout', 'split': args.split,
                      'n': int(len(evaluated)), 'metrics': {name: U.rank_metrics(ranks[name]) for name in SETTINGS}}))


def online_loop(args, model, global_model, splits, num_ent, num_rels, data_dir):
    """--online [STEPS]: RENet.evaluate_online over the split, from the facts before it."""
    import numpy as np
    import torch
    import parallel
    import utils as U
    from model import SETTINGS
    from preprocess import ObservedStream
    present = [q for q in splits if q is not None]
    known = np.concatenate(present)                                    # what the filtered settings filter by, as the plain pass
    k = [n for n, q in zip(('train', 'valid', 'test'), splits) if q is not None].index(args.split)
    evaluated = present[k]
    start = present[:k] + [np.zeros((0, 4), dtype=np.int64)]
    if len(start) < 2:
        raise SystemExit('nothing lies before the %s split' % args.split)
    t0 = time.perf_counter()
    obs = ObservedStream(start, num_ent, num_rels, args.seq_len)
    obs.resident(model, global_model)
    opt = parallel.HipAdam(model, lr=args.lr, weight_decay=1e-5, max_norm=1.0)
    gopt = parallel.HipAdam(global_model, lr=args.lr, weight_decay=1e-5, max_norm=1.0) if args.online_global else None
    prior, gate_opt = None, None
    if args.recurrence is not None:
        import recurrence
        if args.learn_copy:
            prior = recurrence.CopyGate(num_rels, alpha=args.recurrence, half_life=args.half_life,
                                        learn_half_life=args.learn_half_life).to(next(model.parameters()).device)
            gate_opt = torch.optim.Adam(prior.parameters(), lr=args.gate_lr)
        else:
            prior = recurrence.RecurrencePrior(args.recurrence, args.half_life)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ranks, loss, log = model.evaluate_online(obs, evaluated, global_model, opt, steps=args.online, replay=args.replay,
                                             global_optimizer=gopt, all_triplets=known, max_batch=args.max_batch, prior=prior,
                                             learn_prior=args.learn_copy, gate_optimizer=gate_opt)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    n_t = len(log)
    print('observed-history protocol, ONLINE learning (%d step(s) per timestamp, replay %d, global model %s, lr %g), %s split of '
          '%s: %d quadruples at %d timestamps; setup %.2f s, pass %.2f s (%.1f ms per timestamp)'
          % (args.online, args.replay, 'learning' if gopt is not None else 'fixed', args.lr, args.split, data_dir, len(evaluated),
             n_t, t1 - t0, t2 - t1, 1e3 * (t2 - t1) / max(n_t, 1)))
    print('the weights that rank timestamp t have been trained on every evaluated timestamp before t: these numbers are not '
          'those of the static observed, stale-horizon, rollout or multi-step protocols')
    if prior is not None:
        half = 'none (frequency only)' if prior.half_life is None else '%g' % prior.half_life
        if args.learn_copy:
            tab = prior.table().detach().cpu().numpy()
            print('MODEL MIXED WITH THE RECURRENCE PRIOR, LEARNED GATE (online, trained through the mix; initial alpha %g, '
                  'half-life %s, gate lr %g): the gate that ranks timestamp t was fitted on the evaluated timestamps before t; '
                  'gates now: ob side %.3f .. %.3f, sub side %.3f .. %.3f.  Comparable only with numbers of this protocol.'
                  % (args.recurrence, half, args.gate_lr, tab[0].min(), tab[0].max(), tab[1].min(), tab[1].max()))
            if args.learn_half_life:
                print(half_life_line(prior))
        else:
            print('MODEL MIXED WITH THE RECURRENCE PRIOR in the forecast half, fixed alpha %g, half-life %s; learning is not '
                  'touched by it' % (prior.alpha, half))
    step_losses = [x for e in log for x in e['losses']]
    if step_losses:
        print('mean learn-step loss %.6f (first timestamp %.6f, last %.6f)'
              % (float(np.mean(step_losses)), float(np.mean(log[0]['losses'])), float(np.mean(log[-1]['losses']))))
    print('mean loss %.6f' % float(np.mean(loss)))
    for name in SETTINGS:
        m = U.rank_metrics(ranks[name])
        print('%-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
              % (name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
    print(json.dumps({'protocol': 'observed', 'loop': 'online', 'steps': args.online, 'replay': args.replay,
                      'global_model_learns': gopt is not None, 'lr': args.lr, 'split': args.split, 'n': int(len(evaluated)),
                      'recurrence': None if prior is None else {'alpha': args.recurrence, 'half_life': args.half_life,
                                                                'gate_learned': bool(args.learn_copy),
                                                                **(half_life_record(prior) if args.learn_half_life else {})},
                      'metrics': {name: U.rank_metrics(ranks[name]) for name in SETTINGS}}))


def half_life_record(gate):
    """{'half_life_learned': True, 'learned_half_lives': {side: {'min', 'median', 'max'}}} of a gate that learns its decay."""
    import numpy as np
    hl = gate.half_lives()
    return {'half_life_learned': True,
            'learned_half_lives': {side: {'min': float(hl[k].min()), 'median': float(np.median(hl[k])), 'max': float(hl[k].max())}
                                   for k, side in enumerate(('ob', 'sub'))}}


def half_life_line(gate):
    rec = half_life_record(gate)['learned_half_lives']
    return ('LEARNED HALF-LIVES per side and relation (initial %g), min / median / max: ob side %.4g / %.4g / %.4g, sub side '
            '%.4g / %.4g / %.4g' % ((gate.half_life,) + tuple(rec[s][k] for s in ('ob', 'sub') for k in ('min', 'median', 'max'))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('data_dir')
    ap.add_argument('--n-hidden', type=int, required=True)
    ap.add_argument('--seq-len', type=int, required=True)
    ap.add_argument('--split', choices=('valid', 'test'), default='test')
    ap.add_argument('--topk', type=int, default=0, help='also write the K best time-aware filtered predictions per query')
    ap.add_argument('--events', type=int, nargs='?', const=0, default=None, metavar='K',
                    help='also rank the gold (relation, entity) pairs; with K, print the K best forecasts of the first queries')
    ap.add_argument('--model-dir', default=None)
    ap.add_argument('--maxpool', type=int, default=1)
    ap.add_argument('--max-batch', type=int, default=4096)
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--horizon', type=int, default=None, metavar='H',
                    help='evaluate with histories up to H - 1 timestamps stale (blocks of H timestamps of the split)')
    ap.add_argument('--queries', default=None, metavar='FILE', help='TSV of open queries `s r o t` (-1: an absent side)')
    ap.add_argument('--k', type=int, default=10, help='predictions per open query (--queries)')
    ap.add_argument('--observe-loop', action='store_true',
                    help='forecast the split timestamp by timestamp, observing each timestamp on the device after its forecast')
    ap.add_argument('--rollout', type=int, default=None, metavar='H',
                    help='rollout horizon: observe the truth every H timestamps, feed generated facts to the steps in between')
    ap.add_argument('--num-k', type=int, default=1000, help='continuations kept per direction and generated timestamp (--rollout)')
    ap.add_argument('--online', type=int, nargs='?', const=1, default=None, metavar='STEPS',
                    help='online learning: after every observed timestamp, STEPS training steps on its facts (default 1)')
    ap.add_argument('--replay', type=int, default=0, help='earlier timestamps whose facts join every learn step (--online)')
    ap.add_argument('--online-global', action='store_true',
                    help='the global model learns too: one step per timestamp, then the resident table is refreshed (--online)')
    ap.add_argument('--lr', type=float, default=1e-3, help='learning rate of the online steps (--online)')
    ap.add_argument('--recurrence', type=float, default=None, metavar='ALPHA',
                    help='also print the recurrence baseline alone and the model mixed with it at weight ALPHA in [0, 1)')
    ap.add_argument('--half-life', type=float, default=None, metavar='H',
                    help='half-life of the recurrence prior in raw timestamp units (default: frequency only)')
    ap.add_argument('--fit-gate', type=int, default=None, metavar='STEPS',
                    help='fit a per-relation gate on the valid split (model frozen), then evaluate mixed with it (--recurrence); with '
                         '--events: fit the EVENT gate instead, one gate per side through the joint mix, and print the event '
                         'numbers with it')
    ap.add_argument('--learn-copy', action='store_true',
                    help='online steps train through the mix and the gates learn along the stream (--online --recurrence)')
    ap.add_argument('--learn-half-life', action='store_true',
                    help='the gate also learns one half-life per side and relation, from H (--recurrence --half-life with '
                         '--fit-gate or --online --learn-copy); with --events --fit-gate: one half-life per side')
    ap.add_argument('--gate-lr', type=float, default=1e-2, help='learning rate of the gate (--fit-gate, --learn-copy)')
    args = ap.parse_args()
    if args.recurrence is not None:
        if not 0.0 <= args.recurrence < 1.0 or (args.half_life is not None and args.half_life <= 0):
            raise SystemExit('--recurrence takes ALPHA in [0, 1), --half-life a positive H')
        if args.observe_loop or args.rollout is not None or args.queries is not None:
            raise SystemExit('--recurrence goes with the plain pass, --horizon and --online only')
        if (args.fit_gate is not None or args.learn_copy) and not args.recurrence > 0.0:
            raise SystemExit('a learned gate starts from ALPHA in (0, 1)')
        if args.fit_gate is not None and (args.fit_gate < 1 or args.online is not None):
            raise SystemExit('--fit-gate takes STEPS >= 1 and goes with the plain pass and --horizon')
        if args.learn_copy and args.online is None:
            raise SystemExit('--learn-copy belongs to --online --recurrence')
        if args.learn_half_life and (args.half_life is None or not (args.fit_gate is not None or args.learn_copy)):
            raise SystemExit('--learn-half-life needs --half-life H (its initial value) and --fit-gate or --online --learn-copy')
    elif args.half_life is not None or args.fit_gate is not None or args.learn_copy or args.learn_half_life:
        raise SystemExit('--half-life, --fit-gate, --learn-copy and --learn-half-life belong to --recurrence')
    if args.online is not None:
        if args.online < 0 or args.replay < 0:
            raise SystemExit('--online and --replay must be >= 0')
        if args.horizon is not None or args.observe_loop or args.queries is not None or args.events is not None or \
                args.rollout is not None or args.topk:
            raise SystemExit('--online is exclusive with --horizon, --observe-loop, --rollout, --queries, --events and --topk')
    if args.horizon is not None and args.horizon < 1:
        raise SystemExit('--horizon must be >= 1')
    if args.rollout is not None:
        if args.rollout < 1:
            raise SystemExit('--rollout must be >= 1')
        if args.horizon is not None or args.observe_loop or args.queries is not None or args.events is not None:
            raise SystemExit('--rollout is exclusive with --horizon, --observe-loop, --queries and --events')

    os.environ.setdefault('TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD', '1')      # (the drivers' checkpoints hold numpy arrays)
    import numpy as np
    import torch
    import utils as U
    from global_model import RENet_global
    from model import RENet, SETTINGS
    from preprocess import ObservedStream

    data_dir = os.path.abspath(args.data_dir)
    model_dir = args.model_dir or os.path.join('models', os.path.basename(data_dir.rstrip(os.sep)))
    num_ent, num_rels = U.get_total_number(data_dir, 'stat.txt')
    splits = [U.load_quadruples(data_dir, 'train.txt')[0]]
    splits.append(U.load_quadruples(data_dir, 'valid.txt')[0] if os.path.isfile(os.path.join(data_dir, 'valid.txt')) else None)
    splits.append(U.load_quadruples(data_dir, 'test.txt')[0])
    if args.split == 'valid' and splits[1] is None:
        raise SystemExit('%s has no valid.txt' % data_dir)

    dev = torch.device('cuda:%d' % args.gpu)
    torch.cuda.set_device(dev)
    model = RENet(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len)
    global_model = RENet_global(num_ent, args.n_hidden, num_rels, dropout=0.0, seq_len=args.seq_len, maxpool=args.maxpool)
    load = lambda name: torch.load(os.path.join(model_dir, name), map_location='cpu')['state_dict']
    model.load_state_dict(load('rgcn.pth'))
    names = ['max%drgcn_global2.pth' % args.maxpool, 'max%drgcn_global.pth' % args.maxpool]
    found = [n for n in names if os.path.isfile(os.path.join(model_dir, n))]
    if not found:
        raise SystemExit('no global model checkpoint in %s (%s)' % (model_dir, ' / '.join(names)))
    global_model.load_state_dict(load(found[0]))
    model.to(dev).eval()
    global_model.to(dev).eval()

    if args.observe_loop:
        if args.horizon is not None or args.queries is not None or args.events is not None or args.topk:
            raise SystemExit('--observe-loop runs the plain metrics only')
        return observe_loop(args, model, global_model, splits, num_ent, num_rels, data_dir)
    if args.rollout is not None:
        return rollout_loop(args, model, global_model, splits, num_ent, num_rels, data_dir)
    if args.online is not None:
        return online_loop(args, model, global_model, splits, num_ent, num_rels, data_dir)

    t0 = time.perf_counter()
    obs = ObservedStream(splits, num_ent, num_rels, args.seq_len)
    obs.resident(model, global_model)
    idx = obs.positions(args.split)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if args.queries is not None:
        q = np.loadtxt(args.queries, dtype=np.int64, ndmin=2)[:, :4]
        got = model.forecast_topk(obs, q, k=args.k, setting='time_filtered',
                                  sides=[n for n, c in (('sub', 2), ('ob', 0)) if (q[:, c] >= 0).any()])
        got = {name: [x.cpu().numpy() for x in v] for name, v in got.items()}
        for i, (s, r, o, t) in enumerate(q.tolist()):
            for name, given, what in (('ob', s, 'objects of (%d, %d, ?, %d)' % (s, r, t)), ('sub', o, 'subjects of (?, %d, %d, %d)' % (r, o, t))):
                if given >= 0:
                    ent, _, logp, n_valid = got[name]
                    print(what + ': ' + ', '.join('%d %.3f' % (ent[i, j], logp[i, j]) for j in range(int(n_valid[i]))))
        return
    if args.horizon is None:
        ranks, loss = model.evaluate_observed(obs, idx, max_batch=args.max_batch)
    else:
        ranks, loss = model.evaluate_forecast(obs, obs.allq[idx], as_of=obs.horizon_as_of(idx, args.horizon),
                                              max_batch=args.max_batch)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print('observed-history protocol (single-step), %s split of %s: %d quadruples; setup %.2f s, pass %.2f s (%.0f quadruples/s)'
          % (args.split, data_dir, len(idx), t1 - t0, t2 - t1, len(idx) / max(t2 - t1, 1e-9)))
    if args.horizon is not None:
        print('STALE histories, horizon H = %d: as of the first timestamp of every block of %d timestamps of the split'
              % (args.horizon, args.horizon))
    print('mean loss %.6f' % float(np.mean(loss)))
    for name in SETTINGS:
        m = U.rank_metrics(ranks[name])
        print('%-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
              % (name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
    record = {'protocol': 'observed', 'split': args.split, 'n': int(len(idx)),
              'metrics': {name: U.rank_metrics(ranks[name]) for name in SETTINGS}}
    if args.horizon is not None:
        record['horizon'] = args.horizon
    print(json.dumps(record))
    if args.recurrence is not None:
        import recurrence
        prior = recurrence.RecurrencePrior(args.recurrence, args.half_life)
        as_of = None if args.horizon is None else obs.horizon_as_of(idx, args.horizon)
        t3 = time.perf_counter()
        base_ranks, base_loss = recurrence.evaluate(obs, obs.allq[idx], prior, as_of=as_of, max_batch=args.max_batch)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        mix_ranks, mix_loss = model.evaluate_forecast(obs, obs.allq[idx], as_of=as_of, max_batch=args.max_batch, prior=prior)
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        for label, rk, ls, dt in (('RECURRENCE BASELINE ALONE (no model)', base_ranks, base_loss, t4 - t3),
                                  ('MODEL MIXED WITH THE RECURRENCE PRIOR', mix_ranks, mix_loss, t5 - t4)):
            print('%s, alpha %g, half-life %s: pass %.2f s (%.0f quadruples/s), mean loss %.6f'
                  % (label, prior.alpha, 'none (frequency only)' if prior.half_life is None else '%g' % prior.half_life, dt,
                     len(idx) / max(dt, 1e-9), float(np.mean(ls))))
            for name in SETTINGS:
                m = U.rank_metrics(rk[name])
                print('%-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
                      % (name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
        print('(the unmixed model is the block above; all three share the protocol, the filters and the tie rule)')
        extra = dict(record, recurrence={'alpha': prior.alpha, 'half_life': prior.half_life},
                     baseline={name: U.rank_metrics(base_ranks[name]) for name in SETTINGS},
                     mixed={name: U.rank_metrics(mix_ranks[name]) for name in SETTINGS})
        print(json.dumps(extra))
        if args.fit_gate is not None and args.events is None:            # (with --events the EVENT gate is fitted instead, below)
            if splits[1] is None:
                raise SystemExit('--fit-gate fits on the valid split: %s has no valid.txt' % data_dir)
            gate = recurrence.CopyGate(num_rels, alpha=args.recurrence, half_life=args.half_life,
                                       learn_half_life=args.learn_half_life).to(dev)
            t6 = time.perf_counter()
            fit = recurrence.fit_gate(model, obs, obs.positions('valid'), gate, torch.optim.Adam(gate.parameters(), lr=args.gate_lr),
                                      steps=args.fit_gate, max_batch=args.max_batch)
            torch.cuda.synchronize()
            t7 = time.perf_counter()
            gate_ranks, gate_loss = model.evaluate_forecast(obs, obs.allq[idx], as_of=as_of, max_batch=args.max_batch, prior=gate)
            torch.cuda.synchronize()
            t8 = time.perf_counter()
            tab = gate.table().detach().cpu().numpy()
            print('MODEL MIXED WITH THE RECURRENCE PRIOR, LEARNED GATE per side and relation (fitted on the valid split%s, model '
                  'frozen, observed histories, %d Adam steps at lr %g from alpha %g, half-life %s): fit %.2f s, mean mixed loss of '
                  'the valid split %.6f -> %.6f; gates ob side %.3f .. %.3f, sub side %.3f .. %.3f; pass %.2f s (%.0f '
                  'quadruples/s), mean loss %.6f'
                  % (' -- THE EVALUATED SPLIT ITSELF' if args.split == 'valid' else '', args.fit_gate, args.gate_lr, args.recurrence,
                     'none (frequency only)' if gate.half_life is None else '%g' % gate.half_life, t7 - t6, fit[0], fit[-1],
                     tab[0].min(), tab[0].max(), tab[1].min(), tab[1].max(), t8 - t7, len(idx) / max(t8 - t7, 1e-9),
                     float(np.mean(gate_loss))))
            if args.learn_half_life:
                print(half_life_line(gate))
            for name in SETTINGS:
                m = U.rank_metrics(gate_ranks[name])
                print('%-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
                      % (name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
            print('(a LEARNED gate: the same protocol, filters and tie rule as the blocks above, but the gate has seen the valid '
                  'split -- comparable only with numbers obtained the same way)')
            print(json.dumps(dict(record, recurrence={'alpha': args.recurrence, 'half_life': gate.half_life, 'gate_learned': True,
                                                      'fitted_on': 'valid', 'fit_steps': args.fit_gate, 'gate_lr': args.gate_lr,
                                                      **(half_life_record(gate) if args.learn_half_life else {})},
                                  mixed_learned_gate={name: U.rank_metrics(gate_ranks[name]) for name in SETTINGS})))
    if args.events is not None:
        def event_pass(label, run):
            t3 = time.perf_counter()
            ev = run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t3
            print('%s, columns (given o: pairs (r, s) | given s: pairs (r, o)): pass %.2f s (%.0f quadruples/s), '
                  'mean log p of the gold event %.4f | %.4f' % ((label, dt, len(idx) / max(dt, 1e-9)) + tuple(ev['logp'].mean(axis=0))))
            for kind, what in (('pair', 'pair (r, entity) among R x N_ent'), ('relation', 'relation given both endpoints')):
                for name in SETTINGS:
                    m = U.rank_metrics(ev[kind][name])
                    print('%-30s %-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
                          % (what, name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
            return {kind: {name: U.rank_metrics(ev[kind][name]) for name in SETTINGS} for kind in ('pair', 'relation')}

        event_record = {'protocol': 'observed', 'task': 'events', 'split': args.split, 'n': int(len(idx))}
        if args.recurrence is None:
            event_record['metrics'] = event_pass('event forecasts', lambda: model.evaluate_events_observed(obs, idx))
        else:
            # three blocks of ONE protocol (histories as of each query's own t, the same groups, filter lists and tie rule),
            # each labelled with the prior's alpha and half-life: they go beside each other and beside nothing else
            import recurrence
            prior = recurrence.RecurrencePrior(args.recurrence, args.half_life)
            tag = 'alpha %g, half-life %s' % (prior.alpha, 'none (frequency only)' if prior.half_life is None else '%g' % prior.half_life)
            event_record['recurrence'] = {'alpha': prior.alpha, 'half_life': prior.half_life}
            if args.fit_gate is not None:
                # the EVENT gate: one gate (and, with --learn-half-life, one decay) per side, fitted through the joint mix on
                # the valid split with the model frozen -- a protocol of its own, reported with what it started from
                if splits[1] is None:
                    raise SystemExit('--fit-gate fits on the valid split: %s has no valid.txt' % data_dir)
                egate = recurrence.CopyGate(num_rels, alpha=args.recurrence, half_life=args.half_life, per_relation=False,
                                            learn_half_life=args.learn_half_life).to(dev)
                t3 = time.perf_counter()
                efit = recurrence.fit_event_gate(model, obs, obs.positions('valid'), egate,
                                                 torch.optim.Adam(egate.parameters(), lr=args.gate_lr), steps=args.fit_gate,
                                                 max_batch=args.max_batch)
                torch.cuda.synchronize()
                alphas, rates = recurrence.event_scalars(egate)
                lives = {k: (None if v == 0.0 else 1.0 / v) for k, v in rates.items()}
                print('EVENT GATE fitted on the valid split%s (model frozen, %d Adam steps at lr %g from alpha %g, half-life %s): '
                      'fit %.2f s, mean joint loss of the valid split %.6f -> %.6f; alpha ob side %.4f, sub side %.4f; half-life '
                      'ob side %s, sub side %s'
                      % (' -- THE EVALUATED SPLIT ITSELF' if args.split == 'valid' else '', args.fit_gate, args.gate_lr,
                         args.recurrence, 'none (frequency only)' if args.half_life is None else '%g' % args.half_life,
                         time.perf_counter() - t3, efit[0], efit[-1], alphas['ob'], alphas['sub'],
                         *('none' if lives[k] is None else '%.4g' % lives[k] for k in ('ob', 'sub'))))
                event_record['fitted_gate'] = {'alpha': alphas, 'half_life': lives, 'fitted_on': 'valid', 'fit_steps': args.fit_gate,
                                               'gate_lr': args.gate_lr, 'initial_alpha': args.recurrence,
                                               'initial_half_life': args.half_life, 'learn_half_life': bool(args.learn_half_life)}
                event_record['mixed_fitted_gate'] = event_pass(
                    'event forecasts, MODEL MIXED WITH THE FITTED EVENT GATE (a protocol of its own: report it with the initial %s, '
                    'the fitting split, %d steps and lr %g)' % (tag, args.fit_gate, args.gate_lr),
                    lambda: model.evaluate_events_observed(obs, idx, prior=egate))
            event_record['baseline'] = event_pass('event forecasts, RECURRENCE BASELINE ALONE (no model), %s' % tag,
                                                  lambda: recurrence.evaluate_events(obs, idx, prior))
            event_record['mixed'] = event_pass('event forecasts, MODEL MIXED WITH THE RECURRENCE PRIOR, %s' % tag,
                                               lambda: model.evaluate_events_observed(obs, idx, prior=prior))
            event_record['metrics'] = event_pass('event forecasts, THE MODEL ALONE (beside the blocks at %s)' % tag,
                                                 lambda: model.evaluate_events_observed(obs, idx))
        print(json.dumps(event_record))
        if args.events > 0:
            few = idx[:5]
            rel, ent, logp, n_valid = (x.cpu().numpy() for x in
                                       model.predict_events_observed(obs, few, k=args.events, setting='time_filtered')['ob'])
            for i, (s, r, o, t) in enumerate(obs.allq[few].tolist()):
                print('t = %d, subject %d (gold: relation %d, object %d): ' % (t, s, r, o) +
                      ', '.join('(%d, %d) %.3f' % (rel[i, j], ent[i, j], logp[i, j]) for j in range(int(n_valid[i]))))
    if args.topk > 0:
        out = os.path.join(model_dir, 'observed_top%d_%s.npz' % (args.topk, args.split))
        parts = {'sub_idx': [], 'sub_logp': [], 'ob_idx': [], 'ob_logp': []}
        for c in range(0, len(idx), args.max_batch):
            got = model.predict_topk_observed(obs, idx[c:c + args.max_batch], k=args.topk, setting='time_filtered')
            for side in ('sub', 'ob'):
                parts[side + '_idx'].append(got[side][0].cpu().numpy())
                parts[side + '_logp'].append(got[side][2].cpu().numpy())
        np.savez(out, quads=obs.allq[idx], **{k: np.concatenate(v) for k, v in parts.items()})
        print('top-%d time-aware filtered predictions per query written to %s' % (args.topk, out))


if __name__ == '__main__':
    main()
