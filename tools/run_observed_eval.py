#!/usr/bin/env python
"""Observed-history (single-step, ground-truth history) evaluation of a trained model: raw, filtered and time-aware filtered
MRR / Hits of a split, every query at time t seeing all facts before t (the evaluated split's own included) -- the
protocol under which RE-GCN, xERTE and TITer report the time-aware filter.  NOT the reference's multi-step protocol
(test.py; RENet.evaluate_all_stream): the two answer different questions, their numbers must not be mixed.

    python tools/run_observed_eval.py DATA_DIR --n-hidden H --seq-len L [--split valid|test] [--topk K] [--events [K]]
                                      [--model-dir models/<DS>] [--maxpool 1] [--max-batch 4096] [--gpu 0]

--events adds the EVENT forecasts (RENet.evaluate_events_observed): MRR / Hits of the gold (relation, entity) pair among all
pairs of the given entity, and of the gold relation given both endpoints, in the three settings; with K also the K most
probable (relation, object) pairs of the first few queries (RENet.predict_events_observed, time-aware filtered).

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
    args = ap.parse_args()

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

    t0 = time.perf_counter()
    obs = ObservedStream(splits, num_ent, num_rels, args.seq_len)
    obs.resident(model, global_model)
    idx = obs.positions(args.split)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ranks, loss = model.evaluate_observed(obs, idx, max_batch=args.max_batch)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print('observed-history protocol (single-step), %s split of %s: %d quadruples; setup %.2f s, pass %.2f s (%.0f quadruples/s)'
          % (args.split, data_dir, len(idx), t1 - t0, t2 - t1, len(idx) / max(t2 - t1, 1e-9)))
    print('mean loss %.6f' % float(np.mean(loss)))
    for name in SETTINGS:
        m = U.rank_metrics(ranks[name])
        print('%-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
              % (name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
    print(json.dumps({'protocol': 'observed', 'split': args.split, 'n': int(len(idx)),
                      'metrics': {name: U.rank_metrics(ranks[name]) for name in SETTINGS}}))
    if args.events is not None:
        t3 = time.perf_counter()
        ev = model.evaluate_events_observed(obs, idx)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t3
        print('event forecasts, columns (given o: pairs (r, s) | given s: pairs (r, o)): pass %.2f s (%.0f quadruples/s), '
              'mean log p of the gold event %.4f | %.4f' % ((dt, len(idx) / max(dt, 1e-9)) + tuple(ev['logp'].mean(axis=0))))
        for kind, what in (('pair', 'pair (r, entity) among R x N_ent'), ('relation', 'relation given both endpoints')):
            for name in SETTINGS:
                m = U.rank_metrics(ev[kind][name])
                print('%-30s %-14s MRR %.6f  MR %.3f  Hits@1 %.6f  Hits@3 %.6f  Hits@10 %.6f'
                      % (what, name, m['mrr'], m['mr'], m['hits@1'], m['hits@3'], m['hits@10']))
        print(json.dumps({'protocol': 'observed', 'task': 'events', 'split': args.split, 'n': int(len(idx)),
                          'metrics': {kind: {name: U.rank_metrics(ev[kind][name]) for name in SETTINGS}
                                      for kind in ('pair', 'relation')}}))
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
