#!/usr/bin/env python
"""Stage split of one event-forecast pass (RENet.evaluate_events_observed) on the ICEWS18-shaped synthetic stream of
tools/observed_eval_bench.py (40 training timestamps + n_t evaluated ones, hidden 200, seq_len 10), and the two kernels of
csrc/joint_rank.hip against the torch formulation and against the bytes of the block they read.  GPU only; medians of five;
one JSON line (profiles/event_forecast.md).

    python tools/event_bench.py [positions] [n_t]        the first `positions` test positions (default 256, n_t 2)"""
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
REPS = 5


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _median(fn, reps=REPS):
    fn()                                                        # warm-up
    return float(np.median([_wall(fn)[0] for _ in range(reps)]))


def stages(net, obs, idx):
    """One pass with a device synchronisation after every stage (the stages do not overlap here): seconds per stage summed
    over the pass, and the operands of its first rank launch."""
    import model as M
    import renet_hip as K
    t = {'encoder once per chunk (builder, RGCN x2, assembly, encoder_r, p_base GEMMs)': 0.0, 'R-fold GRU': 0.0,
         'score GEMM (+ linear_r)': 0.0, 'offsets kernel': 0.0, 'rank kernel': 0.0}
    keys = list(t)
    state = {'in_chunk': False, 'first': None, 'groups': 0, 'queries': 0, 'blocks': 0}
    real = dict(chunks=M._event_chunks, gru=K.gru_fwd, lin=M._linear_eval, off=K.joint_row_offsets, rank=K.joint_rank_rows)

    def timed(key, fn):
        dt, out = _wall(fn)
        t[key] += dt
        return out

    def chunks(*a, **k):
        it = real['chunks'](*a, **k)
        while True:
            state['in_chunk'] = True
            try:
                ch = timed(keys[0], lambda: next(it, None))
            finally:
                state['in_chunk'] = False
            if ch is None:
                return
            yield ch

    def gru(*a, **k):
        return real['gru'](*a, **k) if state['in_chunk'] else timed(keys[1], lambda: real['gru'](*a, **k))

    def rank(block, R, off, group, *rest):
        if state['first'] is None:
            state['first'] = (block, R, off, group) + rest
        state['groups'] += block.shape[0] // R
        state['queries'] += group.numel()
        state['blocks'] += 1
        return timed(keys[4], lambda: real['rank'](block, R, off, group, *rest))
    M._event_chunks, K.gru_fwd, M._linear_eval = chunks, gru, lambda *a: timed(keys[2], lambda: real['lin'](*a))
    K.joint_row_offsets, K.joint_rank_rows = (lambda *a: timed(keys[3], lambda: real['off'](*a))), rank
    try:
        total, _ = _wall(lambda: net.evaluate_events_observed(obs, idx))
    finally:
        M._event_chunks, K.gru_fwd, M._linear_eval, K.joint_row_offsets, K.joint_rank_rows = \
            real['chunks'], real['gru'], real['lin'], real['off'], real['rank']
    t['everything else (host lookups, uploads, gathers, relation ranks)'] = total - sum(t.values())
    return {k: round(v, 5) for k, v in t.items()}, state


def kernels(net, first):
    """The two kernels on the operands of the pass's first rank launch against torch on the same device block: log_softmax
    and logsumexp for the offsets; add, compare, masked sums for the counts (the masks built outside the timed region)."""
    import renet_hip as K
    block, R, off, group, gold_r, gold_c, cols_a, start_a, count_a, cols_t, start_t, count_t = first
    rows, C = block.shape
    g, Q = rows // R, group.numel()
    logits_r = torch.randn(g, R, device=block.device)
    res = {'block': [rows, C], 'groups': g, 'queries': Q}
    t_off = _median(lambda: K.joint_row_offsets(block, R, logits_r))
    t_rank = _median(lambda: K.joint_rank_rows(block, R, off, group, gold_r, gold_c, cols_a, start_a, count_a, cols_t, start_t, count_t))
    torch_off = lambda: torch.log_softmax(logits_r, dim=1).view(-1) - torch.logsumexp(block, dim=1)
    t_off_torch = _median(torch_off)
    # the masks of the two filtered settings, [Q, R, C] bool each (True: a candidate), outside the timed region
    masks = []
    for cols, start, count in ((cols_a, start_a, count_a), (cols_t, start_t, count_t)):
        keep = torch.ones(Q * R, C, device=block.device, dtype=torch.bool)
        row = torch.repeat_interleave(torch.arange(Q * R, device=block.device), count.long())
        first_of = torch.repeat_interleave(torch.cumsum(count.long(), 0) - count.long(), count.long())
        at = start.long()[row] + torch.arange(row.numel(), device=block.device) - first_of
        keep[row, cols[at].long()] = False
        keep.view(Q, R, C)[torch.arange(Q, device=block.device), gold_r.long(), gold_c.long()] = True
        masks.append(keep.view(Q, R, C))

    def torch_rank():
        J = (block + off.view(-1, 1)).view(g, R, C)[group.long()]                       # [Q, R, C]
        v = J[torch.arange(Q, device=block.device), gold_r.long(), gold_c.long()].view(Q, 1, 1)
        gt, eq = J > v, J == v
        return [x.sum(dim=(1, 2)) for x in (gt, eq, gt & masks[0], eq & masks[0], gt & masks[1], eq & masks[1])]
    t_rank_torch = _median(torch_rank)
    want = torch.stack(torch_rank())
    got = K.joint_rank_rows(block, R, off, group, gold_r, gold_c, cols_a, start_a, count_a, cols_t, start_t, count_t)[0]
    res['counts equal the torch formulation'] = bool(torch.equal(want, got))
    b_off, b_rank = rows * C * 4.0, Q * R * C * 4.0
    res['offsets'] = {'kernel_s': t_off, 'torch_s': t_off_torch, 'bytes': b_off, 'TB_per_s': b_off / t_off / 1e12,
                      'at_copy_bandwidth_s': b_off / (COPY_TBS * 1e12), 'share_of_copy_bandwidth': b_off / t_off / 1e12 / COPY_TBS}
    res['rank'] = {'kernel_s': t_rank, 'torch_s': t_rank_torch, 'bytes': b_rank, 'TB_per_s': b_rank / t_rank / 1e12,
                   'at_copy_bandwidth_s': b_rank / (COPY_TBS * 1e12), 'share_of_copy_bandwidth': b_rank / t_rank / 1e12 / COPY_TBS}
    return res


def main():
    limit = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    n_t = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    dev = torch.device('cuda:0')
    net, obs, idx, setup_s = OB._observed_setup(n_t, dev)
    idx = idx[:limit]
    passes = [_wall(lambda: net.evaluate_events_observed(obs, idx))[0] for _ in range(REPS + 1)][1:]      # pass 0 warms up
    split = [stages(net, obs, idx) for _ in range(REPS)]
    med = {k: float(np.median([s[0][k] for s in split])) for k in split[0][0]}
    state = split[0][1]
    R, N, H = net.num_rels, net.in_dim, net.h_dim
    out = dict(shape=OB.SHAPE, hidden=H, relations=R, entities=N, positions=int(len(idx)), timestamps=n_t, reps=REPS,
               pass_median_s=float(np.median(passes)), positions_per_s=len(idx) / float(np.median(passes)),
               groups=state['groups'], queries=state['queries'], sub_blocks=state['blocks'],
               score_gemm_gflop_per_group=2.0 * R * N * 3 * H / 1e9, stages_synchronised_median_s=med,
               kernels_first_sub_block=kernels(net, state['first']))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
