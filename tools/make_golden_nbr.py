#!/usr/bin/env python
"""Generates the fixtures of the mean / attentive neighbour aggregators by RUNNING THE UNMODIFIED REFERENCE classes
(Aggregator.MeanAggregator, gcn=False / True, and Aggregator.AttnAggregator) on CPU through oracle/ref_loader.py, in eval
mode with fixed seeds.  Runs only where the reference tree is available, like tools/make_golden.py.

    python tools/make_golden_nbr.py

Writes tests/golden/nbr_agg_{mean,gcn,attn}_{100,200}.npz.  Shape: 40 entities, 6 relations, 12 sequences, seq_len 4,
neighbour lists of 1-9 ids with repeats, two empty sequences, several sequences of equal length.  Every file holds
  inputs       s, r, the histories flattened (seq_ptr, nbr_ptr, nbr_o), ent_embeds, rel_embeds
  parameters   param_names / param_shapes / param_seed (values: oracle.fixtures.make_params(param_seed, shapes)) and
               param.<name> itself for the small ones
  reference    s_idx (its length sort), len_s and flat_s (its flattened batch), packed_data, batch_sizes,
               pred_* (predict() of one history), h_n of an nn.GRU fed with the packed input (weights: gru_seed),
               C and grad.<name> = d sum(packed.data * C) / d<name> for every parameter, ent_embeds and rel_embeds
               (large ones as norm + seeded samples, tools/make_golden.py:pack_tensor)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as mg   # noqa: E402
from oracle import fixtures, ref_loader   # noqa: E402

NUM_ENT, NUM_RELS, NUM_SEQ, SEQ_LEN = 40, 6, 12, 4
SMALL = fixtures.BIG


def make_histories(rng):
    """12 sequences: lengths with ties, two of them empty; lists of 1-9 neighbour ids with repeats."""
    lens = [4, 2, 0, 3, 4, 1, 2, 0, 3, 2, 4, 1]
    hist = []
    for n in lens:
        steps = []
        for _ in range(n):
            k = int(rng.randint(1, 10))
            ids = rng.randint(0, NUM_ENT, size=k)
            if k >= 3:
                ids[-1] = ids[0]                              # a repeat inside the list
            steps.append(ids.astype(np.int64))
        hist.append(steps)
    return hist


def gru_shapes(inp, h):
    return {'weight_ih_l0': (3 * h, inp), 'weight_hh_l0': (3 * h, h), 'bias_ih_l0': (3 * h,), 'bias_hh_l0': (3 * h,)}


def gen(kind, d):
    ref = ref_loader.load()
    seed = {'mean': 1, 'gcn': 2, 'attn': 3}[kind] * 1000 + d
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    hist = make_histories(rng)
    s = rng.randint(0, NUM_ENT, size=NUM_SEQ).astype(np.int64)
    r = rng.randint(0, NUM_RELS, size=NUM_SEQ).astype(np.int64)
    emb = fixtures.make_params(seed + 1, {'ent_embeds': (NUM_ENT, d), 'rel_embeds': (NUM_RELS, d)}, scale=0.5)
    A = ref.Aggregator
    agg = A.AttnAggregator(d, 0.2, seq_len=SEQ_LEN) if kind == 'attn' else \
        A.MeanAggregator(d, 0.2, seq_len=SEQ_LEN, gcn=(kind == 'gcn'))
    agg.eval()
    shapes = {k: tuple(v.shape) for k, v in agg.state_dict().items()}
    params = fixtures.make_params(seed + 2, shapes)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    width = (3 if kind == 'attn' else 2) * d
    gru_seed = seed + 3
    gw = fixtures.make_params(gru_seed, gru_shapes(width, d), scale=1.0 / np.sqrt(d))
    gru = torch.nn.GRU(width, d, batch_first=True)
    gru.load_state_dict({k: torch.from_numpy(v) for k, v in gw.items()})

    ent = torch.from_numpy(emb['ent_embeds']).requires_grad_(True)
    rel = torch.from_numpy(emb['rel_embeds']).requires_grad_(True)
    s_t, r_t = torch.from_numpy(s), torch.from_numpy(r)
    out = {}
    with ref_loader.cpu_mode():
        lens = torch.LongTensor(list(map(len, hist)))
        _, s_idx = lens.sort(0, descending=True)
        _, _, _, _, len_s, _ = ref.utils.get_sorted_s_r_embed(hist, s_t, r_t, ent)
        nz = int((lens > 0).sum())
        flat_s = np.concatenate([np.concatenate(hist[int(i)]) for i in s_idx[:nz]])
        packed = agg(hist, s_t, r_t, ent, rel)
        _, h_n = gru(packed)
        c = fixtures.make_params(seed + 4, {'C': tuple(packed.data.shape)}, scale=1.0)['C']
        (packed.data * torch.from_numpy(c)).sum().backward()
        pred_i = int(s_idx[0])
        with torch.no_grad():
            pred = agg.predict(hist[pred_i], s_t[pred_i], r_t[pred_i], ent, rel)
    seq_ptr = np.concatenate(([0], np.cumsum([len(h) for h in hist]))).astype(np.int64)
    steps = [a for h in hist for a in h]
    out.update(kind=kind, d=d, seq_len=SEQ_LEN, s=s, r=r, seq_ptr=seq_ptr,
               nbr_ptr=np.concatenate(([0], np.cumsum([len(a) for a in steps]))).astype(np.int64),
               nbr_o=np.concatenate(steps), ent_embeds=emb['ent_embeds'], rel_embeds=emb['rel_embeds'],
               param_names=json.dumps(sorted(shapes)), param_shapes=json.dumps({k: list(v) for k, v in shapes.items()}),
               param_seed=seed + 2, gru_seed=gru_seed, s_idx=s_idx.numpy(), len_s=np.asarray(len_s, np.int64),
               flat_s=flat_s, packed_data=packed.data.detach().numpy(), batch_sizes=packed.batch_sizes.numpy(),
               pred_index=pred_i, pred_out=pred.numpy(), h_n=h_n[0].detach().numpy(), C=c)
    for k, v in params.items():
        if v.size <= SMALL:
            out['param.' + k] = v
    for k, p in agg.named_parameters():
        mg.pack_tensor(out, 'grad.' + k, p.grad)
    mg.pack_tensor(out, 'grad.ent_embeds', ent.grad)
    mg.pack_tensor(out, 'grad.rel_embeds', rel.grad if rel.grad is not None else torch.zeros_like(rel))
    name = 'nbr_agg_%s_%d.npz' % (kind, d)
    np.savez_compressed(os.path.join(mg.OUT, name), **out)
    return name


def main():
    if not ref_loader.available():
        raise SystemExit('reference tree not available: fixtures can only be generated in the build container')
    for kind in ('mean', 'gcn', 'attn'):
        for d in (100, 200):
            f = gen(kind, d)
            size = os.path.getsize(os.path.join(mg.OUT, f))
            print('%-28s %8.1f KB' % (f, size / 1024.0))
            assert size < (1 << 19), f


if __name__ == '__main__':
    main()
