#!/usr/bin/env python
"""Generates the n_hidden = 300 fixtures by RUNNING THE UNMODIFIED REFERENCE on CPU through oracle/ref_loader.py, with
the generators of tools/make_golden.py (imported, not re-run: every existing fixture stays byte-identical).  Runs only
where the reference tree is available, like tools/make_golden.py.

    python tools/make_golden_d300.py

Writes only
  tests/golden/rgcn_300.npz              RGCNBlockLayer (3x3 relation blocks): the 64-entity / 7-relation / 150-fact recipe
  tests/golden/train_tiny_300.npz        model.RENet, both directions, seq_len 4, batch 40
  tests/golden/global_tiny_300_max1.npz  global_model.RENet_global, max pooling
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as mg   # noqa: E402

D = 300
FILES = ('rgcn_300.npz', 'train_tiny_300.npz', 'global_tiny_300_max1.npz')


def tiny_prep():
    """The reference preprocessing of the tiny dataset, as make_golden.gen_prep runs it, without writing prep_tiny.npz."""
    cfg, tr, va, te = mg.dataset('tiny')
    return mg.run_reference_preprocessing(tr, va, te, cfg['num_ent'], cfg['num_rels'])


def main():
    if not mg.ref_loader.available():
        raise SystemExit('reference tree not available: fixtures can only be generated in the build container')
    torch.manual_seed(0)
    mg.gen_rgcn(D)
    prep = tiny_prep()
    mg.gen_train('tiny', D, 4, 40, prep)
    mg.gen_global('tiny', D, 4, prep, 1)
    for f in FILES:
        size = os.path.getsize(os.path.join(mg.OUT, f))
        print('%-32s %8.1f KB' % (f, size / 1024.0))
        assert size < (1 << 20), f


if __name__ == '__main__':
    main()
