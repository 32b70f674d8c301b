"""Child process of tests/test_gpu_step_reductions.py: optimizer steps of the merged training step through the C launch list
(csrc/step.cpp) under the RENET_STEP_BATCH of the environment -- the switch is read once per process.

    python tests/step_reductions_run.py OUT.pt CONFIG [CONFIG ...]      CONFIG = hidden:streams:dropout-in-percent

The model is small (300 entities, 12 relations, 14 timestamps of ~60 facts, 48 quadruples per batch, 2 optimizer steps) and
its score head runs on planes (the class threshold of renet_hip.use_planes is lowered), so every part of the list is the one
the full-size step runs.  Saves {config: (losses, flat gradients per step, parameters, [forward launches, backward launches]
of the last step)} to OUT.pt.  The training loop is tests/test_gpu_step_plan.py's."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, 're-net_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def small_stream():
    import preprocess as P
    import synth
    synth.SHAPES['SMALL'] = (300, 12, 14, 60, 5, 24, 0.9, 2.2, 0.11)
    quads, num_ent, num_rels, _ = synth.make_stream('SMALL', seed=5)
    gd = P.build_graph_dict(quads, num_rels)
    return quads, num_ent, num_rels, gd, P.HistoryIndex(quads, 's', 10), P.HistoryIndex(quads, 'o', 10)


def main():
    import renet_hip as K
    import step_plan
    import test_gpu_step_plan as T
    K.PLANES_MIN_CLASSES = 256
    out_path, configs = sys.argv[1], sys.argv[2:]
    dev = torch.device('cuda:0')
    data = small_stream()
    res = {}
    for c in configs:
        hidden, n_streams, drop = (int(x) for x in c.split(':'))
        losses, flats, params, used = T._train(dev, data, True, drop / 100.0, steps=2, batch=48, hidden=hidden,
                                               side=n_streams == 2)
        assert all('StepFn' in u for u in used), used          # the C launch list really ran
        res[c] = (losses, [f.cpu() for f in flats], params.cpu(), list(step_plan.StepFn.last_launches))
    torch.save(res, out_path)
    print('ok', len(res))


if __name__ == '__main__':
    main()
