"""Child process of tests/test_gpu_backward_batching.py: a few optimizer steps of the merged training step through the C
launch list (csrc/step.cpp) under the RENET_STEP_BATCH of the environment -- the switch is read once per process, so every
value needs a process of its own.

    python tests/step_batch_run.py OUT.pt CONFIG [CONFIG ...]      CONFIG = hidden:timestamps:batch:steps:streams

Saves {config: (losses, flat gradients per step, parameters, [forward launches, backward launches])} to OUT.pt.  The
training loop is the one of tests/test_gpu_step_plan.py (dropout 0.5, HipAdam, seeded)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, 're-net_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import step_plan
    import test_gpu_step_plan as T
    out_path, configs = sys.argv[1], sys.argv[2:]
    dev = torch.device('cuda:0')
    streams = {}
    res = {}
    for c in configs:
        hidden, num_t, batch, steps, n_streams = (int(x) for x in c.split(':'))
        if num_t not in streams:
            streams[num_t] = T._stream(num_t=num_t)
        losses, flats, params, used = T._train(dev, streams[num_t], True, 0.5, steps=steps, batch=batch, hidden=hidden,
                                               side=n_streams == 2)
        assert all('StepFn' in u for u in used), used          # the C launch list really ran
        res[c] = (losses, [f.cpu() for f in flats], params.cpu(), list(step_plan.StepFn.last_launches))
    torch.save(res, out_path)
    print('ok', len(res))


if __name__ == '__main__':
    main()
