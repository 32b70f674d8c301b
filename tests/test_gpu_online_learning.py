"""GPU tests of the online-learning protocol (re-net_amd/online.py; run with -m gpu on an MI355X): RENet.learn_observed,
RENet_global.learn_observed, ObservedStream.refresh_global and RENet.evaluate_online on a small hand-built stream -- 60
entities, 4 relations, 14 timestamps from 0 with 36-44 facts each, n_hidden 100, seq_len 4, dropout 0 unless stated.

What pins the meaning: a learn step equals, bit for bit, the same step taken on a clone through the HOST-built batch of the
same positions; the batched global table lies as close to a float64 restatement of predict() (oracle.renet_oracle, run in
float64) as twice the existing per-timestamp path does; the global step's loss and gradients equal the existing dense
float64 soft_cross_entropy path on the clean targets to the fp32 step-parity figures (1e-5 / 4e-5 relative L2); the online
loop with no learning is the forecast / observe loop bit for bit."""
import math

import numpy as np
import pytest
import torch

from helpers import O, fixtures, global_shapes, renet_shapes

pytestmark = pytest.mark.gpu

NUM_ENT, NUM_RELS, NUM_T, SEQ_LEN = 60, 4, 14, 4
T_RESIDENT = 10                                   # the resident stream: t < 10; evaluated online: t = 10 .. 13
SETTINGS = ('raw', 'filtered', 'time_filtered')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def make_facts(num_t=NUM_T, seed=11):
    """int64 [n, 4] = (s, r, o, t), time-ordered, t = 0 .. num_t - 1, 36-44 facts each, Zipf-like entities."""
    rng = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, NUM_ENT + 1) ** 0.7
    pop /= pop.sum()
    out = []
    for t in range(num_t):
        m = rng.randint(36, 45)
        q = np.stack((rng.choice(NUM_ENT, m, p=pop), rng.randint(0, NUM_RELS, m), rng.choice(NUM_ENT, m, p=pop),
                      np.full(m, t)), axis=1)
        out.append(q)
    return np.concatenate(out).astype(np.int64)


def stream_of(facts):
    import preprocess as P
    cut = len(facts) // 2
    cut = int(np.searchsorted(facts[:, 3], facts[cut, 3]))             # (a split border at a timestamp border)
    return P.ObservedStream((facts[:cut], facts[cut:]), NUM_ENT, NUM_RELS, SEQ_LEN)


def models(dev, d=100, dropout=0.0, seeds=(61, 62)):
    import global_model as GM
    import model as M
    net = M.RENet(NUM_ENT, d, NUM_RELS, dropout=dropout, seq_len=SEQ_LEN)
    gnet = GM.RENet_global(NUM_ENT, d, NUM_RELS, dropout=0.0, seq_len=SEQ_LEN, maxpool=1)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in fixtures.make_params(seeds[0], renet_shapes(NUM_ENT, NUM_RELS, d)).items()})
    gnet.load_state_dict({k: torch.from_numpy(v) for k, v in fixtures.make_params(seeds[1], global_shapes(NUM_ENT, NUM_RELS, d)).items()})
    return net.to(dev).eval(), gnet.to(dev).eval()


def clone_of(module, dev):
    """A fresh model of the same class and sizes with a copy of the weights, in eval mode (not a deepcopy: a model that has
    run keeps its last batch, device handles included)."""
    import model as M
    if isinstance(module, M.RENet):
        new = M.RENet(module.in_dim, module.h_dim, module.num_rels, dropout=module.drop_p, seq_len=module.seq_len)
    else:
        new = type(module)(module.in_dim, module.h_dim, module.num_rels, dropout=0.0, seq_len=module.seq_len, maxpool=1)
    new.load_state_dict({k: v.detach().cpu().clone() for k, v in module.state_dict().items()})
    return new.to(dev).eval()


_WORLD = {}


def world(dev):
    """The facts, the models and the resident stream of all 14 timestamps -- made once, shared, left unchanged (every test
    that trains does so on clones)."""
    if not _WORLD:
        facts = make_facts()
        per_t = np.bincount(facts[:, 3], minlength=NUM_T)
        assert len(per_t) == NUM_T and per_t.min() >= 36 and per_t.max() <= 44
        net, gnet = models(dev)
        obs = stream_of(facts)
        obs.resident(net, gnet)
        _WORLD.update(facts=facts, net=net, gnet=gnet, obs=obs)
    return _WORLD


def same_parameters(a, b):
    return all(torch.equal(p, q) for (_, p), (_, q) in zip(sorted(a.state_dict().items()), sorted(b.state_dict().items())))


# ---- refresh_global --------------------------------------------------------------------------------------------------
def _fp64_table(gnet, obs):
    """{key: predict()'s embedding in float64}: oracle.renet_oracle's global model on float64 copies of the weights, the keys
    and the times predicted by get_global_emb's rule."""
    params = {k: v.detach().cpu().double() for k, v in gnet.state_dict().items()}
    ogd = O.build_graph_dict(obs.allq, NUM_RELS)
    times = [int(t) for t in obs.times]
    unit = times[1] - times[0]
    assert times[0] == 0
    out = {}
    with torch.no_grad():
        for k, t in enumerate(times):
            nxt = times[k + 1] if k + 1 < len(times) else t + unit
            out[t] = O.global_predict(params, nxt, ogd, SEQ_LEN, subject=True, maxpool=1)[0].numpy()
    return out


@pytest.mark.parametrize('d,num_t', [(100, NUM_T), (200, NUM_T), (100, 3)], ids=['d100', 'd200', 'shorter-than-seq_len'])
def test_refresh_global_is_as_close_to_float64_as_twice_the_per_timestamp_path(dev, d, num_t):
    import online
    net, gnet = models(dev, d)
    obs = stream_of(make_facts(num_t))
    assert len(obs.times) == num_t
    store = obs.resident(net, gnet)
    glob0 = store.glob.clone()
    table = obs.global_table(gnet)
    new = obs.refresh_global(gnet)
    keys = [int(t) for t in new.device._glob_times]
    assert keys == sorted(int(t) for t in table.keys()) == [int(t) for t in online.global_table_batched(obs, gnet)[0]]
    ref = _fp64_table(gnet, obs)
    assert sorted(ref) == keys
    want = np.stack([ref[t] for t in keys])
    old = np.stack([table[t].reshape(-1).double().cpu().numpy() for t in keys])
    got = new.device.glob.double().cpu().numpy()
    assert got.shape == old.shape == want.shape == (len(keys), d)
    e_ref, e_new = float(np.abs(old - want).max()), float(np.abs(got - want).max())
    print('  global table d=%d T=%d: per-timestamp path |err| %.3e, batched |err| %.3e, scale %.3f'
          % (d, num_t, e_ref, e_new, float(np.abs(want).max())))
    assert e_ref > 0 and e_new <= 2 * e_ref
    # the old stream and its store stay valid and untouched; the new store shares every other table
    assert obs.device is store and new.device is not store and new.device.obs is new
    assert torch.equal(store.glob, glob0)
    assert new.device.t is store.t and new.device.quads is store.quads and new.graph_dict is obs.graph_dict
    # and it scores: the same positions through both stores, to GEMM rounding of the table
    idx = np.arange(len(obs) - 30, len(obs))
    a, b = net.observed_scores(obs, idx), net.observed_scores(new, idx)
    assert float((a[1] - b[1]).abs().max()) <= 1e-3 * float(a[1].abs().max())


# ---- RENet.learn_observed --------------------------------------------------------------------------------------------
def _optimizer(kind, module, lr=1e-3):
    import parallel
    if kind == 'hip':
        return parallel.HipAdam(module, lr=lr, weight_decay=1e-5, max_norm=1.0)
    return torch.optim.Adam(module.parameters(), lr=lr, weight_decay=1e-5)


def _host_step(net, opt, kind, obs, gnet, idx):
    """The same step through the HOST-built batch: prepare_both on the stream's own history index and graphs, the model's
    global_emb set to the stream's table."""
    import ops
    net.global_emb = obs.global_table(gnet)
    prep = net.prepare_both(obs.allq[idx], obs.hist_s.take(idx), obs.hist_o.take(idx), obs.graph_dict)
    assert prep is not None
    net.train()
    if kind == 'hip':
        with opt.step_scope(head_passes=1):
            loss = net.loss_prepared_both(prep)
            loss.backward()
            opt.step()
    else:
        loss = net.loss_prepared_both(prep)
        loss.backward()
        ops.join_deferred()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
    net.eval()
    return float(loss.detach())


@pytest.mark.parametrize('kind', ['hip', 'torch'])
def test_a_learn_step_equals_the_step_through_the_host_built_batch(dev, kind):
    w = world(dev)
    obs, gnet = w['obs'], w['gnet']
    idx = np.nonzero(obs.allq[:, 3] >= NUM_T - 3)[0]
    a, b = clone_of(w['net'], dev), clone_of(w['net'], dev)
    opt_a, opt_b = _optimizer(kind, a), _optimizer(kind, b)
    got = a.learn_observed(obs, idx, opt_a, steps=1, batch_size=1024)
    assert not a.training and len(got) == 1
    want = _host_step(b, opt_b, kind, obs, gnet, idx)
    print('  learn step (%s): loss %.6f, host-built %.6f' % (kind, got[0], want))
    assert got[0] == want
    assert same_parameters(a, b)
    assert not same_parameters(a, w['net'])
    # a second step each: the optimizer state moved alike
    assert a.learn_observed(obs, idx, opt_a)[0] == _host_step(b, opt_b, kind, obs, gnet, idx) and same_parameters(a, b)


def test_learn_steps_repeat_under_dropout_and_cut_into_batches(dev):
    import ops
    w = world(dev)
    obs = w['obs']
    idx = np.nonzero(obs.allq[:, 3] >= NUM_T - 3)[0]
    runs = []
    for _ in range(2):
        net, _ = models(dev, dropout=0.5)
        torch.manual_seed(7)
        ops.reset_seed_counter(0)
        losses = net.learn_observed(obs, idx, _optimizer('hip', net), steps=1, batch_size=50)
        assert len(losses) == math.ceil(len(idx) / 50.0) and len(idx) > 100
        runs.append((losses, net))
    assert runs[0][0] == runs[1][0] and same_parameters(runs[0][1], runs[1][1])
    # steps passes over the batches, in order
    net, _ = models(dev)
    assert len(net.learn_observed(obs, idx, _optimizer('torch', net), steps=2, batch_size=64)) == 2 * math.ceil(len(idx) / 64.0)
    with pytest.raises(ValueError):
        net.learn_observed(obs, idx, _optimizer('torch', net), batch_size=4096)
    with pytest.raises(ValueError):
        net.learn_observed(obs, [len(obs)], _optimizer('torch', net))


def test_five_steps_lower_the_observed_loss_of_the_batch(dev):
    w = world(dev)
    obs = w['obs']
    idx = np.nonzero(obs.allq[:, 3] == NUM_T - 1)[0]
    net = clone_of(w['net'], dev)
    before = float(net.evaluate_observed(obs, idx)[1].sum())
    losses = net.learn_observed(obs, idx, _optimizer('hip', net, lr=1e-3), steps=5)
    after = float(net.evaluate_observed(obs, idx)[1].sum())
    print('  observed loss of the batch: %.4f -> %.4f (step losses %s)' % (before, after, ['%.4f' % x for x in losses]))
    assert len(losses) == 5 and after < before


# ---- RENet_global.learn_observed -------------------------------------------------------------------------------------
class _Capture(torch.optim.SGD):
    """lr 0: step() only keeps a copy of every gradient (learn_observed clears them afterwards)."""

    def step(self):
        self.seen = [None if p.grad is None else p.grad.detach().clone() for g in self.param_groups for p in g['params']]


@pytest.mark.parametrize('subject', [None, True, False])
def test_the_global_step_equals_the_dense_float64_path_on_the_clean_targets(dev, subject):
    import online
    w = world(dev)
    obs = w['obs']
    times = np.asarray([5, 0, 13, 2, 9, 1, 12, 7], dtype=np.int64)
    a, b = clone_of(w['gnet'], dev).train(), clone_of(w['gnet'], dev).train()
    cap = _Capture(list(a.parameters()), lr=0.0)
    got = a.learn_observed(obs, times, cap, subject=subject, grad_norm=1e30)
    csr = online.stream_targets(obs.graph_dict, times, NUM_ENT)
    dense_s, dense_o = online.dense_targets(csr['s'], NUM_ENT), online.dense_targets(csr['o'], NUM_ENT)
    heads = (True, False) if subject is None else (subject,)
    want = sum(b(times, dense_s, dense_o, obs.graph_dict, subject=h) for h in heads)
    want.backward()
    want = float(want.detach())
    print('  global step (subject=%s): loss %.6f, dense float64 path %.6f' % (subject, got, want))
    assert abs(got - want) <= 1e-5 * abs(want)
    unused = 0
    for (name, p), g in zip(b.named_parameters(), cap.seen):
        if p.grad is None:                                             # (the other head, with one head only)
            assert g is None or not g.any()
            unused += 1
            continue
        err = float((g - p.grad).norm() / p.grad.norm())
        print('    relative L2 of d %s: %.2e' % (name, err))
        assert err <= 4e-5, name
    assert unused == (0 if subject is None else 2)
    assert all(p.grad is None or not p.grad.any() for p in a.parameters())


def test_refresh_global_follows_a_step_of_the_global_model(dev):
    w = world(dev)
    obs = w['obs']
    gnet = clone_of(w['gnet'], dev).train()
    opt = torch.optim.Adam(gnet.parameters(), lr=1e-2)
    loss = gnet.learn_observed(obs, obs.times[1:], opt)
    assert math.isfinite(loss) and loss > 0
    gnet.eval()
    new = obs.refresh_global(gnet)
    assert new.device.glob.shape == obs.device.glob.shape and not torch.equal(new.device.glob, obs.device.glob)
    table = obs.global_table(gnet)                                     # the per-timestamp path on the UPDATED weights
    want = torch.stack([table[int(t)].reshape(-1) for t in new.device._glob_times])
    assert float((new.device.glob - want).abs().max()) <= 1e-4 * float(want.abs().max())
    # HipAdam drives the same entry
    import parallel
    g2 = clone_of(w['gnet'], dev).train()
    l2 = g2.learn_observed(obs, obs.times[1:], parallel.HipAdam(g2, lr=1e-2, max_norm=1.0))
    assert abs(l2 - loss) <= 1e-5 * abs(loss) and not same_parameters(g2, w['gnet'])


# ---- evaluate_online -------------------------------------------------------------------------------------------------
def _online_world(dev):
    w = world(dev)
    facts = w['facts']
    n = int(np.searchsorted(facts[:, 3], T_RESIDENT))
    return w, facts[:n], facts[n:]


def test_online_without_learning_is_the_forecast_observe_loop(dev):
    w, head, quads = _online_world(dev)
    net, gnet = w['net'], w['gnet']
    obs = stream_of(head)
    obs.resident(net, gnet)
    want = net.evaluate_rollout(obs, quads, 1, gnet)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    got = net.evaluate_online(obs, quads, gnet, None, steps=0)
    for name in SETTINGS:
        assert got[0][name].dtype == want[0][name].dtype and np.array_equal(got[0][name], want[0][name]), name
    assert np.array_equal(got[1], want[1])
    assert [e['t'] for e in got[2]] == list(range(T_RESIDENT, NUM_T)) and all(e['losses'] == [] for e in got[2])
    assert len(net.last_online) == len(obs) + len(quads) and len(obs) == len(head)
    assert all(torch.equal(v, net.state_dict()[k]) for k, v in before.items()) and not net.training


@pytest.mark.parametrize('with_global', [False, True])
def test_online_learning_runs_and_moves_the_weights(dev, with_global):
    w, head, quads = _online_world(dev)
    net, gnet = clone_of(w['net'], dev).eval(), clone_of(w['gnet'], dev).eval()
    obs = stream_of(head)
    obs.resident(net, gnet)
    glob0 = obs.device.glob.clone()
    gopt = torch.optim.Adam(gnet.parameters(), lr=1e-3) if with_global else None
    ranks, loss, log = net.evaluate_online(obs, quads, gnet, _optimizer('hip', net), steps=1, replay=1, global_optimizer=gopt)
    assert all(ranks[name].shape == (len(quads), 2) for name in SETTINGS) and loss.shape == (len(quads),)
    assert np.isfinite(loss).all() and all(ranks[name].min() >= 1 for name in SETTINGS)
    end = net.last_online
    assert len(end) == len(obs) + len(quads) and end.device.n_quads == len(end)
    assert [len(e['losses']) for e in log] == [1] * (NUM_T - T_RESIDENT) and all(math.isfinite(x) for e in log for x in e['losses'])
    assert not same_parameters(net, w['net']) and not net.training
    # the first timestamp is ranked before anything was learnt: the loop's numbers
    first = quads[:, 3] == T_RESIDENT
    want = w['net'].evaluate_forecast(obs, quads[first], all_triplets=np.concatenate((head, quads)))
    assert all(np.array_equal(ranks[name][first], want[0][name]) for name in SETTINGS)
    if with_global:
        assert all(math.isfinite(e['global_loss']) for e in log) and not same_parameters(gnet, w['gnet'])
        assert not torch.equal(end.device.glob[:len(glob0)], glob0)
    else:
        assert all(e['global_loss'] is None for e in log) and same_parameters(gnet, w['gnet'])
        assert torch.equal(end.device.glob[:len(glob0) - 1], glob0[:-1])
    assert torch.equal(obs.device.glob, glob0)                          # the stream handed in stays as it was
