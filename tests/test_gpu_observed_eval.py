"""GPU tests of the observed-history (single-step, ground-truth history) evaluation pass (run with -m gpu on an MI355X):
RENet.observed_scores / evaluate_observed / predict_topk_observed over a preprocess.ObservedStream, on the small stream of
tests/observed_stream.py.  What pins the MEANING are the first two tests: the scores against the oracle's restatement of the
reference forward (model.py:64-104) on the true histories of the whole stream, and the ranks of all three settings against
the intervals those oracle scores allow.  The rest is consistency: the torch rank formulation on the same scores (exact),
RENet.forward's loss, batch cuts, the all-empty first timestamp, the untouched multi-step state, top-k."""
import copy

import numpy as np
import pytest
import torch

from helpers import O, fixtures, global_shapes, renet_shapes
from test_gpu_parity import ATOL, RTOL            # the tolerance of logits against the reference golden, same GEMM mode

import observed_stream as S

pytestmark = pytest.mark.gpu

SETTINGS = ('raw', 'filtered', 'time_filtered')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _models(dev, d, num_k=10):
    import global_model as GM
    import model as M
    params = fixtures.make_params(41, renet_shapes(S.NUM_ENT, S.NUM_RELS, d))
    net = M.RENet(S.NUM_ENT, d, S.NUM_RELS, dropout=0.0, seq_len=S.SEQ_LEN, num_k=num_k)
    gnet = GM.RENet_global(S.NUM_ENT, d, S.NUM_RELS, dropout=0.0, seq_len=S.SEQ_LEN, num_k=num_k, maxpool=1)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    gnet.load_state_dict({k: torch.from_numpy(v) for k, v in
                          fixtures.make_params(42, global_shapes(S.NUM_ENT, S.NUM_RELS, d)).items()})
    return net.to(dev).eval(), gnet.to(dev).eval(), params


def _filter_sets(allq, quads):
    """Per quadruple, by brute force over the fact array: {'ob': [(agnostic, aware)], 'sub': [...]} -- the entities that
    complete (s, r, ?) / (?, r, o) at any time and at the query's own."""
    out = {'ob': [], 'sub': []}
    for s, r, o, t in quads.tolist():
        for name, key, kc, vc in (('ob', s, 0, 2), ('sub', o, 2, 0)):
            m = (allq[:, kc] == key) & (allq[:, 1] == r)
            out[name].append((set(allq[m, vc].tolist()), set(allq[m & (allq[:, 3] == t), vc].tolist())))
    return out


_WORLDS = {}


def _world(dev, d):
    """Model, resident stream and the ORACLE's scores of the valid + test positions (computed once per hidden size, shared
    and left unchanged)."""
    if d in _WORLDS:
        return _WORLDS[d]
    import preprocess as P
    splits = S.make()
    cases = S.check_cases(*splits)
    obs = P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    net, gnet, params = _models(dev, d)
    store = obs.resident(net, gnet)
    allq = obs.allq
    idx = np.concatenate((obs.positions('valid'), obs.positions('test')))
    assert all(i in idx for i in cases.values())
    # the oracle: per direction, on the same histories, graphs and global table, un-permuted with its bg.perm
    op = {k: torch.from_numpy(v) for k, v in params.items()}
    ge = {int(t): store.glob[k].cpu() for k, t in enumerate(obs.times)}
    ogd = O.build_graph_dict(allq, S.NUM_RELS)
    sh, oh, _ = O.build_histories(allq, S.NUM_ENT, history_len=S.SEQ_LEN)
    ref, ref_r = {}, {}
    with torch.no_grad():
        for name, subject, h in (('ob', True, sh), ('sub', False, oh)):
            _, parts = O.renet_forward_loss(op, allq[idx], [h[0][i] for i in idx], [h[1][i] for i in idx], ogd, ge, S.NUM_RELS,
                                            S.SEQ_LEN, subject=subject, return_parts=True)
            full = np.empty((len(idx), S.NUM_ENT), dtype=np.float64)
            full[parts['bg'].perm] = parts['ob_pred'].double().numpy()
            ref[name] = full
            full_r = np.empty((len(idx), S.NUM_RELS), dtype=np.float64)
            full_r[parts['bg'].perm] = parts['ob_pred_r'].double().numpy()
            ref_r[name] = full_r
    w = dict(obs=obs, net=net, gnet=gnet, params=params, store=store, idx=idx, quads=allq[idx], ref=ref, ref_r=ref_r, cases=cases,
             sets=_filter_sets(allq, allq[idx]))
    w['intervals'] = _intervals(w)
    _WORLDS[d] = w
    return w


def _intervals(w):
    """{setting: (lo [n, 2], hi [n, 2])} from the ORACLE's scores: with tol the logits tolerance, lo counts only the columns
    above gold + tol, hi all columns at or above gold - tol; under the filtered settings the same on sigmoid values with
    the other known completions at 0 and tol carried through the sigmoid's largest slope (1/4)."""
    n = len(w['idx'])
    out = {name: (np.zeros((n, 2)), np.zeros((n, 2))) for name in SETTINGS}
    for col, side, gold_col in ((0, 'sub', 0), (1, 'ob', 2)):
        for i in range(n):
            row, gold = w['ref'][side][i], int(w['quads'][i, gold_col])
            tol = ATOL + RTOL * float(np.abs(row).max())
            sig = 1.0 / (1.0 + np.exp(-row))
            agnostic, aware = w['sets'][side][i]
            for name, vals, t in (('raw', row, tol), ('filtered', sig.copy(), tol / 4), ('time_filtered', sig.copy(), tol / 4)):
                if name != 'raw':
                    known = np.asarray(sorted((agnostic if name == 'filtered' else aware) - {gold}), dtype=np.int64)
                    vals[known] = 0.0
                others = np.delete(vals, gold)
                out[name][0][i, col] = 1 + np.count_nonzero(others > vals[gold] + t)
                out[name][1][i, col] = 1 + np.count_nonzero(others >= vals[gold] - t)
    return out


def _torch_ranks(w, sub_pred, ob_pred, quads, sets):
    """model._rank_rows (the torch formulation) on score matrices, all three settings -> {setting: [n, 2]}."""
    import model as M
    dev = ob_pred.device
    out = {}
    for name in SETTINGS:
        cols = []
        for side, pred, gold_col in (('sub', sub_pred, 0), ('ob', ob_pred, 2)):
            lab = torch.from_numpy(quads[:, gold_col].copy()).to(dev)
            if name == 'raw':
                cols.append(M._rank_rows(pred, lab))
                continue
            lists = [sorted(a if name == 'filtered' else b) for a, b in sets[side]]
            rows = torch.from_numpy(np.repeat(np.arange(len(lists)), [len(x) for x in lists])).to(dev)
            fc = torch.from_numpy(np.asarray([c for x in lists for c in x], dtype=np.int64)).to(dev)
            cols.append(M._rank_rows(pred, lab, rows, fc))
        out[name] = np.stack(cols, axis=1)
    return out


# ---- 1. scores against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [100, 300])
def test_scores_equal_the_oracle_forward_on_true_histories(dev, d):
    w = _world(dev, d)
    sub_pred, ob_pred = w['net'].observed_scores(w['obs'], w['idx'])
    assert sub_pred.shape == ob_pred.shape == (len(w['idx']), S.NUM_ENT)
    for name, got in (('ob', ob_pred), ('sub', sub_pred)):
        got = got.cpu().numpy()
        print('d', d, name, 'max |score - oracle|', float(np.abs(got - w['ref'][name]).max()), 'score scale',
              float(np.abs(w['ref'][name]).max()))
        np.testing.assert_allclose(got, w['ref'][name], rtol=RTOL, atol=ATOL)
    # the resident store is also accepted in place of the stream
    again = w['net'].observed_scores(w['store'], w['idx'])
    assert torch.equal(again[0], sub_pred) and torch.equal(again[1], ob_pred)


# ---- 2. ranks, all three settings ------------------------------------------------------------------------------------
def test_ranks_lie_in_the_intervals_the_oracle_scores_allow(dev):
    w = _world(dev, 100)
    ranks, loss = w['net'].evaluate_observed(w['obs'], w['idx'])
    assert sorted(ranks) == sorted(SETTINGS) and loss.shape == (len(w['idx']),)
    for name in SETTINGS:
        lo, hi = w['intervals'][name]
        got = ranks[name]
        assert got.shape == (len(w['idx']), 2) and got.dtype == np.float64
        sharp = float(np.mean(lo == hi))
        print(name, 'rows with lo == hi under the oracle alone', sharp, 'ranks outside', int(((got < lo) | (got > hi)).sum()))
        assert sharp >= 0.9                                    # otherwise the intervals prove nothing
        assert np.all((got >= lo) & (got <= hi)), np.nonzero((got < lo) | (got > hi))
    assert np.all(ranks['filtered'] <= ranks['time_filtered'])
    # the planted cases separate the settings: (c) other objects at the query's own time, (d) a completion known elsewhere only
    k = {name: int(np.nonzero(w['idx'] == w['cases'][name])[0][0]) for name in 'cd'}
    agnostic, aware = w['sets']['ob'][k['d']]
    assert agnostic - aware and len(w['sets']['ob'][k['c']][1]) >= 3


# ---- 3. exact self-consistency ---------------------------------------------------------------------------------------
def test_ranks_equal_the_torch_formulation_on_the_returned_scores(dev):
    w = _world(dev, 100)
    ranks, _ = w['net'].evaluate_observed(w['obs'], w['idx'], max_batch=4096)
    sub_pred, ob_pred = w['net'].observed_scores(w['obs'], w['idx'])
    want = _torch_ranks(w, sub_pred, ob_pred, w['quads'], w['sets'])
    for name in SETTINGS:
        print(name, 'rows differing from the torch formulation', int((ranks[name] != want[name]).sum()))
        assert np.array_equal(ranks[name], want[name])
    # all_triplets given explicitly (the stream itself, as a tensor) is the default
    ranks2, _ = w['net'].evaluate_observed(w['obs'], w['idx'], all_triplets=torch.from_numpy(w['obs'].allq))
    assert all(np.array_equal(ranks2[name], ranks[name]) for name in SETTINGS)


# ---- 4. loss against RENet.forward -----------------------------------------------------------------------------------
def test_losses_equal_forward_in_eval_mode_on_a_second_model(dev):
    import model as M
    w = _world(dev, 100)
    obs, idx = w['obs'], w['idx']
    net2 = M.RENet(S.NUM_ENT, 100, S.NUM_RELS, dropout=0.0, seq_len=S.SEQ_LEN)
    net2.load_state_dict({k: torch.from_numpy(v) for k, v in w['params'].items()})
    net2.to(dev).eval()
    net2.global_emb = {int(t): w['store'].glob[k].view(1, 1, -1) for k, t in enumerate(obs.times)}
    ranks, loss, rel = w['net'].evaluate_observed(obs, idx, relation=True)
    assert rel['rank'].shape == rel['loss'].shape == rel['entity_loss'].shape == (len(idx), 2)
    np.testing.assert_allclose(rel['entity_loss'].sum(axis=1), loss, rtol=1e-6, atol=1e-6)
    assert rel['rank'].min() >= 1 and rel['rank'].max() <= S.NUM_RELS
    fs, fo = obs.hist_s.take(idx, max_len=S.SEQ_LEN), obs.hist_o.take(idx, max_len=S.SEQ_LEN)
    batch = torch.from_numpy(w['quads']).to(dev)
    with torch.no_grad():
        for col, subject in ((1, True), (0, False)):
            want = float(net2(batch, fs, fo, obs.graph_dict, subject=subject))
            got = float(rel['entity_loss'][:, col].astype(np.float64).mean() + 0.1 * rel['loss'][:, col].astype(np.float64).mean())
            print('subject', subject, 'forward', want, 'observed pass', got)
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    # the relation ranks against the oracle's linear_r logits (model.py:98-100), by the interval rule of the entity ranks
    for col, side in ((0, 'sub'), (1, 'ob')):
        for i in range(len(idx)):
            row, gold = w['ref_r'][side][i], int(w['quads'][i, 1])
            tol = ATOL + RTOL * float(np.abs(row).max())
            others = np.delete(row, gold)
            lo, hi = 1 + np.count_nonzero(others > row[gold] + tol), 1 + np.count_nonzero(others >= row[gold] - tol)
            assert lo <= rel['rank'][i, col] <= hi, (side, i, lo, hi, rel['rank'][i, col])


# ---- 5. batch cuts do not matter -------------------------------------------------------------------------------------
def test_batches_cut_inside_timestamps_agree_with_one_batch(dev):
    """max_batch = 7 (cuts inside timestamps, batches spanning two) against max_batch = 4096 (one batch): the ranks of both by
    the interval rule of test 2, the losses to 1e-5.  The cut is the scoring's: the encoder's batch graphs are chunks of idx
    of a fixed size, whatever max_batch is.  (The reference forward merges the histories of a batch GRAPH into one
    node-induced graph per timestamp, utils.py:149-170, so logits depend on what shares a graph: were the graphs cut with
    max_batch, the oracle alone would move scores by 0.045 and 52 of these 326 raw ranks between the two cuts.)"""
    w = _world(dev, 100)
    one, loss_one = w['net'].evaluate_observed(w['obs'], w['idx'], max_batch=4096)
    cut, loss_cut = w['net'].evaluate_observed(w['obs'], w['idx'], max_batch=7)
    t = w['quads'][:, 3]
    assert any(t[c] == t[c - 1] for c in range(7, len(t), 7)) and any(t[c] != t[min(c + 6, len(t) - 1)] for c in range(0, len(t), 7))
    for name in SETTINGS:
        lo, hi = w['intervals'][name]
        print(name, 'ranks differing between max_batch 7 and 4096', int((one[name] != cut[name]).sum()), 'of', one[name].size,
              '; outside the oracle intervals: one batch', int(((one[name] < lo) | (one[name] > hi)).sum()),
              'batches of 7', int(((cut[name] < lo) | (cut[name] > hi)).sum()))
    print('largest loss difference between the cuts', float(np.abs(loss_cut - loss_one).max()))
    for name in SETTINGS:
        lo, hi = w['intervals'][name]
        assert np.all((one[name] >= lo) & (one[name] <= hi)), name
        assert np.all((cut[name] >= lo) & (cut[name] <= hi)), name
    np.testing.assert_allclose(loss_cut, loss_one, rtol=1e-5, atol=1e-5)


def test_more_positions_than_one_batch_graph_holds(dev):
    """2048 + 163 positions (stream positions repeated): two encoder chunks.  The first chunk's rows are those of its
    positions alone (a chunk is a function of idx, not of the scoring cut), one scoring batch gives the torch ranks of
    observed_scores exactly, and scoring cuts that straddle the chunk border change the losses by rounding only."""
    import gpu_builder
    w = _world(dev, 100)
    net, obs = w['net'], w['obs']
    step = gpu_builder.MAX_BOTH
    idx = np.concatenate((np.resize(np.arange(len(obs)), step), w['idx']))
    assert len(idx) == step + len(w['idx'])
    sub_pred, ob_pred = net.observed_scores(obs, idx)
    head = net.observed_scores(obs, idx[:step])
    tail = net.observed_scores(obs, idx[step:])
    assert torch.equal(sub_pred[:step], head[0]) and torch.equal(ob_pred[:step], head[1])
    assert torch.equal(sub_pred[step:], tail[0]) and torch.equal(ob_pred[step:], tail[1])
    one, loss_one = net.evaluate_observed(obs, idx, max_batch=4096)
    want = _torch_ranks(w, sub_pred, ob_pred, obs.allq[idx], _filter_sets(obs.allq, obs.allq[idx]))
    assert all(np.array_equal(one[name], want[name]) for name in SETTINGS)
    cut, loss_cut = net.evaluate_observed(obs, idx, max_batch=1000)
    print('ranks differing between max_batch 1000 and 4096', {name: int((one[name] != cut[name]).sum()) for name in SETTINGS})
    np.testing.assert_allclose(loss_cut, loss_one, rtol=1e-5, atol=1e-5)


# ---- 6. the first timestamp alone ------------------------------------------------------------------------------------
def test_first_timestamp_takes_the_zero_state_scores(dev):
    w = _world(dev, 100)
    net, obs = w['net'], w['obs']
    idx = np.nonzero(obs.allq[:, 3] == obs.times[0])[0]
    assert len(idx) >= 15 and obs.hist_s.count[idx].max() == 0 and obs.hist_o.count[idx].max() == 0
    sub_pred, ob_pred = net.observed_scores(obs, idx)
    q = torch.from_numpy(obs.allq[idx]).to(dev)
    with torch.no_grad():
        ent, rel, zero = net.ent_embeds.double(), net.rel_embeds.double(), torch.zeros(len(idx), 100, device=dev).double()
        lin = lambda f: f @ net.linear.weight.double().t() + net.linear.bias.double()
        want_ob = lin(torch.cat((ent[q[:, 0]], zero, rel[q[:, 1]]), dim=1))
        want_sub = lin(torch.cat((ent[q[:, 2]], zero, rel[S.NUM_RELS + q[:, 1]]), dim=1))
    np.testing.assert_allclose(ob_pred.cpu().numpy(), want_ob.cpu().numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(sub_pred.cpu().numpy(), want_sub.cpu().numpy(), rtol=RTOL, atol=ATOL)
    ranks, loss = net.evaluate_observed(obs, idx)
    want = _torch_ranks(w, sub_pred, ob_pred, obs.allq[idx], _filter_sets(obs.allq, obs.allq[idx]))
    assert all(np.array_equal(ranks[name], want[name]) for name in SETTINGS) and np.all(np.isfinite(loss))


# ---- 7. state untouched ----------------------------------------------------------------------------------------------
def _multi_step_setup(dev, obs):
    """A model in the state test.py has before its evaluation loop over the valid split (multi-step protocol)."""
    import utils as U
    net, gnet, _ = _models(dev, 100)
    tr, va, te = (obs.allq[obs.positions(k)] for k in ('train', 'valid', 'test'))
    H = {k: (obs.hist_s.to_lists(obs.positions(k)), obs.hist_o.to_lists(obs.positions(k))) for k in ('train', 'valid', 'test')}
    gd = U.build_graph_dict(tr, S.NUM_RELS)
    valid = torch.from_numpy(va)
    with torch.no_grad():
        net.global_emb = gnet.get_global_emb(np.unique(tr[:, 3]), gd)
        net.graph_dict = gd
        net.init_history(tr, H['train'][0], H['train'][1], valid, H['valid'][0], H['valid'][1], te, H['test'][0], H['test'][1])
        net.latest_time = valid[0][3]
    return net, gnet, H, valid


STATE = ('s_hist_test', 'o_hist_test', 's_hist_test_t', 'o_hist_test_t', 's_his_cache', 'o_his_cache', 's_his_cache_t',
         'o_his_cache_t', 'graph_dict', 'global_emb', 'preds_list_s', 'preds_ind_s', 'preds_list_o', 'preds_ind_o', 'data')


def _same_content(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    if isinstance(a, dict):
        return list(a.keys()) == list(b.keys()) and all(_same_content(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_content(x, y) for x, y in zip(a, b))
    if hasattr(a, '__slots__') and not isinstance(a, (int, float)):                  # graph.TimeGraph
        return all(_same_content(getattr(a, f), getattr(b, f)) for f in ('ent', 'ls', 'r', 'lo'))
    return a == b


def test_pass_leaves_the_multi_step_state_untouched_and_is_repeatable(dev):
    w = _world(dev, 100)
    obs = w['obs']
    net, gnet, H, valid = _multi_step_setup(dev, obs)
    (vs, vst), (vo, vot) = H['valid']
    held = {k: getattr(net, k) for k in STATE}
    graphs = dict(net.graph_dict)
    snap = copy.deepcopy({k: (dict(v) if k.startswith('preds_') else v) for k, v in held.items() if k != 'graph_dict'})
    latest, last_batch = copy.deepcopy(net.latest_time), net.aggregator.last_batch
    glob_key = net.aggregator.glob_table._key
    # the observed pass, every entry point, on a store of its own for this model; twice: repeatable in place
    store = obs.resident(net, gnet)
    idx = obs.positions('valid')
    first = net.evaluate_observed(store, idx, max_batch=50, relation=True)
    second = net.evaluate_observed(store, idx, max_batch=50, relation=True)
    for name in SETTINGS:
        assert np.array_equal(first[0][name], second[0][name])
    assert np.array_equal(first[1], second[1]) and np.array_equal(first[2]['rank'], second[2]['rank'])
    net.predict_topk_observed(store, idx[:9], k=3, setting='time_filtered')
    net.observed_scores(store, idx[:9])
    obs.device = w['store']                                     # (the shared world's store stays the stream's)
    for k in STATE:
        assert getattr(net, k) is held[k], k
        if k != 'graph_dict':
            now = getattr(net, k)
            assert _same_content(dict(now) if k.startswith('preds_') else now, snap[k]), k
    assert list(net.graph_dict.keys()) == list(graphs.keys()) and all(net.graph_dict[t] is graphs[t] for t in graphs)
    assert _same_content(net.latest_time, latest) and net.aggregator.last_batch is last_batch
    assert net.aggregator.glob_table._key == glob_key
    # ... and the multi-step pass that follows gives what it gives without the observed pass before it
    n = len(valid)
    torch.manual_seed(1234)
    after = net.evaluate_all_stream(valid, (vs, vst), (vo, vot), gnet, torch.from_numpy(obs.allq).to(dev))
    net_b, gnet_b, H_b, valid_b = _multi_step_setup(dev, obs)
    torch.manual_seed(1234)
    plain = net_b.evaluate_all_stream(valid_b, (vs, vst), (vo, vot), gnet_b, torch.from_numpy(obs.allq).to(dev))
    for name in SETTINGS:
        assert after[0][name].shape == (n, 2) and np.array_equal(after[0][name], plain[0][name]), name
    assert np.array_equal(after[1], plain[1])
    # the two protocols answer different questions: from the second valid timestamp on the histories differ
    assert any(not np.array_equal(first[0][name], after[0][name]) for name in SETTINGS)


# ---- 8. top-k ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 10, S.NUM_ENT + 5])
def test_topk_equals_numpy_sorting_of_the_observed_scores(dev, k):
    w = _world(dev, 100)
    net, obs, idx, quads = w['net'], w['obs'], w['idx'], w['quads']
    sub_pred, ob_pred = (x.cpu().numpy() for x in net.observed_scores(obs, idx))
    lse = {name: torch.logsumexp(torch.from_numpy(p).double(), dim=1).numpy() for name, p in (('sub', sub_pred), ('ob', ob_pred))}
    for setting in SETTINGS:
        for keep_gold in (False, True):
            got = net.predict_topk_observed(obs, idx, k=k, setting=setting, keep_gold=keep_gold)
            for name, pred, gold_col in (('sub', sub_pred, 0), ('ob', ob_pred, 2)):
                gi, gv, gl, gn = (x.cpu().numpy() for x in got[name])
                assert gi.shape == gv.shape == gl.shape == (len(idx), k) and gn.shape == (len(idx),)
                for i in range(len(idx)):
                    agnostic, aware = w['sets'][name][i]
                    out = set() if setting == 'raw' else set(agnostic if setting == 'filtered' else aware)
                    if keep_gold:
                        out.discard(int(quads[i, gold_col]))
                    cand = np.asarray([c for c in range(S.NUM_ENT) if c not in out], dtype=np.int64)
                    order = cand[np.lexsort((cand, -pred[i, cand]))][:k]
                    m = len(order)
                    assert gn[i] == m and gi[i, :m].tolist() == order.tolist() and np.all(gi[i, m:] == -1), (setting, name, i)
                    assert np.array_equal(gv[i, :m], pred[i, order]) and np.all(np.isneginf(gv[i, m:]))
                    np.testing.assert_allclose(gl[i, :m], pred[i, order] - lse[name][i], rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        net.predict_topk_observed(obs, idx, k=k, setting='best')

