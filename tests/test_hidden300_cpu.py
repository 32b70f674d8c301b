"""CPU: n_hidden = 300 (3x3 relation blocks).  The committed oracle against the three fixtures that
tools/make_golden_d300.py produced by running the unmodified reference, and the reference's state_dict layout at this width
(tests/test_oracle_golden.py does the same at 100 / 200 / 400)."""
import numpy as np
import torch

from helpers import O, fixtures, load_golden, train_case, renet_shapes, global_shapes

RTOL, ATOL = 2e-4, 2e-5      # tests/test_oracle_golden.py
D = 300


def test_rgcn_layer_matches_reference_300():
    gold = load_golden('rgcn_300.npz')
    n, num_rels = int(gold['n']), int(gold['num_rels'])
    p = fixtures.make_params(200 + D, {'weight': (2 * num_rels, D * D // 100), 'loop_weight': (D, D),
                                       'h': (n, D), 'gout': (n, D)}, scale=0.5)
    assert p['weight'].shape == (2 * num_rels, 900)
    for relu in (0, 1):
        for reverse in (0, 1):
            h = torch.from_numpy(p['h']).clone().requires_grad_(True)
            w = torch.from_numpy(p['weight']).clone().requires_grad_(True)
            lw = torch.from_numpy(p['loop_weight']).clone().requires_grad_(True)
            et = gold['type_o'] if reverse else gold['type_s']
            y = O.rgcn_layer(h, gold['src'], gold['dst'], et, gold['norm'], w, lw, relu=bool(relu))
            (y * torch.from_numpy(p['gout'])).sum().backward()
            tag = 'relu%d_rev%d_' % (relu, reverse)
            np.testing.assert_allclose(y.detach().numpy(), gold[tag + 'out'], rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(h.grad.numpy(), gold[tag + 'dh'], rtol=RTOL, atol=ATOL)
            for key, g in (('dweight', w.grad), ('dloop', lw.grad)):
                ok, err, how = fixtures.check_packed(gold, tag + key, g.numpy(), RTOL, ATOL * 10)
                assert ok, (tag + key, err, how)


def test_training_forward_backward_matches_reference_300():
    c = train_case('tiny', D)
    gold, cfg = c['gold'], c['cfg']
    assert int(gold['seq_len']) == 4 and len(c['batch']) == 40
    params = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in c['params'].items()}
    gd = O.build_graph_dict(c['train'], cfg['num_rels'])
    ge = {t: torch.from_numpy(v) for t, v in c['global_emb'].items()}
    total = 0
    for tag, subject in (('s', True), ('o', False)):
        hist, hist_t = c['hists'][tag]
        loss, parts = O.renet_forward_loss(params, c['batch'], hist, hist_t, gd, ge, cfg['num_rels'],
                                           c['seq_len'], subject=subject, return_parts=True)
        assert abs(loss.item() - float(gold['loss_' + tag])) < 1e-4 * max(1.0, abs(float(gold['loss_' + tag])))
        bg = parts['bg']
        b = len(c['batch'])
        assert bg.num_nodes == int(gold[tag + '_graph_nodes'])
        for key, val in (('h_n', parts['s_h']), ('q_n', parts['s_q'])):
            full = np.zeros((b, D), np.float32)
            full[bg.perm] = val.detach().numpy()
            np.testing.assert_allclose(full, gold['%s_%s' % (tag, key)], rtol=RTOL, atol=ATOL)
        logits = np.zeros((b, cfg['num_ent']), np.float32)
        logits[bg.perm] = parts['ob_pred'].detach().numpy()
        np.testing.assert_allclose(logits, gold[tag + '_logits'], rtol=RTOL, atol=ATOL * 5)
        total = total + loss
    total.backward()
    for k, p in params.items():
        g = p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
        ok, err, how = fixtures.check_packed(gold, 'grad.' + k, g, 1e-3, 2e-5)
        assert ok, (k, err, how)


def test_global_model_matches_reference_300():
    gold = load_golden('global_tiny_300_max1.npz')
    cfg, tr, va, te = fixtures.split_dataset('tiny')
    seq_len, maxpool = int(gold['seq_len']), int(gold['maxpool'])
    assert maxpool == 1
    p = fixtures.make_params(int(gold['param_seed']), global_shapes(cfg['num_ent'], cfg['num_rels'], D))
    params = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in p.items()}
    gd = O.build_graph_dict(tr, cfg['num_rels'])
    times = np.unique(tr[:, 3])
    loss = O.global_forward_loss(params, times, gold['true_o'], gd, seq_len, subject=True, maxpool=maxpool)
    assert abs(loss.item() - float(gold['loss'])) < 1e-4 * max(1.0, abs(float(gold['loss'])))
    loss.backward()
    for k, prm in params.items():
        if ('grad.' + k) in gold or ('grad.' + k + '__samp') in gold:
            ok, err, how = fixtures.check_packed(gold, 'grad.' + k, prm.grad.numpy(), 1e-3, 2e-5)
            assert ok, (k, err, how)
    with torch.no_grad():
        for k, t in enumerate(gold['predict_t']):
            for subj in (True, False):
                emb, logits = O.global_predict(params, int(t), gd, seq_len, subject=subj, maxpool=maxpool)
                tag = 'predict%d_%s_' % (k, 's' if subj else 'o')
                np.testing.assert_allclose(emb.numpy(), gold[tag + 'emb'], rtol=RTOL, atol=ATOL)
                np.testing.assert_allclose(logits.numpy(), gold[tag + 'logits'], rtol=RTOL, atol=ATOL)


def test_state_dict_layout_at_300():
    """The reference's parameter names and shapes at n_hidden = 300: the fixture's gradient keys are exactly the names of
    renet_shapes, with the widths the 3x3 blocks imply."""
    cfg, _, _, _ = fixtures.split_dataset('tiny')
    ne, nr = cfg['num_ent'], cfg['num_rels']
    shapes = renet_shapes(ne, nr, D)
    assert shapes['aggregator.rgcn1.weight'] == (2 * nr, 900) and shapes['aggregator.rgcn2.weight'] == (2 * nr, 900)
    assert shapes['aggregator.rgcn1.loop_weight'] == (300, 300)
    assert shapes['encoder.weight_ih_l0'] == (900, 1200) and shapes['encoder_r.weight_ih_l0'] == (900, 900)
    assert shapes['encoder.weight_hh_l0'] == (900, 300) and shapes['linear.weight'] == (ne, 900)
    gold = load_golden('train_tiny_300.npz')
    keys = set(k[5:].replace('__norm', '').replace('__samp', '') for k in gold.files if k.startswith('grad.'))
    assert keys == set(shapes)
    for k, shp in shapes.items():
        if ('grad.' + k) in gold.files:
            assert tuple(gold['grad.' + k].shape) == shp, k
        else:
            assert len(gold['grad.' + k + '__samp']) == len(fixtures.sample_idx(int(np.prod(shp)))), k
