"""Keeps the bounds of tests/gru_statement.py honest without a GPU: the float64 statement is torch.nn.GRU, and host
evaluations of the same steps in the kernels' arithmetic (plain float32, the six-pair bf16 split product, the one-plane
bf16 product) stay inside every bound.  Run with -s for the ratios.  No bound is fitted to a kernel: each is stated with
its argument in gru_statement.py, and these evaluations are what it has to hold for before a kernel is measured."""
import numpy as np
import pytest
import torch

import gru_statement as G

LENS = [7] * 9 + [6, 6, 5, 3, 3, 3, 2, 1, 1, 1]                         # 19 sequences: a partial second tile of 16


def _case(h, wscale=0.05):
    return G.case(h, LENS, wscale=wscale)


def test_statement_is_torch_gru_in_float64():
    """forward, dX and the parameter gradients of torch.nn.GRU (float64, packed batch) from the statement's dGi / dGh"""
    h, i = 24, 13
    c = _case(h)
    lens, off = c['lens'], c['off']
    torch.manual_seed(3)
    ref = torch.nn.GRU(i, h, batch_first=True).double()
    x = torch.randn(len(lens), max(lens), i, dtype=torch.float64, requires_grad=True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True)
    _, hn = ref(packed)
    dh = torch.from_numpy(c['dh']).double()
    (hn[0] * dh).sum().backward()
    w_ih, w_hh, b_ih, b_hh = (p.detach().numpy() for p in (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0))
    xp = packed.data.detach().numpy()
    gi = xp @ w_ih.T + b_ih
    h_last, saved = G.forward_f64(gi, off, w_hh, b_hh)
    np.testing.assert_allclose(h_last, hn[0].detach().numpy(), rtol=0, atol=1e-14)
    d_gi, d_gh = G.backward_f64(dh.numpy(), off, w_hh, saved)
    dx_ref = torch.nn.utils.rnn.pack_padded_sequence(x.grad, lens, batch_first=True).data.numpy()
    np.testing.assert_allclose(d_gi @ w_ih, dx_ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(d_gi.T @ xp, ref.weight_ih_l0.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(d_gi.sum(0), ref.bias_ih_l0.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(d_gh.T @ saved[:, 4 * h:], ref.weight_hh_l0.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(d_gh.sum(0), ref.bias_hh_l0.grad.numpy(), rtol=0, atol=1e-12)
    # and the float64 recurrence is inside its own bounds with room to spare (ratios of rounding-free values: ~2^-29)
    fr = G.worst(G.forward_ratios('f32', gi, off, w_hh, b_hh, saved, h_last))
    assert max(fr.values()) < 1e-3, fr


@pytest.mark.parametrize('route', G.ROUTES)
@pytest.mark.parametrize('h', [100, 200])
def test_host_evaluations_stay_inside_every_bound(route, h):
    """plain float32 ('f32'), the six-pair split product ('bf16x6': three RNE planes, pairs smallest first, fp32
    accumulation) and the one-plane product ('bf16') through every forward and backward statement"""
    c = _case(h)
    h_last, saved, d_gi, d_gh = G.run_float32(route, c['gi'], c['off'], c['w'], c['b'], c['dh'], out_rows=len(c['lens']) + 3)
    fr = G.forward_ratios(route, c['gi'], c['off'], c['w'], c['b'], saved, h_last)
    br = G.backward_ratios(route, c['dh'], c['off'], c['w'], saved, d_gi, d_gh)
    print('\nhost %-6s H=%d  fwd %s\n                   bwd %s' % (
        route, h, ' '.join('%s %.3f' % kv for kv in G.worst(fr).items()),
        ' '.join('%s %.3f' % kv for kv in G.worst(br).items())))
    G.assert_holds(fr, 'host %s forward' % route)
    G.assert_holds(br, 'host %s backward' % route)
    # the statements are not vacuous: the float64 recurrence and this evaluation agree to fp32 (bf16) class
    h64, _ = G.forward_f64(c['gi'], c['off'], c['w'], c['b'])
    tol = 2e-2 if route == 'bf16' else 2e-5
    assert np.abs(h_last[:len(c['lens'])] - h64).max() < tol


def test_statements_see_a_missing_term_pair_and_a_wrong_row():
    """what the bounds are for: a six-pair product without one of its large pairs, a hidden state handed to the wrong
    sequence and an unwritten (NaN) row all leave their bounds"""
    c = _case(100, wscale=0.3)
    args = (c['gi'], c['off'], c['w'], c['b'])
    h_last, saved, d_gi, d_gh = G.run_float32('bf16x6', *args, c['dh'])
    h = c['h']
    hp = saved[:, 4 * h:]
    # (a dense product hides a missing SMALL pair, 2^-17 of a term, inside the worst-case accumulation bound c_mm u T:
    # those are the business of the single-product census below; the dense statements see the three large pairs)
    for drop in G.PAIRS6[3:]:
        bad = saved.copy()
        bad[:, 3 * h:4 * h] = G.matmul_planes(hp, c['w'][2 * h:], drop=drop) + c['b'][2 * h:]
        assert G.worst(G.forward_ratios('bf16x6', *args, bad, h_last))['hn'] > 1.0, drop
    off = c['off']
    bad = saved.copy()
    bad[off[1]:off[1] + 2, 4 * h:] = saved[off[1]:off[1] + 2, 4 * h:][::-1]         # h of sequences 0 and 1 swapped at step 1
    assert G.worst(G.forward_ratios('bf16x6', *args, bad, h_last))['h_next'] > 1.0
    bad = d_gi.copy()
    bad[3] = np.nan
    with pytest.raises(AssertionError, match='dGi misses its bound at row 3'):
        G.assert_holds(G.backward_ratios('bf16x6', c['dh'], off, c['w'], saved, bad, d_gh), 'nan row')
    bad = d_gh.copy()
    bad[:, 2 * h:] = np.nextafter(np.nextafter(bad[:, 2 * h:], np.float32(np.inf)), np.float32(np.inf))
    assert G.worst(G.backward_ratios('bf16x6', c['dh'], off, c['w'], saved, d_gi, bad))['dGh_n_is_dGi_n_r'] > 1.0


def test_single_products_expose_every_term_pair():
    """the term-pair census of the GPU test, on the host: one product per element.  The six pairs stay inside 2^-22 of the
    float64 product; without any ONE pair at least half of the elements leave it."""
    rng = np.random.RandomState(9)
    a = (rng.rand(400000).astype(np.float32) + np.float32(0.01)) * rng.choice([-1, 1], 400000).astype(np.float32)
    b = rng.randn(400000).astype(np.float32)
    full = G.product_ratio(G.product_planes(a, b), a, b, 'bf16x6')
    print('\nsix pairs: worst error %.3f * 2^-24 of the product' % (full.max() * 4))
    assert full.max() <= 1.0
    for drop in G.PAIRS6:
        frac = float(np.mean(G.product_ratio(G.product_planes(a, b, drop=drop), a, b, 'bf16x6') > 1.0))
        print('without pair %s: %.1f%% of the elements leave the bound' % (drop, 100 * frac))
        assert frac >= 0.5, (drop, frac)
        wide = float(np.mean(G.product_ratio(G.product_planes(a, b, drop=drop), a, b, 'bf16x6', G.PRODUCT_BOUND_BWD) > 1.0))
        assert wide >= 0.5, (drop, wide)                                  # (the backward census observes at 2^-21)
    assert G.product_ratio(G.product_planes(a, b, npl=1), a, b, 'bf16').max() <= 1.0
    assert G.product_ratio(a * b, a, b, 'f32').max() <= 1.0


def test_backward_product_case_is_one_product_per_element():
    """the construction of the backward term-pair census in float64: dGi_n of step 0 IS dGh_n[k0] W_hh[2H + k0][v]"""
    c = G.backward_product_case(100)
    d_gi, d_gh = G.backward_f64(c['dh'], c['off'], c['w'], c['saved'])
    got, a, b = G.backward_product_operands(c, d_gi, d_gh)
    np.testing.assert_allclose(d_gi[:len(c['k0']), 200:], a.astype(np.float64) * b, rtol=1e-7, atol=0)   # (a rounded to fp32)
    np.testing.assert_array_equal(got, d_gi[:len(c['k0']), 200:].astype(np.float32))
    for route in G.ROUTES:                                                # and the host evaluations stay inside the bounds
        e_gi, e_gh = G.backward_float32(route, c['dh'], c['off'], c['w'], c['saved'])
        got, a, b = G.backward_product_operands(c, e_gi, e_gh)
        assert G.product_ratio(got, a, b, route, G.PRODUCT_BOUND_BWD).max() <= 1.0, route
        G.assert_holds(G.backward_ratios(route, c['dh'], c['off'], c['w'], c['saved'], e_gi, e_gh), 'host ' + route)


def test_saturated_gates_on_the_host():
    """gi of +-30 and +-1e4 in every gate and a large b_hh: finite, inside the bounds, saturated derivatives exactly 0"""
    c = G.saturated_case(100)
    for route in ('f32', 'bf16x6'):
        h_last, saved, d_gi, d_gh = G.run_float32(route, c['gi'], c['off'], c['w'], c['b'], c['dh'])
        assert all(np.isfinite(x).all() for x in (h_last, saved, d_gi, d_gh))
        G.assert_holds(G.forward_ratios(route, c['gi'], c['off'], c['w'], c['b'], saved, h_last), 'saturated fwd ' + route)
        G.assert_holds(G.backward_ratios(route, c['dh'], c['off'], c['w'], saved, d_gi, d_gh), 'saturated bwd ' + route)
        G.assert_saturated_derivatives_vanish(saved, d_gi, d_gh)
