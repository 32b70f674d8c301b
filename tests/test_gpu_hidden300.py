"""GPU tests of n_hidden = 300: 3x3 relation blocks through every kernel (one block per lane, 12-byte loads), the GRU
recurrences at H = 300 (not a multiple of 16 or 32), the GEMM fronts at K = 300 / 900 / 1200, the training step, the C
launch list and the global model -- against the fixtures the unmodified reference produced (tools/make_golden_d300.py),
fp64 evaluations written here, torch's CPU GRU and the oracle.  Tolerances are those of the same checks at 100 / 200 / 400
(tests/test_gpu_parity.py, tests/test_gpu_gather.py)."""
import contextlib

import numpy as np
import pytest
import torch

import gather_statement as GS
from helpers import O, fixtures, load_golden, train_case, global_shapes

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 2e-5      # tests/test_gpu_parity.py
D = 300


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _to(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---------------------------------------------------------------------------------------------
# 1. the RGCN layer vs the reference
# ---------------------------------------------------------------------------------------------
def test_rgcn_layer_matches_reference_golden_300(dev):
    import graph as G
    import ops
    gold = load_golden('rgcn_300.npz')
    n, num_rels = int(gold['n']), int(gold['num_rels'])
    p = fixtures.make_params(200 + D, {'weight': (2 * num_rels, D * D // 100), 'loop_weight': (D, D),
                                       'h': (n, D), 'gout': (n, D)}, scale=0.5)
    hb = G.HostBatch.from_edges(n, gold['src'], gold['dst'], gold['type_s'], num_rels)
    np.testing.assert_array_equal(hb.norm, gold['norm'])
    g = G.DeviceGraph(hb, dev)
    for relu in (0, 1):
        for reverse in (0, 1):
            h = _to(p['h'], dev).requires_grad_(True)
            w = _to(p['weight'], dev).requires_grad_(True)
            lw = _to(p['loop_weight'], dev).requires_grad_(True)
            y = ops.RGCNLayerFn.apply(h, w, lw, g, bool(reverse), bool(relu), 0.0, 0, None)
            (y * _to(p['gout'], dev)).sum().backward()
            tag = 'relu%d_rev%d_' % (relu, reverse)
            np.testing.assert_allclose(y.detach().cpu().numpy(), gold[tag + 'out'], rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(h.grad.cpu().numpy(), gold[tag + 'dh'], rtol=RTOL, atol=ATOL)
            for key, gr in (('dweight', w.grad), ('dloop', lw.grad)):
                ok, err, how = fixtures.check_packed(gold, tag + key, gr.cpu().numpy(), RTOL, ATOL * 10)
                assert ok, (tag + key, err, how)


# ---------------------------------------------------------------------------------------------
# 2 / 3. gather and dW vs fp64 on a fresh graph
# ---------------------------------------------------------------------------------------------
N_ROWS, N_OUT, T, HEAVY = 301, 120, 14, 24
_CASE = []


def _gather_fp64(x, src, dst, et, w, shift, tr, norm, addend, relu, n_out, src_limit, addend_rows, mask=None,
                 row_map=None):
    """The operator's fp64 statement (tests/gather_statement.py, written from include/renet_hip.h) -> (out, mag, kept
    in-degree); mask: the dropout multipliers of the addend."""
    return GS.statement(x, src, dst, et, w, D, T, shift, tr, norm, addend, relu, n_out, src_limit, addend_rows, mask=mask,
                        row_map=row_map)


def _within_bound(got, ref):
    """|got - out| <= (kept in-degree * 3 + 3) * 2^-24 * mag at every element: the derived bound of gather_statement."""
    return GS.assert_within_bound(got.cpu().numpy(), ref[0], ref[1], ref[2], D // 100)


def _case(dev):
    """One small multigraph, built once: paired edges (every fact in both directions, types r / r + 7), rows of in-degree 0,
    an exact duplicate edge, one hub row of 150 in-edges (more than two 64-edge index windows, above the heavy threshold:
    the workgroup-per-row path), relation 5 (and 12) without an edge, relation 2 with more edges than one 64-edge dW chunk."""
    if not _CASE:
        import graph as G
        rng = np.random.RandomState(300)
        num_rels, m = T // 2, 520
        a, b = rng.randint(0, N_ROWS - 20, m), rng.randint(0, N_ROWS - 20, m)       # rows >= 281: no edge at all
        r = rng.choice([0, 1, 2, 2, 2, 3, 4, 6], m)                                 # relation 5 never occurs
        b[:150] = 17                                                                # hub row 17 (inside the row prefix)
        a[200], b[200], r[200] = a[201], b[201], r[201]                             # duplicate multi-edge
        src, dst, et = np.concatenate((a, b)), np.concatenate((b, a)), np.concatenate((r, r + num_rels))
        hb = G.HostBatch().set_edges(N_ROWS, src, dst, et, T, heavy=HEAVY)
        hb.set_out_rows(N_OUT, src, dst, et)
        hb.set_gather_plan(N_OUT, heavy=HEAVY, budget=32)
        deg = np.diff(hb.row_ptr)
        assert deg.max() >= 150 and (deg == 0).sum() >= 20 and (r == 2).sum() > 64 and not (r == 5).any()
        g = G.DeviceGraph(hb, dev)
        assert g.heavy_rows is not None and g.heavy_rows.numel() >= 1
        x = rng.randn(N_ROWS, D).astype(np.float32)
        w = (rng.randn(T, 900) * 0.3).astype(np.float32)
        ad = rng.randn(N_ROWS, D).astype(np.float32)
        _CASE.append(dict(hb=hb, g=g, src=src, dst=dst, et=et, x=x, w=w, ad=ad, num_rels=num_rels))
    return _CASE[0]


def _drop_mask(dev, rows, p, seed):
    """The multipliers of the float4-group mask of a [rows, 300] tensor (renet_dropout on ones: group = flat index / 4)."""
    import dropout_masks
    import ops
    mask = ops.DropoutFn.apply(torch.ones(rows, D, device=dev), p, seed).cpu().numpy().astype(np.float64)
    assert np.array_equal(mask, dropout_masks.flat_mask(rows, D, seed, p))       # the host statement of common.h
    return mask


@pytest.mark.parametrize('drop_p', [0.0, 0.5])
def test_gather_300_matches_fp64_block_product(dev, drop_p):
    import renet_hip as K
    c = _case(dev)
    g, hb, src, dst, et, x, w, ad = (c[k] for k in ('g', 'hb', 'src', 'dst', 'et', 'x', 'w', 'ad'))
    tx, tw, tad = _to(x, dev), _to(w, dev), _to(ad, dev)
    seed = 1234567
    mask = _drop_mask(dev, N_ROWS, drop_p, seed) if drop_p else np.ones((N_ROWS, D))
    if drop_p:
        assert set(np.unique(mask).tolist()) == {0.0, 2.0}
    for tr in (False, True):
        for shift in (0, T // 2):
            ref = _gather_fp64(x, src, dst, et, w, shift, tr, None if tr else hb.norm, ad, not tr, N_ROWS, 0, 0, mask=mask)
            out = torch.full((N_ROWS, D), float('nan'), device=dev)
            K.rgcn_gather_items(tx, g, tw, shift, tr, tad, drop_p, seed, not tr, out, use_norm=not tr)
            _within_bound(out, ref)
            out2 = torch.full((N_ROWS, D), float('nan'), device=dev)                 # the plain-CSR kernel
            K.rgcn_gather(tx, g.row_ptr, g.col, g.etype, None if tr else g.norm, tw, shift, tr, tad, drop_p, seed, not tr,
                          out2, g.heavy_rows, g.heavy_thresh)
            _within_bound(out2, ref)
    # pruned forward: rows [0, N_OUT) only; without an addend, and as ops.RGCNLayerFn launches it for the last layer (the
    # self-loop product already in `out`: in-place addend under the mask, ReLU)
    outp = torch.full((N_OUT, D), float('nan'), device=dev)
    K.rgcn_gather_items(tx, g, tw, 0, False, None, 0.0, 0, False, outp, use_norm=True, pruned=True)
    refp = _gather_fp64(x, src, dst, et, w, 0, False, hb.norm, None, False, N_OUT, 0, 0)
    _within_bound(outp, refp)
    outp = _to(ad[:N_OUT].copy(), dev)
    K.rgcn_gather_items(tx, g, tw, 0, False, outp, drop_p, seed, True, outp, use_norm=True, pruned=True)
    refp = _gather_fp64(x, src, dst, et, w, 0, False, hb.norm, ad, True, N_OUT, 0, 0, mask=mask)
    _within_bound(outp, refp)
    # pruned backward: all rows are outputs, sources >= N_OUT skipped, in-place addend (under the mask) on the row prefix only
    rng = np.random.RandomState(2)
    gn = rng.randn(N_OUT, D).astype(np.float32)
    dh0 = np.zeros((N_ROWS, D), np.float32)
    dh0[:N_OUT] = rng.randn(N_OUT, D)
    dh = _to(dh0.copy(), dev)
    dh[N_OUT:] = float('nan')                          # rows >= addend_rows must be overwritten, never read
    K.rgcn_gather_items(_to(gn, dev), g, tw, T // 2, True, dh, drop_p, seed, False, dh, use_norm=False, pruned=True,
                        src_limit=N_OUT, addend_rows=N_OUT)
    gn_full = np.zeros((N_ROWS, D), np.float32)
    gn_full[:N_OUT] = gn
    refb = _gather_fp64(gn_full, src, dst, et, w, T // 2, True, None, dh0, False, N_ROWS, N_OUT, N_OUT, mask=mask)
    _within_bound(dh, refb)


@pytest.mark.parametrize('drop_p', [0.0, 0.5])
def test_table_addressed_first_layer_300_matches_fp64(dev, drop_p):
    """renet_rgcn_gather_items_table: h0 = table[node_ent] is never materialised; the self-loop addend is a table row too."""
    import graph as G
    import renet_hip as K
    c = _case(dev)
    src, dst, et, w = c['src'], c['dst'], c['et'], c['w']
    rng = np.random.RandomState(9)
    n_ent = 70
    hb = G.HostBatch.from_edges(N_ROWS, src, dst, et, c['num_rels'], heavy=HEAVY)
    hb.node_ent = rng.randint(0, n_ent, N_ROWS).astype(np.int32)
    hb.plan_node_ent = G.SegPlan.host(hb.node_ent)
    g = G.DeviceGraph(hb, dev)
    assert g.heavy_rows is not None
    tab = (rng.randn(n_ent, D) * 0.3).astype(np.float32)
    add_tab = rng.randn(n_ent, D).astype(np.float32)
    seed = 77
    mask = _drop_mask(dev, N_ROWS, drop_p, seed) if drop_p else np.ones((N_ROWS, D))
    out = torch.full((N_ROWS, D), float('nan'), device=dev)
    K.rgcn_gather_items_table(_to(tab, dev), g, _to(w, dev), 0, _to(add_tab, dev), drop_p, seed, True, out)
    ref = _gather_fp64(tab, src, dst, et, w, 0, False, hb.norm, add_tab, True, N_ROWS, 0, 0, mask=mask,
                       row_map=hb.node_ent)
    _within_bound(out, ref)


def test_dw_300_matches_fp64(dev, monkeypatch):
    """dW[t] = sum over the edges of type t of x[src]^T (outer, per block) gn[dst]; a type without an edge gets zeros, a
    type with more than 64 edges spans several chunks; beta accumulates."""
    import renet_hip as K
    c = _case(dev)
    g, src, dst, et, x = c['g'], c['src'], c['dst'], c['et'], c['x']
    rng = np.random.RandomState(4)
    gn = rng.randn(N_ROWS, D).astype(np.float32)
    assert int(g.n_chunks) > len(np.unique(et))                      # some type owns more than one chunk
    ref = np.zeros((T, 100, 3, 3))
    np.add.at(ref, et, np.einsum('ebi,ebj->ebij', x.astype(np.float64)[src].reshape(-1, 100, 3),
                                 gn.astype(np.float64)[dst].reshape(-1, 100, 3)))
    ref = ref.reshape(T, 900)
    assert not ref[5].any() and not ref[12].any()
    dw = torch.full((T, 900), float('nan'), device=dev)
    args = (_to(x, dev), _to(gn, dev), g.e_src, g.e_dst, g.chunk_ptr, g.chunk_type, g.n_chunks, g.type_chunk_ptr, T, 0)
    K.rgcn_bwd_w(*args, dw)
    got = dw.cpu().numpy()
    for t in range(T):                                   # the bound of test_full_size_dw_matches_fp64_sampled, every type
        ne = int((et == t).sum())
        np.testing.assert_allclose(got[t], ref[t], rtol=1e-4, atol=1e-4 * max(1.0, ne) ** 0.5, err_msg='type %d' % t)
    assert float(dw[5].abs().max()) == 0.0 and float(dw[12].abs().max()) == 0.0
    acc = dw.clone()                                     # beta = 1: accumulate into an existing gradient
    K.rgcn_bwd_w(*args, acc, beta=1.0)
    assert torch.equal(acc, dw + dw)
    monkeypatch.setenv('RENET_BWDW_64', '1')             # the 64-bit-addressing entry: same arithmetic, same order
    dw64 = torch.full((T, 900), float('nan'), device=dev)
    K.rgcn_bwd_w(*args, dw64)
    assert torch.equal(dw64, dw)


# ---------------------------------------------------------------------------------------------
# 4. GRU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['persistent', 'steps', 'f32'])
@pytest.mark.parametrize('i,h,nseq', [(1200, 300, 31), (900, 300, 77)])
def test_gru_300_matches_torch_cpu(dev, i, h, nseq, route, monkeypatch):
    import model as M
    import renet_hip as K
    if route == 'f32':
        monkeypatch.delenv('RENET_GRU', raising=False)
    else:
        monkeypatch.setenv('RENET_GRU', route)
    torch.manual_seed(7)
    lens = [10] * (nseq - 11) + [9, 9, 7, 5, 5, 5, 3, 2, 1, 1, 1]
    b, l = len(lens), 10
    ref = torch.nn.GRU(i, h, batch_first=True)
    x = torch.randn(b, l, i)
    for k, n in enumerate(lens):
        x[k, n:] = 0
    x.requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True)
    _, hn = ref(packed)
    gout = torch.randn(b, h)
    (hn[0] * gout).sum().backward()
    mine = M.GRU(i, h).to(dev)
    mine.load_state_dict(ref.state_dict())
    xd = packed.data.detach().to(dev).requires_grad_(True)
    pk = torch.nn.utils.rnn.PackedSequence(xd, packed.batch_sizes)
    with K.gemm_mode('f32') if route == 'f32' else contextlib.nullcontext():
        _, hm = mine(pk, total_rows=b + 3)
        assert hm.shape == (1, b + 3, h) and float(hm[0, b:].abs().max()) == 0.0
        (hm[0, :b] * gout.to(dev)).sum().backward()
    np.testing.assert_allclose(hm[0, :b].detach().cpu().numpy(), hn[0].detach().numpy(), rtol=1e-4, atol=1e-5)
    dx_ref = torch.nn.utils.rnn.pack_padded_sequence(x.grad, lens, batch_first=True).data
    np.testing.assert_allclose(xd.grad.cpu().numpy(), dx_ref.numpy(), rtol=1e-3, atol=2e-5)
    for name, p in mine.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), getattr(ref, name).grad.numpy(), rtol=1e-3, atol=1e-4)


_GRU_LAYOUT_CASE = []


def _gru_layout_case():
    """Four problems (W0, A), (W1, A), (W0, B), (W1, B) over two packed layouts at H = 300, and their float64 results."""
    if not _GRU_LAYOUT_CASE:
        import ctypes
        from test_gpu_parity import _gru_float64
        torch.manual_seed(11)
        h_dim = 300
        ws = [(torch.randn(3 * h_dim, h_dim) * 0.05, torch.randn(3 * h_dim)) for _ in range(2)]
        lays = []
        for lens, nstep in (([5] * 20 + [4] * 6 + [3] * 5 + [2] * 3 + [1] * 3, 5), ([3] * 9 + [2] * 6 + [1] * 5, 3)):
            off = [0]
            for j in range(nstep):
                off.append(off[-1] + sum(1 for n in lens if n > j))
            lays.append((off, (ctypes.c_int32 * len(off))(*off), len(lens)))
        probs = []
        for off, off_c, b in lays:
            for w_hh, b_hh in ws:
                gi, dh = torch.randn(off[-1], 3 * h_dim), torch.randn(b, h_dim)
                probs.append(dict(gi=gi, dh=dh, w_hh=w_hh, b_hh=b_hh, off=off_c, b=b,
                                  ref=_gru_float64(gi, off, w_hh, b_hh, dh)))
        _GRU_LAYOUT_CASE.append((h_dim, probs))
    return _GRU_LAYOUT_CASE[0]


@pytest.mark.parametrize('route', ['persistent', 'steps', 'f32'])
def test_gru_300_four_problems_two_layouts_match_a_float64_recurrence(dev, route, monkeypatch):
    import renet_hip as K
    if route == 'f32':
        monkeypatch.delenv('RENET_GRU', raising=False)
    else:
        monkeypatch.setenv('RENET_GRU', route)
    h_dim, probs = _gru_layout_case()
    w_dev = {}
    for p in probs:
        w_dev.setdefault(id(p['w_hh']), (p['w_hh'].to(dev), p['b_hh'].to(dev)))
    w_hhs = [w_dev[id(p['w_hh'])][0] for p in probs]
    b_hhs = [w_dev[id(p['w_hh'])][1] for p in probs]
    offs = [p['off'] for p in probs]
    out_rows = [p['b'] + 3 if k < 2 else p['b'] for k, p in enumerate(probs)]
    with K.gemm_mode('f32') if route == 'f32' else contextlib.nullcontext():
        hs, svs = K.gru_fwd_layouts([p['gi'].to(dev) for p in probs], offs, h_dim, w_hhs, b_hhs, out_rows)
        d_gis, d_ghs = K.gru_bwd_layouts([p['dh'].to(dev) for p in probs], offs, h_dim, w_hhs, svs)
    for k, p in enumerate(probs):
        h_ref, sv_ref, dgi_ref, dgh_ref = p['ref']
        b = p['b']
        assert hs[k].shape == (out_rows[k], h_dim) and float(hs[k][b:].abs().sum()) == 0.0, k
        np.testing.assert_allclose(hs[k][:b].cpu().numpy(), h_ref.numpy(), rtol=1e-4, atol=1e-5, err_msg='h_last %d' % k)
        np.testing.assert_allclose(svs[k].cpu().numpy(), sv_ref.numpy(), rtol=1e-4, atol=1e-5, err_msg='saved %d' % k)
        np.testing.assert_allclose(d_gis[k].cpu().numpy(), dgi_ref.numpy(), rtol=1e-3, atol=2e-5, err_msg='dGi %d' % k)
        np.testing.assert_allclose(d_ghs[k].cpu().numpy(), dgh_ref.numpy(), rtol=1e-3, atol=2e-5, err_msg='dGh %d' % k)


# ---------------------------------------------------------------------------------------------
# 5. GEMM fronts at the shapes of n_hidden = 300
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,k', [(41, 900, 1200), (41, 900, 900), (257, 300, 300), (64, 129, 900)])
@pytest.mark.parametrize('mode', ['bf16x6', 'f32', 'f16x3'])
def test_gemm_300_shapes_match_fp64(dev, m, n, k, mode):
    """Gi = X W_ih^T (K = 1200 / 900, N = 900), the self-loop product (K = N = 300: beyond the skinny weight-resident
    front's K <= 208, so the general kernels, as at 400) and the head (K = 900), with both weight orientations, in the three
    modes."""
    import renet_hip as K
    rng = np.random.RandomState(m * 131 + n * 17 + k)
    a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    bias = rng.uniform(-1, 1, n).astype(np.float32)
    for tb in (0, 1):
        b = rng.uniform(-1, 1, (n, k) if tb else (k, n)).astype(np.float32)
        ref = a.astype(np.float64) @ (b.T if tb else b).astype(np.float64) + bias
        out = K.gemm(_to(a, dev), _to(b, dev), tb=bool(tb), bias=_to(bias, dev), mode=mode)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * k ** 0.5)
    at = rng.uniform(-1, 1, (k, m)).astype(np.float32)                       # weight-gradient orientation: A stored [K, M]
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    out = K.gemm(_to(at, dev), _to(b, dev), ta=True, mode=mode)
    np.testing.assert_allclose(out.cpu().numpy(), at.T.astype(np.float64) @ b.astype(np.float64), rtol=1e-5,
                               atol=1e-5 * k ** 0.5)


def test_planes_head_at_k900_with_the_bias_column(dev):
    """The entity head on planes at 3 * n_hidden = 900 (ops._head_forward / backward): logits = feat W^T + b on the packed
    [feat | 1] matrix viewed without its ones column, dfeat = dlogits W, and dW = dlogits^T [feat | 1] whose last column
    (the 901st: the bias gradient) goes to col_out."""
    import renet_hip as K
    rng = np.random.RandomState(900)
    bsz, n_cls, k = 64, 129, 900
    feat = rng.uniform(-1, 1, (bsz, k)).astype(np.float32)
    w = rng.uniform(-1, 1, (n_cls, k)).astype(np.float32)
    bias = rng.uniform(-1, 1, n_cls).astype(np.float32)
    dl = rng.uniform(-1, 1, (bsz, n_cls)).astype(np.float32)
    f1 = K.pack_planes(_to(feat, dev), ones_col=True)
    assert (f1.R, f1.C) == (bsz, k + 1)
    w_pl = K.pack_planes(_to(w, dev))
    logits = K.gemm_planes(K.PlanesMat(f1.p, f1.R, f1.C - 1), w_pl, tb=True, bias=_to(bias, dev))
    tol = 1e-5 * k ** 0.5
    np.testing.assert_allclose(logits.cpu().numpy(), feat.astype(np.float64) @ w.T.astype(np.float64) + bias, rtol=1e-5,
                               atol=tol)
    dl_pl = K.pack_planes(_to(dl, dev))
    dfeat = K.gemm_planes(dl_pl, w_pl)
    np.testing.assert_allclose(dfeat.cpu().numpy(), dl.astype(np.float64) @ w.astype(np.float64), rtol=1e-5,
                               atol=1e-5 * n_cls ** 0.5)
    d_w = torch.full((n_cls, k), float('nan'), device=dev)
    d_b = torch.full((n_cls,), float('nan'), device=dev)
    K.gemm_planes(dl_pl, f1, ta=True, out=d_w, col_out=d_b)
    np.testing.assert_allclose(d_w.cpu().numpy(), dl.T.astype(np.float64) @ feat.astype(np.float64), rtol=1e-5,
                               atol=1e-5 * bsz ** 0.5)
    np.testing.assert_allclose(d_b.cpu().numpy(), dl.astype(np.float64).sum(0), rtol=1e-5, atol=1e-5 * bsz ** 0.5)


# ---------------------------------------------------------------------------------------------
# 6. the training step vs the reference, and through the C launch list
# ---------------------------------------------------------------------------------------------
def _build_model(c, dev, dropout=0.0):
    import model as M
    import utils as U
    cfg = c['cfg']
    net = M.RENet(cfg['num_ent'], c['d'], cfg['num_rels'], dropout=dropout, seq_len=c['seq_len'])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in c['params'].items()})
    net.global_emb = {t: torch.from_numpy(v).view(1, 1, -1) for t, v in c['global_emb'].items()}
    net.to(dev)
    return net, U.build_graph_dict(c['train'], cfg['num_rels'])


def test_training_step_300_matches_reference_golden(dev):
    c = train_case('tiny', D)
    gold = c['gold']
    net, gd = _build_model(c, dev)
    sd = net.state_dict()
    assert tuple(sd['aggregator.rgcn1.weight'].shape) == (2 * c['cfg']['num_rels'], 900)
    assert tuple(sd['encoder.weight_ih_l0'].shape) == (900, 1200) and tuple(sd['encoder_r.weight_ih_l0'].shape) == (900, 900)
    assert tuple(sd['linear.weight'].shape) == (c['cfg']['num_ent'], 900)
    net.eval()
    batch = torch.from_numpy(c['batch']).to(dev)
    total = 0
    for tag, subject in (('s', True), ('o', False)):
        loss = net(batch, c['hists']['s'], c['hists']['o'], gd, subject=subject)
        ref = float(gold['loss_' + tag])
        assert abs(loss.item() - ref) < 2e-4 * max(1.0, abs(ref)), (tag, loss.item(), ref)
        total = total + loss
    total.backward()
    for k, p in net.named_parameters():
        g = p.grad.cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
        ok, err, how = fixtures.check_packed(gold, 'grad.' + k, g, 2e-3, 3e-5)
        assert ok, (k, err, how)


@pytest.mark.parametrize('dropout', [0.0, 0.5])
def test_c_launch_list_300_is_bit_identical_to_the_autograd_path(dev, dropout):
    """A merged step at 300 is two C-ABI calls like at any other width (step_plan.StepFn), bit-identical to ops.py."""
    from test_gpu_step_plan import _stream, _train
    data = _stream(num_t=24)
    la, fa, pa, ua = _train(dev, data, True, dropout, hidden=D, steps=2, batch=128)
    lb, fb, pb, ub = _train(dev, data, False, dropout, hidden=D, steps=2, batch=128)
    assert all('StepFn' in u for u in ua), ua
    assert not any('StepFn' in u for u in ub), ub
    assert la == lb, (la, lb)
    for x, y in zip(fa, fb):
        assert float(x.abs().max()) > 0 and torch.equal(x, y)
    assert torch.equal(pa, pb)


# ---------------------------------------------------------------------------------------------
# 7. the global model vs the reference
# ---------------------------------------------------------------------------------------------
def test_global_model_300_matches_reference_golden(dev):
    import global_model as GM
    import utils as U
    gold = load_golden('global_tiny_300_max1.npz')
    cfg, tr, va, te = fixtures.split_dataset('tiny')
    seq_len = int(gold['seq_len'])
    p = fixtures.make_params(int(gold['param_seed']), global_shapes(cfg['num_ent'], cfg['num_rels'], D))
    net = GM.RENet_global(cfg['num_ent'], D, cfg['num_rels'], dropout=0.0, seq_len=seq_len, maxpool=1)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    net.to(dev)
    gd = U.build_graph_dict(tr, cfg['num_rels'])
    times = np.unique(tr[:, 3])
    loss = net(torch.from_numpy(times), torch.from_numpy(gold['true_s']).to(dev),
               torch.from_numpy(gold['true_o']).to(dev), gd, subject=True)
    assert abs(loss.item() - float(gold['loss'])) < 2e-4 * max(1.0, abs(float(gold['loss'])))
    loss.backward()
    for k, prm in net.named_parameters():
        if ('grad.' + k) in gold or ('grad.' + k + '__samp') in gold:
            ok, err, how = fixtures.check_packed(gold, 'grad.' + k, prm.grad.cpu().numpy(), 2e-3, 3e-5)
            assert ok, (k, err, how)
    with torch.no_grad():
        for k, t in enumerate(gold['predict_t']):
            for subj in (True, False):
                emb, logits, prob = net.predict(int(t), gd, subject=subj)
                tag = 'predict%d_%s_' % (k, 's' if subj else 'o')
                np.testing.assert_allclose(emb.view(-1).cpu().numpy(), gold[tag + 'emb'], rtol=RTOL, atol=ATOL)
                np.testing.assert_allclose(logits.view(-1).cpu().numpy(), gold[tag + 'logits'], rtol=RTOL, atol=ATOL)
        ge = net.get_global_emb(times, gd)
        assert [int(x) for x in ge.keys()] == gold['global_emb_keys'].tolist()
        vals = np.stack([ge[x].view(-1).cpu().numpy() for x in ge.keys()])
        np.testing.assert_allclose(vals, gold['global_emb_vals'], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------
# 8. train mode vs the oracle under replayed masks; inference on one history vs the oracle
# ---------------------------------------------------------------------------------------------
def test_train_mode_step_300_matches_oracle_under_replayed_masks(dev, monkeypatch):
    """One train-mode step (dropout 0.5 at every site: both RGCN self-loops, X, Xr, both heads) on a fresh seeded stream.
    The seeds the device draws are recorded, each site's float4-group mask is regenerated from its seed (renet_dropout on
    ones of the site's [rows, cols] layout), re-indexed to the oracle's layout (its node numbering; padded [B, L, .] for the
    packed [S, .] sequences) and handed to the oracle in place of torch's generator: both sides then evaluate the same
    function.  Loss per direction and every parameter gradient, at the bounds of the eval-mode step."""
    import graph as G
    import model as M
    import ops
    import utils as U
    from helpers import renet_shapes
    num_ent, num_rels, L, B, p = 150, 6, 10, 96, 0.5
    q = fixtures.tiny_stream(301, num_ent, num_rels, 16, 40, time_unit=24)
    (sh, sht), (oh, oht), _ = O.build_histories(q, num_ent)
    idx = np.sort(np.random.RandomState(3).choice(len(q), B, replace=False))
    hists = {True: ([sh[i] for i in idx], [sht[i] for i in idx]), False: ([oh[i] for i in idx], [oht[i] for i in idx])}
    params = fixtures.make_params(303, renet_shapes(num_ent, num_rels, D))
    times = np.unique(q[:, 3])
    gl = fixtures.make_params(304, {'g': (len(times), D)}, scale=0.3)['g']
    ge = {int(t): torch.from_numpy(gl[k]) for k, t in enumerate(times)}
    # ---- the device step, its seeds recorded in drawing order: per direction rgcn1, rgcn2, X, Xr, head, relation head
    seeds, draw = [], ops.next_seed
    monkeypatch.setattr(ops, 'next_seed', lambda graph_site=False: seeds.append(draw(graph_site)) or seeds[-1])
    net = M.RENet(num_ent, D, num_rels, dropout=p, seq_len=L)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net.global_emb = {t: v.view(1, 1, -1) for t, v in ge.items()}
    net.to(dev)
    net.train()
    gd = U.build_graph_dict(q, num_rels)
    torch.manual_seed(300)
    ops.reset_seed_counter(0)
    losses = [net.loss_prepared(net.prepare(q[idx], hists[subject], gd, subject=subject)) for subject in (True, False)]
    assert len(seeds) == 12 and len(set(seeds)) == 12, seeds
    (losses[0] + losses[1]).backward()

    def mask(rows, cols, seed):
        m = ops.DropoutFn.apply(torch.ones(rows, cols, device=dev), p, seed).cpu()
        assert set(np.unique(m.numpy()).tolist()) == {0.0, 2.0}
        return m

    # ---- the oracle under the same masks
    op = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in params.items()}
    ogd = O.build_graph_dict(q, num_rels)
    ref_losses = []
    for k, subject in enumerate((True, False)):
        s_l1, s_l2, s_x, s_xr, s_h1, s_h2 = seeds[6 * k:6 * k + 6]
        hist, hist_t = hists[subject]
        s_np, r_np = q[idx][:, 0 if subject else 2], q[idx][:, 1]
        hb = G.build_batch(G.store_for(gd), num_ent, num_rels, s_np, r_np, G.FlatHistory.from_lists(hist, hist_t), sort=True)
        bg = O.batch_for_histories(hist, hist_t, s_np, ogd, sort=True)
        assert (hb.N, hb.S, hb.nnz) == (bg.num_nodes, len(bg.subj_row), len(bg.lens)) and np.array_equal(hb.lens, bg.lens)
        assert 0 < hb.nA < hb.N and 0 < hb.nnz                 # the last layer is pruned: the table layer and RGCNLayerFn both run
        # oracle node -> device row, by (graph timestamp, entity)
        ot = np.repeat(np.asarray(bg.graph_t), np.diff(np.asarray(list(bg.graph_off) + [bg.num_nodes])))
        row_of = {(int(t), int(e)): i for i, (t, e) in enumerate(zip(hb.graph_t[hb.node_slot], hb.node_ent))}
        o2d = torch.tensor([row_of[(int(t), int(e))] for t, e in zip(ot, bg.ent)])
        # packed row off[j] + i  <->  step j of sorted sequence i
        off, lens = hb.step_off.astype(np.int64), hb.lens

        def padded(m):
            out = torch.zeros(hb.nnz, L, m.shape[1])
            for i in range(hb.nnz):
                for j in range(int(lens[i])):
                    out[i, j] = m[off[j] + i]
            return out

        pending = [mask(hb.N, D, s_l1)[o2d], mask(hb.N, D, s_l2)[o2d],      # (layer 2: rows >= nA are never read)
                   padded(mask(hb.S, 4 * D, s_x)), padded(mask(hb.S, 3 * D, s_xr)),
                   mask(B, 3 * D, s_h1), mask(B, 2 * D, s_h2)]

        def replay(x, p=0.5, training=True, inplace=False):
            m = pending.pop(0)
            assert training and tuple(m.shape) == tuple(x.shape), (tuple(m.shape), tuple(x.shape))
            return x * m

        with monkeypatch.context() as mp:
            mp.setattr(torch.nn.functional, 'dropout', replay)
            ref_losses.append(O.renet_forward_loss(op, q[idx], hist, hist_t, ogd, ge, num_rels, L, subject=subject,
                                                   dropout=p))
        assert not pending
    (ref_losses[0] + ref_losses[1]).backward()
    for k in (0, 1):
        got, ref = float(losses[k]), float(ref_losses[k])
        print('train-mode 300 loss[%d] %.7f oracle %.7f' % (k, got, ref))
        assert abs(got - ref) < 2e-4 * max(1.0, abs(ref)), (k, got, ref)
    for k, prm in net.named_parameters():
        g = prm.grad.cpu().numpy() if prm.grad is not None else np.zeros(tuple(prm.shape), np.float32)
        ref = op[k].grad.numpy() if op[k].grad is not None else np.zeros(tuple(prm.shape), np.float32)
        ok, err, how = fixtures.check_packed({'grad.' + k: ref}, 'grad.' + k, g, 2e-3, 3e-5)
        print('train-mode 300 grad %-32s max |err| %.3e of max |ref| %.3e' % (k, err, float(np.abs(ref).max())))
        assert ok, (k, err, how)



def test_aggregator_predict_300_matches_oracle(dev):
    """RGCNAggregator.predict (unsorted path) on one history of the tiny stream."""
    c = train_case('tiny', D)
    cfg = c['cfg']
    net, gd = _build_model(c, dev)
    net.eval()
    ogd = O.build_graph_dict(c['train'], cfg['num_rels'])
    (sh, sht), _, _ = O.build_histories(c['train'], cfg['num_ent'])
    k = max(range(len(c['train'])), key=lambda i: len(sh[i]))
    assert len(sh[k]) >= 2
    e, rel_id = int(c['train'][k, 0]), int(c['train'][k, 1])
    hist, hist_t = list(sh[k][-c['seq_len']:]), list(sht[k][-c['seq_len']:])
    params = {kk: torch.from_numpy(v) for kk, v in c['params'].items()}
    oge = {t: torch.from_numpy(v) for t, v in c['global_emb'].items()}
    nr = cfg['num_rels']
    for reverse in (False, True):
        rel = params['rel_embeds'][nr:] if reverse else params['rel_embeds'][:nr]
        bg, h2, x, xr = O.aggregator_sequences(params, [hist], [hist_t], [e], [rel_id], rel, ogd, oge, reverse,
                                               len(hist), sort=False)
        with torch.no_grad():
            rel_d = net.rel_embeds[nr:] if reverse else net.rel_embeds[:nr]
            inp, inp_r = net.aggregator.predict((hist, hist_t), np.asarray([e]), np.asarray([rel_id]), net.ent_embeds,
                                                rel_d, gd, net.global_emb, reverse=reverse)
        np.testing.assert_allclose(inp.cpu().numpy(), x[0].numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(inp_r.cpu().numpy(), xr[0].numpy(), rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------
# 9. what stays refused
# ---------------------------------------------------------------------------------------------
def test_other_widths_and_bf16_storage_at_300_are_refused(dev, monkeypatch):
    import ctypes
    import model as M
    import renet_hip as K
    with pytest.raises(ValueError):
        M.RENet(50, 500, 4, dropout=0.0, seq_len=4)
    # the C ABI answers RENET_ERR_UNSUPPORTED (-2) before any launch: a width without kernels ...
    g = _case(dev)['g']
    with pytest.raises(K.RenetHipError, match='code -2'):
        K.rgcn_gather_items(torch.zeros(N_ROWS, 500, device=dev), g, torch.zeros(T, 2500, device=dev), 0, False, None, 0.0,
                            0, False, torch.zeros(N_ROWS, 500, device=dev))
    # ... and bf16-stored relation blocks at 300 (they do not fall into the 400 arm of the width switch)
    x3, out3 = torch.zeros(N_ROWS, D, device=dev), torch.full((N_ROWS, D), 7.0, device=dev)
    w3 = torch.zeros(T, 900, device=dev)
    with pytest.raises(K.RenetHipError, match='code -2'):
        K.rgcn_gather_items(x3, g, w3, 0, False, None, 0.0, 0, False, out3, w16=K.pack_bf16(w3))
    assert float((out3 - 7.0).abs().max()) == 0.0                       # nothing ran
    # bf16 storage is a process-wide mode (RENET_GEMM=bf16s): the constructor refuses 300 in such a process, and so does
    # the one-plane recurrence entry
    monkeypatch.setattr(K, 'GEMM_MODE', 'bf16s')
    with pytest.raises(ValueError):
        M.RENet(50, D, 4, dropout=0.0, seq_len=4)
    off = (ctypes.c_int32 * 2)(0, 4)
    with pytest.raises(K.RenetHipError, match='code -2'):
        K.gru_fwd_layouts([torch.zeros(4, 900, device=dev)], [off], D, [torch.zeros(900, D, device=dev)],
                          [torch.zeros(900, device=dev)], [4])
