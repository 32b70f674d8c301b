"""The GRU recurrences (re-net_amd/csrc/gru*.hip) through their C entry points against the float64 step statements of
tests/gru_statement.py: every saved quantity against a statement built from the kernel's own upstream saved values, each with
its derived bound (no bound is fitted to a kernel: tests/test_gru_statement_cpu.py holds them to host evaluations).
Outputs are prefilled with a NaN pattern and carry spare sentinel rows, so unwritten rows and overruns show; the workspace is
prefilled too.  Run with -s for the worst error / bound per case.

Routes: 'persistent' (default) and 'steps' (RENET_GRU=steps) of the six-pair bf16 arithmetic, 'f32' (the *_f32 entries),
'bf16' (the one-plane *_bf16 entries, no H = 300)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gru_statement as G

pytestmark = pytest.mark.gpu

HS = [100, 200, 300, 400]
ROUTE_H = [(r, h) for r in ('persistent', 'steps', 'f32', 'bf16') for h in HS if not (r == 'bf16' and h == 300)]
PATTERN = 0x7fc0dead                                    # a quiet NaN no kernel produces
PATTERN16 = 0x7fc1
SPARE = 2                                               # sentinel rows behind every output


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _select(route, monkeypatch):
    """-> (entry point suffix, arithmetic of the statements)"""
    import renet_hip as K
    if route == 'steps':
        monkeypatch.setenv('RENET_GRU', 'steps')
    else:
        monkeypatch.delenv('RENET_GRU', raising=False)
    if route in ('persistent', 'steps'):
        return '', ('f32' if K.GEMM_MODE == 'f32' else 'bf16x6')        # (a RENET_GEMM=f32 process runs the exact kernels)
    return '_' + route, route


def _guarded(rows, cols, dev):
    return torch.full((rows + SPARE, cols), PATTERN, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


def _check_guard(t, rows, what, written=True):
    b = _bits(t)
    assert bool((b[rows:] == PATTERN).all()), '%s: written behind its last row' % what
    if written:
        left = int((b[:rows] == PATTERN).sum())
        assert left == 0, '%s: %d elements of its %d rows never written' % (what, left, rows)
    else:
        assert bool((b[:rows] == PATTERN).all()), '%s: written by a refused call' % what


class Call(object):
    """n problems on the device: dicts of G.case() fields + 'off_c' (one ctypes array per layout) + 'out_rows'."""

    def __init__(self, dev, h, probs):
        self.dev, self.h, self.probs, self.n = dev, h, probs, len(probs)
        up = {}

        def dv(a):
            if id(a) not in up:
                up[id(a)] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            return up[id(a)]
        self.gi = [dv(p['gi']) for p in probs]
        self.w = [dv(p['w']) for p in probs]            # problems of one W_hh pass the SAME device tensor (one plane split)
        self.b = [dv(p['b']) for p in probs]
        self.dh = [dv(p['dh']) for p in probs]
        self.nb = [p['off'][1] - p['off'][0] for p in probs]
        self.rows = [p.get('out_rows', nb) for p, nb in zip(probs, self.nb)]
        self.s = [p['off'][-1] for p in probs]

    def _frame(self, offs=None, ls=None, ws_bytes=None):
        import renet_hip as K
        offs = offs or [p['off_c'] for p in self.probs]
        so = (ctypes.c_void_p * self.n)(*[ctypes.cast(o, ctypes.c_void_p).value for o in offs])
        ls = (ctypes.c_int * self.n)(*(ls or [len(o) - 1 for o in offs]))
        need = self.n * K.lib().renet_gru_workspace(max(self.nb), self.h)
        ws = torch.full((need // 4 + 64,), PATTERN, dtype=torch.int32, device=self.dev)
        return so, ls, ws, (need if ws_bytes is None else ws_bytes)

    def forward(self, suffix, rows=None, **kw):
        import renet_hip as K
        so, ls, ws, nbytes = self._frame(**kw)
        hl = [_guarded(r, self.h, self.dev) for r in self.rows]
        sv = [_guarded(s, 5 * self.h, self.dev) for s in self.s]
        rc = getattr(K.lib(), 'renet_gru_fwd_layouts' + suffix)(
            self.n, K._ptrs(self.gi), so, ls, self.h, K._ptrs(self.w), K._ptrs(self.b), K._ptrs(hl),
            (ctypes.c_int * self.n)(*(rows or self.rows)), K._ptrs(sv), ws.data_ptr(), nbytes, K._stream())
        torch.cuda.synchronize()
        assert bool((ws[nbytes // 4:] == PATTERN).all()) or rc != 0, 'forward wrote behind its workspace'
        return rc, hl, sv

    def backward(self, suffix, sv, out_ld=None, **kw):
        import renet_hip as K
        so, ls, ws, nbytes = self._frame(**kw)
        head = (self.n, K._ptrs(self.dh), so, ls, self.h, K._ptrs(self.w), K._ptrs(sv))
        if out_ld is None:
            dgi = [_guarded(s, 3 * self.h, self.dev) for s in self.s]
            dgh = [_guarded(s, 3 * self.h, self.dev) for s in self.s]
            rc = getattr(K.lib(), 'renet_gru_bwd_layouts' + suffix)(*head, K._ptrs(dgi), K._ptrs(dgh), ws.data_ptr(),
                                                                    nbytes, K._stream())
        else:
            dgi = [torch.full((s + SPARE, out_ld), PATTERN16, dtype=torch.int16, device=self.dev) for s in self.s]
            dgh = [torch.full((s + SPARE, out_ld), PATTERN16, dtype=torch.int16, device=self.dev) for s in self.s]
            rc = K.lib().renet_gru_bwd_layouts_bf16out(*head, K._ptrs(dgi), K._ptrs(dgh), out_ld, ws.data_ptr(), nbytes,
                                                       K._stream())
        torch.cuda.synchronize()
        assert bool((ws[nbytes // 4:] == PATTERN).all()) or rc != 0, 'backward wrote behind its workspace'
        return rc, dgi, dgh


def _run_and_check(dev, suffix, stmt, h, probs, what, fwd=True, bwd=True, twice=True, describe=None):
    """Both directions of one call, twice; guards, bit-reproducibility and every statement.  -> worst ratios"""
    c = Call(dev, h, probs)
    rc, hl, sv = c.forward(suffix)
    assert rc == 0, (what, 'forward', rc)
    rc, dgi, dgh = c.backward(suffix, sv)
    assert rc == 0, (what, 'backward', rc)
    for k in range(c.n):
        _check_guard(hl[k], c.rows[k], '%s h_last %d' % (what, k))
        _check_guard(sv[k], c.s[k], '%s saved %d' % (what, k))
        _check_guard(dgi[k], c.s[k], '%s dGi %d' % (what, k))
        _check_guard(dgh[k], c.s[k], '%s dGh %d' % (what, k))
    if twice:
        _, hl2, sv2 = c.forward(suffix)
        _, dgi2, dgh2 = c.backward(suffix, sv2)
        for a, b_ in zip(hl + sv + dgi + dgh, hl2 + sv2 + dgi2 + dgh2):
            assert torch.equal(_bits(a), _bits(b_)), '%s: a second identical call returns other bits' % what
    worst = {}
    for k, p in enumerate(probs):
        svk = sv[k][:c.s[k]].cpu().numpy()
        parts = []
        if fwd:
            parts.append(G.forward_ratios(stmt, p['gi'], p['off'], p['w'], p['b'], svk, hl[k][:c.rows[k]].cpu().numpy()))
        if bwd:
            parts.append(G.backward_ratios(stmt, p['dh'], p['off'], p['w'], svk, dgi[k][:c.s[k]].cpu().numpy(),
                                           dgh[k][:c.s[k]].cpu().numpy()))
        for r in parts:
            for name, v in G.worst(r).items():
                worst[name] = max(worst.get(name, 0.0), v)
            G.assert_holds(r, '%s problem %d' % (what, k), (lambda name, i, k=k: describe(k, name, i)) if describe else None)
    return worst, (hl, sv, dgi, dgh)


def _show(what, worst):
    print('\n%-44s %s' % (what, ' '.join('%s %.3f' % kv for kv in sorted(worst.items()) if kv[1] > 0)))


def _with_off(c):
    c['off_c'] = (ctypes.c_int32 * len(c['off']))(*c['off'])
    return c


def _lens_of_batch_sizes(bs):
    return sorted([sum(1 for b in bs if b > i) for i in range(bs[0])], reverse=True)


# ---------------------------------------------------------------------------------------------
# 1. step statements at the layout edges
# ---------------------------------------------------------------------------------------------
EDGE_LAYOUTS = [
    ('B=1 L=1', [1]),
    ('B=1 L=32', [32]),
    ('B=16 all of length 3', [3] * 16),
    ('B=17, the second tile lives one step', [4] * 16 + [1]),
    ('batch sizes 65 64 63 49 48 17 16 15 1', _lens_of_batch_sizes([65, 64, 63, 49, 48, 17, 16, 15, 1])),
]


def _four_problems(h):
    """(W0, A), (W1, A), (W0, B), (W1, B): layout A with L = 32 (21 sequences, h_last of B + 3 rows), layout B with L = 1
    (37 sequences, h_last of B rows); the two W_hh are shared."""
    lens_a = [32] * 3 + [31, 20, 17, 17, 16, 9, 9, 8, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1]
    la, lb = _with_off(G.case(h, lens_a, seed=31)), _with_off(G.case(h, [1] * 37, seed=32))
    w1 = G.case(h, [1], seed=33)
    probs = []
    for lay, extra, seed in ((la, 3, 34), (lb, 0, 35)):
        for ws in (la, w1):
            fresh = G.case(h, lay['lens'], seed=seed + len(probs))
            probs.append(dict(lay, w=ws['w'], b=ws['b'], gi=fresh['gi'], dh=fresh['dh'],
                              out_rows=len(lay['lens']) + extra))
    return probs


@pytest.mark.parametrize('route,h', ROUTE_H)
def test_step_statements_at_the_layout_edges(dev, route, h, monkeypatch):
    """L = 1 and L = 32 (MAXL), B = 1, the 16-sequence tile (16 / 17), the 64-row tile of the step kernels (63 / 64 / 65),
    equal lengths, a tile that dies after the first step, and ONE call of four problems over two layouts with two shared
    W_hh: every forward and backward statement, exactly S rows of saved / dGi / dGh written, sentinels intact, h_last
    padding exactly 0, and a second call bit-identical."""
    suffix, stmt = _select(route, monkeypatch)
    for name, lens in EDGE_LAYOUTS:
        p = _with_off(G.case(h, lens, seed=len(lens) + 7))
        p['out_rows'] = len(lens) + (3 if len(lens) in (16, 65) else 0)
        worst, _ = _run_and_check(dev, suffix, stmt, h, [p], '%s H=%d %s' % (route, h, name))
        _show('%s H=%d %s' % (route, h, name), worst)
    worst, _ = _run_and_check(dev, suffix, stmt, h, _four_problems(h), '%s H=%d four problems' % (route, h))
    _show('%s H=%d 4 problems, layouts L=32 / L=1' % (route, h), worst)


@pytest.mark.parametrize('route', ['persistent', 'steps', 'f32', 'bf16'])
def test_host_refusals_come_before_any_launch(dev, route, monkeypatch):
    """L = 33, an increasing batch size, out_rows < B and three distinct layouts are RENET_ERR_BADARG, a short workspace is
    RENET_ERR_WORKSPACE -- and no output element is touched."""
    import renet_hip as K
    suffix, _ = _select(route, monkeypatch)
    h = 100
    p = _with_off(G.case(h, [3, 3, 2, 1, 1]))
    c = Call(dev, h, [p])
    _, _, sv_ok = c.forward(suffix)

    def refused(rc, outs, code, what):
        assert rc == code, (what, rc)
        for t, rows in outs:
            _check_guard(t, rows, what, written=False)

    def both(code, what, fwd=True, **kw):
        rows = kw.pop('rows', None)
        if fwd:
            rc, hl, sv = c.forward(suffix, rows=rows, **kw)
            refused(rc, [(hl[0], c.rows[0]), (sv[0], c.s[0])], code, what + ' forward')
        if rows is None:
            rc, dgi, dgh = c.backward(suffix, sv_ok, **kw)
            refused(rc, [(dgi[0], c.s[0]), (dgh[0], c.s[0])], code, what + ' backward')

    long_off = (ctypes.c_int32 * 34)(*range(0, 34))
    both(-1, 'L = 33', offs=[long_off], ls=[33])
    both(-1, 'increasing batch size', offs=[(ctypes.c_int32 * 4)(0, 2, 5, 6)])
    both(-1, 'out_rows < B', rows=[4])
    # one aligned unit less than the route needs (the step kernels keep their state behind the planes; the exact-fp32
    # forward needs no workspace)
    need = K.lib().renet_gru_workspace(5 if route == 'steps' else 0, h)
    both(-3, 'short workspace', fwd=route != 'f32', ws_bytes=need - 256)
    three = [_with_off(G.case(h, [2, 1], seed=s)) for s in (1, 2, 3)]
    c3 = Call(dev, h, three)
    rc, hl, sv = c3.forward(suffix)
    refused(rc, [(hl[k], 2) for k in range(3)] + [(sv[k], 3) for k in range(3)], -1, 'three layouts forward')
    rc, dgi, dgh = c3.backward(suffix, [t[:3] for t in sv])
    refused(rc, [(dgi[k], 3) for k in range(3)], -1, 'three layouts backward')


# ---------------------------------------------------------------------------------------------
# 2. rotation census
# ---------------------------------------------------------------------------------------------
def _rotation(h, direction, rot_id, rot_mod=0):
    """rot_id -> (rot_k, rot_u): where a persistent workgroup starts in the cyclic W stream.
    forward : gru_planes.hip, gru_fwd_bf_kernel lines 91-95 (H > 200 and the one-plane mode) and gru_fwd_x_kernel lines
              320-321 (six pairs, H <= 200): rot_k = rot_id % KG, rot_u = (rot_id / KG) % NUB, rot_u = 0 for H > 200
    backward: gru_bwd_bf_kernel lines 482-486: rmod = RENET_GRU_ROT (capped at KG3) or 6 for H > 200 or KG3,
              rot_k = (rot_id % rmod) * (KG3 / rmod), rot_u = (rot_id / KG3) % NUB, 0 for H > 200"""
    nub, kg, kg3 = -(-h // 16), -(-h // 32), -(-3 * h // 32)
    if direction == 'fwd':
        return rot_id % kg, ((rot_id // kg) % nub if h <= 200 else 0)
    rmod = min(rot_mod, kg3) if rot_mod > 0 else (6 if h > 200 else kg3)
    return (rot_id % rmod) * (kg3 // rmod), ((rot_id // kg3) % nub if h <= 200 else 0)


def _full_rotation_set(h, direction, rot_mod=0):
    nub, kg, kg3 = -(-h // 16), -(-h // 32), -(-3 * h // 32)
    us = range(nub) if h <= 200 else [0]
    if direction == 'fwd':
        return {(k, u) for k in range(kg) for u in us}
    rmod = min(rot_mod, kg3) if rot_mod > 0 else (6 if h > 200 else kg3)
    return {(i * (kg3 // rmod), u) for i in range(rmod) for u in us}


CENSUS_B = {200: (2912, 7904), 100: (896, 2240), 300: (320, 320), 400: (416, 416)}    # per-problem batch: forward, backward


def _census(dev, suffix, stmt, h, direction, what, rot_mod=0):
    """Four problems over two layouts, L = 2.  At step 0 the state (forward) is 0 and the backward product runs only for
    steps > 0, so a workgroup exercises its W stream only if one of its sequences is alive at the second step: all but the
    last few are (layout A: the last 5 end after one step; layout B: the last 19 -- its last tile lives one step)."""
    nb = CENSUS_B[h][0 if direction == 'fwd' else 1]
    la = _with_off(G.case(h, [2] * (nb - 5) + [1] * 5, seed=41, wscale=0.3))
    lb = _with_off(G.case(h, [2] * (nb - 19) + [1] * 19, seed=42, wscale=0.3))
    probs = [la, dict(la, w=lb['w'], b=lb['b']), dict(lb, w=la['w'], b=la['b']), lb]
    # a condition of the test: the working workgroups (every blockIdx.x here, both layouts have nb rows) start at every
    # (rot_k, rot_u) the kernel can take
    gridx = -(-nb // 16)
    ids = sorted({(bx + gridx * by) >> 3 for by in range(4) for bx in range(gridx)})
    seen = {_rotation(h, direction, i, rot_mod) for i in ids}
    assert seen == _full_rotation_set(h, direction, rot_mod), (h, direction, len(seen))

    def describe(k, name, row):
        off = probs[k]['off']
        i = row - (off[1] if row >= off[1] else 0)
        rot = _rotation(h, direction, ((i // 16) + gridx * k) >> 3, rot_mod)
        return 'problem %d sequence %d: workgroup (%d, %d) with rot_k %d, rot_u %d' % (k, i, i // 16, k, rot[0], rot[1])

    worst, _ = _run_and_check(dev, suffix, stmt, h, probs, what, fwd=direction == 'fwd', bwd=direction == 'bwd',
                              twice=False, describe=describe)
    _show('%s: %d rotations' % (what, len(seen)), worst)


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
@pytest.mark.parametrize('mode,h', [('persistent', 100), ('persistent', 200), ('persistent', 300), ('persistent', 400),
                                    ('bf16', 100), ('bf16', 200)])
def test_rotation_census(dev, mode, h, direction, monkeypatch):
    """every starting position of the W stream of the persistent kernels -- every (rot_k, rot_u) pair for H <= 200, every
    rot_k beyond -- in one launch, the step statements on all rows; a failure names the workgroup's rotation.
    (RENET_GRU_ROT, read once per process, is honoured: the child runs of the next test come through here.)"""
    suffix, stmt = _select(mode, monkeypatch)
    rot_mod = int(os.environ.get('RENET_GRU_ROT', '0'))
    _census(dev, suffix, stmt, h, direction, 'census %s H=%d %s ROT=%d' % (mode, h, direction, rot_mod), rot_mod)


@pytest.mark.parametrize('rot', [1, 3])
def test_rotation_census_under_renet_gru_rot(dev, rot):
    """RENET_GRU_ROT = 1 and 3 (the number of distinct starting k groups of the backward stream; read once per process): the
    H = 200 backward census in a child process."""
    env = dict(os.environ, RENET_GRU_ROT=str(rot))
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-s', '-m', 'gpu', '-x', '-k',
                        'test_rotation_census and persistent-200-bwd'], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '1 passed' in r.stdout and 'ROT=%d' % rot in r.stdout, r.stdout[-2000:]
    print('\n' + '\n'.join(l for l in r.stdout.splitlines() if l.startswith('census')))


# ---------------------------------------------------------------------------------------------
# 3. term-pair census: single products
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route,h', ROUTE_H)
def test_single_products_expose_every_term_pair(dev, route, h, monkeypatch):
    """b_hh = 0 and, at step 0, gi_n = 0 except at unit k0 = row mod H: tanhf(0) = 0, so h_1 = (1 - z) n is exactly one-hot
    with an arbitrary full-width float at k0, and at step 1 hn[u] = h_1[k0] W_n[u][k0] is ONE product of two full-width
    floats.  Six pairs: within 2^-22 of the float64 product (the split drops < 2^-25, five additions of which only the last
    rounds at the full magnitude; the host emulation reaches 1.6 * 2^-24); a missing small pair leaves that bound in 85 % of
    the elements, any other in all of them (asserted here on the kernel's own operands: a condition of the test).  The
    exact-fp32 kernels get 2^-23, the one-plane mode 2^-7."""
    suffix, stmt = _select(route, monkeypatch)
    nb = h + 3
    rng = np.random.RandomState(51)
    p = _with_off(G.case(h, [2] * nb, seed=52, wscale=1.0))
    p['b'] = np.zeros(3 * h, np.float32)
    k0 = np.arange(nb) % h
    p['gi'][:nb, 2 * h:] = 0
    p['gi'][np.arange(nb), 2 * h + k0] = (1.5 * rng.randn(nb)).astype(np.float32)
    c = Call(dev, h, [p])
    rc, hl, sv = c.forward(suffix)
    assert rc == 0
    _check_guard(sv[0], c.s[0], 'saved')
    sv = sv[0][:c.s[0]].cpu().numpy()
    hp1, hn1 = sv[nb:, 4 * h:], sv[nb:, 3 * h:4 * h]
    a = hp1[np.arange(nb), k0]
    rest = hp1.copy()
    rest[np.arange(nb), k0] = 0
    assert np.all(rest == 0) and np.all(np.abs(a) > 1e-6), 'h_1 is not one-hot'
    wn = p['w'][2 * h:]                                  # [u, k]
    b_ = wn[:, k0].T                                     # [row, u] = W_n[u][k0(row)]
    if stmt == 'bf16x6':
        for drop in G.PAIRS6:
            frac = float(np.mean(G.product_ratio(G.product_planes(a[:, None], b_, drop=drop), a[:, None], b_, stmt) > 1.0))
            assert frac >= 0.5, (drop, frac)
    q = G.product_ratio(hn1, a[:, None], b_, stmt)
    _show('single products %s H=%d (bound 2^%d)' % (route, h, round(np.log2(G.PRODUCT_BOUND[stmt]))), {'hn': float(q.max())})
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    assert q.max() <= 1.0, 'row %d unit %d: error / bound = %.3g (%d of %d products over)' % (i[0], i[1], q.max(),
                                                                                             int((q > 1).sum()), q.size)


@pytest.mark.parametrize('route,h', ROUTE_H)
def test_single_products_of_the_backward_recurrence(dev, route, h, monkeypatch):
    """G.backward_product_case: saved (an input of the backward entry) with r = 1, z = 0 at the last step and a one-hot
    dh_last, so dh_prev[v] = dGh_n[k0] W_hh[2H + k0][v] is ONE product, and z = n = 0 at step 0, so dGi_n of step 0 is that
    product unchanged.  Six pairs: within 2^-21 (a missing pair leaves it in more than half of the elements: asserted on
    the kernel's own operands); exact fp32: 2^-23; one plane: 2^-7.  The step statements hold as well."""
    suffix, stmt = _select(route, monkeypatch)
    p = _with_off(G.backward_product_case(h))
    c = Call(dev, h, [p])
    sv = _guarded(c.s[0], 5 * h, dev)
    sv[:c.s[0]] = torch.from_numpy(p['saved']).to(dev)
    rc, dgi, dgh = c.backward(suffix, [sv])
    assert rc == 0
    _check_guard(dgi[0], c.s[0], 'dGi')
    _check_guard(dgh[0], c.s[0], 'dGh')
    d_gi, d_gh = dgi[0][:c.s[0]].cpu().numpy(), dgh[0][:c.s[0]].cpu().numpy()
    G.assert_holds(G.backward_ratios(stmt, p['dh'], p['off'], p['w'], p['saved'], d_gi, d_gh), 'backward products')
    got, a, b_ = G.backward_product_operands(p, d_gi, d_gh)
    if stmt == 'bf16x6':
        for drop in G.PAIRS6:
            frac = float(np.mean(G.product_ratio(G.product_planes(a, b_, drop=drop), a, b_, stmt, G.PRODUCT_BOUND_BWD) > 1.0))
            assert frac >= 0.5, (drop, frac)
    q = G.product_ratio(got, a, b_, stmt, G.PRODUCT_BOUND_BWD)
    _show('single products backward %s H=%d (bound 2^%d)' % (route, h, round(np.log2(G.PRODUCT_BOUND_BWD[stmt]))),
          {'dGi_n': float(q.max())})
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    assert q.max() <= 1.0, 'row %d unit %d: error / bound = %.3g (%d of %d products over)' % (i[0], i[1], q.max(),
                                                                                             int((q > 1).sum()), q.size)


# ---------------------------------------------------------------------------------------------
# 4. saturated gates
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route,h', ROUTE_H)
def test_saturated_gates(dev, route, h, monkeypatch):
    """gi of +-30 and +-1e4 in each gate and b_hh of +-20 (1 / (1 + __expf(-x)) with __expf overflowing to inf or vanishing):
    everything finite, every statement holds, the derivatives through a gate that is saturated in fp32 are exactly 0."""
    suffix, stmt = _select(route, monkeypatch)
    p = _with_off(G.saturated_case(h))
    worst, (hl, sv, dgi, dgh) = _run_and_check(dev, suffix, stmt, h, [p], 'saturated %s H=%d' % (route, h))
    _show('saturated %s H=%d' % (route, h), worst)
    s = p['off'][-1]
    for t in (hl[0][:len(p['lens'])], sv[0][:s], dgi[0][:s], dgh[0][:s]):
        assert bool(torch.isfinite(t).all())
    G.assert_saturated_derivatives_vanish(sv[0][:s].cpu().numpy(), dgi[0][:s].cpu().numpy(), dgh[0][:s].cpu().numpy())


# ---------------------------------------------------------------------------------------------
# 5. bf16 outputs of the one-plane backward
# ---------------------------------------------------------------------------------------------
def _bf16_to_f32(t16):
    return (t16.to(torch.int32) << 16).view(torch.float32)


@pytest.mark.parametrize('h', [100, 200, 400])
def test_bf16out_writes_its_logical_block_and_nothing_else(dev, h, monkeypatch):
    """renet_gru_bwd_layouts_bf16out into NaN-prefilled matrices of the operand row stride (3H rounded up to 256) and of a
    second one: the block [S, 3H] holds the statement's values within the one-plane bound and one RNE rounding, nothing
    outside it is written by the recurrence; renet_bf16_zero_padding zeroes the padding a consumer may read (columns
    up to the next multiple of 64 of the valid rows, rows up to the next multiple of 64) and nothing else."""
    import renet_hip as K
    suffix, stmt = _select('bf16', monkeypatch)
    probs = _four_problems(h)
    c = Call(dev, h, probs)
    rc, hl, sv = c.forward(suffix)
    assert rc == 0
    worst = {}
    for ld in ((3 * h + 255) & ~255, ((3 * h + 255) & ~255) + 24):
        rc, dgi, dgh = c.backward(suffix, sv, out_ld=ld)
        assert rc == 0, rc
        for k, p in enumerate(probs):
            s = c.s[k]
            for t in (dgi[k], dgh[k]):
                assert bool((t[:s, 3 * h:] == PATTERN16).all()) and bool((t[s:] == PATTERN16).all()), 'written outside [S, 3H]'
            r = G.backward_ratios(stmt, p['dh'], p['off'], p['w'], sv[k][:s].cpu().numpy(),
                                  _bf16_to_f32(dgi[k][:s, :3 * h].contiguous()).cpu().numpy(),
                                  _bf16_to_f32(dgh[k][:s, :3 * h].contiguous()).cpu().numpy(), out16=True)
            G.assert_holds(r, 'bf16out H=%d ld=%d problem %d' % (h, ld, k))
            for name, v in G.worst(r).items():
                worst[name] = max(worst.get(name, 0.0), v)
    _show('bf16out H=%d' % h, worst)
    rows, cols = 37, 3 * h
    m = K.bf16_empty(rows, cols, dev)
    m.p.view(torch.int16).fill_(PATTERN16)
    assert K.lib().renet_bf16_zero_padding(m.p.data_ptr(), rows, cols, m.p.shape[1], m.p.shape[0], K._stream()) == 0
    torch.cuda.synchronize()
    got = m.p.view(torch.int16).cpu().numpy()
    want = np.full(got.shape, PATTERN16, np.int16)
    want[:rows, cols:(cols + 63) & ~63] = 0
    want[rows:(rows + 63) & ~63] = 0
    assert np.array_equal(got, want)


def test_bf16out_is_refused_at_300_and_below_its_row_stride(dev, monkeypatch):
    suffix, _ = _select('persistent', monkeypatch)
    c = Call(dev, 300, [_with_off(G.case(300, [2, 1]))])
    rc, _, sv = c.forward(suffix)
    assert rc == 0
    rc, dgi, dgh = c.backward('', sv, out_ld=1024)
    assert rc == -2 and bool((dgi[0] == PATTERN16).all()) and bool((dgh[0] == PATTERN16).all())
    c = Call(dev, 100, [_with_off(G.case(100, [2, 1]))])
    rc, _, sv = c.forward('_bf16')
    rc, dgi, dgh = c.backward('', sv, out_ld=299)
    assert rc == -1 and bool((dgi[0] == PATTERN16).all())

