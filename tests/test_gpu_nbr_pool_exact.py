"""GPU tests of the neighbour pool kernels (csrc/nbr_pool.hip: renet_nbr_pool_fwd / renet_nbr_pool_bwd) through the C ABI
against the host statement of tests/nbr_pool_statement.py: BIT FOR BIT (or within the stated 2u of a quotient) on the exact
designs, and within the derived bounds at every element on float operands -- on ONE census batch whose 35 segments put every
length at which the kernels take another path at a chosen slot of a workgroup (tests/test_nbr_pool_statement_cpu.py asserts
that it does, and that every planted fault is caught), D in {100, 200, 300, 400}.  The test owns the buffers: every result has
three NaN guard rows (entries) behind it that must still be NaN after every call, and every result is NaN before the call.

Every bounded test prints its worst error / bound per check (pytest -s); the measured values are in
profiles/nbr_pool_statement.md."""
import ctypes

import numpy as np
import pytest
import torch

import nbr_pool_statement as NS

pytestmark = pytest.mark.gpu
WIDTHS = (100, 200, 300, 400)
GUARD = 3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


class Pool(object):
    """The two entries on buffers the test owns."""

    def __init__(self, dev):
        import renet_hip as K
        self.dev, self.K, self.L = dev, K, K.lib()

    def to(self, a):
        return None if a is None else torch.from_numpy(np.array(a)).to(self.dev)

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()

    def guarded(self, *shape):
        """a NaN buffer with GUARD more rows (entries) than `shape` asks for"""
        return torch.full((shape[0] + GUARD,) + tuple(shape[1:]), float('nan'), device=self.dev, dtype=torch.float32)

    @staticmethod
    def take(buf, what):
        a = buf.cpu().numpy()
        assert np.isnan(a[-GUARD:]).all(), '%s: the guard rows behind it were written' % what
        return a[:-GUARD]

    def index(self, b):
        host = np.ascontiguousarray(b.seg_ptr, np.int32)
        dev = {f: self.to(getattr(b, f)) for f in ('nbr', 'seg_ptr', 'seg_s', 'seg_r', 'seg_q', 'out_row')}
        return host, dev

    def forward(self, E, R, P, q, v, b, attn):
        """-> out [S, parts * D] and, in attention mode, w [nnz], stats [S, 2]"""
        d = E.shape[1]
        host, ix = self.index(b)
        t = [self.to(a) if attn or k == 0 else None for k, a in enumerate((E, R, P, q, v))]
        out = self.guarded(b.S, (3 if attn else 2) * d)
        stats, w = (self.guarded(b.S, 2), self.guarded(b.nnz)) if attn else (None, None)
        p = self.ptr
        rc = self.L.renet_nbr_pool_fwd(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(ix['nbr']), p(ix['seg_ptr']),
                                       host.ctypes.data_as(ctypes.c_void_p), p(ix['seg_s']), p(ix['seg_r']) if attn else None,
                                       p(ix['seg_q']) if attn else None, p(ix['out_row']), b.S, d, int(attn), p(out), p(stats),
                                       p(w), self.K._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        if not attn:
            return self.take(out, 'out')
        return self.take(out, 'out'), self.take(w, 'w'), self.take(stats, 'stats')

    def backward(self, dOut, out, E, P, q, v, w, b, attn):
        """-> dict of cE, ds_rows and, in attention mode, cP, dq_rows, dv_rows, dr_rows"""
        d = dOut.shape[1] // (3 if attn else 2)
        host, ix = self.index(b)
        t = [self.to(np.ascontiguousarray(a)) if a is not None else None for a in (dOut, out, E, P, q, v, w)]
        names = ('cE', 'cP', 'dq_rows', 'dv_rows', 'ds_rows', 'dr_rows')
        res = {f: self.guarded(b.nnz if f in ('cE', 'cP') else b.S, d)
               for f in names if attn or f in ('cE', 'ds_rows')}
        p = self.ptr
        rc = self.L.renet_nbr_pool_bwd(*[p(a) for a in t], p(ix['nbr']), p(ix['seg_ptr']),
                                       host.ctypes.data_as(ctypes.c_void_p), p(ix['seg_q']) if attn else None,
                                       p(ix['out_row']), b.S, d, int(attn), *[p(res.get(f)) for f in names], self.K._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return {f: self.take(a, f) for f, a in res.items()}


_POOL = []


@pytest.fixture(scope='module')
def pool(dev):
    if not _POOL:
        _POOL.append(Pool(dev))
    return _POOL[0]


def _report(tag, verdict):
    print('nbr-pool-bound %s %s' % (tag, ' | '.join('%s=%.3g' % kv for kv in verdict.items())))
    return NS.assert_verdict(verdict, tag)


# ---------------------------------------------------------------------------------------------
# 1, 2: the mean mode on integers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', WIDTHS)
def test_mean_forward_on_integers(pool, d):
    """out == S / n: bit for bit at power-of-two n, within 2u elsewhere (S the exact integer row sum); E[s] bit for bit."""
    op = NS.int_operands(d)
    b = op.batch
    out = pool.forward(op.E, None, None, None, None, b, False)
    fw = NS.forward(op.E, None, None, None, None, b, False)
    _report('mean forward integers D=%d' % d,
            {'out == S / n': NS.quotient_ratio(NS.pooled_of(out, b, d), fw.pooled * fw.n[:, None], fw.n),
             'copied E[s] block': NS.copied_blocks(out, op.E, None, b, False)})
    # and the derived bound on float operands
    o = NS.float_operands(d, 'plain')
    out = pool.forward(o.E, None, None, None, None, b, False)
    _report('mean forward float D=%d' % d,
            NS.check_mean_forward(NS.forward(o.E, None, None, None, None, b, False), out, o.E, b))


@pytest.mark.parametrize('d', WIDTHS)
def test_mean_backward_on_integers(pool, d):
    """ds_rows an exact copy; all rows cE[k] of a segment the same bits: g / n bit for bit at power-of-two n, within 2u."""
    for op in (NS.int_operands(d), NS.float_operands(d, 'plain')):
        b = NS.census()
        dOut = np.ascontiguousarray(op.dOut[:, :2 * d])
        got = pool.backward(dOut, None, None, None, None, None, None, b, False)
        bw = NS.backward(dOut, None, op.E, None, None, None, None, b, False)
        _report('mean backward %s D=%d' % (op.kind, d), NS.check_mean_backward(bw, got, b))


# ---------------------------------------------------------------------------------------------
# 3, 4: the exact attention designs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', WIDTHS)
def test_attention_uniform(pool, d):
    """Every row of P the same: w[k] == float32(1 / n) bit for bit, out == S / n."""
    o = NS.uniform(d)
    out, w, stats = pool.forward(o.E, o.R, o.P, o.q, o.v, o.batch, True)
    _report('uniform D=%d' % d, NS.check_exact_forward(o, out, w, stats))


@pytest.mark.parametrize('pattern', NS.PATTERNS)
@pytest.mark.parametrize('d', WIDTHS)
def test_attention_hot_cold(pool, d, pattern):
    """Scores exactly +-64: w == float32(1 / h) on hot neighbours and 0 on cold ones, out == S_hot / h, stats == (64, log h);
    the premise (stats0 == 64.0 bitwise) is asserted before anything else."""
    for cstar in (d - 1, 0):
        o = NS.hot_cold(d, pattern, cstar)
        out, w, stats = pool.forward(o.E, o.R, o.P, o.q, o.v, o.batch, True)
        _report('hot_cold %s c*=%d D=%d' % (pattern, cstar, d), NS.check_exact_forward(o, out, w, stats))


# ---------------------------------------------------------------------------------------------
# 5: the attention forward on float operands
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', NS.FLOAT_KINDS)
@pytest.mark.parametrize('d', WIDTHS)
def test_attention_forward_on_floats(pool, d, kind):
    """w, stats against float64; out and sum w against the kernel's own w; n = 1 and the copied blocks bit for bit."""
    o = NS.float_operands(d, kind)
    out, w, stats = pool.forward(o.E, o.R, o.P, o.q, o.v, o.batch, True)
    fw = NS.forward(o.E, o.R, o.P, o.q, o.v, o.batch, True)
    _report('attention forward %s D=%d' % (kind, d), NS.check_attn_forward(fw, out, w, stats, o.E, o.R, o.batch))


# ---------------------------------------------------------------------------------------------
# 6, 7: the attention backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('t0', 'pm30'))
@pytest.mark.parametrize('d', WIDTHS)
def test_attention_backward_exact_designs(pool, d, kind):
    """Small integers, w in {1, 1/2, 1/4} that is no softmax: every result value-equal to float64."""
    o = NS.bwd_exact(d, kind)
    got = pool.backward(o.dOut, o.out, o.E, o.P, o.q, o.v, o.w, o.batch, True)
    bw = NS.backward(o.dOut, o.out, o.E, o.P, o.q, o.v, o.w, o.batch, True)
    _report('attention backward %s D=%d' % (kind, d),
            NS.check_attn_backward(bw, got, o.dOut, o.w, o.batch, exact_design=True))


@pytest.mark.parametrize('kind', NS.FLOAT_KINDS)
@pytest.mark.parametrize('d', WIDTHS)
def test_attention_backward_on_floats(pool, d, kind):
    """Fed the forward's own w and out (the statement takes them as inputs: no forward error enters), and once more with a w
    that does not sum to 1."""
    o = NS.float_operands(d, kind)
    b = o.batch
    out, w, _ = pool.forward(o.E, o.R, o.P, o.q, o.v, b, True)
    runs = [('own w', w)]
    if kind == 'plain':
        rng = np.random.RandomState(d)
        runs.append(('w that does not sum to 1', (w * rng.uniform(0.5, 1.5, b.nnz)).astype(np.float32)))
    for tag, ww in runs:
        got = pool.backward(o.dOut, out, o.E, o.P, o.q, o.v, ww, b, True)
        bw = NS.backward(o.dOut, out, o.E, o.P, o.q, o.v, ww, b, True)
        _report('attention backward %s D=%d, %s' % (kind, d, tag), NS.check_attn_backward(bw, got, o.dOut, ww, b))


# ---------------------------------------------------------------------------------------------
# 8: run-to-run bit identity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', WIDTHS)
def test_two_calls_give_equal_bits(pool, d):
    o = NS.float_operands(d, 'ascending')
    b = o.batch
    first = pool.forward(o.E, o.R, o.P, o.q, o.v, b, True)
    again = pool.forward(o.E, o.R, o.P, o.q, o.v, b, True)
    for name, x, y in zip(('out', 'w', 'stats'), first, again):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    out, w, _ = first
    g1 = pool.backward(o.dOut, out, o.E, o.P, o.q, o.v, w, b, True)
    g2 = pool.backward(o.dOut, out, o.E, o.P, o.q, o.v, w, b, True)
    for name in g1:
        assert np.array_equal(g1[name].view(np.uint32), g2[name].view(np.uint32)), name
    m1 = pool.forward(o.E, None, None, None, None, b, False)
    m2 = pool.forward(o.E, None, None, None, None, b, False)
    assert np.array_equal(m1.view(np.uint32), m2.view(np.uint32))
