"""Host tests of tests/nbr_pool_statement.py (no GPU): the census batch has every property it promises; the integer and exact
designs keep their premises; two float32 emulations of the C ABI in different orders (a two-pass softmax with serial sums, and
the online batches of four with the four-range split) stay inside every derived bound on the three float kinds; and the checks
have teeth -- every planted fault breaks an exact design or exceeds a bound on the census, and the test names the check that
caught it.  This file is the evidence that tests/test_gpu_nbr_pool_exact.py would fail on a subtly wrong kernel.

Measured here (worst error / bound of the emulations over D = 100 and 400 and the three kinds): see
profiles/nbr_pool_statement.md."""
import numpy as np
import pytest

import nbr_pool_statement as NS

WIDTHS = (100, 400)


# ---------------------------------------------------------------------------------------------
# conditions of the GPU tests
# ---------------------------------------------------------------------------------------------
def test_census_has_the_designed_segments():
    f = NS.census_facts()
    b = NS.census()
    assert f['S'] == 35 and f['nnz'] == 7477 and f['S_mod_waves'] == 3
    assert f['workgroups'] == [(1, 2, 3, 4), (5, 8, 9, 63), (64, 65, 128, 129), (255, 256, 7, 16), (257, 1, 1, 1),
                               (2, 260, 3, 261), (258, 259, 512, 1025), (1000, 1023, 1024, 300), (12, 6, 257)]
    assert f['longest'] == 1025 and f['ranges_of_257'] == [65, 65, 65, 62]
    for name, value in f.items():
        if isinstance(value, (bool, np.bool_)):
            assert value, name
    assert len(b.nbr) == b.nnz == b.seg_ptr[-1] and len(b.seg_ptr) == b.S + 1 and b.seg_ptr[0] == 0
    for a in (b.nbr, b.seg_ptr, b.seg_s, b.seg_r, b.seg_q, b.out_row):
        assert a.dtype == np.int32 and not a.flags.writeable
    assert 0 <= b.nbr.min() and b.nbr.max() < NS.N_ENT and b.seg_q.max() < NS.N_Q and b.seg_r.max() < NS.N_REL


@pytest.mark.parametrize('pattern', NS.PATTERNS)
def test_hot_patterns_are_what_they_say(pattern):
    b = NS.census()
    n = NS.lengths(b)
    for u in range(b.S):
        pos = NS.hot_positions(int(n[u]), pattern)
        assert len(pos) >= 1 and len(set(pos)) == len(pos) and 0 <= min(pos) and max(pos) < n[u], (pattern, u)
        if n[u] > NS.SPLIT:
            rngs = NS.sub_ranges(int(n[u]))
            per = [sum(s <= p < e for p in pos) for s, e in rngs]
            if pattern == 'wave4':
                assert per[:3] == [0, 0, 0] and per[3] == rngs[3][1] - rngs[3][0]
            if pattern == 'one_per_wave':
                assert per == [1, 1, 1, 1]
            if pattern == 'last':
                assert per == [0, 0, 0, 1]
        if pattern == 'pos63_64' and n[u] > 64:
            assert pos == [63, 64]
        if pattern == 'pow2_spread':
            assert len(pos) & (len(pos) - 1) == 0 and len(pos) == min(16, 1 << (int(n[u]).bit_length() - 1))
    d = NS.hot_cold(100, pattern, 99)
    assert d.batch.nbr.min() == 0 and d.batch.nbr.max() == NS.N_ENT - 1
    hot_ids = (d.batch.nbr >= 1) & (d.batch.nbr <= NS.N_HOT_IDS)
    assert np.array_equal(hot_ids, d.hot) and (d.h >= 1).all()
    if pattern == 'last':                                      # a clamped tail batch wherever n is no multiple of 4
        assert (d.h == 1).all() and int((n % 4 != 0).sum()) >= 20


@pytest.mark.parametrize('d', (100, 200, 300, 400))
def test_integer_and_exact_designs_keep_their_premises(d):
    op = NS.int_operands(d)
    b = op.batch
    starts = b.seg_ptr[:-1].astype(np.int64)
    for a in (op.E, op.R, op.dOut, op.out):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() == 8
    assert NS.exactness_margin(np.add.reduceat(np.abs(NS.f64(op.E))[b.nbr], starts, axis=0)) > 1024     # neighbour sums
    # the premises of the attention designs, in this host's float32 arithmetic
    with np.errstate(under='ignore'):
        assert np.tanh(np.float32(30)) == 1 and np.tanh(np.float32(-30)) == -1
        assert np.exp(np.float32(0)) == 1 and np.exp(np.float32(-128)) == 0
    u = NS.uniform(d)
    assert (u.P == u.P[0]).all() and np.array_equal(u.num, np.round(u.num))
    for cstar in (0, d - 1):
        h = NS.hot_cold(d, 'one_per_wave', cstar)
        assert np.count_nonzero(h.v) == 1 and h.v[cstar] == 64 and (h.q[:, cstar] == 0).all()
        assert set(np.unique(h.P[:, cstar])) == {-30.0, 30.0}
        a = NS._scores64(h.P, h.q, h.v, h.batch)
        assert np.allclose(np.abs(a), 64.0, rtol=0, atol=1e-9) and np.array_equal(a > 0, h.hot)
    if d >= 300:
        assert (d - 1) // 4 >= 64                              # c* = D - 1 lies in a lane's second chunk
    # the backward designs
    for kind in ('t0', 'pm30'):
        o = NS.bwd_exact(d, kind)
        assert set(np.unique(o.w)) == {0.25, 0.5, 1.0} and set(np.unique(np.abs(o.v))) == {0.5, 1.0, 2.0}
        assert (o.v < 0).any() and (o.v > 0).any() and (o.q == 0).all()
        sums = np.add.reduceat(NS.f64(o.w), starts)
        assert np.abs(sums[NS.lengths(b) > 4] - 1).min() > 0.1   # no softmax
        m = NS.bwd_exact_margins(o)
        print('nbr-pool-premise D=%d design=%s margins %s' % (d, kind, ' '.join('%s=%.1f' % kv for kv in sorted(m.items()))))
        assert min(m.values()) > 2, m
        bw = NS.backward(o.dOut, o.out, o.E, o.P, o.q, o.v, o.w, b, True)
        for a, quantum in ((bw.cE, 4), (bw.cP, 8), (bw.dq_rows, 8), (bw.dv_rows, 4)):
            assert np.array_equal(a * quantum, np.round(a * quantum))
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
        if kind == 't0':
            assert (bw.dv_rows == 0).all() and np.array_equal(bw.cP, bw.da[:, None] * NS.f64(o.v)[None, :])
            assert np.count_nonzero(bw.dq_rows) > 0.9 * bw.dq_rows.size
        else:
            assert (bw.cP == 0).all() and (bw.dq_rows == 0).all() and np.count_nonzero(bw.dv_rows) > 0.9 * bw.dv_rows.size


@pytest.mark.parametrize('d', WIDTHS)
def test_float_kinds_are_what_they_say(d):
    spreads = {}
    for kind in NS.FLOAT_KINDS:
        o = NS.float_operands(d, kind)
        b = o.batch
        a = NS._scores64(o.P, o.q, o.v, b)
        fw = NS.forward(o.E, o.R, o.P, o.q, o.v, b, True)
        spreads[kind] = float(fw.spread.max())
        if kind == 'ascending':
            for u in range(b.S):
                assert (np.diff(a[b.seg_ptr[u]:b.seg_ptr[u + 1]]) >= 0).all()
            assert sorted(b.nbr.tolist()) == sorted(NS.census().nbr.tolist())
        if kind == 'large':
            assert 55 <= np.abs(a).max() <= 60
    assert 2 <= spreads['plain'] <= 4 and spreads['plain'] == pytest.approx(spreads['ascending']) and spreads['large'] > 60


# ---------------------------------------------------------------------------------------------
# two float32 emulations against every bound
# ---------------------------------------------------------------------------------------------
def _forward_verdict(o, order, fault=None):
    out, w, stats = NS.emulate_forward(o.E, o.R, o.P, o.q, o.v, o.batch, True, order, fault)
    fw = NS.forward(o.E, o.R, o.P, o.q, o.v, o.batch, True)
    return NS.check_attn_forward(fw, out, w, stats, o.E, o.R, o.batch), (out, w)


def _show(tag, verdict):
    print('nbr-pool-bound %s %s' % (tag, ' | '.join('%s=%.3g' % kv for kv in verdict.items())))


@pytest.mark.parametrize('order', ('twopass', 'online'))
@pytest.mark.parametrize('kind', NS.FLOAT_KINDS)
@pytest.mark.parametrize('d', WIDTHS)
def test_float32_emulations_stay_within_every_bound(d, kind, order):
    o = NS.float_operands(d, kind)
    b = o.batch
    v, (out, w) = _forward_verdict(o, order)
    _show('emulation=%s D=%d kind=%s attention forward:' % (order, d, kind), v)
    assert 0 < NS.assert_verdict(v, 'forward %s %s D=%d' % (order, kind, d)) <= 1
    # the backward on the emulation's own w and out, and on a w that is no softmax
    rng = np.random.RandomState(d)
    for tag, ww in (('own w', w), ('w that does not sum to 1', (w * rng.uniform(0.5, 1.5, b.nnz)).astype(np.float32))):
        got = NS.emulate_backward(o.dOut, out, o.E, o.P, o.q, o.v, ww, b, True, order)
        bw = NS.backward(o.dOut, out, o.E, o.P, o.q, o.v, ww, b, True)
        v = NS.check_attn_backward(bw, got, o.dOut, ww, b)
        _show('emulation=%s D=%d kind=%s attention backward, %s:' % (order, d, kind, tag), v)
        assert 0 < NS.assert_verdict(v, 'backward %s %s D=%d' % (order, kind, d)) <= 1
    if kind == 'plain':
        out = NS.emulate_forward(o.E, None, None, None, None, b, False, order)[0]
        v = NS.check_mean_forward(NS.forward(o.E, None, None, None, None, b, False), out, o.E, b)
        _show('emulation=%s D=%d mean forward:' % (order, d), v)
        assert 0 < NS.assert_verdict(v, 'mean forward') <= 1
        got = NS.emulate_backward(o.dOut[:, :2 * d], None, o.E, None, None, None, None, b, False, order)
        v = NS.check_mean_backward(NS.backward(o.dOut[:, :2 * d], None, o.E, None, None, None, None, b, False), got, b)
        NS.assert_verdict(v, 'mean backward')


@pytest.mark.parametrize('d', WIDTHS)
def test_online_emulation_meets_every_exact_design(d):
    designs = [NS.uniform(d)] + [NS.hot_cold(d, p, c) for p in NS.PATTERNS for c in ((0, d - 1) if d == 100 else (d - 1,))]
    for o in designs:
        out, w, stats = NS.emulate_forward(o.E, o.R, o.P, o.q, o.v, o.batch, True, 'online')
        NS.assert_verdict(NS.check_exact_forward(o, out, w, stats), '%s %s' % (o.kind, getattr(o, 'pattern', '')))
    op = NS.int_operands(d)
    b = op.batch
    for order in ('twopass', 'online'):
        out = NS.emulate_forward(op.E, None, None, None, None, b, False, order)[0]
        fw = NS.forward(op.E, None, None, None, None, b, False)
        assert NS.quotient_ratio(NS.pooled_of(out, b, d), fw.pooled * fw.n[:, None], fw.n) <= 1
        got = NS.emulate_backward(op.dOut[:, :2 * d], None, op.E, None, None, None, None, b, False, order)
        bw = NS.backward(op.dOut[:, :2 * d], None, op.E, None, None, None, None, b, False)
        NS.assert_verdict(NS.check_mean_backward(bw, got, b), 'mean backward %s' % order)
        for kind in ('t0', 'pm30'):
            o = NS.bwd_exact(d, kind)
            got = NS.emulate_backward(o.dOut, o.out, o.E, o.P, o.q, o.v, o.w, b, True, order)
            bw = NS.backward(o.dOut, o.out, o.E, o.P, o.q, o.v, o.w, b, True)
            NS.assert_verdict(NS.check_attn_backward(bw, got, o.dOut, o.w, b, exact_design=True), 'backward %s' % kind)


# ---------------------------------------------------------------------------------------------
# teeth: every planted fault is caught, by a named check
# ---------------------------------------------------------------------------------------------
# fault -> (design, the check that must catch it)
W_CHECK = 'w == float32(1/h) on hot neighbours, 0 on cold ones'
FWD_CAUGHT_BY = {
    'no_rescale': [(('hot_cold', 'last'), W_CHECK), (('float', 'ascending'), 'out against the own weights')],
    'tail_counted': [(('hot_cold', 'last'), W_CHECK), (('uniform',), W_CHECK), (('float', 'plain'), 'sum of the own weights')],
    'last_of_1025_dropped': [(('hot_cold', 'last'), NS.PREMISE), (('float', 'plain'), 'w')],
    'w_wave_local': [(('hot_cold', 'wave4'), W_CHECK), (('float', 'plain'), 'sum of the own weights'),
                     (('float', 'ascending'), 'w')],
    'merge_l_without_f': [(('hot_cold', 'wave4'), W_CHECK), (('float', 'ascending'), 'sum of the own weights')],
    'stale_merge_row': [(('hot_cold', 'one_per_wave'), 'out == S_hot / h'), (('float', 'plain'), 'out against the own weights')],
    'last_segment_skipped': [(('hot_cold', 'first'), NS.PREMISE), (('float', 'plain'), 'w')],
}


def _design(key, d):
    if key[0] == 'uniform':
        return NS.uniform(d)
    if key[0] == 'hot_cold':
        return NS.hot_cold(d, key[1], d - 1)
    return NS.float_operands(d, key[1])


@pytest.mark.parametrize('fault', NS.FWD_FAULTS)
def test_every_planted_forward_fault_is_caught(fault):
    d = 100
    assert set(FWD_CAUGHT_BY) == set(NS.FWD_FAULTS)
    for key, check in FWD_CAUGHT_BY[fault]:
        o = _design(key, d)
        if key[0] == 'float':
            sound, faulty = _forward_verdict(o, 'online')[0], _forward_verdict(o, 'online', fault)[0]
        else:
            sound = NS.check_exact_forward(o, *NS.emulate_forward(o.E, o.R, o.P, o.q, o.v, o.batch, True, 'online'))
            faulty = NS.check_exact_forward(o, *NS.emulate_forward(o.E, o.R, o.P, o.q, o.v, o.batch, True, 'online', fault))
        assert not NS.failed(sound), (key, NS.failed(sound))
        print('nbr-pool-teeth fault=%s design=%s caught by: %s' % (fault, '/'.join(key), '; '.join(NS.failed(faulty))))
        assert check in NS.failed(faulty), (fault, key, check, faulty)
        with pytest.raises(AssertionError):
            NS.assert_verdict(faulty)


@pytest.mark.parametrize('fault,kind,check', [('c0_zero', 't0', 'cP exact'), ('c0_zero', 'pm30', 'dv_rows exact'),
                                              ('dv_without_da', 'pm30', 'dv_rows exact'),
                                              ('c0_zero', 'plain', 'cP'), ('dv_without_da', 'plain', 'dv_rows')])
def test_every_planted_backward_fault_is_caught(fault, kind, check):
    d = 100
    assert fault in NS.BWD_FAULTS
    if kind == 'plain':
        o = NS.float_operands(d, kind)
        out, w, _ = NS.emulate_forward(o.E, o.R, o.P, o.q, o.v, o.batch, True, 'online')
    else:
        o = NS.bwd_exact(d, kind)
        out, w = o.out, o.w
    bw = NS.backward(o.dOut, out, o.E, o.P, o.q, o.v, w, o.batch, True)
    verdicts = []
    for f in (None, fault):
        got = NS.emulate_backward(o.dOut, out, o.E, o.P, o.q, o.v, w, o.batch, True, 'online', f)
        verdicts.append(NS.check_attn_backward(bw, got, o.dOut, w, o.batch, exact_design=kind != 'plain'))
    assert not NS.failed(verdicts[0]), NS.failed(verdicts[0])
    print('nbr-pool-teeth fault=%s design=%s caught by: %s' % (fault, kind, '; '.join(NS.failed(verdicts[1]))))
    assert check in NS.failed(verdicts[1]), verdicts[1]


def test_checks_catch_unwritten_rows_and_wrong_copies():
    o = NS.float_operands(100, 'plain')
    b = o.batch
    out, w, stats = NS.emulate_forward(o.E, o.R, o.P, o.q, o.v, b, True, 'online')
    fw = NS.forward(o.E, o.R, o.P, o.q, o.v, b, True)
    bad = out.copy()
    bad[b.out_row[7], 100:200] = o.E[(b.seg_s[7] + 1) % NS.N_ENT]          # the neighbouring entity's row as E[s]
    assert NS.failed(NS.check_attn_forward(fw, bad, w, stats, o.E, o.R, b)) == ['copied E[s] / R[r] blocks']
    bad = out.copy()
    bad[b.out_row[0], 5] = np.nextafter(bad[b.out_row[0], 5], np.float32(9))  # n = 1: one ulp off E[nbr]
    assert 'n = 1: out == E[nbr]' in NS.failed(NS.check_attn_forward(fw, bad, w, stats, o.E, o.R, b))
    bad = w.copy()
    bad[b.seg_ptr[20]] = np.nan
    f = NS.failed(NS.check_attn_forward(fw, out, bad, stats, o.E, o.R, b))
    assert 'w' in f and 'sum of the own weights' in f and 'out against the own weights' in f
