"""The deterministic reductions of the backward pass through their C entry points against the float64 statements of
tests/reduction_statements.py: the relation-weight gradient (csrc/rgcn_bwd.hip), the column sums and the device-scalar
scalings (csrc/gemm.hip), the operand-bound maxima (csrc/gemm_h3.hip), the segmented add (csrc/rows.hip) and the small
entries renet_compose_table_items, renet_add_inplace, renet_zero.

A mistake in these kernels is a dropped or doubled row, edge or chunk, which randn data under a loose tolerance can hide.
So every reduction runs on small INTEGER operands, where each partial sum of any order is exact in fp32 (the premise is
checked in tests/test_reduction_statements_cpu.py) and the result must equal the statement exactly, and on randn operands
within the derived bound gamma(n + 2) * sum |terms| (no bound is fitted to a kernel).  Outputs and workspaces are prefilled
with a quiet-NaN pattern, carry sentinel elements behind them, and workspaces have exactly the size the library asks for: an
element the kernel never wrote shows as NaN, a write behind the end in the sentinels.  Refused calls must leave every
buffer untouched.  Run with -s for the worst error / bound per kernel."""
import numpy as np
import pytest
import torch

import reduction_statements as R

pytestmark = pytest.mark.gpu

DS = [100, 200, 300, 400]
PATTERN = 0x7fc0dead                                    # a quiet NaN no kernel produces
PATTERN16 = 0x7fc1
SPARE = 2                                               # sentinel rows behind every matrix output
TAIL = 8                                                # sentinel elements behind every flat buffer


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _to(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def _nanbuf(n, dev, tail=TAIL):
    """n + tail int32 elements holding PATTERN; pass .data_ptr() as a float buffer of n elements"""
    return torch.full((n + tail,), PATTERN, dtype=torch.int32, device=dev)


def _nanrows(rows, cols, dev):
    return torch.full((rows + SPARE, cols), PATTERN, dtype=torch.int32, device=dev)


def _set(buf, values):
    """writes the float32 array `values` to the front of the PATTERN buffer (rows of a matrix, elements of a flat one)"""
    v = _to(np.ascontiguousarray(values, np.float32), buf.device).view(torch.int32)
    buf[:v.shape[0]] = v
    return buf


def _tail_intact(buf, n, what):
    assert bool((buf[n:] == PATTERN).all()), '%s: written behind its end' % what


def _untouched(buf, what):
    assert bool((buf == PATTERN).all()), '%s: written by a call that must not launch' % what


def _f32(buf, n):
    return buf[:n].cpu().numpy().view(np.float32)


def _assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, (what, got.shape, want.shape)
    view = {4: np.uint32, 2: np.uint16}[got.dtype.itemsize]
    bad = np.nonzero(got.view(view).reshape(-1) != want.view(view).reshape(-1))[0]
    assert bad.size == 0, '%s: %d of %d elements differ, first at flat index %d: got %r, want %r' % (
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _assert_exact(got, ref, what):
    """an integer-operand sum: equal to the statement exactly (a NaN -- an element never written, or a workspace slot read
    that was never written -- equals nothing; the sign of a zero is not part of the statement)"""
    want = np.asarray(ref, np.float64).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref), what + ': the statement is not representable'
    bad = np.nonzero(~(np.asarray(got) == want).reshape(-1))[0]
    assert bad.size == 0, '%s: %d of %d elements differ (%d NaN), first at flat index %d: got %r, want %r' % (
        what, bad.size, want.size, int(np.isnan(got).sum()), bad[0], np.asarray(got).reshape(-1)[bad[0]],
        want.reshape(-1)[bad[0]])


WORST = {}


def _within(got, ref, n, mag, kernel, what):
    q = R.ratio(got, ref, n, mag)
    w = float(q.max()) if q.size else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), w)
    i = np.unravel_index(int(np.argmax(q)), q.shape) if q.size else ()
    assert w <= 1.0, '%s: error / bound = %.3g at %s (%d of %d elements over)' % (what, w, i, int((q > 1).sum()), q.size)
    return w


def _show(kernel):
    print('\n  worst error / bound  %-28s %.3f' % (kernel, WORST.get(kernel, 0.0)))


# ---------------------------------------------------------------------------------------------
# 1. dW: renet_rgcn_bwd_w / renet_rgcn_bwd_w64
# ---------------------------------------------------------------------------------------------
ENTRIES = ['renet_rgcn_bwd_w', 'renet_rgcn_bwd_w64']
_lay_dev, _dw_sums = {}, {}


def _layout_on(dev):
    if 'census' not in _lay_dev:
        lay = R.census_layout()
        _lay_dev['census'] = {k: _to(lay[k], dev) for k in ('e_src', 'e_dst', 'chunk_ptr', 'chunk_type', 'type_chunk_ptr')}
    return _lay_dev['census']


def _dw_ref(d, kind, shift, beta):
    """the statement on the census layout; the per-type float64 sums are computed once per (D, kind) and shared"""
    x, gn, old = R.dw_operands(d, kind)
    if (d, kind) not in _dw_sums:
        _dw_sums[(d, kind)] = R.dw_type_sums(x, gn, R.census_layout())
    return R.dw_place(_dw_sums[(d, kind)], R.CENSUS_T, shift, beta, old)


def _dw_call(dev, entry, ld, x, gn, d, shift, beta, old=None, n_chunks=None, t_n=None, ws_short=0, d_arg=None):
    """-> rc, dW buffer [T + SPARE rows] (old or NaN in its T rows), workspace buffer, its size in floats"""
    import renet_hip as K
    t_n = R.CENSUS_T if t_n is None else t_n
    n_chunks = R.census_layout()['n_chunks'] if n_chunks is None else n_chunks
    w = d * (d // 100)
    dw = _nanrows(R.CENSUS_T, w, dev)
    if old is not None:
        _set(dw, old)
    need = K.lib().renet_rgcn_bwd_w_workspace(max(n_chunks, 0), d)
    assert need == max(n_chunks, 0) * w * 4
    ws = _nanbuf(need // 4, dev, tail=64)
    rc = getattr(K.lib(), entry)(x.data_ptr(), gn.data_ptr(), ld['e_src'].data_ptr(), ld['e_dst'].data_ptr(),
                                 ld['chunk_ptr'].data_ptr(), ld['chunk_type'].data_ptr(), n_chunks,
                                 ld['type_chunk_ptr'].data_ptr(), t_n, shift, d if d_arg is None else d_arg,
                                 dw.data_ptr(), beta, ws.data_ptr(), need - ws_short, K._stream())
    torch.cuda.synchronize()
    return rc, dw, ws, need // 4


def _dw_checked(dev, entry, ld, x, gn, d, shift, beta, old, what):
    rc, dw, ws, nws = _dw_call(dev, entry, ld, x, gn, d, shift, beta, old if beta != 0.0 else None)
    assert rc == 0, (what, rc)
    _tail_intact(ws, nws, what + ' workspace')
    assert bool((dw[R.CENSUS_T:] == PATTERN).all()), what + ': written behind the last type'
    return _f32(dw, R.CENSUS_T)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('d', DS)
def test_dw_census_layout_is_exact_on_integers(dev, d, entry):
    """the census layout (every c0 mod 8 and c1 mod 8, types of 0, 1, 2, 8, 9, 17 and 1197 chunks, chunks of 0 .. 150 edges)
    with x, gn in {-2..2}: dW equals the integer statement for every type, at type_shift 0, 1, T/2, T-1 and beta 0, 1, -0.5.
    The workspace is NaN-prefilled and exactly renet_rgcn_bwd_w_workspace bytes: a NaN in dW is a slot the reduce pass read
    and the partial pass never wrote; beta = 0 runs on a NaN-prefilled dW (overwrite, not accumulate)."""
    ld = _layout_on(dev)
    x, gn, old = R.dw_operands(d, 'int')
    xd, gd = _to(x, dev), _to(gn, dev)
    t_n = R.CENSUS_T
    for shift in (0, 1, t_n // 2, t_n - 1):
        for beta in R.BETAS:
            what = '%s D=%d shift=%d beta=%g' % (entry, d, shift, beta)
            got = _dw_checked(dev, entry, ld, xd, gd, d, shift, beta, old, what)
            ref, _, n_e = _dw_ref(d, 'int', shift, beta)
            for tau in range(t_n):
                _assert_exact(got[tau], ref[tau], '%s: dW[%d] (stored type %d, %d edges, census %s)' % (
                    what, tau, (tau - shift) % t_n, n_e[tau], R.CENSUS_TABLE[(tau - shift) % t_n]))


@pytest.mark.parametrize('d', DS)
def test_dw_census_layout_within_the_bound_on_randn(dev, d):
    """randn operands: every element within gamma(edges + 2) * sum |terms|; the 32-bit and the 64-bit addressing entries
    agree bit for bit, and so do two runs."""
    ld = _layout_on(dev)
    x, gn, old = R.dw_operands(d, 'randn')
    xd, gd = _to(x, dev), _to(gn, dev)
    for shift, beta in ((0, 0.0), (R.CENSUS_T // 2, 1.0), (1, -0.5)):
        what = 'dW D=%d shift=%d beta=%g' % (d, shift, beta)
        got = _dw_checked(dev, ENTRIES[0], ld, xd, gd, d, shift, beta, old, what)
        again = _dw_checked(dev, ENTRIES[0], ld, xd, gd, d, shift, beta, old, what)
        got64 = _dw_checked(dev, ENTRIES[1], ld, xd, gd, d, shift, beta, old, what)
        _assert_bits(again, got, what + ': a second run')
        _assert_bits(got64, got, what + ': renet_rgcn_bwd_w64 against renet_rgcn_bwd_w')
        ref, mag, n_e = _dw_ref(d, 'randn', shift, beta)
        _within(got, ref, n_e[:, None], mag, 'rgcn_bwd_w D=%d' % d, what)
    _show('rgcn_bwd_w D=%d' % d)


def _probe_edges():
    """(edge, stored type) of single edges at distinct places of the census layout"""
    lay = R.census_layout()
    tcp, cp = lay['type_chunk_ptr'], lay['chunk_ptr']
    picks = [(tcp[1], 63),                  # the first chunk, its last edge
             (tcp[8], 64), (tcp[8], 149),   # the 150-edge chunk: first edge of the second round, last of the third
             (tcp[6] + 3, 64),              # the 65-edge chunk of the 17-chunk type: the one edge of its second round
             (tcp[12] + 602, 0),            # inside the hot type, sixth of the 8 chunks of its workgroup
             (lay['n_chunks'] - 1, 0)]      # the last chunk: one edge
    out = []
    assert picks[4][0] % R.GROUP == 5
    for c, k in picks:
        assert k < cp[c + 1] - cp[c]
        out.append((int(cp[c] + k), int(lay['chunk_type'][c])))
    return out


@pytest.mark.parametrize('d', DS)
def test_dw_one_hot_probes(dev, d):
    """x and gn are zero but for ONE element of one row each, that row the source and destination of ONE edge: exactly one
    entry of dW is non-zero, dW[tau, b, i, j] = x[.., b si + i] gn[.., b si + j] -- a swapped i / j, a wrong block, a wrong
    type or the second half-row (D = 300 / 400) show as a misplaced entry.  Feature positions 0, 1, D/2 - 1, D/2, D - 2,
    D - 1 of x, every j of the block for gn."""
    ld = dict(_layout_on(dev))
    ld['e_src'], ld['e_dst'] = ld['e_src'].clone(), ld['e_dst'].clone()
    si, w, t_n, row = d // 100, d * (d // 100), R.CENSUS_T, R.CENSUS_ROWS
    x = torch.zeros(row + 1, d, device=dev)               # row CENSUS_ROWS: referenced by the probe edge only
    gn = torch.zeros(row + 1, d, device=dev)
    want = torch.zeros(t_n, w, device=dev)
    shift, n = 1, 0
    for e, t in _probe_edges():
        keep = (int(ld['e_src'][e]), int(ld['e_dst'][e]))
        ld['e_src'][e], ld['e_dst'][e] = row, row
        for p in (0, 1, d // 2 - 1, d // 2, d - 2, d - 1):
            b, i = p // si, p % si
            for j in range(si):
                x[row, p], gn[row, b * si + j] = 3.0, -5.0
                tau, col = (t + shift) % t_n, b * si * si + i * si + j
                want[tau, col] = -15.0
                for entry in ENTRIES:
                    rc, dw, ws, nws = _dw_call(dev, entry, ld, x, gn, d, shift, 0.0)
                    got = dw[:t_n].view(torch.float32)
                    if rc != 0 or not torch.equal(got, want):
                        nz = torch.nonzero(got != want).tolist()
                        raise AssertionError('%s D=%d edge %d (type %d), x at %d, gn at %d: rc %d, wanted only dW[%d, %d, '
                                             '%d, %d]; wrong at (type, flat entry) %s' % (entry, d, e, t, p, b * si + j, rc,
                                                                                         tau, b, i, j, nz[:4]))
                    _tail_intact(ws, nws, 'probe workspace')
                    n += 1
                x[row, p], gn[row, b * si + j], want[tau, col] = 0.0, 0.0, 0.0
        ld['e_src'][e], ld['e_dst'][e] = keep
    assert n == 6 * 6 * si * 2


@pytest.mark.parametrize('d', DS)
def test_dw_without_chunks_scales_the_old_gradient(dev, d):
    """n_chunks = 0, every type empty: dW = beta * dW exactly (beta = 0 over a NaN-prefilled dW gives zeros)"""
    ld = dict(_layout_on(dev), type_chunk_ptr=torch.zeros(R.CENSUS_T + 1, dtype=torch.int32, device=dev))
    x, gn, old = R.dw_operands(d, 'int')
    xd, gd = _to(x, dev), _to(gn, dev)
    for entry in ENTRIES:
        for beta in (0.0, 1.0):
            rc, dw, ws, nws = _dw_call(dev, entry, ld, xd, gd, d, 0, beta, old if beta else None, n_chunks=0)
            assert rc == 0 and nws == 0
            _untouched(ws, 'workspace of a call without chunks')
            assert bool((dw[R.CENSUS_T:] == PATTERN).all())
            _assert_exact(_f32(dw, R.CENSUS_T), beta * old.astype(np.float64), '%s D=%d no chunks beta=%g' % (entry, d, beta))


@pytest.mark.parametrize('entry', ENTRIES)
def test_dw_refusals_come_before_any_launch(dev, entry):
    ld = _layout_on(dev)
    d, t_n = 100, R.CENSUS_T
    x, gn, old = R.dw_operands(d, 'int')
    xd, gd = _to(x, dev), _to(gn, dev)
    for code, what, kw in ((-2, 'D = 500', dict(d_arg=500)), (-1, 'type_shift = T', dict(shift=t_n)),
                           (-1, 'type_shift = -1', dict(shift=-1)), (-1, 'T = 0', dict(t_n=0)),
                           (-1, 'n_chunks = -1', dict(n_chunks=-1)), (-3, 'a workspace one byte short', dict(ws_short=1))):
        kw.setdefault('shift', 0)
        rc, dw, ws, _ = _dw_call(dev, entry, ld, xd, gd, d, kw.pop('shift'), 1.0, None, **kw)
        assert rc == code, (what, rc)
        _untouched(dw, what + ': dW')
        _untouched(ws, what + ': workspace')


# ---------------------------------------------------------------------------------------------
# 2. column sums: renet_colsum / renet_colsum_bf16
# ---------------------------------------------------------------------------------------------
def _colsum_input(dev, x, ldx, bf16):
    """X as [M + 2, ldx] with NaN in the excluded columns and in two rows behind the matrix"""
    m, n = x.shape
    if bf16:
        buf = torch.full((m + 2, ldx), PATTERN16, dtype=torch.int16, device=dev)
        if m:
            buf[:m, :n] = _to(R.rne_bf16(x).view(np.int16).reshape(m, n), dev)
    else:
        buf = torch.full((m + 2, ldx), PATTERN, dtype=torch.int32, device=dev)
        if m:
            buf[:m, :n] = _to(x, dev).view(torch.int32)
    return buf


def _colsum_call(dev, bf16, xbuf, m, n, ldx, beta, old, ws_short=0):
    import renet_hip as K
    out = _nanbuf(n, dev)
    if old is not None:
        _set(out, old)
    need = K.lib().renet_colsum_workspace(m, n)
    assert need == (R.colsum_groups(m) * n * 4 if m > 128 else 0), (m, n, need)
    ws = _nanbuf(need // 4, dev, tail=16)
    fn = K.lib().renet_colsum_bf16 if bf16 else K.lib().renet_colsum
    rc = fn(xbuf.data_ptr(), m, n, ldx, out.data_ptr(), beta, ws.data_ptr(), need - ws_short, K._stream())
    torch.cuda.synchronize()
    return rc, out, ws, need // 4


@pytest.mark.parametrize('kind', ['int', 'randn'])
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_colsum_equals_the_statement(dev, bf16, kind):
    """M across the one-pass / two-pass threshold (128 | 129), the 16-row unrolled loop and its 4-row tail (M = 1 .. 17, and
    the 129 rows of a group of M = 8193), the cap of 64 groups (8192 | 8193); N across the 64-column block (63, 64, 65);
    ldx = N and N + 3 with NaN in the excluded columns and behind the matrix.  Integer operands (|v| <= 8, exact in bf16):
    equal to the statement exactly; randn: within gamma(M + 2) * sum |terms| (bf16: of the bf16 values).  M = 0 gives
    out = beta * out.  beta = 0 runs over a NaN-prefilled out; the workspace is NaN-prefilled and of exact size."""
    kernel = 'colsum_bf16' if bf16 else 'colsum'
    for m, n in R.COLSUM_SHAPES:
        x, old = R.colsum_operands(m, n, kind, bf16)
        for ldx in (n, n + 3):
            xbuf = _colsum_input(dev, x, ldx, bf16)
            for beta in R.BETAS:
                what = '%s %s M=%d N=%d ldx=%d beta=%g' % (kernel, kind, m, n, ldx, beta)
                rc, out, ws, nws = _colsum_call(dev, bf16, xbuf, m, n, ldx, beta, old if beta != 0.0 else None)
                assert rc == 0, (what, rc)
                _tail_intact(out, n, what + ' out')
                _tail_intact(ws, nws, what + ' workspace')
                ref, mag = R.colsum_statement(x, beta, old)
                if kind == 'int':
                    _assert_exact(_f32(out, n), ref, what)
                else:
                    _within(_f32(out, n), ref, m, mag, kernel, what)
    if kind == 'randn':
        _show(kernel)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_colsum_refusals_come_before_any_launch(dev, bf16):
    for m, n in ((129, 65), (8193, 200)):
        x, old = R.colsum_operands(m, n, 'int')
        xbuf = _colsum_input(dev, x, n + 3, bf16)
        rc, out, ws, _ = _colsum_call(dev, bf16, xbuf, m, n, n + 3, 1.0, None, ws_short=4)
        assert rc == -3, rc
        _untouched(out, 'out of a call with a short workspace')
        _untouched(ws, 'the short workspace')
        rc, out, ws, _ = _colsum_call(dev, bf16, xbuf, m, n, n - 1, 1.0, None)
        assert rc == -1, rc
        _untouched(out, 'out of a call with ldx < N')
        _untouched(ws, 'workspace of a call with ldx < N')


# ---------------------------------------------------------------------------------------------
# 3. operand bounds: renet_maxabs_partials, renet_maxabs_partials_multi, the scalings
# ---------------------------------------------------------------------------------------------
FLAT = [(64, 64), (1024, 600), (4099, 4), (1024, 1100)]      # renet_maxabs_blocks: 1, 150, 4 and the cap of 256


def _maxabs_cases():
    """(rows, cols, ld, pointer offset in floats)"""
    cases = [(r, c, c, 0) for r, c in FLAT]
    for r in (1, 255, 256, 257):
        for c in (600, 601, 602, 603, 1103):
            cases.append((r, c, ((c + 3) & ~3) + 4, 0))      # rows of float4 (ld % 4 == 0), a column tail of c % 4
            cases.append((r, c, c + 1, 0))                   # scalar rows (c = 603, 1103: ld % 4 == 0 again, a tail of 3)
        cases.append((r, 3, 8, 0))                           # nothing but a column tail
        cases.append((r, 600, 600, 1))                       # contiguous, but the pointer is not 16-byte aligned
        cases.append((r, 602, 604, 1))
    return cases


def _maxabs_run(dev, xd, off, rows, cols, ld, part):
    import renet_hip as K
    part.fill_(PATTERN)
    rc = K.lib().renet_maxabs_partials(xd.data_ptr() + 4 * off, rows, cols, ld, part.data_ptr(), K._stream())
    torch.cuda.synchronize()
    return rc, part.cpu().numpy()


def test_maxabs_partials_on_every_path(dev):
    """the flat 4-way unrolled sweep (1, 4, 150 and 256 workgroups; with and without a remainder round), rows of float4
    with a column tail of 0 .. 3, scalar rows, unaligned pointers, ld > cols with 1e30 and NaN in the excluded columns,
    rows 1 / 255 / 256 / 257 around the cap of 256 workgroups.  The maximum is planted, positive and negative, at the
    first element, the last element, inside the column tail and in the last row: the maximum of the partials equals
    max |x| bit for bit, every one of the renet_maxabs_blocks partials is written and none behind them; a NaN inside the
    matrix is ignored, an inf gives inf."""
    import renet_hip as K
    assert [K.lib().renet_maxabs_blocks(r, c, c) for r, c in FLAT] == [1, 150, 4, 256]
    part = _nanbuf(256, dev)
    rng = np.random.RandomState(9)
    for rows, cols, ld, off in _maxabs_cases():
        what = 'maxabs [%d, %d] ld %d offset %d' % (rows, cols, ld, off)
        host = np.empty((rows, ld), np.float32)
        host[:, :cols] = rng.randn(rows, cols)
        host[:, cols:] = np.where(np.arange(ld - cols) % 2 == 0, np.float32(1e30), np.float32(np.nan))
        flat = np.concatenate((np.full(off, 1e30, np.float32), host.reshape(-1), np.full(TAIL, 1e30, np.float32)))
        xd = _to(flat, dev)
        nb = K.lib().renet_maxabs_blocks(rows, cols, ld)
        assert 1 <= nb <= 256

        def check(want, note):
            rc, p = _maxabs_run(dev, xd, off, rows, cols, ld, part)
            assert rc == 0, (what, note, rc)
            assert not (p[:nb] == PATTERN).any(), '%s %s: %d of %d partials never written' % (
                what, note, int((p[:nb] == PATTERN).sum()), nb)
            assert (p[nb:] == PATTERN).all(), '%s %s: written behind the %d partials' % (what, note, nb)
            got = p[:nb].view(np.float32)
            assert not np.isnan(got).any() and (got >= 0).all(), (what, note)
            _assert_bits(np.float32(got.max()).reshape(1), np.float32(want).reshape(1), '%s %s' % (what, note))

        check(R.maxabs_statement(host[:, :cols]), 'as drawn')
        tail_col = (cols & ~3) if cols & 3 else max(cols - 2, 0)
        spots = [(0, 0), (rows - 1, cols - 1), (rows // 2, tail_col), (rows - 1, 0)]
        for k, (r, c) in enumerate(spots):
            i, drawn = off + r * ld + c, float(host[r, c])
            for v in (1000.5 + k, -(2000.25 + k)):
                xd[i] = v
                check(abs(v), 'maximum %g planted at (%d, %d)' % (v, r, c))
            xd[i] = drawn
        for r, c in spots:                                   # NaNs inside the matrix, the maximum elsewhere
            xd[off + r * ld + c] = float('nan')
        nan_host = host.copy()
        for r, c in spots:
            nan_host[r, c] = np.nan
        check(R.maxabs_statement(nan_host[:, :cols]), 'NaN at the four spots')
        xd[off + (rows - 1) * ld + cols - 1] = float('-inf')
        check(np.inf, '-inf as the last element')


def test_maxabs_partials_empty_and_refused(dev):
    import renet_hip as K
    x = torch.ones(64, device=dev)
    part = _nanbuf(256, dev)
    for rows, cols in ((0, 8), (8, 0), (0, 0)):
        rc, p = _maxabs_run(dev, x, 0, rows, cols, 8, part)
        assert rc == 0 and p[0] == 0 and (p[1:] == PATTERN).all(), (rows, cols, rc)
        assert K.lib().renet_maxabs_blocks(rows, cols, 8) == 1
    rc, p = _maxabs_run(dev, x, 0, 8, 8, 7, part)
    assert rc == -1 and (p == PATTERN).all()
    assert K.lib().renet_maxabs_partials(x.data_ptr(), 8, 8, 8, None, K._stream()) == -1
    torch.cuda.synchronize()


def test_maxabs_partials_multi(dev):
    """one launch over 15 arrays: n4 (float4 per array) in {1, 255, 256, 257, 65 539} x nblocks in {1, 7, 256}, the records
    built as renet_hip._measure_all_weights builds them ({x, n4, part, nblocks | pad} as four int64).  Every array's
    maximum is bit-equal, exactly its nblocks partials are written, a NaN is ignored; n_jobs = 0 launches nothing."""
    import renet_hip as K
    rng = np.random.RandomState(13)
    jobs, rows = [], []
    for n4 in (1, 255, 256, 257, 65536 + 3):
        for nblocks in (1, 7, 256):
            x = rng.randn(4 * n4).astype(np.float32)
            x[rng.randint(0, 4 * n4)] = np.nan
            x[(4 * n4 - 1) if nblocks == 7 else rng.randint(0, 4 * n4)] = -(50.0 + len(jobs))     # (7: in the last float4)
            xd, part = _to(x, dev), _nanbuf(nblocks, dev)
            assert xd.data_ptr() % 16 == 0
            jobs.append((x, xd, part, nblocks))
            rows.append([xd.data_ptr(), n4, part.data_ptr(), nblocks])
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    assert K.lib().renet_maxabs_partials_multi(table.data_ptr(), 0, K._stream()) == 0
    torch.cuda.synchronize()
    for _, _, part, _ in jobs:
        _untouched(part, 'partials of a launch over no array')
    assert K.lib().renet_maxabs_partials_multi(table.data_ptr(), len(jobs), K._stream()) == 0
    torch.cuda.synchronize()
    for k, (x, _, part, nblocks) in enumerate(jobs):
        p = part.cpu().numpy()
        what = 'array %d (n4 %d, %d partials)' % (k, x.size // 4, nblocks)
        assert not (p[:nblocks] == PATTERN).any(), what + ': partials never written'
        assert (p[nblocks:] == PATTERN).all(), what + ': written behind its partials'
        _assert_bits(np.float32(p[:nblocks].view(np.float32).max()).reshape(1), R.maxabs_statement(x).reshape(1), what)


SCALE_NS = [1, 2, 3, 4, 5, 1023, 1024, 1027, 2048 * 256 * 4 + 5]
FACTORS = [1.0, -1.0, 0.0, 0.1, -3.0]


@pytest.mark.parametrize('n', [0] + SCALE_NS)
def test_scale_by_device_scalar_and_its_bound(dev, n):
    """x[i] = float32(x[i]) * float32(f) bit for bit, the factor read from device memory, for n across the float4 body, the
    tail of n % 4 elements and the grid cap (2048 workgroups); f = 1 leaves every bit in place (NaN payloads, -0);
    *bound_out = |f| * bound_in even then; nothing is written behind x[n)."""
    import renet_hip as K
    rng = np.random.RandomState(n % 1000)
    x = rng.randn(n).astype(np.float32)
    bits = x.view(np.uint32)
    if n:
        bits[0] = 0x80000000                                            # -0
        bits[n - 1] = 0xffc00001 if n > 1 else bits[n - 1]              # NaN payloads
        bits[n // 2] = 0x7fc12345 if n > 2 else bits[n // 2]
    bound_in = np.float32(3.7)
    for f in FACTORS:
        fd = torch.tensor([f], dtype=torch.float32, device=dev)
        for with_bound in ((True,) if n == 0 else (False, True)):
            what = 'scale n=%d f=%g %s' % (n, f, 'with bound' if with_bound else 'plain')
            buf, bo = _nanbuf(n, dev), _nanbuf(1, dev)
            buf[:n] = _to(bits.view(np.int32), dev)
            if with_bound:
                rc = K.lib().renet_scale_by_device_scalar_bound(buf.data_ptr(), n, fd.data_ptr(), float(bound_in),
                                                                bo.data_ptr(), K._stream())
            else:
                rc = K.lib().renet_scale_by_device_scalar(buf.data_ptr(), n, fd.data_ptr(), K._stream())
            torch.cuda.synchronize()
            assert rc == 0, (what, rc)
            _tail_intact(buf, n, what)
            got = buf[:n].cpu().numpy().view(np.uint32)
            if np.float32(f) == 1:
                _assert_bits(got, bits, what)
            else:
                with np.errstate(invalid='ignore'):
                    want = x * np.float32(f)
                nan = np.isnan(x)
                assert np.isnan(got.view(np.float32)[nan]).all(), what + ': a NaN did not stay one'
                _assert_bits(got[~nan], want.view(np.uint32)[~nan], what)
            if with_bound:
                _tail_intact(bo, 1, what + ' bound_out')
                _assert_bits(_f32(bo, 1), (np.abs(np.float32(f)) * bound_in).reshape(1), what + ' bound_out')
            else:
                _untouched(bo, what + ' bound_out')


def test_scale_by_device_scalar_refuses_an_unaligned_pointer(dev):
    import renet_hip as K
    fd = torch.tensor([2.0], device=dev)
    buf, bo = _nanbuf(64, dev), _nanbuf(1, dev)
    assert K.lib().renet_scale_by_device_scalar(buf.data_ptr() + 4, 8, fd.data_ptr(), K._stream()) == -1
    assert K.lib().renet_scale_by_device_scalar_bound(buf.data_ptr() + 4, 8, fd.data_ptr(), 1.0, bo.data_ptr(),
                                                      K._stream()) == -1
    assert K.lib().renet_scale_by_device_scalar(buf.data_ptr(), 0, fd.data_ptr(), K._stream()) == 0
    torch.cuda.synchronize()
    _untouched(buf, 'x of a refused scaling')
    _untouched(bo, 'bound_out of a refused scaling')


def test_scale_bf16_by_device_scalar(dev):
    """over the renet_pack_bf16 buffer ([512, 256] bf16) of a [257, 200] matrix: rne_bf16(float32(x) * f) bit for bit, the
    zero padding stays zero, f = 1 changes nothing, nothing is written behind the buffer"""
    import renet_hip as K
    r, c, rp, cp = 257, 200, 512, 256
    x = np.random.RandomState(21).randn(r, c).astype(np.float32)
    assert K.lib().renet_bf16_bytes(r, c) == rp * cp * 2
    packed = torch.full((rp * cp + 16,), PATTERN16, dtype=torch.int16, device=dev)
    assert K.lib().renet_pack_bf16(_to(x, dev).data_ptr(), r, c, c, packed.data_ptr(), K._stream()) == 0
    torch.cuda.synchronize()
    bits = packed.cpu().numpy().view(np.uint16)
    want = np.zeros((rp, cp), np.uint16)
    want[:r, :c] = R.rne_bf16(x).reshape(r, c)
    _assert_bits(bits[:rp * cp].reshape(rp, cp), want, 'renet_pack_bf16')
    assert (bits[rp * cp:] == PATTERN16).all()
    for f in FACTORS:
        buf = packed.clone()
        fd = torch.tensor([f], dtype=torch.float32, device=dev)
        assert K.lib().renet_scale_bf16_by_device_scalar(buf.data_ptr(), rp * cp, fd.data_ptr(), K._stream()) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint16)
        assert (got[rp * cp:] == PATTERN16).all(), 'written behind the buffer'
        got = got[:rp * cp].reshape(rp, cp)
        _assert_bits(got, R.scale_bf16_statement(want, f), 'scale_bf16 f=%g' % f)
        pad = R.bf16_to_f32(got).reshape(rp, cp)
        assert (pad[r:] == 0).all() and (pad[:, c:] == 0).all(), 'padding no longer zero at f=%g' % f


# ---------------------------------------------------------------------------------------------
# 4. segmented add: renet_segment_add / renet_segment_add2
# ---------------------------------------------------------------------------------------------
def _seg_call(dev, lay_d, lay, d, srcs, olds, d_arg=None, u_arg=None):
    import renet_hip as K
    dsts = [_set(_nanrows(lay['n_dst'], d, dev), o) for o in olds]
    u_n, d_arg = lay['U'] if u_arg is None else u_arg, d if d_arg is None else d_arg
    plan = (lay_d['order'].data_ptr(), lay_d['seg_ptr'].data_ptr(), lay_d['seg_target'].data_ptr(), u_n, d_arg)
    if len(srcs) == 1:
        rc = K.lib().renet_segment_add(srcs[0].data_ptr(), *plan, dsts[0].data_ptr(), K._stream())
    else:
        rc = K.lib().renet_segment_add2(srcs[0].data_ptr(), srcs[1].data_ptr(), *plan, dsts[0].data_ptr(),
                                        dsts[1].data_ptr(), K._stream())
    torch.cuda.synchronize()
    return rc, dsts


@pytest.mark.parametrize('u_n', R.SEG_US)
@pytest.mark.parametrize('d', DS)
def test_segment_add_equals_the_statement(dev, d, u_n):
    """segments of 0, 1, 7, 8, 9, 15, 16 | 17, 24, 127, 128, 129, 257 and 1000 rows (one wave per segment up to 16 rows, the
    whole workgroup beyond; 8 rows per wave and round, 128 per workgroup and round), U across the grid formula (one
    workgroup per segment up to 512, 16 segments per workgroup beyond: short and long segments then share a workgroup),
    D = 300 with its lane tail.  Targets are distinct and unsorted, `order` repeats rows; dst has 3 rows no segment
    targets, which must keep their bits.  Integer operands: exact, for renet_segment_add and for both outputs of
    renet_segment_add2 (src1 differs from src0); randn: within gamma(len + 3) * sum |terms|."""
    for kind in ('int', 'randn'):
        lay, src0, src1, old0, old1 = R.segment_case(u_n, d, kind)
        lay_d = {k: _to(lay[k], dev) for k in ('order', 'seg_ptr', 'seg_target')}
        s0, s1 = _to(src0, dev), _to(src1, dev)
        refs = [R.segment_add_statement(s, lay, o) for s, o in ((src0, old0), (src1, old1))]
        for srcs, olds in (((s0,), (old0,)), ((s0, s1), (old0, old1))):
            rc, dsts = _seg_call(dev, lay_d, lay, d, srcs, olds)
            assert rc == 0, rc
            for k, dst in enumerate(dsts):
                what = 'segment_add%s[%d] %s U=%d D=%d' % ('2' if len(srcs) == 2 else '', k, kind, u_n, d)
                assert bool((dst[lay['n_dst']:] == PATTERN).all()), what + ': written behind the last row'
                got = _f32(dst, lay['n_dst'])
                ref, mag, n = refs[k]
                _assert_bits(got[n == 0], olds[k][n == 0], what + ': a row no segment targets')
                if kind == 'int':
                    _assert_exact(got, ref, what)
                else:
                    _within(got, ref, n[:, None], mag, 'segment_add D=%d' % d, what)
    if u_n == R.SEG_US[-1]:
        _show('segment_add D=%d' % d)


def test_segment_add_refusals_and_the_empty_plan(dev):
    lay, src0, src1, old0, old1 = R.segment_case(17, 100, 'int')
    lay_d = {k: _to(lay[k], dev) for k in ('order', 'seg_ptr', 'seg_target')}
    s0, s1 = _to(src0, dev), _to(src1, dev)
    for srcs, olds in (((s0,), (old0,)), ((s0, s1), (old0, old1))):
        for code, kw in ((-2, dict(d_arg=516)), (-1, dict(d_arg=6)), (0, dict(u_arg=0)), (-1, dict(u_arg=-1))):
            rc, dsts = _seg_call(dev, lay_d, lay, 100, srcs, olds, **kw)
            assert rc == code, (kw, rc)
            for dst, old in zip(dsts, olds):
                _assert_bits(_f32(dst, lay['n_dst']), old, 'dst of a call that must not launch %r' % kw)


# ---------------------------------------------------------------------------------------------
# 5. small entries
# ---------------------------------------------------------------------------------------------
def test_compose_table_items(dev):
    """an item stream of edge items, flush items (-1) and a few types <= -2, n_items and E no multiples of 4: the four
    outputs equal the statement bit for bit, the sentinels behind them are intact; n_items = 0 and E = 0 launch nothing"""
    import renet_hip as K
    rng = np.random.RandomState(17)
    n_rows, n_items, e = 301, 1203, 997
    row_map = rng.permutation(5000)[:n_rows].astype(np.int32)
    it_src = rng.randint(0, n_rows, n_items).astype(np.int32)
    it_type = rng.randint(0, 40, n_items).astype(np.int32)
    it_type[rng.rand(n_items) < 0.25] = -1
    it_type[[5, 77, 1200]] = [-2, -3, -17]
    it_src[[0, 1]], it_type[[0, 1]] = [n_rows - 1, 0], [0, -1]
    col, e_src = rng.randint(0, n_rows, e).astype(np.int32), rng.randint(0, n_rows, e).astype(np.int32)
    want = R.compose_statement(row_map, it_src, it_type, col, e_src)
    ins = [_to(a, dev) for a in (row_map, it_src, it_type, col, e_src)]

    def run(ni, ne):
        outs = [_nanbuf(k, dev) for k in (n_items, n_items, e, e)]
        rc = K.lib().renet_compose_table_items(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ni, ins[3].data_ptr(),
                                               ins[4].data_ptr(), ne, *[o.data_ptr() for o in outs], K._stream())
        torch.cuda.synchronize()
        return rc, outs

    rc, outs = run(n_items, e)
    assert rc == 0
    for name, o, w in zip(('it_src_t', 'it_type_t', 'col_t', 'e_src_t'), outs, want):
        _tail_intact(o, len(w), name)
        _assert_bits(o[:len(w)].cpu().numpy(), w, name)
    rc, outs = run(0, 0)
    assert rc == 0
    for o in outs:
        _untouched(o, 'an output of the empty composition')
    rc, outs = run(n_items, 0)                               # E = 0: the item arrays alone
    assert rc == 0
    _assert_bits(outs[0][:n_items].cpu().numpy(), want[0], 'it_src_t with E = 0')
    _assert_bits(outs[1][:n_items].cpu().numpy(), want[1], 'it_type_t with E = 0')
    _untouched(outs[2], 'col_t with E = 0')
    _untouched(outs[3], 'e_src_t with E = 0')


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, 2048 * 256 * 4 + 5])
def test_add_inplace_and_zero(dev, n):
    import renet_hip as K
    rng = np.random.RandomState(n % 997)
    x, y = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    buf, yd = _set(_nanbuf(n, dev), x), _to(y, dev)
    assert K.lib().renet_add_inplace(buf.data_ptr(), yd.data_ptr(), n, K._stream()) == 0
    torch.cuda.synchronize()
    _tail_intact(buf, n, 'add_inplace n=%d' % n)
    _assert_bits(_f32(buf, n), x + y, 'add_inplace n=%d' % n)
    assert K.lib().renet_zero(buf.data_ptr(), n, K._stream()) == 0
    torch.cuda.synchronize()
    _tail_intact(buf, n, 'zero n=%d' % n)
    assert bool((buf[:n] == 0).all()), 'renet_zero n=%d left something' % n
    fresh = _nanbuf(8, dev)
    assert K.lib().renet_zero(fresh.data_ptr(), 0, K._stream()) == 0
    assert K.lib().renet_add_inplace(fresh.data_ptr(), yd.data_ptr(), 0, K._stream()) == 0
    torch.cuda.synchronize()
    _untouched(fresh, 'a buffer of n = 0')
