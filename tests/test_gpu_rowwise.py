"""GPU tests of the row-wise "glue" kernels and the optimizer against plain numpy float64 statements written here:
csrc/seq.hip (dropout, sequence assembly, concat3, the softmax-CE kernels, the segment pool), rgcn_bwd_prep
(csrc/rgcn_bwd.hip), gather_rows (csrc/rows.hip) and csrc/optim.hip.

Element-wise kernels produce one fp32 product of an input and a mask multiplier per output, so float32(float64(x) * mult)
with the host statement of the mask (tests/dropout_masks.py) is what they must produce BIT FOR BIT.  The reductions carry
bounds derived from their arithmetic (stated at each test); every softmax / reduction test prints the worst observed
error-to-bound ratio (`pytest -s`; recorded in profiles/rowwise_float64_tests.md)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import dropout_masks as DM

pytestmark = pytest.mark.gpu

U23, U24 = 2.0 ** -23, 2.0 ** -24
SEEDS = (0, 1234567, (1 << 40) + 3)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _to(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _mul32(x, mult):
    """float32(float64(x) * mult): the correctly rounded fp32 product, i.e. the product the kernel forms."""
    return (x.astype(np.float64) * mult).astype(np.float32)


def _assert_bits(got, want, what=''):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    view = {4: np.uint32, 2: np.uint16}[got.dtype.itemsize]
    bad = np.nonzero(got.view(view).reshape(-1) != want.view(view).reshape(-1))[0]
    assert bad.size == 0, '%s: %d of %d elements differ, first at flat index %d: got %r, want %r' % (
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _report(what, ratio):
    print('  ratio %-58s %.3f' % (what, ratio))


def _index(rng, n_rows, n):
    """n row indices into a table of n_rows rows: the last row, the first row and a duplicate are always there (as far
    as n allows)."""
    idx = rng.randint(0, n_rows, n).astype(np.int32)
    idx[0] = n_rows - 1
    if n > 1:
        idx[1] = 0
    if n > 3:
        idx[3] = idx[2]
    return idx


@contextlib.contextmanager
def _bounds_mode(monkeypatch, fused):
    """The f16x3 mode, in which the producers' wrappers return operand bounds -- from the kernel that writes the tensor
    (RENET_FUSED_BOUNDS=1: the `_bounds` entry, at most 1024 workgroups) or not at all (=0: the plain entry, at most 2048).
    The switch is read at every call, so both settings run in this process."""
    import renet_hip as K
    monkeypatch.setenv('RENET_FUSED_BOUNDS', '1' if fused else '0')
    with K.gemm_mode('f16x3'):
        yield


def _check_bound(t, ref, what):
    """fused mode: the partial maxima noted on the tensor; their maximum is max |t| exactly."""
    part, n = t._renet_bound
    assert float(part[:n].max()) == float(np.abs(ref).max()), what


# ---------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [4, 1024, 4 * (2048 * 256 + 77)], ids=['n4', 'n1024', 'n2097460-grid-cap'])
@pytest.mark.parametrize('p', [0.0, 0.2, 0.5])
def test_dropout_equals_the_host_mask(dev, n, p):
    import renet_hip as K
    x = np.random.RandomState(n % 1000 + int(p * 10)).randn(n).astype(np.float32)
    tx = _to(x, dev)
    for seed in SEEDS:
        mult = DM.drop_multipliers(seed, 0, n // 4, p)
        _assert_bits(_np(K.dropout(tx, p, seed)), _mul32(x, mult), 'dropout n=%d p=%g seed=%d' % (n, p, seed))
    if p > 0:
        assert not np.array_equal(DM.drop_multipliers(SEEDS[1], 0, n // 4, p), DM.drop_multipliers(SEEDS[2], 0, n // 4, p))


# ---------------------------------------------------------------------------------------------
# sequence assembly, forward
# ---------------------------------------------------------------------------------------------
_SEQ_CASES = [(s, d) for d in (4, 100, 300) for s in (1, 37)] + [(2700, 200)]
_SEQ_IDS = ['S%d-D%d' % c for c in _SEQ_CASES[:-1]] + ['S2700-D200-grid-caps']
SEED_X, SEED_XR = 1234567, (1 << 40) + 3


def _seq_inputs(s, d):
    rng = np.random.RandomState(1000 * d + s)
    tabs = [rng.randn(n, d).astype(np.float32) for n in (11, 7, 5, 3)]             # h2, ent, rel, glob
    idx = [_index(rng, t.shape[0], s) for t in tabs]
    return tabs, idx


def _seq_reference(tabs, idx, s, d, p):
    h2, ent, rel, glob = (t[i] for t, i in zip(tabs, idx))
    x = _mul32(np.concatenate((h2, ent, rel, glob), axis=1), DM.x_mask(s, d, SEED_X, p))
    xr = _mul32(np.concatenate((h2, ent, glob), axis=1), DM.xr_mask(s, d, SEED_XR, p))
    return x, xr


@pytest.mark.parametrize('s,d', _SEQ_CASES, ids=_SEQ_IDS)
@pytest.mark.parametrize('p', [0.0, 0.5])
def test_seq_assemble_fwd_equals_the_statement(dev, monkeypatch, s, d, p):
    import renet_hip as K
    tabs, idx = _seq_inputs(s, d)
    x_ref, xr_ref = _seq_reference(tabs, idx, s, d, p)
    if p > 0 and s * d >= 400:
        assert not np.array_equal(DM.x_mask(s, d, SEED_X, p)[:, :3 * d], DM.xr_mask(s, d, SEED_XR, p))
    args = [_to(t, dev) for t in tabs] + [_to(i, dev) for i in idx] + [p, SEED_X, SEED_XR]
    outs = []
    for fused in (True, False):
        with _bounds_mode(monkeypatch, fused):
            x, xr = K.seq_assemble_fwd(*args)
        assert hasattr(x, '_renet_bound') == fused and hasattr(xr, '_renet_bound') == fused
        _assert_bits(_np(x), x_ref, 'X fused=%d' % fused)
        _assert_bits(_np(xr), xr_ref, 'Xr fused=%d' % fused)
        if fused:
            _check_bound(x, x_ref, 'max |X|')
            _check_bound(xr, xr_ref, 'max |Xr|')
        outs.append((x, xr))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    x, xr = K.seq_assemble_fwd(*args)                        # the process default mode
    _assert_bits(_np(x), x_ref, 'X')
    _assert_bits(_np(xr), xr_ref, 'Xr')


def _ceil(n, m):
    return (n + m - 1) // m * m


def _bf16_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bf16_padded_expectation(ref32, rows_alloc, ld, zero_rows_to):
    """What a producer of a zero-padded bf16 operand matrix must leave in a NaN-prefilled [rows_alloc, ld] buffer: the RNE
    rounding of ref32 [R, C] in the logical block, zeros in columns [C, min(ceil64(C), ld)) of its rows and in rows
    [R, zero_rows_to), the NaN sentinel everywhere else.  -> uint16 bit patterns."""
    r, c = ref32.shape
    want = _bf16_bits(torch.full((rows_alloc, ld), float('nan'), dtype=torch.bfloat16))
    want[:r, :c] = _bf16_bits(torch.tensor(ref32).to(torch.bfloat16))
    want[:r, c:min(_ceil(c, 64), ld)] = 0
    want[r:zero_rows_to, :] = 0
    return want


@pytest.mark.parametrize('s,d', _SEQ_CASES, ids=_SEQ_IDS)
@pytest.mark.parametrize('p', [0.0, 0.5])
def test_seq_assemble_fwd_bf16_is_the_rounded_statement_in_a_zero_padded_matrix(dev, s, d, p):
    import renet_hip as K
    tabs, idx = _seq_inputs(s, d)
    x_ref, xr_ref = _seq_reference(tabs, idx, s, d, p)
    # the sizes of renet_hip.bf16_empty, plus 3 rows so that rows_alloc is no multiple of 64
    rows_alloc, ldx, ldxr = _ceil(s, 256) + 3 if s > 1 else 40, _ceil(4 * d, 256), _ceil(3 * d, 256)
    x = torch.full((rows_alloc, ldx), float('nan'), device=dev, dtype=torch.bfloat16)
    xr = torch.full((rows_alloc, ldxr), float('nan'), device=dev, dtype=torch.bfloat16)
    dt = [_to(t, dev) for t in tabs]
    di = [_to(i, dev) for i in idx]
    K._check(K.lib().renet_seq_assemble_fwd_bf16(*[t.data_ptr() for t in dt], *[i.data_ptr() for i in di], s, d, p, SEED_X,
                                                 SEED_XR, x.data_ptr(), ldx, xr.data_ptr(), ldxr, rows_alloc, K._stream()),
             'seq_assemble_fwd_bf16')
    torch.cuda.synchronize()
    zero_to = min(_ceil(s, 64), rows_alloc)
    assert zero_to < rows_alloc or s == 1                    # (S = 1: rows [1, 40) are all padding rows)
    _assert_bits(_bf16_bits(x), _bf16_padded_expectation(x_ref, rows_alloc, ldx, zero_to), 'X bf16')
    _assert_bits(_bf16_bits(xr), _bf16_padded_expectation(xr_ref, rows_alloc, ldxr, zero_to), 'Xr bf16')


# ---------------------------------------------------------------------------------------------
# sequence assembly, backward
# ---------------------------------------------------------------------------------------------
def _seq_bwd_case(d, p):
    """Packed layout with decreasing lengths (row of step j of sequence i is off[j] + i), random dX / dXr, and three
    statements of every output: float64 (value, sum of |terms|, number of terms) and the kernels' own arithmetic in numpy
    float32 -- products of the masked terms, added serially in the kernels' order.  The mask multipliers are 0, 1 or 2, so
    the products are exact and a fused multiply-add changes nothing: the float32 statement is exact to the bit."""
    L = 5
    lens = np.array([5] * 6 + [4] * 3 + [2] * 2 + [1] * 3)
    nseq, num_seq = len(lens), len(lens) + 3
    off = np.concatenate(([0], np.cumsum([(lens > j).sum() for j in range(L)]))).astype(np.int32)
    s = int(off[-1])
    assert s == lens.sum() == 49
    rng = np.random.RandomState(d + int(p * 10))
    dx, dxr = rng.randn(s, 4 * d).astype(np.float32), rng.randn(s, 3 * d).astype(np.float32)
    tx = dx.astype(np.float64) * DM.x_mask(s, d, SEED_X, p)
    txr = dxr.astype(np.float64) * DM.xr_mask(s, d, SEED_XR, p)
    tx32, txr32 = tx.astype(np.float32), txr.astype(np.float32)
    assert np.array_equal(tx32, tx) and np.array_equal(txr32, txr)            # exact products
    ref = {'dRows': (tx[:, :d] + txr[:, :d], np.abs(tx[:, :d]) + np.abs(txr[:, :d]), np.full((s, 1), 2)),
           'dEnt': tuple(np.zeros((num_seq, d)) for _ in range(2)) + (np.zeros((num_seq, 1)),),
           'dRel': tuple(np.zeros((num_seq, d)) for _ in range(2)) + (np.zeros((num_seq, 1)),)}
    f32 = {'dRows': tx32[:, :d] + txr32[:, :d], 'dEnt': np.zeros((num_seq, d), dtype=np.float32),
           'dRel': np.zeros((num_seq, d), dtype=np.float32)}
    for i in range(nseq):
        for j in range(lens[i]):
            r = off[j] + i
            for name, terms in (('dEnt', ((tx, tx32), (txr, txr32))), ('dRel', ((tx, tx32),))):
                c0 = d if name == 'dEnt' else 2 * d
                for t64, t32 in terms:
                    ref[name][0][i] += t64[r, c0:c0 + d]
                    ref[name][1][i] += np.abs(t64[r, c0:c0 + d])
                    ref[name][2][i] += 1
                    f32[name][i] = f32[name][i] + t32[r, c0:c0 + d]
    return dict(L=L, nseq=nseq, num_seq=num_seq, off=off, dx=dx, dxr=dxr, ref=ref, f32=f32)


@pytest.mark.parametrize('d', [100, 300])
@pytest.mark.parametrize('p', [0.0, 0.5])
def test_seq_assemble_bwd_matches_fp64_sums_under_the_forward_masks(dev, d, p):
    """dRows = dX[:, :D] m + dXr[:, :D] m; dEnt[i] / dRel[i] = the sums over the steps of sequence i of the ent / rel parts.
    Bound per element against float64: n * 2^-24 * (sum of |terms|) for a sum of n terms (at least 2) -- the products'
    roundings add up to at most 2^-24 * sum |terms| and each of the n - 1 additions rounds a partial sum that sum |terms|
    bounds.  (2^-23 * sum |terms| for every n, the bound this test was first written with, holds for n = 2 only: the float32
    statement of the same serial sums, computed on the host, exceeds it at n = 10 -- both ratios are printed.)  The kernel
    must also equal that float32 statement bit for bit, and rows that belong to no sequence must be exactly zero."""
    import renet_hip as K
    c = _seq_bwd_case(d, p)
    got = K.seq_assemble_bwd(_to(c['dx'], dev), _to(c['dxr'], dev), _to(c['off'], dev), c['L'], c['num_seq'], d, p,
                             SEED_X, SEED_XR)
    for name, out in zip(('dRows', 'dEnt', 'dRel'), got):
        ref, mag, n_terms = c['ref'][name]
        out = _np(out)
        assert out.shape == ref.shape
        tol = np.maximum(n_terms, 2) * U24 * mag * (1 + 2.0 ** -20)
        live = mag > 0
        for who, val in (('kernel', out), ('float32 statement', c['f32'][name])):
            err = np.abs(val.astype(np.float64) - ref)
            _report('seq_assemble_bwd %s D=%d p=%g, %s' % (name, d, p, who), float((err[live] / tol[live]).max()))
            _report('    against 2^-23 sum|terms|', float((err[live] / (U23 * mag[live])).max()))
            assert (err <= tol).all(), (name, who, float((err[live] / tol[live]).max()))
        _assert_bits(out, c['f32'][name], name + ' against the float32 statement')
    assert not _np(got[1])[c['nseq']:].any() and not _np(got[2])[c['nseq']:].any()


# ---------------------------------------------------------------------------------------------
# concat3
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('parts', [2, 3])
@pytest.mark.parametrize('b', [1, 33])
@pytest.mark.parametrize('d', [100, 300])
@pytest.mark.parametrize('p', [0.0, 0.5])
def test_concat3_fwd_and_bwd_equal_the_statement_under_one_mask(dev, monkeypatch, parts, b, d, p):
    import renet_hip as K
    rng = np.random.RandomState(parts * 7 + b * 13 + d + int(p * 10))
    a, hmid, c = (rng.randn(n, d).astype(np.float32) for n in (9, b, 6))
    ia, ic = _index(rng, 9, b), _index(rng, 6, b)
    seed = SEEDS[2]
    mask = DM.concat_mask(b, parts, d, seed, p)
    cols = [a[ia], hmid] + ([c[ic]] if parts == 3 else [])
    ref = _mul32(np.concatenate(cols, axis=1), mask)
    args = (_to(a, dev), _to(ia, dev), _to(hmid, dev), _to(c, dev) if parts == 3 else None,
            _to(ic, dev) if parts == 3 else None, p, seed)
    for fused in (True, False):
        with _bounds_mode(monkeypatch, fused):
            feat = K.concat3_fwd(*args)
        assert hasattr(feat, '_renet_bound') == fused
        _assert_bits(_np(feat), ref, 'feat fused=%d' % fused)
        if fused:
            _check_bound(feat, ref, 'max |feat|')
    _assert_bits(_np(K.concat3_fwd(*args)), ref, 'feat')
    # backward of a random dfeat
    dfeat = rng.randn(b, parts * d).astype(np.float32)
    dref = _mul32(dfeat, mask)
    got = K.concat3_bwd(_to(dfeat, dev), d, parts, p, seed)
    assert (got[2] is None) == (parts == 2)
    for k in range(parts):
        _assert_bits(_np(got[k]), dref[:, k * d:(k + 1) * d], 'concat3_bwd part %d' % k)
    # the masks themselves, read from both kernels with ones as data: one array, the host statement
    ones = torch.ones(9, d, device=dev)
    i0 = torch.zeros(b, device=dev, dtype=torch.int32)
    fmask = K.concat3_fwd(ones, i0, ones[:b] if b <= 9 else torch.ones(b, d, device=dev), ones if parts == 3 else None,
                          i0 if parts == 3 else None, p, seed)
    bparts = K.concat3_bwd(torch.ones(b, parts * d, device=dev), d, parts, p, seed)
    bmask = torch.cat([t for t in bparts if t is not None], dim=1)
    assert torch.equal(fmask, bmask)
    _assert_bits(_np(fmask), mask.astype(np.float32), 'mask')


# ---------------------------------------------------------------------------------------------
# rgcn_bwd_prep
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('n', [1, 50])
@pytest.mark.parametrize('d', [100, 200, 300, 400])
def test_rgcn_bwd_prep_equals_the_statement(dev, monkeypatch, relu, p, n, d):
    """gn = float32(g [out > 0] norm[row]), g_loop = float32(g [out > 0] mask); [out > 0] selects g or +0 (the kernel
    replaces the value, it does not multiply), so exact zeros and negative zeros of `out` both close the gate."""
    import renet_hip as K
    rng = np.random.RandomState(relu + 2 * n + d + int(p * 10))
    g = rng.randn(n, d).astype(np.float32)
    out = rng.randn(n, d).astype(np.float32)
    out[rng.rand(n, d) < 0.15] = 0.0
    out[rng.rand(n, d) < 0.15] = -0.0
    assert (out == 0).any() and np.signbit(out[out == 0]).any() and not np.signbit(out[out == 0]).all()
    norm = (1.0 / rng.randint(1, 9, n)).astype(np.float32)
    seed = SEEDS[1]
    gated = np.where(out > 0, g, np.float32(0.0)) if relu else g
    gn_ref = _mul32(gated, norm.astype(np.float64)[:, None])
    gl_ref = _mul32(gated, DM.flat_mask(n, d, seed, p))
    tg, tout, tnorm = _to(g, dev), _to(out, dev), _to(norm, dev)
    for mode in ('fused', 'unfused', 'default'):
        gn = torch.full((n, d), float('nan'), device=dev)
        gl = torch.full((n, d), float('nan'), device=dev)
        with (_bounds_mode(monkeypatch, mode == 'fused') if mode != 'default' else contextlib.nullcontext()):
            K.rgcn_bwd_prep(tg, tout, tnorm, relu, p, seed, gn, gl)
        _assert_bits(_np(gn), gn_ref, 'gn ' + mode)
        _assert_bits(_np(gl), gl_ref, 'g_loop ' + mode)
        assert hasattr(gl, '_renet_bound') == (mode == 'fused')
        if mode == 'fused':
            _check_bound(gl, gl_ref, 'max |g_loop|')


def test_rgcn_bwd_prep_beyond_both_grid_caps(dev, monkeypatch):
    """N * D/4 > 2048 * 256 float4 groups: the grid-stride loop of the plain entry (2048 workgroups) and of the `_bounds`
    entry (1024)."""
    import renet_hip as K
    n, d, p, seed = 5300, 400, 0.5, SEEDS[2]
    assert n * d // 4 > 2048 * 256
    rng = np.random.RandomState(53)
    g, out = rng.randn(n, d).astype(np.float32), rng.randn(n, d).astype(np.float32)
    norm = (1.0 / rng.randint(1, 9, n)).astype(np.float32)
    gated = np.where(out > 0, g, np.float32(0.0))
    gn_ref, gl_ref = _mul32(gated, norm.astype(np.float64)[:, None]), _mul32(gated, DM.flat_mask(n, d, seed, p))
    for fused in (True, False):
        gn, gl = torch.full((n, d), float('nan'), device=dev), torch.full((n, d), float('nan'), device=dev)
        with _bounds_mode(monkeypatch, fused):
            K.rgcn_bwd_prep(_to(g, dev), _to(out, dev), _to(norm, dev), 1, p, seed, gn, gl)
        _assert_bits(_np(gn), gn_ref, 'gn')
        _assert_bits(_np(gl), gl_ref, 'g_loop')
        if fused:
            _check_bound(gl, gl_ref, 'max |g_loop|')


# ---------------------------------------------------------------------------------------------
# gather_rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [100, 200, 300, 400])
@pytest.mark.parametrize('n', [1, 513])
def test_gather_rows_is_exact(dev, d, n):
    import renet_hip as K
    rng = np.random.RandomState(d + n)
    table = rng.randn(23, d).astype(np.float32)
    idx = _index(rng, 23, n)
    out = torch.full((n, d), float('nan'), device=dev)
    assert K.gather_rows(_to(table, dev), _to(idx, dev), out=out) is out
    _assert_bits(_np(out), table[idx], 'gather_rows')


def test_gather_rows_beyond_the_grid_cap(dev):
    import renet_hip as K
    n, d = 21001, 100
    assert n * d // 4 > 2048 * 256
    rng = np.random.RandomState(21001)
    table = rng.randn(301, d).astype(np.float32)
    idx = _index(rng, 301, n)
    out = torch.full((n, d), float('nan'), device=dev)
    K.gather_rows(_to(table, dev), _to(idx, dev), out=out)
    _assert_bits(_np(out), table[idx], 'gather_rows')


# ---------------------------------------------------------------------------------------------
# segment pool
# ---------------------------------------------------------------------------------------------
SEG_LENS = [1, 2, 3, 4, 5, 7, 64, 1000]


def _pool_rows(d, ties):
    """h [1086, D] and seg_ptr of SEG_LENS.  ties: in every segment the column maximum is planted several times --
    column c has its winner in wave position (c % 4) (a segment's row k is read by wave k % 4), a second copy later in
    the SAME wave, and copies at later rows of the other waves, so that the in-wave scan (strict >) and the four-wave
    combine (equal value: smaller row index) must both keep the first maximum in row order."""
    rng = np.random.RandomState(d)
    seg_ptr = np.concatenate(([0], np.cumsum(SEG_LENS))).astype(np.int32)
    h = rng.randn(int(seg_ptr[-1]), d).astype(np.float32)
    if ties:
        top = np.float32(7.5)
        for r0, r1 in zip(seg_ptr[:-1], seg_ptr[1:]):
            n = r1 - r0
            for c in range(d):
                first = (c % 4) % n + (4 if n > 8 else 0)
                rows = [first] + [k for k in (first + 4, first + 5, first + 6, first + 7, n - 1) if first < k < n]
                h[r0 + np.array(rows), c] = top
        dup = seg_ptr[6]                                     # whole duplicated rows as well
        h[dup + 40:dup + 44] = h[dup + 20:dup + 24]
    return h, seg_ptr


def _pool_call(K, dev, h, seg_ptr, is_max):
    g, d = len(seg_ptr) - 1, h.shape[1]
    out = torch.full((g, d), float('nan'), device=dev)
    arg = torch.full((g, d), -7, device=dev, dtype=torch.int32)
    th, tp = _to(h, dev), _to(seg_ptr, dev)                  # (named: alive until the kernel has run)
    K._check(K.lib().renet_segment_pool_fwd(th.data_ptr(), tp.data_ptr(), g, d, int(is_max), out.data_ptr(), arg.data_ptr(),
                                            K._stream()), 'segment_pool_fwd')
    torch.cuda.synchronize()
    return out, arg


def _pool_bwd_call(K, dev, dout, seg_ptr, arg, is_max, n):
    g, d = dout.shape
    dh = torch.full((n, d), float('nan'), device=dev)
    td, tp = _to(dout, dev), _to(seg_ptr, dev)
    K._check(K.lib().renet_segment_pool_bwd(td.data_ptr(), tp.data_ptr(), arg.data_ptr(), g, d, int(is_max), n, dh.data_ptr(),
                                            K._stream()), 'segment_pool_bwd')
    torch.cuda.synchronize()
    return dh


@pytest.mark.parametrize('d', [100, 200, 300])
def test_segment_pool_max_is_exact_with_the_first_maximum(dev, d):
    import renet_hip as K
    h, seg_ptr = _pool_rows(d, ties=True)
    g = len(SEG_LENS)
    out, arg = _pool_call(K, dev, h, seg_ptr, True)
    want = np.stack([h[a:b].max(axis=0) for a, b in zip(seg_ptr[:-1], seg_ptr[1:])])
    want_arg = np.stack([a + np.argmax(h[a:b], axis=0) for a, b in zip(seg_ptr[:-1], seg_ptr[1:])]).astype(np.int32)
    # the planted ties are there: in the long segments the maximum occurs more than once, with winners in all four waves
    assert ((h[seg_ptr[7]:] == want[7]).sum(axis=0) > 1).all()
    assert set(((want_arg[7] - seg_ptr[7]) % 4).tolist()) == {0, 1, 2, 3}
    _assert_bits(_np(out), want, 'max values')
    assert np.array_equal(_np(arg), want_arg), np.nonzero(_np(arg) != want_arg)
    # wrapper: same result
    out2, arg2 = K.segment_pool_fwd(_to(h, dev), _to(seg_ptr, dev), g, True)
    assert torch.equal(out2, out) and torch.equal(arg2, arg)
    # backward: dout lands on the argmax row, exact zeros elsewhere
    dout = np.random.RandomState(d + 1).randn(g, d).astype(np.float32)
    dh = _pool_bwd_call(K, dev, dout, seg_ptr, arg, True, h.shape[0])
    ref = np.zeros_like(h)
    for gi in range(g):
        ref[want_arg[gi], np.arange(d)] = dout[gi]
    _assert_bits(_np(dh), ref, 'max backward')
    assert torch.equal(K.segment_pool_bwd(_to(dout, dev), _to(seg_ptr, dev), arg, g, True, h.shape[0]), dh)


@pytest.mark.parametrize('d', [100, 200, 300])
def test_segment_pool_mean_matches_fp64(dev, d):
    """Forward bound per column: len * 2^-24 * (sum |h|) / len -- every element passes through at most len / 4 + 3 adds and
    one division, each 2^-24 relative to a partial sum that sum |h| bounds, and the result is divided by len.  Backward:
    one division, 2^-23 relative."""
    import renet_hip as K
    h, seg_ptr = _pool_rows(d, ties=False)
    g = len(SEG_LENS)
    out, arg = _pool_call(K, dev, h, seg_ptr, False)
    h64 = h.astype(np.float64)
    worst = 0.0
    for gi, (a, b) in enumerate(zip(seg_ptr[:-1], seg_ptr[1:])):
        ref = h64[a:b].mean(axis=0)
        tol = (b - a) * U24 * np.abs(h64[a:b]).sum(axis=0) / (b - a)
        err = np.abs(_np(out)[gi].astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (gi, float((err / tol).max()))
    _report('segment_pool mean fwd D=%d' % d, worst)
    assert (_np(arg) == -7).all()                            # mean mode writes no argmax
    assert torch.equal(K.segment_pool_fwd(_to(h, dev), _to(seg_ptr, dev), g, False)[0], out)
    # an empty segment gives 0
    sp2 = np.array([0, 3, 3, 10], dtype=np.int32)
    out2, _ = _pool_call(K, dev, h[:10], sp2, False)
    assert not _np(out2)[1].any()
    for gi, (a, b) in ((0, (0, 3)), (2, (3, 10))):
        tol = U24 * np.abs(h64[a:b]).sum(axis=0)
        assert (np.abs(_np(out2)[gi] - h64[a:b].mean(axis=0)) <= tol).all()
    # backward
    dout = np.random.RandomState(d + 2).randn(g, d).astype(np.float32)
    dh = _pool_bwd_call(K, dev, dout, seg_ptr, arg, False, h.shape[0])
    ref = np.concatenate([np.repeat(dout[gi:gi + 1].astype(np.float64) / n, n, axis=0) for gi, n in enumerate(SEG_LENS)])
    err = np.abs(_np(dh).astype(np.float64) - ref)
    _report('segment_pool mean bwd D=%d' % d, float((err / (U23 * np.abs(ref))).max()))
    assert (err <= U23 * np.abs(ref)).all()


# ---------------------------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------------------------
def _fp32_branch(c):
    """softmax_ce_impl (csrc/seq.hip) for fp32 output."""
    if 4096 <= c <= 48 * 512:
        return 'reg16' if c <= 16 * 512 else 'reg32' if c <= 32 * 512 else 'reg48'
    if c * 4 <= 128 * 1024 and c >= 4096:
        return 'lds'
    return 'streamed'


def _bf16_branch(c):
    """softmax_ce_impl for bf16 output (the register kernels have no bf16 store)."""
    return 'lds' if c * 4 <= 128 * 1024 and c >= 4096 else 'streamed'


FP32_WIDTHS = [(1, 'streamed'), (2, 'streamed'), (255, 'streamed'), (257, 'streamed'), (4095, 'streamed'), (4096, 'reg16'),
               (4097, 'reg16'), (8191, 'reg16'), (8192, 'reg16'), (8193, 'reg32'), (16384, 'reg32'), (16385, 'reg48'),
               (24575, 'reg48'), (24576, 'reg48'), (24577, 'lds'), (40000, 'streamed')]
BF16_WIDTHS = [(1, 'streamed'), (63, 'streamed'), (65, 'streamed'), (4095, 'streamed'), (4096, 'lds'), (4097, 'lds'),
               (8191, 'lds'), (32767, 'lds'), (32768, 'lds'), (32769, 'streamed')]
FAMILIES = ('spike', 'shifted', 'wide', 'strided')
B_ROWS = 6


def test_softmax_width_ids_name_the_branch_the_dispatch_takes():
    assert all(_fp32_branch(c) == name for c, name in FP32_WIDTHS)
    assert all(_bf16_branch(c) == name for c, name in BF16_WIDTHS)
    assert {name for _, name in FP32_WIDTHS} == {'streamed', 'reg16', 'reg32', 'reg48', 'lds'}
    assert {name for _, name in BF16_WIDTHS} == {'streamed', 'lds'}


def _edges(c):
    return sorted({j for j in (0, 511, 512, 1023, c - 513, c - 512, c - 2, c - 1) if 0 <= j < c})


def _softmax_rows(c, family):
    """-> list of (logits [6, C] float32, target [6] int32) batches of one family.
    spike / strided: 0.1 randn with +12 on one edge column j; over the batches j runs through the whole edge set, the
      target is j in half of the rows and another edge column in the other half (each edge column in both roles).
    shifted: the spike rows minus 40, so that every logit is negative: an element that is not part of the row (a column
      >= C read as 0) would become the row maximum.
    wide: 20 randn, random target, two entries of -inf per row (never the target)."""
    rng = np.random.RandomState(c * 7 + len(family))
    if family == 'wide':
        x = (20.0 * rng.randn(B_ROWS, c)).astype(np.float32)
        t = rng.randint(0, c, B_ROWS).astype(np.int32)
        for b in range(B_ROWS):
            others = np.setdiff1d(np.arange(c) if c < 64 else rng.randint(0, c, 8), [t[b]])
            x[b, others[:2]] = -np.inf
        return [(x, t)]
    e = _edges(c)
    n = len(e)
    rows = _ceil(2 * n, B_ROWS)                             # one pass with target = j, one with the next edge column
    x = (0.1 * rng.randn(rows, c)).astype(np.float32)
    t = np.zeros(rows, dtype=np.int32)
    for r in range(rows):
        j = e[r % n]
        x[r, j] += np.float32(12.0)
        t[r] = j if (r // n) % 2 == 0 else e[(r + 1) % n]
    if family == 'shifted':
        x -= np.float32(40.0)
    return [(x[k:k + B_ROWS], t[k:k + B_ROWS]) for k in range(0, rows, B_ROWS)]


def _softmax_fp64(x, t, grad_scale):
    """float64 log-sum-exp; -> loss, gradient, and the bounds
    loss: (|m| + |x_t| + ln C + 32) 2^-23;  gradient: grad_scale (p (|x - m| + 32) 2^-23 + [c == t] 2^-23 + 2^-126)
    (argument rounding of x - m, a few ulp of expf, the per-thread serial sum, the reciprocal and the product)."""
    x64 = x.astype(np.float64)
    b, c = x64.shape
    m = x64.max(axis=1, keepdims=True)
    with np.errstate(invalid='ignore'):
        z = x64 - m
    e = np.exp(z)
    ssum = e.sum(axis=1, keepdims=True)
    p = e / ssum
    xt = x64[np.arange(b), t]
    loss = np.log(ssum[:, 0]) + m[:, 0] - xt
    onehot = np.zeros((b, c))
    onehot[np.arange(b), t] = 1.0
    grad = (p - onehot) * grad_scale
    loss_tol = (np.abs(m[:, 0]) + np.abs(xt) + math.log(c) + 32.0) * U23
    absz = np.where(p > 0, np.abs(z), 0.0)                  # (p = 0 at -inf: no 0 * inf)
    grad_tol = grad_scale * (p * (absz + 32.0) * U23 + onehot * U23 + 2.0 ** -126)
    return loss, grad, loss_tol, grad_tol, p


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('c,branch', FP32_WIDTHS, ids=['C%d-%s' % w for w in FP32_WIDTHS])
def test_softmax_ce_fp32_matches_fp64(dev, c, branch, family):
    import renet_hip as K
    assert _fp32_branch(c) == branch
    worst_loss = worst_grad = 0.0
    for x, t in _softmax_rows(c, 'spike' if family == 'strided' else family):
        tt = _to(t, dev)
        for gs in (1.0, 1.0 / 2048):
            loss_ref, grad_ref, loss_tol, grad_tol, p = _softmax_fp64(x, t, gs)
            assert np.isfinite(loss_ref).all()
            if family == 'wide' and c > 2:
                assert (p[np.isneginf(x)] == 0).all() and np.isneginf(x).sum() == 2 * B_ROWS
            if family == 'strided':                          # a view of a buffer with ld = C + 5, +inf beside every row
                buf = torch.full((B_ROWS, c + 5), float('inf'), device=dev)
                lg = buf[:, :c]
                lg.copy_(_to(x, dev))
                assert lg.stride(0) == c + 5
            else:
                lg = _to(x, dev)
            # loss only: the logits stay as they are
            loss0 = K.softmax_ce(lg, tt, gs, False)
            _assert_bits(_np(lg), x, 'logits after a loss-only call')
            # in place
            loss = K.softmax_ce(lg, tt, gs, True)
            assert torch.equal(loss, loss0)
            got_loss, got = _np(loss).astype(np.float64), _np(lg).astype(np.float64)
            assert np.isfinite(got_loss).all() and np.isfinite(got).all()
            if family == 'wide':
                assert (got[np.isneginf(x)] == 0).all()
            if family == 'strided':
                assert bool(torch.isposinf(buf[:, c:]).all())
                ref_run = _to(x, dev)                        # the contiguous run: same bits
                assert torch.equal(K.softmax_ce(ref_run, tt, gs, True), loss) and torch.equal(ref_run, lg)
            le, ge = np.abs(got_loss - loss_ref) / loss_tol, np.abs(got - grad_ref) / grad_tol
            worst_loss, worst_grad = max(worst_loss, float(le.max())), max(worst_grad, float(ge.max()))
            assert (le <= 1).all(), ('loss', c, family, gs, got_loss, loss_ref, float(le.max()))
            assert (ge <= 1).all(), ('gradient', c, family, gs, float(ge.max()), np.unravel_index(ge.argmax(), ge.shape))
    _report('softmax_ce fp32 C=%d (%s) %s: loss' % (c, branch, family), worst_loss)
    _report('softmax_ce fp32 C=%d (%s) %s: gradient' % (c, branch, family), worst_grad)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('c,branch', BF16_WIDTHS, ids=['C%d-%s' % w for w in BF16_WIDTHS])
def test_softmax_ce_bf16_matches_fp64_in_a_zero_padded_matrix(dev, c, branch, family):
    """renet_softmax_ce_bf16 into a NaN-prefilled padded buffer.  Logical block: within one bf16 rounding of the float64
    gradient, max(2^-8 |ref|, 2^-134), plus the fp32 bound (2^-134 is half the spacing 2^-133 of bf16 below 2^-126: with
    grad_scale = 2^-11 the wide rows put gradients there, where 2^-8 |ref| alone understates the format's rounding error
    by up to a factor 8); padding columns [C, min(ceil64(C), ld16)) of the rows < B and the rows
    [B, rows16) are zero; nothing else is written; the fp32 logits are not modified.  Two row strides: the one of
    renet_hip.bf16_empty (a multiple of 256) and an even one that ends inside the 64-column padding."""
    import renet_hip as K
    assert _bf16_branch(c) == branch
    rows_alloc, rows16 = 70, 64
    worst_loss = worst_grad = 0.0
    for x, t in _softmax_rows(c, 'spike' if family == 'strided' else family):
        tt = _to(t, dev)
        for gs, ld16 in ((1.0, _ceil(c, 256)), (1.0 / 2048, _ceil(c, 2) + 2)):
            loss_ref, grad_ref, loss_tol, grad_tol, _ = _softmax_fp64(x, t, gs)
            if family == 'strided':
                buf = torch.full((B_ROWS, c + 5), float('inf'), device=dev)
                lg = buf[:, :c]
                lg.copy_(_to(x, dev))
            else:
                lg = _to(x, dev)
            out = torch.full((rows_alloc, ld16), float('nan'), device=dev, dtype=torch.bfloat16)
            loss = torch.full((B_ROWS,), float('nan'), device=dev)
            K._check(K.lib().renet_softmax_ce_bf16(lg.data_ptr(), tt.data_ptr(), B_ROWS, c, lg.stride(0), gs, loss.data_ptr(),
                                                   out.data_ptr(), ld16, rows16, K._stream()), 'softmax_ce_bf16')
            _assert_bits(_np(lg), x, 'fp32 logits')
            if family == 'strided':
                assert bool(torch.isposinf(buf[:, c:]).all())
            # padding and sentinel: the expectation with the logical block taken from the result itself
            got16 = _bf16_bits(out)
            want = _bf16_padded_expectation(np.zeros((B_ROWS, c), dtype=np.float32), rows_alloc, ld16, rows16)
            want[:B_ROWS, :c] = got16[:B_ROWS, :c]
            _assert_bits(got16, want, 'padding / sentinel')
            got = _np(out[:B_ROWS, :c].float()).astype(np.float64)
            got_loss = _np(loss).astype(np.float64)
            assert np.isfinite(got).all() and np.isfinite(got_loss).all()
            le = np.abs(got_loss - loss_ref) / loss_tol
            ge = np.abs(got - grad_ref) / (np.maximum(2.0 ** -8 * np.abs(grad_ref), 2.0 ** -134) + grad_tol)
            worst_loss, worst_grad = max(worst_loss, float(le.max())), max(worst_grad, float(ge.max()))
            assert (le <= 1).all(), ('loss', c, family, gs, float(le.max()))
            assert (ge <= 1).all(), ('gradient', c, family, gs, float(ge.max()), np.unravel_index(ge.argmax(), ge.shape))
    _report('softmax_ce bf16 C=%d (%s) %s: loss' % (c, branch, family), worst_loss)
    _report('softmax_ce bf16 C=%d (%s) %s: gradient' % (c, branch, family), worst_grad)


# ---------------------------------------------------------------------------------------------
# fused Adam
# ---------------------------------------------------------------------------------------------
LR, BETA1, BETA2, EPS = 1e-2, 0.9, 0.999, 1e-8
ADAM_SIZES = [1, 3, 4, 5, 1023, 4 * 256 * 7 + 2, 4 * (2048 * 256) + 4 * 256 * 3 + 3]
# (clip, weight_decay, grad_scale, zero_grad); clip: 'active' (max_norm = 0.3 of the norm), 'inactive' (3 x), 'off' (0)
# the last case starts from m = v = 0 (the first training step) and runs step 1 only
ADAM_CASES = [('active', 1e-5, 1.0, 1), ('inactive', 0.0, 0.125, 0), ('off', 1e-5, 0.125, 1), ('active', 0.0, 0.125, 0),
              ('inactive', 1e-5, 1.0, 1), ('off', 0.0, 1.0, 0), ('off', 1e-5, 1.0, 1)]
G_SCALE = 0.002


def _f(v):
    """The float32 value of a hyper-parameter as float64: what the C ABI (float arguments) hands to the kernel."""
    return float(np.float32(v))


def _adam_fp64(p, g, m, v, max_norm, wd, gs, step):
    """clip_grad_norm_ (norm of the scaled gradient, coefficient min(max_norm / (norm + 1e-6), 1)) followed by
    torch.optim.Adam with L2 weight decay, in float64, on the hyper-parameters' float32 values."""
    lr, b1, b2, eps, wd, max_norm, gs = _f(LR), _f(BETA1), _f(BETA2), _f(EPS), _f(wd), _f(max_norm), _f(gs)
    norm = gs * math.sqrt(float((g * g).sum()))
    coef = min(max_norm / (norm + _f(1e-6)), 1.0) if max_norm > 0 else 1.0
    ge = g * (coef * gs) + wd * p
    m = b1 * m + (1.0 - b1) * ge
    v = b2 * v + (1.0 - b2) * ge * ge
    denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + eps
    p = p - (lr / (1.0 - b1 ** step)) * (m / denom)
    return p, m, v, norm


def _adam_state(rng, n, fresh):
    """Random p, m, v >= 0.  The moments are kept away from cancellation so that the purely RELATIVE tolerances on m and v
    are valid: |m| in [0.02, 0.06] of either sign against gradients G_SCALE randn (|0.1 g| < 0.0011 over 2.1 M draws, so
    over four steps |0.9 m| stays above 0.0085, |m'| >= 0.78 (|0.9 m| + |0.1 g|), and the three roundings of 2^-24 of
    m' = b1 m + (1 - b1) g stay below 3e-7 relative); v in [0.5e-3, 1.5e-3] (all terms of v' are positive).
    fresh: m = v = 0, the state before the first training step (m' and v' are then single products)."""
    p = rng.randn(n)
    m = rng.choice([-1.0, 1.0], n) * rng.uniform(0.02, 0.06, n)
    v = rng.uniform(0.5e-3, 1.5e-3, n)
    if fresh:
        m, v = np.zeros(n), np.zeros(n)
    return [a.astype(np.float32) for a in (p, m, v)]


def _adam_check(what, got, ref, rtol, atol):
    got = _np(got).astype(np.float64)
    err = np.abs(got - ref)
    tol = atol + rtol * np.abs(ref)
    assert (err <= tol).all(), (what, float((err / tol).max()), int((err / tol).argmax()))
    return float((err / tol).max())


@pytest.mark.parametrize('n', ADAM_SIZES, ids=['n%d' % n for n in ADAM_SIZES])
def test_fused_adam_matches_fp64_clip_and_adam(dev, n):
    """Three consecutive steps (and one call at step 1000) per case; tolerances of
    test_fused_adam_matches_torch_adam_with_clipping: parameters rtol 2e-5 / atol 2e-7, norm relative 1e-5; m, v rtol 1e-5."""
    import renet_hip as K
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0, 'norm': 0.0}
    for k, (clip, wd, gs, zero_grad) in enumerate(ADAM_CASES):
        rng = np.random.RandomState(n % 100000 + k)
        fresh = k == len(ADAM_CASES) - 1
        p, m, v = _adam_state(rng, n, fresh)
        tp, tm, tv = _to(p, dev), _to(m, dev), _to(v, dev)
        p64, m64, v64 = (a.astype(np.float64) for a in (p, m, v))
        steps = [1] if fresh else [1, 2, 3] if k % 2 else [1, 2, 3, 1000]
        for step in steps:
            g = (G_SCALE * rng.randn(n)).astype(np.float32)
            g64 = g.astype(np.float64)
            norm_true = gs * math.sqrt(float((g64 * g64).sum()))
            max_norm = {'active': 0.3, 'inactive': 3.0, 'off': 0.0}[clip] * norm_true
            tg = _to(g, dev)
            norm_out = torch.full((1,), float('nan'), device=dev)
            K.adam_step(tp, tg, tm, tv, LR, BETA1, BETA2, EPS, wd, max_norm, step, zero_grad=bool(zero_grad),
                        norm_out=norm_out, grad_scale=gs)
            # the reference advances from the kernel's own state of the step before (float32 values)
            p_ref, m_ref, v_ref, norm_ref = _adam_fp64(p64, g64, m64, v64, max_norm, wd, gs, step)
            if clip == 'active':
                assert _f(max_norm) < norm_ref
            what = 'n=%d case=%d step=%d ' % (n, k, step)
            if norm_ref > 0:
                rel = abs(float(norm_out) - norm_ref) / norm_ref
                assert rel <= 1e-5, (what, float(norm_out), norm_ref)
                worst['norm'] = max(worst['norm'], rel / 1e-5)
            worst['p'] = max(worst['p'], _adam_check(what + 'p', tp, p_ref, 2e-5, 2e-7))
            worst['m'] = max(worst['m'], _adam_check(what + 'm', tm, m_ref, 1e-5, 0.0))
            worst['v'] = max(worst['v'], _adam_check(what + 'v', tv, v_ref, 1e-5, 0.0))
            if zero_grad:
                assert not _np(tg).any(), what
            else:
                _assert_bits(_np(tg), g, what + 'gradient kept')
            p64, m64, v64 = (_np(t).astype(np.float64) for t in (tp, tm, tv))
    for key in ('p', 'm', 'v', 'norm'):
        _report('adam n=%d: %s' % (n, key), worst[key])


@pytest.mark.parametrize('zero_grad', [1, 0])
def test_presummed_adam_equals_the_unfused_call(dev, zero_grad):
    """renet_sumsq_partials over two regions of one flat gradient into one partial array (more slots than the regions
    need: the spare ones come out 0), then renet_adam_step_presummed on the partials."""
    import renet_hip as K
    n, n1 = 4 * 256 * 7 + 2, 4 * 256 * 3
    rng = np.random.RandomState(77)
    p, m, v = _adam_state(rng, n, False)
    g = (G_SCALE * rng.randn(n)).astype(np.float32)
    g64 = g.astype(np.float64)
    sumsq = float((g64 * g64).sum())
    gs, wd, step = 0.125, 1e-5, 2
    max_norm = 0.3 * gs * math.sqrt(sumsq)

    def run(presummed):
        tp, tg, tm, tv = (_to(a, dev) for a in (p, g, m, v))
        norm_out = torch.full((1,), float('nan'), device=dev)
        part = None
        if presummed:
            part = torch.full((16,), float('nan'), device=dev)
            K.sumsq_partials(tg[:n1], part, 0, 5)            # 3 workgroups of work in 5 slots
            K.sumsq_partials(tg[n1:], part, 5, 6)            # 4 workgroups + a 2-element tail in 6 slots
        K.adam_step(tp, tg, tm, tv, LR, BETA1, BETA2, EPS, wd, max_norm, step, zero_grad=bool(zero_grad), norm_out=norm_out,
                    grad_scale=gs, presummed=(part, 11) if presummed else None)
        return [_np(t) for t in (tp, tg, tm, tv, norm_out)] + [None if part is None else _np(part)]

    plain, pre, pre2 = run(False), run(True), run(True)
    part = pre[5]
    assert not part[[3, 4, 9, 10]].any() and np.isnan(part[11:]).all() and (part[[0, 1, 2, 5, 6, 7, 8]] > 0).all()
    assert abs(float(part[:11].astype(np.float64).sum()) - sumsq) <= 1e-5 * sumsq
    assert abs(float(part[:5].astype(np.float64).sum()) - float((g64[:n1] ** 2).sum())) <= 1e-5 * float((g64[:n1] ** 2).sum())
    for a, b in zip(pre[:5], pre2[:5]):                      # two identical calls: the same bits
        _assert_bits(a, b, 'presummed twice')
    p_ref, m_ref, v_ref, norm_ref = _adam_fp64(p.astype(np.float64), g64, m.astype(np.float64), v.astype(np.float64),
                                               max_norm, wd, gs, step)
    for res in (plain, pre):
        assert abs(float(res[4][0]) - norm_ref) <= 1e-5 * norm_ref
        assert (np.abs(res[0] - p_ref) <= 2e-7 + 2e-5 * np.abs(p_ref)).all()
        assert (np.abs(res[2] - m_ref) <= 1e-5 * np.abs(m_ref)).all()
        assert (np.abs(res[3] - v_ref) <= 1e-5 * np.abs(v_ref)).all()
        if zero_grad:
            assert not res[1].any()
        else:
            _assert_bits(res[1], g, 'gradient kept')
    np.testing.assert_allclose(pre[0], plain[0], rtol=2e-5, atol=2e-7)
    np.testing.assert_allclose(pre[2], plain[2], rtol=1e-5, atol=0)
    np.testing.assert_allclose(pre[3], plain[3], rtol=1e-5, atol=0)
