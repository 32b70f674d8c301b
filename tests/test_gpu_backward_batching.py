"""The batched small launches of the encoder backward (RENET_STEP_BATCH, csrc/step.cpp) against the launches they replace:

  renet_segment_add_multi  several two-stage segmented adds in one launch: equal to renet_add_inplace + renet_segment_add
                           calls issued one by one, bit for bit; `overwrite` equal to renet_zero + renet_segment_add
  renet_gru_split_weights / renet_gru_{fwd,bwd}_layouts_presplit
                           the W_hh split issued on a second stream, ordered by an event: the recurrences' outputs
                           torch.equal to the plain entries'
  the whole step           child processes with RENET_STEP_BATCH = 0 (one launch per sum) against 6 (default) and each single
                           bit: losses equal, flat gradients and parameters torch.equal

Operands are randn: integer operands are exact in any order and would hide a changed order of additions.  The results are
also held to the float64 statements of tests/reduction_statements.py (error / bound <= 1; the bound holds for any order, so
it says that nothing was dropped or doubled, the bit comparison that the order is the old one).  Outputs and workspaces carry
quiet-NaN fences, workspaces have exactly the size the library asks for, refused calls leave every buffer untouched."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reduction_statements as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 0x7fc0dead                                    # a quiet NaN no kernel produces
TAIL = 8
SPARE = 2


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _to(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _as_f32(buf):
    return buf.view(torch.float32)


def _within(got, ref, n, mag, what):
    q = R.ratio(got, ref, n, mag)
    w = float(q.max()) if q.size else 0.0
    assert w <= 1.0, '%s: error / bound = %.3g (%d of %d elements over)' % (what, w, int((q > 1).sum()), q.size)
    return w


# ---------------------------------------------------------------------------------------------
# 1. renet_segment_add_multi
# ---------------------------------------------------------------------------------------------
SEG_US = [1, 17, 513, 8198]
SEG_DS = [100, 200, 300, 400]


class _Plan(object):
    def __init__(self, lay, dev):
        self.order, self.seg_ptr, self.target = (_to(lay[k], dev) for k in ('order', 'seg_ptr', 'seg_target'))
        self.num_segments = lay['U']


def _rows(values, dev, rows=None):
    """[rows + SPARE, D] int32 PATTERN buffer with `values` in its first rows -> (buffer, float view of the rows)"""
    v = _to(np.ascontiguousarray(values, np.float32), dev)
    buf = torch.full((v.shape[0] + SPARE, v.shape[1]), PATTERN, dtype=torch.int32, device=dev)
    buf[:v.shape[0]] = _bits(v)
    return buf, _as_f32(buf)[:v.shape[0]]


def _third(u_n, d, n_src):
    return np.random.RandomState(11 * u_n + d).randn(n_src, d).astype(np.float32)


def _sequential(dev, plan, old, a0, a1, b):
    """what the merged job replaces: a0 += a1, then one renet_segment_add per stage"""
    import renet_hip as K
    buf, dst = _rows(old, dev)
    a = a0.clone()
    if a1 is not None:
        K.lib().renet_add_inplace(a.data_ptr(), a1.data_ptr(), a.numel(), K._stream())
    K.segment_add(a, plan, dst)
    if b is not None:
        K.segment_add(b, plan, dst)
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize('u_n', SEG_US)
@pytest.mark.parametrize('d', SEG_DS)
def test_segment_add_multi_two_stage_job_equals_the_calls_it_replaces(dev, d, u_n):
    """segments of 0 .. 1000 rows across the one-wave / whole-workgroup threshold (16 | 17), U across the grid formula (one
    workgroup per segment up to 512, 16 per workgroup beyond: short and long segments share a workgroup), D = 300 with its
    lane tail; every form of a job (a0 | a0 + a1) x (no stage B | stage B).  Bound: a row of 3 len + 1 terms (old, len
    rows of a0, a1 and b each) summed in some binary tree -- a0 + a1 at load is one of its additions -- so
    gamma(3 len + 3) * sum |terms|, the statement's bound for that many terms."""
    import renet_hip as K
    lay, src0, src1, old0, _ = R.segment_case(u_n, d, 'randn')
    plan = _Plan(lay, dev)
    a0, a1, b = _to(src0, dev), _to(src1, dev), _to(_third(u_n, d, lay['n_src']), dev)
    zeros = np.zeros_like(old0)
    for use_a1 in (False, True):
        for use_b in (False, True):
            what = 'U=%d D=%d a1=%d b=%d' % (u_n, d, use_a1, use_b)
            want = _sequential(dev, plan, old0, a0, a1 if use_a1 else None, b if use_b else None)
            buf, dst = _rows(old0, dev)
            keep = a0.clone()
            rc = K.segment_add_multi([(plan, dst, a0, a1 if use_a1 else None, b if use_b else None, False)])
            torch.cuda.synchronize()
            assert rc == 0, (what, rc)
            assert torch.equal(buf, want), what + ': differs from add_inplace + segment_add calls (or wrote a fence row)'
            assert torch.equal(a0, keep), what + ': a0 was modified'
            ref, mag, n = R.segment_add_statement(src0, lay, old0)
            for s, used in ((src1, use_a1), (b.cpu().numpy(), use_b)):
                if used:
                    r2, m2, n2 = R.segment_add_statement(s, lay, zeros)
                    ref, mag, n = ref + r2, mag + m2, n + np.maximum(n2 - 1, 0)
            got = buf[:lay['n_dst']].cpu().numpy().view(np.float32)
            untouched = n == 0
            assert np.array_equal(got[untouched].view(np.uint32), old0[untouched].view(np.uint32)), what + ': a row no segment targets'
            _within(got, ref, n[:, None], mag, what)


def test_segment_add_multi_three_jobs_equal_the_same_calls_issued_separately(dev):
    """the step's shape of a call: (b-stage job, a0 + a1 + b job, overwrite job) over three different plans and widths of
    grid in ONE launch, against the three jobs issued one by one"""
    import renet_hip as K
    d = 200
    cases = []
    for u_n in (17, 513, 8198):
        lay, src0, src1, old0, _ = R.segment_case(u_n, d, 'randn')
        cases.append((_Plan(lay, dev), old0, _to(src0, dev), _to(src1, dev), _to(_third(u_n, d, lay['n_src']), dev)))
    lay_o = R.segment_layout(R.segment_lengths(600), 1500, seed=5, spare=0)           # names every row of its dst
    src_o = np.random.RandomState(5).randn(1500, d).astype(np.float32)
    forms = [(0, False, True), (1, True, True), (2, False, False)]                     # (case, a1, b)
    together, apart = [], []
    for bufs in (together, apart):
        jobs = []
        for i, use_a1, use_b in forms:
            plan, old, a0, a1, b = cases[i]
            buf, dst = _rows(old, dev)
            bufs.append(buf)
            jobs.append((plan, dst, a0, a1 if use_a1 else None, b if use_b else None, False))
        buf, dst = _rows(np.full((600, d), np.nan, np.float32), dev)                  # overwrite: the old rows are not read
        bufs.append(buf)
        jobs.append((_Plan(lay_o, dev), dst, _to(src_o, dev), None, None, True))
        if bufs is together:
            assert K.segment_add_multi(jobs) == 0
        else:
            for j in jobs:
                assert K.segment_add_multi([j]) == 0
        torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(together, apart)):
        assert torch.equal(x, y), 'job %d of the merged call differs from the job alone' % k
    for i, use_a1, use_b in forms:                                                      # ... and from the replaced calls
        plan, old, a0, a1, b = cases[i]
        assert torch.equal(together[forms.index((i, use_a1, use_b))],
                           _sequential(dev, plan, old, a0, a1 if use_a1 else None, b if use_b else None))


@pytest.mark.parametrize('d', [100, 300])
def test_segment_add_multi_overwrite_equals_zero_then_add(dev, d):
    """a plan that names every row of dst (segments of every length, empty ones included), dst prefilled with NaN: equal to
    renet_zero + renet_segment_add bit for bit -- a segment whose rows are all -0.0 gives +0.0 (0.f + sum), an empty segment
    +0.0; with a stage B on top"""
    import renet_hip as K
    u_n = 600
    lay = R.segment_layout(R.segment_lengths(u_n), 1500, seed=9, spare=0)
    rng = np.random.RandomState(d)
    src, srcb = rng.randn(1500, d).astype(np.float32), rng.randn(1500, d).astype(np.float32)
    ptr = lay['seg_ptr']
    for u in (2, 3, 4):                                   # segments of 17, 1 and 257 rows: only -0.0 terms
        assert ptr[u + 1] > ptr[u]
        lay['order'][ptr[u]:ptr[u + 1]] = 7 + u
        src[7 + u] = -0.0
    others = np.ones(len(lay['order']), bool)
    others[ptr[2]:ptr[5]] = False
    clash = np.isin(lay['order'], (9, 10, 11)) & others
    lay['order'][clash] = 12                              # the -0.0 rows belong to those three segments only
    plan = _Plan(lay, dev)
    a, b = _to(src, dev), _to(srcb, dev)
    for use_b in (False, True):
        wbuf, wdst = _rows(np.full((u_n, d), np.nan, np.float32), dev)
        K.lib().renet_zero(wdst.data_ptr(), wdst.numel(), K._stream())
        K.segment_add(a, plan, wdst)
        if use_b:
            K.segment_add(b, plan, wdst)
        buf, dst = _rows(np.full((u_n, d), np.nan, np.float32), dev)
        rc = K.segment_add_multi([(plan, dst, a, None, b if use_b else None, True)])
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(buf, wbuf), 'overwrite differs from zero-then-add (stage B: %d)' % use_b
        if not use_b:
            t = lay['seg_target'][[2, 3, 4]]
            assert bool((buf[_to(t.astype(np.int64), dev)] == 0).all()), 'a sum of -0.0 terms must come out as +0.0'
        ref, mag, n = R.segment_add_statement(src, lay, np.zeros((u_n, d), np.float32))
        if use_b:
            r2, m2, n2 = R.segment_add_statement(srcb, lay, np.zeros((u_n, d), np.float32))
            ref, mag, n = ref + r2, mag + m2, n + np.maximum(n2 - 1, 0)
        _within(buf[:u_n].cpu().numpy().view(np.float32), ref, n[:, None], mag, 'overwrite D=%d b=%d' % (d, use_b))


def test_segment_add_multi_refusals_come_before_any_launch(dev):
    import renet_hip as K
    d = 100
    lay, src0, src1, old0, old1 = R.segment_case(17, d, 'randn')
    plan = _Plan(lay, dev)
    a0, a1 = _to(src0, dev), _to(src1, dev)

    def call(jobs_of, n=None, d_arg=None):
        bufs = [_rows(old0, dev), _rows(old1, dev)]
        jobs = jobs_of(bufs[0][1], bufs[1][1])
        if n is not None or d_arg is not None:
            arr = (K.SegAddJobC * 8)()
            for j in arr:
                j.order, j.seg_ptr, j.seg_target, j.U = plan.order.data_ptr(), plan.seg_ptr.data_ptr(), plan.target.data_ptr(), 17
                j.dst, j.dst_rows, j.a0 = bufs[0][1].data_ptr(), lay['n_dst'], a0.data_ptr()
            rc = K.lib().renet_segment_add_multi(1 if n is None else n, ctypes.addressof(arr), d if d_arg is None else d_arg,
                                                 K._stream())
        else:
            rc = K.segment_add_multi(jobs)
        torch.cuda.synchronize()
        want0, want1 = _rows(old0, dev)[0], _rows(old1, dev)[0]
        assert torch.equal(bufs[0][0], want0) and torch.equal(bufs[1][0], want1), 'a refused call wrote a destination'
        return rc

    assert call(lambda x, y: [(plan, x, a0, None, None, False), (plan, x, a1, None, None, False)]) == -1     # one dst twice
    assert call(lambda x, y: [(plan, x, a0, None, None, False), (plan, y, a0, a1, None, True)]) == -1        # U != rows of dst
    assert call(lambda x, y: [], n=5) == -1
    assert call(lambda x, y: [], n=0) == -1
    assert call(lambda x, y: [], d_arg=6) == -1
    assert call(lambda x, y: [], d_arg=516) == -2
    empty = _Plan(dict(order=np.zeros(0, np.int32), seg_ptr=np.zeros(1, np.int32), seg_target=np.zeros(0, np.int32), U=0), dev)
    assert call(lambda x, y: [(empty, x, a0, None, None, False)]) == 0                                          # a no-op


# ---------------------------------------------------------------------------------------------
# 2. the W_hh split as a call of its own
# ---------------------------------------------------------------------------------------------
def _offsets(batch_sizes):
    off = np.concatenate(([0], np.cumsum(batch_sizes))).astype(np.int32)
    return (ctypes.c_int32 * len(off))(*off)


@pytest.mark.parametrize('shared', [False, True], ids=['distinct-weights', 'shared-weights'])
@pytest.mark.parametrize('h', [100, 200, 300, 400])
def test_gru_with_the_split_on_a_second_stream_equals_the_plain_entries(dev, h, shared):
    """two problems of two packed layouts (33 and 17 sequences, 3 steps of shrinking batch), W_hh distinct or one shared
    pointer (split once, into the slot of the first): the split runs on a second stream, an event orders the recurrence
    behind it; h_last, saved, dGi and dGh torch.equal to renet_gru_{fwd,bwd}_layouts"""
    import renet_hip as K
    gen = torch.Generator().manual_seed(100 + h)
    offs = [_offsets([33, 20, 7]), _offsets([17, 9, 4])]
    rows = [33, 17]
    s_n = [60, 30]
    mk = lambda *shape: (torch.randn(*shape, generator=gen)).to(dev)
    gis = [mk(s, 3 * h) for s in s_n]
    w = [mk(3 * h, h) * 0.1, mk(3 * h, h) * 0.1]
    whhs = [w[0], w[0] if shared else w[1]]
    bhhs = [mk(3 * h) * 0.1, mk(3 * h) * 0.1]
    dhs = [mk(r, h) for r in rows]
    hs, svs = K.gru_fwd_layouts(gis, offs, h, whhs, bhhs, rows)
    dgis, dghs = K.gru_bwd_layouts(dhs, offs, h, whhs, svs)
    torch.cuda.synchronize()

    lib = K.lib()
    nbytes = 2 * lib.renet_gru_workspace(33, h)
    ws = torch.full((nbytes // 4 + TAIL,), PATTERN, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    so, ls = K._offs(offs)

    def split(backward):
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            rc = K.gru_split_weights(whhs, h, backward, ws, nbytes)
            ev = torch.cuda.Event()
            ev.record(side)
        assert rc == 0, rc
        torch.cuda.current_stream(dev).wait_event(ev)

    split(False)
    hs2 = [torch.empty_like(t) for t in hs]
    svs2 = [torch.empty_like(t) for t in svs]
    rc = lib.renet_gru_fwd_layouts_presplit(2, K._ptrs(gis), so, ls, h, K._ptrs(whhs), K._ptrs(bhhs), K._ptrs(hs2),
                                            (ctypes.c_int * 2)(*rows), K._ptrs(svs2), ws.data_ptr(), nbytes, K._stream())
    assert rc == 0, rc
    split(True)
    dgis2 = [torch.empty_like(t) for t in dgis]
    dghs2 = [torch.empty_like(t) for t in dghs]
    rc = lib.renet_gru_bwd_layouts_presplit(2, K._ptrs(dhs), so, ls, h, K._ptrs(whhs), K._ptrs(svs), K._ptrs(dgis2),
                                            K._ptrs(dghs2), ws.data_ptr(), nbytes, K._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((ws[nbytes // 4:] == PATTERN).all()), 'written behind the workspace'
    for name, xs, ys in (('h_last', hs, hs2), ('saved', svs, svs2), ('dGi', dgis, dgis2), ('dGh', dghs, dghs2)):
        for k, (x, y) in enumerate(zip(xs, ys)):
            assert float(x.abs().max()) > 0
            assert torch.equal(x, y), '%s of problem %d differs from the plain entry (H = %d)' % (name, k, h)
    # refusals: before any launch
    fence = ws.clone()
    assert K.gru_split_weights(whhs, h, False, ws, 2 * lib.renet_gru_workspace(0, h) - 4) == -3     # (the planes' slots only)
    assert lib.renet_gru_split_weights(5, K._ptrs(whhs), h, 0, ws.data_ptr(), nbytes, K._stream()) == -1
    assert K.gru_split_weights(whhs, 128, False, ws, nbytes) == -2
    torch.cuda.synchronize()
    assert torch.equal(ws, fence)


# ---------------------------------------------------------------------------------------------
# 3. the whole step: RENET_STEP_BATCH = 0 against the default and against every single bit
# ---------------------------------------------------------------------------------------------
H200 = ['200:40:256:3:2', '200:40:256:3:1']                                      # hidden:timestamps:batch:steps:streams
OTHERS = ['%d:24:128:2:%d' % (h, s) for h in (100, 300, 400) for s in (2, 1)]
_runs = {}


def _step_run(mask, tmp_path_factory):
    """the child's results for RENET_STEP_BATCH = mask (one child per mask, shared by the tests)"""
    if mask not in _runs:
        out = str(tmp_path_factory.mktemp('step_batch') / ('mask%d.pt' % mask))
        configs = H200 + (OTHERS if mask in (0, 6) else [])
        env = dict(os.environ, RENET_STEP_BATCH=str(mask))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'step_batch_run.py'), out] + configs, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (mask, r.stdout[-2000:], r.stderr[-4000:])
        _runs[mask] = torch.load(out)
    return _runs[mask]


@pytest.mark.parametrize('mask', [6, 2, 4])
def test_whole_step_is_bit_identical_to_the_unbatched_launch_list(dev, mask, tmp_path_factory):
    """40 timestamps, batch 256, hidden 200, 3 optimizer steps, and (all parts together) 24 timestamps, batch 128, 2 steps
    for hidden 100, 300, 400; dropout 0.5; two streams and one.  Losses equal, flat gradients and parameters torch.equal;
    the batched list really ran, by its launch counts: the segmented adds are 6 entries fewer (5 where the zero pass of
    d_h2 stays), the splits 1 more per direction."""
    base, new = _step_run(0, tmp_path_factory), _step_run(mask, tmp_path_factory)
    assert set(new) <= set(base) and len(new) >= 2
    for c in new:
        (l0, f0, p0, n0), (l1, f1, p1, n1) = base[c], new[c]
        assert l0 == l1, (c, l0, l1)
        assert len(f0) == len(f1)
        for x, y in zip(f0, f1):
            assert float(x.abs().max()) > 0
            assert torch.equal(x, y), c
        assert torch.equal(p0, p1), c
        fwd = n0[0] + (1 if mask & 4 else 0)
        assert n1[0] == fwd, (c, n0, n1)
        lo = n0[1] - (6 if mask & 2 else 0) + (1 if mask & 4 else 0)
        assert lo <= n1[1] <= lo + (1 if mask & 2 else 0), (c, n0, n1)
        assert 15 <= n1[0] <= 40 and 25 <= n1[1] <= 60, n1
