"""GPU tests of the gather-SpMM family (csrc/rgcn_items.hip, csrc/rgcn_csr.hip) through the C ABI against the host statement
of tests/gather_statement.py: BIT FOR BIT on integer operands every format holds exactly, and within the derived bound
(kept_deg * si + 3) * 2^-24 * mag at every element on float operands -- on ONE census graph that contains every structural
edge of the kernels by construction (tests/test_gather_statement_cpu.py asserts that it does), for the five launch classes of
a training step, D in {100, 200, 300, 400}, three plans, fp32 / bf16-W / bf16-table storage, the plain-CSR entry with and
without its hub list, a hand-built group of exactly 64 items, every RENET_GATHER_UNR instantiation, and the second row group
of a wave in the plain-CSR kernel.

Measured on the MI355X (profiles/gather_statement.md): every integer case bit for bit; worst error / bound of the float cases
0.42 (item entries, fp32 and bf16 storage alike), 0.42 (plain CSR) and 0.13 (the 64-item group); the whole file runs in 14 s,
12.5 s of them the five child processes of the UNR variants (one interpreter + HIP start each)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gather_statement as GS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), 're-net_amd')
WIDTHS = (100, 200, 300, 400)
# RENET_GATHER_UNR -> the widths that have an instantiation for it.  The library has no query for the UNR that ran: this
# table restates csrc/rgcn_items.hip, gather_items_impl (the three launch_items_unr<SI, DFLT, ALT...> lines); any other
# (value, width) pair silently runs the width's default, which the in-process tests cover.
UNR_WIDTHS = {2: (200,), 3: (300, 400), 4: (100, 200, 300, 400), 6: (200,), 8: (100, 200)}
ITEM_CLASSES = {'fp32': GS.CLASSES, 'w16': ('fwd_full', 'fwd_pruned', 'bwd_full', 'bwd_pruned'), 'table16': ('fwd_table',)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


class Census(object):
    """The census graph on the device under every plan, the launches of the five classes through the Python wrappers of the
    C ABI, and the statement of every launch (computed once per class / width / operand kind and shared)."""

    def __init__(self, dev):
        self.dev, self._graphs, self._refs, self.worst = dev, {}, {}, {}

    def to(self, a):
        return None if a is None else torch.from_numpy(np.array(a)).to(self.dev)

    def graph(self, plan, op):
        """(HostBatch, DeviceGraph); the integer operands put their power-of-two scale into hb.norm first."""
        import graph as G
        key = (plan, op.kind)
        if key not in self._graphs:
            hb = GS.host_batch(*plan, scale=op.scale)
            self._graphs[key] = (hb, G.DeviceGraph(hb, self.dev))
        return self._graphs[key]

    def case(self, cls, op, drop_on, shift):
        return GS.launch_case(cls, op, self.graph(GS.PLANS[0], op)[0].norm, drop_on=drop_on, shift=shift)

    def reference(self, cls, op, drop_on, shift, storage):
        """statement of the case; bf16 storage: on the bf16-rounded W (and table)."""
        key = (cls, op.kind, op.d, bool(drop_on), shift, storage)
        if key not in self._refs:
            c = self.case(cls, op, drop_on, shift)
            w = op.w if storage == 'fp32' else GS.round_bf16(op.w)
            x = GS.round_bf16(c.x) if storage == 'table16' else None
            self._refs[key] = GS.case_statement(c, w, x=x)
        return self._refs[key]

    def launch(self, entry, cls, op, plan, storage='fp32', drop_on=True, shift=None, hubs=True):
        """-> (output [n_rows, d], the three guard rows behind it) as numpy arrays."""
        import renet_hip as K
        c = self.case(cls, op, drop_on, shift)
        g = self.graph(plan, op)[1]
        x, w = self.to(c.x), self.to(op.w)
        buf = torch.full((c.n_rows + 3, op.d), float('nan'), device=self.dev)
        out = buf[:c.n_rows]
        if c.out0 is not None:
            out.copy_(self.to(c.out0))
        addend = out if c.out0 is not None else self.to(c.addend)
        w16 = K.pack_bf16(w) if storage != 'fp32' else None
        if entry == 'csr':
            heavy = (g.heavy_rows_out if c.n_rows < g.N else g.heavy_rows) if hubs else None
            K.rgcn_gather(x, g.row_ptr, g.col, g.etype, g.norm if c.use_norm else None, w, c.shift, c.tr, addend, c.p,
                          c.seed, c.relu, out, heavy, g.heavy_thresh if hubs else 0, c.src_limit, c.addend_rows)
        elif cls == 'fwd_table':
            K.rgcn_gather_items_table(x, g, w, c.shift, addend, c.p, c.seed, c.relu, out,
                                      table16=K.pack_bf16(x) if storage == 'table16' else None, w16=w16)
        else:
            K.rgcn_gather_items(x, g, w, c.shift, c.tr, addend, c.p, c.seed, c.relu, out, use_norm=c.use_norm,
                                pruned=c.pruned, src_limit=c.src_limit, addend_rows=c.addend_rows, w16=w16)
        torch.cuda.synchronize()
        res = buf.cpu().numpy()
        return res[:c.n_rows], res[c.n_rows:]

    def check(self, entry, cls, op, plan, storage='fp32', drop_on=True, shift=None, hubs=True):
        got, guard = self.launch(entry, cls, op, plan, storage, drop_on, shift, hubs)
        ref, mag, deg = self.reference(cls, op, drop_on, shift, storage)
        what = '%s %s D=%d %s plan=%s drop=%s shift=%s hubs=%s %s' % (entry, cls, op.d, storage, plan, drop_on, shift, hubs,
                                                                      op.kind)
        if op.kind == 'int':
            GS.assert_exact(got, ref, untouched=guard, what=what)
        else:
            assert np.isnan(guard).all(), what
            r = GS.assert_within_bound(got, ref, mag, deg, op.d // 100, what=what)
            key = (entry, cls, op.d, storage)
            old = GS.old_ratio(got, ref)
            self.worst[key] = tuple(max(a, b) for a, b in zip(self.worst.get(key, (0.0, 0.0)), (r, old)))

    def report(self):
        for (entry, cls, d, storage), (r, old) in sorted(self.worst.items()):
            print('gather-bound entry=%s class=%s D=%d storage=%s ratio=%.3f old=%.5f' % (entry, cls, d, storage, r, old))
        self.worst = {}

    def run_items(self, d, storage, kinds=('int', 'float')):
        """Every launch class of `storage` under the three plans (dropout on under the first and last, off under the
        second), the full backward at type_shift 3 and T - 1."""
        for kind in kinds:
            op = GS.int_operands(d) if kind == 'int' else GS.float_operands(d)
            for k, plan in enumerate(GS.PLANS):
                for cls in ITEM_CLASSES[storage]:
                    for shift in ((3, GS.T - 1) if cls == 'bwd_full' else (None,)):
                        self.check('items', cls, op, plan, storage, drop_on=k != 1, shift=shift)


_CENSUS = []


@pytest.fixture(scope='module')
def census(dev):
    if not _CENSUS:
        _CENSUS.append(Census(dev))
    return _CENSUS[0]


# ---------------------------------------------------------------------------------------------
# the item entries on the census graph
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage', ['fp32', 'w16', 'table16'])
@pytest.mark.parametrize('d', WIDTHS)
def test_item_entries_on_the_census(census, d, storage):
    """renet_rgcn_gather_items / _items_table and their bf16-storage forms: exact on the integer operands, within the derived
    bound on the float operands (bf16 storage: against the statement on the bf16-rounded W and table)."""
    import renet_hip as K
    if storage != 'fp32' and d == 300:                         # no bf16 storage of 3x3 blocks: the entry answers unsupported
        op = GS.int_operands(d)
        for cls in ITEM_CLASSES[storage]:
            with pytest.raises(K.RenetHipError, match='code -2'):
                census.launch('items', cls, op, GS.PLANS[0], storage)
        return
    census.run_items(d, storage)
    census.report()


# ---------------------------------------------------------------------------------------------
# the plain-CSR entry on the same CSR
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', WIDTHS)
def test_csr_entry_on_the_census(census, d):
    """renet_rgcn_gather with the hub list (hub rows by a workgroup each) and without it (every row in the row-group walk)."""
    for op in (GS.int_operands(d), GS.float_operands(d)):
        for hubs in (True, False):
            for k, plan in enumerate(GS.PLANS[:2]):            # (the CSR is the same; the plan sets the hub threshold)
                for cls in ITEM_CLASSES['w16']:                # the four classes without the table
                    for shift in ((3, GS.T - 1) if cls == 'bwd_full' else (None,)):
                        census.check('csr', cls, op, plan, drop_on=k != 1, shift=shift, hubs=hubs)
    census.report()


# ---------------------------------------------------------------------------------------------
# a group of exactly 64 items, through the raw C entry
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', WIDTHS)
def test_hand_built_group_of_64_items(dev, d):
    """The header allows groups of <= 64 items; the planner stops at 63.  Forward (scale, addend under dropout, ReLU), full
    backward and the compacted pruned backward (in place, NaN in the sources >= src_limit and in the addend row beyond
    addend_rows), fp32 and bf16 relation blocks."""
    import renet_hip as K
    h = GS.hand_stream()
    L = K.lib()
    si, n, T = d // 100, GS.HAND_ROWS, GS.T

    def to(a):
        return torch.from_numpy(np.array(a)).to(dev)
    idx = {f: to(getattr(h, f)) for f in ('it_src', 'it_type', 'grp_ptr', 'row_ptr', 'col', 'etype')}
    worst = 0.0
    for kind in ('int', 'float'):
        rng = np.random.RandomState(d + (kind == 'int'))
        if kind == 'int':
            x = rng.randint(-8, 9, (GS.HAND_X_ROWS, d)).astype(np.float32)
            w = rng.randint(-4, 5, (T, d * si)).astype(np.float32)
            ad = rng.randint(-64, 65, (n, d)).astype(np.float32)
            scale, p = np.asarray([0.5, 0.25, 1.0], np.float32), 0.5
        else:
            x = rng.randn(GS.HAND_X_ROWS, d).astype(np.float32)
            w = (rng.randn(T, d * si) * 0.3).astype(np.float32)
            ad = rng.randn(n, d).astype(np.float32)
            scale, p = (1.0 / np.diff(h.row_ptr)).astype(np.float32), 0.4
        tw, tscale = to(w), to(scale)
        for b16 in ((False, True) if d != 300 else (False,)):
            w16 = K.pack_bf16(tw) if b16 else None
            wref = GS.round_bf16(w) if b16 else w
            for cls in ('fwd', 'bwd', 'bwd_compact'):
                tr, fwd, compact = cls != 'fwd', cls == 'fwd', cls == 'bwd_compact'
                xs, out0 = x.copy(), np.full((n, d), np.nan, np.float32)
                if compact:
                    xs[GS.HAND_SRC_LIMIT:] = np.nan
                    out0[:2] = ad[:2]
                src_limit, addend_rows = (GS.HAND_SRC_LIMIT, 2) if compact else (0, 0)
                tx, out = to(xs), to(out0)
                addend = to(ad) if fwd else out if compact else None
                head = (tx.data_ptr(), d, idx['it_src'].data_ptr(), idx['it_type'].data_ptr(), idx['grp_ptr'].data_ptr(), 1,
                        idx['row_ptr'].data_ptr(), idx['col'].data_ptr(), idx['etype'].data_ptr(),
                        tscale.data_ptr() if fwd else None)
                tail = (T, 0 if fwd else T - 1, int(tr), None if addend is None else addend.data_ptr(), p if fwd else 0.0,
                        GS.SEED, int(fwd), out.data_ptr(), n, None, 0, src_limit, addend_rows, int(compact), K._stream())
                if b16:
                    rc = L.renet_rgcn_gather_items_bf16(*head, w16.p.data_ptr(), w16.p.shape[1], *tail)
                else:
                    rc = L.renet_rgcn_gather_items(*head, tw.data_ptr(), *tail)
                assert rc == 0, (cls, b16, rc)
                torch.cuda.synchronize()
                ref, mag, deg = GS.statement(xs, h.src, h.dst, h.et, wref, d, T, 0 if fwd else T - 1, tr,
                                             scale if fwd else None, ad if fwd else out0 if compact else None, fwd, n,
                                             src_limit, addend_rows, drop=(p, GS.SEED) if fwd else None)
                what = 'hand stream %s D=%d bf16=%s %s' % (cls, d, b16, kind)
                if kind == 'int':
                    GS.assert_exact(out.cpu().numpy(), ref, what=what)
                else:
                    worst = max(worst, GS.assert_within_bound(out.cpu().numpy(), ref, mag, deg, si, what=what))
    print('gather-bound entry=items_raw class=group64 D=%d storage=fp32+w16 ratio=%.3f' % (d, worst))


# ---------------------------------------------------------------------------------------------
# every RENET_GATHER_UNR instantiation (read once per process: one child each)
# ---------------------------------------------------------------------------------------------
_UNR_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import torch
import renet_hip
renet_hip.lib()
from test_gpu_gather_exact import Census
c = Census(torch.device('cuda:0'))
for d in sys.argv[3].split(','):
    c.run_items(int(d), 'fp32', kinds=('int',))
print('ok')
'''
_CHILD_FAULT = []


@pytest.mark.parametrize('unr', sorted(UNR_WIDTHS))
def test_every_unroll_instantiation_on_the_integer_census(dev, unr):
    """All five launch classes under the three plans, bit for bit, at every width that has an instantiation for this UNR."""
    assert not _CHILD_FAULT, 'not started: the child of RENET_GATHER_UNR=%s faulted or timed out' % _CHILD_FAULT[0]
    env = dict(os.environ, RENET_GATHER_UNR=str(unr))
    widths = ','.join(str(d) for d in UNR_WIDTHS[unr])
    try:
        r = subprocess.run([sys.executable, '-c', _UNR_CHILD, PKG, HERE, widths], env=env, capture_output=True, text=True,
                           timeout=300)
    except subprocess.TimeoutExpired:
        _CHILD_FAULT.append(unr)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _CHILD_FAULT.append(unr)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------
# the plain-CSR kernel's second row group of a wave
# ---------------------------------------------------------------------------------------------
def test_csr_second_row_group_of_a_wave(dev):
    """The launch has at most 2048 workgroups of 4 waves, a wave takes 8 rows at a time: beyond 8 192 row groups a wave walks
    a second one.  N = 65 600 (8 200 groups) at D = 100, about 2 000 edges, one into the last row and one into the first row
    of group 8 199, a hub row, integers: every row of the output (NaN before the launch) must be the statement exactly."""
    import graph as G
    import renet_hip as K
    n, d, T, heavy = 65600, 100, GS.T, 8
    rng = np.random.RandomState(8199)
    m = 2000
    src, dst, et = rng.randint(0, n, m), rng.randint(0, n, m), rng.choice(GS.TYPES_USED, m)
    dst[0], dst[1] = n - 1, 8199 * 8
    dst[2:32] = 40039                                          # a hub row inside a second row group (see below)
    hub = int(dst[2])
    hb = G.HostBatch().set_edges(n, src, dst, et, T, heavy=heavy).set_gather_plan(heavy=heavy)
    assert (n + 7) // 8 == 8200 > 2048 * 4 and hub in hb.heavy_rows.tolist()
    # row groups per workgroup = ceil(8200 / 2048) = 5: a workgroup walks groups 5 b .. 5 b + 4, its wave 0 takes the first
    # and then the fifth -- group 8 199 is such a second group, and so is the hub row's, which the walk has to step over
    assert 8199 % 5 == 4 and (hub // 8) % 5 == 4
    scale = (2.0 ** -(np.arange(n) % 4)).astype(np.float32)
    hb.norm = scale
    g = G.DeviceGraph(hb, dev)
    x = rng.randint(-8, 9, (n, d)).astype(np.float32)
    w = rng.randint(-4, 5, (T, d)).astype(np.float32)
    ad = rng.randint(-64, 65, (n, d)).astype(np.float32)
    tx, tw, tad = (torch.from_numpy(a).to(dev) for a in (x, w, ad))
    for tr in (False, True):
        shift, p = (T - 1, 0.0) if tr else (0, 0.5)
        ref = GS.statement(x, src, dst, et, w, d, T, shift, tr, None if tr else scale, None if tr else ad, not tr, n,
                           drop=None if tr else (p, GS.SEED))[0]
        for hubs in (True, False):
            out = torch.full((n, d), float('nan'), device=dev)
            K.rgcn_gather(tx, g.row_ptr, g.col, g.etype, None if tr else g.norm, tw, shift, tr, None if tr else tad, p,
                          GS.SEED, not tr, out, g.heavy_rows if hubs else None, heavy if hubs else 0)
            GS.assert_exact(out.cpu().numpy(), ref, what='csr N=65600 tr=%s hubs=%s' % (tr, hubs))


# ---------------------------------------------------------------------------------------------
# run-to-run bit identity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', WIDTHS)
def test_five_classes_are_bit_identical_run_to_run(census, d):
    op = GS.float_operands(d)
    for cls in GS.CLASSES:
        a = census.launch('items', cls, op, GS.PLANS[0])[0]
        b = census.launch('items', cls, op, GS.PLANS[0])[0]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), cls
