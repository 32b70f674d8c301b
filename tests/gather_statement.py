"""Host statement (numpy float64, no GPU) of the RGCN block-diagonal gather-SpMM, written from the operator's definition in
include/renet_hip.h (the comment above renet_rgcn_gather, and the table form above renet_rgcn_gather_items_table) and from
tests/dropout_masks.py -- not from a kernel:

    out[v, :] = act( scale[v] * sum_{e: dst(e) = v, kept} blockmul(x[src(e), :], W[(type(e) + type_shift) mod T])
                     + addend[v, :] * mask[v, :] )                                       v < n_out (the row prefix)
    kept     : src(e) < src_limit (src_limit > 0);   addend only for v < addend_rows (addend_rows > 0)
    blockmul : x viewed [100, si], W[tau] viewed [100, si, si];  y[b, j] = sum_i x[b, i] W[b, i, j]   (transpose_w == 0)
                                                                 y[b, i] = sum_j x[b, j] W[b, i, j]   (transpose_w == 1)
    mask     : dropout_masks.flat_mask(rows, D, seed, p)  (group = row * D/4 + col/4)
    table    : x = table[row_map[src(e)]], addend = addend_table[row_map[v]]

`statement` returns the float64 output, the magnitude mag[v, c] = |scale[v]| * sum |x| |W| + |addend * mask| and the number
of kept in-edges of every row.

Error bound of an fp32 evaluation, for ANY summation order, hub or light routing, with or without fma contraction.  Row v
has n = kept_deg[v] * si products per output element.  The sum is the root of some binary tree of fp32 additions in which a
product is rounded once on its own (an fma folds that rounding into an addition) and then passes through at most n - 1
further additions: at most n roundings.  The scale multiplies the sum (one rounding); the addend is multiplied by its mask
multiplier (one rounding) and added (one rounding, which the scaled sum shares).  Every term of the exact result therefore
carries a factor prod (1 + d_k), |d_k| <= u = 2^-24, of at most n + 2 roundings, and (1 + u)^(n+2) - 1 <= (n + 3) u for every
n this project can meet ((n + 2)^2 u^2 / 2 < u as long as n < 5 000).  ReLU is 1-Lipschitz and exact.  Hence

    |got - ref64| <= (kept_deg[v] * si + 3) * 2^-24 * mag[v, c]                           at every element,

and where mag is 0 (a row without kept in-edge and without addend) the result must be exactly the reference.  The bound is
derived, not fitted to a kernel: tests/test_gather_statement_cpu.py holds the float32 torch emulation of the C ABI to it.
For the bf16-STORAGE forms the reference is the statement on the bf16-rounded W (and table): widening bf16 to fp32 is exact,
so the same bound holds.

With the integer operands of `int_operands` every product, every partial sum of any subset in any order (|.| <= 150 * 4 * 32
< 2^15), the power-of-two scale, the mask multiplier 2 and the addend are exact in fp32 and every operand is a single bf16
term: the fp32 result is then the statement BIT FOR BIT (`exactness_margin` checks the premise).

The census graph (`census`) is ONE deterministic multigraph, N = 333, n_out = 120, T = 7, shared by all widths, that
contains by construction -- each at a named row -- the structural edges a random graph produces only by accident."""
import functools
import types

import numpy as np

import dropout_masks

U24 = 2.0 ** -24
OLD_RTOL = OLD_ATOL = 1e-4                       # the tolerance these statements replace

N, N_OUT, T, N_ENT = 333, 120, 7, 70
PLANS = ((8, 12), (31, 32), (62, 1))             # (heavy, budget): production, then two extremes of the planner
TYPES_USED = (0, 1, 2, 3, 4, 6)
TYPE_UNUSED = 5                                  # a type that never occurs
# designated rows: no in-edge / last row of the prefix / first row beyond it / last row
ROW_EMPTY, ROW_PREFIX_LAST, ROW_BEYOND, ROW_LAST = 0, 119, 120, 332
HUB150 = 17                                      # prefix hub, 150 in-edges in three index windows (64 + 64 + 22)
HUB150_LIVE_SRC = 33                             # source of the ONE live edge (src < n_out) of its third window
ROW_DUP, ROW_SELF = 50, 60                       # a duplicate multi-edge 7 -> 50 (type 2) twice; a self-edge 60 -> 60
# outside the prefix: the smallest hub of every plan next to its largest light row
ROW_DEG = {200: 9, 201: 8, 202: 32, 203: 31, 204: 63, 205: 62}
HUB64, HUB65 = 210, 211                          # one window of exactly 64 edges; 64 + a window of a single edge
DEAD_RUN = (230, 254)                            # rows [230, 254): 3 in-edges each, every source >= n_out
ROW_LIGHT_DEAD = 230
ROW_ENT0_LIGHT, ROW_ENT0_HUB = ROW_SELF, HUB150   # node_ent == 0 on a light row (flush it_type == -3) and on a hub row
SEED = 20240531                                  # dropout seed of the census launches


def round_bf16(a):
    """float32 -> the float32 value of its bf16 rounding (nearest even), as renet_pack_bf16 stores it."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


# ---------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------
def _blockmul(xs, ws, si, tr):
    xs = xs.reshape(-1, 100, si)
    ws = ws.reshape(-1, 100, si, si)
    y = np.einsum('ebj,ebij->ebi', xs, ws) if tr else np.einsum('ebi,ebij->ebj', xs, ws)
    return y.reshape(-1, 100 * si)


def statement(x, src, dst, et, w, d, T, shift, tr, norm, addend, relu, n_out, src_limit=0, addend_rows=0, drop=None,
              row_map=None, mask=None):
    """-> (out float64 [n_out, d], mag float64 [n_out, d], kept_deg int64 [n_out]).
    x [rows, d] (the table with row_map), w [T, d * d/100], norm [>= n_out] or None, addend [rows, d] (the addend table with
    row_map) or None; drop = (p, seed) or None; mask = explicit float64 multipliers [>= n_out, d] instead of drop.  Rows of
    x at or beyond src_limit and rows of addend at or beyond addend_rows are never touched (they may hold NaN)."""
    si = d // 100
    src, dst, et = (np.asarray(a, np.int64) for a in (src, dst, et))
    keep = dst < n_out
    if src_limit > 0:
        keep &= src < src_limit
    s, v, tau = src[keep], dst[keep], (et[keep] + shift) % T
    rows = s if row_map is None else np.asarray(row_map, np.int64)[s]
    xs = np.asarray(x)[rows].astype(np.float64)
    ws = np.asarray(w)[tau].astype(np.float64)
    acc, amag = np.zeros((n_out, d)), np.zeros((n_out, d))
    np.add.at(acc, v, _blockmul(xs, ws, si, tr))
    np.add.at(amag, v, _blockmul(np.abs(xs), np.abs(ws), si, tr))
    sc = np.ones(n_out) if norm is None else np.asarray(norm)[:n_out].astype(np.float64)
    out, mag = acc * sc[:, None], amag * np.abs(sc)[:, None]
    if addend is not None:
        m = min(addend_rows, n_out) if addend_rows > 0 else n_out
        arow = np.arange(m) if row_map is None else np.asarray(row_map, np.int64)[:m]
        a = np.asarray(addend)[arow].astype(np.float64)
        if mask is None and drop is not None:
            mask = dropout_masks.flat_mask(n_out, d, drop[1], drop[0])
        if mask is not None:
            a = a * np.asarray(mask, np.float64)[:m]
        out[:m] += a
        mag[:m] += np.abs(a)
    if relu:
        out = np.maximum(out, 0.0)
    return out, mag, np.bincount(v, minlength=n_out).astype(np.int64)


def bound(mag, kept_deg, si):
    return (np.asarray(kept_deg, np.float64)[:, None] * si + 3.0) * U24 * mag


def ratio(got, ref, mag, kept_deg, si):
    """error / bound per element; a non-finite `got` counts as infinitely wrong; 0 / 0 = 0 and x / 0 = inf."""
    got = np.asarray(got, np.float64)
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0, 0.0, err / bound(mag, kept_deg, si))


def old_ratio(got, ref):
    """error / (atol + rtol |ref|) of the tolerance this file replaces (what np.testing.assert_allclose evaluates)."""
    got = np.asarray(got, np.float64)
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    return float((err / (OLD_ATOL + OLD_RTOL * np.abs(ref))).max()) if err.size else 0.0


def assert_within_bound(got, ref, mag, kept_deg, si, what=''):
    """|got - ref| <= (kept_deg * si + 3) 2^-24 mag at EVERY element (exact where the bound is 0) -> the worst ratio."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = ratio(got, ref, mag, kept_deg, si)
    if r.size and not r.max() <= 1.0:
        v, c = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError('%s: %d of %d elements beyond the derived bound; worst error / bound %.4g at row %d col %d '
                             '(got %r, statement %r, kept in-degree %d)' % (what, int((r > 1.0).sum()), r.size, r[v, c], v,
                                                                            c, float(got[v, c]), float(ref[v, c]),
                                                                            int(kept_deg[v])))
    return float(r.max()) if r.size else 0.0


def assert_exact(got, ref, untouched=None, what=''):
    """got.astype(float64) == statement at every element.  The caller prefills the output with NaN and puts NaN into the
    rows that must not be read (sources >= src_limit, addend rows >= addend_rows): a row that was not overwritten, or a
    sentinel that was read, is a NaN here and fails.  `untouched`: memory behind the output that must still be all NaN."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    g64 = got.astype(np.float64)
    bad = ~(g64 == ref)                                          # NaN compares unequal
    if bad.any():
        v, c = np.argwhere(bad)[0]
        raise AssertionError('%s: %d of %d elements differ from the integer statement (%d of them NaN: a row not written or '
                             'a sentinel read); first at row %d col %d: got %r, statement %r; rows %s' %
                             (what, int(bad.sum()), bad.size, int(np.isnan(g64).sum()), v, c, float(g64[v, c]),
                              float(ref[v, c]), np.unique(np.argwhere(bad)[:, 0])[:12].tolist()))
    if untouched is not None and not np.isnan(np.asarray(untouched)).all():
        raise AssertionError('%s: rows beyond the output were written' % what)


def exactness_margin(mag):
    """2^24 / the largest magnitude an fp32 partial sum can reach (mag bounds every partial sum of any subset); > 1 (and
    operands that are multiples of 2^-3 of modest size) is the premise of assert_exact."""
    return 2.0 ** 24 / max(float(np.max(mag)), 1.0)


# ---------------------------------------------------------------------------------------------
# the census graph
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def census():
    """-> namespace(src, dst, et, node_ent): int64 edge lists (shuffled: the CSR builder sorts them by destination, then
    type, then input order) and the int32 entity of every row for the table form."""
    rng = np.random.RandomState(333)
    S, Dst, Ty = [], [], []

    def add(srcs, v, types):
        S.extend(int(a) for a in srcs)
        Dst.extend([int(v)] * len(srcs))
        Ty.extend(int(a) for a in types)

    def types_of(n):
        return rng.choice(TYPES_USED, n)

    # the prefix hub: window 1 (types 0, 1) mixed sources, window 2 (types 2, 3) every source >= n_out, window 3 (types 4,
    # 6; 22 edges) one live edge
    add(rng.randint(0, N, 64), HUB150, [0] * 32 + [1] * 32)
    add(rng.randint(N_OUT, N, 64), HUB150, [2] * 32 + [3] * 32)
    w3 = rng.randint(N_OUT, N, 22)
    w3[5] = HUB150_LIVE_SRC
    add(w3, HUB150, [4] * 11 + [6] * 11)
    for v, deg in sorted(ROW_DEG.items()):
        add(rng.randint(0, N, deg), v, types_of(deg))
    add(rng.randint(0, N, 64), HUB64, types_of(64))
    add(rng.randint(0, N, 65), HUB65, types_of(65))
    for v in range(*DEAD_RUN):
        add(rng.randint(N_OUT, N, 3), v, types_of(3))
    add([7, 7, 130], ROW_DUP, [2, 2, 0])
    add([ROW_SELF, 3], ROW_SELF, [1, 4])
    add(rng.randint(0, N, 3), ROW_PREFIX_LAST, types_of(3))
    add(rng.randint(0, N, 2), ROW_BEYOND, types_of(2))
    add(rng.randint(0, N, 4), ROW_LAST, types_of(4))
    special = {ROW_EMPTY, ROW_PREFIX_LAST, ROW_BEYOND, ROW_LAST, HUB150, ROW_DUP, ROW_SELF, HUB64, HUB65}
    special |= set(ROW_DEG) | set(range(*DEAD_RUN))
    for v in range(N):
        if v not in special:
            deg = int(rng.randint(0, 6))
            add(rng.randint(0, N, deg), v, types_of(deg))
    perm = rng.permutation(len(S))
    node_ent = rng.randint(0, N_ENT, N).astype(np.int32)
    node_ent[ROW_ENT0_LIGHT] = node_ent[ROW_ENT0_HUB] = 0
    c = types.SimpleNamespace(src=np.asarray(S, np.int64)[perm], dst=np.asarray(Dst, np.int64)[perm],
                              et=np.asarray(Ty, np.int64)[perm], node_ent=node_ent)
    for a in (c.src, c.dst, c.et, c.node_ent):
        a.setflags(write=False)
    return c


def host_batch(heavy, budget, scale=None):
    """graph.HostBatch of the census graph under plan (heavy, budget), with the row prefix n_out and the entity map; `scale`
    replaces the 1/deg norm (before a DeviceGraph is made of it)."""
    import graph as G
    c = census()
    hb = G.HostBatch().set_edges(N, c.src, c.dst, c.et, T, heavy=heavy)
    hb.set_out_rows(N_OUT, c.src, c.dst, c.et)
    hb.set_gather_plan(N_OUT, heavy=heavy, budget=budget)
    hb.node_ent = c.node_ent.copy()
    hb.plan_node_ent = G.SegPlan.host(hb.node_ent)
    if scale is not None:
        hb.norm = np.array(scale, np.float32)
    return hb


HAND_ROWS, HAND_X_ROWS, HAND_SRC_LIMIT = 3, 40, 30


@functools.lru_cache(maxsize=None)
def hand_stream():
    """A hand-built item stream whose ONE group holds exactly 64 items (the header allows it, the planner stops at 63): three
    light rows of 20, 20 and 21 in-edges, each followed by its flush item.  Sources are rows of a 40-row x; some lie at or
    beyond HAND_SRC_LIMIT.  -> namespace(src, dst, et; it_src, it_type, grp_ptr; row_ptr, col, etype)"""
    rng = np.random.RandomState(64)
    degs = (20, 20, 21)
    src = rng.randint(0, HAND_X_ROWS, sum(degs)).astype(np.int64)
    dst = np.repeat(np.arange(HAND_ROWS), degs).astype(np.int64)
    et = np.concatenate([np.sort(rng.choice(TYPES_USED, n)) for n in degs]).astype(np.int64)
    it_src, it_type = [], []
    for v in range(HAND_ROWS):
        it_src += src[dst == v].tolist() + [v]
        it_type += et[dst == v].tolist() + [-1]
    assert len(it_src) == 64
    return types.SimpleNamespace(src=src, dst=dst, et=et, it_src=np.asarray(it_src, np.int32),
                                 it_type=np.asarray(it_type, np.int32), grp_ptr=np.asarray([0, 64], np.int32),
                                 row_ptr=np.concatenate(([0], np.cumsum(degs))).astype(np.int32),
                                 col=src.astype(np.int32), etype=et.astype(np.int32))


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_operands(d):
    """Small integers: x, gn, table in [-8, 8], W in [-4, 4], the addends in [-64, 64]; scale[v] = 2^-(v mod 4) (goes into
    hb.norm in place of 1/deg before the DeviceGraph is made); dropout p = 0.5 (multiplier exactly 2)."""
    rng = np.random.RandomState(1000 + d)
    si = d // 100

    def ints(hi, *shape):
        return rng.randint(-hi, hi + 1, shape).astype(np.float32)
    o = types.SimpleNamespace(kind='int', d=d, p=0.5, x=ints(8, N, d), w=ints(4, T, d * si), ad=ints(64, N, d),
                              gn=ints(8, N, d), dh=ints(64, N, d), table=ints(8, N_ENT, d), ad_table=ints(64, N_ENT, d),
                              scale=(2.0 ** -(np.arange(N) % 4)).astype(np.float32))
    return _freeze(o)


@functools.lru_cache(maxsize=None)
def float_operands(d):
    """randn x / gn / table and addends, 0.3 randn W; scale = None: the graph's own 1/deg norm; dropout p = 0.4."""
    rng = np.random.RandomState(2000 + d)
    si = d // 100

    def rn(*shape):
        return rng.randn(*shape).astype(np.float32)
    o = types.SimpleNamespace(kind='float', d=d, p=0.4, x=rn(N, d), w=(rng.randn(T, d * si) * 0.3).astype(np.float32),
                              ad=rn(N, d), gn=rn(N, d), dh=rn(N, d), table=rn(N_ENT, d), ad_table=rn(N_ENT, d), scale=None)
    return _freeze(o)


def _freeze(o):
    for a in vars(o).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


# ---------------------------------------------------------------------------------------------
# the five launch classes of a training step, as arguments of the statement and of an entry
# ---------------------------------------------------------------------------------------------
CLASSES = ('fwd_full', 'fwd_table', 'fwd_pruned', 'bwd_full', 'bwd_pruned')


def launch_case(cls, op, norm, drop_on=True, shift=None, sentinels=True):
    """The host arrays and arguments of launch class `cls` on operands `op` (norm: the scale the graph carries).
      x            source rows (fwd_table: the table); bwd_pruned: rows >= n_out are NaN (must not be read)
      addend       separate addend tensor, or None
      out0         initial contents of the output buffer when the addend is taken IN PLACE from it (else the caller fills
                   the output with NaN); bwd_pruned: rows >= addend_rows are NaN (must be overwritten, never read)
      n_rows, tr, shift, use_norm, relu, p, src_limit, addend_rows, pruned, row_map
    sentinels=False keeps finite values where the NaNs would be (for host evaluations that model a kernel reading them)."""
    p = op.p if drop_on else 0.0
    c = types.SimpleNamespace(cls=cls, d=op.d, n_rows=N, tr=False, shift=0, use_norm=True, relu=False, p=0.0, seed=SEED,
                              src_limit=0, addend_rows=0, pruned=False, row_map=None, addend=None, out0=None, x=op.x)
    if cls == 'fwd_full':                 # layer 1: norm, addend, dropout, ReLU
        c.addend, c.p, c.relu = op.ad, p, True
    elif cls == 'fwd_table':              # layer 1 addressed through the entity table
        c.x, c.addend, c.p, c.relu, c.row_map = op.table, op.ad_table, p, True, census().node_ent
    elif cls == 'fwd_pruned':             # last layer on the row prefix, self-loop product already in the output
        c.n_rows, c.pruned, c.p, c.out0 = N_OUT, True, p, op.ad[:N_OUT].copy()
    elif cls == 'bwd_full':               # transposed blocks, no norm, no addend
        c.x, c.tr, c.use_norm, c.shift = op.gn, True, False, 3 if shift is None else shift
    elif cls == 'bwd_pruned':             # all rows written, sources and addend rows of the prefix only, in place
        c.x, c.out0 = op.gn.copy(), op.dh.copy()
        if sentinels:
            c.x[N_OUT:] = np.nan
            c.out0[N_OUT:] = np.nan
        c.tr, c.use_norm, c.shift, c.pruned = True, False, T - 1 if shift is None else shift, True
        c.src_limit = c.addend_rows = N_OUT
    else:
        raise ValueError(cls)
    c.norm = norm if c.use_norm else None
    return c


def case_statement(c, w=None, x=None, edges=None, **over):
    """statement(...) of launch case c on the relation blocks w; x / edges / any keyword of `statement` replace the case's
    own (the bf16-rounded table, a graph with an edge taken out, ...)."""
    g = census() if edges is None else edges
    a = dict(x=c.x if x is None else x, src=g.src, dst=g.dst, et=g.et, w=w, d=c.d, T=T, shift=c.shift, tr=c.tr, norm=c.norm,
             addend=c.out0 if c.out0 is not None else c.addend, relu=c.relu, n_out=c.n_rows, src_limit=c.src_limit,
             addend_rows=c.addend_rows, drop=(c.p, c.seed) if c.p > 0 else None, row_map=c.row_map)
    a.update(over)
    return statement(**a)


# ---------------------------------------------------------------------------------------------
# defective host evaluations: what a subtly wrong kernel would return (tests/test_gather_statement_cpu.py: teeth)
# ---------------------------------------------------------------------------------------------
INT_DEFECTS = {                     # kind -> the launch class on which the defect is active
    'hub_edge_dropped': 'fwd_full', 'edge_twice': 'fwd_full', 'shift_no_wrap': 'bwd_full', 'other_orientation': 'fwd_full',
    'neighbour_scale': 'fwd_full', 'addend_row_off': 'fwd_full', 'mask_group_off': 'fwd_full',
    'src_limit_ignored': 'bwd_pruned', 'addend_rows_ignored': 'bwd_pruned', 'addend_before_scale': 'fwd_full',
    'table_flush_row_v': 'fwd_table'}
FLOAT_DEFECTS = ('w_bf16', 'x_fp16', 'edge_dropped_150', 'w_bf16x2')


def _without_edge(g, which):
    keep = np.ones(len(g.src), bool)
    keep[which] = False
    return types.SimpleNamespace(src=g.src[keep], dst=g.dst[keep], et=g.et[keep])


def _hub_live_edge(g):
    """index of the live edge of HUB150's last window"""
    (i,) = np.nonzero((g.dst == HUB150) & (g.src == HUB150_LIVE_SRC) & (g.et >= 4))
    return int(i[0])


def defective(kind, c, w):
    """float32 result of launch case c (built with sentinels=False) evaluated with defect `kind`."""
    g = census()
    if kind in ('hub_edge_dropped', 'edge_dropped_150'):
        out = case_statement(c, w, edges=_without_edge(g, _hub_live_edge(g)))[0]
    elif kind == 'edge_twice':
        i = _hub_live_edge(g)
        e2 = types.SimpleNamespace(src=np.append(g.src, g.src[i]), dst=np.append(g.dst, g.dst[i]), et=np.append(g.et, g.et[i]))
        out = case_statement(c, w, edges=e2)[0]
    elif kind == 'shift_no_wrap':             # W[type + shift] without the wrap: rows T .. 2T-1 lie beyond the table (zeros)
        w2 = np.concatenate((w, np.zeros_like(w)))
        out = case_statement(c, w2, T=2 * T)[0]
    elif kind == 'other_orientation':
        out = case_statement(c, w, tr=not c.tr)[0]
    elif kind == 'neighbour_scale':
        out = case_statement(c, w, norm=np.roll(c.norm, -1))[0]
    elif kind == 'addend_row_off':
        out = case_statement(c, w, addend=np.roll(c.addend, -1, axis=0))[0]
    elif kind == 'mask_group_off':            # the multipliers of group g + 1 on group g
        m = dropout_masks.flat_mask(c.n_rows, c.d, c.seed, c.p)
        out = case_statement(c, w, mask=np.roll(m.reshape(-1), -4).reshape(m.shape))[0]
    elif kind == 'src_limit_ignored':
        out = case_statement(c, w, src_limit=0)[0]
    elif kind == 'addend_rows_ignored':
        out = case_statement(c, w, addend_rows=0)[0]
    elif kind == 'addend_before_scale':       # act(scale * (sum + addend * mask))
        s = case_statement(c, w, addend=None, relu=False)[0]
        a = case_statement(c, w, norm=None, relu=False)[0] - case_statement(c, w, norm=None, addend=None, relu=False)[0]
        out = s + a * np.asarray(c.norm, np.float64)[:c.n_rows, None]
        out = np.maximum(out, 0.0) if c.relu else out
    elif kind == 'table_flush_row_v':         # addend_table[v] instead of addend_table[row_map[v]] (beyond the table: zeros)
        pad = np.zeros((N, c.d), np.float32)
        pad[:N_ENT] = c.addend
        out = case_statement(c, w, x=c.x[c.row_map], row_map=None, addend=pad)[0]
    elif kind == 'w_bf16':
        out = case_statement(c, round_bf16(w))[0]
    elif kind == 'x_fp16':
        out = case_statement(c, w, x=c.x.astype(np.float16).astype(np.float32))[0]
    elif kind == 'w_bf16x2':                  # two bf16 terms of W (16 significant bits) where three make an fp32
        hi = round_bf16(w)
        out = case_statement(c, hi + round_bf16(w - hi))[0]
    else:
        raise ValueError(kind)
    return out.astype(np.float32)
