"""Host statements (numpy float64, no GPU) of the deterministic reductions of the backward pass, written from the header
text of include/renet_hip.h and not from the kernels: the relation-weight gradient (renet_rgcn_bwd_w), the column sums
(renet_colsum), the segmented add (renet_segment_add), the operand-bound maxima (renet_maxabs_partials) and the index
composition of the table-addressed layer (renet_compose_table_items).  Each reduction statement returns the float64 result
and the per-element sum of |terms|.

Error bound of an fp32 sum, for ANY summation order.  An output that is the fp32 sum of n terms (an fma product counts as
one rounding) plus an optional beta * old is the root of some binary tree of additions; a term reaches the root through at
most n additions (n - 1 among the terms, one with beta * old) after at most one rounding of its own (the product, or
beta * old), so it carries a factor prod (1 + d_k) of at most n + 1 <= n + 2 roundings |d_k| <= u = 2^-24:

    |got - exact| <= gamma(n + 2) * (sum |terms| + |beta * old|),   gamma(k) = k u / (1 - k u)

The only absolute floor is the underflow of the terms themselves: 2^-149 per term.  No bound here is fitted to a kernel:
tests/test_reduction_statements_cpu.py pushes each through float32 numpy evaluations of the same operands in three orders.

With small integer operands every partial sum (of any subset, in any order) is an integer below 2^24 in magnitude and so
exactly representable: the result must then equal the integer statement BIT FOR BIT (`exactness_margin` checks the
premise).  The operands of the GPU tests (tests/test_gpu_reductions.py) are generated here, so that the host tests judge
the same numbers."""
import functools

import numpy as np

U24 = 2.0 ** -24
TINY = 2.0 ** -149


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U24 / (1.0 - k * U24)


def sum_bound(n, mag):
    """bound of an fp32 sum of n terms (+ beta * old, already inside mag): gamma(n + 2) * mag + 2^-149 * n"""
    n = np.asarray(n, np.float64)
    return gamma(n + 2) * mag + TINY * n


def ratio(got, ref, n, mag):
    """error / bound per element; a non-finite `got` counts as infinitely wrong; 0 / 0 = 0"""
    got = np.asarray(got, np.float64)
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    b = np.broadcast_to(sum_bound(n, mag), err.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0, 0.0, err / b)


# ---------------------------------------------------------------------------------------------
# float32 host evaluations of a sum in three orders (what the bounds are held to)
# ---------------------------------------------------------------------------------------------
def _pairwise32(t):
    t = np.asarray(t, np.float32)
    while t.shape[0] > 1:
        if t.shape[0] & 1:
            t = np.concatenate((t, np.zeros((1,) + t.shape[1:], np.float32)))
        t = (t[0::2] + t[1::2]).astype(np.float32)
    return t[0]


def f32_sums(terms):
    """terms [n, ...] float32 -> the three float32 sums over axis 0: forward, reversed, pairwise tree"""
    terms = np.asarray(terms, np.float32)
    if terms.shape[0] == 0:
        z = np.zeros(terms.shape[1:], np.float32)
        return [z, z, z]
    fwd = np.cumsum(terms, axis=0, dtype=np.float32)[-1]
    rev = np.cumsum(terms[::-1], axis=0, dtype=np.float32)[-1]
    return [fwd, rev, _pairwise32(terms)]


def exactness_margin(terms64):
    """largest possible |partial sum| of any subset of the terms [n, ...]: sum |terms|.  < 2^24 with integer terms makes
    every order of summation exact in fp32."""
    t = np.asarray(terms64, np.float64)
    assert np.array_equal(t, np.rint(t * 2) / 2), 'terms are not (half-)integers'
    return float(np.abs(t).sum(axis=0).max()) if t.size else 0.0


# ---------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------
def rne_bf16(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even; finite inputs"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def scale_bf16_statement(bits, f):
    """renet_scale_bf16_by_device_scalar: rne_bf16(float32(x) * f) bit for bit; f == 1 leaves x alone"""
    if np.float32(f) == np.float32(1):
        return np.array(bits, np.uint16)
    return rne_bf16(bf16_to_f32(bits) * np.float32(f))


# ---------------------------------------------------------------------------------------------
# dW: the relation-weight gradient
# ---------------------------------------------------------------------------------------------
def chunk_layout(spec, num_types, n_rows, seed=0):
    """spec: [(type, [chunk lengths])] with increasing types -> the relation-bucketed chunk list of renet_rgcn_bwd_w:
    chunk c covers the sorted edges [chunk_ptr[c], chunk_ptr[c + 1]), all of type chunk_type[c]; type_chunk_ptr[T + 1]
    lists, per type, its range of chunks.  Sources and destinations are random rows of [0, n_rows) and contain row 0 and
    row n_rows - 1."""
    types = [t for t, _ in spec]
    assert types == sorted(set(types)) and (not types or (types[0] >= 0 and types[-1] < num_types))
    chunk_type = np.array([t for t, ls in spec for _ in ls], np.int32)
    lens = np.array([l for _, ls in spec for l in ls], np.int64)
    chunk_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    per_type = np.zeros(num_types, np.int64)
    for t, ls in spec:
        per_type[t] = len(ls)
    type_chunk_ptr = np.concatenate(([0], np.cumsum(per_type))).astype(np.int32)
    e = int(chunk_ptr[-1])
    rng = np.random.RandomState(seed)
    e_src, e_dst = rng.randint(0, n_rows, e).astype(np.int32), rng.randint(0, n_rows, e).astype(np.int32)
    if e >= 4:
        e_src[0], e_src[e - 1], e_dst[1], e_dst[e - 2] = 0, n_rows - 1, n_rows - 1, 0
    return dict(e_src=e_src, e_dst=e_dst, chunk_ptr=chunk_ptr, chunk_type=chunk_type, type_chunk_ptr=type_chunk_ptr,
                n_chunks=len(chunk_type), T=num_types, E=e, n_rows=n_rows)


def planner_spec(type_counts, chunk=64):
    """the spec a planner produces that cuts every type into `chunk`-edge chunks and a remainder"""
    return [(t, [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])) for t, n in enumerate(type_counts) if n > 0]


GROUP = 8                                       # consecutive chunks one workgroup of the partial pass sums through LDS
CENSUS_T = 19
CENSUS_ROWS = 600
_BIG = 1197                                     # chunks of the hot type: 149 group starts inside it
CENSUS_SPEC = [
    # type 0: no chunk
    (1, [64]),
    (2, [65, 0]),                                                   # an empty chunk ends a type
    (3, [1, 2, 3, 5, 7, 8, 9, 63]),                                 # 8 chunks across one group boundary
    # type 4: no chunk
    (5, [64] * 8 + [17]),                                           # 9 chunks, what a CHUNK = 64 planner makes of 529 edges
    (6, [9, 0, 7, 65, 3, 2, 1, 8, 5, 64, 63, 150, 0, 1, 2, 3, 5]),  # 17 chunks
    (7, [63]),
    (8, [150]),                                                     # one chunk of three 64-edge rounds
    (9, [2]),                                                       # ends on a group boundary
    (10, [1, 64, 2, 65, 3, 63, 0, 8]),                              # exactly one whole group
    (11, [0, 150, 5]),                                              # an empty chunk starts a type (and a group)
    (12, [k % 3 + 1 for k in range(_BIG)]),                         # the hot type: starts at c0 mod 8 = 3
    # type 13: no chunk
    (14, [7, 9]),
    (15, [(7 * k) % 10 for k in range(16)]),                        # 16 chunks off the boundary: two group starts inside
    (16, [8] * 7),                                                  # its last chunk is alone at a group start
    (17, [1]),                                                      # the last chunk: one edge
    # type 18: no chunk
]
# per type (c0 mod 8, c1 mod 8, group starts inside (c0, c1)) -- asserted literally by the host test
CENSUS_TABLE = {
    0: (0, 0, 0), 1: (0, 1, 0), 2: (1, 3, 0), 3: (3, 3, 1), 4: (3, 3, 0), 5: (3, 4, 1), 6: (4, 5, 2), 7: (5, 6, 0),
    8: (6, 7, 0), 9: (7, 0, 0), 10: (0, 0, 0), 11: (0, 3, 0), 12: (3, 0, 149), 13: (0, 0, 0), 14: (0, 2, 0),
    15: (2, 2, 2), 16: (2, 1, 1), 17: (1, 2, 0), 18: (2, 2, 0),
}


def census(lay):
    """per type (c0 mod 8, c1 mod 8, number of group starts inside (c0, c1)): which slots of the workspace the partial pass
    writes for the type (c0 and those group starts) and the reduce pass reads"""
    out = {}
    for t in range(lay['T']):
        c0, c1 = int(lay['type_chunk_ptr'][t]), int(lay['type_chunk_ptr'][t + 1])
        out[t] = (c0 % GROUP, c1 % GROUP, len([g for g in range(c0 + 1, c1) if g % GROUP == 0]))
    return out


@functools.lru_cache(maxsize=None)
def census_layout():
    return chunk_layout(CENSUS_SPEC, CENSUS_T, CENSUS_ROWS, seed=11)


def edge_types(lay):
    return np.repeat(lay['chunk_type'].astype(np.int64), np.diff(lay['chunk_ptr'].astype(np.int64)))


def dw_statement(x, gn, lay, type_shift=0, beta=0.0, old=None):
    """dW[tau, b, i, j] = beta * old + sum_{e: tau(e) == tau} x[src[e], b si + i] gn[dst[e], b si + j], tau(e) =
    (type(e) + type_shift) mod T, si = D / 100.  -> (dW [T, D si], sum |terms| + |beta old|, edges per OUTPUT type [T])"""
    return dw_place(dw_type_sums(x, gn, lay), lay['T'], type_shift, beta, old)


def dw_type_sums(x, gn, lay):
    """per STORED type t: sum over its edges of the blockwise outer products, the same of the magnitudes, its edge count"""
    d = x.shape[1]
    si, t_n = d // 100, lay['T']
    et = edge_types(lay)
    x64, g64 = np.asarray(x, np.float64), np.asarray(gn, np.float64)
    ref, mag, n = np.zeros((t_n, 100, si, si)), np.zeros((t_n, 100, si, si)), np.zeros(t_n, np.int64)
    for t in range(t_n):
        e = np.nonzero(et == t)[0]
        if e.size == 0:
            continue
        xs, gs = x64[lay['e_src'][e]].reshape(-1, 100, si), g64[lay['e_dst'][e]].reshape(-1, 100, si)
        ref[t] = np.einsum('ebi,ebj->bij', xs, gs)
        mag[t] = np.einsum('ebi,ebj->bij', np.abs(xs), np.abs(gs))
        n[t] = e.size
    return ref.reshape(t_n, -1), mag.reshape(t_n, -1), n


def dw_place(sums, t_n, type_shift=0, beta=0.0, old=None):
    """the stored type t accumulates into dW[(t + type_shift) mod T]; dW = beta * old + ..."""
    tau = (np.arange(t_n) + type_shift) % t_n
    ref, mag, n = (np.zeros_like(a) for a in sums)
    ref[tau], mag[tau], n[tau] = sums
    if beta != 0.0:
        b = np.float64(np.float32(beta)) * np.asarray(old, np.float64)
        ref, mag = ref + b, mag + np.abs(b)
    return ref, mag, n


def dw_terms32(x, gn, lay, t):
    """the float32 products of stored type t, [edges, D si]: what a host evaluation of the sum adds up"""
    si = x.shape[1] // 100
    e = np.nonzero(edge_types(lay) == t)[0]
    xs, gs = x[lay['e_src'][e]].reshape(-1, 100, si, 1), gn[lay['e_dst'][e]].reshape(-1, 100, 1, si)
    return (xs * gs).astype(np.float32).reshape(len(e), x.shape[1] * si)


@functools.lru_cache(maxsize=None)
def dw_operands(d, kind):
    """x, gn [CENSUS_ROWS, D] and an old dW [T, D si]: 'int' in {-2..2} / {-3..3}, 'randn' standard normal"""
    rng = np.random.RandomState(d + (0 if kind == 'int' else 1))
    shape, wshape = (CENSUS_ROWS, d), (CENSUS_T, d * (d // 100))
    if kind == 'int':
        ops = (rng.randint(-2, 3, shape), rng.randint(-2, 3, shape), rng.randint(-3, 4, wshape))
    else:
        ops = (rng.randn(*shape), rng.randn(*shape), rng.randn(*wshape))
    ops = tuple(a.astype(np.float32) for a in ops)
    for a in ops:
        a.setflags(write=False)
    return ops


# ---------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------
COLSUM_MS = [0, 1, 3, 4, 5, 15, 16, 17, 127, 128, 129, 257, 8191, 8192, 8193]
COLSUM_NS = [1, 63, 64, 65, 200]
COLSUM_SHAPES = sorted({(m, 65) for m in COLSUM_MS} | {(m, n) for m in (129, 8193) for n in COLSUM_NS}
                       | {(m, n) for m in (0, 1, 5, 17) for n in COLSUM_NS}       # the full cross where it is cheap
                       | {(250, 65)})       # two groups of 125 rows, 125 mod 16 = 13: one 16-row step too many of a
#                                             wave lands on the FIRST ROW OF THE NEXT GROUP (inside the matrix, no NaN there)
BETAS = [0.0, 1.0, -0.5]


def colsum_groups(m):
    """row groups of the two-pass split: G = min(64, ceil(M / 128)) groups of ceil(M / G) rows; one pass for M <= 128"""
    return max(1, min(64, -(-m // 128)))


def colsum_statement(x, beta=0.0, old=None):
    """out[n] = beta * old[n] + sum_m X[m, n] -> (out, sum |terms| + |beta old|)"""
    x64 = np.asarray(x, np.float64)
    ref, mag = x64.sum(axis=0), np.abs(x64).sum(axis=0)
    if beta != 0.0:
        b = np.float64(np.float32(beta)) * np.asarray(old, np.float64)
        ref, mag = ref + b, mag + np.abs(b)
    return ref, mag


@functools.lru_cache(maxsize=None)
def colsum_operands(m, n, kind, bf16=False):
    """X [M, N] and an old out [N]: 'int' with |v| <= 8 (exact in bf16 too), 'randn' (rounded to bf16 for the bf16 entry:
    the statement sums the values the kernel reads)"""
    rng = np.random.RandomState(1000 * n + m + (0 if kind == 'int' else 7))
    if kind == 'int':
        x, old = rng.randint(-8, 9, (m, n)).astype(np.float32), rng.randint(-8, 9, n).astype(np.float32)
    else:
        x, old = rng.randn(m, n).astype(np.float32), rng.randn(n).astype(np.float32)
        if bf16:
            x = bf16_to_f32(rne_bf16(x)).reshape(m, n)
    x.setflags(write=False)
    old.setflags(write=False)
    return x, old


# ---------------------------------------------------------------------------------------------
# segmented add
# ---------------------------------------------------------------------------------------------
SEG_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 24, 127, 128, 129, 257, 1000]
SEG_US = [1, 16, 17, 512, 513, 8193 + 5]
_SEG_HEAD = [1000, 0, 17, 1, 257, 7, 129, 8, 128, 9, 127, 15, 24, 16]          # SEG_LENGTHS, short and long interleaved
_SEG_MID = [l for l in _SEG_HEAD if l not in (1000, 257)]
_SEG_TAIL = [1, 0, 1, 2, 1, 7, 1, 8, 1, 16, 1, 17, 1, 3, 1, 9]


def segment_lengths(u_n):
    """every length of SEG_LENGTHS first; then the list without its two longest, eight times; then short segments only
    (most segments of a batch own 1-8 rows): U = 8198 stays near 40 000 rows"""
    out = []
    for u in range(u_n):
        if u < len(_SEG_HEAD):
            out.append(_SEG_HEAD[u])
        elif u < len(_SEG_HEAD) + 8 * len(_SEG_MID):
            out.append(_SEG_MID[(u - len(_SEG_HEAD)) % len(_SEG_MID)])
        else:
            out.append(_SEG_TAIL[u % len(_SEG_TAIL)])
    return out


def segment_layout(lengths, n_src, seed=0, spare=3):
    """order (rows of src, repeats allowed), seg_ptr, seg_target for segments of the given lengths; the targets are
    distinct rows of a dst with `spare` rows more than segments, and deliberately not sorted by row"""
    rng = np.random.RandomState(seed)
    u_n = len(lengths)
    seg_ptr = np.concatenate(([0], np.cumsum(np.asarray(lengths, np.int64)))).astype(np.int32)
    order = rng.randint(0, n_src, int(seg_ptr[-1])).astype(np.int32)
    if order.size >= 2:
        order[0], order[-1] = n_src - 1, 0
    seg_target = rng.permutation(u_n + spare)[:u_n].astype(np.int32)
    return dict(order=order, seg_ptr=seg_ptr, seg_target=seg_target, U=u_n, n_dst=u_n + spare, n_src=n_src)


def segment_add_statement(src, lay, old):
    """dst[seg_target[u]] = old[seg_target[u]] + sum_{k in [seg_ptr[u], seg_ptr[u + 1])} src[order[k]]; the other rows
    keep their values.  -> (dst, sum |terms| incl. |old|, terms per row: segment length + 1, 0 for an untouched row)"""
    ptr, u_n = lay['seg_ptr'].astype(np.int64), lay['U']
    ref, mag = np.array(old, np.float64), np.abs(np.asarray(old, np.float64))
    n = np.zeros(lay['n_dst'], np.int64)
    lens = np.diff(ptr)
    n[lay['seg_target']] = lens + 1
    full = np.nonzero(lens > 0)[0]
    if full.size:
        rows = np.asarray(src, np.float64)[lay['order']]
        # empty segments own no rows, so the starts of the others partition `rows`
        ref[lay['seg_target'][full]] += np.add.reduceat(rows, ptr[full], axis=0)
        mag[lay['seg_target'][full]] += np.add.reduceat(np.abs(rows), ptr[full], axis=0)
    assert u_n == len(lens)
    return ref, mag, n


@functools.lru_cache(maxsize=None)
def segment_case(u_n, d, kind):
    """-> (layout, src0, src1, old0, old1): two sources (a swap of the pairs of renet_segment_add2 shows) of 1 500 rows"""
    n_src = 1500
    lay = segment_layout(segment_lengths(u_n), n_src, seed=u_n)
    rng = np.random.RandomState(7 * u_n + d + (0 if kind == 'int' else 3))
    shapes = [(n_src, d), (n_src, d), (lay['n_dst'], d), (lay['n_dst'], d)]
    if kind == 'int':
        arrs = [rng.randint(-2, 3, s).astype(np.float32) for s in shapes]
    else:
        arrs = [rng.randn(*s).astype(np.float32) for s in shapes]
    for a in arrs:
        a.setflags(write=False)
    return (lay,) + tuple(arrs)


# ---------------------------------------------------------------------------------------------
# maxima, index composition
# ---------------------------------------------------------------------------------------------
def maxabs_statement(x):
    """max |x| over the matrix as a float32; NaNs are ignored; 0 for an empty matrix (or one of NaNs only)"""
    a = np.abs(np.asarray(x, np.float32)).reshape(-1)
    a = a[~np.isnan(a)]
    return np.float32(a.max()) if a.size else np.float32(0)


def compose_statement(row_map, it_src, it_type, col, e_src):
    """the plain arrays with every SOURCE row u replaced by row_map[u]: edge items (type >= 0), the CSR columns and the
    relation-bucketed sources; a flush item (type -1) keeps its OUTPUT row v and carries -3 - row_map[v] as its type;
    any other negative type is no row reference and passes through.  -> (it_src_t, it_type_t, col_t, e_src_t)"""
    row_map, it_src, it_type = (np.asarray(a, np.int64) for a in (row_map, it_src, it_type))
    edge, flush = it_type >= 0, it_type == -1
    it_src_t = np.where(edge, row_map[np.where(edge, it_src, 0)], it_src)
    it_type_t = np.where(flush, -3 - row_map[np.where(flush, it_src, 0)], it_type)
    i32 = lambda a: np.asarray(a).astype(np.int32)
    return i32(it_src_t), i32(it_type_t), i32(row_map[np.asarray(col, np.int64)]), i32(row_map[np.asarray(e_src, np.int64)])
