"""Host statement (numpy float64, no GPU) of the neighbour pooling of the mean / attentive history encoders, written from the
comment above renet_nbr_pool_fwd in include/renet_hip.h -- not from a kernel.  Per segment u (n neighbours, entity ids
nbr[seg_ptr[u] .. seg_ptr[u + 1]), g = dOut[out_row[u], 0:D]):

    attn == 0:  out[out_row[u]] = [ mean_j E[nbr_j] | E[s] ]
                cE[k] = g / n,  ds_rows[u] = dOut[out_row[u], D:2D]
    attn != 0:  a_j = v . tanh(P[nbr_j] + q[seg_q[u]]),  M = max_j a_j,  L = sum_j exp(a_j - M),  w_j = exp(a_j - M) / L
                out[out_row[u]] = [ sum_j w_j E[nbr_j] | E[s] | R[r] ],  stats[u] = (M, log L)
                da = w_k (g . E[nbr_k] - g . out[out_row[u], 0:D]),  t = tanh(P[nbr_k] + q)
                cE[k] = w_k g,  cP[k] = da v (1 - t^2),  dq_rows[u] = sum_k cP[k],  dv_rows[u] = sum_k da t
                ds_rows[u] / dr_rows[u] = dOut[out_row[u], D:2D] / [2D:3D]

The backward is a pure function of its arguments, w and out included: `backward` takes them as inputs, so every backward
bound is local and no forward error enters (the principle of tests/gru_statement.py).

Error bounds of an fp32 evaluation (u = 2^-24; every quantity on a right-hand side is float64 and of the statement).  Taken,
not derived: tanhf within 4u|t| (as gru_statement.py takes it), expf within XE = 4 ulp, logf within 4 ulp.  R = 12 is the
number of roundings a product can meet in a D-term dot product that is summed four at a time (the product and three
additions), then across the chunks one lane owns (one addition), then by a six-step butterfly over 64 lanes (six) -- 11, and
one to spare.  A kernel that summed serially over D would need R = D + 1; this statement does not admit one.

  scores      dt_jc = u (|P_jc| + |q_c|) + 4u |t_jc|      (the rounded sum moves tanh by at most its own error; tanh' <= 1)
              A_j   = sum_c |v_c| dt_jc + R u sum_c |v_c t_jc|,   delta = max_j A_j over the segment
              bounds the error of every score and of the maximum:           |stats0 - M| <= delta
  sums        the header: one wave per segment, segments longer than 256 split over the (four) waves of a workgroup and merged
              in wave order; four neighbours in flight.  n_r = n (n <= 256) or ceil(n / 4): the terms one wave adds;
              K = ceil(n_r / 4) + 1 counts the rescales of the running sums (one per batch at most) and the merge factor;
              spread = max a - min a;  kappa = 3u spread + (K + 2)(XE + 1) u  (the arguments of the exponentials are
              differences of magnitude <= spread: the subtraction, the rescale argument and the merge argument each round
              once; every exponential and the product by it cost XE + 1);  loc = kappa + (n_r + 5) u  (the additions, the
              three of the merge, the reciprocal and the product by it)
  weights     |w_k - w64_k| <= w64_k (2 delta + u |a_k - M| + XE u + loc + 2u) + 2^-126
              (2 delta: the score and the maximum; the last term: a result below the smallest normal may be flushed to 0)
  statistics  |stats0 + stats1 - lse64| <= delta + loc + 4u |log L| + u (|M| + |log L|)
  LOCAL forward statements, on the evaluation's OWN w widened to float64 -- no delta in them, tight at 1e-6 .. 4e-5 relative:
              |out_c - sum_k w_k E_kc| <= loc sum_k w_k |E_kc| + 2^-126,      |sum_k w_k - 1| <= loc + 2u,
              n = 1: w == 1.0 and out == E[nbr] bit for bit
  mean        |out - ref| <= (n + 1) u mean_j |E_j|
  backward    cE[k] == float32(g w_k) bit for bit on any operands (one product); ds_rows / dr_rows are exact copies
              dd = R u sum_c |g_c E_kc|,  dc0 = R u sum_c |g_c out_c|,  dda = |w_k| (dd + dc0) + 2u |da|
              s = 1 - t^2:  ds = 2 |t| dt + u t^2 + u |s|    (the middle term is the `C` term of gru_statement.py)
              |cP - ref| <= |v| (|s| dda + |da| ds) + 2u |cP| + 2^-126
              dv term: |t| dda + |da| dt + u |t da|
              dq_rows / dv_rows: the sum of the term bounds + (n_r + 4) u sum_k |term|
              dq_rows against the sum of the evaluation's own cP rows: (n_r + 4) u sum_k |cP|

A quotient S / h (an exact integer sum over a count) is required BIT FOR BIT where h is a power of two; elsewhere
|got - S/h| <= 2u |S/h|, which admits a division as well as a multiplication by fl(1/h).

EXACT DESIGNS, each with its premise (tests/test_nbr_pool_statement_cpu.py asserts the premises):
  int_operands   E, dOut, out small integers (|.| <= 8): every sum over <= 1025 neighbours and every D-term dot product is
                 exact in fp32 in any order (`exactness_margin`).
  uniform        every row of P the same: all scores of a segment are the same bits whatever q and v are, so every
                 exponential is expf(0) == 1, l == n exactly:  w[k] == float32(1/n) bit for bit, out == S / n.
  hot_cold       v zero except v[c*] = 64; P[e, c*] = +30 on hot entities, -30 on cold ones; q[:, c*] = 0.  Premises:
                 tanhf(+-30) == +-1, expf(0) == 1, expf(-128) == 0.  Then the scores are exactly +-64, cold weights are exactly
                 0, a rescale from -64 to +64 multiplies by 0:  w == float32(1/h) on hot neighbours, 0 on cold ones,
                 out == S_hot / h, stats0 == 64, stats1 == 0 where h == 1.
  bwd_exact      E, dOut, out small integers, w in {1, 1/2, 1/4} (NOT a softmax: the kernel must not care), v in
                 {+-1/2, +-1, +-2}.  't0': P = q = 0 (t = 0): cE, da, cP = da v, dq_rows value-equal to float64, dv_rows == 0.
                 'pm30': P = +-30, q = 0 (t = +-1, 1 - t^2 = 0): cP == 0, dq_rows == 0, dv_rows[u][c] = sum_k +-da_k exact.

The census (`census`) is ONE deterministic batch shared by all widths; `census_facts` names what it contains by construction."""
import functools
import types

import numpy as np

U = 2.0 ** -24
XE = 4.0                                         # ulp of expf (taken), likewise 4 ulp for tanhf and logf
R_DOT = 12.0
TINY = 2.0 ** -126
SPLIT, WAVES, UNR_ATTN = 256, 4, 4               # the header: longer segments are split over the waves of a workgroup

N_ENT, N_REL, N_Q = 97, 5, 12
LENGTHS = (1, 2, 3, 4,
           5, 8, 9, 63,
           64, 65, 128, 129,
           255, 256, 7, 16,
           257, 1, 1, 1,
           2, 260, 3, 261,
           258, 259, 512, 1025,
           1000, 1023, 1024, 300,
           12, 6, 257)
SEG_REPEATED = 31                                # the segment of 300 copies of one entity id
REPEATED_ID = 41
PATTERNS = ('last', 'first', 'wave4', 'one_per_wave', 'pos63_64', 'pow2_spread')
FLOAT_KINDS = ('plain', 'ascending', 'large')
N_HOT_IDS = 48                                   # hot_cold: entities 1 .. 48 are hot, 0 and 49 .. 96 cold


def _freeze(o):
    for a in vars(o).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def f64(a):
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------
# the census batch
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def census():
    """-> the batch: nbr [nnz], seg_ptr [S + 1], seg_s / seg_r / seg_q / out_row [S] (int32), S, nnz."""
    rng = np.random.RandomState(7477)
    lens = np.asarray(LENGTHS, np.int64)
    S = len(lens)
    seg_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    nbr = rng.randint(0, N_ENT, int(seg_ptr[-1])).astype(np.int32)
    nbr[seg_ptr[SEG_REPEATED]:seg_ptr[SEG_REPEATED + 1]] = REPEATED_ID
    nbr[0], nbr[-1] = 0, N_ENT - 1                           # the first and the last id of the table, at both ends
    nbr[seg_ptr[13] + 255] = 0
    nbr[seg_ptr[27] + 1024] = N_ENT - 1
    nbr[seg_ptr[5]:seg_ptr[5] + 2] = 7                       # a repeat inside a short segment as well
    seg_s = rng.randint(0, N_ENT, S).astype(np.int32)
    seg_s[3], seg_s[S - 1] = 0, N_ENT - 1
    seg_r = rng.randint(0, N_REL, S).astype(np.int32)
    seg_r[0], seg_r[S - 1] = N_REL - 1, 0
    seg_q = rng.randint(0, N_Q, S).astype(np.int32)
    seg_q[2], seg_q[27], seg_q[S - 1], seg_q[S - 2] = 0, 0, N_Q - 1, N_Q - 1
    out_row = rng.permutation(S).astype(np.int32)
    return _freeze(types.SimpleNamespace(nbr=nbr, seg_ptr=seg_ptr, seg_s=seg_s, seg_r=seg_r, seg_q=seg_q, out_row=out_row,
                                         S=S, nnz=int(seg_ptr[-1])))


def with_nbr(batch, nbr):
    b = types.SimpleNamespace(**vars(batch))
    b.nbr = np.ascontiguousarray(nbr, np.int32)
    return _freeze(b)


def lengths(batch):
    return np.diff(batch.seg_ptr).astype(np.int64)


def seg_of(batch):
    return np.repeat(np.arange(batch.S), lengths(batch))


def sub_ranges(n):
    """The contiguous ranges of a segment of n > SPLIT neighbours over the waves: ceil(n / 4) each, the last one shorter."""
    sub = -(-n // WAVES)
    return [(min(w * sub, n), min(min(w * sub, n) + sub, n)) for w in range(WAVES)]


def census_facts():
    """The properties the GPU tests rely on, by name (tests/test_nbr_pool_statement_cpu.py asserts every one)."""
    b = census()
    n = lengths(b)
    wg = [tuple(int(x) for x in n[i:i + WAVES]) for i in range(0, b.S, WAVES)]
    longs = [[j for j, x in enumerate(g) if x > SPLIT] for g in wg]
    rep = [len(np.unique(b.nbr[b.seg_ptr[u]:b.seg_ptr[u + 1]])) < n[u] for u in range(b.S)]
    one = b.nbr[b.seg_ptr[SEG_REPEATED]:b.seg_ptr[SEG_REPEATED + 1]]
    return {
        'S': b.S, 'nnz': b.nnz, 'workgroups': wg,
        'S_mod_waves': b.S % WAVES,
        'last_workgroup_partly_filled_and_ends_long': len(wg[-1]) == 3 and wg[-1][-1] > SPLIT,
        'lengths_below_at_and_above_the_split': {255, 256, 257} <= set(n.tolist()),
        'lengths_around_the_batches': {1, 2, 3, 4, 5, 7, 8, 9, 16, 63, 64, 65, 128, 129} <= set(n.tolist()),
        'longest': int(n.max()),
        'ranges_of_257': [e - s for s, e in sub_ranges(257)],
        'long_at_slot_0_only': longs[4] == [0],
        'long_at_slots_1_and_3': longs[5] == [1, 3],
        'four_long_in_one_workgroup': longs[6] == [0, 1, 2, 3],
        'a_second_workgroup_of_four_long': longs[7] == [0, 1, 2, 3],
        'one_id_300_times': len(one) == 300 and len(np.unique(one)) == 1,
        'out_row_is_a_non_identity_permutation': (sorted(b.out_row.tolist()) == list(range(b.S))
                                                  and not np.array_equal(b.out_row, np.arange(b.S))),
        'seg_q_shares_rows': len(np.unique(b.seg_q)) < b.S,
        'seg_q_uses_first_and_last_row': b.seg_q.min() == 0 and b.seg_q.max() == N_Q - 1,
        'nbr_uses_first_and_last_id': b.nbr.min() == 0 and b.nbr.max() == N_ENT - 1,
        'seg_s_uses_first_and_last_id': b.seg_s.min() == 0 and b.seg_s.max() == N_ENT - 1,
        'seg_r_uses_first_and_last_id': b.seg_r.min() == 0 and b.seg_r.max() == N_REL - 1,
        'ids_repeat_inside_segments': int(np.sum(rep)) >= 20 and bool(rep[5]),
        'last_id_is_the_last_neighbour_of_1025': int(b.nbr[b.seg_ptr[27] + 1024]) == N_ENT - 1 and n[27] == 1025,
    }


# ---------------------------------------------------------------------------------------------
# ratios
# ---------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
    """worst error / bound; a non-finite `got` counts as infinitely wrong; 0 / 0 = 0 and x / 0 = inf."""
    got = f64(got)
    assert got.shape == np.shape(ref), (got.shape, np.shape(ref))
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def exact(got, ref):
    """0 where got == ref as values at every element (NaN is unequal), else inf."""
    got = f64(got)
    assert got.shape == np.shape(ref), (got.shape, np.shape(ref))
    return 0.0 if bool(np.all(got == ref)) else np.inf


def same_bits(got, ref32):
    got, ref32 = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref32, np.float32)
    assert got.shape == ref32.shape, (got.shape, ref32.shape)
    return 0.0 if np.array_equal(got.view(np.uint32), ref32.view(np.uint32)) else np.inf


def quotient_ratio(got, num, den):
    """got [S, D] against the exact integer sums num [S, D] over the counts den [S]: bit for bit where den is a power of two,
    else error / (2u |num / den|)."""
    den = np.asarray(den, np.int64)
    ref = f64(num) / den[:, None]
    pow2 = (den & (den - 1)) == 0
    bound = np.where(pow2[:, None], 0.0, 2 * U * np.abs(ref))
    return ratio(got, ref, bound)


def exactness_margin(mag, quantum=1.0):
    """2^24 / the largest magnitude (in units of `quantum`) an fp32 partial sum can reach: mag bounds every partial sum of
    any subset; > 1 with every term a multiple of quantum is the premise of an exact comparison."""
    return 2.0 ** 24 * quantum / max(float(np.max(mag)), quantum)


def assert_verdict(verdict, what=''):
    """verdict: check name -> worst error / bound, in the order the checks were made.  The first one beyond 1 fails."""
    for name, r in verdict.items():
        assert r <= 1.0, '%s: check `%s` failed, worst error / bound %.4g  (all: %s)' % (
            what, name, r, ', '.join('%s=%.3g' % kv for kv in verdict.items()))
    return max(verdict.values()) if verdict else 0.0


def failed(verdict):
    return [k for k, r in verdict.items() if not r <= 1.0]


# ---------------------------------------------------------------------------------------------
# the statement: forward
# ---------------------------------------------------------------------------------------------
def _n_r(n):
    return np.where(n <= SPLIT, n, -(-n // WAVES))


def forward(E, R, P, q, v, batch, attn):
    """-> namespace.  Both modes: out [S, parts * D] float64 (row out_row[u] = segment u), pooled [S, D] (by segment).
    mean: pooled_bound [S, D].  attention: a [nnz], w [nnz], w_bound [nnz], stats [S, 2], stats0_bound [S], lse [S],
    lse_bound [S], delta, spread, loc [S]."""
    b = batch
    D = E.shape[1]
    n = lengths(b)
    seg = seg_of(b)
    starts = b.seg_ptr[:-1].astype(np.int64)
    En = f64(E)[b.nbr]
    parts = 3 if attn else 2
    r = types.SimpleNamespace(attn=bool(attn), D=D, n=n)
    out = np.zeros((b.S, parts * D))
    out[b.out_row, D:2 * D] = f64(E)[b.seg_s]
    if attn:
        out[b.out_row, 2 * D:] = f64(R)[b.seg_r]
    if not attn:
        r.pooled = np.add.reduceat(En, starts, axis=0) / n[:, None]
        r.pooled_bound = (n + 1.0)[:, None] * U * np.add.reduceat(np.abs(En), starts, axis=0) / n[:, None]
    else:
        Pn, qn, va = f64(P)[b.nbr], f64(q)[b.seg_q][seg], np.abs(f64(v))
        t = np.tanh(Pn + qn)
        r.a = a = (t * f64(v)).sum(axis=1)
        dt = U * (np.abs(Pn) + np.abs(qn)) + 4 * U * np.abs(t)
        A = dt @ va + R_DOT * U * (np.abs(t) @ va)
        M = np.maximum.reduceat(a, starts)
        r.delta = delta = np.maximum.reduceat(A, starts)
        r.spread = spread = M - np.minimum.reduceat(a, starts)
        ex = np.exp(a - M[seg])
        L = np.add.reduceat(ex, starts)
        r.w = w = ex / L[seg]
        n_r = _n_r(n)
        K = -(-n_r // UNR_ATTN) + 1
        kappa = 3 * U * spread + (K + 2) * (XE + 1) * U
        r.loc = loc = kappa + (n_r + 5) * U
        r.w_bound = w * (2 * delta[seg] + U * np.abs(a - M[seg]) + XE * U + loc[seg] + 2 * U) + TINY
        logL = np.log(L)
        r.stats = np.stack((M, logL), axis=1)
        r.stats0_bound = delta
        r.lse = M + logL
        r.lse_bound = delta + loc + 4 * U * np.abs(logL) + U * (np.abs(M) + np.abs(logL))
        r.pooled = np.add.reduceat(w[:, None] * En, starts, axis=0)
    out[b.out_row, :D] = r.pooled
    r.out = out
    return r


def pooled_of(out, batch, D):
    return np.asarray(out)[batch.out_row, :D]


def copied_blocks(got_out, E, R, batch, attn):
    """the E[s] (and R[r]) column blocks of every packed row, bit for bit"""
    D = E.shape[1]
    got = np.asarray(got_out)[batch.out_row]
    r = same_bits(got[:, D:2 * D], np.asarray(E)[batch.seg_s])
    if attn:
        r = max(r, same_bits(got[:, 2 * D:3 * D], np.asarray(R)[batch.seg_r]))
    return r


def check_mean_forward(fw, got_out, E, batch):
    return {'mean out': ratio(pooled_of(got_out, batch, fw.D), fw.pooled, fw.pooled_bound),
            'copied E[s] block': copied_blocks(got_out, E, None, batch, False)}


def local_forward(got_out, got_w, E, batch, loc):
    """The two local statements and the n = 1 statement on the evaluation's own w -> verdict."""
    D = E.shape[1]
    n = lengths(batch)
    starts = batch.seg_ptr[:-1].astype(np.int64)
    w = f64(got_w)
    w = np.where(np.isfinite(w), w, np.inf)                   # an unwritten weight makes its segment infinitely wrong
    En = f64(E)[batch.nbr]
    with np.errstate(invalid='ignore', over='ignore'):
        ref = np.add.reduceat(w[:, None] * En, starts, axis=0)
        mag = np.add.reduceat(np.abs(w)[:, None] * np.abs(En), starts, axis=0)
        sw = np.add.reduceat(w, starts)
    got = pooled_of(got_out, batch, D)
    ref = np.where(np.isfinite(ref), ref, np.inf)
    one = n == 1
    first = starts[one]
    v = {'out against the own weights': ratio(got, ref, loc[:, None] * mag + TINY),
         'sum of the own weights': ratio(sw, np.ones(batch.S), loc + 2 * U),
         'n = 1: w == 1': same_bits(np.asarray(got_w)[first], np.ones(len(first), np.float32)),
         'n = 1: out == E[nbr]': same_bits(got[one], np.asarray(E)[batch.nbr[first]])}
    return v


def check_attn_forward(fw, got_out, got_w, got_stats, E, R, batch):
    st = f64(got_stats)
    v = {'w': ratio(got_w, fw.w, fw.w_bound),
         'stats0 (the maximum)': ratio(st[:, 0], fw.stats[:, 0], fw.stats0_bound),
         'stats0 + stats1 (log-sum-exp)': ratio(st[:, 0] + st[:, 1], fw.lse, fw.lse_bound)}
    v.update(local_forward(got_out, got_w, E, batch, fw.loc))
    v['copied E[s] / R[r] blocks'] = copied_blocks(got_out, E, R, batch, True)
    return v


# ---------------------------------------------------------------------------------------------
# the statement: backward
# ---------------------------------------------------------------------------------------------
def backward(dOut, out, E, P, q, v, w, batch, attn):
    """-> namespace of float64 cE [nnz, D], ds_rows [S, D] and, in attention mode, cP, dq_rows, dv_rows, dr_rows, da [nnz] with
    the bounds cP_bound, dq_bound, dv_bound and sum_bound(cP rows) of the header's statements."""
    b = batch
    D = np.shape(dOut)[1] // (3 if attn else 2)
    n = lengths(b)
    seg = seg_of(b)
    starts = b.seg_ptr[:-1].astype(np.int64)
    rows = f64(dOut)[b.out_row]
    g = rows[:, :D]
    r = types.SimpleNamespace(attn=bool(attn), D=D, n=n, g=g, ds_rows=rows[:, D:2 * D])
    if not attn:
        r.cE = (g / n[:, None])[seg]
        return r
    r.dr_rows = rows[:, 2 * D:]
    o = f64(out)[b.out_row, :D]
    En, Pn, qn = f64(E)[b.nbr], f64(P)[b.nbr], f64(q)[b.seg_q][seg]
    v64, w64 = f64(v), f64(w)
    gs = g[seg]
    d = np.einsum('kc,kc->k', gs, En)
    c0 = np.einsum('uc,uc->u', g, o)
    r.da = da = w64 * (d - c0[seg])
    t = np.tanh(Pn + qn)
    s = 1.0 - t * t
    r.cE = w64[:, None] * gs
    r.cP = cP = da[:, None] * v64[None, :] * s
    dvt = da[:, None] * t
    r.dq_rows = np.add.reduceat(cP, starts, axis=0)
    r.dv_rows = np.add.reduceat(dvt, starts, axis=0)
    # bounds
    dd = R_DOT * U * np.einsum('kc,kc->k', np.abs(gs), np.abs(En))
    dc0 = R_DOT * U * np.einsum('uc,uc->u', np.abs(g), np.abs(o))
    dda = np.abs(w64) * (dd + dc0[seg]) + 2 * U * np.abs(da)
    dt = U * (np.abs(Pn) + np.abs(qn)) + 4 * U * np.abs(t)
    ds = 2 * np.abs(t) * dt + U * t * t + U * np.abs(s)
    ada = np.abs(da)[:, None]
    r.cP_bound = np.abs(v64)[None, :] * (np.abs(s) * dda[:, None] + ada * ds) + 2 * U * np.abs(cP) + TINY
    dv_term = np.abs(t) * dda[:, None] + ada * dt + U * np.abs(t) * ada
    r.sum_factor = sf = ((_n_r(n) + 4) * U)[:, None]
    r.dq_bound = np.add.reduceat(r.cP_bound, starts, axis=0) + sf * np.add.reduceat(np.abs(cP), starts, axis=0)
    r.dv_bound = np.add.reduceat(dv_term, starts, axis=0) + sf * np.add.reduceat(np.abs(dvt), starts, axis=0)
    r.starts = starts
    return r


def check_attn_backward(bw, got, dOut, w, batch, exact_design=False):
    """got: dict of the six float32 results.  exact_design: cP, dq_rows, dv_rows are required value-equal to float64."""
    gs32 = np.asarray(dOut, np.float32)[batch.out_row][:, :bw.D][seg_of(batch)]
    v = {'cE == float32(g w) bit for bit': same_bits(got['cE'], gs32 * np.asarray(w, np.float32)[:, None]),
         'ds_rows copy': same_bits(got['ds_rows'], bw.ds_rows.astype(np.float32)),
         'dr_rows copy': same_bits(got['dr_rows'], bw.dr_rows.astype(np.float32))}
    if exact_design:
        v['cP exact'] = exact(got['cP'], bw.cP)
        v['dq_rows exact'] = exact(got['dq_rows'], bw.dq_rows)
        v['dv_rows exact'] = exact(got['dv_rows'], bw.dv_rows)
        return v
    v['cP'] = ratio(got['cP'], bw.cP, bw.cP_bound)
    v['dq_rows'] = ratio(got['dq_rows'], bw.dq_rows, bw.dq_bound)
    v['dv_rows'] = ratio(got['dv_rows'], bw.dv_rows, bw.dv_bound)
    own = f64(got['cP'])
    own = np.where(np.isfinite(own), own, np.inf)
    with np.errstate(invalid='ignore'):
        ref = np.add.reduceat(own, bw.starts, axis=0)
        mag = np.add.reduceat(np.abs(own), bw.starts, axis=0)
    v['dq_rows against the own cP rows'] = ratio(got['dq_rows'], np.where(np.isfinite(ref), ref, np.inf), bw.sum_factor * mag)
    return v


def check_mean_backward(bw, got, batch):
    """ds_rows an exact copy; the rows cE[k] of a segment carry the same bits; g / n bit for bit at power-of-two n, within
    2u |g / n| elsewhere."""
    seg = seg_of(batch)
    ce = np.ascontiguousarray(got['cE'], np.float32)
    first = ce[batch.seg_ptr[:-1].astype(np.int64)]
    return {'ds_rows copy': same_bits(got['ds_rows'], bw.ds_rows.astype(np.float32)),
            'cE rows of a segment carry the same bits': same_bits(ce, first[seg]),
            'cE == g / n': quotient_ratio(first, bw.g, bw.n)}


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_operands(d):
    """Small integers in [-8, 8]: E, R, dOut [S, 3d] (mean mode takes its first 2d columns) and a packed `out` [S, 3d]."""
    rng = np.random.RandomState(1000 + d)
    S = census().S

    def ints(*shape):
        return rng.randint(-8, 9, shape).astype(np.float32)
    return _freeze(types.SimpleNamespace(kind='int', d=d, E=ints(N_ENT, d), R=ints(N_REL, d), dOut=ints(S, 3 * d),
                                         out=ints(S, 3 * d), batch=census()))


def _scores64(P, q, v, batch):
    return (np.tanh(f64(P)[batch.nbr] + f64(q)[batch.seg_q][seg_of(batch)]) * f64(v)).sum(axis=1)   # (equal rows: equal bits)


@functools.lru_cache(maxsize=None)
def float_operands(d, kind):
    """Seeded randn operands.  'plain': scores of spread about 2-3.  'ascending': the same operands with the neighbours of
    every segment sorted by float64 score, so the running maximum moves in every batch of every wave.  'large': v scaled so
    that max |a_j| lies in [55, 60]."""
    assert kind in FLOAT_KINDS
    rng = np.random.RandomState(3000 + d)
    b = census()

    def rn(*shape):
        return rng.randn(*shape).astype(np.float32)
    o = types.SimpleNamespace(kind=kind, d=d, E=rn(N_ENT, d), R=rn(N_REL, d), P=rn(N_ENT, d), q=rn(N_Q, d),
                              v=(rng.randn(d) * 0.9 / np.sqrt(d)).astype(np.float32), dOut=rn(b.S, 3 * d), batch=b)
    if kind == 'ascending':
        a = _scores64(o.P, o.q, o.v, b)
        nbr = b.nbr.copy()
        for u in range(b.S):
            k0, k1 = int(b.seg_ptr[u]), int(b.seg_ptr[u + 1])
            nbr[k0:k1] = nbr[k0:k1][np.argsort(a[k0:k1], kind='stable')]
        o.batch = with_nbr(b, nbr)
    elif kind == 'large':
        o.v = (o.v * np.float32(57.5 / np.abs(_scores64(o.P, o.q, o.v, b)).max())).astype(np.float32)
    return _freeze(o)


# ---------------------------------------------------------------------------------------------
# exact designs for attention
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uniform(d):
    """Every row of P the same (q, v random floats): w_exact [nnz] float32 = 1 / n, num [S, d] the exact integer row sums."""
    op = int_operands(d)
    rng = np.random.RandomState(4000 + d)
    b = op.batch
    n = lengths(b)
    P = np.repeat(rng.randn(1, d).astype(np.float32), N_ENT, axis=0)
    o = types.SimpleNamespace(kind='uniform', d=d, E=op.E, R=op.R, P=P, q=rng.randn(N_Q, d).astype(np.float32),
                              v=rng.randn(d).astype(np.float32), batch=b, h=n, hot=np.ones(b.nnz, bool),
                              w_exact=(np.float32(1) / n.astype(np.float32))[seg_of(b)],
                              num=np.add.reduceat(f64(op.E)[b.nbr], b.seg_ptr[:-1].astype(np.int64), axis=0))
    return _freeze(o)


def hot_positions(n, pattern):
    """The hot positions of a segment of n neighbours (never empty)."""
    sub = -(-n // WAVES)
    ranges = [(s, e) for s, e in ((min(w * sub, n), min(min(w * sub, n) + sub, n)) for w in range(WAVES)) if e > s]
    if pattern == 'last':                # in a clamped tail batch wherever n is no multiple of 4
        return [n - 1]
    if pattern == 'first':
        return [0]
    if pattern == 'wave4':               # only neighbours of the fourth wave's range (of the last quarter, if unsplit)
        return list(range(min(3 * sub, n - 1), n))
    if pattern == 'one_per_wave':        # exactly one per wave range, at a different offset in each
        return [s + (7 * w + 3) % (e - s) for w, (s, e) in enumerate(ranges)]
    if pattern == 'pos63_64':            # the last lane of the first round of parked scores and the first of the second
        return [p for p in (63, 64) if p < n] or [n - 1]
    if pattern == 'pow2_spread':         # a power-of-two count spread evenly
        h = 1
        while h * 2 <= min(n, 16):
            h *= 2
        return [(i * n) // h for i in range(h)]
    raise ValueError(pattern)


@functools.lru_cache(maxsize=None)
def hot_cold(d, pattern, cstar):
    """v = 64 e_c*, P[e, c*] = +30 on the hot entities 1 .. 48 and -30 on the others, q[:, c*] = 0; the other columns of P and
    q are random floats (v is 0 there).  The census with its ids mapped so that exactly the pattern's positions are hot."""
    op = int_operands(d)
    rng = np.random.RandomState(5000 + d)
    b0 = op.batch
    n = lengths(b0)
    hot = np.zeros(b0.nnz, bool)
    for u in range(b0.S):
        hot[int(b0.seg_ptr[u]) + np.asarray(hot_positions(int(n[u]), pattern), np.int64)] = True
    base = b0.nbr.astype(np.int64) % N_HOT_IDS
    nbr = np.where(hot, base + 1, base + 1 + N_HOT_IDS)
    nbr[(~hot) & (b0.nbr == 0)] = 0                           # keep the first id of the table (cold)
    b = with_nbr(b0, nbr)
    P = rng.randn(N_ENT, d).astype(np.float32)
    q = rng.randn(N_Q, d).astype(np.float32)
    v = np.zeros(d, np.float32)
    ids = np.arange(N_ENT)
    P[:, cstar] = np.where((ids >= 1) & (ids <= N_HOT_IDS), 30.0, -30.0)
    q[:, cstar] = 0.0
    v[cstar] = 64.0
    starts = b.seg_ptr[:-1].astype(np.int64)
    h = np.add.reduceat(hot.astype(np.int64), starts)
    w_exact = np.where(hot, (np.float32(1) / h.astype(np.float32))[seg_of(b)], np.float32(0)).astype(np.float32)
    num = np.add.reduceat(f64(op.E)[b.nbr] * hot[:, None], starts, axis=0)
    return _freeze(types.SimpleNamespace(kind='hot_cold', pattern=pattern, cstar=cstar, d=d, E=op.E, R=op.R, P=P, q=q, v=v,
                                         batch=b, h=h, hot=hot, w_exact=w_exact, num=num))


PREMISE = 'premise tanhf(+-30) == +-1, expf(0) == 1, expf(-128) == 0: stats0 == 64.0'


def check_exact_forward(design, got_out, got_w, got_stats):
    """The verdict of an exact attention design (uniform or hot_cold); the premise first."""
    o = design
    st = np.ascontiguousarray(got_stats, np.float32)
    v = {}
    if o.kind == 'hot_cold':
        v[PREMISE] = same_bits(st[:, 0], np.full(o.batch.S, 64.0, np.float32))
    v['w == float32(1/h) on hot neighbours, 0 on cold ones'] = same_bits(got_w, o.w_exact)
    v['out == S_hot / h'] = quotient_ratio(pooled_of(got_out, o.batch, o.d), o.num, o.h)
    one = o.h == 1
    v['stats1 == 0 where h == 1'] = exact(st[one, 1], np.zeros(int(one.sum())))
    # logf within 4 ulp (taken, as in the log-sum-exp bound)
    v['stats1 against log h'] = ratio(st[:, 1], np.log(f64(o.h)), 4 * U * np.log(f64(o.h)))
    v['copied E[s] / R[r] blocks'] = copied_blocks(got_out, o.E, o.R, o.batch, True)
    return v


# ---------------------------------------------------------------------------------------------
# exact designs for the backward
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bwd_exact(d, kind):
    """kind 't0': P = q = 0.  kind 'pm30': P = +-30 (a seeded sign per entity and column), q = 0.  w in {1, 1/2, 1/4} (no
    softmax), v in {+-1/2, +-1, +-2}, E / dOut / out small integers."""
    op = int_operands(d)
    rng = np.random.RandomState(6000 + d)
    b = op.batch
    w = rng.choice(np.asarray([1.0, 0.5, 0.25], np.float32), b.nnz)
    v = (rng.choice(np.asarray([0.5, 1.0, 2.0], np.float32), d) * rng.choice(np.asarray([-1.0, 1.0], np.float32), d))
    P = np.zeros((N_ENT, d), np.float32)
    if kind == 'pm30':
        P = (rng.choice(np.asarray([-30.0, 30.0], np.float32), (N_ENT, d))).astype(np.float32)
    else:
        assert kind == 't0'
    return _freeze(types.SimpleNamespace(kind=kind, d=d, E=op.E, P=P, q=np.zeros((N_Q, d), np.float32),
                                         v=v.astype(np.float32), w=w.astype(np.float32), dOut=op.dOut, out=op.out, batch=b))


def bwd_exact_margins(o):
    """The exactness margins of a backward exact design: the dot products (integers), da (multiples of 1/4), and the
    per-segment sums of cP (multiples of 1/8) and of da t (multiples of 1/4)."""
    b = o.batch
    seg = seg_of(b)
    starts = b.seg_ptr[:-1].astype(np.int64)
    g = np.abs(f64(o.dOut)[b.out_row][:, :o.d])
    dot = max((g[seg] * np.abs(f64(o.E)[b.nbr])).sum(1).max(), (g * np.abs(f64(o.out)[b.out_row, :o.d])).sum(1).max())
    bw = backward(o.dOut, o.out, o.E, o.P, o.q, o.v, o.w, b, True)
    t = np.tanh(f64(o.P)[b.nbr])
    return {'dot': exactness_margin(2 * dot), 'da': exactness_margin(np.abs(bw.da), 0.25),
            'sum cP': exactness_margin(np.add.reduceat(np.abs(bw.cP), starts, axis=0), 0.125),
            'sum da t': exactness_margin(np.add.reduceat(np.abs(bw.da)[:, None] * np.abs(t), starts, axis=0), 0.25)}


# ---------------------------------------------------------------------------------------------
# float32 emulations of the C ABI in two orders, and what a subtly wrong kernel would return
# (tests/test_nbr_pool_statement_cpu.py: the emulations stay within every bound, every planted fault is caught)
# ---------------------------------------------------------------------------------------------
FWD_FAULTS = ('no_rescale', 'tail_counted', 'last_of_1025_dropped', 'w_wave_local', 'merge_l_without_f', 'stale_merge_row',
              'last_segment_skipped')
BWD_FAULTS = ('c0_zero', 'dv_without_da')
F32 = np.float32


def _dot32(x, y, order):
    """Row-wise fp32 dot products of [k, D] arrays: four at a time, then a binary tree over the (zero-padded) 128 chunks --
    'online': halves (a lane's two chunks, then the butterfly); 'twopass': neighbouring pairs.  At most 11 roundings."""
    p = (x * y).astype(F32)
    k, D = p.shape
    p = p.reshape(k, D // 4, 4)
    c = ((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]) + p[:, :, 3]
    c = np.concatenate((c, np.zeros((k, 128 - D // 4), F32)), axis=1)
    while c.shape[1] > 1:
        h = c.shape[1] // 2
        c = (c[:, :h] + c[:, h:]) if order == 'online' else (c[:, 0::2] + c[:, 1::2])
    return c[:, 0]


def _scores32(P, q, v, b, order):
    x = (np.asarray(P, F32)[b.nbr] + np.asarray(q, F32)[b.seg_q][seg_of(b)]).astype(F32)
    t = np.tanh(x).astype(F32)
    return _dot32(t, np.broadcast_to(np.asarray(v, F32), t.shape), order), t


def _online_range(a, En, kb, ke, fault):
    """(m, l, acc) of the neighbours [kb, ke): batches of four, the tail clamped to the last neighbour with score -inf."""
    m, l, acc = F32(-np.inf), F32(0), np.zeros(En.shape[1], F32)
    for k in range(kb, ke, UNR_ATTN):
        idx = np.minimum(np.arange(k, k + UNR_ATTN), ke - 1)
        live = np.arange(k, k + UNR_ATTN) < ke
        s = a[idx] if fault == 'tail_counted' else np.where(live, a[idx], F32(-np.inf)).astype(F32)
        mb = max(m, s.max())
        if mb > m:
            if fault != 'no_rescale':
                r = np.exp(F32(m - mb))
                l = F32(l * r)
                acc = acc * r
            m = mb
        for j in range(UNR_ATTN):
            wj = np.exp(F32(s[j] - m))
            l = F32(l + wj)
            acc = acc + En[idx[j]] * wj
    return m, l, acc


def emulate_forward(E, R, P, q, v, batch, attn, order, fault=None):
    """float32 forward -> (out [S, parts * D], w [nnz], stats [S, 2]); everything not written stays NaN.
    order 'twopass': max, exponentials, serial sums over the whole segment, weights by division.
    order 'online':  the online softmax in batches of four with the four-range split above 256 and the merge in wave order;
    only this order takes a `fault`."""
    b = batch
    E = np.asarray(E, F32)
    D = E.shape[1]
    n = lengths(b)
    parts = 3 if attn else 2
    out = np.full((b.S, parts * D), np.nan, F32)
    w = np.full(b.nnz, np.nan, F32)
    stats = np.full((b.S, 2), np.nan, F32)
    En = E[b.nbr]
    if attn:
        a, _ = _scores32(P, q, v, b, order)
    stale = None
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        for u in range(b.S):
            if fault == 'last_segment_skipped' and u == b.S - 1:
                continue
            if u % WAVES == 0:
                stale = None
            k0, k1 = int(b.seg_ptr[u]), int(b.seg_ptr[u + 1])
            row = int(b.out_row[u])
            out[row, D:2 * D] = E[b.seg_s[u]]
            if attn:
                out[row, 2 * D:] = np.asarray(R, F32)[b.seg_r[u]]
            rngs = [(k0, k1)] if n[u] <= SPLIT or order == 'twopass' else [(k0 + s, k0 + e) for s, e in sub_ranges(int(n[u]))]
            if not attn:
                acc = np.zeros(D, F32)
                for kb, ke in rngs:
                    acc = acc + np.cumsum(En[kb:ke], axis=0, dtype=F32)[-1]
                out[row, :D] = acc / F32(n[u])
                continue
            if order == 'twopass':
                m = a[k0:k1].max()
                e = np.exp((a[k0:k1] - m).astype(F32))
                l = np.cumsum(e, dtype=F32)[-1]
                w[k0:k1] = e / l
                out[row, :D] = np.cumsum(w[k0:k1, None] * En[k0:k1], axis=0, dtype=F32)[-1]
                stats[u] = m, np.log(l)
                continue
            if fault == 'last_of_1025_dropped' and n[u] == 1025:
                rngs[-1] = (rngs[-1][0], rngs[-1][1] - 1)
            st = [_online_range(a, En, kb, ke, fault) for kb, ke in rngs]
            if len(st) == 1:
                M, L, acc = st[0]
            else:
                M = max(s[0] for s in st)
                f = [np.exp(F32(s[0] - M)) for s in st]
                L, acc = F32(0), np.zeros(D, F32)
                for i, s in enumerate(st):
                    L = F32(L + (s[1] if fault == 'merge_l_without_f' else F32(s[1] * f[i])))
                    row_i = stale if (fault == 'stale_merge_row' and i == WAVES - 1 and stale is not None) else s[2]
                    acc = acc + row_i * f[i]
                stale = st[-1][2]
            inv = F32(1) / L
            out[row, :D] = acc * inv
            stats[u] = M, np.log(L)
            for (kb, ke), s in zip(rngs, st):
                if fault == 'w_wave_local':
                    w[kb:ke] = np.exp((a[kb:ke] - s[0]).astype(F32)) * (F32(1) / s[1])
                else:
                    w[kb:ke] = np.exp((a[kb:ke] - M).astype(F32)) * inv
    return out, w, stats


def emulate_backward(dOut, out, E, P, q, v, w, batch, attn, order, fault=None):
    """float32 backward -> dict of the six results.  order 'twopass': serial sums over the whole segment, cE of the mean by
    division; order 'online': the four-range split above 256 merged in wave order, cE of the mean by the reciprocal."""
    b = batch
    dOut = np.asarray(dOut, F32)
    D = dOut.shape[1] // (3 if attn else 2)
    n = lengths(b)
    seg = seg_of(b)
    rows = dOut[b.out_row]
    g = rows[:, :D]
    got = {'ds_rows': rows[:, D:2 * D].copy()}
    if not attn:
        r = (g / n.astype(F32)[:, None]) if order == 'twopass' else g * (F32(1) / n.astype(F32))[:, None]
        got['cE'] = r.astype(F32)[seg]
        return got
    got['dr_rows'] = rows[:, 2 * D:].copy()
    w = np.asarray(w, F32)
    d = _dot32(g[seg], np.asarray(E, F32)[b.nbr], order)
    c0 = _dot32(g, np.asarray(out, F32)[b.out_row, :D], order)
    if fault == 'c0_zero':
        c0 = np.zeros_like(c0)
    da = (w * (d - c0[seg]).astype(F32)).astype(F32)
    _, t = _scores32(P, q, v, b, order)
    s = (F32(1) - (t * t).astype(F32)).astype(F32)
    got['cE'] = (g[seg] * w[:, None]).astype(F32)
    got['cP'] = cP = ((np.asarray(v, F32)[None, :] * s).astype(F32) * da[:, None]).astype(F32)
    dvt = t.copy() if fault == 'dv_without_da' else (t * da[:, None]).astype(F32)
    dq, dv = np.zeros((b.S, D), F32), np.zeros((b.S, D), F32)
    for u in range(b.S):
        k0, k1 = int(b.seg_ptr[u]), int(b.seg_ptr[u + 1])
        rngs = [(k0, k1)] if n[u] <= SPLIT or order == 'twopass' else [(k0 + s_, k0 + e) for s_, e in sub_ranges(int(n[u]))]
        for src, dst in ((cP, dq), (dvt, dv)):
            part = [np.cumsum(src[kb:ke], axis=0, dtype=F32)[-1] for kb, ke in rngs]
            acc = part[0]
            for p_ in part[1:]:
                acc = acc + p_
            dst[u] = acc
    got['dq_rows'], got['dv_rows'] = dq, dv
    return got
