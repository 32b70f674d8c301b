"""A float64 statement of ONE GRU step and of the backward recurrence over packed rows, each paired with its error bound
(numpy only: importable without a GPU).  tests/test_gru_statement_cpu.py keeps the bounds honest (float64 torch.nn.GRU, a
plain float32 evaluation and an emulation of the six-pair bf16 split product go through them); tests/test_gpu_gru.py puts
the HIP recurrences (re-net_amd/csrc/gru*.hip) through the same functions.

Every saved quantity is checked against a statement built from the implementation's OWN upstream saved values (as the fused
Adam test advances from the kernel's state), so errors do not compound over steps and every bound is local.

Notation: u = 2^-24.  Packed row p of step j holds saved[p] = r | z | n | hn | hp (5H wide) and the input gi[p] (3H wide);
off[j] is the first packed row of step j, the batch is length-sorted (the sequences alive at a step are a prefix).

Forward, per gate g, with T_g = |hp| |W_g|^T + |b_g| and E_g = (c_mm u + m) T_g:
  c_mm = MFMA instructions that accumulate into one element + 2 (6 ceil(K/32) + 2 for the six-pair bf16 products,
         ceil(K/4) + 2 for the f32-input MFMA, ceil(K/32) + 2 for the one-plane bf16 mode): at most one fp32 rounding of
         size u T per instruction, one for the bias add, one to spare.  m = 2^-7 + 2^-16 in the one-plane mode, else 0:
         both operands are rounded to bf16, 8 significant bits, unit roundoff 2^-8 each, (1 + 2^-8)^2 - 1 = 2^-7 + 2^-16.
         (Corrected from 2^-8 + 2^-16, which takes bf16's unit roundoff for 2^-9: the one-plane HOST evaluation left that
         bound on the single products of backward_product_case, error / bound 1.86, where nothing averages.)
  hn  vs hp W_n^T + b_n                          bound E_n
  r,z vs s = sigma(a), a = gi_g + hp W_g^T + b_g bound (E_g + 2u(|gi_g| + |gh_g|)) / 4 + S,
         S = u (2|a| + 16) s(1-s) + 2u s + 2^-126 (argument scaling of __expf, a few ulp, the reciprocal; a result below
         the smallest normal fp32 may be flushed to 0: sigma(-100) = 4e-44 is not representable)
  n   vs tanh(gi_n + r hn)  (saved r, hn)        bound 3u(|gi_n| + |r hn|) + 4u|n|
  h'  vs (1-z) n + z hp     (saved z, n, hp)     bound 3u(|(1-z) n| + |z hp|);  h' = hp of the same sequence at the next
         step, or its h_last row; hp at step 0 and the rows [B, out_rows) of h_last are exactly 0.

Backward, driven by saved (forward error excluded):  dn = dh(1-z), dz = dh(hp-n), da_n = dn(1-n^2), da_z = dz z(1-z),
da_r = da_n hn r(1-r), dGi = [da_r, da_z, da_n], dGh = [da_r, da_z, da_n r], dh_prev = dGh W_hh + z dh.  A running bound
E_dh travels with dh (0 where dh = dh_last):
  out in dGi / dGh:  |d out / d dh| E_dh + 8u|out| + C,   C = u n^2 |dn| |d out / d da_n|
         (C: the kernels form 1 - n*n in fp32; the rounding of n*n is an ABSOLUTE error u n^2 of the factor, which 8u|out|
         does not cover where 1 - n^2 is tiny -- saturated candidate gates.)
  dh_prev: E(dGh)|W| (1 + m) + (c_mm' u + m)(|dGh||W|) + c_mm' u |z dh| + z E_dh + 2u(|z dh| + |dGh||W|), c_mm' as above at K = 3H
         (the direct term z dh is the initial value of the MFMA accumulator in the persistent kernels: it takes part in
         every accumulation rounding, so it stands next to |dGh||W| under c_mm').
  bf16 outputs (bf16out): + max(2^-8 |ref|, 2^-134) + 2^-8 (bound so far)   (one RNE rounding, 8 significant bits, of the
         COMPUTED value, which is within the bound so far of ref)
  inside one step, exact: dGh_r == dGi_r and dGh_z == dGi_z bit for bit; dGh_n within 1 ulp of fl(dGi_n * r).
"""
import numpy as np

U = 2.0 ** -24
ROUTES = ('bf16x6', 'f32', 'bf16')
M_BF16 = 2.0 ** -7 + 2.0 ** -16
PAIRS6 = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))           # mfma6 of gru_common.h: smallest first


def c_mm(route, k):
    return {'bf16x6': 6 * -(-k // 32), 'f32': -(-k // 4), 'bf16': -(-k // 32)}[route] + 2


def m_rel(route):
    return M_BF16 if route == 'bf16' else 0.0


def offsets(lens, nstep=None):
    """Length-sorted sequence lengths -> packed step offsets [nstep + 1]."""
    assert list(lens) == sorted(lens, reverse=True)
    nstep = max(lens) if nstep is None else nstep
    off = [0]
    for j in range(nstep):
        off.append(off[-1] + sum(1 for n in lens if n > j))
    return off


def case(h, lens, seed=5, wscale=0.05, nstep=None):
    """Random float32 inputs of one problem: small W_hh (0.05 randn: gates far from saturation), b_hh, gi, dh_last."""
    rng = np.random.RandomState(seed)
    off = offsets(lens, nstep)
    f = np.float32
    return dict(h=h, off=off, lens=list(lens), gi=rng.randn(off[-1], 3 * h).astype(f),
                w=(wscale * rng.randn(3 * h, h)).astype(f), b=(0.5 * rng.randn(3 * h)).astype(f),
                dh=rng.randn(len(lens), h).astype(f))


def saturated_case(h, seed=21):
    """Rows whose gi holds +-30 and +-1e4 in each gate (a fifth of the elements, every step), b_hh of +-20 on a fifth of
    the units."""
    rng = np.random.RandomState(seed)
    c = case(h, [3] * 14 + [2] * 5 + [1] * 2, seed=seed)
    gi, b = c['gi'], c['b']
    vals = np.array([30, -30, 1e4, -1e4], np.float32)
    pick = rng.rand(*gi.shape) < 0.2
    gi[pick] = vals[rng.randint(0, 4, int(pick.sum()))]
    pick = rng.rand(3 * h) < 0.2
    b[pick] = rng.choice([20, -20], int(pick.sum())).astype(np.float32)
    return c


def _sigmoid(a):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-a))


def _gates(sv, h):
    return sv[:, :h], sv[:, h:2 * h], sv[:, 2 * h:3 * h], sv[:, 3 * h:4 * h], sv[:, 4 * h:5 * h]


def ratio(err, bound):
    """err / bound elementwise; 0 where err == 0; inf where the bound is 0 (or anything is NaN) and err is not."""
    with np.errstate(all='ignore'):
        q = err / bound
    q = np.where(err == 0, 0.0, q)
    return np.where(np.isnan(q), np.inf, q)


# ---- the recurrence itself in float64 ---------------------------------------------------------------------------------
def forward_f64(gi, off, w_hh, b_hh, out_rows=None):
    gi, w, b = np.asarray(gi, np.float64), np.asarray(w_hh, np.float64), np.asarray(b_hh, np.float64)
    h, nb = w.shape[1], off[1] - off[0]
    hcur = np.zeros((max(nb, out_rows or 0), h))
    saved = np.zeros((off[-1], 5 * h))
    for j in range(len(off) - 1):
        bs = off[j + 1] - off[j]
        hp = hcur[:bs]
        gh = hp @ w.T + b
        g = gi[off[j]:off[j + 1]]
        r, z = _sigmoid(g[:, :h] + gh[:, :h]), _sigmoid(g[:, h:2 * h] + gh[:, h:2 * h])
        n = np.tanh(g[:, 2 * h:] + r * gh[:, 2 * h:])
        saved[off[j]:off[j + 1]] = np.concatenate([r, z, n, gh[:, 2 * h:], hp], 1)
        hcur[:bs] = (1 - z) * n + z * hp
    return hcur, saved


def backward_f64(dh_last, off, w_hh, saved):
    out = backward_ratios('f32', dh_last, off, w_hh, saved, None, None)
    return out['ref_dGi'], out['ref_dGh']


# ---- statements with bounds -------------------------------------------------------------------------------------------
def forward_ratios(route, gi, off, w_hh, b_hh, saved, h_last):
    """error / bound of every forward statement -> {name: array}; r, z, n, hn, h_next, hp0: one value per packed row (the
    worst unit); h_pad: per padding row of h_last.  Everything <= 1 means the statements hold."""
    gi, w, b = np.asarray(gi, np.float64), np.asarray(w_hh, np.float64), np.asarray(b_hh, np.float64)
    sv32, hl32 = np.asarray(saved), np.asarray(h_last)
    sv, hl = sv32.astype(np.float64), hl32.astype(np.float64)
    h, nb, nrow = w.shape[1], off[1] - off[0], off[-1]
    assert sv.shape == (nrow, 5 * h) and gi.shape == (nrow, 3 * h) and hl.shape[0] >= nb
    r, z, n, hn, hp = _gates(sv, h)
    live = np.flatnonzero(np.any(hp != 0, 1))          # rows with hp = 0 (step 0): gh = b exactly, T = |b|
    gh, t = np.tile(b, (nrow, 1)), np.tile(np.abs(b), (nrow, 1))
    if len(live):
        gh[live] += hp[live] @ w.T
        t[live] += np.abs(hp[live]) @ np.abs(w).T
    e = (c_mm(route, h) * U + m_rel(route)) * t
    out = {'hn': ratio(np.abs(hn - gh[:, 2 * h:]), e[:, 2 * h:]).max(1)}
    for name, got, c in (('r', r, 0), ('z', z, 1)):
        g_, gh_, e_ = gi[:, c * h:(c + 1) * h], gh[:, c * h:(c + 1) * h], e[:, c * h:(c + 1) * h]
        a = g_ + gh_
        s = _sigmoid(a)
        bound = 0.25 * (e_ + 2 * U * (np.abs(g_) + np.abs(gh_))) + U * (2 * np.abs(a) + 16) * s * (1 - s) + 2 * U * s \
            + 2.0 ** -126
        out[name] = ratio(np.abs(got - s), bound).max(1)
    gn = gi[:, 2 * h:]
    out['n'] = ratio(np.abs(n - np.tanh(gn + r * hn)), 3 * U * (np.abs(gn) + np.abs(r * hn)) + 4 * U * np.abs(n)).max(1)
    succ = np.empty((nrow, h))                                           # h' as the implementation handed it on
    for j in range(len(off) - 1):
        bs = off[j + 1] - off[j]
        bs_next = off[j + 2] - off[j + 1] if j + 2 < len(off) else 0
        succ[off[j]:off[j] + bs_next] = hp[off[j + 1]:off[j + 1] + bs_next]
        succ[off[j] + bs_next:off[j + 1]] = hl[bs_next:bs]
    a1, a2 = (1 - z) * n, z * hp
    out['h_next'] = ratio(np.abs(succ - (a1 + a2)), 3 * U * (np.abs(a1) + np.abs(a2))).max(1)
    out['hp0'] = np.where(np.all(sv32[:nb, 4 * h:] == 0, 1), 0.0, np.inf)
    out['h_pad'] = np.where(np.all(hl32[nb:] == 0, 1), 0.0, np.inf)
    return out


def backward_ratios(route, dh_last, off, w_hh, saved, d_gi, d_gh, out16=False):
    """error / bound of dGi, dGh per packed row (the worst unit) and of the identities inside a step -> {name: array};
    d_gi = None: only the float64 recurrence ('ref_dGi', 'ref_dGh')."""
    w, sv = np.asarray(w_hh, np.float64), np.asarray(saved).astype(np.float64)
    h, nb, nrow = w.shape[1], off[1] - off[0], off[-1]
    aw = np.abs(w)
    dh = np.array(np.asarray(dh_last)[:nb], np.float64)
    e_dh = np.zeros_like(dh)
    cm, m = c_mm(route, 3 * h), m_rel(route)
    ref_i, ref_h, b_i, b_h = (np.zeros((nrow, 3 * h)) for _ in range(4))
    for j in range(len(off) - 2, -1, -1):
        p0, bs = off[j], off[j + 1] - off[j]
        r, z, n, hn, hp = _gates(sv[p0:p0 + bs], h)
        g, e = dh[:bs], e_dh[:bs]
        cn = (1 - z) * (1 - n * n)
        cz = (hp - n) * z * (1 - z)
        kr = hn * r * (1 - r)
        canc = U * n * n * np.abs(g * (1 - z))                           # the rounding of n*n inside 1 - n*n
        da_n, da_z = g * cn, g * cz
        da_r, dh_n = da_n * kr, da_n * r
        bn = np.abs(cn) * e + 8 * U * np.abs(da_n) + canc
        bz = np.abs(cz) * e + 8 * U * np.abs(da_z)
        br = np.abs(cn * kr) * e + 8 * U * np.abs(da_r) + canc * np.abs(kr)
        bhn = np.abs(cn * r) * e + 8 * U * np.abs(dh_n) + canc * np.abs(r)
        ref_i[p0:p0 + bs] = np.concatenate([da_r, da_z, da_n], 1)
        ref_h[p0:p0 + bs] = np.concatenate([da_r, da_z, dh_n], 1)
        b_i[p0:p0 + bs] = np.concatenate([br, bz, bn], 1)
        b_h[p0:p0 + bs] = np.concatenate([br, bz, bhn], 1)
        if j > 0:
            direct = z * g
            tm = np.abs(ref_h[p0:p0 + bs]) @ aw
            e_new = (b_h[p0:p0 + bs] @ aw) * (1 + m) + (cm * U + m) * tm + cm * U * np.abs(direct) + z * e \
                + 2 * U * (np.abs(direct) + tm)
            dh[:bs] = ref_h[p0:p0 + bs] @ w + direct
            e_dh[:bs] = e_new
    out = {'ref_dGi': ref_i, 'ref_dGh': ref_h}
    if d_gi is None:
        return out
    gi32, gh32 = np.asarray(d_gi, np.float32), np.asarray(d_gh, np.float32)
    assert gi32.shape == (nrow, 3 * h) and gh32.shape == (nrow, 3 * h)
    if out16:
        b_i = b_i + np.maximum(2.0 ** -8 * np.abs(ref_i), 2.0 ** -134) + 2.0 ** -8 * b_i
        b_h = b_h + np.maximum(2.0 ** -8 * np.abs(ref_h), 2.0 ** -134) + 2.0 ** -8 * b_h
    out['dGi'] = ratio(np.abs(gi32.astype(np.float64) - ref_i), b_i).max(1)
    out['dGh'] = ratio(np.abs(gh32.astype(np.float64) - ref_h), b_h).max(1)
    if not out16:                                                        # (two roundings to bf16 do not keep them)
        same = np.all(gi32[:, :2 * h].view(np.int32) == gh32[:, :2 * h].view(np.int32), 1)
        out['dGh_rz_is_dGi_rz'] = np.where(same, 0.0, np.inf)
        prod = gi32[:, 2 * h:] * np.asarray(saved, np.float32)[:, :h]    # fl(dGi_n * r)
        with np.errstate(invalid='ignore'):
            ulp = np.maximum(np.spacing(np.abs(prod)), np.float32(2.0 ** -149))
            out['dGh_n_is_dGi_n_r'] = ratio(np.abs(gh32[:, 2 * h:].astype(np.float64) - prod), ulp.astype(np.float64)).max(1)
    return out


def worst(ratios):
    """{name: largest ratio} of a forward_ratios / backward_ratios result."""
    return {k: (float(np.max(v)) if np.size(v) else 0.0) for k, v in ratios.items() if not k.startswith('ref_')}


def assert_holds(ratios, what, describe_row=None):
    """Raises with the worst quantity and its packed row when a ratio exceeds 1 (or is NaN)."""
    for k, v in ratios.items():
        if k.startswith('ref_') or not np.size(v):
            continue
        v = np.where(np.isnan(v), np.inf, v)
        i = int(np.argmax(v))
        if not v[i] <= 1.0:
            where = ' [%s]' % describe_row(k, i) if describe_row else ''
            raise AssertionError('%s: %s misses its bound at row %d%s: error / bound = %.3g (%d rows over)'
                                 % (what, k, i, where, v[i], int(np.sum(v > 1.0))))


def assert_saturated_derivatives_vanish(saved, d_gi, d_gh):
    """Where a saved gate is saturated IN fp32 (n = +-1, r or z = 0 or 1) the derivatives through it are exactly 0, and the
    case holds many such elements of each kind."""
    sv, d_gi, d_gh = np.asarray(saved), np.asarray(d_gi), np.asarray(d_gh)
    h = sv.shape[1] // 5
    r, z, n = sv[:, :h], sv[:, h:2 * h], sv[:, 2 * h:3 * h]
    sat_n, sat_r, sat_z = np.abs(n) == 1, (r == 0) | (r == 1), (z == 0) | (z == 1)
    assert min(int(sat_n.sum()), int(sat_r.sum()), int(sat_z.sum())) > 50, (sat_n.sum(), sat_r.sum(), sat_z.sum())
    assert np.all(d_gi[:, 2 * h:][sat_n] == 0) and np.all(d_gi[:, :h][sat_n] == 0) and np.all(d_gh[:, 2 * h:][sat_n] == 0)
    assert np.all(d_gi[:, :h][sat_r] == 0) and np.all(d_gh[:, :h][sat_r] == 0)
    assert np.all(d_gi[:, h:2 * h][sat_z] == 0) and np.all(d_gh[:, h:2 * h][sat_z] == 0)


# ---- host evaluations of the same steps (what the CPU test pushes through the bounds) ----------------------------------
def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32)


def split3(x):
    """split3 of gru_common.h: x = p0 + p1 + p2, round-to-nearest bf16 terms."""
    x = np.asarray(x, np.float32)
    p0 = bf16_rne(x)
    r1 = x - p0
    p1 = bf16_rne(r1)
    return p0, p1, bf16_rne(r1 - p1)


def matmul_planes(a, b, acc=None, npl=3, drop=None):
    """a [M, K] b[N, K]^T as the bf16-plane kernels form it: K in groups of 32, per group the six term pairs smallest
    first (npl = 1: the one bf16 product), every MFMA = one exact 32-term sum added to the fp32 accumulator with ONE
    rounding.  drop: a pair of PAIRS6 left out (what a missing mfma6 line computes)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    k = a.shape[1]
    kp = -(-k // 32) * 32
    ap = [np.pad(p, ((0, 0), (0, kp - k))).astype(np.float64) for p in split3(a)]
    bp = [np.pad(p, ((0, 0), (0, kp - k))).astype(np.float64) for p in split3(b)]
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32) if acc is None else np.asarray(acc, np.float32)
    pairs = [pq for pq in PAIRS6 if pq != drop] if npl == 3 else [(0, 0)]
    for k0 in range(0, kp, 32):
        for p, q in pairs:
            acc = (acc.astype(np.float64) + ap[p][:, k0:k0 + 32] @ bp[q][:, k0:k0 + 32].T).astype(np.float32)
    return acc


def product_planes(a, b, npl=3, drop=None):
    """ONE product a * b per element as the plane kernels form it (every other term of the MFMA sums is zero): the term pairs
    are exact in fp32 (8 x 8 significant bits), each addition rounds once."""
    ap, bp = split3(a), split3(b)
    acc = np.zeros(np.broadcast(ap[0], bp[0]).shape, np.float32)
    for p, q in ([pq for pq in PAIRS6 if pq != drop] if npl == 3 else [(0, 0)]):
        acc = acc + ap[p] * bp[q]
    return acc


PRODUCT_BOUND = {'bf16x6': 2.0 ** -22, 'f32': 2.0 ** -23, 'bf16': 2.0 ** -7}   # relative, of a single product


PRODUCT_BOUND_BWD = dict(PRODUCT_BOUND, bf16x6=2.0 ** -21)                     # observed through dGi_n of the step before


def product_ratio(got, a, b, route, bounds=PRODUCT_BOUND):
    ref = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    return ratio(np.abs(np.asarray(got, np.float64) - ref), bounds[route] * np.abs(ref))


def backward_product_case(h, seed=61):
    """Inputs of the backward entry (saved is an INPUT there) under which dh_prev is ONE product per element: two steps, all
    h + 3 sequences alive at both; dh_last one-hot at k0 = row mod H; at the last step r = 1 and z = 0 exactly, so dGh is
    one-hot at column 2H + k0 with the full-width value a = dh (1 - n^2) and the direct term z dh vanishes:
    dh_prev[v] = a W_hh[2H + k0][v].  At step 0, z = 0 and n = 0 make dGi_n = dh_prev (1 - z)(1 - n^2) = dh_prev exactly.
    -> dict of case() fields + 'saved', 'k0'."""
    rng = np.random.RandomState(seed)
    nb, f = h + 3, np.float32
    c = case(h, [2] * nb, seed=seed, wscale=1.0)
    k0 = np.arange(nb) % h
    sv = np.zeros((2 * nb, 5 * h), f)
    sv[:nb, :h] = rng.uniform(0.1, 0.9, (nb, h))                         # step 0: r, hn arbitrary; z = n = hp = 0
    sv[:nb, 3 * h:4 * h] = rng.randn(nb, h)
    sv[nb:, :h] = 1                                                      # step 1: r = 1, z = 0, n, hn, hp arbitrary
    sv[nb:, 2 * h:3 * h] = rng.uniform(-0.9, 0.9, (nb, h))
    sv[nb:, 3 * h:4 * h] = rng.randn(nb, h)
    sv[nb:, 4 * h:] = 0.3 * rng.randn(nb, h)
    dh = np.zeros((nb, h), f)
    dh[np.arange(nb), k0] = (1.5 * rng.randn(nb)).astype(f)
    c.update(saved=sv, dh=dh, k0=k0)
    return c


def backward_product_operands(c, d_gi, d_gh):
    """-> (got [nb, H], a [nb, 1], b [nb, H]) of backward_product_case from an implementation's outputs; asserts that its
    dGh of the last step is one-hot."""
    h, k0 = c['h'], c['k0']
    nb = len(k0)
    d_gi, d_gh = np.asarray(d_gi, np.float32), np.asarray(d_gh, np.float32)
    a = d_gh[nb + np.arange(nb), 2 * h + k0]
    rest = d_gh[nb:].copy()
    rest[np.arange(nb), 2 * h + k0] = 0
    assert np.all(rest == 0) and np.all(np.abs(a) > 1e-6), 'dGh of the last step is not one-hot'
    return d_gi[:nb, 2 * h:], a[:, None], c['w'][2 * h + k0, :]


def _matmul(route, a, b, acc=None):
    if route == 'f32':
        c = np.asarray(a, np.float32) @ np.asarray(b, np.float32).T
        return c if acc is None else acc + c
    return matmul_planes(a, b, acc, 3 if route == 'bf16x6' else 1)


def run_float32(route, gi, off, w_hh, b_hh, dh_last, out_rows=None):
    """The kernels' arithmetic in numpy float32 (route 'f32': plain float32 products; 'bf16x6' / 'bf16': matmul_planes)
    -> (h_last, saved, dGi, dGh), float32."""
    f = np.float32
    gi, w, b = np.asarray(gi, f), np.asarray(w_hh, f), np.asarray(b_hh, f)
    h, nb, nrow = w.shape[1], off[1] - off[0], off[-1]
    hcur = np.zeros((max(nb, out_rows or 0), h), f)
    saved = np.zeros((nrow, 5 * h), f)
    one = f(1)
    for j in range(len(off) - 1):
        bs = off[j + 1] - off[j]
        hp = hcur[:bs].copy()
        gh = _matmul(route, hp, w) + b
        g = gi[off[j]:off[j + 1]]
        with np.errstate(over='ignore'):
            r = one / (one + np.exp(-(g[:, :h] + gh[:, :h]), dtype=f))
            z = one / (one + np.exp(-(g[:, h:2 * h] + gh[:, h:2 * h]), dtype=f))
        n = np.tanh(g[:, 2 * h:] + r * gh[:, 2 * h:], dtype=f)
        saved[off[j]:off[j + 1]] = np.concatenate([r, z, n, gh[:, 2 * h:], hp], 1)
        hcur[:bs] = (one - z) * n + z * hp
    d_gi, d_gh = backward_float32(route, dh_last, off, w, saved)
    return hcur, saved, d_gi, d_gh


def backward_float32(route, dh_last, off, w_hh, saved):
    """The backward half of run_float32 from given saved values -> (dGi, dGh)."""
    f = np.float32
    w, saved = np.asarray(w_hh, f), np.asarray(saved, f)
    h, nb, nrow = w.shape[1], off[1] - off[0], off[-1]
    one = f(1)
    dh = np.array(np.asarray(dh_last)[:nb], f)
    d_gi, d_gh = np.zeros((nrow, 3 * h), f), np.zeros((nrow, 3 * h), f)
    wt = np.ascontiguousarray(w.T)                                      # [H, 3H]: dh_prev = dGh W_hh
    for j in range(len(off) - 2, -1, -1):
        p0, bs = off[j], off[j + 1] - off[j]
        r, z, n, hn, hp = _gates(saved[p0:p0 + bs], h)
        g = dh[:bs]
        dan = g * (one - z) * (one - n * n)
        daz = g * (hp - n) * z * (one - z)
        dar = dan * hn * r * (one - r)
        d_gi[p0:p0 + bs] = np.concatenate([dar, daz, dan], 1)
        d_gh[p0:p0 + bs] = np.concatenate([dar, daz, dan * r], 1)
        if j > 0:
            dh[:bs] = _matmul(route, d_gh[p0:p0 + bs], wt, acc=g * z)
    return d_gi, d_gh
