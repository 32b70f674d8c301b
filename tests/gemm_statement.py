"""Host statements of the split GEMM kernels (re-net_amd/csrc/gemm_split.hip, gemm_skinny.hip, gemm_planes.hip, gemm_h3.hip,
gemm.hip) -- TEST INFRASTRUCTURE, numpy only, importable without a GPU.  The six-pair bf16 arithmetic is the one of
tests/gru_statement.py (imported, not copied); the f16x3 arithmetic moved here from tests/test_f16x3_arithmetic_cpu.py.
tests/test_gemm_statement_cpu.py holds every condition the GPU tests rest on, on the very operands they use;
tests/test_gpu_gemm_products.py puts the kernels through the same operand builders and the same assertion helpers.

Three measures, none of them taken from a kernel:
  single products  every output is ONE product a * b (one-hot operand): |c - a b| <= PRODUCT_REL[family] |a b|.  A missing
                   low-order term pair of a split (2^-16 of the product) has nowhere to hide.
  units            |c - ref64| / (|a| @ |b| 2^-24): the error of a dense product in units of its own fp32 bound.
  integers         operands that every format holds exactly, partial sums below 2^24: the float64 product bit for bit."""
import numpy as np

from gru_statement import (PAIRS6, split3, product_planes, matmul_planes, product_ratio, PRODUCT_BOUND,   # noqa: F401
                           M_BF16, bf16_rne, ratio)

SMALL_PAIRS = PAIRS6[:3]                           # (2, 0), (1, 1), (0, 2): 2^-16 of the product each
H3_TERMS = ('a1b1', 'a1b2', 'a2b1')
H3_BOUND = 2.0 ** -21                              # header of gemm_h3.hip: every product accurate to 2^-21

# relative bound of a single product per kernel family
PRODUCT_REL = {'bf16x6': PRODUCT_BOUND['bf16x6'], 'planes': PRODUCT_BOUND['bf16x6'],   # six term pairs: 2^-22
               'f16x3': H3_BOUND,
               'f32': 2.0 ** -24,                  # one rounding of an exact product
               'bf16': M_BF16, 'bf16s': M_BF16}    # two operand roundings; the product of the rounded operands is exact in fp32

# dense products in units: (m, n, k); K stops at 200 -- at K = 4097 a dropped pair is 3 units and drowns in rounding
DENSE_SHAPES = [(130, 257, 33), (257, 130, 71), (130, 130, 200)]
UNITS_FACTOR = {f: 2.0 for f in PRODUCT_REL}       # kernel <= factor x host emulation (summation order inside an MFMA
                                                   # and across k-steps; profiles/gemm_products.md)


def seed_of(m, n, k):
    return m * 131 + n * 17 + k


# ---- the cases of tests/test_gpu_gemm_products.py: (m, n, k, ta, tb, split_k) ---------------------------------------------
# the smallest shapes with two full k-tiles and a tail, ragged row and column tiles, two 256-row tiles, a short last split
P1 = [(260, 130, 71, ta, tb, 1) for ta in (0, 1) for tb in (0, 1)]
P2 = [(260, 130, 200, 1, 0, 3), (260, 130, 200, 0, 1, 3)]                      # k ranges of 96, 96 and 8
S = [(300, n, k, 0, tb, 1) for n, k in ((130, 72), (250, 204)) for tb in (0, 1)]   # weight-resident kernel, K16 = 7 and 13
PP = (3000, 3000, 48, 0, 1, 1)                     # 576 tiles: more than a persistent planes grid has workgroups (512)
INT_LONG = (96, 100, 600, 1, 0, 7)
ROLES, SHIFTS = ('A', 'B'), (0, 1, 2, 3)
SIX_PAIR = ('bf16x6', 'planes')

# configuration -> (environment, families run in its child, kernel index renet_gemm_split_plan must report for bf16x6)
CONFIGS = {
    'default': ({}, ('bf16x6', 'f16x3', 'f32', 'bf16', 'planes'), 0),
    'two_phase_128': ({'RENET_GEMM_KERNEL': 'split', 'RENET_GEMM_TALL': '0', 'RENET_GEMM_SKINNY': '0'}, ('bf16x6',), 1),
    'two_phase_256': ({'RENET_GEMM_KERNEL': 'split', 'RENET_GEMM_TALL': '1', 'RENET_H3_TALL': '1', 'RENET_GEMM_SKINNY': '0'},
                      ('bf16x6', 'f16x3'), 2),
    'f32_generic': ({'RENET_GEMM_F32_GENERIC': '1'}, ('f32',), None),
    'bf16_storage': ({'RENET_GEMM': 'bf16s'}, ('bf16s',), None),
    'planes_256': ({'RENET_P6_TILE': '256'}, ('planes',), None),
    'planes_persistent': ({'RENET_P6_PERSISTENT': '1'}, ('planes',), None),
}
CONFIG_ENV_KEYS = sorted({k for env, _, _ in CONFIGS.values() for k in env} | {'RENET_GEMM_EPILOGUE'})


def one_hot_seed(m, n, k, role, shift):
    return seed_of(m, n, k) * 8 + shift * 2 + (role == 'B')


def single_cases(config, family):
    """-> [(m, n, k, ta, tb, split_k, role, shift)]"""
    shapes = P1 + P2 + (S if config == 'default' and family == 'bf16x6' else [])
    out = [s + (role, shift) for s in shapes for role in ROLES for shift in SHIFTS]
    return out + ([PP + ('A', 0)] if config == 'planes_persistent' else [])


def dense_cases(config, family):
    """-> [(m, n, k, ta, tb, split_k)]"""
    out = [(m, n, k, ta, tb, sk) for m, n, k in DENSE_SHAPES for sk in ((1, 3) if k == 200 else (1,))
           for ta in (0, 1) for tb in (0, 1)]
    return out + (S if config == 'default' and family == 'bf16x6' else [])


def int_cases(config, family):
    """-> [(m, n, k, ta, tb, split_k, epilogue)]; epilogue 1: alpha = 0.5, beta = 1, integer bias, row-padded output"""
    return [s + (epi,) for s in P1 + P2 + S + [INT_LONG] for epi in (0, 1)]


# ---- f16x3 (gemm_h3.hip) ------------------------------------------------------------------------------------------------
def scale_of(bound):
    """2^(15 - e) for bound = m 2^e, m in [0.5, 1)  (h3_scale_of)."""
    if not np.isfinite(bound) or bound <= 0:
        return 2.0 ** 126
    _, e = np.frexp(np.float32(bound))
    return float(2.0 ** min(max(15 - int(e), -126), 126))


def split(x, s):
    xs = (x.astype(np.float32) * np.float32(s)).astype(np.float32)
    h1 = xs.astype(np.float16)
    h2 = ((xs - h1.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return h1, h2


def _h3_scales(a, b, bound_a, bound_b):
    return (scale_of(np.abs(a).max() if bound_a is None else bound_a),
            scale_of(np.abs(b).max() if bound_b is None else bound_b))


def _h3_keep(drop):
    assert drop is None or drop in H3_TERMS, drop
    return [np.float32(t != drop) for t in H3_TERMS]


def f16x3_matmul(a, b, bound_a=None, bound_b=None, drop=None):
    """a [M, K] @ b [N, K]^T as the kernel computes it (fp32 accumulation by numpy's float32 matmul).  drop: one of H3_TERMS
    left out (what a missing MFMA line computes)."""
    sa, sb = _h3_scales(a, b, bound_a, bound_b)
    a1, a2 = split(a, sa)
    b1, b2 = split(b, sb)
    f = lambda h: h.astype(np.float32)                                        # noqa: E731
    k11, k12, k21 = _h3_keep(drop)
    main = (f(a1) @ f(b1).T) * k11
    corr = (f(a1) @ f(b2).T) * k12 + (f(a2) @ f(b1).T) * k21
    return ((main + corr * np.float32(2.0 ** -11)).astype(np.float64) / sa) / sb


def f16x3_product(a, b, drop=None, bound_a=None, bound_b=None):
    """ONE product a * b per element (broadcast) as the f16x3 kernels form it: the term products are exact in fp32 (11 x 11
    significant bits), corr = a2 b1 + a1 b2 rounds once, main + 2^-11 corr is one fma.  The scales come from bound_a /
    bound_b (default: the largest magnitude of the array): the kernels scale per TENSOR."""
    sa, sb = _h3_scales(a, b, bound_a, bound_b)
    a1, a2 = split(np.asarray(a, np.float32), sa)
    b1, b2 = split(np.asarray(b, np.float32), sb)
    f = lambda h: h.astype(np.float32)                                        # noqa: E731
    k11, k12, k21 = _h3_keep(drop)
    main = f(a1) * f(b1) * k11
    corr = f(a2) * f(b1) * k21 + f(a1) * f(b2) * k12
    out = (main.astype(np.float64) + corr.astype(np.float64) * 2.0 ** -11).astype(np.float32)
    return (out.astype(np.float64) / sa) / sb


def units(a, b, c):
    """|c - a b^T| / (|a| |b|^T 2^-24), a [M, K], b [N, K]: the error in units of the dot product's own fp32 bound."""
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    unit = (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64).T) * 2.0 ** -24
    return np.abs(c - ref) / unit


# ---- operands -----------------------------------------------------------------------------------------------------------
def _values(rng, shape, family):
    if family == 'f16x3':                          # per-TENSOR scale: small elements lose relative accuracy by design
        return (rng.uniform(1.0, 2.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    x = (1.5 * rng.standard_normal(shape)).astype(np.float32)
    while True:
        small = np.abs(x) < 1e-6
        if not small.any():
            return x
        x[small] = (1.5 * rng.standard_normal(int(small.sum()))).astype(np.float32)


def one_hot_case(role, m, n, k, shift, seed, family):
    """Operands of a single-product census -> (A [m, k], B [k, n], fa, fb, kidx): the logical matrices (the caller stores
    them transposed for ta / tb) and the factors with C = fa * fb elementwise (broadcast), C[i, j] taken at k = kidx.
    role 'A': A[i, (i + shift) % k] = a_i, zero elsewhere, B dense: C[i, j] = a_i B[(i + shift) % k, j].
    role 'B': B[(j + shift) % k, j] = b_j, zero elsewhere, A dense: C[i, j] = A[i, (j + shift) % k] b_j.
    shift = 0..3 puts the one-hot into each position of a float4 item.  Values: full-width 1.5 randn (none below 1e-6); for
    f16x3 magnitudes in [1, 2) with random signs."""
    rng = np.random.RandomState(seed)
    if role == 'A':
        kidx = (np.arange(m) + shift) % k
        hot, b = _values(rng, m, family), _values(rng, (k, n), family)
        a = np.zeros((m, k), np.float32)
        a[np.arange(m), kidx] = hot
        return a, b, hot[:, None], b[kidx, :], np.broadcast_to(kidx[:, None], (m, n))
    assert role == 'B', role
    kidx = (np.arange(n) + shift) % k
    hot, a = _values(rng, n, family), _values(rng, (m, k), family)
    b = np.zeros((k, n), np.float32)
    b[kidx, np.arange(n)] = hot
    return a, b, a[:, kidx], hot[None, :], np.broadcast_to(kidx[None, :], (m, n))


def dense_case(m, n, k, seed=None):
    """uniform(-1, 1) operands -> (A [m, k], B [k, n])."""
    rng = np.random.RandomState(seed_of(m, n, k) if seed is None else seed)
    return rng.uniform(-1, 1, (m, k)).astype(np.float32), rng.uniform(-1, 1, (k, n)).astype(np.float32)


def int_case(m, n, k, seed):
    """Integers in [-64, 64] -> (A [m, k], B [k, n], bias [n], C0 [m, n]), float32: one bf16 / f16 term each."""
    rng = np.random.RandomState(seed)
    f = np.float32
    return (rng.randint(-64, 65, (m, k)).astype(f), rng.randint(-64, 65, (k, n)).astype(f),
            rng.randint(-64, 65, n).astype(f), rng.randint(-64, 65, (m, n)).astype(f))


def int_statement(a, b, bias=None, c0=None, alpha=1.0, beta=0.0):
    out = alpha * (a.astype(np.float64) @ b.astype(np.float64))
    if bias is not None:
        out = out + bias.astype(np.float64)[None, :]
    return out if c0 is None else out + beta * c0.astype(np.float64)


# ---- host evaluations (the yardstick of the dense test, and the stand-in for a defective kernel) ---------------------------
def emulate(family, a, b, drop=None):
    """The dense product a [m, k] @ b [k, n] as the family's kernels form it -> float64 [m, n]."""
    bt = np.ascontiguousarray(b.T)
    if family in ('bf16x6', 'planes'):
        return matmul_planes(a, bt, drop=drop).astype(np.float64)
    if family == 'f16x3':
        return f16x3_matmul(a, bt, drop=drop)
    assert drop is None, drop
    if family == 'f32':
        return (a @ b).astype(np.float64)
    return matmul_planes(a, bt, npl=1).astype(np.float64)                      # bf16, bf16s


def units_operands(family, a, b):
    """-> (a [m, k], b^T [n, k]) that units() measures against: the two one-plane families against the product of their
    bf16-rounded operands (as tests/test_gpu_bf16.py does)."""
    bt = np.ascontiguousarray(b.T)
    return (bf16_rne(a), bf16_rne(bt)) if family in ('bf16', 'bf16s') else (a, bt)


def dense_units(family, a, b, c):
    """Worst units value of c against the dense product a @ b."""
    ar, btr = units_operands(family, a, b)
    return float(units(ar, btr, np.asarray(c, np.float64)).max())


def dropped_terms(family):
    return SMALL_PAIRS if family in ('bf16x6', 'planes') else H3_TERMS if family == 'f16x3' else ()


# ---- assertion helpers (GPU tests and the CPU teeth test call the same ones) ---------------------------------------------
def single_product_ratio(family, got, fa, fb):
    """error / bound of every single product -> array of got's shape."""
    ref = np.asarray(fa, np.float64) * np.asarray(fb, np.float64)
    return ratio(np.abs(np.asarray(got, np.float64) - ref), PRODUCT_REL[family] * np.abs(ref))


def assert_single_products(family, got, fa, fb, kidx, what):
    """Every output within the family's bound of the float64 product of its two factors -> the worst error / bound."""
    q = single_product_ratio(family, got, fa, fb)
    q = np.where(np.isnan(q), np.inf, q)
    i, j = np.unravel_index(int(np.argmax(q)), q.shape)
    if not q[i, j] <= 1.0:
        raise AssertionError('%s: single product at (row %d, column %d, k %d) misses the %s bound 2^%.2f: error / bound = %.3g '
                             '(%d of %d products over)' % (what, i, j, int(kidx[i, j]), family, np.log2(PRODUCT_REL[family]),
                                                           q[i, j], int(np.sum(q > 1.0)), q.size))
    return float(q[i, j])


def assert_units(family, a, b, got, emulated, what, factor=None):
    """units(got).max() <= factor x units(host emulation).max() on the same operands -> (kernel, emulation) worst values."""
    factor = UNITS_FACTOR[family] if factor is None else factor
    ar, btr = units_operands(family, a, b)
    u = units(ar, btr, np.asarray(got, np.float64))
    u = np.where(np.isnan(u), np.inf, u)
    emu = dense_units(family, a, b, emulated)
    i, j = np.unravel_index(int(np.argmax(u)), u.shape)
    if not u[i, j] <= factor * emu:
        raise AssertionError('%s: %.3g units at (row %d, column %d), the host emulation has %.3g: over %.3g x emulation '
                             '(%d of %d elements over)' % (what, u[i, j], i, j, emu, factor,
                                                           int(np.sum(u > factor * emu)), u.size))
    return float(u[i, j]), emu


def assert_exact(got, ref64, what):
    got = np.asarray(got)
    bad = got.astype(np.float64) != ref64
    if got.shape != ref64.shape or bad.any():
        i, j = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError('%s: %d of %d integer results differ from the float64 statement, first at (row %d, column %d): '
                             '%r vs %r' % (what, int(bad.sum()), bad.size, i, j, float(got[i, j]), float(ref64[i, j])))
