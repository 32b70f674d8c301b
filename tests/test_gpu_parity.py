"""GPU parity tests (run with -m gpu on an MI355X): the HIP path through the C ABI against
  (a) the golden fixtures produced by the unmodified reference (tests/golden/, tools/make_golden.py),
  (b) the oracle restatement (oracle/renet_oracle.py) on fresh seeded inputs,
  (c) size-independent properties at BASELINE.json's full sizes.
Tolerances are fp32: the kernels sum in a different order than torch-CPU / the reference.
"""
import os

import numpy as np
import pytest
import torch

from helpers import O, fixtures, load_golden, train_case, global_shapes, renet_shapes

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 2e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _to(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,k', [(1, 1, 1), (7, 5, 3), (128, 128, 32), (200, 200, 200), (257, 130, 71),
                                   (1024, 777, 600), (64, 600, 200), (333, 200, 4)])
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('mode', ['f32', 'bf16x6', 'f16x3'])
def test_gemm_matches_fp64(dev, m, n, k, ta, tb, mode):
    import renet_hip as K
    rng = np.random.RandomState(m * 131 + n * 17 + k + ta * 2 + tb)
    a = rng.uniform(-1, 1, (k, m) if ta else (m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, (n, k) if tb else (k, n)).astype(np.float32)       # asymmetric operands
    bias = rng.uniform(-1, 1, n).astype(np.float32)
    ref = (a.T if ta else a).astype(np.float64) @ (b.T if tb else b).astype(np.float64) + bias
    out = K.gemm(_to(a, dev), _to(b, dev), ta=bool(ta), tb=bool(tb), bias=_to(bias, dev), mode=mode)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * max(1, k) ** 0.5)


_GEMM_KERNEL_CHECK = r'''
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import renet_hip as K
dev = torch.device('cuda:0')
rng = np.random.RandomState(11)
# (m, n, k, ta, tb, split_k): ragged edges in every dimension, K < one tile, one k-tile, two, many; split-K
for m, n, k, ta, tb, sk in [(1, 1, 4, 0, 1, 1), (130, 257, 31, 0, 1, 1), (130, 257, 33, 0, 0, 1), (300, 129, 64, 1, 0, 1),
                            (257, 130, 71, 1, 1, 1), (64, 600, 200, 0, 1, 1), (1024, 777, 600, 0, 0, 1),
                            (96, 100, 5000, 1, 0, 7), (2500, 2300, 96, 0, 1, 1), (200, 200, 4097, 1, 0, 3)]:
    a = rng.uniform(-1, 1, (k, m) if ta else (m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, (n, k) if tb else (k, n)).astype(np.float32)
    ref = (a.T if ta else a).astype(np.float64) @ (b.T if tb else b).astype(np.float64)
    out = K.gemm(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), ta=bool(ta), tb=bool(tb), split_k=sk,
                 mode='bf16x6')
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * max(1, k) ** 0.5)
print('ok')
'''


@pytest.mark.parametrize('kernel', ['fused', 'split', 'tall'])
def test_gemm_both_k_loop_structures(dev, kernel):
    """The bf16x6 GEMM has two k-loop structures (gemm_split.hip) picked by grid size, the two-phase one with a
    128 x 128 or a 256 x 128 ('tall') tile; force each one over shapes on both sides of the thresholds."""
    import subprocess
    import sys
    env = dict(os.environ, RENET_GEMM_KERNEL='split' if kernel == 'tall' else kernel,
               RENET_GEMM_TALL='1' if kernel == 'tall' else '0')
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 're-net_amd')
    r = subprocess.run([sys.executable, '-c', _GEMM_KERNEL_CHECK, pkg], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


@pytest.mark.parametrize('generic', ['0', '1'])
def test_exact_f32_gemm_every_tile_and_edge(dev, generic):
    """renet_gemm_f32 (exact fp32 products on v_mfma_f32_32x32x2_f32): the buffer-addressed production kernel
    (round 4) and, forced with RENET_GEMM_F32_GENERIC=1, the generic fallback for operands it cannot address -- over
    ragged shapes, K below one k-tile, one, two, many k-tiles, split-K (child process: the switch is read once)."""
    import subprocess
    import sys
    env = dict(os.environ, RENET_GEMM_F32_GENERIC=generic)
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 're-net_amd')
    r = subprocess.run([sys.executable, '-c', _GEMM_KERNEL_CHECK.replace("mode='bf16x6'", "mode='f32'"), pkg],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_exact_f32_gemm_products_are_exact_and_views_are_respected(dev):
    """(a) Operands whose products and partial sums are all exactly representable in fp32 (small integers) must come
    out EXACT -- no operand rounding anywhere in the exact-fp32 kernel, unlike the split modes' 22 / 24-bit operands
    (checked with 24-bit odd integers scaled so that every partial sum stays below 2^24).  (b) Row-strided views with
    odd leading dimensions, garbage (NaN) outside the logical extent of every operand: nothing outside may leak in."""
    import renet_hip as K
    rng = np.random.RandomState(5)
    for m, n, k, ta, tb in [(130, 257, 100, 0, 1), (257, 130, 71, 1, 0), (64, 96, 33, 0, 0), (96, 64, 600, 1, 1)]:
        a = rng.randint(-64, 65, (k, m) if ta else (m, k)).astype(np.float32)
        b = rng.randint(-64, 65, (n, k) if tb else (k, n)).astype(np.float32)
        ref = (a.T if ta else a).astype(np.float64) @ (b.T if tb else b).astype(np.float64)
        out = K.gemm(_to(a, dev), _to(b, dev), ta=bool(ta), tb=bool(tb), mode='f32').cpu().numpy()
        assert np.array_equal(out.astype(np.float64), ref), (m, n, k, ta, tb)
        # full-width significands: x = odd 24-bit integer * 2^-23, one product per output (K = 1) must be the fp32
        # rounding of the exact product
        a1 = ((rng.randint(2 ** 22, 2 ** 23, (m, 1)) * 2 + 1) * 2.0 ** -23).astype(np.float32)
        b1 = ((rng.randint(2 ** 22, 2 ** 23, (1, n)) * 2 + 1) * 2.0 ** -23).astype(np.float32)
        o1 = K.gemm(_to(a1, dev), _to(b1, dev), mode='f32').cpu().numpy()
        assert np.array_equal(o1, (a1.astype(np.float64) @ b1.astype(np.float64)).astype(np.float32))
    # (b) views inside NaN-filled buffers
    for m, n, k, ta, tb, lda, ldb in [(130, 70, 45, 0, 1, 51, 47), (70, 130, 45, 1, 0, 73, 133), (33, 35, 37, 0, 0, 41, 39),
                                      (129, 131, 64, 1, 1, 131, 67)]:
        ra, ca = (k, m) if ta else (m, k)
        rb, cb = (n, k) if tb else (k, n)
        A = torch.full((ra + 2, lda), float('nan'), device=dev)
        B = torch.full((rb + 2, ldb), float('nan'), device=dev)
        a = rng.uniform(-1, 1, (ra, ca)).astype(np.float32)
        b = rng.uniform(-1, 1, (rb, cb)).astype(np.float32)
        A[1:1 + ra, :ca] = _to(a, dev)
        B[1:1 + rb, :cb] = _to(b, dev)
        C = torch.full((m + 2, n + 5), float('nan'), device=dev)
        K.gemm(A[1:1 + ra, :ca], B[1:1 + rb, :cb], ta=bool(ta), tb=bool(tb), out=C[1:1 + m, :n], mode='f32')
        ref = (a.T if ta else a).astype(np.float64) @ (b.T if tb else b).astype(np.float64)
        got = C.cpu().numpy()
        np.testing.assert_allclose(got[1:1 + m, :n], ref, rtol=1e-5, atol=1e-5 * k ** 0.5)
        assert np.isnan(got[0]).all() and np.isnan(got[-1]).all() and np.isnan(got[:, n:]).all()


@pytest.mark.parametrize('tall', ['0', '1'])
def test_f16x3_gemm_every_tile_and_edge(dev, tall):
    """renet_gemm_f32_h3 with the 128-row and the 256-row tile forced (RENET_H3_TALL) over ragged shapes, one k-tile,
    many, split-K (child process: the switch is read once per process)."""
    import subprocess
    import sys
    env = dict(os.environ, RENET_H3_TALL='1' if tall == '1' else '0', RENET_GEMM_SKINNY='0')
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 're-net_amd')
    r = subprocess.run([sys.executable, '-c', _GEMM_KERNEL_CHECK.replace("mode='bf16x6'", "mode='f16x3'"), pkg],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


@pytest.mark.parametrize('scale_a,scale_b', [(1.0, 1.0), (3e-9, 7e4), (5e7, 2e-6), (1e-20, 1e-12), (1e15, 1e10)])
def test_f16x3_gemm_is_fp32_class_at_any_tensor_magnitude(dev, scale_a, scale_b):
    """The f16x3 split scales each operand TENSOR by a power of two: its error against fp64, relative to the result's
    magnitude, must not depend on the operands' magnitudes and must stay in the class of the exact-fp32 kernel
    (v_mfma_f32_32x32x2_f32, fp32 products and accumulation).  Rows / columns spanning 2^20 in magnitude included."""
    import renet_hip as K
    rng = np.random.RandomState(9)
    m, n, k = 700, 520, 1500
    a = rng.standard_normal((m, k)) * np.exp2(rng.uniform(-20, 0, (m, 1)))        # per-row dynamic range
    b = rng.standard_normal((n, k)) * np.exp2(rng.uniform(-20, 0, (1, k)))        # per-k dynamic range
    a, b = (a * scale_a).astype(np.float32), (b * scale_b).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    # per-element error in units of the fp32-rounding bound of that dot product: sum_k |a_ik b_jk| 2^-24
    unit = (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64).T) * 2.0 ** -24
    errs = {}
    for mode in ('f32', 'bf16x6', 'f16x3'):
        out = K.gemm(_to(a, dev), _to(b, dev), tb=True, mode=mode).cpu().numpy().astype(np.float64)
        assert np.isfinite(out).all(), mode
        errs[mode] = float((np.abs(out - ref) / unit).max())
    assert errs['f16x3'] <= 4.0, errs                       # a handful of fp32 roundings of the largest term
    assert errs['f16x3'] <= 3.0 * max(errs['f32'], errs['bf16x6'], 0.5), errs


def test_f16x3_gemm_on_sparse_magnitude_operands(dev):
    """Review r3 (weak 1e): the f16x3 split's element accuracy is per TENSOR (an ABSOLUTE 2^-39 max|x| below 2^-29 max|x|),
    so the operands to worry about are the ones whose magnitudes are sparse: a late-training CE gradient (softmax -
    onehot: one entry of O(1/B) per row among thousands of 1e-9..1e-6) and a mostly-zero embedding gradient.  For
    both, every output's error against fp64 -- in units of that dot product's OWN fp32 rounding bound sum_k |a b| 2^-24 plus
    the absolute floor the header states (k 2^-39 max|a| max|b|) -- must stay within 3x of what the 24-bit split and the
    exact-fp32 kernel give on the same operands."""
    import renet_hip as K
    rng = np.random.RandomState(21)
    b_, c_, d_ = 512, 6000, 600
    # dlogits of a confident model: probabilities ~1e-9..1e-5 except a handful per row, minus the one-hot, over B
    logit = rng.standard_normal((b_, c_)) * 4.0
    logit[np.arange(b_), rng.randint(0, c_, b_)] += 25.0
    p_ = np.exp(logit - logit.max(1, keepdims=True))
    p_ /= p_.sum(1, keepdims=True)
    tgt = rng.randint(0, c_, b_)
    dl = p_.copy()
    dl[np.arange(b_), tgt] -= 1.0
    dl = (dl / b_).astype(np.float32)
    w = (rng.standard_normal((c_, d_)) * 0.05).astype(np.float32)
    feat = rng.standard_normal((b_, d_)).astype(np.float32)
    feat[rng.uniform(size=feat.shape) < 0.5] = 0.0                      # dropout zeros
    # a mostly-zero gradient matrix (rows of entities the batch never touched) times a dense weight
    sparse = np.zeros((4000, 200), dtype=np.float32)
    rows = rng.choice(4000, 60, replace=False)
    sparse[rows] = (rng.standard_normal((60, 200)) * np.exp2(rng.uniform(-30, 0, (60, 1)))).astype(np.float32)
    wl = (rng.standard_normal((200, 200)) * 0.1).astype(np.float32)
    cases = [('dfeat = dlogits W', dl, w, False, False), ('dW = dlogits^T feat', dl, feat, True, False),
             ('sparse rows x W', sparse, wl, False, False)]
    for name, a, b, ta, tb in cases:
        a64 = (a.T if ta else a).astype(np.float64)
        b64 = (b.T if tb else b).astype(np.float64)
        ref = a64 @ b64
        bound = (np.abs(a64) @ np.abs(b64)) * 2.0 ** -24 + a64.shape[1] * 2.0 ** -39 * np.abs(a).max() * np.abs(b).max()
        errs = {}
        for mode in ('f32', 'bf16x6', 'f16x3'):
            out = K.gemm(_to(a, dev), _to(b, dev), ta=ta, tb=tb, mode=mode, split_k=1).cpu().numpy().astype(np.float64)
            errs[mode] = float((np.abs(out - ref) / np.maximum(bound, 1e-300)).max())
        print('%-22s worst error in units of the dot product\'s fp32 bound: %s' % (name, {k: round(v, 2) for k, v in
                                                                                      errs.items()}))
        # (fp32 ACCUMULATION over K = 6000 / 512 terms alone puts the exact-fp32 kernel at tens of these units: observed on
        # MI355X f32 47.8 / bf16x6 31.7 / f16x3 27.0 for dfeat -- the split modes are not the limiting error here)
        assert errs['f16x3'] <= 3.0 * max(errs['f32'], errs['bf16x6'], 1.0), (name, errs)
        assert errs['f16x3'] <= 0.25 * a64.shape[1], (name, errs)


def test_f16x3_gemm_bounds_and_special_values(dev):
    """Operand handles: a bound larger than the true maximum (by 2^10) only costs binades; zero operands; NaN flows
    through; a registered weight's maxima are cached and refreshed when the weight changes."""
    import renet_hip as K
    rng = np.random.RandomState(3)
    a = rng.uniform(-1, 1, (300, 96)).astype(np.float32)
    b = rng.uniform(-1, 1, (96, 200)).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    ta_, tb_ = _to(a, dev), _to(b, dev)
    loose = K.F32Op(ta_, torch.full((1,), 1024.0, device=dev), 1)
    out = K.gemm(loose, tb_, mode='f16x3')
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * 96 ** 0.5)
    z = K.gemm(torch.zeros_like(ta_), tb_, mode='f16x3')
    assert float(z.abs().max()) == 0.0
    an = ta_.clone()
    an[5, 7] = float('nan')
    o = K.gemm(an, tb_, mode='f16x3')
    assert bool(torch.isnan(o[5]).all()) and not bool(torch.isnan(o[6]).any())
    w = tb_.clone()
    plain = K.gemm(ta_, w, mode='f16x3')
    K.register_weights([w])
    try:
        o1 = K.gemm(ta_, w, mode='f16x3')                    # bound from the weight cache
        assert torch.equal(o1, plain)
        ob = K.gemm(ta_, w[:, :130], mode='f16x3')           # a leading column block of the cached copy
        np.testing.assert_allclose(ob.cpu().numpy(), ref[:, :130], rtol=1e-5, atol=1e-5 * 96 ** 0.5)
        ot = K.gemm(_to(rng.uniform(-1, 1, (64, 200)).astype(np.float32), dev), w, tb=True, mode='f16x3')
        assert ot.shape == (64, 96) and bool(torch.isfinite(ot).all())
        w.mul_(4096.0)                                       # in-place torch write: version stamp changes
        o2 = K.gemm(ta_, w, mode='f16x3')
        np.testing.assert_allclose(o2.cpu().numpy(), 4096.0 * ref, rtol=1e-5, atol=4096 * 1e-5 * 96 ** 0.5)
        np.testing.assert_allclose(o1.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * 96 ** 0.5)
    finally:
        K.unregister_weights([w])


@pytest.mark.parametrize('m,n,k', [(23033, 200, 200), (14001, 200, 200), (257, 256, 208), (300, 64, 16), (4097, 100, 100),
                                   (1000, 200, 112), (999, 250, 204), (2048, 256, 128)])
@pytest.mark.parametrize('tb', [0, 1])
def test_skinny_weight_resident_gemm_matches_fp64_and_the_general_kernel(dev, m, n, k, tb):
    """gemm_skinny.hip (tall activation x small weight: K <= 208, N <= 256, the RGCN self-loop shapes) -- picked by
    renet_gemm_f32_split for eligible shapes -- against fp64 with bias, alpha and beta accumulation, row-strided
    operand views, and against the general kernel (RENET_GEMM_SKINNY=0 in a child process computes the same
    product; the two agree to fp32-class accuracy, not bit for bit: different summation order)."""
    import renet_hip as K
    rng = np.random.RandomState(m + 7 * n + 13 * k + tb)
    a_full = rng.uniform(-1, 1, (m, k + 8)).astype(np.float32)
    a = a_full[:, 4:4 + k]                                        # view: lda = k + 8, base 16-byte aligned
    b = rng.uniform(-1, 1, (n, k) if tb else (k, n)).astype(np.float32)
    bias = rng.uniform(-1, 1, n).astype(np.float32)
    c0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    prod = a.astype(np.float64) @ (b.T if tb else b).astype(np.float64)
    a_dev = _to(a_full, dev)[:, 4:4 + k]
    out = K.gemm(a_dev, _to(b, dev), tb=bool(tb), bias=_to(bias, dev))
    np.testing.assert_allclose(out.cpu().numpy(), prod + bias, rtol=1e-5, atol=1e-5 * k ** 0.5)
    acc = _to(c0, dev).clone()
    K.gemm(a_dev, _to(b, dev), tb=bool(tb), out=acc, alpha=0.5, beta=1.0)
    np.testing.assert_allclose(acc.cpu().numpy(), 0.5 * prod + c0, rtol=1e-5, atol=1e-5 * k ** 0.5)
    wide = torch.zeros(m, n + 40, device=dev)
    K.gemm(a_dev, _to(b, dev), tb=bool(tb), out=wide[:, 8:8 + n])            # ldc > N: neighbours untouched
    np.testing.assert_allclose(wide[:, 8:8 + n].cpu().numpy(), prod, rtol=1e-5, atol=1e-5 * k ** 0.5)
    assert float(wide[:, :8].abs().max()) == 0.0 and float(wide[:, 8 + n:].abs().max()) == 0.0
    again = K.gemm(a_dev, _to(b, dev), tb=bool(tb), bias=_to(bias, dev))
    assert torch.equal(out, again), 'deterministic'


def test_gemm_splitk_beta_and_strided_views(dev):
    import renet_hip as K
    rng = np.random.RandomState(5)
    a = rng.uniform(-1, 1, (5000, 96)).astype(np.float32)       # A^T stored: [K=5000, M=96]
    big = rng.uniform(-1, 1, (5000, 500)).astype(np.float32)
    b_view = _to(big, dev)[:, 400:]                             # strided [K, N=100], ld = 500
    c0 = rng.uniform(-1, 1, (96, 100)).astype(np.float32)
    ref = 0.5 * a.T.astype(np.float64) @ big[:, 400:].astype(np.float64) + 2.0 * c0
    for sk in (1, 4, 37):
        for mode in ('f32', 'bf16x6', 'f16x3'):
            out = _to(c0, dev).clone()
            K.gemm(_to(a, dev), b_view, ta=True, out=out, alpha=0.5, beta=2.0, split_k=sk, mode=mode)
            np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=2e-4)
    one = K.gemm(_to(a, dev), b_view, ta=True, split_k=8)
    two = K.gemm(_to(a, dev), b_view, ta=True, split_k=8)
    assert torch.equal(one, two), 'split-K must be deterministic'
    cs = K.colsum(_to(big, dev)[:, 100:333])
    np.testing.assert_allclose(cs.cpu().numpy(), big[:, 100:333].astype(np.float64).sum(0), rtol=1e-5, atol=1e-3)
    K.colsum(_to(big, dev)[:, 100:333], out=cs, beta=1.0)                   # accumulate into an existing buffer
    np.testing.assert_allclose(cs.cpu().numpy(), 2 * big[:, 100:333].astype(np.float64).sum(0), rtol=1e-5, atol=2e-3)
    x = _to(big, dev).clone()
    for f in (1.0, 0.1):
        K.scale_by_device_scalar(x, torch.tensor(f, device=dev))
    np.testing.assert_allclose(x.cpu().numpy(), big * np.float32(0.1), rtol=1e-6)
    odd = _to(big.reshape(-1)[:1003].copy(), dev)                           # n % 4 != 0
    K.scale_by_device_scalar(odd, torch.tensor(3.0, device=dev))
    np.testing.assert_allclose(odd.cpu().numpy(), big.reshape(-1)[:1003] * np.float32(3.0), rtol=1e-6)


# ---------------------------------------------------------------------------------------------
# RGCN layer vs the reference's RGCNBlockLayer (golden)
# ---------------------------------------------------------------------------------------------
def _graph_from_fixture(gold, dev):
    import graph as G
    hb = G.HostBatch.from_edges(int(gold['n']), gold['src'], gold['dst'], gold['type_s'], int(gold['num_rels']))
    np.testing.assert_array_equal(hb.norm, gold['norm'])
    return G.DeviceGraph(hb, dev)


@pytest.mark.parametrize('d', [100, 200, 400])
def test_rgcn_layer_matches_reference_golden(dev, d):
    import ops
    gold = load_golden('rgcn_%d.npz' % d)
    n, num_rels = int(gold['n']), int(gold['num_rels'])
    p = fixtures.make_params(200 + d, {'weight': (2 * num_rels, d * d // 100), 'loop_weight': (d, d),
                                       'h': (n, d), 'gout': (n, d)}, scale=0.5)
    g = _graph_from_fixture(gold, dev)
    for relu in (0, 1):
        for reverse in (0, 1):
            h = _to(p['h'], dev).requires_grad_(True)
            w = _to(p['weight'], dev).requires_grad_(True)
            lw = _to(p['loop_weight'], dev).requires_grad_(True)
            y = ops.RGCNLayerFn.apply(h, w, lw, g, bool(reverse), bool(relu), 0.0, 0, None)
            (y * _to(p['gout'], dev)).sum().backward()
            tag = 'relu%d_rev%d_' % (relu, reverse)
            np.testing.assert_allclose(y.detach().cpu().numpy(), gold[tag + 'out'], rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(h.grad.cpu().numpy(), gold[tag + 'dh'], rtol=RTOL, atol=ATOL)
            for key, gr in (('dweight', w.grad), ('dloop', lw.grad)):
                ok, err, how = fixtures.check_packed(gold, tag + key, gr.cpu().numpy(), RTOL, ATOL * 10)
                assert ok, (tag + key, err, how)


# ---------------------------------------------------------------------------------------------
# full training step of both directions vs the reference (golden) and vs the oracle
# ---------------------------------------------------------------------------------------------
def _build_model(c, dev, dropout=0.0):
    import model as M
    import utils as U
    cfg = c['cfg']
    net = M.RENet(cfg['num_ent'], c['d'], cfg['num_rels'], dropout=dropout, seq_len=c['seq_len'])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in c['params'].items()})
    net.global_emb = {t: torch.from_numpy(v).view(1, 1, -1) for t, v in c['global_emb'].items()}
    net.to(dev)
    gd = U.build_graph_dict(c['train'], cfg['num_rels'])
    return net, gd


@pytest.mark.parametrize('name,d', [('tiny', 100), ('tiny', 200), ('small', 200)])
def test_training_step_matches_reference_golden(dev, name, d):
    c = train_case(name, d)
    gold, cfg = c['gold'], c['cfg']
    net, gd = _build_model(c, dev)
    net.eval()
    batch = torch.from_numpy(c['batch']).to(dev)
    total = 0
    for tag, subject in (('s', True), ('o', False)):
        loss = net(batch, c['hists']['s'], c['hists']['o'], gd, subject=subject)
        ref = float(gold['loss_' + tag])
        assert abs(loss.item() - ref) < 2e-4 * max(1.0, abs(ref)), (tag, loss.item(), ref)
        total = total + loss
    total.backward()
    for k, p in net.named_parameters():
        g = p.grad.cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
        ok, err, how = fixtures.check_packed(gold, 'grad.' + k, g, 2e-3, 3e-5)
        assert ok, (k, err, how)


@pytest.mark.parametrize('name,d', [('tiny', 200), ('small', 200)])
def test_encoder_internals_match_reference_golden(dev, name, d):
    """h2 subject rows, GRU h_n and entity logits, re-keyed by original batch position."""
    import ops
    c = train_case(name, d)
    gold, cfg = c['gold'], c['cfg']
    net, gd = _build_model(c, dev)
    net.eval()
    b = len(c['batch'])
    with torch.no_grad():
        for tag, subject in (('s', True), ('o', False)):
            s, r, o, rel, reverse = net._direction(c['batch'], subject)
            px, pxr = net.aggregator(c['hists'][tag], s, r, net.ent_embeds, rel, gd, net.global_emb, reverse=reverse)
            g = net.aggregator.last_batch
            hb = g.host
            _, hn = net.encoder(px, total_rows=b)
            _, qn = net.encoder_r(pxr, total_rows=b)
            for key, val in (('h_n', hn[0]), ('q_n', qn[0])):
                full = np.zeros((b, d), np.float32)
                full[hb.perm] = val.cpu().numpy()
                np.testing.assert_allclose(full, gold['%s_%s' % (tag, key)], rtol=RTOL, atol=ATOL)
            # first D columns of the packed X rows are the gathered h2 rows (dropout off)
            rows_packed = px.data[:, :d].cpu().numpy()
            k_of_p = hb.packed_from_seqmajor
            rows_k = np.empty_like(rows_packed)
            rows_k[k_of_p] = rows_packed
            per_seq = np.split(rows_k, np.cumsum(hb.lens)[:-1]) if hb.nnz else []
            byorig = {int(hb.perm[i]): per_seq[i] for i in range(hb.nnz)}
            mine = np.concatenate([byorig[i] for i in sorted(byorig)])
            np.testing.assert_allclose(mine, gold[tag + '_subj_rows'], rtol=RTOL, atol=ATOL)
            assert hb.N == int(gold[tag + '_graph_nodes'])


def test_training_step_matches_oracle_on_fresh_inputs(dev):
    """Not a fixture: a new seeded stream, bigger batch, oracle computed here on CPU."""
    import model as M
    import utils as U
    rng_seed, num_ent, num_rels, d, L, B = 77, 300, 9, 200, 10, 256
    q = fixtures.tiny_stream(rng_seed, num_ent, num_rels, 40, 80, time_unit=24)
    (sh, sht), (oh, oht), _ = O.build_histories(q, num_ent)
    idx = np.sort(np.random.RandomState(1).choice(len(q), B, replace=False))
    hs = ([sh[i] for i in idx], [sht[i] for i in idx])
    ho = ([oh[i] for i in idx], [oht[i] for i in idx])
    params = fixtures.make_params(99, renet_shapes(num_ent, num_rels, d))
    times = np.unique(q[:, 3])
    gl = fixtures.make_params(98, {'g': (len(times), d)}, scale=0.3)['g']
    ge = {int(t): torch.from_numpy(gl[k]) for k, t in enumerate(times)}
    # oracle
    op = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in params.items()}
    ogd = O.build_graph_dict(q, num_rels)
    lo = O.renet_forward_loss(op, q[idx], hs[0], hs[1], ogd, ge, num_rels, L, subject=True) + \
        O.renet_forward_loss(op, q[idx], ho[0], ho[1], ogd, ge, num_rels, L, subject=False)
    lo.backward()
    # HIP
    net = M.RENet(num_ent, d, num_rels, dropout=0.0, seq_len=L)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net.global_emb = {t: v.view(1, 1, -1) for t, v in ge.items()}
    net.to(dev)
    gd = U.build_graph_dict(q, num_rels)
    batch = torch.from_numpy(q[idx]).to(dev)
    lh = net(batch, hs, ho, gd, subject=True) + net(batch, hs, ho, gd, subject=False)
    lh.backward()
    assert abs(lh.item() - lo.item()) < 2e-4 * abs(lo.item())
    for k, p in net.named_parameters():
        ref = op[k].grad.numpy() if op[k].grad is not None else np.zeros(tuple(p.shape), np.float32)
        scale = max(1e-6, float(np.abs(ref).max()))
        err = float(np.abs(p.grad.cpu().numpy() - ref).max())
        assert err < 2e-3 * scale + 2e-6, (k, err, scale)


# ---------------------------------------------------------------------------------------------
# GRU vs torch.nn.GRU on CPU (the third-party op being replaced)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernels', ['persistent', 'steps'])
@pytest.mark.parametrize('i,h,nseq', [(800, 200, 31), (300, 100, 31), (400, 400, 31), (200, 200, 77), (100, 400, 45),
                                      (64, 200, 150)])
def test_gru_matches_torch_cpu(dev, i, h, nseq, kernels, monkeypatch):
    """both bf16x6 recurrences: the one-launch persistent kernels and the per-step launches (RENET_GRU)"""
    import model as M
    monkeypatch.setenv('RENET_GRU', kernels)
    torch.manual_seed(7)
    lens = [10] * (nseq - 11) + [9, 9, 7, 5, 5, 5, 3, 2, 1, 1, 1]
    b, l = len(lens), 10
    ref = torch.nn.GRU(i, h, batch_first=True)
    x = torch.randn(b, l, i)
    for k, n in enumerate(lens):
        x[k, n:] = 0
    x.requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True)
    _, hn = ref(packed)
    gout = torch.randn(b, h)
    (hn[0] * gout).sum().backward()
    mine = M.GRU(i, h).to(dev)
    mine.load_state_dict(ref.state_dict())
    xd = packed.data.detach().to(dev).requires_grad_(True)
    pk = torch.nn.utils.rnn.PackedSequence(xd, packed.batch_sizes)
    _, hm = mine(pk, total_rows=b + 3)
    assert hm.shape == (1, b + 3, h) and float(hm[0, b:].abs().max()) == 0.0
    (hm[0, :b] * gout.to(dev)).sum().backward()
    np.testing.assert_allclose(hm[0, :b].detach().cpu().numpy(), hn[0].detach().numpy(), rtol=1e-4, atol=1e-5)
    dx_ref = torch.nn.utils.rnn.pack_padded_sequence(x.grad, lens, batch_first=True).data
    np.testing.assert_allclose(xd.grad.cpu().numpy(), dx_ref.numpy(), rtol=1e-3, atol=2e-5)
    for name, p in mine.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), getattr(ref, name).grad.numpy(), rtol=1e-3, atol=1e-4)


def _gru_float64(gi, off, w_hh, b_hh, dh_last):
    """The recurrence over packed rows in float64 -> (h_last [B, H], saved [S, 5H], dGi, dGh)."""
    h_dim, nstep = w_hh.shape[1], len(off) - 1
    gi = gi.double().requires_grad_(True)
    h = torch.zeros(off[1] - off[0], h_dim, dtype=torch.float64, requires_grad=True)     # (so that every gh has a grad)
    ghs, saved = [], []
    for j in range(nstep):
        bs = off[j + 1] - off[j]
        hp = h[:bs]
        gh = hp @ w_hh.double().t() + b_hh.double()
        gh.retain_grad()
        g = gi[off[j]:off[j + 1]]
        r = torch.sigmoid(g[:, :h_dim] + gh[:, :h_dim])
        z = torch.sigmoid(g[:, h_dim:2 * h_dim] + gh[:, h_dim:2 * h_dim])
        n = torch.tanh(g[:, 2 * h_dim:] + r * gh[:, 2 * h_dim:])
        saved.append(torch.cat([r, z, n, gh[:, 2 * h_dim:], hp], 1).detach())
        h = torch.cat([(1 - z) * n + z * hp, h[bs:]])
        ghs.append(gh)
    (h * dh_last.double()).sum().backward()
    return h.detach(), torch.cat(saved), gi.grad, torch.cat([g.grad for g in ghs])


_GRU_LAYOUT_CASE = []


def _gru_layout_case():
    """Four problems (W0, A), (W1, A), (W0, B), (W1, B) over two packed layouts, and their float64 results (built once)."""
    if not _GRU_LAYOUT_CASE:
        import ctypes
        torch.manual_seed(11)
        h_dim = 100
        ws = [(torch.randn(3 * h_dim, h_dim) * 0.05, torch.randn(3 * h_dim)) for _ in range(2)]
        lays = []
        for lens, nstep in (([5] * 20 + [4] * 6 + [3] * 5 + [2] * 3 + [1] * 3, 5), ([3] * 9 + [2] * 6 + [1] * 5, 3)):
            off = [0]
            for j in range(nstep):
                off.append(off[-1] + sum(1 for n in lens if n > j))
            lays.append((off, (ctypes.c_int32 * len(off))(*off), len(lens)))
        probs = []
        for off, off_c, b in lays:
            for w_hh, b_hh in ws:
                gi, dh = torch.randn(off[-1], 3 * h_dim), torch.randn(b, h_dim)
                probs.append(dict(gi=gi, dh=dh, w_hh=w_hh, b_hh=b_hh, off=off_c, b=b,
                                  ref=_gru_float64(gi, off, w_hh, b_hh, dh)))
        _GRU_LAYOUT_CASE.append((h_dim, probs))
    return _GRU_LAYOUT_CASE[0]


@pytest.mark.parametrize('route', ['persistent', 'steps', 'f32'])
def test_gru_layouts_four_problems_two_layouts_match_a_float64_recurrence(dev, route, monkeypatch):
    """renet_gru_{fwd,bwd}_layouts directly: four problems, two layouts (three workgroup tiles with a partial last one,
    tiles that finish early), two shared W_hh -- both bf16x6 structures (RENET_GRU) and the exact-fp32 kernels (per-model
    mode 'f32') against a float64 recurrence, with the tolerances of test_gru_matches_torch_cpu."""
    import contextlib
    import renet_hip as K
    if route == 'f32':
        monkeypatch.delenv('RENET_GRU', raising=False)
    else:
        monkeypatch.setenv('RENET_GRU', route)
    h_dim, probs = _gru_layout_case()
    w_dev = {}                                   # problems of one W_hh pass the SAME device tensor (one plane split)
    for p in probs:
        w_dev.setdefault(id(p['w_hh']), (p['w_hh'].to(dev), p['b_hh'].to(dev)))
    w_hhs = [w_dev[id(p['w_hh'])][0] for p in probs]
    b_hhs = [w_dev[id(p['w_hh'])][1] for p in probs]
    offs = [p['off'] for p in probs]
    out_rows = [p['b'] + 3 if k < 2 else p['b'] for k, p in enumerate(probs)]
    with K.gemm_mode('f32') if route == 'f32' else contextlib.nullcontext():
        hs, svs = K.gru_fwd_layouts([p['gi'].to(dev) for p in probs], offs, h_dim, w_hhs, b_hhs, out_rows)
        d_gis, d_ghs = K.gru_bwd_layouts([p['dh'].to(dev) for p in probs], offs, h_dim, w_hhs, svs)
    for k, p in enumerate(probs):
        h_ref, sv_ref, dgi_ref, dgh_ref = p['ref']
        b = p['b']
        assert hs[k].shape == (out_rows[k], h_dim) and float(hs[k][b:].abs().sum()) == 0.0, k
        np.testing.assert_allclose(hs[k][:b].cpu().numpy(), h_ref.numpy(), rtol=1e-4, atol=1e-5, err_msg='h_last %d' % k)
        sv = svs[k].cpu().numpy()
        for c, name in enumerate(('r', 'z', 'n', 'hn', 'hp')):
            np.testing.assert_allclose(sv[:, c * h_dim:(c + 1) * h_dim], sv_ref.numpy()[:, c * h_dim:(c + 1) * h_dim],
                                       rtol=1e-4, atol=1e-5, err_msg='saved %s %d' % (name, k))
        np.testing.assert_allclose(d_gis[k].cpu().numpy(), dgi_ref.numpy(), rtol=1e-3, atol=2e-5, err_msg='dGi %d' % k)
        np.testing.assert_allclose(d_ghs[k].cpu().numpy(), dgh_ref.numpy(), rtol=1e-3, atol=2e-5, err_msg='dGh %d' % k)


def test_fused_directions_of_forward_equal_the_two_calls_of_train_py(dev):
    """RENet.fuse_directions through the real kernels: train.py:136-138's two model() calls as one merged pass (eval-mode
    masks: dropout 0, so both forms are deterministic) -- per-direction values and the gradient of the sum."""
    c = train_case('small', 200)
    net, gd = _build_model(c, dev, dropout=0.0)
    net.train()
    batch = torch.from_numpy(c['batch']).to(dev)
    (sh, sht), (oh, oht) = c['hists']['s'], c['hists']['o']

    def two_calls():
        net.zero_grad()
        ls = net(batch, (sh, sht), (oh, oht), gd, subject=True)
        lo = net(batch, (sh, sht), (oh, oht), gd, subject=False)
        (ls + lo).backward()
        return float(ls), float(lo), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    ls0, lo0, g0 = two_calls()
    net.fuse_directions = True
    ls1, lo1, g1 = two_calls()
    assert net._fused_pending is None
    assert abs(ls0 - ls1) <= 2e-5 * abs(ls0) and abs(lo0 - lo1) <= 2e-5 * abs(lo0), (ls0, ls1, lo0, lo1)
    assert g0.keys() == g1.keys()
    for k in g0:
        scale = float(g0[k].abs().max())
        assert float((g0[k] - g1[k]).abs().max()) <= 2e-4 * scale + 1e-9, k


@pytest.mark.parametrize('passes', ['separate', 'merged'])
def test_train_mode_gradients_match_finite_differences_under_replayed_masks(dev, passes):
    """Train mode (dropout 0.5 at all four sites: RGCN self-loop, sequence assembly x2, both heads): with the seed
    counter reset before every forward the masks replay, so loss(theta) is a fixed function -- its analytic gradient
    (every backward kernel regenerating its forward mask) must match the directional finite difference along the
    gradient, per parameter tensor."""
    import ops
    c = train_case('small', 200)
    net, gd = _build_model(c, dev, dropout=0.5)
    net.train()
    batch_np = c['batch']
    batch = torch.from_numpy(batch_np).to(dev)

    def loss_fn():
        torch.manual_seed(4242)
        ops.reset_seed_counter(0)
        if passes == 'merged':
            return net.loss_prepared_both(net.prepare_both(batch_np, c['hists']['s'], c['hists']['o'], gd))
        return net(batch, c['hists']['s'], c['hists']['o'], gd, subject=True) + \
            net(batch, c['hists']['s'], c['hists']['o'], gd, subject=False)

    net.zero_grad()
    l0 = loss_fn()
    l0.backward()
    assert float(loss_fn()) == float(l0), 'masks must replay'
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    checked = 0
    for k, p in net.named_parameters():
        g = grads.get(k)
        if g is None or float(g.norm()) < 1e-6:
            continue
        d = g / g.norm()
        eps = 2e-2 * max(float(p.detach().abs().max()), 1e-3)
        with torch.no_grad():
            p.add_(eps * d)
            lp = float(loss_fn())
            p.sub_(2 * eps * d)
            lm = float(loss_fn())
            p.add_(eps * d)
        fd = (lp - lm) / (2 * eps)
        an = float(g.norm())                          # directional derivative along g / |g|
        assert abs(fd - an) <= 0.05 * an + 2e-4, (passes, k, fd, an)
        checked += 1
    assert checked >= 10


# ---------------------------------------------------------------------------------------------
# global model vs the reference (golden)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,d,maxpool', [('tiny', 100, 1), ('tiny', 200, 0), ('small', 200, 1)])
def test_global_model_matches_reference_golden(dev, name, d, maxpool):
    import global_model as GM
    import utils as U
    gold = load_golden('global_%s_%d_max%d.npz' % (name, d, maxpool))
    cfg, tr, va, te = fixtures.split_dataset(name)
    seq_len = int(gold['seq_len'])
    p = fixtures.make_params(int(gold['param_seed']), global_shapes(cfg['num_ent'], cfg['num_rels'], d))
    net = GM.RENet_global(cfg['num_ent'], d, cfg['num_rels'], dropout=0.0, seq_len=seq_len, maxpool=maxpool)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    net.to(dev)
    gd = U.build_graph_dict(tr, cfg['num_rels'])
    times = np.unique(tr[:, 3])
    loss = net(torch.from_numpy(times), torch.from_numpy(gold['true_s']).to(dev),
               torch.from_numpy(gold['true_o']).to(dev), gd, subject=True)
    assert abs(loss.item() - float(gold['loss'])) < 2e-4 * max(1.0, abs(float(gold['loss'])))
    loss.backward()
    for k, prm in net.named_parameters():
        if ('grad.' + k) in gold or ('grad.' + k + '__samp') in gold:
            ok, err, how = fixtures.check_packed(gold, 'grad.' + k, prm.grad.cpu().numpy(), 2e-3, 3e-5)
            assert ok, (k, err, how)
    with torch.no_grad():
        for k, t in enumerate(gold['predict_t']):
            for subj in (True, False):
                emb, logits, prob = net.predict(int(t), gd, subject=subj)
                tag = 'predict%d_%s_' % (k, 's' if subj else 'o')
                np.testing.assert_allclose(emb.view(-1).cpu().numpy(), gold[tag + 'emb'], rtol=RTOL, atol=ATOL)
                np.testing.assert_allclose(logits.view(-1).cpu().numpy(), gold[tag + 'logits'], rtol=RTOL, atol=ATOL)
        ge = net.get_global_emb(times, gd)
        assert [int(x) for x in ge.keys()] == gold['global_emb_keys'].tolist()
        vals = np.stack([ge[x].view(-1).cpu().numpy() for x in ge.keys()])
        np.testing.assert_allclose(vals, gold['global_emb_vals'], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------
# dropout: statistics, determinism, backward uses the same mask
# ---------------------------------------------------------------------------------------------
def test_dropout_mask_statistics_and_backward_consistency(dev):
    import ops
    x = torch.ones(4096, 200, device=dev, requires_grad=True)
    y = ops.DropoutFn.apply(x, 0.5, 1234)
    frac = float((y == 0).float().mean())
    assert abs(frac - 0.5) < 0.01
    assert set(torch.unique(y.detach()).cpu().tolist()) == {0.0, 2.0}
    y.sum().backward()
    assert torch.equal(x.grad, y.detach()), 'backward must regenerate the forward mask'
    y2 = ops.DropoutFn.apply(x, 0.5, 1234)
    y3 = ops.DropoutFn.apply(x, 0.5, 1235)
    assert torch.equal(y, y2) and not torch.equal(y, y3)
    y4 = ops.DropoutFn.apply(x, 0.25, 7)
    assert abs(float((y4 == 0).float().mean()) - 0.25) < 0.01


def test_training_mode_runs_and_is_seed_reproducible(dev):
    c = train_case('small', 200)
    net, gd = _build_model(c, dev, dropout=0.5)
    net.train()
    batch = torch.from_numpy(c['batch']).to(dev)
    import ops
    vals = []
    for _ in range(2):
        torch.manual_seed(999)
        ops._seed_state['counter'] = 0
        net.zero_grad()
        loss = net(batch, c['hists']['s'], c['hists']['o'], gd, subject=True)
        loss.backward()
        vals.append((loss.item(), net.ent_embeds.grad.clone()))
    assert vals[0][0] == vals[1][0] and torch.equal(vals[0][1], vals[1][1])
    assert np.isfinite(vals[0][0]) and abs(vals[0][0] - float(c['gold']['loss_s'])) > 1e-6


# ---------------------------------------------------------------------------------------------
# full-size properties (ICEWS18-shaped batch graph, D=200): linearity, permutation invariance,
# paired-edge adjointness <y, A x> == <A^T y, x>
# ---------------------------------------------------------------------------------------------
def _big_graph(dev, n=20000, m=45000, num_rels=256, seed=3):
    import graph as G
    rng = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, n + 1) ** 0.9
    pop /= pop.sum()
    s = rng.choice(n, m, p=pop)
    o = rng.choice(n, m, p=pop)
    r = np.minimum((rng.pareto(1.2, m) * 3).astype(np.int64), num_rels - 1)
    src = np.concatenate((s, o))
    dst = np.concatenate((o, s))
    et = np.concatenate((r, r + num_rels))
    hb = G.HostBatch.from_edges(n, src, dst, et, num_rels)
    return hb, G.DeviceGraph(hb, dev), (src, dst, et)


def test_full_size_gather_properties(dev):
    import graph as G
    import renet_hip as K
    d, R = 200, 256
    hb, g, (src, dst, et) = _big_graph(dev, num_rels=R)
    torch.manual_seed(0)
    w = torch.randn(2 * R, d * 2, device=dev) * 0.1
    x1 = torch.randn(hb.N, d, device=dev)
    x2 = torch.randn(hb.N, d, device=dev)

    def A(x, shift=0, tr=False, graph=g, heavy=True):
        out = torch.empty_like(x)
        if heavy:       # the production kernel: planned item stream + one workgroup per hub row
            K.rgcn_gather_items(x, graph, w, shift, tr, None, 0.0, 0, False, out, use_norm=not tr)
        else:           # the plain-CSR kernel walking every row, hubs included, in one wave
            K.rgcn_gather(x, graph.row_ptr, graph.col, graph.etype, graph.norm if not tr else None, w, shift, tr,
                          None, 0.0, 0, False, out, None, 0)
        return out
    y1, y2, y12 = A(x1), A(x2), A(2.0 * x1 - 3.0 * x2)
    # hub rows (in-degree > graph.HEAVY) go through the workgroup-per-row kernel: same values as the
    # single-kernel walk up to summation order
    assert g.heavy_rows is not None and g.heavy_rows.numel() > 10 and int(np.diff(hb.row_ptr).max()) > 200
    np.testing.assert_allclose(A(x1, heavy=False).cpu().numpy(), y1.cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(y12.cpu().numpy(), (2.0 * y1 - 3.0 * y2).cpu().numpy(), rtol=1e-4, atol=1e-4)
    # edge-order invariance: a different edge permutation builds the same rows up to summation order
    perm = np.random.RandomState(9).permutation(len(src))
    hb2 = G.HostBatch.from_edges(hb.N, src[perm], dst[perm], et[perm], R)
    g2 = G.DeviceGraph(hb2, dev)
    np.testing.assert_allclose(A(x1, graph=g2).cpu().numpy(), y1.cpu().numpy(), rtol=1e-4, atol=1e-5)
    # adjointness of the backward-wrt-h formulation:  <z, norm * M x> == <M^T (norm * z), x>
    z = torch.randn(hb.N, d, device=dev)
    lhs = float((z.double() * y1.double()).sum())
    gn = z * g.norm.view(-1, 1)
    rhs = float((A(gn.contiguous(), shift=R, tr=True).double() * x1.double()).sum())
    assert abs(lhs - rhs) < 1e-5 * max(1.0, abs(lhs)), (lhs, rhs)
    # zero in-degree rows stay exactly zero without an addend
    zero_rows = np.nonzero(np.diff(hb.row_ptr) == 0)[0]
    assert len(zero_rows) > 0 and float(y1[torch.from_numpy(zero_rows).to(dev)].abs().max()) == 0.0
    # run-to-run bit reproducibility (no atomics anywhere)
    assert torch.equal(A(x1), y1)


def test_full_size_dw_matches_fp64_sampled(dev):
    import renet_hip as K
    d, R = 200, 256
    hb, g, (src, dst, et) = _big_graph(dev, num_rels=R, seed=4)
    torch.manual_seed(1)
    x = torch.randn(hb.N, d, device=dev)
    gn = torch.randn(hb.N, d, device=dev)
    dw = torch.empty(2 * R, 2 * d, device=dev)
    K.rgcn_bwd_w(x, gn, g.e_src, g.e_dst, g.chunk_ptr, g.chunk_type, g.n_chunks, g.type_chunk_ptr, 2 * R, 0, dw)
    dw2 = torch.empty_like(dw)
    K.rgcn_bwd_w(x, gn, g.e_src, g.e_dst, g.chunk_ptr, g.chunk_type, g.n_chunks, g.type_chunk_ptr, 2 * R, 0, dw2)
    acc = dw.clone()                                      # beta = 1: accumulate into an existing gradient
    K.rgcn_bwd_w(x, gn, g.e_src, g.e_dst, g.chunk_ptr, g.chunk_type, g.n_chunks, g.type_chunk_ptr, 2 * R, 0, acc,
                 beta=1.0)
    assert torch.equal(acc, dw + dw)
    assert torch.equal(dw, dw2)
    # the 64-bit-addressing entry (feature tensors >= 2 GiB) is the same arithmetic in the same order
    os.environ['RENET_BWDW_64'] = '1'
    try:
        dw64 = torch.empty_like(dw)
        K.rgcn_bwd_w(x, gn, g.e_src, g.e_dst, g.chunk_ptr, g.chunk_type, g.n_chunks, g.type_chunk_ptr, 2 * R, 0, dw64)
    finally:
        del os.environ['RENET_BWDW_64']
    assert torch.equal(dw64, dw)
    xc, gc = x.cpu().double().numpy(), gn.cpu().double().numpy()
    got = dw.cpu().numpy()
    for t in (0, 1, 5, R, R + 2, 2 * R - 1):
        e = np.nonzero(et == t)[0]
        xs, gs = xc[src[e]].reshape(-1, 100, 2), gc[dst[e]].reshape(-1, 100, 2)
        ref = np.einsum('ebi,ebj->bij', xs, gs).reshape(-1)
        np.testing.assert_allclose(got[t], ref, rtol=1e-4, atol=1e-4 * max(1.0, len(e)) ** 0.5)


def test_softmax_ce_in_place_is_race_free(dev):
    """renet_softmax_ce with dlogits aliasing logits (the training path): the row loss must not depend on when other
    waves overwrite the row.  (Round 2 found thread 0's read of x[target] sunk below the barrier by the compiler
    because both pointers were declared __restrict__ and, in the streamed kernel, again as a scalar load sunk into the
    thread-0 branch: a rare wrong LOSS with correct gradients.)  Repeated launches
    on recycled allocations, against torch's cross entropy; both kernels (row in LDS / streamed)."""
    import renet_hip as K
    torch.manual_seed(3)
    for b, c in ((96, 150), (4096, 150), (2048, 700), (64, 23033), (33, 40000)):
        logits0 = torch.randn(b, c, device=dev) * 3
        tgt = torch.randint(0, c, (b,), device=dev)
        ref = torch.nn.functional.cross_entropy(logits0, tgt, reduction='none')
        p = torch.softmax(logits0, dim=1)
        p[torch.arange(b, device=dev), tgt] -= 1.0
        for it in range(60):
            junk = torch.full((b * c + it,), float('nan'), device=dev)
            del junk
            lg = logits0.clone()
            loss = K.softmax_ce(lg, tgt.int(), 0.5, True)
            assert float((loss - ref).abs().max()) < 1e-4, (b, c, it)
            assert float((lg - 0.5 * p).abs().max()) < 1e-5, (b, c, it)


def test_stale_hip_error_of_another_caller_does_not_fail_our_launches(dev):
    """hipGetLastError() is per-thread state shared with every other HIP user in the process: an expected-to-fail
    call of the host framework (here: hipMalloc of an absurd size) must not be reported as OUR launch failure."""
    import ctypes
    import renet_hip as K
    hip = ctypes.CDLL('libamdhip64.so')
    table = torch.arange(40, device=dev, dtype=torch.float32).view(10, 4)
    idx = torch.tensor([3, 1], device=dev, dtype=torch.int32)
    torch.cuda.synchronize()
    ptr = ctypes.c_void_p()
    rc = hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(1 << 60))
    assert rc != 0                                   # failed, and left its error code in the thread's slot
    out = K.gather_rows(table, idx)                  # our launch clears the slot and reports only its own status
    assert out.tolist() == [[12.0, 13.0, 14.0, 15.0], [4.0, 5.0, 6.0, 7.0]]


def test_exact_fp32_mode_in_a_subprocess(dev):
    """RENET_GEMM=f32 selects the exact-fp32 MFMA kernels (gemm.hip, gru_fwd/bwd_kernel) for the whole library;
    the switch is read once per process, so the GRU / training-step parity tests are re-run in a child process."""
    import subprocess
    import sys
    if os.environ.get('RENET_GEMM') == 'f32':
        pytest.skip('already running in f32 mode')
    env = dict(os.environ, RENET_GEMM='f32')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-m', 'gpu', '-x', '-k',
                        'gru_matches_torch_cpu or training_step or global_model'], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'no tests ran' not in r.stdout


def test_f16x3_fast_mode_in_a_subprocess(dev):
    """RENET_GEMM=f16x3 (22-bit operand split, the opt-in fast mode since round 4; the default is the 24-bit bf16x6
    split): the GRU / training-step / global-model parity tests and the stream / operand-bound tests re-run in a child
    process with the switch set (it is read once per process)."""
    import subprocess
    import sys
    if os.environ.get('RENET_GEMM') == 'f16x3':
        pytest.skip('already running in f16x3 mode')
    env = dict(os.environ, RENET_GEMM='f16x3')
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), os.path.join(here, 'test_gpu_streams.py'),
                        '-q', '-m', 'gpu', '-x', '-k',
                        'gru_matches_torch_cpu or training_step or global_model or stream or bounds or dual_head'],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'no tests ran' not in r.stdout


# ---------------------------------------------------------------------------------------------
# multi-step inference (model.py:216-419): evaluate_filter trajectory vs the reference (golden)
# ---------------------------------------------------------------------------------------------
def _eval_setup(dev, gold):
    """Model, global model, histories and graph dict in the state test.py has before its evaluation loop."""
    import global_model as GM
    import model as M
    import preprocess as P
    import utils as U
    cfg, tr, va, te = fixtures.split_dataset('small')
    d, seq_len, num_k = int(gold['d']), int(gold['seq_len']), int(gold['num_k'])
    net = M.RENet(cfg['num_ent'], d, cfg['num_rels'], dropout=0.0, seq_len=seq_len, num_k=num_k)
    gnet = GM.RENet_global(cfg['num_ent'], d, cfg['num_rels'], dropout=0.0, seq_len=seq_len, num_k=num_k, maxpool=1)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in
                         fixtures.make_params(int(gold['model_seed']), renet_shapes(cfg['num_ent'], cfg['num_rels'], d)).items()})
    gnet.load_state_dict({k: torch.from_numpy(v) for k, v in
                          fixtures.make_params(int(gold['global_seed']), global_shapes(cfg['num_ent'], cfg['num_rels'], d)).items()})
    net.to(dev).eval()
    gnet.to(dev).eval()
    allq = np.concatenate((tr, va, te))
    hs, ho = P.HistoryIndex(allq, 's', 10), P.HistoryIndex(allq, 'o', 10)
    rng = {'train': np.arange(0, len(tr)), 'valid': np.arange(len(tr), len(tr) + len(va)),
           'test': np.arange(len(tr) + len(va), len(allq))}
    H = {k: (hs.to_lists(v), ho.to_lists(v)) for k, v in rng.items()}
    gd = U.build_graph_dict(tr, cfg['num_rels'])
    samples = [torch.from_numpy(x).to(dev) for x in gold['samples']]
    net.sample_entities = lambda prob: samples.pop(0)          # drive the reference's random trajectory
    total = torch.from_numpy(allq).to(dev)
    valid = torch.from_numpy(va)
    with torch.no_grad():
        net.global_emb = gnet.get_global_emb(np.unique(tr[:, 3]), gd)
        net.graph_dict = gd
        net.init_history(tr, H['train'][0], H['train'][1], valid, H['valid'][0], H['valid'][1], te,
                         H['test'][0], H['test'][1])
        net.latest_time = valid[0][3]
    return net, gnet, H, gd, samples, total, valid, va


def test_evaluate_filter_stream_equals_sequential_calls(dev):
    """evaluate_filter_stream / evaluate_filter_batch / predict_batch (all quadruples of a timestamp in one batch,
    member graphs kept separate per entity) vs one evaluate_filter call per quadruple on an identical model."""
    gold = load_golden('eval_small_100.npz')
    n_eval = int(gold['n_eval'])
    net, gnet, H, gd, samples, total, valid, va = _eval_setup(dev, gold)
    (vs, vst), (vo, vot) = H['valid']
    with torch.no_grad():
        seq = [net.evaluate_filter(valid[i], (vs[i], vst[i]), (vo[i], vot[i]), gnet, total) for i in range(n_eval)]
    ranks_seq = np.asarray([r for r, _ in seq])
    loss_seq = np.asarray([float(l) for _, l in seq])
    net2, gnet2, H2, gd2, samples2, total2, valid2, _ = _eval_setup(dev, gold)
    ranks, loss = net2.evaluate_filter_stream(valid2[:n_eval], (vs[:n_eval], vst[:n_eval]), (vo[:n_eval], vot[:n_eval]),
                                              gnet2, total2)
    assert len(samples) == len(samples2) == 0
    assert list(gd.keys()) == list(gd2.keys())
    for t in gd.keys():
        a, b = gd[t].global_triples(), gd2[t].global_triples()
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    np.testing.assert_allclose(loss, loss_seq, rtol=1e-5, atol=1e-5)
    assert float(np.mean(ranks == ranks_seq)) >= 0.99 and np.abs(ranks - ranks_seq).max() <= 1
    # the quadruples of the timestamp the state is at, in a different order and with a repeated row
    t0 = int(va[n_eval - 1, 3])
    m = np.nonzero(va[:n_eval, 3] == t0)[0][::-1]
    m = np.concatenate((m, m[:1]))
    rk, ls = net2.evaluate_filter_batch(va[m], ([vs[i] for i in m], [vst[i] for i in m]),
                                        ([vo[i] for i in m], [vot[i] for i in m]), gnet2, total2)
    assert rk.shape == (len(m), 2) and np.array_equal(rk[0], rk[-1]) and float(ls[0]) == float(ls[-1])
    np.testing.assert_allclose(ls.cpu().numpy()[:-1], loss_seq[m[:-1]], rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        net2.predict_batch(va[:n_eval], (vs[:n_eval], vst[:n_eval]), (vo[:n_eval], vot[:n_eval]), gnet2)


def test_lookahead_evaluation_equals_the_per_quadruple_calls(dev):
    """RENet.lookahead_eval through the real kernels: test.py's loop (one evaluate_filter call per quadruple, the whole stream
    as all_triplets) answered from one batched evaluation per timestamp vs the plain per-call path on an identical model."""
    gold = load_golden('eval_small_100.npz')
    n_eval = int(gold['n_eval'])
    out = []
    for look in (False, True):
        net, gnet, H, gd, samples, total, valid, va = _eval_setup(dev, gold)
        net.lookahead_eval = look
        (vs, vst), (vo, vot) = H['valid']
        with torch.no_grad():
            res = [net.evaluate_filter(valid[i].to(dev), (vs[i], vst[i]), (vo[i], vot[i]), gnet, total) for i in range(n_eval)]
        assert len(samples) == 0
        graphs = {t: gd[t].global_triples() for t in gd.keys()}
        out.append((np.asarray([r for r, _ in res]), np.asarray([float(l) for _, l in res]), graphs, net))
    (r0, l0, g0, _), (r1, l1, g1, net1) = out
    assert net1._la is not None and list(g0.keys()) == list(g1.keys())
    for t in g0:
        assert all(np.array_equal(x, y) for x, y in zip(g0[t], g1[t]))
    np.testing.assert_allclose(l1, l0, rtol=1e-5, atol=1e-5)
    assert float(np.mean(r0 == r1)) >= 0.99 and np.abs(r0 - r1).max() <= 1


def test_evaluate_filter_matches_reference_golden(dev):
    gold = load_golden('eval_small_100.npz')
    cfg, tr, va, te = fixtures.split_dataset('small')
    n_eval = int(gold['n_eval'])
    net, gnet, H, gd, samples, total, valid, va = _eval_setup(dev, gold)
    n_graphs0 = len(gd) - 0
    with torch.no_grad():
        ranks, losses = [], []
        for i in range(n_eval):
            (vs, vst), (vo, vot) = H['valid']
            rk, loss = net.evaluate_filter(valid[i], (vs[i], vst[i]), (vo[i], vot[i]), gnet, total)
            ranks.append(rk)
            losses.append(float(loss))
    assert len(samples) == 0 and len(gd) - n_graphs0 == int(gold['n_new_graphs'])
    ranks, losses = np.asarray(ranks), np.asarray(losses)
    # the predicted graphs of the timestamps advanced over (top-k of a [R*N_ent] joint distribution)
    mine = []
    for t in list(gd.keys())[n_graphs0:]:
        s_, r_, o_ = gd[t].global_triples()
        q = np.stack((s_, r_, o_, np.full(len(s_), t)), axis=1)
        mine.append(q[np.lexsort((q[:, 2], q[:, 1], q[:, 0]))])
    mine = np.concatenate(mine)
    ref_q = gold['new_graph_quads']
    same_graphs = mine.shape == ref_q.shape and np.array_equal(mine, ref_q)
    bad = np.nonzero(~np.isclose(losses, gold['losses'], rtol=2e-4, atol=2e-4))[0]
    print('predicted graphs identical:', same_graphs, 'loss mismatches at', bad.tolist())
    if not same_graphs:
        a = set(map(tuple, mine.tolist())); b = set(map(tuple, ref_q.tolist()))
        print('only mine', sorted(a - b), 'only ref', sorted(b - a))
    assert same_graphs
    # Reference quirk (documented in DESIGN.md): inside model.py:229-297 the loop variables `s` / `o` shadow
    # the quadruple's own subject / object, so the FIRST quadruple of every new timestamp is scored for the
    # last sampled candidate entities instead of its own.  We score the right entities; those rows are
    # therefore excluded here -- and must be the ONLY rows that differ.
    first_of_t = np.nonzero(np.diff(va[:n_eval, 3]) != 0)[0] + 1
    assert set(bad.tolist()) <= set(first_of_t.tolist()), (bad, first_of_t)
    keep = np.ones(n_eval, dtype=bool)
    keep[first_of_t] = False
    np.testing.assert_allclose(losses[keep], gold['losses'][keep], rtol=2e-4, atol=2e-4)
    agree = float(np.mean(ranks[keep] == gold['ranks'][keep]))
    assert agree >= 0.97, agree                       # fp32 near-ties may swap a rank by one
    assert np.abs(ranks[keep] - gold['ranks'][keep]).max() <= 2
    ranks, gold_ranks = ranks[keep], gold['ranks'][keep]
    mine, ref = O.mrr_hits(ranks.reshape(-1)), O.mrr_hits(gold_ranks.reshape(-1))
    assert abs(mine['mrr'] - ref['mrr']) < 2e-3


@pytest.mark.parametrize('api', ['sequential', 'stream'])
def test_reference_shadowing_switch_reproduces_the_reference_on_every_row(dev, api):
    """RENet.reference_shadowing = True reproduces model.py:229-297's name shadowing: the first quadruple of every
    new timestamp is scored for the entities of the last unsorted-top-k candidates.  Which candidate comes last is
    device dependent, so the test hands the model the entities the reference run recorded (fixture `shadow`) through
    `shadow_pick`, after asserting they ARE candidates of our own top-k -- then EVERY row (the first-of-timestamp
    rows included) matches the reference's losses and ranks."""
    gold = load_golden('eval_small_100.npz')
    n_eval = int(gold['n_eval'])
    net, gnet, H, gd, samples, total, valid, va = _eval_setup(dev, gold)
    shadow = [tuple(int(x) for x in row) for row in gold['shadow']]
    picks = []

    def pick(side, cands):
        k = len(picks) // 2
        want = shadow[k][0 if side == 's' else 1]
        assert want in cands, (side, want, cands)
        picks.append(want)
        return want
    net.reference_shadowing, net.shadow_pick = True, pick
    (vs, vst), (vo, vot) = H['valid']
    with torch.no_grad():
        if api == 'sequential':
            res = [net.evaluate_filter(valid[i], (vs[i], vst[i]), (vo[i], vot[i]), gnet, total) for i in range(n_eval)]
            ranks = np.asarray([r for r, _ in res])
            losses = np.asarray([float(l) for _, l in res])
        else:
            ranks, losses = net.evaluate_filter_stream(valid[:n_eval], (vs[:n_eval], vst[:n_eval]),
                                                       (vo[:n_eval], vot[:n_eval]), gnet, total)
    assert len(picks) == 2 * len(shadow) and len(samples) == 0
    np.testing.assert_allclose(losses, gold['losses'], rtol=2e-4, atol=2e-4)
    assert float(np.mean(ranks == gold['ranks'])) >= 0.97 and np.abs(ranks - gold['ranks']).max() <= 2
    first_of_t = np.nonzero(np.diff(va[:n_eval, 3]) != 0)[0] + 1
    np.testing.assert_allclose(losses[first_of_t], gold['losses'][first_of_t], rtol=2e-4, atol=2e-4)
    # and the default (False) differs from the reference exactly on those rows (the existing golden test)


def test_aggregator_predict_with_appended_graph_matches_oracle(dev):
    """Aggregator.predict / predict_batch (unsorted path) on a history whose last step lives in a graph
    that was appended to graph_dict out of timeline order (what inference does, model.py:301)."""
    import model as M
    import utils as U
    c = train_case('small', 200)
    cfg = c['cfg']
    net, gd = _build_model(c, dev)
    net.eval()
    ogd = O.build_graph_dict(c['train'], cfg['num_rels'])
    rng = np.random.RandomState(4)
    e, new_t = 7, int(max(gd.keys())) + 24
    trip = np.stack((np.full(9, e), rng.randint(0, cfg['num_rels'], 9), rng.randint(0, cfg['num_ent'], 9)), axis=1)
    extra = np.stack((rng.randint(0, cfg['num_ent'], 30), rng.randint(0, cfg['num_rels'], 30),
                      rng.randint(0, cfg['num_ent'], 30)), axis=1)
    data = np.unique(np.concatenate((trip, extra)), axis=0)
    gd[new_t] = U.get_big_graph(data, cfg['num_rels'])
    ogd[new_t] = O.build_time_graph(data, cfg['num_rels'])
    ge = dict(c['global_emb'])
    ge[new_t] = np.linspace(-0.2, 0.2, c['d']).astype(np.float32)
    net.global_emb = {t: torch.from_numpy(v).view(1, 1, -1) for t, v in ge.items()}
    (sh, sht), _, _ = O.build_histories(c['train'], cfg['num_ent'])
    k = max(i for i in range(len(c['train'])) if c['train'][i, 0] == e and len(sh[i]) >= 3)
    hist = list(sh[k][-4:]) + [trip[:, 1:3]]
    hist_t = list(sht[k][-4:]) + [new_t]
    params = {kk: torch.from_numpy(v) for kk, v in c['params'].items()}
    oge = {t: torch.from_numpy(v) for t, v in ge.items()}
    for reverse in (False, True):
        rel = params['rel_embeds'][cfg['num_rels']:] if reverse else params['rel_embeds'][:cfg['num_rels']]
        bg, h2, x, xr = O.aggregator_sequences(params, [hist], [hist_t], [e], [3], rel, ogd, oge, reverse,
                                               len(hist), sort=False)
        with torch.no_grad():
            rel_d = net.rel_embeds[cfg['num_rels']:] if reverse else net.rel_embeds[:cfg['num_rels']]
            inp, inp_r = net.aggregator.predict((hist, hist_t), np.asarray([e]), np.asarray([3]), net.ent_embeds,
                                                rel_d, gd, net.global_emb, reverse=reverse)
        np.testing.assert_allclose(inp.cpu().numpy(), x[0].numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(inp_r.cpu().numpy(), xr[0].numpy(), rtol=RTOL, atol=ATOL)


def test_pruned_last_layer_equals_full_layer_on_kept_rows(dev):
    """RGCNLayerFn with n_out < N (layer evaluated on the subject-row prefix only) vs the full layer:
    identical outputs on the kept rows and identical gradients for a loss that only reads those rows."""
    import graph as G
    import ops
    import preprocess as P
    import synth
    quads, ne, nr, _ = synth.make_stream('ICEWS18', seed=5, num_t=40)
    gd = P.build_graph_dict(quads, nr)
    hs = P.HistoryIndex(quads, 's', 10)
    idx = np.random.RandomState(1).permutation(len(quads))[:512]
    hb = G.build_batch(G.store_for(gd), ne, nr, quads[idx, 0], quads[idx, 1], hs.take(idx), sort=True)
    g = G.DeviceGraph(hb, dev)
    assert 0 < hb.nA < hb.N
    d = 200
    torch.manual_seed(3)
    gout = torch.randn(hb.nA, d, device=dev)
    res = []
    for n_out in (None, hb.nA):
        h = (torch.randn(hb.N, d, device=dev, generator=torch.Generator(device=dev).manual_seed(1))).requires_grad_(True)
        w = (torch.randn(2 * nr, 2 * d, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 0.1).requires_grad_(True)
        lw = (torch.randn(d, d, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 0.1).requires_grad_(True)
        y = ops.RGCNLayerFn.apply(h, w, lw, g, True, False, 0.0, 0, n_out)
        (y[:hb.nA] * gout).sum().backward()
        res.append((y[:hb.nA].detach(), h.grad, w.grad, lw.grad))
    for a, b in zip(res[0], res[1]):
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 2e-5 * max(scale, 1.0), (a.shape, float((a - b).abs().max()), scale)


def test_fused_adam_matches_torch_adam_with_clipping(dev):
    """renet_adam_step (clip + Adam + weight decay + zero_grad on flat buffers) vs
    clip_grad_norm_ + torch.optim.Adam (train.py:61,140-142)."""
    import parallel
    torch.manual_seed(11)

    def make():
        torch.manual_seed(5)
        return torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Tanh(), torch.nn.Linear(53, 23033 % 97)).to(dev)
    ref, mine = make(), make()
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-5)
    opt = parallel.HipAdam(mine, lr=1e-2, weight_decay=1e-5, max_norm=0.05)
    for step in range(4):
        x = torch.randn(64, 37, device=dev)
        for net in (ref, mine):
            (net(x) ** 2).mean().backward()
        nref = torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.05)
        opt_ref.step()
        opt_ref.zero_grad()
        opt.step()
        assert abs(float(opt.norm) - float(nref)) < 1e-5 * float(nref)
        assert float(opt.grads.flat.abs().max()) == 0.0 and opt.grads.check_views()
        for a, b in zip(ref.parameters(), mine.parameters()):
            torch.testing.assert_close(a, b, rtol=2e-5, atol=2e-7)


def test_inplace_gradient_accumulation_equals_autograd_accumulation(dev):
    """With persistent .grad buffers (parallel.FlatGrads) the backward kernels accumulate straight into them;
    the result must equal the ordinary autograd path (fresh .grad tensors), incl. a second accumulation."""
    import ops
    import parallel
    c = train_case('small', 200)
    batch = torch.from_numpy(c['batch']).to(dev)
    grads = []
    for inplace in (False, True):
        net, gd = _build_model(c, dev)
        net.eval()
        ops.INPLACE_GRADS = inplace
        flat = parallel.FlatGrads(net) if inplace else None
        try:
            for _ in range(2):                                   # accumulate two backward passes
                loss = net(batch, c['hists']['s'], c['hists']['o'], gd, subject=True) + \
                    net(batch, c['hists']['s'], c['hists']['o'], gd, subject=False)
                loss.backward()
        finally:
            ops.INPLACE_GRADS = True
        if inplace:
            assert flat.check_views()
        grads.append({k: p.grad.clone() for k, p in net.named_parameters()})
    for k in grads[0]:
        a, b = grads[0][k], grads[1][k]
        scale = max(float(a.abs().max()), 1e-6)
        assert float((a - b).abs().max()) <= 1e-5 * scale, (k, float((a - b).abs().max()), scale)


# ---------------------------------------------------------------------------------------------
# edge cases of the reference semantics: empty / single / ragged histories
# ---------------------------------------------------------------------------------------------
def test_edge_case_batches_match_oracle(dev):
    c = train_case('small', 200)
    cfg = c['cfg']
    net, gd = _build_model(c, dev)
    net.eval()
    ogd = O.build_graph_dict(c['train'], cfg['num_rels'])
    params = {k: torch.from_numpy(v) for k, v in c['params'].items()}
    ge = {t: torch.from_numpy(v) for t, v in c['global_emb'].items()}
    hs, hst = c['hists']['s']
    lens = np.asarray([len(h) for h in hs])
    empty = np.nonzero(lens == 0)[0]
    full = np.nonzero(lens > 0)[0]
    assert len(empty) >= 3 and len(full) >= 3
    cases = {
        'all_empty': empty[:3],                                  # reference: unbound variable crash (quirk 1); we use h = 0
        'one_nonempty': np.concatenate((empty[:2], full[:1])),   # reference: squeeze() drops the batch dim (quirk 2)
        'single_sequence': full[1:2],
        'ragged': np.concatenate((full[:5], empty[:1], full[5:9])),
    }
    for name, sel in cases.items():
        batch = c['batch'][sel]
        h = ([hs[i] for i in sel], [hst[i] for i in sel])
        with torch.no_grad():
            mine = float(net(torch.from_numpy(batch).to(dev), h, h, gd, subject=True))
        if name == 'all_empty':
            # oracle formula with s_h = 0 (what the reference would compute had it not crashed)
            s, r, o = batch[:, 0], batch[:, 1], batch[:, 2]
            ent, rel = params['ent_embeds'], params['rel_embeds'][:cfg['num_rels']]
            z = torch.zeros(len(s), c['d'])
            lo = O.cross_entropy_mean(torch.cat((ent[s], z, rel[r]), 1) @ params['linear.weight'].t() + params['linear.bias'], o)
            lr = O.cross_entropy_mean(torch.cat((ent[s], z), 1) @ params['linear_r.weight'].t() + params['linear_r.bias'], r)
            ref = float(lo + 0.1 * lr)
        else:
            ref = float(O.renet_forward_loss(params, batch, h[0], h[1], ogd, ge, cfg['num_rels'], c['seq_len'], subject=True))
        assert abs(mine - ref) < 2e-4 * max(1.0, abs(ref)), (name, mine, ref)


# ---------------------------------------------------------------------------------------------
# inference selection kernels (model.py:205-209,239): fused joint softmax + radix-select top-k
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,m,k', [(1, 5000, 1), (3, 70001, 10), (11, 256 * 23033, 1000), (2, 4097, 4097), (5, 100000, 999)])
def test_topk_positive_equals_torch_topk(dev, n, m, k):
    import renet_hip as K
    g = torch.Generator(device='cpu').manual_seed(n * 7 + k)
    x = torch.rand(n, m, generator=g).pow(8.0)                   # skewed, many tiny values
    if m >= 70001:
        x[:, ::7] = x[:, 3:4]                                    # blocks of exact ties, some at the threshold
    x = x.to(dev)
    x[0, :3] = 0.0
    vals, idx = K.topk_positive(x, k)
    ref_v, _ = torch.topk(x, k, dim=1, sorted=True)
    got_v, order = torch.sort(vals, dim=1, descending=True)
    assert torch.equal(got_v, ref_v)                             # exact multiset of values
    assert torch.equal(torch.gather(x, 1, idx), vals)            # indices address those values
    srt = torch.sort(idx, dim=1)[0]
    assert bool((srt[:, 1:] != srt[:, :-1]).all()) if k > 1 else True    # no index twice
    assert int(idx.min()) >= 0 and int(idx.max()) < m
    # row-strided view: the joint block of the inference path is a view [n, R * N] of a [n * R, N] matrix
    wide = torch.zeros(n, m + 13, device=dev)
    wide[:, :m] = x
    v2, i2 = K.topk_positive(wide[:, :m], k)
    assert torch.equal(torch.sort(v2, dim=1, descending=True)[0], ref_v)


def test_topk_orders_signed_values_zeros_and_nans(dev):
    """the radix select orders by an order-preserving key, not by the raw bit pattern -- negative values,
    -0.0 and NaNs (which the raw pattern ranks ABOVE every positive number) must not be selected before larger numbers."""
    import renet_hip as K
    g = torch.Generator(device='cpu').manual_seed(3)
    x = torch.randn(5, 6000, generator=g)
    x[:, ::11] = -0.0
    x[:, 5::13] = 0.0
    x[1] = -x[1].abs() - 1.0                                     # an all-negative row
    x[2, 100:140] = float('nan')                                # NaNs: never taken while a number is left
    x = x.to(dev)
    for k in (1, 7, 300):
        vals, idx = K.topk_positive(x, k)
        assert not torch.isnan(vals).any()
        ref_v, _ = torch.topk(torch.nan_to_num(x, nan=float('-inf')), k, dim=1, sorted=True)
        got_v, _ = torch.sort(vals, dim=1, descending=True)
        assert torch.equal(got_v + 0.0, ref_v + 0.0)            # (+0.0: -0.0 and 0.0 compare equal, their bits may differ)
        assert torch.equal(torch.gather(x, 1, idx), vals)


def test_joint_softmax_matches_the_reference_expression(dev):
    """renet_joint_softmax == softmax(logits) * softmax(logits_r)[r] * prob[e] (model.py:205-209 + 239), and the
    fused top-k of the block picks the same (relation, object) continuations as torch.topk on the reference expression."""
    import renet_hip as K
    n, R, N, k = 5, 24, 12554, 100
    g = torch.Generator().manual_seed(4)
    logits = (torch.randn(n * R, N, generator=g) * 3).to(dev)
    lr = (torch.randn(n, R, generator=g) * 2).to(dev)
    prob = torch.rand(n, generator=g).to(dev) * 1e-3
    ref = (torch.softmax(logits, dim=1) * torch.softmax(lr, dim=1).reshape(n * R, 1)).view(n, R * N) * prob.view(n, 1)
    mine = logits.clone()
    K.joint_softmax(mine, R, lr, prob)
    torch.testing.assert_close(mine.view(n, R * N), ref, rtol=5e-6, atol=0.0)      # (different reduction order of the row sums)
    vals, idx = K.topk_positive(mine.view(n, R * N), k)
    rv, ri = torch.topk(ref, k, dim=1)
    same = [len(set(idx[i].tolist()) & set(ri[i].tolist())) for i in range(n)]
    assert min(same) >= k - 1, same                              # identical sets up to a near-tie at the boundary
    torch.testing.assert_close(torch.sort(vals, dim=1, descending=True)[0], rv, rtol=5e-6, atol=0.0)
