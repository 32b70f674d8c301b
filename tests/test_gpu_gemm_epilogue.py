"""GPU tests of the staged GEMM epilogue (store_tile_staged in csrc/gemm_tiles.h): every tiled MFMA GEMM family sends its
64 x 64 accumulator blocks through LDS and stores 16-byte row pieces.  The staged path must give the bits of the direct
path (RENET_GEMM_EPILOGUE=direct, read once per process: child pairs), and must touch nothing outside the logical output:
not the row-stride padding, not the rows around a view, not a column at or beyond N when a 16-byte group straddles it."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), 're-net_amd')

# (m, n, k, ta, tb, split_k): the smallest shapes that reach every branch of the epilogue
SHAPES = [
    (1, 1, 1, 0, 0, 1),                          # single element
    (130, 257, 33, 0, 0, 1),                     # ragged rows, N % 4 = 1, K tail
    (257, 130, 71, 1, 1, 1),                     # transposed operands, ragged tile edges
    (300, 129, 64, 1, 0, 1),                     # transposed A
    (96, 100, 5000, 0, 0, 7),                    # partial planes, N a multiple of 4
    (200, 200, 4097, 0, 0, 3),                   # partial planes, K tail
    (260, 23033 % 512 + 512, 48, 0, 0, 1),       # a straddling group behind full column tiles
]
# the weight-gradient form of the planes GEMM (test_gemm_planes_epilogue_accumulate_device_alpha_and_bias_column)
COL_OUT_SHAPES = [(700, 130, 520, 1), (2100, 600, 300, 1), (600, 200, 5000, 6)]
# shapes that reach the kernels the small ones do not (with bias, beta = 1 only): 576 tiles -- the two-phase 128-row kernels,
# the 256-row bf16-storage kernel, and more tiles than a persistent planes grid has workgroups (512: RENET_P6_PERSISTENT=1
# then stores a tile and starts the DMA of its next one); 216 split tiles with K-contiguous A -- the 256-row split kernels
KERNEL_SHAPES = [(3000, 3000, 48, 0, 1, 1), (1300, 1100, 256, 0, 0, 4)]

# argv: package dir, output .npz, families (comma separated)
_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import renet_hip as K
dev = torch.device('cuda:0')
SHAPES, COL_OUT_SHAPES, KERNEL_SHAPES = %r, %r, %r
out = {}

def padded(x):
    """x [m, n] as a view of a buffer whose row stride is a multiple of 4 floats (what the staged path needs)"""
    m, n = x.shape
    buf = torch.zeros(m, (n + 3) & ~3, device=dev)
    buf[:, :n] = torch.from_numpy(x).to(dev)
    return buf[:, :n]

def operands(m, n, k, ta, tb, seed):
    rng = np.random.RandomState(seed)
    a = rng.uniform(-1, 1, (k, m) if ta else (m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, (n, k) if tb else (k, n)).astype(np.float32)
    bias = rng.uniform(-1, 1, n).astype(np.float32)
    c0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    return a, b, bias, c0

for fam in sys.argv[3].split(','):
    for m, n, k, ta, tb, sk in SHAPES + KERNEL_SHAPES:
        a, b, bias, c0 = operands(m, n, k, ta, tb, m * 131 + n * 17 + k)
        ad, bd, biasd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(bias).to(dev)
        if fam == 'planes':
            ad, bd = K.pack_planes(ad), K.pack_planes(bd)
        small = (m, n, k, ta, tb, sk) in SHAPES
        for with_bias, beta in ((0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0)) if small else ((1, 1.0),):
            c = padded(c0)
            kw = dict(ta=bool(ta), tb=bool(tb), out=c, bias=biasd if with_bias else None, alpha=0.75, beta=beta, split_k=sk)
            if fam == 'planes':
                K.gemm_planes(ad, bd, **kw)
            elif fam == 'bf16s':
                K.gemm(ad, bd, **kw)                     # RENET_GEMM=bf16s in the environment
            else:
                K.gemm(ad, bd, mode=fam, **kw)
            out['%%s_%%d_%%d_%%d_%%d_%%d_b%%d_beta%%d' %% (fam, m, n, k, ta, tb, with_bias, int(beta))] = c.cpu().numpy()
    if fam == 'planes':
        for m, n, k, sk in COL_OUT_SHAPES:
            rng = np.random.RandomState(m + n + k)
            a = rng.uniform(-1, 1, (k, m)).astype(np.float32)
            b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
            c = padded(rng.uniform(-1, 1, (m, n)).astype(np.float32))
            v = torch.from_numpy(rng.uniform(-1, 1, m).astype(np.float32)).to(dev)
            K.gemm_planes(K.pack_planes(torch.from_numpy(a).to(dev)), K.pack_planes(torch.from_numpy(b).to(dev), ones_col=True),
                          ta=True, out=c, col_out=v, alpha=0.5, alpha_dev=torch.full((), 0.37, device=dev), beta=1.0,
                          split_k=sk)
            out['planes_colout_%%d_%%d_%%d_c' %% (m, n, k)] = c.cpu().numpy()
            out['planes_colout_%%d_%%d_%%d_v' %% (m, n, k)] = v.cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[2], **out)
print('ok')
''' % (SHAPES, COL_OUT_SHAPES, KERNEL_SHAPES)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _child_pair(families, extra_env):
    """The same seeded cases in two fresh child processes, staged and direct (side by side): {name: (staged, direct)}."""
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for tag, env in (('staged', {}), ('direct', {'RENET_GEMM_EPILOGUE': 'direct'})):
            e = dict(os.environ, **extra_env)
            e.pop('RENET_GEMM_EPILOGUE', None)
            e.update(env)
            path = os.path.join(tmp, tag + '.npz')
            procs.append((tag, path, subprocess.Popen([sys.executable, '-c', _CHILD, PKG, path, families], env=e,
                                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        res = {}
        for tag, path, p in procs:
            text, _ = p.communicate(timeout=600)
            assert p.returncode == 0 and text.strip().endswith('ok'), tag + ': ' + text
            with np.load(path) as z:
                res[tag] = {k: z[k] for k in z.files}
    assert sorted(res['staged']) == sorted(res['direct']) and res['staged']
    return {k: (res['staged'][k], res['direct'][k]) for k in res['staged']}


def _assert_same_bits(pairs):
    bad = [k for k, (s, d) in sorted(pairs.items()) if not np.array_equal(s.view(np.uint32), d.view(np.uint32))]
    for k in bad[:8]:
        s, d = pairs[k]
        print('%s: %d of %d elements differ, max |diff| %.3e' % (k, int((s != d).sum()), s.size, float(np.abs(s - d).max())))
    assert not bad, 'staged epilogue differs from the direct one in %d of %d outputs: %s' % (len(bad), len(pairs), bad[:8])


def test_staged_epilogue_equals_direct_bit_for_bit_fp32_class_families(dev):
    """bf16x6 (kernel by grid size), f16x3 and the planes GEMM (128-row tile), every shape with and without bias, beta = 0
    and beta = 1; the planes GEMM also with alpha_dev and the ones column / col_out.  The fused bf16x6 kernel (grids of at
    most 256 tiles) and the single-plane bf16 kernel have the direct epilogue only: they run along so that the switch keeps
    meaning nothing to them."""
    _assert_same_bits(_child_pair('bf16x6,f16x3,bf16,planes', {}))


def test_staged_epilogue_equals_direct_bit_for_bit_two_phase_kernels_at_every_shape(dev):
    """RENET_GEMM_KERNEL=split sends the small grids to the two-phase 128-row bf16x6 kernel as well (by default they run
    the fused one): its un-split epilogue with and without bias, beta = 0 and 1, ragged edges and the straddling group."""
    _assert_same_bits(_child_pair('bf16x6', {'RENET_GEMM_KERNEL': 'split'}))


def test_staged_epilogue_equals_direct_bit_for_bit_256_row_in_loop_kernels_at_every_shape(dev):
    """RENET_GEMM_TALL=1 / RENET_H3_TALL=1 select the 8-wave 256-row bf16x6 and f16x3 kernels for every grid (by default
    from 1000 tiles on, or 200 split ones): their un-split epilogue too, 16-row passes in the f16x3 one."""
    _assert_same_bits(_child_pair('bf16x6,f16x3', {'RENET_GEMM_KERNEL': 'split', 'RENET_GEMM_TALL': '1', 'RENET_H3_TALL': '1'}))


def test_staged_epilogue_equals_direct_bit_for_bit_bf16_storage(dev):
    """RENET_GEMM=bf16s is process-wide: a child pair of its own."""
    _assert_same_bits(_child_pair('bf16s', {'RENET_GEMM': 'bf16s'}))


def test_staged_epilogue_equals_direct_bit_for_bit_planes_256_row_tile(dev):
    _assert_same_bits(_child_pair('planes', {'RENET_P6_TILE': '256'}))


def test_staged_epilogue_equals_direct_bit_for_bit_planes_persistent(dev):
    """RENET_P6_PERSISTENT=1: a workgroup stores a tile through the ring and then starts the DMA of its next one."""
    _assert_same_bits(_child_pair('planes', {'RENET_P6_PERSISTENT': '1'}))


def _run_family(K, fam, a, b, out):
    ad, bd = torch.from_numpy(a).to(out.device), torch.from_numpy(b).to(out.device)
    if fam == 'planes':
        K.gemm_planes(K.pack_planes(ad), K.pack_planes(bd), tb=True, out=out)
    else:
        K.gemm(ad, bd, tb=True, out=out, mode=fam)


# (ld, n, first column of the view): staged with a straddling group | unaligned stride: direct | misaligned base: direct
VIEWS = [(260, 257, 0), (341, 333, 0), (340, 333, 1)]


@pytest.mark.parametrize('fam', ['bf16x6', 'f16x3', 'planes', 'bf16', 'bf16s'])
@pytest.mark.parametrize('ld,n,c0', VIEWS)
def test_nothing_outside_the_logical_output_is_written(dev, fam, ld, n, c0):
    """The output is a view buf[1:1+m, c0:c0+n] of a NaN-filled [m + 2, ld] buffer: afterwards everything outside the view
    is still NaN and the view holds the product (fp64 reference, the tolerances of test_gpu_planes.py; the two bf16
    families against the product of their bf16-rounded operands)."""
    import renet_hip as K
    m, k = 130, 90
    rng = np.random.RandomState(ld * 7 + n + c0)
    a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    buf = torch.full((m + 2, ld), float('nan'), device=dev)
    out = buf[1:1 + m, c0:c0 + n]
    _run_family(K, fam, a, b, out)
    torch.cuda.synchronize()
    if fam in ('bf16', 'bf16s'):
        a = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
        b = torch.from_numpy(b).to(torch.bfloat16).float().numpy()
    ref = a.astype(np.float64) @ b.T.astype(np.float64)
    got = buf.cpu().numpy()
    np.testing.assert_allclose(got[1:1 + m, c0:c0 + n], ref, rtol=1e-5, atol=1e-5 * k ** 0.5)
    outside = np.ones(got.shape, dtype=bool)
    outside[1:1 + m, c0:c0 + n] = False
    assert np.isnan(got[outside]).all(), 'written outside the view: %d elements' % int((~np.isnan(got[outside])).sum())

