"""GPU tests of the arithmetic of every split GEMM kernel against float64, in measures that see a missing low-order term
(tests/gemm_statement.py; tests/test_gemm_statement_cpu.py holds the conditions they rest on without a GPU):

  (a) single products   one operand is one-hot along k, in each of the four positions of a float4 item: every output is ONE
                        product and must lie within the family's relative bound of the float64 product of its two factors
                        (2^-22 six-pair bf16, 2^-21 f16x3, 2^-24 exact fp32, 2^-7 + 2^-16 one-plane bf16);
  (b) dense products    uniform(-1, 1) operands, the error in units of |a| @ |b| 2^-24 within UNITS_FACTOR x the host
                        emulation's worst value on the same operands;
  (c) integers          operands every format holds exactly: the float64 statement bit for bit, plain and through
                        alpha = 0.5, beta = 1, an integer bias and a row-padded output.

The kernel switches are read once per process, so every configuration of gemm_statement.CONFIGS runs in a child process of its
own (one per test); for the bf16x6 family the child asks renet_gemm_split_plan which kernel each call launches, and the parent
asserts it -- a census must not silently run on another kernel.  None of the bounds is taken from a kernel."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import gemm_statement as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), 're-net_amd')
KERNEL_INDEX = {'fused': 0, 'two_phase_128': 1, 'two_phase_256': 2, 'weight_resident': 3, 'bf16': 4}

# argv: package dir, tests dir, output .npz, families (comma separated); CASES: {family: [(kind, m, n, k, ta, tb, split_k, ...)]}
_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import renet_hip as K
import gemm_statement as S
dev = torch.device('cuda:0')
CASES, KERNEL_INDEX = %r, %r
out = {}

def padded(x):
    m, n = x.shape
    buf = torch.zeros(m, ((n + 3) & ~3) + 4, device=dev)
    buf[:, :n] = torch.from_numpy(x).to(dev)
    return buf[:, :n]

for fam in sys.argv[4].split(','):
    for idx, case in enumerate(CASES[fam]):
        kind, m, n, k, ta, tb, sk = case[:7]
        kw = {}
        if kind == 'single':
            a, b = S.one_hot_case(case[7], m, n, k, case[8], S.one_hot_seed(m, n, k, case[7], case[8]), fam)[:2]
        elif kind == 'dense':
            a, b = S.dense_case(m, n, k)
        else:
            a, b, bias, c0 = S.int_case(m, n, k, S.seed_of(m, n, k))
            if case[7]:
                kw = dict(out=padded(c0), bias=torch.from_numpy(bias).to(dev), alpha=0.5, beta=1.0)
        ad = torch.from_numpy(np.ascontiguousarray(a.T if ta else a)).to(dev)
        bd = torch.from_numpy(np.ascontiguousarray(b.T if tb else b)).to(dev)
        kw.update(ta=bool(ta), tb=bool(tb), split_k=sk)
        if fam == 'planes':
            c = K.gemm_planes(K.pack_planes(ad), K.pack_planes(bd), **kw)
        elif fam == 'bf16s':
            c = K.gemm(ad, bd, **kw)                     # RENET_GEMM=bf16s in the environment
        else:
            c = K.gemm(ad, bd, mode=fam, **kw)
        if fam == 'bf16x6':
            plan = K.gemm_split_plan(ta, tb, m, n, k, lda=ad.stride(0), ldb=bd.stride(0), split_k=sk, a_ptr=ad.data_ptr(),
                                     b_ptr=bd.data_ptr())
            out['plan|%%d' %% idx] = np.int32(KERNEL_INDEX[plan['kernel']])
        out['%%s|%%d' %% (fam, idx)] = c.cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[3], **out)
print('ok')
'''


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()
    return torch.device('cuda:0')


def _skinny_eligible(m, n, k, ta, tb, split_k):
    """renet_gemm_skinny_eligible (gemm_skinny.hip) for the contiguous, 16-byte aligned operands of these tests (lda = k; ldb =
    k when tb), together with the split_k <= 1 of its callers."""
    return not ta and split_k <= 1 and 1 <= n <= 256 and 16 <= k <= 208 and k % 4 == 0 and m >= 256


def _run_config(config, kind, lister):
    """One child process for `config`: every family's cases of `kind` -> ({family: cases}, {name: array})."""
    env_add, families, _ = S.CONFIGS[config]
    cases = {fam: [(kind,) + c for c in lister(config, fam)] for fam in families}
    env = {k: v for k, v in os.environ.items() if k not in S.CONFIG_ENV_KEYS}
    env.update(env_add)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'out.npz')
        p = subprocess.run([sys.executable, '-c', _CHILD % (cases, KERNEL_INDEX), PKG, HERE, path, ','.join(families)], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert p.returncode == 0 and p.stdout.strip().endswith('ok'), '%s: child ended with status %d: %s' % (
            config, p.returncode, p.stdout)
        with np.load(path) as z:
            res = {k: z[k] for k in z.files}
    for fam in families:
        for idx, case in enumerate(cases[fam]):
            m, n, k, ta, tb, sk = case[1:7]
            if fam == 'bf16x6':
                # the kernel of the configuration -- the weight-resident one where the unforced launcher prefers it
                want = 3 if config == 'default' and _skinny_eligible(m, n, k, ta, tb, sk) else S.CONFIGS[config][2]
                assert int(res['plan|%d' % idx]) == want, '%s: %r runs kernel %d, not %d' % (config, case, res['plan|%d' % idx], want)
                if kind != 'int':
                    assert (want == 3) == (case[1:7] in S.S), (config, case)
            if fam == 'f16x3' and kind != 'int':
                # mode f16x3 hands skinny-eligible shapes to the bf16x6 weight-resident kernel: none of these cases is
                assert not _skinny_eligible(m, n, k, ta, tb, sk), case
    return cases, res


def _shape(case):
    return '(m %d, n %d, k %d, ta %d, tb %d, split_k %d)' % tuple(case[1:7])


@pytest.mark.parametrize('config', list(S.CONFIGS))
def test_single_products_stay_within_the_bound_of_their_family(dev, config):
    """(a): alpha = 1, beta = 0, no bias; the split-K reduction adds exact zeros and gets the same bound."""
    cases, res = _run_config(config, 'single', S.single_cases)
    for fam, lst in cases.items():
        worst = {}
        for idx, case in enumerate(lst):
            m, n, k = case[1:4]
            role, shift = case[7:9]
            _, _, fa, fb, kidx = S.one_hot_case(role, m, n, k, shift, S.one_hot_seed(m, n, k, role, shift), fam)
            what = '%s %s %s one-hot %s shift %d' % (config, fam, _shape(case), role, shift)
            q = S.assert_single_products(fam, res['%s|%d' % (fam, idx)], fa, fb, kidx, what)
            worst[case[1:7]] = max(worst.get(case[1:7], 0.0), q)
        for shape, q in worst.items():
            print('single %s %s %s error/bound %.3f' % (config, fam, shape, q))


_emulated = {}


def _emulation(fam, m, n, k):
    """The host emulation of a dense case, computed once per arithmetic and shape and left unchanged."""
    key = ('bf16x6' if fam in S.SIX_PAIR else 'bf16' if fam == 'bf16s' else fam, m, n, k)
    if key not in _emulated:
        a, b = S.dense_case(m, n, k)
        e = S.emulate(key[0], a, b)
        e.setflags(write=False)
        _emulated[key] = e
    return _emulated[key]


@pytest.mark.parametrize('config', list(S.CONFIGS))
def test_dense_products_in_units_stay_within_twice_the_host_emulation(dev, config):
    """(b): every orientation of the three CPU-checked shapes, K = 200 also split three ways."""
    cases, res = _run_config(config, 'dense', S.dense_cases)
    for fam, lst in cases.items():
        for idx, case in enumerate(lst):
            m, n, k = case[1:4]
            a, b = S.dense_case(m, n, k)
            got, emu = S.assert_units(fam, a, b, res['%s|%d' % (fam, idx)], _emulation(fam, m, n, k),
                                      '%s %s %s' % (config, fam, _shape(case)))
            print('dense %s %s %s units %.3f emulation %.3f' % (config, fam, case[1:7], got, emu))


@pytest.mark.parametrize('config', list(S.CONFIGS))
def test_integer_products_are_exact(dev, config):
    """(c): every operand is one bf16 / f16 term, every partial sum is below 2^24, the scales are powers of two."""
    cases, res = _run_config(config, 'int', S.int_cases)
    for fam, lst in cases.items():
        for idx, case in enumerate(lst):
            m, n, k = case[1:4]
            a, b, bias, c0 = S.int_case(m, n, k, S.seed_of(m, n, k))
            ref = S.int_statement(a, b, bias, c0, alpha=0.5, beta=1.0) if case[7] else S.int_statement(a, b)
            S.assert_exact(res['%s|%d' % (fam, idx)], ref, '%s %s %s%s' % (
                config, fam, _shape(case), ' alpha 0.5 beta 1 bias, padded rows' if case[7] else ''))
