"""The conditions tests/test_gpu_gemm_products.py rests on, held without a GPU on the very operands it uses
(tests/gemm_statement.py): the host emulations of the six-pair bf16 split and of the f16x3 split keep every bound the GPU
test asserts, a missing low-order term does not, and the two stay far enough apart for the dense test's factor.  The last
test documents the gap this closes: an emulation that loses a3 b1, a2 b2 or a1 b3 passes the rtol / atol check of the other
GEMM tests at a third of its tolerance and fails both new checks."""
import numpy as np
import pytest

import gemm_statement as S

SINGLE_SHAPES = sorted({c[:3] for c in S.P1 + S.P2 + S.S})
SINGLE_SHAPES_H3 = sorted({c[:3] for c in S.P1 + S.P2})
DENSE_SHAPES = S.DENSE_SHAPES + sorted({c[:3] for c in S.S})


def _one_hot(m, n, k, role, shift, family):
    return S.one_hot_case(role, m, n, k, shift, S.one_hot_seed(m, n, k, role, shift), family)


@pytest.mark.parametrize('m,n,k', SINGLE_SHAPES)
def test_six_pair_single_products_keep_2_pow_minus_22_and_every_pair_is_needed(m, n, k):
    """product_planes (all six pairs) within PRODUCT_BOUND['bf16x6'] everywhere; without one of the three small pairs at
    least half of the products leave it; without one of the three large ones practically all do (a factor whose second term
    is below 2^-22 of it -- one value in 2^14 -- is exact without that pair: 99.9 % is asserted, not 100 %)."""
    for role in S.ROLES:
        for shift in S.SHIFTS:
            _, _, fa, fb, _ = _one_hot(m, n, k, role, shift, 'bf16x6')
            assert np.all(np.abs(fa) >= 1e-6) and np.all(np.abs(fb) >= 1e-6)
            clean = S.product_ratio(S.product_planes(fa, fb), fa, fb, 'bf16x6')
            assert clean.max() <= 1.0, (role, shift, clean.max())
            assert np.array_equal(clean, S.single_product_ratio('bf16x6', S.product_planes(fa, fb), fa, fb))
            for pair in S.PAIRS6:
                over = (S.product_ratio(S.product_planes(fa, fb, drop=pair), fa, fb, 'bf16x6') > 1.0).mean()
                assert over >= (0.5 if pair in S.SMALL_PAIRS else 0.999), (role, shift, pair, over)


def test_six_pair_single_products_of_the_persistent_case():
    m, n, k = S.PP[:3]
    _, _, fa, fb, _ = _one_hot(m, n, k, 'A', 0, 'planes')
    assert S.single_product_ratio('planes', S.product_planes(fa, fb), fa, fb).max() <= 1.0
    for pair in S.SMALL_PAIRS:
        assert (S.single_product_ratio('planes', S.product_planes(fa, fb, drop=pair), fa, fb) > 1.0).mean() >= 0.5


@pytest.mark.parametrize('m,n,k', SINGLE_SHAPES_H3)
def test_f16x3_single_products_keep_2_pow_minus_21_and_every_term_is_needed(m, n, k):
    """f16x3_product within the 2^-21 of the header of gemm_h3.hip on magnitudes in [1, 2); without any of its three terms at
    least half of the products leave it."""
    for role in S.ROLES:
        for shift in S.SHIFTS:
            a, b, fa, fb, _ = _one_hot(m, n, k, role, shift, 'f16x3')
            assert 1.0 <= np.abs(fa).min() and np.abs(fa).max() < 2.0 and 1.0 <= np.abs(fb).min() and np.abs(fb).max() < 2.0
            ba, bb = np.abs(a).max(), np.abs(b).max()
            clean = S.single_product_ratio('f16x3', S.f16x3_product(fa, fb, bound_a=ba, bound_b=bb), fa, fb)
            assert clean.max() <= 1.0, (role, shift, clean.max())
            for term in S.H3_TERMS:
                got = S.f16x3_product(fa, fb, drop=term, bound_a=ba, bound_b=bb)
                over = (S.single_product_ratio('f16x3', got, fa, fb) > 1.0).mean()
                assert over >= 0.5, (role, shift, term, over)


def test_f16x3_product_is_the_single_product_form_of_f16x3_matmul():
    rng = np.random.RandomState(3)
    a = rng.uniform(1, 2, (40, 1)).astype(np.float32)
    b = rng.uniform(1, 2, (30, 1)).astype(np.float32)
    for drop in (None,) + S.H3_TERMS:
        assert np.array_equal(S.f16x3_matmul(a, b, drop=drop), S.f16x3_product(a, b.T, drop=drop))


@pytest.mark.parametrize('family', ['bf16x6', 'f16x3'])
@pytest.mark.parametrize('m,n,k', DENSE_SHAPES)
def test_dense_products_in_units_leave_room_between_rounding_and_a_dropped_term(family, m, n, k):
    """2 x (worst units of the emulation) stays below half of the least worst-units value over the dropped low-order terms:
    the GPU test's bound (UNITS_FACTOR x emulation) can tell the defect from rounding at these shapes."""
    a, b = S.dense_case(m, n, k)
    clean = S.dense_units(family, a, b, S.emulate(family, a, b))
    least = min(S.dense_units(family, a, b, S.emulate(family, a, b, drop=d)) for d in S.dropped_terms(family))
    print('%s %s: emulation %.2f units, least dropped-term value %.1f' % (family, (m, n, k), clean, least))
    assert 2.0 * clean < least / 2.0, (clean, least)
    assert S.UNITS_FACTOR[family] * clean < least / 2.0, (clean, least)


@pytest.mark.parametrize('family', ['bf16x6', 'f16x3', 'f32', 'bf16'])
def test_integer_products_are_exact_in_every_emulation(family):
    cases = sorted({c[:3] for c in S.P1 + S.P2 + S.S + [S.INT_LONG]})
    assert max(c[2] for c in cases) == 600
    for m, n, k in cases:
        a, b, bias, c0 = S.int_case(m, n, k, S.seed_of(m, n, k))
        assert np.abs(a).max() == 64 and np.abs(bias).max() <= 64 and np.array_equal(a, np.round(a))
        S.assert_exact(S.emulate(family, a, b).astype(np.float32), S.int_statement(a, b), (family, m, n, k))
        # the epilogue of the GPU test stays exact in fp32 as well: half-integers below 2^23
        ref = S.int_statement(a, b, bias, c0, alpha=0.5, beta=1.0)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.abs(ref).max() < 2.0 ** 23


def test_case_lists_reach_what_they_are_for():
    assert len(S.P1) == 4 and len(S.S) == 4 and {c[2] for c in S.S} == {72, 204}
    for config, (env, families, _) in S.CONFIGS.items():
        for fam in families:
            single, dense, ints = S.single_cases(config, fam), S.dense_cases(config, fam), S.int_cases(config, fam)
            assert {c[7] for c in single} == set(S.SHIFTS) and {c[6] for c in single} == set(S.ROLES)
            assert (S.PP + ('A', 0) in single) == (config == 'planes_persistent')
            assert any(c[:4] == (300, 250, 204, 0) for c in single) == (config == 'default' and fam == 'bf16x6')
            assert {c[:3] for c in dense} >= set(S.DENSE_SHAPES) and (130, 130, 200, 1, 1, 3) in dense
            assert S.INT_LONG + (1,) in ints and len(single) == len(set(single))


@pytest.mark.parametrize('pair', S.SMALL_PAIRS)
def test_a_dropped_small_pair_passes_the_old_tolerance_and_fails_both_new_checks(pair):
    """The census has teeth: the six-pair emulation without (2, 0), (1, 1) or (0, 2), standing in for a kernel's output, goes
    through the assertion helpers the GPU tests call.  It fails the single-product check and the units check, and it passes
    rtol = 1e-5, atol = 1e-5 sqrt(K) -- the one tolerance of test_gpu_parity.py, test_gpu_planes.py, test_gpu_hidden300.py,
    test_gpu_bf16.py and test_gpu_gemm_epilogue.py -- with room to spare."""
    for m, n, k in S.DENSE_SHAPES:
        a, b = S.dense_case(m, n, k)
        got = S.emulate('bf16x6', a, b, drop=pair)
        ref = a.astype(np.float64) @ b.astype(np.float64)
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * k ** 0.5)
        assert (np.abs(got - ref) / (1e-5 * k ** 0.5 + 1e-5 * np.abs(ref))).max() < 0.5
        emulated = S.emulate('bf16x6', a, b)
        S.assert_units('bf16x6', a, b, emulated, emulated, 'clean')
        with pytest.raises(AssertionError, match='units at'):
            S.assert_units('bf16x6', a, b, got, emulated, 'dropped %r' % (pair,))
    m, n, k = S.P1[0][:3]
    for role in S.ROLES:
        for shift in S.SHIFTS:
            _, _, fa, fb, kidx = _one_hot(m, n, k, role, shift, 'bf16x6')
            S.assert_single_products('bf16x6', S.product_planes(fa, fb), fa, fb, kidx, 'clean')
            with pytest.raises(AssertionError, match='single product at'):
                S.assert_single_products('bf16x6', S.product_planes(fa, fb, drop=pair), fa, fb, kidx, 'dropped %r' % (pair,))


@pytest.mark.parametrize('term', S.H3_TERMS[1:])
def test_a_dropped_f16x3_cross_term_fails_both_new_checks(term):
    m, n, k = S.DENSE_SHAPES[1]
    a, b = S.dense_case(m, n, k)
    emulated = S.emulate('f16x3', a, b)
    with pytest.raises(AssertionError, match='units at'):
        S.assert_units('f16x3', a, b, S.emulate('f16x3', a, b, drop=term), emulated, term)
    m, n, k = S.P1[0][:3]
    a, b, fa, fb, kidx = _one_hot(m, n, k, 'A', 1, 'f16x3')
    got = S.f16x3_product(fa, fb, drop=term, bound_a=np.abs(a).max(), bound_b=np.abs(b).max())
    with pytest.raises(AssertionError, match='single product at'):
        S.assert_single_products('f16x3', got, fa, fb, kidx, term)
