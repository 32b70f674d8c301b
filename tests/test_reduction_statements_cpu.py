"""Keeps tests/reduction_statements.py honest without a GPU: the census of the fixed dW layout holds literally, the
statements agree with independent formulations, every derived bound holds for float32 numpy evaluations of the GPU tests'
own operands in three summation orders, and the integer operands really make every order exact.  Run with -s for the
ratios."""
import ctypes

import numpy as np
import pytest
import torch

import reduction_statements as R


def _show(what, v):
    print('\n  host ratio %-50s %.3f' % (what, v))


# ---------------------------------------------------------------------------------------------
# the census layout
# ---------------------------------------------------------------------------------------------
def test_census_of_the_fixed_layout():
    lay = R.census_layout()
    cen = R.census(lay)
    assert cen == R.CENSUS_TABLE
    tcp = lay['type_chunk_ptr']
    chunks = {t: int(tcp[t + 1] - tcp[t]) for t in range(lay['T'])}
    live = [t for t in range(lay['T']) if chunks[t] > 0]
    assert sorted({cen[t][0] for t in live}) == [0, 1, 2, 3, 4, 5, 6, 7]
    assert sorted({cen[t][1] for t in live}) == [0, 1, 2, 3, 4, 5, 6, 7]
    assert {1, 2, 8, 9, 17} <= set(chunks.values())
    assert chunks[0] == 0 and chunks[lay['T'] - 1] == 0 and any(chunks[t] == 0 for t in range(1, lay['T'] - 1))
    assert [t for t in range(lay['T']) if chunks[t] == 0] == [0, 4, 13, 18]
    # the hot type: >= 1120 chunks of 1-3 edges, off a group boundary; 16 reduce waves stride its group starts, wave w
    # takes the starts w, w + 16, ...: two 4-way unrolled rounds need start w + 112 (< n), the remainder loop start
    # w + 128, a third unrolled round would need w + 176: 144 <= n <= 176 for every wave
    hot = max(live, key=lambda t: chunks[t])
    lens = np.diff(lay['chunk_ptr'])
    hot_lens = lens[tcp[hot]:tcp[hot + 1]]
    assert chunks[hot] >= 1120 and cen[hot][0] != 0 and set(hot_lens.tolist()) == {1, 2, 3}
    assert 15 + 128 < cen[hot][2] <= 176
    assert {0, 1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 150} <= set(lens.tolist())
    last = max(live)
    assert lay['chunk_type'][-1] == last and lens[-1] == 1
    assert lay['chunk_ptr'][-1] == lay['E'] == len(lay['e_src']) < 6000
    for a in (lay['e_src'], lay['e_dst']):
        assert a.min() == 0 and a.max() == lay['n_rows'] - 1
    assert np.all(np.diff(lay['chunk_type']) >= 0) and lay['n_chunks'] == tcp[-1]
    for t in range(lay['T']):
        assert np.all(lay['chunk_type'][tcp[t]:tcp[t + 1]] == t)


def test_chunk_layout_reproduces_the_planner():
    """every type cut into 64-edge chunks: chunk_ptr, chunk_type, type_chunk_ptr of renet_host_type_chunks and of
    graph.HostBatch.set_edges"""
    import graph
    import renet_hip as K
    rng = np.random.RandomState(5)
    t_n, n = 9, 40
    counts = [0, 64, 1, 200, 0, 63, 65, 128, 0]
    et = rng.permutation(np.repeat(np.arange(t_n), counts)).astype(np.int64)
    e = len(et)
    src, dst = rng.randint(0, n, e).astype(np.int64), rng.randint(0, n, e).astype(np.int64)
    lay = R.chunk_layout(R.planner_spec(counts, graph.CHUNK), t_n, n)
    cap = e // graph.CHUNK + t_n + 1
    e_src, e_dst = np.empty(e, np.int32), np.empty(e, np.int32)
    tcp, ctype, cptr = np.empty(t_n + 1, np.int32), np.empty(cap, np.int32), np.empty(cap + 1, np.int32)
    nc = ctypes.c_int64(0)
    p = lambda a: a.ctypes.data
    kept = K.lib().renet_host_type_chunks(e, p(src), p(dst), p(et), t_n, graph.CHUNK, n, p(e_src), p(e_dst), p(tcp),
                                         p(ctype), p(cptr), ctypes.addressof(nc))
    assert kept == e and nc.value == lay['n_chunks']
    assert np.array_equal(tcp, lay['type_chunk_ptr'])
    assert np.array_equal(ctype[:nc.value], lay['chunk_type']) and np.array_equal(cptr[:nc.value + 1], lay['chunk_ptr'])
    hb = graph.HostBatch().set_edges(n, src, dst, et, t_n)
    assert hb.n_chunks == lay['n_chunks'] and np.array_equal(hb.type_chunk_ptr, lay['type_chunk_ptr'])
    assert np.array_equal(hb.chunk_type, lay['chunk_type']) and np.array_equal(hb.chunk_ptr, lay['chunk_ptr'])


# ---------------------------------------------------------------------------------------------
# statements against independent formulations
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [100, 300])
def test_dw_statement_is_the_einsum_and_the_abi_emulation(d):
    import cpu_abi_emulation as E
    rng = np.random.RandomState(d)
    t_n, n, si = 7, 50, d // 100
    lay = R.chunk_layout(R.planner_spec([70, 0, 3, 130, 1, 0, 64]), t_n, n, seed=3)
    x, gn = rng.randn(n, d).astype(np.float32), rng.randn(n, d).astype(np.float32)
    old = rng.randn(t_n, d * si).astype(np.float32)
    et, src, dst = R.edge_types(lay), lay['e_src'], lay['e_dst']
    want = np.zeros((t_n, 100, si, si))                       # the einsum of test_dw_300_matches_fp64
    np.add.at(want, et, np.einsum('ebi,ebj->ebij', x.astype(np.float64)[src].reshape(-1, 100, si),
                                  gn.astype(np.float64)[dst].reshape(-1, 100, si)))
    ref, mag, n_e = R.dw_statement(x, gn, lay)
    np.testing.assert_allclose(ref, want.reshape(t_n, -1), rtol=0, atol=1e-12)
    assert np.array_equal(n_e, np.bincount(et, minlength=t_n))
    for shift, beta in ((0, 0.0), (3, 1.0), (6, -0.5)):
        ref, mag, n_e = R.dw_statement(x, gn, lay, shift, beta, old)
        np.testing.assert_allclose(ref, np.roll(want.reshape(t_n, -1), shift, axis=0) + beta * old.astype(np.float64),
                                   rtol=0, atol=1e-12)
        emu = torch.from_numpy(old.copy())
        ti = lambda a: torch.from_numpy(np.asarray(a))
        E.rgcn_bwd_w(ti(x), ti(gn), ti(src), ti(dst), ti(lay['chunk_ptr']), ti(lay['chunk_type']), lay['n_chunks'],
                     ti(lay['type_chunk_ptr']), t_n, shift, emu, beta=beta)
        q = R.ratio(emu.numpy(), ref, n_e[:, None], mag)
        _show('float32 emulation of dW, D=%d shift=%d beta=%g' % (d, shift, beta), q.max())
        assert q.max() <= 1.0


def test_small_statements():
    x = np.array([[1, -7, np.nan], [np.nan, 2, -3]], np.float32)
    assert R.maxabs_statement(x) == 7 and R.maxabs_statement(x[:, 2:]) == 3 and R.maxabs_statement(x[:0]) == 0
    assert R.maxabs_statement(np.array([-np.inf, 1], np.float32)) == np.inf
    row_map = np.array([10, 11, 12, 13])
    got = R.compose_statement(row_map, [2, 1, 3, 0], [5, -1, 0, -2], [3, 0], [1, 1, 2])
    assert [a.tolist() for a in got] == [[12, 1, 13, 0], [5, -3 - 11, 0, -2], [13, 10], [11, 11, 12]]
    t = torch.randn(4000) * torch.tensor([1e-3, 1.0, 300.0, 1e20]).repeat(1000)
    assert np.array_equal(R.rne_bf16(t.numpy()), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.bf16_to_f32(R.rne_bf16(t.numpy())), t.to(torch.bfloat16).float().numpy())
    lay = R.segment_layout([2, 0, 3], 5, seed=1)
    src, old = np.arange(10.0).reshape(5, 2), np.ones((6, 2))
    ref, mag, n = R.segment_add_statement(src, lay, old)
    want = old.copy()
    for u in range(3):
        for k in range(lay['seg_ptr'][u], lay['seg_ptr'][u + 1]):
            want[lay['seg_target'][u]] += src[lay['order'][k]]
    assert np.array_equal(ref, want) and np.array_equal(mag, want)
    assert sorted(n.tolist()) == [0, 0, 0, 1, 3, 4] and len(set(lay['seg_target'].tolist())) == 3
    for u_n in R.SEG_US:
        lens = R.segment_lengths(u_n)
        assert len(lens) == u_n and sum(lens) <= 42000
        if u_n >= 16:
            assert set(lens) >= set(R.SEG_LENGTHS)
    assert [R.colsum_groups(m) for m in (0, 1, 128, 129, 256, 257, 8192, 8193, 100000)] == [1, 1, 1, 2, 2, 3, 64, 64, 64]


# ---------------------------------------------------------------------------------------------
# the bounds against float32 evaluations in three orders, on the GPU tests' own operands
# ---------------------------------------------------------------------------------------------
def _worst_over_orders(terms32, ref, n, mag):
    return max(float(R.ratio(s, ref, n, mag).max()) for s in R.f32_sums(terms32))


@pytest.mark.parametrize('d', [100, 200, 300, 400])
def test_dw_bound_holds_for_float32_sums_in_three_orders(d):
    lay = R.census_layout()
    x, gn, old = R.dw_operands(d, 'randn')
    worst = 0.0
    for beta in R.BETAS:
        ref, mag, n_e = R.dw_statement(x, gn, lay, 0, beta, old)
        for t in range(lay['T']):
            terms = R.dw_terms32(x, gn, lay, t)
            if beta != 0.0:
                terms = np.concatenate((terms, (np.float32(beta) * old[t])[None]))
            worst = max(worst, _worst_over_orders(terms, ref[t], n_e[t], mag[t]))
    _show('dW D=%d, float32 numpy, 3 orders' % d, worst)
    assert 0 < worst <= 1.0


def test_colsum_bound_holds_for_float32_sums_in_three_orders():
    worst = 0.0
    for m, n in R.COLSUM_SHAPES:
        for bf16 in (False, True):
            x, old = R.colsum_operands(m, n, 'randn', bf16)
            for beta in R.BETAS:
                ref, mag = R.colsum_statement(x, beta, old)
                terms = x if beta == 0.0 else np.concatenate((x, (np.float32(beta) * old)[None]))
                worst = max(worst, _worst_over_orders(terms, ref, m, mag))
    _show('colsum, float32 numpy, 3 orders', worst)
    assert 0 < worst <= 1.0


@pytest.mark.parametrize('u_n,d', [(17, 100), (17, 300), (513, 200), (8198, 100)])
def test_segment_add_bound_holds_for_float32_sums_in_three_orders(u_n, d):
    lay, src0, _, old0, _ = R.segment_case(u_n, d, 'randn')
    ref, mag, n = R.segment_add_statement(src0, lay, old0)
    worst = 0.0
    for u in range(min(u_n, 600)):
        k0, k1, tgt = lay['seg_ptr'][u], lay['seg_ptr'][u + 1], lay['seg_target'][u]
        terms = np.concatenate((old0[tgt][None], src0[lay['order'][k0:k1]]))
        worst = max(worst, _worst_over_orders(terms, ref[tgt], n[tgt], mag[tgt]))
    _show('segment add U=%d D=%d, float32 numpy, 3 orders' % (u_n, d), worst)
    assert 0 < worst <= 1.0


# ---------------------------------------------------------------------------------------------
# "bit-equal in any order": the premise
# ---------------------------------------------------------------------------------------------
def test_integer_cases_are_exact_in_any_order():
    """for every integer-operand case of tests/test_gpu_reductions.py the sum of |terms| (which bounds every partial sum of
    every order, and the float64 reference) stays below 2^24, and all terms are integers or, with beta = -0.5, halves"""
    lay = R.census_layout()
    worst = 0.0
    for d in (100, 200, 300, 400):
        x, gn, old = R.dw_operands(d, 'int')
        for beta in R.BETAS:
            ref, mag, _ = R.dw_statement(x, gn, lay, 0, beta, old)
            assert np.array_equal(ref, np.rint(ref * 2) / 2) and np.abs(ref).max() <= mag.max()
            worst = max(worst, mag.max())
        for t in (6, 12):
            worst = max(worst, R.exactness_margin(R.dw_terms32(x, gn, lay, t).astype(np.float64)))
    for m, n in R.COLSUM_SHAPES:
        x, old = R.colsum_operands(m, n, 'int')
        assert np.array_equal(R.bf16_to_f32(R.rne_bf16(x)).reshape(x.shape), x)          # exact in bf16 too
        for beta in R.BETAS:
            ref, mag = R.colsum_statement(x, beta, old)
            assert np.array_equal(ref, np.rint(ref * 2) / 2)
            worst = max(worst, mag.max())
    for u_n in R.SEG_US:
        for d in (100, 400):
            lay_s, src0, src1, old0, old1 = R.segment_case(u_n, d, 'int')
            for s, o in ((src0, old0), (src1, old1)):
                ref, mag, _ = R.segment_add_statement(s, lay_s, o)
                assert np.array_equal(ref, np.rint(ref))
                worst = max(worst, mag.max())
            assert not np.array_equal(src0, src1) and not np.array_equal(old0, old1)
    print('\n  largest sum |terms| of an integer case: %d (2^24 = %d)' % (worst, 2 ** 24))
    assert worst < 2 ** 24
