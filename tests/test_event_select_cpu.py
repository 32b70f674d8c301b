"""CPU tests of the host statement of renet_select_events (tests/event_select_statement.py): the sort-and-prefix form
against the brute-force multiset form of the reference's rule, the fold over blocks against the one-shot call, and the
planted ties of the contract.  Everything is compared exactly."""
import numpy as np
import pytest

import event_select_statement as E


def assert_same(a, b, what=''):
    assert len(a) == len(b) == 6
    for name, x, y in zip(('given', 'rel', 'other', 'val', 'mult', 'n'), a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), (what, name, x, y)
    assert np.array_equal(a[3].view(np.int32), b[3].view(np.int32)), what            # bit patterns


def split_groups(block, cuts, R):
    ent, val, off, g_ent, lp, mult = block
    out = []
    for a, b in zip([0] + list(cuts), list(cuts) + [len(g_ent)]):
        out.append((ent[a * R:b * R], val[a * R:b * R], off[a * R:b * R], g_ent[a:b], lp[a:b], mult[a:b]))
    return out


@pytest.mark.parametrize('seed', range(8))
@pytest.mark.parametrize('tie_levels', [None, 3])
def test_statement_equals_the_multiset_form(seed, tie_levels):
    rng = np.random.RandomState(seed)
    G, R, k = int(rng.randint(1, 7)), int(rng.randint(1, 5)), int(rng.randint(1, 9))
    block = E.random_block(rng, G, R, k, tie_levels=tie_levels, max_mult=4)
    carry = None
    for num_k in (1, 3, 8, 40, 1024):
        got, want = E.select_events(block, None, num_k), E.select_events_brute(block, None, num_k)
        assert_same(got, want, (seed, num_k))
        assert int(got[5][0]) <= num_k
    carry = E.select_events(E.random_block(rng, 2, R, k, tie_levels=tie_levels, ent0=100), None, 8)
    assert_same(E.select_events(block, carry, 8), E.select_events_brute(block, carry, 8), (seed, 'carry'))


@pytest.mark.parametrize('seed', range(6))
@pytest.mark.parametrize('n_blocks', [1, 2, 5])
@pytest.mark.parametrize('tie_levels', [None, 3])
def test_fold_over_blocks_equals_the_one_shot_call(seed, n_blocks, tie_levels):
    rng = np.random.RandomState(50 + seed)
    G, R, k = 10, 3, 6
    block = E.random_block(rng, G, R, k, tie_levels=tie_levels, max_mult=5)
    cuts = sorted(rng.choice(np.arange(1, G), n_blocks - 1, replace=False).tolist())
    blocks = split_groups(block, cuts, R)
    assert len(blocks) == n_blocks
    assert all(np.array_equal(a, b) for a, b in zip(E.merge_blocks(blocks), block))
    for num_k in (1, 7, 30, 500):
        assert_same(E.fold(blocks, num_k), E.select_events(block, None, num_k), (seed, n_blocks, num_k))
        assert_same(E.fold(blocks, num_k, E.select_events_brute), E.select_events(block, None, num_k))


def planted(k=3):
    """G = 3 groups (entities 4, 7, 9; multiplicities 2, 1, 3), R = 2, k = 3.  With zero offsets and priors V = val."""
    ninf = -np.inf
    ent = np.array([[5, 6, -1], [1, 2, -1], [-1, -1, -1], [8, 0, -1], [2, -1, -1], [3, 4, -1]], dtype=np.int32)
    val = np.array([[2.0, 1.0, ninf], [3.0, 1.0, ninf], [ninf] * 3, [1.0, ninf, ninf], [1.0, ninf, ninf], [0.5, 0.25, ninf]],
                   dtype=np.float32)
    off = np.zeros(6, dtype=np.float32)
    return ent, val, off, np.array([4, 7, 9], dtype=np.int32), np.zeros(3, dtype=np.float32), np.array([2, 1, 3], dtype=np.int32)


def winners(res):
    n = int(res[5][0])
    return [tuple(int(res[j][i]) for j in (0, 1, 2, 4)) + (float(res[3][i]),) for i in range(n)]


def test_threshold_ties_go_by_position():
    b = planted()
    # order: (4,1,1) 3.0 w2 | (4,0,5) 2.0 w2 | ties at 1.0 by position: (4,0,6) w2, (4,1,2) w2, (7,1,8) w1, (9,0,2) w3 | ...
    assert winners(E.select_events(b, None, 5)) == [(4, 1, 1, 2, 3.0), (4, 0, 5, 2, 2.0), (4, 0, 6, 2, 1.0)]
    assert winners(E.select_events(b, None, 7))[-1] == (4, 1, 2, 2, 1.0)
    assert winners(E.select_events(b, None, 9))[-1] == (7, 1, 8, 1, 1.0)
    assert winners(E.select_events(b, None, 10))[-1] == (9, 0, 2, 3, 1.0)
    assert len(winners(E.select_events(b, None, 9))) == 5


def test_carry_entry_goes_before_an_equal_block_candidate():
    b = planted()
    carry = lambda num_k: E.pack([np.array([1]), np.array([0]), np.array([9]), np.array([2.0], dtype=np.float32),
                                  np.array([1])], num_k)
    got = winners(E.select_events(b, carry(4), 4))
    assert got == [(4, 1, 1, 2, 3.0), (1, 0, 9, 1, 2.0), (4, 0, 5, 2, 2.0)]
    assert winners(E.select_events(b, carry(3), 3)) == got[:2]


def test_empty_slots_minus_inf_and_short_totals():
    b = planted()
    # (7, 1, 0) holds -inf: an ordinary candidate, last; total weight 2*4 + 1*2 + 3*3 = 19
    full = winners(E.select_events(b, None, 1024))
    assert len(full) == 9 and full[-1] == (7, 1, 0, 1, -np.inf) and sum(w[3] for w in full) == 19
    assert len(winners(E.select_events(b, None, 19))) == 9 and len(winners(E.select_events(b, None, 18))) == 8
    res = E.select_events(b, None, 1024)
    assert res[0][9] == -1 and res[1][9] == -1 and res[2][9] == -1 and res[3][9] == -np.inf and res[4][9] == 0
    # all rows empty: nothing
    none = (np.full((2, 3), -1, dtype=np.int32), np.full((2, 3), -np.inf, dtype=np.float32), np.zeros(2, dtype=np.float32),
            np.array([3], dtype=np.int32), np.zeros(1, dtype=np.float32), np.array([1], dtype=np.int32))
    assert int(E.select_events(none, None, 8)[5][0]) == 0


def test_one_heavy_candidate_fills_the_prefix_and_no_block_copies_the_carry():
    ent, val, off, g_ent, lp, mult = planted()
    heavy = (ent, val, off, g_ent, lp, np.array([16, 1, 3], dtype=np.int32))
    assert winners(E.select_events(heavy, None, 16)) == [(4, 1, 1, 16, 3.0)]
    carry = E.select_events(planted(), None, 6)
    assert_same(E.select_events(None, carry, 6), carry)
    assert_same(E.select_events(None, None, 6), E.empty_result(6))


def test_values_are_two_fp32_additions_in_the_stated_order():
    ent = np.array([[0]], dtype=np.int32)
    val = np.array([[1.0]], dtype=np.float32)
    off = np.array([2.0 ** -24], dtype=np.float32)
    lp = np.array([2.0 ** -24], dtype=np.float32)
    res = E.select_events((ent, val, off, np.array([0], dtype=np.int32), lp, np.array([1], dtype=np.int32)), None, 1)
    assert res[3][0] == np.float32(1.0)                        # (1 + 2^-24) rounds to 1 twice; 1 + (2^-24 + 2^-24) would not


def test_symbols_are_bound():
    import renet_hip as K
    assert 'renet_select_events' in K.EXPORTS and 'renet_select_events_workspace' in K.EXPORTS
