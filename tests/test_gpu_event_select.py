"""GPU tests of renet_select_events (csrc/event_select.hip; run with -m gpu on an MI355X) against its host statement
(tests/event_select_statement.py).  All six result arrays are compared with array_equal, the values by their bit patterns as
well: V is two stated IEEE fp32 additions, so nothing here carries a tolerance."""
import numpy as np
import pytest
import torch

import event_select_statement as E
from test_event_select_cpu import planted

pytestmark = pytest.mark.gpu

BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3                 # RENET_ERR_* of include/renet_hip.h


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def up(arrays, dev):
    return None if arrays is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def run(block, carry, num_k, dev):
    import renet_hip as K
    b = up(block, dev) if block is not None else (None,) * 6
    got = K.select_events(*b, num_k, carry=up(carry, dev))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in got)


def assert_same(got, want, what=''):
    assert len(got) == len(want) == 6
    for name, x, y in zip(('given', 'rel', 'other', 'val', 'mult', 'n'), got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (what, name)
    assert np.array_equal(got[3].view(np.int32), want[3].view(np.int32)), (what, 'value bits')


def check(block, carry, num_k, dev, what=''):
    got, want = run(block, carry, num_k, dev), E.select_events(block, carry, num_k)
    assert_same(got, want, what)
    return got


GRID = [(G, R, k) for G in (1, 3, 7, 40) for R in (1, 5, 33) for k in (1, 4, 33)] + [(1, 5, 1024)]


@pytest.mark.parametrize('G,R,k', GRID)
def test_shape_grid(dev, G, R, k):
    rng = np.random.RandomState(1000 * G + 10 * R + k)
    block = E.random_block(rng, G, R, k, n_ent=max(50, 2 * k), max_mult=4)
    ties = E.random_block(rng, G, R, k, n_ent=max(50, 2 * k), tie_levels=4, max_mult=4)
    for num_k in (1, 8, 100, 1024):
        carry = check(block, None, num_k, dev, ('plain', num_k))
        check(ties, carry, num_k, dev, ('ties + carry', num_k))


def test_planted_threshold_ties_go_by_position(dev):
    """(a): the same V in different rows and groups at the threshold."""
    b = planted()
    for num_k in range(1, 21):
        check(b, None, num_k, dev, num_k)
    rng = np.random.RandomState(3)
    wide = E.random_block(rng, 40, 33, 33, tie_levels=2, max_mult=3)                 # 3 distinct V over ~35 000 candidates
    for num_k in (1, 8, 100, 1024):
        got = check(wide, None, num_k, dev, num_k)
        n = int(got[5][0])
        assert n >= min(num_k, 8) and got[3][0] == got[3][n - 1]                                # the whole prefix is one tie


def test_planted_carry_goes_before_an_equal_block_candidate(dev):
    """(b)."""
    b = planted()
    carry = lambda num_k: E.pack([np.array([1]), np.array([0]), np.array([9]), np.array([2.0], dtype=np.float32),
                                  np.array([1])], num_k)
    got = check(b, carry(4), 4, dev)
    assert (got[0][1], got[1][1], got[2][1]) == (1, 0, 9) and (got[0][2], got[2][2]) == (4, 5) and got[3][1] == got[3][2]
    assert int(check(b, carry(3), 3, dev)[5][0]) == 2


def test_planted_empty_rows_minus_inf_and_short_totals(dev):
    """(c), (d), (e): empty slots and rows; -inf values taken because the total weight is short; everything returned."""
    b = planted()
    got = check(b, None, 1024, dev)
    assert int(got[5][0]) == 9 and got[3][8] == -np.inf and (got[0][8], got[1][8], got[2][8]) == (7, 1, 0)
    check(b, None, 19, dev)
    check(b, None, 18, dev)
    none = (np.full((2, 3), -1, dtype=np.int32), np.full((2, 3), -np.inf, dtype=np.float32), np.zeros(2, dtype=np.float32),
            np.array([3], dtype=np.int32), np.zeros(1, dtype=np.float32), np.array([1], dtype=np.int32))
    assert int(check(none, None, 8, dev)[5][0]) == 0
    rng = np.random.RandomState(4)
    ent, val, off, g_ent, lp, mult = E.random_block(rng, 7, 5, 33, p_empty=0.5, max_mult=1)
    val[ent >= 0] = np.where(rng.rand(int((ent >= 0).sum())) < 0.5, -np.inf, val[ent >= 0])
    val = -np.sort(-val, axis=1)
    got = check((ent, val, off, g_ent, lp, mult), None, 1024, dev)
    n = int(got[5][0])
    assert n == int((ent >= 0).sum()) < 1024 and np.isneginf(got[3][:n]).sum() > 10


def test_planted_heavy_multiplicities(dev):
    """(f): g_mult up to num_k -- a single candidate fills the whole prefix."""
    ent, val, off, g_ent, lp, mult = planted()
    for num_k in (16, 1024):
        heavy = (ent, val, off, g_ent, lp, np.array([num_k, 1, 3], dtype=np.int32))
        assert int(check(heavy, None, num_k, dev)[5][0]) == 1
        later = (ent, val, off, g_ent, lp, np.array([1, 1, num_k], dtype=np.int32))
        check(later, None, num_k, dev)
    rng = np.random.RandomState(5)
    check(E.random_block(rng, 40, 5, 33, max_mult=1024), None, 1024, dev)


def test_planted_chain_of_three_blocks_equals_the_one_shot_statement(dev):
    """(g)."""
    import renet_hip as K
    rng = np.random.RandomState(6)
    for tie_levels in (None, 3):
        blocks, ent0 = [], 0
        for G in (5, 9, 3):
            blocks.append(E.random_block(rng, G, 5, 33, tie_levels=tie_levels, max_mult=6, ent0=ent0))
            ent0 = int(blocks[-1][3][-1]) + 1
        for num_k in (8, 100, 1024):
            carry = None
            for b in blocks:
                carry = K.select_events(*up(b, dev), num_k, carry=carry)
            got = tuple(x.cpu().numpy() for x in carry)
            assert_same(got, E.select_events(E.merge_blocks(blocks), None, num_k), (tie_levels, num_k))


def test_planted_no_block_copies_the_carry(dev):
    """(h): G == 0."""
    carry = E.select_events(planted(), None, 6)
    assert_same(run(None, carry, 6, dev), carry)
    full = E.select_events(E.random_block(np.random.RandomState(7), 40, 5, 33), None, 1024)
    assert int(full[5][0]) > 300
    assert_same(run(None, full, 1024, dev), full)


@pytest.fixture(scope='module')
def large():
    """(i): 40 x 33 x 200 slots, ~10^5 candidates (> 2^16), more than one workgroup per pass."""
    rng = np.random.RandomState(8)
    block = E.random_block(rng, 40, 33, 200, n_ent=300, p_empty=0.1, max_mult=4)
    assert int((block[0] >= 0).sum()) > 1 << 16
    return block, {num_k: E.select_events(block, None, num_k) for num_k in (100, 1024)}


def test_planted_more_than_65536_candidates(dev, large):
    block, want = large
    for num_k, w in want.items():
        assert_same(run(block, None, num_k, dev), w, num_k)


def test_repeatable(dev, large):
    block, want = large
    a, b = run(block, None, 1024, dev), run(block, None, 1024, dev)
    assert_same(a, b)
    assert_same(a, want[1024])


def test_refusals_come_before_any_launch(dev):
    import renet_hip as K
    L = K.lib()
    block = up(planted(), dev)
    out = up(E.empty_result(8), dev)
    before = [x.clone() for x in out]
    ws = torch.zeros(L.renet_select_events_workspace(3, 2, 3, 8) // 8, device=dev, dtype=torch.int64)
    assert ws.numel() > 0
    p = lambda ts: [t.data_ptr() for t in ts]

    def call(G=3, R=2, k=3, num_k=8, blk=None, carry=(None,) * 6, outs=None, w=ws.data_ptr(), wb=None):
        return L.renet_select_events(*(p(block) if blk is None else blk), G, R, k, num_k, *carry, *(p(out) if outs is None else outs),
                                     w, ws.numel() * 8 if wb is None else wb, None)

    assert call() == 0
    torch.cuda.synchronize()
    done = [x.clone() for x in out]
    for o, b in zip(out, before):
        o.copy_(b)
    for kw in (dict(G=-1), dict(R=0), dict(R=1025), dict(k=0), dict(k=1025), dict(num_k=0), dict(num_k=1025),
               dict(blk=[None] + p(block)[1:]), dict(outs=p(out)[:5] + [None]), dict(carry=tuple(p(out)[:5]) + (None,))):
        assert call(**kw) == BADARG, kw
    assert call(G=1 << 20, R=1024, k=1024) == UNSUPPORTED
    for kw in (dict(w=None), dict(wb=ws.numel() * 8 - 8), dict(w=ws.data_ptr() + 4)):
        assert call(**kw) == WORKSPACE, kw
    for bad in ((-1, 2, 3, 8), (3, 0, 3, 8), (3, 2, 1025, 8), (3, 2, 3, 0)):
        assert L.renet_select_events_workspace(*bad) == 0
    torch.cuda.synchronize()
    for o, b in zip(out, before):                                                    # nothing ran: the outputs are untouched
        assert torch.equal(o, b)
    assert_same(tuple(x.cpu().numpy() for x in done), E.select_events(planted(), None, 8))
