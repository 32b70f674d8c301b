"""GPU tests of csrc/joint_rank.hip alone (run with -m gpu on an MI355X): renet_joint_row_offsets against numpy fp64, and
renet_joint_rank_rows -- counts, at_gold, listed -- EXACTLY against a numpy fp32 restatement, on blocks whose additions are
exact by construction (scores in multiples of 1/8, offsets in multiples of 1/4: ties within and across rows) and on the
kernel's own offsets of random scores.  ld = C throughout, so an odd C gives rows that are not 16-byte aligned."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CS = (1, 3, 5, 50, 257, 1031, 23033)
RS = (1, 5, 7)
GS = (1, 3)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    import renet_hip
    renet_hip.lib()                      # fails loudly if the extension is missing
    return torch.device('cuda:0')


def _lse64(x):
    x = x.astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def _offsets64(scores, logits_r):
    """fp64: logsoftmax(logits_r[g])[r] - logsumexp(scores[g, r, :]) for scores [G, R, C], logits_r [G, R]."""
    return (logits_r.astype(np.float64) - _lse64(logits_r)[:, None]) - _lse64(scores)


# ---- offsets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 30.0])
@pytest.mark.parametrize('C', CS)
def test_offsets_equal_numpy_fp64_within_one_ulp(dev, C, scale):
    """One fp32 ulp of the reference value: half an ulp for the single rounding, the other half for fp64 summation-order
    noise that moves a value across a rounding boundary."""
    import renet_hip as K
    rng = np.random.RandomState(C + int(scale))
    for R in RS:
        for G in GS:
            scores = (rng.standard_normal((G, R, C)) * scale).astype(np.float32)
            logits_r = (rng.standard_normal((G, R)) * scale).astype(np.float32)
            got = K.joint_row_offsets(torch.from_numpy(scores).to(dev).view(G * R, C), R, torch.from_numpy(logits_r).to(dev))
            assert got.shape == (G * R,) and got.dtype == torch.float32
            ref = _offsets64(scores, logits_r).reshape(-1)
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
            print('C', C, 'R', R, 'G', G, 'scale', scale, 'largest error in ulps', float((err / ulp).max()))
            assert np.all(err <= ulp), (C, R, G, float((err / ulp).max()))


# ---- counts ------------------------------------------------------------------------------------------------------------
def _queries(rng, G, R, C):
    """Q > G queries, several per group, the LAST group without one when G > 1: (group, gold_r, gold_c) int32 [Q]."""
    used = max(G - 1, 1)
    Q = 3 * used + 1
    group = (np.arange(Q) % used).astype(np.int32)
    return group, rng.randint(0, R, Q).astype(np.int32), rng.randint(0, C, Q).astype(np.int32)


def _lists(rng, Q, R, C, gold_r, gold_c):
    """Per (query, relation) row a list of distinct columns, as ranges of one table: row kinds cycle through empty, all C
    columns, a random subset, and a subset that holds gold_c -- in the gold row (the gold pair: it must stay) and in the other
    rows (it must go, and set `listed`).  -> (cols int32 [len], start [Q * R], count [Q * R], python sets per row)."""
    cols, start, count, sets = [np.asarray([-3, C, C + 7], dtype=np.int32)], [], [], []      # (entries outside the row: ignored)
    at = 3
    for q in range(Q):
        for r in range(R):
            kind = (q * R + r) % 4
            if kind == 0:
                mine = np.zeros(0, dtype=np.int32)
            elif kind == 1:
                mine = rng.permutation(C).astype(np.int32)
            else:
                mine = rng.choice(C, size=rng.randint(0, min(C, 40) + 1), replace=False).astype(np.int32)
                if kind == 3 and gold_c[q] not in mine:
                    mine = np.concatenate((mine, [gold_c[q]])).astype(np.int32)
            # a range may reach the out-of-row entries at the head of the table
            lead = 2 if (kind == 2 and len(mine)) else 0
            if lead:
                cols.append(np.asarray([C + 1, -1], dtype=np.int32))
                at += 2
            start.append(at - lead)
            count.append(len(mine) + lead)
            sets.append(set(mine.tolist()))
            cols.append(mine)
            at += len(mine)
    return np.concatenate(cols), np.asarray(start, dtype=np.int32), np.asarray(count, dtype=np.int32), sets


def _restate(scores, off, group, gold_r, gold_c, sets_a, sets_t):
    """numpy fp32: (counts [6, Q, R], at_gold [Q, R], listed [2, Q, R]) of the definitions in include/renet_hip.h."""
    G, R, C = scores.shape
    Q = len(group)
    J = scores + off.reshape(G, R, 1).astype(np.float32)
    assert J.dtype == np.float32
    counts, at_gold, listed = np.zeros((6, Q, R), dtype=np.int64), np.zeros((Q, R), dtype=np.float32), np.zeros((2, Q, R), dtype=np.int64)
    for q in range(Q):
        g, gr, gc = int(group[q]), int(gold_r[q]), int(gold_c[q])
        v = J[g, gr, gc]
        for r in range(R):
            row = J[g, r]
            at_gold[q, r] = row[gc]
            for k, sets in enumerate((None, sets_a, sets_t)):
                keep = np.ones(C, dtype=bool)
                if sets is not None:
                    mine = sets[q * R + r]
                    keep[np.asarray(sorted(mine), dtype=np.int64)] = False
                    listed[k - 1, q, r] = int(gc in mine)
                    if r == gr:
                        keep[gc] = True
                counts[2 * k, q, r] = np.count_nonzero(row[keep] > v)
                counts[2 * k + 1, q, r] = np.count_nonzero(row[keep] == v)
    return counts, at_gold, listed


def _run(dev, scores, off, group, gold_r, gold_c, la, lt):
    import renet_hip as K
    G, R, C = scores.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    la, lt = (la[:3] if la is not None else (None,) * 3), (lt[:3] if lt is not None else (None,) * 3)
    block = t(scores).view(G * R, C)
    before = block.clone()
    counts, at_gold, listed, rows = K.joint_rank_rows(block, R, t(off), t(group), t(gold_r), t(gold_c), *map(t, la), *map(t, lt))
    assert torch.equal(block, before)                                   # scores is never written
    assert torch.equal(counts, rows.sum(dim=-1))
    return rows.cpu().numpy(), at_gold.cpu().numpy(), listed.cpu().numpy()


def _check(dev, scores, off, rng, timed=True):
    G, R, C = scores.shape
    group, gold_r, gold_c = _queries(rng, G, R, C)
    Q = len(group)
    la = _lists(rng, Q, R, C, gold_r, gold_c)
    lt = _lists(rng, Q, R, C, gold_r, gold_c) if timed else None
    rows, at_gold, listed = _run(dev, scores, off, group, gold_r, gold_c, la, lt)
    want = _restate(scores, off, group, gold_r, gold_c, la[3], lt[3] if timed else None)
    assert np.array_equal(rows, want[0]), (G, R, C, np.argwhere(rows != want[0])[:5])
    assert np.array_equal(at_gold, want[1]) and np.array_equal(listed, want[2])
    if not timed:                      # no time-aware table: that setting gives the raw counts and lists nothing
        assert la[2].sum() > 0 and np.array_equal(rows[4:6], rows[0:2]) and not listed[1].any()
        if C >= 50:
            assert not np.array_equal(rows[2:4], rows[0:2])            # ... while list a did filter
    if G > 1:
        assert G - 1 not in group                                      # a group without a query
    assert Q > G and rows[1].sum(axis=1).min() >= 1                    # the gold pair counts itself
    return rows


@pytest.mark.parametrize('C', CS)
def test_counts_are_exactly_the_numpy_restatement_on_exact_sums(dev, C):
    """Scores in multiples of 1/8 and offsets in multiples of 1/4: every J is exact, and ties occur within and across rows."""
    rng = np.random.RandomState(100 + C)
    ties = 0
    without = []
    for R in RS:
        for G in GS:
            scores = (rng.randint(-24, 25, (G, R, C)) / 8.0).astype(np.float32)
            off = (rng.randint(-8, 9, G * R) / 4.0).astype(np.float32)
            timed = G == 1                                            # G = 3: list a alone, the time-aware table None
            without.append(not timed)
            rows = _check(dev, scores, off, rng, timed=timed)
            ties += int(rows[1].sum()) - rows.shape[1]
    assert any(without) and not all(without)
    if C >= 50:
        assert ties > 0


@pytest.mark.parametrize('C', CS)
def test_counts_on_the_kernels_own_offsets_of_random_scores(dev, C):
    import renet_hip as K
    rng = np.random.RandomState(200 + C)
    for R in RS:
        for G in GS:
            scores = (rng.standard_normal((G, R, C)) * 3).astype(np.float32)
            logits_r = rng.standard_normal((G, R)).astype(np.float32)
            off = K.joint_row_offsets(torch.from_numpy(scores).to(dev).view(G * R, C), R, torch.from_numpy(logits_r).to(dev))
            _check(dev, scores, off.cpu().numpy(), rng, timed=G == 3)   # G = 1: the time-aware table None


def test_indices_out_of_range_are_clamped(dev):
    G, R, C = 3, 5, 257
    rng = np.random.RandomState(7)
    scores = (rng.randint(-24, 25, (G, R, C)) / 8.0).astype(np.float32)
    off = (rng.randint(-8, 9, G * R) / 4.0).astype(np.float32)
    group = np.asarray([-5, G, 1, 2 ** 30], dtype=np.int32)
    gold_r = np.asarray([R, -1, 2, -2 ** 31], dtype=np.int32)
    gold_c = np.asarray([-1, C, 2 ** 31 - 1, 3], dtype=np.int32)
    got = _run(dev, scores, off, group, gold_r, gold_c, None, None)
    clamp = lambda a, n: np.clip(a.astype(np.int64), 0, n - 1)
    want = _restate(scores, off, clamp(group, G), clamp(gold_r, R), clamp(gold_c, C), None, None)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not got[2].any()


def test_bad_arguments_return_the_status_code(dev):
    """Through the return value only: nothing is launched."""
    import renet_hip as K
    L, BAD = K.lib(), -1
    x = torch.zeros(6, 8, device=dev)
    lr, off, at = torch.zeros(2, 3, device=dev), torch.zeros(6, device=dev), torch.zeros(6, device=dev)
    i = torch.zeros(6, device=dev, dtype=torch.int32)
    cnt, lst = torch.zeros(36, device=dev, dtype=torch.int32), torch.zeros(12, device=dev, dtype=torch.int32)
    p = lambda t: t.data_ptr()
    ok = lambda **k: L.renet_joint_row_offsets(k.get('x', p(x)), k.get('ld', 8), k.get('G', 2), k.get('R', 3), k.get('C', 8),
                                               k.get('lr', p(lr)), k.get('ld_r', 3), k.get('off', p(off)), None)
    assert ok() == 0 and ok(G=0) == 0
    for bad in (dict(G=-1), dict(R=0), dict(R=1025), dict(C=0), dict(ld=7), dict(ld_r=2), dict(x=None), dict(lr=None), dict(off=None)):
        assert ok(**bad) == BAD, bad

    def rank(**k):
        a = dict(x=p(x), ld=8, G=2, C=8, R=3, off=p(off), Q=2, group=p(i), gold_r=p(i), gold_c=p(i), cols_a=None, start_a=None,
                 count_a=None, len_a=0, cols_t=None, start_t=None, count_t=None, len_t=0, counts=p(cnt), at_gold=p(at), listed=p(lst))
        a.update(k)
        return L.renet_joint_rank_rows(*a.values(), None)
    assert rank() == 0 and rank(Q=0) == 0
    assert rank(cols_a=p(i), start_a=p(i), count_a=p(i), len_a=6) == 0
    for bad in (dict(Q=-1), dict(G=0), dict(R=0), dict(C=0), dict(ld=7), dict(x=None), dict(off=None), dict(group=None),
                dict(gold_r=None), dict(gold_c=None), dict(counts=None), dict(at_gold=None), dict(listed=None),
                dict(cols_a=p(i)), dict(start_t=p(i), count_t=p(i)), dict(cols_a=p(i), start_a=p(i), count_a=p(i), len_a=-1)):
        assert rank(**bad) == BAD, bad
    torch.cuda.synchronize()
