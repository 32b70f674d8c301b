"""Host statement of renet_select_events (include/renet_hip.h; csrc/event_select.hip), in numpy, and an independent
brute-force form of the same rule.

A block is (ent int32 [G * R, k], val fp32 [G * R, k], off fp32 [G * R], g_ent int32 [G], g_lprior fp32 [G], g_mult int32
[G]); a carry / result is (given, rel, other int32 [num_k], val fp32 [num_k], mult int32 [num_k], n int32 [1]), the slots
behind n holding -1, -1, -1, -inf, 0.  Candidate values are V = (val + off[row]) + g_lprior[g] in np.float32, the two additions
in that order."""
import numpy as np

EMPTY = (-1, -1, -1, np.float32(-np.inf), 0)


def empty_result(num_k):
    return pack([np.zeros(0, dtype=np.int64)] * 3 + [np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64)], num_k)


def pack(cols, num_k):
    """(given, rel, other, V, mult) of the winners, in order -> the padded result."""
    n = len(cols[0])
    assert n <= num_k
    out = []
    for c, fill, dt in zip(cols, EMPTY, (np.int32, np.int32, np.int32, np.float32, np.int32)):
        a = np.full(num_k, fill, dtype=dt)
        a[:n] = c
        out.append(a)
    return tuple(out) + (np.asarray([n], dtype=np.int32),)


def candidates(block, carry, num_k):
    """Every candidate in (carry in stored order, then flat position) order: (given, rel, other, V fp32, mult)."""
    cols = [[], [], [], [], []]
    if carry is not None:
        n = min(max(int(carry[5][0]), 0), num_k)
        for j in range(5):
            cols[j].append(np.asarray(carry[j][:n]))
    if block is not None:
        ent, val, off, g_ent, g_lprior, g_mult = block
        rows, k = ent.shape
        G = len(g_ent)
        R = rows // G
        assert rows == G * R
        v = (val.astype(np.float32) + off.astype(np.float32).reshape(-1, 1)).astype(np.float32)
        v = (v + np.repeat(g_lprior.astype(np.float32), R).reshape(-1, 1)).astype(np.float32)
        keep = (ent >= 0).reshape(-1)                       # flat position order = row-major order of [G * R, k]
        given = np.repeat(np.repeat(g_ent, R), k)
        rel = np.repeat(np.tile(np.arange(R), G), k)
        mult = np.repeat(np.repeat(g_mult, R), k)
        for j, a in enumerate((given, rel, ent.reshape(-1), v.reshape(-1), mult)):
            cols[j].append(np.asarray(a)[keep])
    if not cols[0]:
        return [np.zeros(0, dtype=np.int64)] * 3 + [np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64)]
    return [np.concatenate(c) for c in cols]


def select_events(block, carry, num_k):
    """The statement: a stable sort on -V of the candidates in (carry first, position) order, a cumulative weight, the
    shortest prefix that reaches num_k."""
    given, rel, other, v, mult = candidates(block, carry, num_k)
    order = np.argsort(-v.astype(np.float32), kind='stable')
    w = np.cumsum(np.minimum(np.maximum(mult[order].astype(np.int64), 1), num_k))
    n = min(len(order), int(np.searchsorted(w, num_k, side='left')) + 1)
    take = order[:n]
    return pack([given[take], rel[take], other[take], v[take], mult[take]], num_k)


def select_events_brute(block, carry, num_k):
    """The reference's multiset rule (model.py:229-258): every candidate stands in the list `mult` times, the list is ordered
    by value descending (Python's stable sort over the same candidate order), the first num_k entries are taken, and the
    distinct candidates among them are returned, in order."""
    given, rel, other, v, mult = candidates(block, carry, num_k)
    expanded = []
    for i in range(len(v)):
        expanded += [i] * min(max(int(mult[i]), 1), num_k)
    expanded.sort(key=lambda i: -float(v[i]))
    take = []
    for i in expanded[:num_k]:
        if not take or take[-1] != i:
            take.append(i)
    take = np.asarray(take, dtype=np.int64)
    return pack([given[take], rel[take], other[take], v[take], mult[take]], num_k)


def fold(blocks, num_k, select=select_events):
    carry = None
    for b in blocks:
        carry = select(b, carry, num_k)
    return carry if carry is not None else empty_result(num_k)


def merge_blocks(blocks):
    """The blocks (same R, same k) as ONE block: groups concatenated."""
    return tuple(np.concatenate([b[j] for b in blocks]) for j in range(6))


def random_block(rng, G, R, k, n_ent=50, tie_levels=None, p_empty=0.2, max_mult=3, ent0=0):
    """A block as topk_rows and the generation front produce it: rows sorted by value descending with distinct entities,
    a random number of valid slots per row (some rows empty), ascending group entities from ent0 on.  tie_levels: draw the
    values, offsets and priors from that many levels (multiples of 1/4: every sum is exact, so equal V abound)."""
    ent = np.full((G * R, k), -1, dtype=np.int32)
    val = np.full((G * R, k), -np.inf, dtype=np.float32)
    for row in range(G * R):
        n = 0 if rng.rand() < p_empty else int(rng.randint(1, min(k, n_ent) + 1))
        if tie_levels:
            v = rng.randint(0, tie_levels, n).astype(np.float32) / 4
        else:
            v = rng.randn(n).astype(np.float32)
        order = np.argsort(-v, kind='stable')
        ent[row, :n], val[row, :n] = rng.choice(n_ent, n, replace=False), v[order]
        for a in range(n):                                  # equal scores go to the lower column, as topk_rows gives them
            b = a
            while b + 1 < n and val[row, b + 1] == val[row, a]:
                b += 1
            ent[row, a:b + 1] = np.sort(ent[row, a:b + 1])
    if tie_levels:
        off = rng.randint(-tie_levels, 1, G * R).astype(np.float32) / 4
        lprior = rng.randint(-tie_levels, 1, G).astype(np.float32) / 4
    else:
        off = -np.abs(rng.randn(G * R)).astype(np.float32) * 3
        lprior = -np.abs(rng.randn(G)).astype(np.float32) * 2
    g_ent = (ent0 + np.sort(rng.choice(max(4 * G, G + 1), G, replace=False))).astype(np.int32)
    g_mult = rng.randint(1, max_mult + 1, G).astype(np.int32)
    return ent, val, off, g_ent, lprior, g_mult
