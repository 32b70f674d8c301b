"""Float64 statement of the recurrence mix (renet_recurrence_mix_rows) and the synthetic stream its tests share.

mix_rows restates include/renet_hip.h's definition on the CSR lists of preprocess.PairIndex.prior_rows:
    a_i    = alpha if W_i > 0 else 0,  W_i = sum of the row's w
    out[o] = log((1 - a_i) softmax(logits_i)[o] + a_i w_i[o] / W_i)
make_stream() is the GPU test stream: 70 entities (not a multiple of 64), 3 relations, 14 timestamps with step 24, about 600
facts; the pair (subject 5, relation 1) has more than 300 facts over 68 distinct objects with counts 1 .. 9 (more partners
than a wave has lanes, more facts than a workgroup has threads), the group (5, 1, 7) has a fact at every timestamp,
duplicates are frequent, entities 60 .. 63 are never a subject, 68 and 69 never an object, and the pairs (subject 64,
relation 2) / (object 66, relation 2) have no facts at all."""
import numpy as np

NUM_ENT, NUM_RELS, NUM_T, STEP, SEQ_LEN = 70, 3, 14, 24, 4
HOT_S, HOT_R, HOT_O = 5, 1, 7
NEVER_SUBJECT, NEVER_OBJECT = (60, 61, 62, 63), (68, 69)
BARE_S, BARE_O, BARE_R = 64, 66, 2


def make_stream(seed=7):
    """int64 [n, 4] = (s, r, o, t), sorted by time (stable)."""
    rng = np.random.RandomState(seed)
    times = np.arange(NUM_T) * STEP
    facts = []
    for o in range(68):                                                   # the hot pair: count 1 + (7 o mod 9) per object
        for _ in range(1 + (7 * o) % 9):
            facts.append((HOT_S, HOT_R, o, int(rng.choice(times))))
    facts += [(HOT_S, HOT_R, HOT_O, int(t)) for t in times]
    subjects = np.asarray([e for e in range(NUM_ENT) if e not in NEVER_SUBJECT])
    objects = np.asarray([e for e in range(NUM_ENT) if e not in NEVER_OBJECT])
    for _ in range(250):
        s, r, o = int(rng.choice(subjects)), int(rng.randint(NUM_RELS)), int(rng.choice(objects))
        if (s == BARE_S and r == BARE_R) or (o == BARE_O and r == BARE_R):
            continue
        facts.append((s, r, o, int(rng.choice(times))))
    facts += [facts[i] for i in rng.choice(len(facts), 8, replace=False)]  # duplicates of whatever they hit
    q = np.asarray(facts, dtype=np.int64)
    return q[np.argsort(q[:, 3], kind='stable')]


def log_softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))


def mix_rows(logits, num_cols, ptr, col, w, alpha):
    """float64 [n, num_cols]: the mixed log-probability rows; logits [n, num_cols] or None (uniform)."""
    n = len(ptr) - 1
    lp = log_softmax64(logits) if logits is not None else np.full((n, num_cols), -np.log(float(num_cols)))
    out = np.empty((n, num_cols), dtype=np.float64)
    for i in range(n):
        a, b = ptr[i], ptr[i + 1]
        W = float(np.sum(w[a:b]))
        al = float(alpha) if W > 0.0 else 0.0
        p = (1.0 - al) * np.exp(lp[i])
        if al > 0.0:
            np.add.at(p, col[a:b], al * w[a:b] / W)
        out[i] = np.log(p)
    return out


def partner_counts(quads, role, ent, rel, as_of, num_ent=NUM_ENT):
    """int64 [num_ent]: per partner the number of facts (ent, rel, partner, t' < as_of) of `quads` -- a mask over the
    quadruples as they stand, no index: the brute-force side of the tests."""
    q = np.asarray(quads)
    e_col, p_col = (0, 2) if role == 0 else (2, 0)
    hit = (q[:, e_col] == ent) & (q[:, 1] == rel) & (q[:, 3] < as_of)
    return np.bincount(q[hit, p_col], minlength=num_ent).astype(np.int64)
