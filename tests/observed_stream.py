"""The small stream of the observed-history evaluation tests (test_observed_stream_cpu.py, test_gpu_observed_eval.py): ~50
entities, 5 relations, 24 timestamps of 15-25 facts, split 16 / 4 / 4, generated from a fixed seed and CONSTRUCTED to hold
the cases the protocol is about; check_cases() asserts them on the arrays, so that a changed seed cannot hollow the tests
out:
  (a) an entity whose first appearance is in the test split;
  (b) a test query whose entity was active in more than seq_len earlier timestamps;
  (c) several objects for one (s, r, t);
  (d) an (s, r) pair known at another timestamp but not at the query's (time-agnostic set > time-aware set);
  (e) a test query whose subject history is empty while its object history is not."""
import numpy as np

NUM_ENT, NUM_RELS, NUM_T, SEQ_LEN = 50, 5, 24, 3
SPLIT_T = (16, 20)                      # train: t < 16, valid: 16 <= t < 20, test: t >= 20
NEW_ENT = NUM_ENT - 1                   # (a): kept out of the stream until the test split
SEED = 5


def make(seed=SEED):
    """(train, valid, test): int64 [n, 4] = (s, r, o, t), time-ordered."""
    rng = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, NUM_ENT) ** 0.8                  # entities 0 .. NUM_ENT - 2, Zipf-like
    pop /= pop.sum()
    planted = {10: [(0, 1, 7)],                                # (d): (0, 1, 7) holds at t = 10 and never again
               20: [(0, 1, 3), (0, 1, 4), (0, 1, 5)],          # (c): three objects of (0, 1) at t = 20
               21: [(NEW_ENT, 2, 0)],                          # (a), (e): a new subject meets the most popular object
               22: [(1, 3, NEW_ENT), (NEW_ENT, 2, 1)]}
    out = []
    for t in range(NUM_T):
        own = planted.get(t, [])
        m = rng.randint(15, 26) - len(own)
        s, o = rng.choice(NUM_ENT - 1, m, p=pop), rng.choice(NUM_ENT - 1, m, p=pop)
        r = rng.randint(0, NUM_RELS, m)
        q = np.stack((s, r, o), axis=1)
        q[(q[:, 0] == 0) & (q[:, 1] == 1), 1] = 0              # (0, 1, .) facts are the planted ones only
        if own:
            q = np.concatenate((q, np.asarray(own)))[rng.permutation(len(q) + len(own))]
        out.append(np.concatenate((q, np.full((len(q), 1), t)), axis=1))
    allq = np.concatenate(out).astype(np.int64)
    t = allq[:, 3]
    return allq[t < SPLIT_T[0]], allq[(t >= SPLIT_T[0]) & (t < SPLIT_T[1])], allq[t >= SPLIT_T[1]]


def check_cases(train, valid, test, seq_len=SEQ_LEN):
    """Asserts (a)-(e) on the arrays; returns the positions (in the concatenated stream) of the queries that carry them."""
    allq = np.concatenate((train, valid, test))
    first_test = len(train) + len(valid)
    per_t = np.bincount(allq[:, 3], minlength=NUM_T)
    assert len(per_t) == NUM_T and per_t.min() >= 15 and per_t.max() <= 25, per_t
    assert allq[:, [0, 2]].max() == NUM_ENT - 1 and allq[:, 1].max() == NUM_RELS - 1
    found = {}
    # (a)
    before = allq[:first_test]
    assert NEW_ENT not in before[:, 0] and NEW_ENT not in before[:, 2]
    assert NEW_ENT in test[:, 0] and NEW_ENT in test[:, 2]
    # (b), (e): active timestamps per role strictly before the query's
    for i in range(first_test, len(allq)):
        s, r, o, t = allq[i]
        ts = np.unique(allq[(allq[:, 0] == s) & (allq[:, 3] < t), 3])
        to = np.unique(allq[(allq[:, 2] == o) & (allq[:, 3] < t), 3])
        if len(ts) > seq_len:
            found.setdefault('b', i)
        if len(ts) == 0 and len(to) > 0:
            found.setdefault('e', i)
    assert 'b' in found and 'e' in found, found
    # (c), (d)
    for i in range(first_test, len(allq)):
        s, r, o, t = allq[i]
        same = allq[(allq[:, 0] == s) & (allq[:, 1] == r)]
        aware, agnostic = set(same[same[:, 3] == t, 2].tolist()), set(same[:, 2].tolist())
        if len(aware) >= 3:
            found.setdefault('c', i)
        if agnostic - aware:
            found.setdefault('d', i)
    assert 'c' in found and 'd' in found, found
    return found
