"""Float64 statement of training through the JOINT copy mix (renet_joint_gold_rows(_decay), renet_joint_mix_ce(_planes)),
shared by the CPU and the GPU tests.

A row is the given entity e, the gold relation r*, the gold partner g, the query time t and the window as_of.  With the lag
D = t - t' and the weight w = 2^(-D rate) of a fact at t':
    G  = sum of w over the facts (e, r*, g, t' < as_of)       GD = the same sum of D w
    W  = sum of w over ALL facts (e, *, *, t' < as_of)        WD = the same sum of D w      (entity-wide: event_rows' row sum)
    q  = G / W                 dq/drate = -ln2 (GD W - G WD) / W^2
and with p = softmax(entity logits x), pr = softmax(relation logits y)[r*], lp = log pr, the gate a (0 where W = 0):
    m = (1 - a) p_g pr + a q     L = -log m     s = (1 - a) p_g pr / m
    dL/dx[c] = s (p_c - [c == g])     dL/dy[k] = s (pr_k - [k == r*])     dL/da = (p_g pr - q) / m     dL/dq = -a / m
gold_rows states the first block on preprocess.PairIndex.event_rows (G and W) and on the index's own tables (GD and WD: the
lists hold no lags); joint_mix_ce the second."""
import numpy as np

from recurrence_statement import log_softmax64

LN2 = float(np.log(2.0))


def gold_rows(pair_index, ent, rel, t, as_of, gold, rate, num_rels, num_cols):
    """float64 (q, W, dq, G, GD, WD) [n] of the rows (ent, rel, t, as_of, gold) with the decay `rate` (a scalar or one per
    row).  q = dq = W = 0 for an entity without a counted fact; q = dq = 0 (W kept) for a gold outside [0, num_cols), a
    relation outside [0, num_rels) or a pair without a counted fact."""
    ent, rel, t, gold = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (ent, rel, t, gold))
    as_of = np.broadcast_to(np.asarray(as_of, dtype=np.int64).reshape(-1), ent.shape)
    rate = np.broadcast_to(np.asarray(rate, dtype=np.float64).reshape(-1), ent.shape)
    n = len(ent)
    q, W, dq, G, GD, WD = (np.zeros(n) for _ in range(6))
    for i in range(n):
        ptr, r_, c_, w_ = pair_index.event_rows(ent[i:i + 1], t[i:i + 1], as_of[i:i + 1], inv_half_life=float(rate[i]))
        W[i] = float(np.sum(w_))
        inside = 0 <= gold[i] < num_cols and 0 <= rel[i] < num_rels
        hit = (r_ == rel[i]) & (c_ == gold[i])
        if not (W[i] > 0.0 and inside and hit.any()):
            continue
        G[i] = float(np.sum(w_[hit]))
        a, b = int(pair_index.run_ptr[ent[i]]), int(pair_index.run_ptr[ent[i] + 1])
        seen = pair_index.p_t[a:b] < as_of[i]
        pr, po, pt = pair_index.p_rel[a:b][seen], pair_index.p_other[a:b][seen], pair_index.p_t[a:b][seen]
        lag = (t[i] - pt).astype(np.float64)
        lw = lag * np.exp2(-lag * rate[i])
        WD[i] = float(lw.sum())
        GD[i] = float(lw[(pr == rel[i]) & (po == gold[i])].sum())
        q[i] = G[i] / W[i]
        dq[i] = -LN2 * (GD[i] * W[i] - G[i] * WD[i]) / (W[i] * W[i])
    return q, W, dq, G, GD, WD


def joint_mix_ce(x, gold, y, rel, a, q):
    """float64 (L [n], dx [n, C], dy [n, R], d_a [n], d_q [n], s [n]) of L = -log((1 - a) softmax(x)[gold] softmax(y)[rel] +
    a q) per row.  Where a == 0 or q == 0 the copy term adds nothing and the statement stays in logs."""
    lpy = log_softmax64(y)
    rows = np.arange(lpy.shape[0])
    loss, dx, d_a, d_q, s = joint_mix_ce_lp(x, gold, lpy[rows, rel], a, q)
    onehot = np.zeros_like(lpy)
    onehot[rows, rel] = 1.0
    return loss, dx, s[:, None] * (np.exp(lpy) - onehot), d_a, d_q, s


def joint_mix_ce_lp(x, gold, lp, a, q):
    """The same with the relation head reduced to lp = log pr [n]: float64 (L, dx, d_a, d_q, s); dy = s (pr_k - [k == r*])."""
    lpx = log_softmax64(x)
    n = lpx.shape[0]
    rows = np.arange(n)
    a, q, lp = (np.asarray(v, dtype=np.float64) for v in (a, q, lp))
    p = np.exp(lpx)
    lj = lpx[rows, gold] + lp                                              # log(p_g pr)
    pj = np.exp(lj)
    m = (1.0 - a) * pj + a * q
    plain = (a == 0.0) | (q == 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        loss = np.where(plain, -lj - np.log1p(-a), -np.log(m))
        s = np.where(plain, 1.0, (1.0 - a) * pj / m)
        d_a = np.where(m > 0.0, (pj - q) / m, 0.0)
        d_q = np.where(m > 0.0, -a / m, 0.0)
    onehot = np.zeros_like(p)
    onehot[rows, gold] = 1.0
    return loss, s[:, None] * (p - onehot), d_a, d_q, s
