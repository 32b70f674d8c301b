"""Float64 statement of the learned half-life of the recurrence prior (renet_recurrence_mix_rows_decay,
renet_recurrence_gold_rows_decay, recurrence.CopyGate(learn_half_life=True)), shared by the CPU and the GPU tests.

For a row with query time t, decay lam (1 / half-life), counted facts j (t'_j < as_of) at lag D_j = t - t'_j and weights
w_j = 2^(-D_j lam):
    G = sum over gold's facts of w_j     W = sum over all of w_j     GD = sum over gold's of D_j w_j     WD = sum over all of D_j w_j
    q = G / W          dq/dlam = -ln2 (GD W - G WD) / W^2 = -ln2 q (E_gold[D] - E_all[D])
and, with the gate a and m = (1 - a) p_g + a q, L = -log m has dL/dq = -a / m.  rate_k = exp(log_rate_k), so
    dLoss / dlog_rate[k] = rate_k * sum over the rows i of k of weight_i (-a_i / m_i) dq_i
scale = ln2 (GD W + G WD) / W^2 is the magnitude the difference GD W - G WD is taken at: a summation-order error of n 2^-53
per sum shows in dq as at most n 2^-50 scale (four sums, two products), the bound the tests hold dq to.

make_stream() is recurrence_statement.make_stream() plus 150 facts (HOT_S, HOT_R, 9, t), t cycling over the 14 timestamps: 754
facts; the partner group (subject 5, relation 1, object 9) -- and (object 9, relation 1, subject 5) for role 1 -- has more than
150 facts, more than a partner group may have before a whole wave sums it (128), so that path runs with a per-row decay."""
import numpy as np

import recurrence_statement as RS

LONG_S, LONG_R, LONG_O, LONG_EXTRA = RS.HOT_S, RS.HOT_R, 9, 150
RATES = (0.0, float(np.float32(1.0 / 24.0)), float(np.float32(1.0 / 240.0)))
LN2 = float(np.log(2.0))


def make_stream():
    """int64 [754, 4] = (s, r, o, t), sorted by time (stable)."""
    base = RS.make_stream()
    times = np.arange(RS.NUM_T) * RS.STEP
    extra = np.asarray([(LONG_S, LONG_R, LONG_O, int(times[i % RS.NUM_T])) for i in range(LONG_EXTRA)], dtype=np.int64)
    q = np.concatenate((base, extra))
    return q[np.argsort(q[:, 3], kind='stable')]


def long_row(facts, role):
    """(ent, rel, gold, t) of one query on the long partner group of `role`, one step behind the stream's end."""
    end = int(facts[:, 3].max())
    return ((LONG_S, LONG_R, LONG_O) if role == 0 else (LONG_O, LONG_R, LONG_S)) + (end + RS.STEP,)


def statement_queries(facts, role, stale=0):
    """41 queries (ent, rel, t, as_of, gold) of `role`: 40 facts of the stream asked for their own partner at their own time,
    and the long group's row."""
    e_col, p_col = (0, 2) if role == 0 else (2, 0)
    pick = facts[np.random.RandomState(53 + role).choice(len(facts), 40, replace=False)]
    ent, rel, gold, t = (list(pick[:, k]) for k in (e_col, 1, p_col, 3))
    e, r, g, tt = long_row(facts, role)
    ent.append(e), rel.append(r), gold.append(g), t.append(tt)
    ent, rel, gold, t = (np.asarray(x, dtype=np.int64) for x in (ent, rel, gold, t))
    return ent, rel, t, t - stale * RS.STEP, gold


def counted(pair_index, ent, rel, as_of):
    """(partner, t') of the counted facts of one row, in table order."""
    a, b = pair_index.sub_run(int(ent), int(rel))
    seen = pair_index.p_t[a:b] < as_of
    return pair_index.p_other[a:b][seen], pair_index.p_t[a:b][seen]


def gold_rows_decay(pair_index, ent, rel, t, as_of, gold, ihl_row, num_cols):
    """float64 (q, W, dq, scale) [n] and int64 n_counted [n] of the rows (ent, rel, t, as_of) with gold columns `gold` and the
    per-row decays ihl_row; q = dq = 0 for an empty row, a gold outside [0, num_cols) or one without a counted fact."""
    ent, rel, t, gold = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (ent, rel, t, gold))
    as_of = np.broadcast_to(np.asarray(as_of, dtype=np.int64).reshape(-1), ent.shape)
    ihl_row = np.broadcast_to(np.asarray(ihl_row, dtype=np.float64).reshape(-1), ent.shape)
    n = len(ent)
    q, W, dq, scale, cnt = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for i in range(n):
        o, tp = counted(pair_index, ent[i], rel[i], as_of[i])
        cnt[i] = len(o)
        if not len(o):
            continue
        lag = (t[i] - tp).astype(np.float64)
        w = np.exp2(-lag * ihl_row[i])
        hit = (o == gold[i]) & (0 <= gold[i] < num_cols)
        Ws, WD, G, GD = float(w.sum()), float((lag * w).sum()), float(w[hit].sum()), float((lag * w)[hit].sum())
        W[i] = Ws
        if Ws > 0.0 and G > 0.0:
            q[i] = G / Ws
            dq[i] = -LN2 * (GD * Ws - G * WD) / (Ws * Ws)
            scale[i] = LN2 * (GD * Ws + G * WD) / (Ws * Ws)
    return q, W, dq, scale, cnt


def q_autograd(pair_index, ent, rel, t, as_of, gold, ihl_row, num_cols):
    """(q, dq/dlam) float64 [n] by torch float64 autograd of q(lam) = G(lam) / W(lam), row by row: the closed form's check."""
    import torch
    ent, rel, t, gold = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (ent, rel, t, gold))
    as_of = np.broadcast_to(np.asarray(as_of, dtype=np.int64).reshape(-1), ent.shape)
    ihl_row = np.broadcast_to(np.asarray(ihl_row, dtype=np.float64).reshape(-1), ent.shape)
    q, dq = np.zeros(len(ent)), np.zeros(len(ent))
    for i in range(len(ent)):
        o, tp = counted(pair_index, ent[i], rel[i], as_of[i])
        hit = (o == gold[i]) & (0 <= gold[i] < num_cols)
        if not hit.any():
            continue
        lam = torch.tensor(float(ihl_row[i]), dtype=torch.float64, requires_grad=True)
        w = torch.exp2(-torch.from_numpy((t[i] - tp).astype(np.float64)) * lam)
        val = w[torch.from_numpy(hit)].sum() / w.sum()
        val.backward()
        q[i], dq[i] = float(val.detach()), float(lam.grad)
    return q, dq


def mix_rows_decay(pair_index, logits, num_cols, ent, rel, t, as_of, alpha_row, ihl_row):
    """float64 [n, num_cols]: recurrence_statement.mix_rows row by row, each row with its own gate and its own decay."""
    out = []
    for i in range(len(ent)):
        lists = pair_index.prior_rows(ent[i:i + 1], rel[i:i + 1], t[i:i + 1], as_of[i:i + 1], inv_half_life=float(ihl_row[i]))
        out.append(RS.mix_rows(None if logits is None else logits[i:i + 1], num_cols, *lists, float(alpha_row[i])))
    return np.concatenate(out)


def log_rate_gradient(rate, index, weight, a, m, dq):
    """float64 (grad, magnitude) [len(rate)] and int64 rows [len(rate)]: grad[k] = rate_k * sum over the rows i with index_i
    == k of term_i, term_i = weight_i (-a_i / m_i) dq_i; magnitude[k] = rate_k * sum of |term_i| and rows[k] the number of
    rows of k with a non-zero term (what a summation bound is written with)."""
    rate = np.asarray(rate, dtype=np.float64).reshape(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        term = np.where((a > 0) & (dq != 0), weight * (-a / m) * dq, 0.0)
    grad, mag = np.zeros(len(rate)), np.zeros(len(rate))
    np.add.at(grad, index, term)
    np.add.at(mag, index, np.abs(term))
    rows = np.bincount(np.asarray(index)[term != 0], minlength=len(rate)).astype(np.int64)
    return grad * rate, mag * rate, rows
