"""Float64 statement of training through the copy mix (renet_recurrence_gold_rows, renet_mix_ce / renet_mix_ce_planes and
recurrence.CopyGate), shared by the CPU and the GPU tests.

For a row with gold column g, p = softmax(logits), gate a in [0, 1) and the prior's mass on the gold column q = w[g] / W:
    m = (1 - a) p_g + a q,   L = -log m,   dL/dlogits[c] = s (p_c - [c == g]),  s = (1 - a) p_g / m,   dL/da = (p_g - q) / m
gold_rows states q and W on the CSR lists of preprocess.PairIndex.prior_rows; mix_ce the loss and both gradients."""
import numpy as np

from recurrence_statement import log_softmax64


def gold_rows(ptr, col, w, gold, num_cols):
    """(q, W) float64 [n] of the CSR rows (ptr, col, w) for the gold columns `gold`: W the row's sum, q = w[gold] / W; both 0
    for an empty row, q = 0 for a gold outside [0, num_cols) or without a counted fact."""
    n = len(ptr) - 1
    q, W = np.zeros(n), np.zeros(n)
    for i in range(n):
        a, b = ptr[i], ptr[i + 1]
        W[i] = float(np.sum(w[a:b]))
        hit = col[a:b] == gold[i]
        if W[i] > 0.0 and 0 <= gold[i] < num_cols and hit.any():
            q[i] = float(np.sum(w[a:b][hit])) / W[i]
    return q, W


def mix_ce(logits, gold, a, q):
    """float64 (loss [n], dlogits [n, C], d_a [n]) of L = -log((1 - a) softmax(logits)[gold] + a q), per row."""
    lp = log_softmax64(logits)
    n = lp.shape[0]
    a, q = np.asarray(a, dtype=np.float64), np.asarray(q, dtype=np.float64)
    rows = np.arange(n)
    p = np.exp(lp)
    pg = p[rows, gold]
    m = (1.0 - a) * pg + a * q
    plain = (a == 0.0) | (q == 0.0)                                       # the copy term adds nothing: stay in logs
    with np.errstate(divide='ignore', invalid='ignore'):
        loss = np.where(plain, -lp[rows, gold] - np.log1p(-a), -np.log(m))
        s = np.where(plain, 1.0, (1.0 - a) * pg / m)
        d_a = np.where(m > 0.0, (pg - q) / m, 0.0)
    onehot = np.zeros_like(p)
    onehot[rows, gold] = 1.0
    return loss, s[:, None] * (p - onehot), d_a
