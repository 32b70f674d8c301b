"""Float64 statement of the joint copy mix (renet_joint_mix_rows) on the CSR lists of preprocess.PairIndex.event_rows.

Per group g with the pairs (r, c) -> w of its row, W = the sum of ALL of the row's w and a = alpha if W > 0 else 0, and with J
the fp32 joint values (scores + off as ONE fp32 addition, which the caller has done) widened to float64:
    M[r, c] = J[r, c] + log1p(-a)                          for a pair without a counted fact
    M[r, c] = log((1 - a) exp(J[r, c]) + a w[r, c] / W)    for a pair with counted facts
A pair whose relation lies outside [0, R) or whose partner lies outside [0, C) counts in W and is not addressed.  A group that
abstains has M = J exactly."""
import numpy as np


def group_mass(rows):
    """float64 [G]: W of every group."""
    ptr, rel, col, w = rows
    return np.asarray([float(np.sum(w[a:b])) for a, b in zip(ptr[:-1], ptr[1:])], dtype=np.float64)


def mix_block(J32, rows, alpha):
    """float64 [G, R, C] from the fp32 joint values J32 [G, R, C] and rows = (ptr, rel, col, w) of event_rows."""
    J32 = np.asarray(J32)
    assert J32.dtype == np.float32 and J32.ndim == 3
    G, R, C = J32.shape
    ptr, rel, col, w = rows
    assert len(ptr) == G + 1
    J = J32.astype(np.float64)
    out = np.empty_like(J)
    for g in range(G):
        a, b = ptr[g], ptr[g + 1]
        W = float(np.sum(w[a:b]))
        al = float(alpha) if W > 0.0 else 0.0
        if al == 0.0:
            out[g] = J[g]                                   # (log1p(-0) = 0 and log(exp(J)) = J: the definition's M is J)
            continue
        out[g] = J[g] + np.log1p(-al)
        r, c, ww = rel[a:b], col[a:b], w[a:b]
        inside = (r >= 0) & (r < R) & (c >= 0) & (c < C) & (ww > 0.0)
        r, c, ww = r[inside], c[inside], ww[inside]
        out[g, r, c] = np.log((1.0 - al) * np.exp(J[g, r, c]) + al * ww / W)
    return out


def logsumexp64(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))
