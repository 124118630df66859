"""CPU references for the mesh-to-scan distance (cape_amd/point_distance.py).  TEST INFRASTRUCTURE ONLY.

  brute_force(q, p, dtype)           the nearest point over ALL points in the difference form |q - p|^2 evaluated in ``dtype``:
                                     float64 is the reference, float32 the restatement whose error sets the bar
  own_d2(q, p, index)                float64 |q - p[index]|^2 of GIVEN indices
  gradients(q, p, index, g, dtype)   the gradient formulas of d2 for given indices and seed g
"""
import numpy as np


def brute_force(q, p, dtype=np.float64, chunk=None):
    """(index [Q] int64, d2 [Q]) of queries q [Q, 3] against points p [M, 3] (M may be 0): every pair in ``dtype``; the lowest
    index among equal values; -1 / NaN where no point has a finite distance (no finite point, or a non-finite query)."""
    q, p = np.asarray(q, dtype=dtype), np.asarray(p, dtype=dtype)
    Q, M = len(q), len(p)
    index, d2 = np.full(Q, -1, np.int64), np.full(Q, np.nan, dtype)
    if M == 0:
        return index, d2
    chunk = chunk or max(1, (1 << 21) // M)
    with np.errstate(all="ignore"):
        for j0 in range(0, Q, chunk):
            d = q[j0:j0 + chunk, None, :] - p[None]
            s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            s = np.where(np.isfinite(s), s, dtype(np.inf))
            best = np.argmin(s, 1)                                 # the first among equal values
            val = s[np.arange(len(best)), best]
            ok = np.isfinite(val)
            index[j0:j0 + chunk] = np.where(ok, best, -1)
            d2[j0:j0 + chunk][ok] = val[ok]
    return index, d2


def own_d2(q, p, index):
    """float64 |q_j - p[index_j]|^2 [Q] (NaN where index < 0)."""
    q, p, index = np.asarray(q, np.float64), np.asarray(p, np.float64), np.asarray(index, np.int64)
    out = np.full(len(q), np.nan)
    ok = index >= 0
    out[ok] = ((q[ok] - p[index[ok]]) ** 2).sum(-1)
    return out


def gradients(q, p, index, g, dtype=np.float64):
    """(dq [Q, 3], dp [M, 3]) of sum_j g_j d2_j with the indices held, in ``dtype``: dq_j = 2 g_j (q_j - p_index),
    dp[index_j] += -2 g_j (q_j - p_index).  Queries with index < 0 add nothing."""
    q, p, g = np.asarray(q, dtype), np.asarray(p, dtype), np.asarray(g, dtype)
    index = np.asarray(index, np.int64)
    dq, dp = np.zeros_like(q), np.zeros_like(p)
    ok = index >= 0
    r = dtype(2.0) * g[ok, None] * (q[ok] - p[index[ok]])
    dq[ok] = r
    np.add.at(dp, index[ok], -r)
    return dq, dp
