"""numpy restatement of the evaluation error, written from its definition:

    d[s, j] = sqrt( sum_c ((pred[s, idx[j], c] - gt[s, idx[j], c]) * std[idx[j], c])^2 )

in a chosen precision (float64: the reference value; float32: the restatement the parity bar is measured against), and the
statistics of a distance buffer in float64.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np


def distances(pred, gt, std, idx, dtype=np.float64):
    idx = np.asarray(idx)
    p = np.asarray(pred)[:, idx, :3].astype(dtype)
    g = np.asarray(gt)[:, idx, :3].astype(dtype)
    s = np.asarray(std)[idx].astype(dtype)
    e = (p - g) * s
    return np.sqrt((e * e).sum(-1, dtype=dtype))


def rel_err(d, d64):
    """max |d - d64| / d64 (the inputs of the parity tests keep d64 away from 0)."""
    return float((np.abs(np.asarray(d, dtype=np.float64) - d64) / d64).max())


def fsum_mean(values):
    """The correctly rounded sum of the values (math.fsum), divided by their number."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    return math.fsum(v.tolist()) / v.size


def two_pass_var(buf):
    a = np.asarray(buf, dtype=np.float64).reshape(-1)
    m = fsum_mean(a)
    return math.fsum(((a - m) ** 2).tolist()) / a.size
