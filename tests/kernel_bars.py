"""The two bars of the kernel-level tests of the small training-step kernels (test_gpu_optim / test_gpu_latent /
test_gpu_elementwise), and the bit comparisons they share.  TEST INFRASTRUCTURE ONLY.

element_bar  outputs that are a short float32 expression or a contraction of a few hundred terms: SURVEY 8(c)'s acceptance
             bar (tests/parity_bar.py, factor 4) on max-abs error over max-abs of the float64 result, against the same measure
             of a float32 restatement on the CPU, plus the backstop 2e-5 that does not move with the restatement.
sum_bar      fixed-order float32 sums of thousands to millions of terms: per output element |dev - ref64| <= 2e-6 * sum |terms|
             (the figure tests/test_gpu_ops.py holds the device's fixed-order reductions to), on the condition-aware scale so
             that cancellation in the inputs can neither hide nor fake an error.  The worst measured figure is printed, with
             the same figure of a float32 numpy sum next to it for the record."""
import numpy as np

import parity_bar

TOL = 2e-5            # tests/test_gpu_ops.py
SUM_REL = 2e-6


def mat_err(a, ref):
    a, r = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - r).max() / max(np.abs(r).max(), 1e-30)


def element_bar(test, quantity, dev, f32, ref64):
    dev, f32, ref64 = (np.asarray(v) for v in (dev, f32, ref64))
    assert dev.shape == ref64.shape == f32.shape, (test, quantity, dev.shape, f32.shape, ref64.shape)
    assert np.isfinite(dev).all(), (test, quantity)
    return parity_bar.check(test, quantity, mat_err(dev, ref64), mat_err(f32, ref64), TOL, factor=4.0)


def sum_bar(test, quantity, dev, ref64, abs_terms, f32=None):
    """``abs_terms``: sum of the absolute values of the terms of each output element (same shape as the outputs)."""
    dev, ref64, scale = (np.asarray(v, np.float64) for v in (dev, ref64, abs_terms))
    assert dev.shape == ref64.shape == scale.shape, (test, quantity, dev.shape, ref64.shape, scale.shape)
    assert np.isfinite(dev).all(), (test, quantity)
    err = np.abs(dev - ref64)
    safe = np.where(scale > 0, scale, 1.0)
    worst = float((err / safe).max())
    line = "%s / %s: worst |err| / sum|terms| = %.2e over %d sums" % (test, quantity, worst, dev.size)
    if f32 is not None:
        line += " (float32 numpy sum: %.2e)" % float((np.abs(np.asarray(f32, np.float64) - ref64) / safe).max())
    print(line)
    assert (err <= SUM_REL * scale).all(), line
    return worst


def bits(a):
    """int32 view of a float32 array (negative zero, payloads and all)."""
    a = np.ascontiguousarray(np.asarray(a))
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))
