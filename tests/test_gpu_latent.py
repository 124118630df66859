"""The latent and condition kernels of the training step on their own, against float64 restatements of include/cape_hip.h:

``ops.VaeSampleKLFn`` (csrc/optim.hip ``vae_fwd_kernel`` / ``vae_bwd_kernel``; reference lib/models.py:193-196, :371-372)

    z = mean + exp(0.5 logvar) eps;  kl = (-0.5 / N) sum(1 + logvar - mean^2 - exp(logvar));  [z | cond] in one buffer
    dmean = gz + (gkl / N) mean;  dlogvar = 0.5 (gz std eps + (gkl / N)(exp(logvar) - 1));  dcond = gz[:, nz:]

``ops.CondNetsFn`` (csrc/condnet.hip; reference lib/models.py:479-511 as called at :284-290)

    h = leaky_0.2(c1 W1 + b1);  ycat = [h W2 + b2 | c2 Wc + bc]  and the six parameter gradients of dycat (+ dycat_b)

at the batch sizes the benchmark runs, at sizes where nothing is a multiple of anything, on both sides of the launch geometry
(several passes of the single forward block, the backward's block cap, workgroups with an empty row slice, the pose /
clothing split inside a 64-column pass) and with the strided gradients the model hands over.  References are plain numpy,
written here; the whole-model tests reach these kernels only at batch 2 with a tolerance sized for a network."""
import types

import numpy as np
import pytest
import torch

from kernel_bars import element_bar, sum_bar, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- sampling + KL
VAE_SHAPES = [(1, 1, 0), (2, 18, 0), (2, 64, 96), (16, 64, 40), (7, 37, 5), (64, 64, 96), (64, 512, 0), (33, 500, 3),
              (16, 18, 32), (32, 64, 64)]            # the last two: shipped nz / condition widths at benchmark batch sizes
GKL = 0.75
BIG = 3.0e6                                          # fills every column the kernels must not read


def _vae_inputs(N, nz, Cc, seed):
    rng = np.random.default_rng(seed)
    mean = (1.5 * rng.standard_normal((N, nz))).astype(np.float32)
    logvar = rng.uniform(-12.0, 4.0, (N, nz)).astype(np.float32)
    logvar.reshape(-1)[::7] = 0.0
    eps = rng.standard_normal((N, nz)).astype(np.float32)
    wide = rng.standard_normal((N, Cc + 7)).astype(np.float32)           # cond = wide[:, 3:3 + Cc]: a row-strided view
    gz = rng.standard_normal((N, nz + Cc)).astype(np.float32)
    gz[:, nz:] *= BIG                                                    # would show in dmean / dlogvar if read
    return mean, logvar, eps, wide, gz


def _vae_ref(mean, logvar, eps, gz, gkl, T):
    """Forward and backward in precision T (float64: the reference; float32: the restatement of the element bar)."""
    mu, lv, ep = mean.astype(T), logvar.astype(T), eps.astype(T)
    N = mu.shape[0]
    sd = np.exp(T(0.5) * lv)
    z = mu + sd * ep
    terms = T(1) + lv - mu * mu - np.exp(lv)
    kl = (T(-0.5) / T(N)) * terms.sum(dtype=T)
    g = np.zeros_like(mu) if gz is None else gz.astype(T)
    c = T(0.0 if gkl is None else gkl) / T(N)
    dmean = g + c * mu
    dlogvar = T(0.5) * (g * sd * ep + c * (np.exp(lv) - T(1)))
    return z, kl, terms, dmean, dlogvar


@pytest.mark.parametrize("N,nz,Cc", VAE_SHAPES, ids=["%dx%d+%d" % s for s in VAE_SHAPES])
def test_vae_sample_kl_matches_float64(N, nz, Cc, dev):
    """Measured on an MI355X: largest ratio to the float32 restatement 1.44 (dlogvar, where the kernel squares exp(0.5 logvar)
    instead of evaluating exp(logvar)); kl within 1.5e-07 of sum |terms| at every shape."""
    from cape_amd import ops
    tag = "vae[%dx%d+%d]" % (N, nz, Cc)
    mean, logvar, eps, wide, gz = _vae_inputs(N, nz, Cc, 100 + N + nz + Cc)
    t = lambda a: torch.from_numpy(a).to(dev)
    dmean_t, dlv_t = t(mean).requires_grad_(True), t(logvar).requires_grad_(True)
    dwide = t(wide).requires_grad_(Cc > 0)
    cond = dwide[:, 3:3 + Cc] if Cc else None
    if Cc:
        assert cond.stride(0) == Cc + 7 and not (cond.is_contiguous() and N > 1)
    z, kl = ops.VaeSampleKLFn.apply(dmean_t, dlv_t, t(eps), cond)
    assert tuple(z.shape) == (N, nz + Cc) and kl.dim() == 0
    z64, kl64, terms, _, _ = _vae_ref(mean, logvar, eps, None, None, np.float64)
    z32, kl32, _, _, _ = _vae_ref(mean, logvar, eps, None, None, np.float32)
    zh = _host(z)
    element_bar(tag, "z", zh[:, :nz], z32, z64)
    if Cc:
        assert same_bits(zh[:, nz:], wide[:, 3:3 + Cc]), "the condition columns of [z | cond] are a copy"
    scale = (0.5 / N) * np.abs(terms).sum()
    sum_bar(tag, "kl", float(kl.detach().cpu()), kl64, scale, f32=float(kl32))

    gz_t, gkl_t = t(gz), torch.tensor(GKL, device=dev)
    ins = (dmean_t, dlv_t) + ((dwide,) if Cc else ())
    variants = {"both": ((z, kl), (gz_t, gkl_t), gz, GKL),
                "z_only": ((z,), (gz_t,), gz, None),
                "kl_only": ((kl,), (gkl_t,), None, GKL)}
    for name, (outs, gouts, gz_h, gkl_h) in variants.items():
        grads = torch.autograd.grad(outs, ins, gouts, retain_graph=True, allow_unused=True)
        _, _, _, dm64, dl64 = _vae_ref(mean, logvar, eps, None if gz_h is None else gz_h[:, :nz], gkl_h, np.float64)
        _, _, _, dm32, dl32 = _vae_ref(mean, logvar, eps, None if gz_h is None else gz_h[:, :nz], gkl_h, np.float32)
        element_bar(tag, "dmean[%s]" % name, _host(grads[0]), dm32, dm64)
        element_bar(tag, "dlogvar[%s]" % name, _host(grads[1]), dl32, dl64)
        if Cc:
            want = np.zeros_like(wide)
            if gz_h is not None:
                want[:, 3:3 + Cc] = gz_h[:, nz:]
            got = np.zeros_like(wide) if grads[2] is None else _host(grads[2])
            assert same_bits(got, want), "the condition's gradient is gz[:, nz:] (%s)" % name


@pytest.mark.parametrize("N,nz,Cc", VAE_SHAPES, ids=["%dx%d+%d" % s for s in VAE_SHAPES])
def test_vae_backward_with_missing_and_strided_gradients(N, nz, Cc, dev):
    """The backward exactly as autograd calls it when an output got no gradient (``gz is None`` / ``gkl is None``: the NULL
    branches of the kernel) and with gz a row-strided view of a wider buffer (its other columns hold values that would
    show), twice each: same bits."""
    from cape_amd import ops
    tag = "vae_bwd[%dx%d+%d]" % (N, nz, Cc)
    mean, logvar, eps, _, gz = _vae_inputs(N, nz, Cc, 200 + N + nz + Cc)
    t = lambda a: torch.from_numpy(a).to(dev)
    ctx = types.SimpleNamespace(saved_tensors=(t(mean), t(logvar), t(eps)), Cc=Cc)
    widebuf = torch.full((N, nz + Cc + 9), BIG, device=dev)
    widebuf[:, 5:5 + nz + Cc] = t(gz)
    strided = widebuf[:, 5:5 + nz + Cc]
    gkl_t = torch.tensor(GKL, device=dev)
    for name, gz_t, gk in (("gz_none", None, gkl_t), ("gkl_none", t(gz), None), ("gkl_none_strided", strided, None),
                           ("both_strided", strided, gkl_t)):
        runs = [ops.VaeSampleKLFn.backward(ctx, gz_t, gk) for _ in range(2)]
        dm, dl, none, dcond = runs[0]
        assert none is None
        gz_h = None if gz_t is None else gz[:, :nz]
        gkl_h = None if gk is None else GKL
        _, _, _, dm64, dl64 = _vae_ref(mean, logvar, eps, gz_h, gkl_h, np.float64)
        _, _, _, dm32, dl32 = _vae_ref(mean, logvar, eps, gz_h, gkl_h, np.float32)
        element_bar(tag, "dmean[%s]" % name, _host(dm), dm32, dm64)
        element_bar(tag, "dlogvar[%s]" % name, _host(dl), dl32, dl64)
        if Cc and gz_t is not None:
            assert same_bits(_host(dcond), gz[:, nz:])
        else:
            assert dcond is None
        assert same_bits(_host(runs[1][0]), _host(dm)) and same_bits(_host(runs[1][1]), _host(dl))
    assert float(widebuf[:, :5].min().cpu()) == BIG and float(widebuf[:, 5 + nz + Cc:].min().cpu()) == BIG


# ---------------------------------------------------------------------------------------------- condition networks
# (N, in1, hid, out1, in2, out2) -> seed of the inputs, chosen on the CPU so that no pre-activation of the hidden layer is within
# rounding of 0 (asserted below): the backward takes leaky' from the sign of the DEVICE's h, and float32 and float64 can
# disagree on that sign only there
CONDNET_SHAPES = {
    (2, 126, 63, 32, 4, 8): 0,
    (16, 126, 63, 32, 4, 8): 1,
    (64, 126, 63, 32, 4, 8): 4,
    (64, 126, 126, 64, 4, 16): 0,               # 52.7 KB of the 60 KB LDS limit of the backward
    (37, 72, 36, 18, 4, 3): 0,
    (1, 512, 256, 96, 7, 5): 0,                 # both static limits of the forward
    (33, 9, 5, 130, 1, 70): 0,                  # 10 rows of gW1 for 16 workgroups; the split at column 130 of 200; in2 = 1
    (5, 200, 100, 250, 3, 2): 0,
    (16, 126, 63, 24, 4, 8): 1,                 # the shipped nz18_pose24_clotype8 configurations at benchmark batch sizes
    (32, 126, 63, 24, 4, 8): 1,
    (32, 126, 63, 32, 4, 32): 1,                # the shipped nz64_pose32_clotype32 configurations
    (64, 126, 63, 32, 4, 32): 4,
}
PARAMS = ("W1", "b1", "W2", "b2", "Wc", "bc")
SENT = -7.0e8


def _condnet_inputs(shape, seed):
    N, in1, hid, out1, in2, out2 = shape
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)
    d = dict(c1=f(rng.standard_normal((N, in1))), c2=f(rng.standard_normal((N, in2))),
             W1=f(rng.standard_normal((in1, hid)) / np.sqrt(in1)), b1=f(0.1 * rng.standard_normal(hid)),
             W2=f(rng.standard_normal((hid, out1)) / np.sqrt(hid)), b2=f(0.1 * rng.standard_normal(out1)),
             Wc=f(rng.standard_normal((in2, out2)) / np.sqrt(in2)), bc=f(0.1 * rng.standard_normal(out2)))
    d["dy"] = f(rng.standard_normal((N, out1 + out2)))
    d["dy_b"] = f(rng.standard_normal((N, out1 + out2)))
    return d


def _mm(a, b, T):
    """a @ b in precision T.  float32: accumulated IN INDEX ORDER, one rounding per product and per addition -- the formula's
    own op order, and the same figure on every host (numpy's float32 matmul is whatever order the BLAS it was built with
    prefers: blocked and vectorised, so neither the formula's order nor the same from one CPU to the next)."""
    if T is np.float64:
        return a @ b
    acc = np.zeros((a.shape[0], b.shape[1]), T)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * b[None, k, :]
    return acc


def _condnet_fwd(d, T):
    c = {k: v.astype(T) for k, v in d.items()}
    pre = _mm(c["c1"], c["W1"], T) + c["b1"]
    h = np.where(pre > 0, pre, T(0.2) * pre)
    ycat = np.concatenate([_mm(h, c["W2"], T) + c["b2"], _mm(c["c2"], c["Wc"], T) + c["bc"]], axis=1)
    return pre, h, ycat


def _condnet_bwd(d, dsum, T):
    c = {k: v.astype(T) for k, v in d.items()}
    pre, h, _ = _condnet_fwd(d, T)
    out1 = c["W2"].shape[1]
    d1, d2 = np.ascontiguousarray(dsum.astype(T)[:, :out1]), np.ascontiguousarray(dsum.astype(T)[:, out1:])
    dh = _mm(d1, c["W2"].T, T) * np.where(pre > 0, T(1), T(0.2))
    ones = np.ones((1, dh.shape[0]), T)
    return dict(W1=_mm(c["c1"].T, dh, T), b1=_mm(ones, dh, T)[0], W2=_mm(h.T, d1, T), b2=_mm(ones, d1, T)[0],
                Wc=_mm(c["c2"].T, d2, T), bc=_mm(ones, d2, T)[0])


def _no_kink(d):
    pre = np.abs(_condnet_fwd(d, np.float64)[0])
    return pre.min() >= 1e-5 * pre.max()


def _in_wide(a, dev, left=3, right=6, fill=SENT):
    """``a`` as a row-strided view of a wider device tensor whose other columns hold ``fill``."""
    buf = torch.full((a.shape[0], a.shape[1] + left + right), fill, device=dev)
    buf[:, left:left + a.shape[1]] = torch.from_numpy(a).to(dev)
    return buf[:, left:left + a.shape[1]]


def _gbuf_views(shapes, dev):
    """Six views into one flat buffer with a sentinel block between them; returns (flat, views, mask of the sentinels)."""
    gap, offs, pos = 12, [], 8
    for s in shapes:
        offs.append(pos)
        pos += int(np.prod(s)) + gap
    flat = torch.full((pos,), SENT, device=dev)
    keep = np.ones(pos, bool)
    views = []
    for s, o in zip(shapes, offs):
        views.append(flat[o:o + int(np.prod(s))].view(s))
        keep[o:o + int(np.prod(s))] = False
    return flat, views, keep


# (copies, gradient into the first output, into the second, second row-strided, bucket views, row-strided c1 / c2)
CONDNET_VARIANTS = {
    "one_copy": (1, True, False, False, False, False),
    "one_copy_views_strided_in": (1, True, False, False, True, True),
    "two_both": (2, True, True, False, True, False),
    "two_both_strided": (2, True, True, True, False, False),
    "two_first_only": (2, True, False, False, False, True),
    "two_second_only": (2, False, True, False, True, False),
    "two_second_only_strided": (2, False, True, True, True, False),
}


@pytest.mark.parametrize("shape", list(CONDNET_SHAPES), ids=["x".join(map(str, s)) for s in CONDNET_SHAPES])
def test_condnets_match_float64(shape, dev):
    """Measured on an MI355X: largest ratio to the float32 restatement 1.98 (gb1 at 32x126x63x32x4x32); h, ycat and the
    gradients of the shipped sizes stay below 2.  The kernel's hidden-layer gradient is ONE fused-multiply-add chain over
    out1: at out1 = 96 / 250 (no shipped configuration) its error is 3.9e-07 / 4.4e-07 of the largest gW1 -- the very
    figure of the index-order float32 restatement (_mm), 4.3 / 4.0 times what numpy's blocked BLAS matmul leaves."""
    from cape_amd import ops
    N, in1, hid, out1, in2, out2 = shape
    oc = out1 + out2
    assert 4 * N * (hid + oc) <= 60 * 1024
    d = _condnet_inputs(shape, CONDNET_SHAPES[shape])
    assert _no_kink(d), "the seed of this shape leaves a hidden pre-activation within rounding of 0"
    tag = "condnets[%s]" % "x".join(map(str, shape))
    t = lambda a: torch.from_numpy(a).to(dev)
    _, h64, y64 = _condnet_fwd(d, np.float64)
    _, h32, y32 = _condnet_fwd(d, np.float32)
    for vname, (copies, g1, g2, strided2, views, strided_in) in CONDNET_VARIANTS.items():
        P = [t(d[k]).requires_grad_(True) for k in PARAMS]
        c1 = _in_wide(d["c1"], dev, fill=1.0e9) if strided_in else t(d["c1"])
        c2 = _in_wide(d["c2"], dev, fill=1.0e9) if strided_in else t(d["c2"])
        flat = keep = None
        gbufs = None
        if views:
            flat, gbufs, keep = _gbuf_views([d[k].shape for k in PARAMS], dev)
        res = ops.CondNetsFn.apply(c1, c2, *P, gbufs, copies)
        ycat, ycat_b = res if copies == 2 else (res, None)
        yh = _host(ycat)
        element_bar(tag, "ycat[%s]" % vname, yh, y32, y64)
        if copies == 2:
            assert same_bits(_host(ycat_b), yh), "the second copy holds the same values"
        # h is the kernel's saved hidden layer: the last tensor of its shape that the node kept for its backward
        saved = [s for s in ycat.grad_fn.saved_tensors if tuple(s.shape) == (N, hid)]
        hh = _host(saved[-1])
        element_bar(tag, "h[%s]" % vname, hh, h32, h64)
        assert np.array_equal(hh > 0, h64 > 0), "sign of the hidden layer"
        outs, gouts, dsum = [], [], np.zeros((N, oc), np.float64)
        if g1:
            outs.append(ycat)
            gouts.append(t(d["dy"]))
            dsum += d["dy"]
        if g2:
            outs.append(ycat_b)
            gouts.append(_in_wide(d["dy_b"], dev, left=64, right=5) if strided2 else t(d["dy_b"]))
            if strided2:
                assert gouts[-1].stride(0) == oc + 69 and gouts[-1].stride(1) == 1
            dsum += d["dy_b"]
        g64 = _condnet_bwd(d, dsum, np.float64)
        g32 = _condnet_bwd(d, dsum.astype(np.float32), np.float32)
        first = None
        for rep in range(2):
            grads = torch.autograd.grad(outs, P, gouts, retain_graph=True)
            got = [_host(g).copy() for g in grads]
            if views:
                fh = _host(flat)
                assert (fh[keep] == np.float32(SENT)).all(), "a gradient was written outside its bucket view"
                for k, v, g in zip(PARAMS, gbufs, got):
                    assert same_bits(_host(v), g), "gradient %s did not land in its bucket view" % k
            if rep == 0:
                first = got
                for k, g in zip(PARAMS, got):
                    element_bar(tag, "g%s[%s]" % (k, vname), g, g32[k], g64[k])
                if views:
                    flat.fill_(SENT)                 # the second run must write everything again (written, not accumulated)
            else:
                for k, a, b in zip(PARAMS, first, got):
                    assert same_bits(a, b), "gradient %s differs between two runs of the same backward" % k


def test_condnets_reject_bad_arguments(dev):
    """Host-side checks of csrc/condnet.hip (condnet_check and the entry points): refused before any launch."""
    from cape_amd import ops

    def forward(shape):
        d = _condnet_inputs(shape, 0)
        args = [torch.from_numpy(d[k]).to(dev) for k in ("c1", "c2") + PARAMS]
        return ops.CondNetsFn.apply(*args, None, 1)

    for shape in ((65, 16, 8, 8, 4, 4),          # N > 64
                  (2, 16, 257, 8, 4, 4),         # hid > 256
                  (2, 513, 8, 8, 4, 4),          # in1 > 512
                  (64, 126, 200, 64, 4, 16)):    # 4 * 64 * 280 bytes of LDS: over the 60 KB of the backward
        with pytest.raises(RuntimeError):
            forward(shape)
    forward((64, 126, 126, 64, 4, 16))           # (just inside: accepted)

    # lddy < out1 + out2: the autograd wrapper never forms such a call (it copies such a gradient), so the entry point itself
    shape = (4, 16, 8, 8, 4, 4)
    N, in1, hid, out1, in2, out2 = shape
    d = _condnet_inputs(shape, 0)
    T = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    h = torch.zeros((N, hid), device=dev)
    outs = [torch.full(d[k].shape, SENT, device=dev) for k in PARAMS]
    call = lambda dy, lddy, dy2, lddy2: ops.lib.cape_condnet_bwd(
        ops._ptr(T["c1"]), in1, ops._ptr(T["c2"]), in2, ops._ptr(T["W2"]), ops._ptr(h), ops._ptr(dy), lddy, ops._ptr(dy2), lddy2,
        *[ops._ptr(o) for o in outs], N, in1, hid, out1, in2, out2, ops._stream())
    oc = out1 + out2
    assert call(T["dy"], oc - 1, None, 0) != 0
    assert call(T["dy"], oc, T["dy_b"], oc - 1) != 0
    assert call(None, 0, None, 0) != 0
    torch.cuda.synchronize()
    assert all(float(o.max().cpu()) == SENT and float(o.min().cpu()) == SENT for o in outs)      # nothing was launched
    assert call(T["dy"], oc, T["dy_b"], oc) == 0

    # both gradients None: backward returns None for every input
    ctx = types.SimpleNamespace(saved_tensors=(T["c1"], T["c2"], T["W2"], h), dims=shape, gbufs=None,
                                shapes=[d[k].shape for k in PARAMS])
    assert ops.CondNetsFn.backward(ctx, None, None) == (None,) * 10
