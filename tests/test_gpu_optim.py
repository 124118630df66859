"""The optimiser kernels of every training step (csrc/optim.hip: ``gradnorm_partial_kernel`` + ``flat_final_kernel``,
``momentum_update_kernel``, ``sumsq_ranges_partial_kernel``) against the formula of include/cape_hip.h in float64

    ge = grad_scale * g;  ge[b:e] += coef * w[b:e] for every regularised range
    sumsq = sum(ge^2);  s = clip / max(sqrt(sumsq), clip)           (tf.clip_by_global_norm, reference lib/models.py:461)
    m = momentum * m + s * ge;  w = w + neg_lr * m                  (tf.train.MomentumOptimizer, non-Nesterov, :448-456)

on their own: several consecutive steps FROM A NON-ZERO m (the whole-model test takes one step from m = 0, where a kernel
that drops, misplaces or doubles ``momentum * m`` passes), grad_scale != 1, every layout of the regularised ranges, and bucket
sizes on both sides of the launch geometry (one float4; a second grid-stride trip of the norm kernel with a ragged tail;
the 4096-block cap of the update launch).  The reference is plain numpy, written here; nothing of cape_amd computes it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MOMENTUM, CLIP, COEF, LR = 0.9, 5.0, 0.25, 3e-3
MOMF = float(np.float32(MOMENTUM))          # the kernel receives float32 scalars: the reference uses the same rounded constants
NLRF = float(np.float32(-LR))
SENT = 1.0e9                                 # fills the buffers behind the buckets: must be neither read nor written
TAIL = 64

N_ONE = 4                                    # one float4
N_MID = 1 << 17                              # the size of tests/test_gpu_adam.py: one trip, below every cap
N_TRIP2 = 4 * (1024 * 256 + 37)              # norm kernel: a second grid-stride trip of 37 float4 (n/4 not a multiple of 256)
N_CAP = 4 * (4096 * 256 + 201475)            # update kernel: past the 4096-block cap, ragged second trip (5 000 204 floats)
assert (N_TRIP2 // 4) % 256 and (N_CAP // 4) % 256 and N_CAP > 4096 * 256 * 4


def _q(v):
    return int(v) // 4 * 4


def _layout(name, n):
    """Regularised [begin, end) ranges (multiples of 4) of a bucket of n floats."""
    if name == "none":
        return []
    if n == 4:
        return [(0, 4)]                      # the only range a single float4 admits: starts at 0 and ends at n
    if name == "inside2":
        return [(_q(0.1 * n) + 4, _q(0.3 * n)), (_q(0.5 * n), _q(0.8 * n) - 4)]
    if name == "start0":
        return [(0, _q(0.4 * n))]
    if name == "endn":
        return [(_q(0.6 * n), n)]
    if name == "max8":
        return [(_q(n * (2 * k + 0.5) / 16), _q(n * (2 * k + 1.5) / 16)) for k in range(8)]
    raise KeyError(name)


class _Bucket(object):
    """A float32 bucket ``buf[:n]`` of a larger device buffer whose tail holds a sentinel."""

    def __init__(self, values, dev):
        self.n = len(values)
        host = np.full(self.n + TAIL, SENT, np.float32)
        host[:self.n] = values
        self.buf = torch.from_numpy(host).to(dev)
        self.t = self.buf[:self.n]
        assert self.t.data_ptr() % 16 == 0

    def set(self, values):
        self.t.copy_(torch.from_numpy(np.asarray(values, np.float32)))

    def f64(self):
        return self.t.cpu().numpy().astype(np.float64)

    def tail_untouched(self):
        return bool((self.buf[self.n:].cpu().numpy().view(np.int32) == np.float32(SENT).view(np.int32)).all())


def _effective(g64, w64, ranges, coef, gs):
    ge = gs * g64
    for b, e in ranges:
        ge[b:e] += coef * w64[b:e]
    return ge


def _scale_to_norm(g, w64, ranges, coef, gs, target):
    """a > 0 with || gs * a * g + reg || = target (reg does not scale with the gradient): root of the quadratic."""
    G = gs * g
    R = np.zeros_like(G)
    for b, e in ranges:
        R[b:e] = coef * w64[b:e]
    GG, GR, RR = float(G @ G), float(G @ R), float(R @ R)
    assert RR < target * target, "the regulariser alone exceeds the target norm: the test's own scaling is off"
    return (-GR + np.sqrt(GR * GR - GG * (RR - target * target))) / GG


# norm of the effective gradient per step, in units of the clip threshold
REGIMES = {
    "clipped": [3.0, 1.7, 6.0, 2.2, 4.1],
    "unclipped": [0.3, 0.6, 0.15, 0.45, 0.8],
    "edge": [2.0, 1.0 + 5e-4, 1.0 - 5e-4, 0.5, 1.0 + 2e-4, 1.0 - 2e-4],     # within 1e-3 of clip, on either side
}

CASES = []
for _li, _lay in enumerate(["none", "inside2", "start0", "endn", "max8"]):
    for _ri, _reg in enumerate(["clipped", "unclipped", "edge"]):
        CASES.append((N_MID, _lay, _reg, [1.0, 0.5, 0.125][(_li + _ri) % 3]))
CASES += [(N_ONE, "none", "clipped", 1.0), (N_ONE, "start0", "unclipped", 0.5), (N_ONE, "endn", "edge", 0.125),
          (N_TRIP2, "inside2", "clipped", 0.5), (N_TRIP2, "endn", "unclipped", 1.0), (N_TRIP2, "max8", "edge", 0.125),
          (N_TRIP2, "none", "edge", 1.0),
          (N_CAP, "max8", "clipped", 0.125), (N_CAP, "endn", "edge", 0.5), (N_CAP, "inside2", "unclipped", 1.0),
          (N_CAP, "start0", "clipped", 1.0)]


def _case_id(c):
    return "n%d-%s-%s-gs%g" % c


def _setup(n, layout, dev, seed):
    rng = np.random.default_rng(seed)
    ranges = _layout(layout, n)
    # || coef * w || <= ~1 over the whole bucket: the regulariser is a visible part of every norm used below without exceeding it
    w = _Bucket(rng.standard_normal(n) / (COEF * np.sqrt(n)) * (0.5 if n == 4 else 1.0), dev)
    m = _Bucket(rng.standard_normal(n) * 3.0 / np.sqrt(n), dev)          # NON-ZERO momentum: the term under test
    g = _Bucket(np.zeros(n), dev)
    return rng, ranges, w, m, g


@pytest.mark.parametrize("n,layout,regime,gs", CASES, ids=[_case_id(c) for c in CASES])
def test_momentum_kernel_matches_tf_formula(n, layout, regime, gs):
    """Measured on an MI355X over all cases: sumsq within 1.2e-07 (relative), m within 1.2e-07 of max |m|, w within the bar
    below: at most 2.1e-05 of the update, reached where the update is a few thousandths of max |w| (the unclipped cases), so
    that the one rounding of w itself (6e-08 |w|) is what is seen."""
    from cape_amd import ops
    dev = torch.device("cuda:0")
    rng, ranges, w, m, g = _setup(n, layout, dev, 11)
    sumsq = torch.zeros((), device=dev)
    neg_lr = torch.full((), -LR, device=dev)
    ws = ops.flat_workspace(dev)
    w64, m64 = w.f64(), m.f64()
    assert np.abs(m64).max() > 0
    worst_w = worst_m = worst_s = 0.0
    for step, rel_norm in enumerate(REGIMES[regime], 1):
        raw = rng.standard_normal(n)
        raw[::97] = 0.0
        raw *= _scale_to_norm(raw, w64, ranges, COEF, gs, rel_norm * CLIP)
        g.set(raw)
        g64 = g.f64()
        ops.flat_gradnorm(g.t, w.t, ranges, COEF, sumsq, ws, grad_scale=gs)
        ops.flat_momentum_update(w.t, g.t, m.t, MOMENTUM, CLIP, sumsq, neg_lr, ranges, COEF, grad_scale=gs)
        # float64 reference of this step, from the device's fp32 state before it
        ge = _effective(g64, w64, ranges, COEF, gs)
        ss_ref = float((ge * ge).sum())
        norm = np.sqrt(ss_ref)
        assert abs(norm / CLIP - rel_norm) < 1e-5 * rel_norm, (norm, rel_norm)      # the regime is what the case says it is
        m_ref = MOMF * m64 + (CLIP / max(norm, CLIP)) * ge
        w_ref = w64 + NLRF * m_ref
        ss_dev, w_dev, m_dev = float(sumsq.cpu()), w.f64(), m.f64()
        upd = np.abs(w_ref - w64).max()
        err_s = abs(ss_dev - ss_ref) / ss_ref
        err_w, err_m = np.abs(w_dev - w_ref).max(), np.abs(m_dev - m_ref).max()
        print("momentum %s step %d: sumsq rel err %.2e, |dw| / update %.2e, |dm| / max|m| %.2e" %
              (_case_id((n, layout, regime, gs)), step, err_s, err_w / upd, err_m / np.abs(m_ref).max()))
        assert err_s <= 2e-6, (step, ss_dev, ss_ref)
        # the device holds w and m in fp32: one rounding of w (6e-8 |w|) plus the update's own fp32 evaluation (1e-5 of it)
        assert upd > 0 and err_w <= 1e-5 * upd + 1.2e-7 * np.abs(w_ref).max(), (step, err_w, upd)
        assert err_m <= 2e-6 * np.abs(m_ref).max(), (step, err_m, np.abs(m_ref).max())
        assert w.tail_untouched() and m.tail_untouched() and g.tail_untouched(), step
        worst_s, worst_w, worst_m = max(worst_s, err_s), max(worst_w, err_w / upd), max(worst_m, err_m / np.abs(m_ref).max())
        w64, m64 = w_dev, m_dev                                 # follow the device's fp32 state (no drift accumulation)
    assert len(REGIMES[regime]) >= 5
    print("momentum %s: worst sumsq %.2e, w / update %.2e, m %.2e" % (_case_id((n, layout, regime, gs)), worst_s, worst_w, worst_m))


@pytest.mark.parametrize("n,layout", [(N_TRIP2, "inside2"), (N_CAP, "max8"), (N_MID, "none")],
                         ids=["trip2", "capped", "mid"])
def test_momentum_step_is_deterministic(n, layout):
    """The header promises fixed-order sums: the same step from the same state leaves the same bits."""
    from cape_amd import ops
    dev = torch.device("cuda:0")
    rng, ranges, w, m, g = _setup(n, layout, dev, 5)
    g.set(rng.standard_normal(n) * 4.0 * CLIP / np.sqrt(n))
    w0, m0 = w.buf.clone(), m.buf.clone()
    neg_lr = torch.full((), -LR, device=dev)
    ws = ops.flat_workspace(dev)
    got = []
    for _ in range(2):
        w.buf.copy_(w0)
        m.buf.copy_(m0)
        sumsq = torch.zeros((), device=dev)
        ops.flat_gradnorm(g.t, w.t, ranges, COEF, sumsq, ws, grad_scale=0.5)
        ops.flat_momentum_update(w.t, g.t, m.t, MOMENTUM, CLIP, sumsq, neg_lr, ranges, COEF, grad_scale=0.5)
        got.append([t.cpu().numpy().view(np.int32).copy() for t in (w.buf, m.buf, sumsq.reshape(1))])
    assert not np.array_equal(got[0][0], w0.cpu().numpy().view(np.int32))           # (the step did something)
    for a, b in zip(*got):
        assert np.array_equal(a, b)


SUM_CASES = [(n, lay) for n in (N_ONE, N_MID, N_TRIP2, N_CAP) for lay in ("none", "inside2", "start0", "endn", "max8")
             if not (n == N_ONE and lay in ("inside2", "max8", "endn"))]


@pytest.mark.parametrize("n,layout", SUM_CASES, ids=["n%d-%s" % c for c in SUM_CASES])
def test_gradnorm_and_sumsq_ranges(n, layout):
    """The two fixed-order sums on inputs spanning ~12 binades, per bucket size and range layout, against float64: relative
    error <= 2e-6 (all terms are non-negative, so sum |terms| is the sum itself)."""
    from cape_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(17)
    ranges = _layout(layout, n)
    spread = lambda: rng.standard_normal(n) * np.exp2(rng.uniform(-6.0, 6.0, n))
    g, w = _Bucket(spread(), dev), _Bucket(spread(), dev)
    g64, w64 = g.f64(), w.f64()
    ws = ops.flat_workspace(dev)
    gs, scale = 0.5, 0.37
    out = torch.full((), -1.0, device=dev)
    ops.flat_gradnorm(g.t, w.t, ranges, COEF, out, ws, grad_scale=gs)
    ge = _effective(g64, w64, ranges, COEF, gs)
    ref = float((ge * ge).sum())
    f32 = float(np.sum(ge.astype(np.float32) ** 2, dtype=np.float32))
    err = abs(float(out.cpu()) - ref) / ref
    print("flat_gradnorm n=%d %s: |err| / sum|terms| = %.2e (np.sum float32: %.2e)" % (n, layout, err, abs(f32 - ref) / ref))
    assert err <= 2e-6, (float(out.cpu()), ref)
    # sumsq_ranges needs at least one range: the whole bucket where the layout has none
    rr = ranges or [(0, n)]
    got = float(ops.sumsq_ranges(g.t, rr, scale, ws).cpu())
    terms = np.concatenate([g64[b:e] ** 2 for b, e in rr])
    ref = float(np.float32(scale)) * float(terms.sum())
    f32 = float(np.float32(scale) * np.sum(terms.astype(np.float32), dtype=np.float32))
    err = abs(got - ref) / ref
    print("sumsq_ranges n=%d %s: |err| / sum|terms| = %.2e (np.sum float32: %.2e)" % (n, layout, err, abs(f32 - ref) / ref))
    assert err <= 2e-6, (got, ref)
    assert g.tail_untouched() and w.tail_untouched()


@pytest.mark.parametrize("n", [N_ONE, N_MID, N_TRIP2], ids=lambda n: "n%d" % n)
def test_sums_of_an_all_zero_bucket_are_exactly_zero(n):
    from cape_amd import ops
    dev = torch.device("cuda:0")
    g, w = _Bucket(np.zeros(n), dev), _Bucket(np.zeros(n), dev)
    ws = ops.flat_workspace(dev)
    ws.fill_(7.0)                                                # stale partials of an earlier call must not leak in
    out = torch.full((), -1.0, device=dev)
    ops.flat_gradnorm(g.t, w.t, [(0, n)], COEF, out, ws, grad_scale=0.5)
    assert float(out.cpu()) == 0.0
    ws.fill_(7.0)
    assert float(ops.sumsq_ranges(g.t, [(0, n)], 3.0, ws).cpu()) == 0.0


def test_sumsq_over_ranges_of_total_length_four():
    from cape_amd import ops
    dev = torch.device("cuda:0")
    n = N_TRIP2
    rng = np.random.default_rng(23)
    x = _Bucket(rng.standard_normal(n), dev)
    x64 = x.f64()
    ws = ops.flat_workspace(dev)
    for rr in ([(8, 12)], [(4, 4), (n - 4, n)], [(0, 4)], [(0, 0)] * 7 + [(1024 * 256 * 4, 1024 * 256 * 4 + 4)]):
        got = float(ops.sumsq_ranges(x.t, rr, 0.5, ws).cpu())
        ref = 0.5 * sum(float((x64[b:e] ** 2).sum()) for b, e in rr)
        assert abs(got - ref) <= 2e-6 * ref, (rr, got, ref)


def test_momentum_kernel_rejects_bad_arguments():
    """Refused by the host-side checks before any launch (every pointer handed over is a valid device pointer)."""
    from cape_amd import ops
    dev = torch.device("cuda:0")
    z = torch.zeros(128, device=dev)
    a = z[:64]
    s = torch.ones((), device=dev)
    nlr = torch.full((), -LR, device=dev)
    ws = ops.flat_workspace(dev)
    upd = lambda w, g, m, clip=CLIP, ranges=(), gs=1.0: ops.flat_momentum_update(w, g, m, MOMENTUM, clip, s, nlr, list(ranges), COEF, grad_scale=gs)
    nrm = lambda g, w, ranges=(), gs=1.0: ops.flat_gradnorm(g, w, list(ranges), COEF, s, ws, grad_scale=gs)
    mis = z[1:65]                                               # 64 floats, 4 bytes off a 16-byte boundary
    assert mis.numel() == 64 and mis.data_ptr() % 16 == 4
    nine = [(8 * k, 8 * k + 4) for k in range(9)]
    bad = [lambda: upd(mis, a, a), lambda: upd(a, mis, a), lambda: upd(a, a, mis),
           lambda: nrm(mis, a), lambda: nrm(a, mis, [(0, 4)]),
           lambda: upd(z[:62], z[:62], z[:62]), lambda: nrm(z[:62], z[:62]),          # n % 4 != 0
           lambda: upd(a, a, a, clip=0.0), lambda: upd(a, a, a, clip=-1.0),
           lambda: upd(a, a, a, gs=0.0), lambda: upd(a, a, a, gs=-0.5), lambda: nrm(a, a, gs=0.0),
           lambda: upd(a, a, a, ranges=[(2, 8)]), lambda: upd(a, a, a, ranges=[(4, 10)]), lambda: nrm(a, a, [(2, 8)]),
           lambda: upd(a, a, a, ranges=[(8, 4)]),
           lambda: upd(a, a, a, ranges=nine), lambda: nrm(a, a, nine), lambda: ops.sumsq_ranges(a, nine, 1.0, ws),
           lambda: ops.sumsq_ranges(a, [], 1.0, ws), lambda: ops.sumsq_ranges(mis, [(0, 4)], 1.0, ws),
           lambda: ops.sumsq_ranges(a, [(2, 8)], 1.0, ws)]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail("bad argument set %d was accepted" % i)
    torch.cuda.synchronize()
    assert float(z.abs().max().cpu()) == 0.0 and float(s.cpu()) == 1.0               # nothing was launched
    upd(a, a, a, ranges=[(k * 8, k * 8 + 4) for k in range(8)])                       # the same calls, valid: accepted
    nrm(a, a, [(0, 64)])
