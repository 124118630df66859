"""The on-chip Chebyshev recurrence (csrc/cheb_fused.hip: cheb_fused_fwd_kernel, cheb_fused_dw_kernel, cheb_fused_dx_kernel,
cheb_fused_dw_reduce_kernel) on the small synthetic graphs of tests/cheb_synth.py: ELL rows of 0, 2 and exactly 12 entries and a
hub row, patches of 1 .. 2, 10, 63 .. 64, 255 .. 256 rows, patch + halo from 7 rows to all 1024 threads, a halo that is the whole
graph, two components, 4 / 6 / 96 patches, every order K = 2 .. 8 at Cin 8 and 16, batch sizes on both branches of the block map
and around the 32 groups of the weight-gradient reduction, padded views through the C entries, accumulate = 1, and every argument
the entries refuse.  Graphs the plan declines (rows of 14 entries, no plan that fits the LDS, fewer vertices than patches, an
asymmetric operator) must run the materialised form.

Every output is held to the dense float64 evaluation (cheb_synth.reference) with tests/kernel_bars.py: y and dx to element_bar
(4 x the float32 restatement oracle.torch_twin.chebyshev5 + autograd on the CPU, backstop 2e-5), dW to sum_bar (2e-6 of
sum |terms| per element).  Each test asserts from ops.LAUNCH_LOG which kernels ran.  No test launches a plan with an empty patch.

Measured on an MI355X when the module was written: the on-chip kernels' worst element_bar ratio 2.13 (y, K = 6, Cin = 16 on the
17 x 15 grid; bar 4) and worst sum_bar figure 2.6e-7 (bar 2e-6); the materialised form of the declined graphs 2.09 and 1.2e-6 (dW
on the 3-vertex ring, six terms per sum; the float32 numpy sum of the same terms is 1.2e-6 as well)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cheb_synth as S
from kernel_bars import element_bar, sum_bar, same_bits

pytestmark = pytest.mark.gpu
FOUT = S.FOUT
EINVAL, EWORKSPACE = -1, -4
FUSED = ["cheb_fused_fwd_kernel", "cheb_fused_dw_kernel + cheb_fused_dx_kernel"]
WORST = dict(element=0.0, sum=0.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield torch.device("cuda:0")
    print("\ntest_gpu_cheb_fused worst figures: element_bar ratio %.3f, sum_bar %.2e" % (WORST["element"], WORST["sum"]))


def _ops():
    from cape_amd import ops
    return ops


_DOPS = {}


def conv_ops(key, L, K, dev):
    """DeviceConvOps of the layer in its recurrence form (K <= 3 would otherwise get precomposed operators), built once."""
    if (key, K) not in _DOPS:
        import cape_amd.graph as G
        old = G.FUSE_MAX_K
        G.FUSE_MAX_K = 1
        try:
            host = G.ConvOperators(L, K)
        finally:
            G.FUSE_MAX_K = old
        assert not host.fused
        _DOPS[key, K] = _ops().DeviceConvOps(host, dev)
    return _DOPS[key, K]


def fused_plan(family, K, Cin, dev):
    """The device plan of an accepted case; its facts are the ones tests/test_cheb_synth_host.py asserts on the CPU."""
    dops = conv_ops(family, S.graph(family)[1], K, dev)
    plan = dops.patch_plan(Cin, FOUT)
    assert plan is not None, (family, K, Cin)
    facts = S.plan_facts(plan.host, K)
    for k, want in (S.expected_plan(family, K, Cin) or {}).items():
        assert facts[k] == want, (family, K, Cin, k, facts)
    assert (plan.host.pinfo[:, 3] >= 1).all()
    return dops, plan


def run_layer(dops, x, W, dy, dev):
    """ops.chebyshev5 forward + backward: (y, dx, dW) as float32 numpy and the names of the launches."""
    ops = _ops()
    hx = torch.tensor(x, dtype=torch.float32, device=dev, requires_grad=True)
    hW = torch.tensor(W, dtype=torch.float32, device=dev, requires_grad=True)
    hdy = torch.tensor(dy, dtype=torch.float32, device=dev)
    ops.LAUNCH_LOG = []
    try:
        hy = ops.chebyshev5(hx, hW, dops)
        hy.backward(hdy)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    return (hy.detach().cpu().numpy(), hx.grad.cpu().numpy(), hW.grad.cpu().numpy()), names


def ebar(tag, quantity, dev_, f32_, ref):
    r = element_bar(tag, quantity, dev_, f32_, ref)
    WORST["element"] = max(WORST["element"], r)
    print("%s / %s: element_bar ratio %.3f" % (tag, quantity, r))


def sbar(tag, quantity, dev_, ref, abs_terms, f32_=None):
    WORST["sum"] = max(WORST["sum"], sum_bar(tag, quantity, dev_, ref, abs_terms, f32=f32_))


def hold(tag, L, K, x, W, dy, got):
    """y, dx, dW of one layer against the float64 reference."""
    y64, dx64, dW64, dWabs = S.reference(L, K, x, W, dy)
    y32, dx32, dW32 = S.twin32(L, K, x, W, dy)
    ebar(tag, "y", got[0], y32, y64)
    ebar(tag, "dx", got[1], dx32, dx64)
    sbar(tag, "dW", got[2], dW64, dWabs, dW32)


# ---- families ----------------------------------------------------------------------------------------------------------------------
FAMILY_CASES = [(f, K, Cin, 2) for f, K in (("ring7", 6), ("ring40", 6), ("grid17x15", 6), ("grid17x15_isolated5", 6), ("grid33x31", 8),
                                            ("grid33x32", 6), ("ring300_hops6", 6), ("hub_grid", 6), ("grid10x10+ring37", 8))
                for Cin in (8, 16)]
FAMILY_CASES += [("matchings2_1024", 6, 8, 3), ("matchings3_1000", 4, 16, 3), ("matchings3_1000", 4, 8, 3)]


@pytest.mark.parametrize("family,K,Cin,N", FAMILY_CASES, ids=lambda v: str(v))
def test_families(family, K, Cin, N, dev):
    L = S.graph(family)[1]
    dops, plan = fused_plan(family, K, Cin, dev)
    x, W, dy = S.inputs(100 * K + Cin, N, L.shape[0], K, Cin)
    got, names = run_layer(dops, x, W, dy, dev)
    assert names == FUSED, names
    hold("families[%s,K%d,Cin%d,N%d,P%d,rmax%d]" % (family, K, Cin, N, plan.P, plan.rmax), L, K, x, W, dy, got)


# ---- orders ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", [8, 16])
@pytest.mark.parametrize("K", [2, 3, 4, 5, 6, 7, 8])
def test_orders(K, Cin, dev):
    """Every order on the 17 x 15 grid; the second weight set has only order K - 1: a halo short by one ring, or a recurrence that
    stops a step early, is then a full-scale error instead of one term in K."""
    family = "grid17x15"
    L = S.graph(family)[1]
    dops, plan = fused_plan(family, K, Cin, dev)
    for only in (None, K - 1):
        x, W, dy = S.inputs(1000 + 10 * K + Cin, 2, L.shape[0], K, Cin, only_order=only)
        got, names = run_layer(dops, x, W, dy, dev)
        assert names == FUSED, names
        assert only is None or np.abs(got[0]).max() > 0.1
        hold("orders[K%d,Cin%d,%s]" % (K, Cin, "all orders" if only is None else "order %d only" % only), L, K, x, W, dy, got)


# ---- block map and weight-gradient reduction -----------------------------------------------------------------------------------------
BATCHES = [1, 8, 9, 16, 25, 33]                      # x 4 patches: 4, 32, 36, 64, 100, 132 slabs -> 1, 1, 2, 2, 4, 5 slabs per group
_SINGLE = {}


def _single_runs(Cin, dev):
    """y and dx of every sample of the batch pool run alone (N = 1), once per Cin."""
    if Cin not in _SINGLE:
        K, family = 6, "ring40"
        dops, _ = fused_plan(family, K, Cin, dev)
        x, W, dy = S.inputs(4000 + Cin, max(BATCHES), 40, K, Cin)
        runs = [run_layer(dops, x[n:n + 1], W, dy[n:n + 1], dev)[0] for n in range(max(BATCHES))]
        _SINGLE[Cin] = (dops, x, W, dy, np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs]))
    return _SINGLE[Cin]


@pytest.mark.parametrize("Cin", [8, 16])
@pytest.mark.parametrize("N", BATCHES)
def test_batch_map_and_reduction(N, Cin, dev):
    """N = 1 and N % 8 == 0 against the plain branch of cape_map_block; N * P below, at and above the 32 groups of the first
    reduction stage, with a partial last group (36 = 18 x 2, 100 = 25 x 4, 132 = 26 x 5 + 2) and both loops of the reduction kernel
    (groups of 4 and 5 slabs).  A workgroup's arithmetic does not depend on N, and the reduction order is fixed."""
    K, L = 6, S.graph("ring40")[1]
    dops, x, W, dy, y1, dx1 = _single_runs(Cin, dev)
    nslab = 4 * N
    per = (nslab + 31) // 32
    assert (nslab, per) in ((4, 1), (32, 1), (36, 2), (64, 2), (100, 4), (132, 5))
    got, names = run_layer(dops, x[:N], W, dy[:N], dev)
    assert names == FUSED, names
    assert same_bits(got[0], y1[:N]) and same_bits(got[1], dx1[:N])
    again, _ = run_layer(dops, x[:N], W, dy[:N], dev)
    assert same_bits(again[2], got[2]) and same_bits(again[0], got[0]) and same_bits(again[1], got[1])
    hold("batch[N%d,Cin%d,slabs%d,per%d]" % (N, Cin, nslab, per), L, K, x[:N], W, dy[:N], got)


# ---- fallbacks ---------------------------------------------------------------------------------------------------------------------
FALLBACKS = [("ring300_hops7", 6, 16, 2), ("matchings2_1024", 6, 16, 3)] + [(f, 6, 16, 2) for f in S.TINY] + [("path3", 2, 8, 2), ("asymmetric_hub", 6, 16, 2)]


@pytest.mark.parametrize("family,K,Cin,N", FALLBACKS, ids=lambda v: str(v))
def test_fallbacks(family, K, Cin, N, dev):
    """Graphs the on-chip form declines: no plan, and the layer runs the materialised recurrence to the same bars."""
    L = S.row_normalised_laplacian(S.graph("hub_grid")[0]) if family == "asymmetric_hub" else S.graph(family)[1]
    dops = conv_ops(family, L, K, dev)
    assert _ops().lib.cape_cheb_fused_supported(Cin, FOUT, K) == 1
    assert dops.patch_plan(Cin, FOUT) is None
    x, W, dy = S.inputs(7000 + K + Cin, N, L.shape[0], K, Cin)
    got, names = run_layer(dops, x, W, dy, dev)
    assert names and not any("cheb_fused" in n for n in names), names
    hold("fallback[%s,K%d,Cin%d]" % (family, K, Cin), L, K, x, W, dy, got)


# ---- the C entries directly ----------------------------------------------------------------------------------------------------------
def _padded(a, pad_row, pad_sample, dev, fill=float("nan")):
    """Device view [N, M, C] of ``a`` (None: nothing is copied) in a buffer of row length C + pad_row and sample stride
    M * (C + pad_row) + pad_sample, all padding = ``fill``.  Returns (view, buffer, bool mask of the payload)."""
    N, M, Cn = a if isinstance(a, tuple) else a.shape
    ld = Cn + pad_row
    buf = torch.full((N, M * ld + pad_sample), fill, device=dev, dtype=torch.float32)
    v = buf[:, :M * ld].view(N, M, ld)[:, :, :Cn]
    if not isinstance(a, tuple):
        v.copy_(torch.tensor(a, dtype=torch.float32))
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask[:, :M * ld].view(N, M, ld)[:, :, :Cn] = True
    return v, buf, mask


def _untouched(buf, mask):
    return bool(torch.isnan(buf[~mask]).all())


class Abi(object):
    """One valid argument set of cape_cheb_fused_fwd / _bwd on the 17 x 15 grid; ``call`` overrides single arguments."""

    def __init__(self, dev, K=5, Cin=16, N=2):
        ops = _ops()
        self.ops, self.dev, self.K, self.Cin, self.N = ops, dev, K, Cin, N
        self.L = S.graph("grid17x15")[1]
        self.M = M = self.L.shape[0]
        _, self.plan = fused_plan("grid17x15", K, Cin, dev)
        self.x, self.W, self.dy = S.inputs(9000 + K, N, M, K, Cin)
        self.hx = _padded(self.x, 4, 16, dev)[0]                     # ldx = Cin + 4, sample stride padded by 16 floats, NaN padding
        self.hdy = _padded(self.dy, 4, 0, dev)[0]                    # lddy = Fout + 4
        self.hW = torch.tensor(self.W, dtype=torch.float32, device=dev)
        self.need = int(ops.lib.cape_cheb_fused_bwd_workspace_bytes(N, Cin, FOUT, K, self.plan.P))
        assert self.need == (N * self.plan.P + 32) * K * Cin * FOUT * 4
        self.ws = torch.empty(self.need // 4 + 4, device=dev)

    def _plan_args(self, kw):
        p, ptr = self.plan, self.ops._ptr
        return (kw.get("P", p.P), ptr(p.pinfo), ptr(p.vid), ptr(p.ell_col), ptr(p.ell_val), kw.get("rmax", p.rmax))

    @staticmethod
    def _view(v, kw, name):
        p, ss, ld = _ops()._v(v)
        return C.c_void_p(p.value + kw.get(name + "_off", 0)), kw.get(name + "_ss", ss), kw.get("ld" + name, ld)

    def fwd(self, y, **kw):
        ops = self.ops
        xa, ya = self._view(self.hx, kw, "x"), self._view(y, kw, "y")
        return ops.lib.cape_cheb_fused_fwd(*xa, ops._ptr(self.hW), *ya, self.N, self.M, kw.get("Cin", self.Cin), kw.get("Fout", FOUT),
                                           kw.get("K", self.K), *self._plan_args(kw), ops._stream())

    def bwd(self, dx, dW, accumulate=0, **kw):
        ops = self.ops
        xa, ga = self._view(self.hx, kw, "x"), self._view(self.hdy, kw, "dy")
        da = self._view(dx, kw, "dx") if dx is not None else (None, 0, 0)
        Wp = C.c_void_p(self.hW.data_ptr() + kw.get("W_off", 0))
        return ops.lib.cape_cheb_fused_bwd(*xa, *ga, Wp, *da, ops._ptr(dW), accumulate, self.N, self.M, kw.get("Cin", self.Cin),
                                           kw.get("Fout", FOUT), kw.get("K", self.K), *self._plan_args(kw), ops._ptr(self.ws),
                                           kw.get("ws_bytes", self.need), ops._stream())


def test_direct_abi_padded_views_accumulate_and_halves(dev):
    a = Abi(dev)
    N, M, K, Cin = a.N, a.M, a.K, a.Cin
    y, ybuf, ymask = _padded((N, M, FOUT), 4, 0, dev)                # ldy = Fout + 4, NaN sentinels
    assert a.fwd(y) == 0
    dx, dxbuf, dxmask = _padded((N, M, Cin), 4, 0, dev)              # lddx = Cin + 4
    dW = torch.full((Cin * K, FOUT), float("nan"), device=dev)
    assert a.bwd(dx, dW) == 0
    torch.cuda.synchronize()
    assert _untouched(ybuf, ymask) and _untouched(dxbuf, dxmask)     # padding never written (and NaN input padding never read:
    got = (y.cpu().numpy(), dx.cpu().numpy(), dW.cpu().numpy())      #  element_bar asserts that every output is finite)
    y64, dx64, dW64, dWabs = S.reference(a.L, K, a.x, a.W, a.dy)
    y32, dx32, dW32 = S.twin32(a.L, K, a.x, a.W, a.dy)
    tag = "abi[grid17x15,K%d,Cin%d]" % (K, Cin)
    ebar(tag, "y", got[0], y32, y64)
    ebar(tag, "dx", got[1], dx32, dx64)
    sbar(tag, "dW", got[2], dW64, dWabs, dW32)
    # either half alone = its half of the full call, bit for bit
    dx2, dxbuf2, _ = _padded((N, M, Cin), 4, 0, dev)
    dW2 = torch.full_like(dW, float("nan"))
    assert a.bwd(dx2, None) == 0 and a.bwd(None, dW2) == 0
    torch.cuda.synchronize()
    assert same_bits(dx2.cpu().numpy(), got[1]) and _untouched(dxbuf2, dxmask) and same_bits(dW2.cpu().numpy(), got[2])
    # accumulate = 1: pre-fill + gradient, the pre-fill counted among the terms
    pre = np.random.default_rng(5).standard_normal((Cin * K, FOUT)).astype(np.float32)
    dW3 = torch.tensor(pre, device=dev)
    assert a.bwd(None, dW3, accumulate=1) == 0
    torch.cuda.synchronize()
    sbar(tag, "dW accumulated", dW3.cpu().numpy(), pre.astype(np.float64) + dW64, np.abs(pre).astype(np.float64) + dWabs,
         pre + dW32)
    assert same_bits(dW3.cpu().numpy(), pre + got[2])                # one float32 addition per element onto the reduced gradient


def test_refused_arguments(dev):
    """Every refusal returns before a launch: the outputs keep their sentinels."""
    a = Abi(dev)
    lib = a.ops.lib
    N, M, K, Cin = a.N, a.M, a.K, a.Cin
    for k in range(2, 9):
        assert lib.cape_cheb_fused_supported(8, FOUT, k) == 1 and lib.cape_cheb_fused_supported(16, FOUT, k) == 1
    y = torch.full((N, M, 64), 7.0, device=dev)[:, :, :FOUT]          # (wide enough for the refused Fout = 64 as well)
    dx = torch.full((N, M, 32), 7.0, device=dev)[:, :, :Cin]
    dW = torch.full((32 * 9, 64), 7.0, device=dev)
    for kw in (dict(Cin=24), dict(Fout=64), dict(K=1), dict(K=9)):
        shape = (kw.get("Cin", Cin), kw.get("Fout", FOUT), kw.get("K", K))
        assert lib.cape_cheb_fused_supported(*shape) == 0, kw
        assert lib.cape_cheb_fused_bwd_workspace_bytes(N, shape[0], shape[1], shape[2], a.plan.P) == EINVAL, kw
        assert a.fwd(y, **kw) == EINVAL and a.bwd(dx, dW, **kw) == EINVAL, kw
    both = [dict(rmax=1028), dict(ldx=Cin - 4), dict(x_off=4), dict(ldx=Cin + 2)]
    for kw in both + [dict(ldy=FOUT - 4)]:
        assert a.fwd(y, **kw) == EINVAL, kw
    for kw in both + [dict(lddx=Cin + 2), dict(lddx=Cin - 4), dict(lddy=FOUT - 4),
                      dict(lddy=FOUT + 1), dict(dy_off=4), dict(W_off=4)]:         # (the last three: dy and W are read as float4)
        assert a.bwd(dx, dW, **kw) == EINVAL, kw
    assert a.bwd(None, None) == EINVAL
    assert a.bwd(dx, dW, ws_bytes=a.need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((dx == 7.0).all()) and bool((dW == 7.0).all())
    assert a.fwd(y) == 0 and a.bwd(dx, dW[:Cin * K * FOUT // 64].view(Cin * K, FOUT)) == 0      # the argument set itself is valid
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and not bool((y == 7.0).all())
