"""The dense-layer kernels of csrc/fc.hip and csrc/fc_mfma.h (encoder fc_mean / fc_var, decoder fc1) on their own, against
float64 restatements (tests/fc_cases.py), through the C entry points ``cape_fc_long_fwd / _bwd`` and ``cape_fc_wide_fwd /
_bwd`` at the smallest shapes that reach every kernel, every template instantiation and every edge of a tile; then the
autograd wrappers ``ops.dense`` / ``ops.dense_pair`` at their gates.

Every output (y, dx, dW_m, db_m, the workspace) is a window of a larger buffer full of a sentinel: the floats in front of
it, the pad columns of a larger leading dimension, the row behind the last one and the floats behind that keep their bits.
The pad columns of the inputs are NaN.  Every call runs twice on fresh buffers and gives the same bits.  Bare contractions
are held to kernel_bars.sum_bar (2e-6 of sum |terms| per element), the wide forward behind an activation to
kernel_bars.element_bar.  The table of cases states the kernel each one reaches for the CAPE_FC_MFMA of the process
(tests/test_gpu_knobs.py runs this file again with CAPE_FC_MFMA=0); tests/test_fc_cases_host.py proves the table."""
import numpy as np
import pytest
import torch

import fc_cases as F
from kernel_bars import element_bar, sum_bar, same_bits, bits

pytestmark = pytest.mark.gpu

SENT = np.float32(-31337.5)
NAN = np.float32(np.nan)
EINVAL, EWORKSPACE = -1, -4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class Win:
    """rows x cols window, rows ``ld`` floats apart, of a 1-D device buffer: 4 floats in front of it (5 when the window has
    to sit off a 16-byte boundary), one spare row and 8 floats behind it, everything outside the window = ``pad``."""

    def __init__(self, dev, rows, cols, ld=None, off=False, data=None, pad=SENT):
        ld = cols if ld is None else ld
        assert ld >= cols and rows >= 1 and cols >= 1
        lead = 5 if off else 4
        host = np.full(lead + (rows + 1) * ld + 8, pad, np.float32)
        self.idx = lead + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
        assert self.idx.max() < host.size - 8                               # the window lies inside the allocation
        self.outside = np.ones(host.size, bool)
        self.outside[self.idx.reshape(-1)] = False
        if data is not None:
            host[self.idx] = np.asarray(data, np.float32).reshape(rows, cols)
        self.pad_bits = bits(np.full(1, pad, np.float32))[0]
        self.buf = torch.from_numpy(host).to(dev)
        self.t = self.buf[lead:]
        assert (self.t.data_ptr() % 16 != 0) == bool(off)

    def read(self):
        """(the window, whether everything outside it kept its bits)"""
        host = self.buf.cpu().numpy()
        return host[self.idx].copy(), bool((bits(host[self.outside]) == self.pad_bits).all())


def _t(w):
    return None if w is None else w.t


def execute(dev, c, d, over=None, null=()):
    """One call of the case's entry point on fresh buffers.  ``over``: scalar arguments replaced in the CALL only (the buffers
    are those of the case); ``null``: pointers passed as NULL although allocated.  Returns (rc, {name: Win} of the outputs)."""
    from cape_amd import ops
    lib, P, S = ops.lib, ops._ptr, ops._stream
    N, in_, out, nmat, off, ld = c["N"], c["in_"], c["out"], c["nmat"], c["off"], c["ld"]
    a = dict(N=N, in_=in_, out=out, nmat=nmat, act=c["act"], ldx=ld.get("x", in_), ldy=ld.get("y", out), ldg=ld.get("g", out),
             lddx=ld.get("dx", in_))
    gone = set(c["null"]) | set(null)
    arg = lambda w, name: None if name in gone else _t(w)
    x = Win(dev, N, in_, a["ldx"], "x" in off, d["x"], pad=NAN)
    outs = {}
    if c["entry"] in ("long_fwd", "long_bwd"):
        na = max(nmat, (over or {}).get("nmat", nmat))                      # pointer arrays as long as the call claims
        ms = [min(m, nmat - 1) for m in range(na)]
        Ws = [Win(dev, in_, out, off=("W%d" % m) in off, data=d["W%d" % m], pad=NAN) for m in range(nmat)]
        parr = lambda ws_, pre: ops._parr([arg(ws_[m], "%s%d" % (pre, m)) for m in ms])
        if c["entry"] == "long_fwd":
            bs = [None if d["b%d" % m] is None else Win(dev, 1, out, data=d["b%d" % m], pad=NAN) for m in range(nmat)]
            ys = [Win(dev, N, out, off=("y%d" % m) in off) for m in range(nmat)]
            need = F.long_workspace_bytes(N, in_, out, nmat)
            ws = Win(dev, 1, need // 4, off="ws" in off)
            a["ws_bytes"] = need
            a.update(over or {})
            rc = lib.cape_fc_long_fwd(P(x.t), a["ldx"], a["N"], a["in_"], a["out"], a["nmat"], parr(Ws, "W"), parr(bs, "b"), parr(ys, "y"),
                                      P(arg(ws, "ws")), a["ws_bytes"], S())
            outs = dict({"y%d" % m: ys[m] for m in range(nmat)}, ws=ws)
        else:
            gs = [Win(dev, N, out, off=("g%d" % m) in off, data=d["g%d" % m], pad=NAN) for m in range(nmat)]
            dWs = [Win(dev, in_, out, off=("dW%d" % m) in off) for m in range(nmat)]
            dbs = [Win(dev, 1, out, off=("db%d" % m) in off) for m in range(nmat)]
            dx = Win(dev, N, in_, a["lddx"], "dx" in off)
            a.update(over or {})
            rc = lib.cape_fc_long_bwd(P(x.t), a["ldx"], a["N"], a["in_"], a["out"], a["nmat"], parr(Ws, "W"), parr(gs, "g"), parr(dWs, "dW"),
                                      parr(dbs, "db"), P(arg(dx, "dx")), a["lddx"], S())
            outs = dict({"dW%d" % m: dWs[m] for m in range(nmat)}, dx=dx, **{"db%d" % m: dbs[m] for m in range(nmat)})
    else:
        W = Win(dev, in_, out, off="W" in off, data=d["W"], pad=NAN)
        if c["entry"] == "wide_fwd":
            b = None if d["b"] is None else Win(dev, 1, out, off="b" in off, data=d["b"], pad=NAN)
            y = Win(dev, N, out, a["ldy"], "y" in off)
            a.update(over or {})
            rc = lib.cape_fc_wide_fwd(P(x.t), a["ldx"], a["N"], a["in_"], a["out"], P(arg(W, "W")), P(arg(b, "b")), a["act"], P(arg(y, "y")), a["ldy"], S())
            outs = dict(y=y)
        else:
            g = Win(dev, N, out, a["ldg"], "g" in off, d["g"], pad=NAN)
            y = None if d["y"] is None else Win(dev, N, out, a["ldy"], "y" in off, d["y"], pad=NAN)
            dW, db = Win(dev, in_, out, off="dW" in off), Win(dev, 1, out, off="db" in off)
            dx = Win(dev, N, in_, a["lddx"], "dx" in off)
            need = F.wide_workspace_bytes(N, in_, out)
            ws = Win(dev, 1, need // 4, off="ws" in off)
            a["ws_bytes"] = need
            a.update(over or {})
            rc = lib.cape_fc_wide_bwd(P(x.t), a["ldx"], P(arg(g, "g")), a["ldg"], P(arg(y, "y")), a["ldy"], a["act"], a["N"], a["in_"], a["out"],
                                      P(arg(W, "W")), P(arg(dW, "dW")), P(arg(db, "db")), P(arg(dx, "dx")), a["lddx"], P(arg(ws, "ws")),
                                      a["ws_bytes"], S())
            outs = dict(dW=dW, db=db, dx=dx, ws=ws)
    torch.cuda.synchronize()
    return int(rc), outs


def _untouched(outs):
    for k, w in outs.items():
        v, ok = w.read()
        if not ok or not (bits(v) == w.pad_bits).all():
            return False
    return True


def _kernels_of(c, quantity, kernels):
    """The kernels a quantity of a case went through (the figure printed per kernel)."""
    if c["entry"] != "wide_bwd":
        return kernels
    return tuple(k for k in kernels if ("_dx_" in k) == (quantity == "dx"))


def run_table(dev, cases):
    """Every case twice; returns (failures, {kernel: (worst figure in units of its bar, case / quantity)})."""
    from cape_amd import ops
    failures, worst = [], {}
    for c in cases:
        d = F.inputs(c)
        want = F.expected_tier(c)
        if F.case_tier(c) != want:
            failures.append("%s: tier() says %s, the table %s" % (c["name"], F.case_tier(c), want))
            continue
        rc, outs = execute(dev, c, d)
        if want == F.EINVAL:                                    # (CAPE_FC_MFMA=0 only: no dx kernel has the LDS for in = 256)
            if rc != EINVAL or not _untouched(outs):
                failures.append("%s: rc %d, expected a refusal before any launch" % (c["name"], rc))
            continue
        if rc != 0:
            failures.append("%s: rc %d (%s)" % (c["name"], rc, c["why"]))
            continue
        if c["entry"] == "long_fwd":
            assert int(ops.lib.cape_fc_long_workspace_bytes(c["N"], c["in_"], c["out"], c["nmat"])) == F.long_workspace_bytes(c["N"], c["in_"], c["out"], c["nmat"])
        if c["entry"] == "wide_bwd":
            assert int(ops.lib.cape_fc_wide_bwd_workspace_bytes(c["N"], c["in_"], c["out"])) == F.wide_workspace_bytes(c["N"], c["in_"], c["out"])
        rc2, outs2 = execute(dev, c, d)
        ref = F.reference(c, d, np.float64)
        f32 = F.reference(c, d, np.float32)
        for k, w in outs.items():
            v, ok = w.read()
            v2, ok2 = outs2[k].read()
            if not (ok and ok2):
                failures.append("%s / %s: wrote outside its window (%s)" % (c["name"], k, c["why"]))
            if rc2 != 0 or not same_bits(v, v2):
                failures.append("%s / %s: two runs differ" % (c["name"], k))
            if k == "ws":
                continue
            if k in c["null"]:
                if not (bits(v) == w.pad_bits).all():
                    failures.append("%s / %s: written although passed as NULL" % (c["name"], k))
                continue
            want_v, scale = ref[k]
            v = v.reshape(want_v.shape)
            try:
                if F.uses_element_bar(c):
                    fig = element_bar("fc", "%s / %s" % (c["name"], k), v, f32[k][0], want_v) / 4.0
                else:
                    fig = sum_bar("fc", "%s / %s" % (c["name"], k), v, want_v, scale, f32=f32[k][0]) / 2e-6
            except AssertionError as e:
                failures.append("%s / %s (%s): %s" % (c["name"], k, "+".join(want), str(e)[:300]))
                continue
            for kern in _kernels_of(c, k, want):
                if fig >= worst.get(kern, (-1.0, ""))[0]:
                    worst[kern] = (fig, "%s / %s" % (c["name"], k))
    for kern in sorted(worst):
        print("WORST %-40s %.3f of its bar at %s" % (kern, worst[kern][0], worst[kern][1]))
    return failures, worst


def _judge(failures, worst, cases):
    assert not failures, "\n".join(failures)
    reached = {k for c in cases for k in F.expected_tier(c)} - {F.EINVAL[0]}
    assert set(worst) == reached, reached - set(worst)


def test_long_forward_every_tier(dev):
    """cape_fc_long_fwd: fc_long_partial_kernel / _v4 / _m16<1> / _m16<2> and fc_long_final_kernel over 1 .. 130 splits.
    y is held to sum_bar (2e-6 of sum |terms|).  Worst measured, as a fraction of that bar: partial 0.105 and final 0.105
    (lf_g_n64), partial_v4 0.030 (lf_v_in130), m16<1> 0.035 (lf_m1_in4), m16<2> 0.034 (lf_m2_in144); the float32 numpy
    restatement of the same cases reaches 0.12."""
    failures, worst = run_table(dev, F.LONG_FWD_CASES)
    _judge(failures, worst, F.LONG_FWD_CASES)


def test_long_backward_every_tier(dev):
    """cape_fc_long_bwd: fc_long_bwd_kernel / _v4 / _m16<1,1> / <1,2> / <2,1> with each of dW[m], db[m], dx NULL in turn.
    The lb_v_f1_* cases are the ones the MFMA kernel failed before the dispatcher asked for in % 4 == 0 under a dx: its
    float4 store wrote columns 130 and 131 (6 and 7) of every dx row.  lb_g_nodw0 and lb_g_n58_out20 are the ones the generic
    kernel failed while it skipped db[m] together with a NULL dW[m].  Worst measured fraction of sum_bar: generic 0.116
    (lb_g_n58 / dW0), v4 0.097 (lb_v_out128x2 / dW0), m16<1,1> 0.084, m16<1,2> 0.102, m16<2,1> 0.096."""
    failures, worst = run_table(dev, F.LONG_BWD_CASES)
    _judge(failures, worst, F.LONG_BWD_CASES)


def test_wide_forward_every_tier_and_activation(dev):
    """cape_fc_wide_fwd: fc_wide_fwd_kernel / _v4 / _m16<1> / <2> / <4> under every activation.  act = none: sum_bar; leaky /
    relu / tanh: element_bar against the float32 restatement.  Worst measured fraction of the bar (for element_bar: error over
    4 x the restatement's): generic 0.258 (wf_g_out1030_act3), v4 0.326 (wf_v_in3_act3), m16<1> 0.432 (wf_m1_n1_act1), m16<2>
    0.143, m16<4> 0.172."""
    failures, worst = run_table(dev, F.WIDE_FWD_CASES)
    _judge(failures, worst, F.WIDE_FWD_CASES)


def test_wide_backward_every_tier_of_both_halves(dev):
    """cape_fc_wide_bwd: the dW / db half (fc_wide_bwd_dw_kernel / _v4 / _m16<1,2,4>) and the dx half (fc_wide_bwd_dx_partial_kernel
    / _v4 / fc_wide_bwd_dx_m16_kernel<1,2,4> + fc_wide_bwd_dx_final_kernel) are dispatched separately.  The in = 256 cases were
    refused outright before the LDS bound of the generic dx kernel was applied to that kernel alone.  Worst measured fraction
    of sum_bar: dw 0.126, dw_v4 0.111, dw_m16<1> 0.094, <2> 0.108, <4> 0.108; dx_partial 0.068, dx_partial_v4 0.105, dx_m16<1> 0.057,
    <2> 0.062, <4> 0.092, dx_final 0.105."""
    failures, worst = run_table(dev, F.WIDE_BWD_CASES)
    _judge(failures, worst, F.WIDE_BWD_CASES)


# ------------------------------------------------------------------------------------------- refused before any launch
def _case(table, name):
    return next(c for c in table if c["name"] == name)


def _refused(dev, c, over=None, null=(), rc_want=EINVAL, alloc=None):
    ca = dict(c, **(alloc or {}))
    rc, outs = execute(dev, ca, F.inputs(ca), over=over, null=null)
    assert rc == rc_want, (c["name"], over, null, rc)
    assert _untouched(outs), (c["name"], over, null)


def test_entry_points_refuse_bad_arguments(dev):
    """Host-side checks of the four entry points: a non-zero return and every output buffer still full of the sentinel."""
    lf, lb = _case(F.LONG_FWD_CASES, "lf_m1_in132"), _case(F.LONG_BWD_CASES, "lb_m12_all")
    wf, wb = _case(F.WIDE_FWD_CASES, "wf_m2_out192_act1"), _case(F.WIDE_BWD_CASES, "wb_m2_out192")
    for c in (lf, lb, wf, wb):
        rc, outs = execute(dev, c, F.inputs(c))
        assert rc == 0 and not _untouched(outs)                               # (the base cases are accepted)
        _refused(dev, c, over=dict(N=0))
        _refused(dev, c, over=dict(N=65), alloc=dict(N=65))
        _refused(dev, c, over=dict(in_=0))
        _refused(dev, c, over=dict(out=0))
        _refused(dev, c, over=dict(ldx=c["in_"] - 1))
    for c in (lf, lb):
        _refused(dev, c, over=dict(nmat=0))
        _refused(dev, c, over=dict(nmat=3))
        _refused(dev, c, null=("W1",))
        _refused(dev, c, null=("W0",))
    _refused(dev, lf, null=("y1",))
    _refused(dev, lf, null=("ws",))
    _refused(dev, lf, over=dict(ws_bytes=F.long_workspace_bytes(lf["N"], lf["in_"], lf["out"], lf["nmat"]) - 1), rc_want=EWORKSPACE)
    _refused(dev, lb, null=("g1",))
    _refused(dev, lb, over=dict(lddx=lb["in_"] - 1))
    for c in (wf, wb):
        _refused(dev, c, over=dict(act=-1))
        _refused(dev, c, over=dict(act=4))
        _refused(dev, c, null=("W",))
        big = dict(N=64, in_=193, out=8, ld={}, off=frozenset())                # N * in * 4 = 49 408 > 48 KB
        _refused(dev, c, alloc=big)
    _refused(dev, wf, over=dict(ldy=wf["out"] - 1))
    _refused(dev, wf, null=("y",))
    _refused(dev, wb, over=dict(ldg=wb["out"] - 1))
    _refused(dev, wb, over=dict(ldy=wb["out"] - 1))
    _refused(dev, wb, over=dict(lddx=wb["in_"] - 1))
    _refused(dev, wb, null=("y",))                                              # an activation with y = NULL
    _refused(dev, wb, null=("g",))
    _refused(dev, wb, null=("ws",))
    _refused(dev, wb, over=dict(ws_bytes=F.wide_workspace_bytes(wb["N"], wb["in_"], wb["out"]) - 1), rc_want=EWORKSPACE)
    # the LDS bounds of the generic backward kernels, each on the kernel that has the layout
    _refused(dev, dict(lb, name="lb_refused_n59"), alloc=dict(N=59, in_=70, ld={}))
    _refused(dev, dict(wb, name="wb_refused_n37"), alloc=dict(N=37, in_=200, out=70, ld={}))
    c = dict(wb, name="wb_n37_nodx", N=37, in_=200, out=70, ld={}, null=frozenset(("dx",)), tier=(F.DW_G,), tier0=(F.DW_G,), why="no dx: no bound")
    failures, _ = run_table(dev, [c])
    assert not failures, failures


# --------------------------------------------------------------------------- the wrappers at the gates of ops.py
def _leaf(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True)


def _np(t):
    return t.detach().cpu().numpy()


def _randn(rng, *s):
    return rng.standard_normal(s).astype(np.float32)


PAIR_GATES = [(58, 8192, 64, ["fc_long_fwd", "fc_long_bwd"]),                  # the last batch the two-matrix backward has the LDS for
              (59, 8192, 64, ["fc_long_fwd"] * 2 + ["fc_long_bwd"] * 2),       # one matrix per launch from here on
              (64, 8192, 64, ["fc_long_fwd"] * 2 + ["fc_long_bwd"] * 2),
              (64, 8192, 18, ["fc_long_fwd", "fc_long_bwd"])]


def _pair(dev, N, kin, out, launches, b0_none=False, unused=None, bufs=False):
    from cape_amd import ops
    rng = np.random.default_rng(1000 * N + out + 7 * b0_none)
    x, k0, k1, b0, b1 = _randn(rng, N, kin), _randn(rng, kin, out), _randn(rng, kin, out), _randn(rng, out), _randn(rng, out)
    g0, g1 = _randn(rng, N, out), _randn(rng, N, out)
    if b0_none:
        b0 = None
    tx, tk0, tk1, tb1 = (_leaf(dev, v) for v in (x, k0, k1, b1))
    tb0 = None if b0 is None else _leaf(dev, b0)
    grad_bufs, parent, spans = ((None, None), (None, None)), None, []
    if bufs:
        sizes = [kin * out, out, kin * out, out]
        offs, o = [], 8
        for s in sizes:
            offs.append(o)
            o += s + 12                                                        # a gap of 12 floats between the views
        parent = torch.full((o,), float(SENT), device=dev)
        v = [parent[a:a + s] for a, s in zip(offs, sizes)]
        grad_bufs = ((v[0].view(kin, out), v[1]), (v[2].view(kin, out), v[3]))
        spans = list(zip(offs, sizes))
    ops.LAUNCH_LOG = []
    try:
        y0, y1 = ops.dense_pair(tx, tk0, tb0, tk1, tb1, grad_bufs=grad_bufs)
        loss = (y1 * torch.from_numpy(g1).to(dev)).sum()
        if unused != 0:
            loss = loss + (y0 * torch.from_numpy(g0).to(dev)).sum()
        leaves = dict(dx=tx, dW0=tk0, dW1=tk1, db1=tb1, **({} if tb0 is None else dict(db0=tb0)))
        got = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))      # (the tensors the backward returned)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert names == launches, names
    if unused == 0:
        g0 = np.zeros_like(g0)
    tag = "dense_pair %dx%dx%d" % (N, kin, out)
    (r0, a0), (r1, a1) = F.long_fwd_ref(x, [k0, k1], [b0, b1], np.float64)
    sum_bar(tag, "y0", _np(y0), r0, a0)
    sum_bar(tag, "y1", _np(y1), r1, a1)
    r = F.long_bwd_ref(x, [k0, k1], [g0, g1], np.float64)
    for k, t in got.items():
        assert t is not None, k
        sum_bar(tag, k, _np(t).reshape(r[k][0].shape), *r[k])
    if bufs:
        for t, (a, s) in zip((got["dW0"], got["db0"], got["dW1"], got["db1"]), spans):
            assert t.data_ptr() == parent.data_ptr() + 4 * a, "the gradient did not land in the given view"
        host = parent.cpu().numpy()
        keep = np.ones(host.size, bool)
        for a, s in spans:
            keep[a:a + s] = False
        assert (bits(host[keep]) == bits(np.full(1, SENT, np.float32))[0]).all()


@pytest.mark.parametrize("N,kin,out,launches", PAIR_GATES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_dense_pair_at_its_gate(dev, N, kin, out, launches):
    """ops.dense_pair across _fc_long_ok: batch 59 .. 64 of the shipped nz = 64 pair used to pass the gate, run its forward and
    raise CAPE_EINVAL in the backward (the generic kernel's 60 KB of LDS hold two matrices up to N = 58)."""
    _pair(dev, N, kin, out, launches)


def test_dense_pair_without_a_bias_with_an_unused_output_and_into_given_views(dev):
    _pair(dev, 5, 8192, 20, ["fc_long_fwd", "fc_long_bwd"], b0_none=True)
    _pair(dev, 16, 8192, 64, ["fc_long_fwd", "fc_long_bwd"], unused=0)
    _pair(dev, 3, 8192, 18, ["fc_long_fwd", "fc_long_bwd"], bufs=True)


DENSE_GATES = [(36, 200, 8192, "leaky_relu", ["fc_wide_fwd", "fc_wide_bwd"]),   # the last batch the generic dx kernel has the LDS for
               (37, 200, 8192, None, []),                                       # from here on: torch
               (61, 200, 8192, "leaky_relu", []),
               (64, 128, 8192, None, ["fc_wide_fwd", "fc_wide_bwd"])]


def _dense(dev, N, kin, out, activation, launches, bias=True, bufs=False):
    from cape_amd import ops
    rng = np.random.default_rng(77 * N + kin)
    x, W, b, g = _randn(rng, N, kin), (_randn(rng, kin, out) / np.float32(np.sqrt(kin))).astype(np.float32), _randn(rng, out), _randn(rng, N, out)
    tx, tW = _leaf(dev, x), _leaf(dev, W)
    tb = _leaf(dev, b) if bias else None
    grad_bufs, parent = (None, None), None
    if bufs:
        parent = torch.full((8 + kin * out + 12 + out + 8,), float(SENT), device=dev)
        grad_bufs = (parent[8:8 + kin * out].view(kin, out), parent[8 + kin * out + 12:8 + kin * out + 12 + out])
    ops.LAUNCH_LOG = []
    try:
        y = ops.dense(tx, tW, tb, activation=activation, grad_bufs=grad_bufs)
        leaves = [tx, tW] + ([tb] if bias else [])
        grads = torch.autograd.grad((y * torch.from_numpy(g).to(dev)).sum(), leaves)      # (the tensors the backward returned)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert names == launches, names
    act = 1 if activation else 0
    tag = "dense %dx%dx%d %s" % (N, kin, out, activation)
    yd = _np(y)
    r64, a = F.wide_fwd_ref(x, W, b if bias else None, act, np.float64)
    if act:
        element_bar(tag, "y", yd, F.wide_fwd_ref(x, W, b if bias else None, act, np.float32)[0], r64)
        assert (yd != 0).all()
    else:
        sum_bar(tag, "y", yd, r64, a)
    r = F.wide_bwd_ref(x, g, yd, act, W, np.float64)                            # dz from the y the device wrote
    sum_bar(tag, "dx", _np(grads[0]), *r["dx"])
    sum_bar(tag, "dW", _np(grads[1]), *r["dW"])
    if bias:
        sum_bar(tag, "db", _np(grads[2]), *r["db"])
    if bufs:
        assert grads[1].data_ptr() == grad_bufs[0].data_ptr() and grads[2].data_ptr() == grad_bufs[1].data_ptr()
        host = parent.cpu().numpy()
        keep = np.ones(host.size, bool)
        keep[8:8 + kin * out] = False
        keep[8 + kin * out + 12:8 + kin * out + 12 + out] = False
        assert (bits(host[keep]) == bits(np.full(1, SENT, np.float32))[0]).all()


@pytest.mark.parametrize("N,kin,out,activation,launches", DENSE_GATES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_dense_at_its_gate(dev, N, kin, out, activation, launches):
    """ops.dense across _fc_wide_ok: at kin = 200 the gate used to admit N = 37 .. 61, which cape_fc_wide_bwd refuses."""
    _dense(dev, N, kin, out, activation, launches)


def test_dense_without_a_bias_and_into_given_views(dev):
    _dense(dev, 4, 64, 8192, "leaky_relu", ["fc_wide_fwd", "fc_wide_bwd"], bias=False)
    _dense(dev, 16, 82, 8192, "leaky_relu", ["fc_wide_fwd", "fc_wide_bwd"], bufs=True)
    # the long single-matrix form of ops.dense
    from cape_amd import ops
    rng = np.random.default_rng(5)
    x, W, b, g = _randn(rng, 64, 8192), _randn(rng, 8192, 20), _randn(rng, 20), _randn(rng, 64, 20)
    tx, tW, tb = _leaf(dev, x), _leaf(dev, W), _leaf(dev, b)
    y = ops.dense(tx, tW, tb)
    grads = torch.autograd.grad((y * torch.from_numpy(g).to(dev)).sum(), [tx, tW, tb])
    (r0, a0), = F.long_fwd_ref(x, [W], [b], np.float64)
    sum_bar("dense long", "y", _np(y), r0, a0)
    r = F.long_bwd_ref(x, [W], [g], np.float64)
    for k, t in zip(("dx", "dW0", "db0"), grads):
        sum_bar("dense long", k, _np(t), *r[k])
