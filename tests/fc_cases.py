"""The cases of tests/test_gpu_fc.py: the dense-layer kernels of csrc/fc.hip and csrc/fc_mfma.h called through the four
``cape_fc_*`` entry points at the smallest shapes that still reach every kernel, every template instantiation and every
edge of a tile.  TEST INFRASTRUCTURE ONLY (no GPU needed here; tests/test_fc_cases_host.py checks this file on the CPU).

* ``tier(entry, ...)`` restates the host dispatch of the four ``extern "C"`` functions: from shapes, leading dimensions, which
  pointers are off a 16-byte boundary, which optional pointers are NULL and CAPE_FC_MFMA it names the kernels that run.
* ``*_ref`` are plain-numpy restatements of the four operations in a precision ``T`` (float64: the reference; float32: the
  restatement the element bar compares with).  Each value comes with sum |terms| of every output element for
  kernel_bars.sum_bar.  The wide backward takes dz = g * act'(y) from the ``y`` array it is GIVEN, as the kernels do.
* One case table per entry point; every case names the kernels it is meant to reach, with and without the MFMA tier, and why
  it is there.

Pointer names: long side  x ws W0 W1 b0 b1 y0 y1 g0 g1 dW0 dW1 db0 db1 dx;  wide side  x W b y g dW db dx ws."""
import os
import re
import zlib

import numpy as np

FC_MAXN, FC_RS, FC_MAXMAT, FC_DXC = 64, 128, 2, 2
LDS_MAX = 60 * 1024
EINVAL = ("CAPE_EINVAL",)

FINAL, DXFINAL = "fc_long_final_kernel", "fc_wide_bwd_dx_final_kernel"
LF_G, LF_V = "fc_long_partial_kernel", "fc_long_partial_v4_kernel"
LB_G, LB_V = "fc_long_bwd_kernel", "fc_long_bwd_v4_kernel"
WF_G, WF_V = "fc_wide_fwd_kernel", "fc_wide_fwd_v4_kernel"
DW_G, DW_V = "fc_wide_bwd_dw_kernel", "fc_wide_bwd_dw_v4_kernel"
DX_G, DX_V = "fc_wide_bwd_dx_partial_kernel", "fc_wide_bwd_dx_partial_v4_kernel"


def LF_M(q):
    return "fc_long_partial_m16_kernel<%d>" % q


def LB_M(q, nm):
    return "fc_long_bwd_m16_kernel<%d,%d>" % (q, nm)


def WF_M(nr):
    return "fc_wide_fwd_m16_kernel<%d>" % nr


def DW_M(nr):
    return "fc_wide_bwd_dw_m16_kernel<%d>" % nr


def DX_M(nr):
    return "fc_wide_bwd_dx_m16_kernel<%d>" % nr


# every __global__ of the two files, every instantiation the dispatcher can launch
ALL_KERNELS = sorted([FINAL, DXFINAL, LF_G, LF_V, LB_G, LB_V, WF_G, WF_V, DW_G, DW_V, DX_G, DX_V,
                      LF_M(1), LF_M(2), LB_M(1, 1), LB_M(1, 2), LB_M(2, 1),
                      WF_M(1), WF_M(2), WF_M(4), DW_M(1), DW_M(2), DW_M(4), DX_M(1), DX_M(2), DX_M(4)])


def mfma_on():
    """fc_m16_on of csrc/fc_mfma.h: off only when atoi(CAPE_FC_MFMA) == 0."""
    v = os.environ.get("CAPE_FC_MFMA")
    if v is None:
        return True
    m = re.match(r"\s*[+-]?\d+", v)
    return (int(m.group(0)) if m else 0) != 0


def long_workspace_bytes(N, in_, out, nmat):
    return nmat * ((in_ + FC_RS - 1) // FC_RS) * N * out * 4


def wide_workspace_bytes(N, in_, out):
    return ((out + 63) // 64) * N * in_ * 4


def tier(entry, N, in_, out, nmat=1, ld=None, off=(), null=(), act=0, mfma=None):
    """Names of the kernels the entry point launches, in order, or EINVAL.  ``ld``: leading dimensions that differ from the
    dense ones (keys x y g dx); ``off``: pointers NOT on a 16-byte boundary; ``null``: optional pointers passed as NULL."""
    ld = dict(ld or {})
    mfma = mfma_on() if mfma is None else mfma
    al = lambda p: p not in off
    has = lambda p: p not in null
    ldx, lddx = ld.get("x", in_), ld.get("dx", in_)
    ldy, ldg = ld.get("y", out), ld.get("g", out)
    if N < 1 or N > FC_MAXN or in_ < 1 or out < 1 or ldx < in_:
        return EINVAL
    ms = range(nmat)
    if entry == "long_fwd":
        if nmat < 1 or nmat > FC_MAXMAT:
            return EINVAL
        v4 = N <= 16 and out % 4 == 0 and all(al("W%d" % m) for m in ms)
        m16 = mfma and v4 and out in (64, 128) and in_ % 4 == 0 and ldx % 4 == 0 and al("x") and al("ws")
        return (LF_M(out // 64) if m16 else LF_V if v4 else LF_G, FINAL)
    if entry == "long_bwd":
        if nmat < 1 or nmat > FC_MAXMAT or (has("dx") and lddx < in_):
            return EINVAL
        v4 = N <= 16 and out % 4 == 0 and (16 * 64 + nmat * 16 * out) * 4 <= LDS_MAX
        v4 = v4 and all(al("W%d" % m) and (not has("dW%d" % m) or al("dW%d" % m)) for m in ms)
        m16 = mfma and v4 and (out == 64 or (out == 128 and nmat == 1))
        m16 = m16 and (not has("dx") or (in_ % 4 == 0 and lddx % 4 == 0 and al("dx"))) and all(al("g%d" % m) for m in ms)
        if m16:
            return (LB_M(out // 64, nmat),)
        if v4:
            return (LB_V,)
        if (N * 64 + nmat * N * out + 64 * 65) * 4 > LDS_MAX:
            return EINVAL
        return (LB_G,)
    if act < 0 or act > 3 or N * in_ * 4 > 48 * 1024:
        return EINVAL
    mshape = mfma and N <= 16 and out % 64 == 0 and in_ in (64, 128, 256)
    if entry == "wide_fwd":
        if ldy < out:
            return EINVAL
        m16 = mshape and al("W") and al("x") and ldx % 4 == 0 and al("y") and ldy % 4 == 0 and (not has("b") or al("b"))
        if m16:
            return (WF_M(in_ // 64),)
        if N <= 16 and out % 4 == 0 and al("W") and (16 * in_ + 4 * 16 * 128) * 4 <= LDS_MAX:
            return (WF_V,)
        return (WF_G,)
    assert entry == "wide_bwd", entry
    if ldg < out or (act != 0 and (not has("y") or ldy < out)):
        return EINVAL
    yok = act == 0 or (ldy % 4 == 0 and al("y"))
    ks = []
    if has("dW") or has("db"):
        v4 = N <= 16 and out % 4 == 0 and ldg % 4 == 0 and al("g") and (not has("dW") or al("dW")) and (not has("db") or al("db")) and yok
        ks.append(DW_M(in_ // 64) if (mshape and v4 and ldx % 4 == 0) else DW_V if v4 else DW_G)
    if has("dx"):
        if lddx < in_ or not has("ws"):
            return EINVAL
        if mshape and al("W") and al("g") and ldg % 4 == 0 and yok:
            ks.append(DX_M(in_ // 64))
        elif N <= 16 and in_ % 4 == 0 and al("ws") and (64 * (in_ + 4) + 16 * 64) * 4 <= LDS_MAX:
            ks.append(DX_V)
        elif (in_ * 65 + N * 64) * 4 > LDS_MAX:
            return EINVAL                                   # the LDS layout of the generic kernel alone
        else:
            ks.append(DX_G)
        ks.append(DXFINAL)
    return tuple(ks)


def wide_dx_slabs(kernels, out):
    """Partial slabs fc_wide_bwd_dx_final_kernel sums: one per 64 columns, one per FC_DXC * 64 on the MFMA kernel."""
    chunks = (out + 63) // 64
    return (chunks + FC_DXC - 1) // FC_DXC if any(k.startswith("fc_wide_bwd_dx_m16") for k in kernels) else chunks


# ----------------------------------------------------------------------------------------------------- references
def act_fn(v, act, T):
    if act == 1:
        return np.where(v > 0, v, T(0.2) * v).astype(T)
    if act == 2:
        return np.where(v > 0, v, T(0)).astype(T)
    if act == 3:
        return np.tanh(v).astype(T)
    return v


def act_grad_from_out(y, act, T):
    y = y.astype(T)
    if act == 1:
        return np.where(y > 0, T(1), T(0.2)).astype(T)
    if act == 2:
        return np.where(y > 0, T(1), T(0)).astype(T)
    if act == 3:
        return (T(1) - y * y).astype(T)
    return np.ones_like(y)


def long_fwd_ref(x, Ws, bs, T):
    """[(y_m, sum |terms|)]:  y_m = x W_m + b_m."""
    xs = x.astype(T)
    res = []
    for W, b in zip(Ws, bs):
        Wt = W.astype(T)
        y, a = xs @ Wt, np.abs(xs) @ np.abs(Wt)
        if b is not None:
            y, a = y + b.astype(T), a + np.abs(b.astype(T))
        res.append((y, a))
    return res


def long_bwd_ref(x, Ws, gs, T):
    """dict of (value, sum |terms|): dW0.. , db0.. , dx = sum_m g_m W_m^T."""
    xs = x.astype(T)
    res = {}
    dx, da = 0, 0
    for m, (W, g) in enumerate(zip(Ws, gs)):
        Wt, gt = W.astype(T), g.astype(T)
        res["dW%d" % m] = (xs.T @ gt, np.abs(xs).T @ np.abs(gt))
        res["db%d" % m] = (gt.sum(0, dtype=T), np.abs(gt).sum(0, dtype=T))
        dx, da = dx + gt @ Wt.T, da + np.abs(gt) @ np.abs(Wt).T
    res["dx"] = (dx, da)
    return res


def wide_fwd_ref(x, W, b, act, T):
    """(act(x W + b), sum |terms| of the pre-activation)."""
    xs, Wt = x.astype(T), W.astype(T)
    pre, a = xs @ Wt, np.abs(xs) @ np.abs(Wt)
    if b is not None:
        pre, a = pre + b.astype(T), a + np.abs(b.astype(T))
    return act_fn(pre, act, T), a


def wide_bwd_ref(x, g, y, act, W, T):
    """dict of (value, sum |terms|) for dW, db, dx with dz = g * act'(y) from the GIVEN y."""
    xs, Wt = x.astype(T), W.astype(T)
    dz = g.astype(T) if act == 0 else (g.astype(T) * act_grad_from_out(y, act, T)).astype(T)
    return {"dW": (xs.T @ dz, np.abs(xs).T @ np.abs(dz)),
            "db": (dz.sum(0, dtype=T), np.abs(dz).sum(0, dtype=T)),
            "dx": (dz @ Wt.T, np.abs(dz) @ np.abs(Wt).T)}


# ----------------------------------------------------------------------------------------------------- case tables
def _case(entry, name, N, in_, out, want, want0=None, why="", nmat=1, act=0, ld=None, off=(), null=()):
    return dict(entry=entry, name=name, N=N, in_=in_, out=out, nmat=nmat, act=act, ld=dict(ld or {}), off=frozenset(off),
                null=frozenset(null), tier=tuple(want), tier0=tuple(want0 if want0 is not None else want), why=why)


def case_tier(c, mfma=None):
    return tier(c["entry"], c["N"], c["in_"], c["out"], nmat=c["nmat"], ld=c["ld"], off=c["off"], null=c["null"], act=c["act"], mfma=mfma)


def expected_tier(c, mfma=None):
    return c["tier"] if (mfma_on() if mfma is None else mfma) else c["tier0"]


def _lf(name, N, in_, out, nmat, want, want0=None, why="", **kw):
    return _case("long_fwd", name, N, in_, out, (want, FINAL), None if want0 is None else (want0, FINAL), why, nmat=nmat, **kw)


LONG_FWD_CASES = [
    _lf("lf_g_n17", 17, 130, 18, 2, LF_G, why="two sample passes of 16, ragged columns and rows"),
    _lf("lf_g_n64", 64, 37, 70, 1, LF_G, why="full batch, two column passes, one short split"),
    _lf("lf_g_nob1", 5, 300, 18, 2, LF_G, why="out % 4 != 0 at N <= 16; b[1] = NULL", null=("b1",)),
    _lf("lf_g_n33", 33, 129, 5, 2, LF_G, why="last split of ONE row, 5 columns"),
    _lf("lf_g_n17_out64", 17, 64, 64, 1, LF_G, why="only N > 16 keeps this off the tiled kernels"),
    _lf("lf_g_w0_off", 4, 132, 64, 1, LF_G, why="W[0] off a 16-byte boundary", off=("W0",)),
    _lf("lf_g_w1_off", 4, 132, 64, 2, LF_G, why="only W[1] off a 16-byte boundary", off=("W1",)),
    _lf("lf_v_1row_split", 1, 129, 20, 1, LF_V, why="last split has one row: min(il, rows - 1) clamp"),
    _lf("lf_v_out68", 16, 260, 68, 2, LF_V, why="two column passes, the second with one quad"),
    _lf("lf_v_out132", 7, 128, 132, 1, LF_V, why="three column passes, exactly one split"),
    _lf("lf_v_ldx_odd", 3, 256, 64, 2, LF_V, why="m16 shape pushed to v4 by ldx % 4", ld={"x": 257}),
    _lf("lf_v_in130", 16, 130, 64, 2, LF_V, why="m16 shape pushed to v4 by in % 4"),
    _lf("lf_v_in130_ldx132", 16, 130, 64, 2, LF_V, why="only in % 4 keeps this off m16: its x quad at 128 would take the NaN pad", ld={"x": 132}),
    _lf("lf_v_x_off", 4, 132, 64, 1, LF_V, why="m16 shape pushed to v4 by x alignment", off=("x",)),
    _lf("lf_v_ws_off", 4, 132, 128, 1, LF_V, why="m16 shape pushed to v4 by workspace alignment", off=("ws",)),
    _lf("lf_m1_in4", 1, 4, 64, 1, LF_M(1), LF_V, "one quad of rows, one sample", ld={"x": 8}),
    _lf("lf_m1_in132", 3, 132, 64, 2, LF_M(1), LF_V, "second split holds one quad", ld={"x": 136}),
    _lf("lf_m1_in400", 16, 400, 64, 2, LF_M(1), LF_V, "four splits, the last 16 rows", ld={"x": 404}),
    _lf("lf_m2_in144", 13, 144, 128, 1, LF_M(2), LF_V, "Q = 2, N = 13", ld={"x": 148}),
    _lf("lf_m2_in260", 16, 260, 128, 2, LF_M(2), LF_V, "Q = 2, two matrices, last split one quad", ld={"x": 264}),
]
for _ns in (1, 16, 17, 49, 64, 65, 130):
    LONG_FWD_CASES.append(_lf("lf_final_v_ns%d" % _ns, 2, 128 * _ns - 3, 4, 1, LF_V, why="final kernel over %d splits" % _ns))
    LONG_FWD_CASES.append(_lf("lf_final_g_ns%d" % _ns, 3, 128 * _ns - 3, 5, 2, LF_G, why="final kernel over %d splits, 2 matrices" % _ns))


def _lb(name, N, in_, out, nmat, want, want0=None, why="", **kw):
    return _case("long_bwd", name, N, in_, out, (want,), None if want0 is None else (want0,), why, nmat=nmat, **kw)


LONG_BWD_CASES = [
    _lb("lb_g_n17", 17, 37, 5, 1, LB_G, why="two sample groups past 16, ragged everything"),
    _lb("lb_g_n58", 58, 130, 64, 2, LB_G, why="largest batch inside the generic kernel's 60 KB for out = 64, nmat = 2"),
    _lb("lb_g_nodw0", 3, 65, 70, 2, LB_G, why="dW[0] = NULL, second block of one row", null=("dW0",)),
    _lb("lb_g_nodb1", 16, 200, 5, 2, LB_G, why="db[1] = NULL", null=("db1",)),
    _lb("lb_g_nodx", 17, 64, 128, 1, LB_G, why="dx = NULL, two column tiles", null=("dx",)),
    _lb("lb_g_dxonly", 1, 130, 70, 1, LB_G, why="dx only", null=("dW0", "db0")),
    _lb("lb_g_n58_out20", 58, 65, 20, 2, LB_G, why="only N > 16 keeps this off v4", null=("dW1", "db0")),
    _lb("lb_g_dw_off", 4, 65, 64, 1, LB_G, why="dW[0] off a 16-byte boundary", off=("dW0",)),
    _lb("lb_g_w1_off", 4, 64, 64, 2, LB_G, why="W[1] off a 16-byte boundary", off=("W1",)),
    _lb("lb_v_n1", 1, 37, 20, 1, LB_V, why="one sample, one short block"),
    _lb("lb_v_nodw1", 3, 64, 20, 2, LB_V, why="dW[1] = NULL", null=("dW1",)),
    _lb("lb_v_nodb0", 16, 65, 20, 2, LB_V, why="db[0] = NULL, second block of one row", null=("db0",)),
    _lb("lb_v_out128x2", 16, 130, 128, 2, LB_V, why="out = 128 with two matrices: m16 is refused"),
    _lb("lb_v_out68", 16, 200, 68, 1, LB_V, why="two column passes, the second with one quad"),
    _lb("lb_v_g0_off", 3, 200, 64, 1, LB_V, why="m16 -> v4: g[0] offset by one float", off=("g0",)),
    _lb("lb_v_g1_off", 16, 130, 64, 2, LB_V, why="m16 -> v4: g[1] offset by one float, no dx", off=("g1",), null=("dx",)),
    _lb("lb_v_dxonly", 13, 64, 128, 2, LB_V, why="dx only", null=("dW0", "dW1", "db0", "db1")),
    _lb("lb_v_f1_nmat1", 16, 130, 64, 1, LB_V, why="in % 4 != 0 with a dx: the MFMA kernel's float4 dx store would cross in", ld={"dx": 132}),
    _lb("lb_v_f1_nmat2", 16, 130, 64, 2, LB_V, why="the same with two matrices", ld={"dx": 132}),
    _lb("lb_v_f1_in6", 3, 6, 64, 1, LB_V, why="the same at in = 6", ld={"dx": 8}),
    _lb("lb_v_dx_off", 4, 64, 64, 1, LB_V, why="m16 -> v4: dx off a 16-byte boundary", off=("dx",)),
    _lb("lb_v_lddx_odd", 4, 64, 64, 1, LB_V, why="m16 -> v4: lddx % 4", ld={"dx": 65}),
    _lb("lb_m11_n1", 1, 64, 64, 1, LB_M(1, 1), LB_V, "one sample, half a block of rows"),
    _lb("lb_m11_nodw", 16, 200, 64, 1, LB_M(1, 1), LB_V, "dW = NULL; second block of 72 rows", null=("dW0",), ld={"x": 204, "dx": 204}),
    _lb("lb_m11_in37_nodx", 16, 37, 64, 1, LB_M(1, 1), LB_V, "in % 4 != 0 without dx stays on m16: the row < in guard", null=("dx",)),
    _lb("lb_m12_all", 16, 200, 64, 2, LB_M(1, 2), LB_V, "the shipped form at a small in"),
    _lb("lb_m12_nodb1", 3, 64, 64, 2, LB_M(1, 2), LB_V, "db[1] = NULL", null=("db1",)),
    _lb("lb_m12_in130_nodx", 16, 130, 64, 2, LB_M(1, 2), LB_V, "in % 4 != 0 without dx", null=("dx",)),
    _lb("lb_m12_nodw1", 13, 64, 64, 2, LB_M(1, 2), LB_V, "dW[1] = NULL", null=("dW1",), ld={"dx": 68}),
    _lb("lb_m21_all", 16, 200, 128, 1, LB_M(2, 1), LB_V, "Q = 2"),
    _lb("lb_m21_nodx", 3, 65, 128, 1, LB_M(2, 1), LB_V, "Q = 2, dx = NULL, last step one row", null=("dx",)),
    _lb("lb_m21_nodb", 1, 64, 128, 1, LB_M(2, 1), LB_V, "Q = 2, db = NULL", null=("db0",)),
]

WIDE_FWD_CASES = []
for _act in range(4):
    for _n, _N, _in, _out, _want, _want0, _ld, _why in [
            ("g_n17", 17, 50, 301, WF_G, None, {}, "two sample passes, two column blocks"),
            ("g_n64", 64, 9, 257, WF_G, None, {}, "four sample passes, second block of one column"),
            ("g_out1030", 3, 50, 1030, WF_G, None, {}, "out % 4 != 0 at N <= 16, five blocks"),
            ("v_in3", 1, 3, 132, WF_V, None, {}, "fewer rows than the eight row groups; second block one quad"),
            ("v_out260", 16, 50, 260, WF_V, None, {}, "three blocks, the last one quad"),
            ("v_ldx_odd", 9, 128, 192, WF_V, None, {"x": 129}, "m16 shape pushed to v4 by ldx % 4"),
            ("m1_n1", 1, 64, 64, WF_M(1), WF_V, {"y": 68}, "NR = 1, one sample, one block"),
            ("m2_out192", 3, 128, 192, WF_M(2), WF_V, {"y": 196}, "NR = 2"),
            ("m4_out128", 16, 256, 128, WF_M(4), WF_V, {"y": 132}, "NR = 4: in = 256"),
            ("m1_out320", 13, 64, 320, WF_M(1), WF_V, {"y": 324}, "five blocks, N = 13")]:
        WIDE_FWD_CASES.append(_case("wide_fwd", "wf_%s_act%d" % (_n, _act), _N, _in, _out, (_want,), None if _want0 is None else (_want0,),
                                    _why, act=_act, ld=_ld))
WIDE_FWD_CASES += [
    _case("wide_fwd", "wf_m1_nob", 1, 64, 64, (WF_M(1),), (WF_V,), "b = NULL", act=1, null=("b",), ld={"y": 68}),
    _case("wide_fwd", "wf_m2_nob", 3, 128, 192, (WF_M(2),), (WF_V,), "b = NULL", act=2, null=("b",), ld={"y": 196}),
    _case("wide_fwd", "wf_m4_nob", 16, 256, 128, (WF_M(4),), (WF_V,), "b = NULL", act=3, null=("b",), ld={"y": 132}),
    _case("wide_fwd", "wf_m1_out320_nob", 13, 64, 320, (WF_M(1),), (WF_V,), "b = NULL", act=0, null=("b",), ld={"y": 324}),
    _case("wide_fwd", "wf_g_nob", 17, 50, 301, (WF_G,), None, "b = NULL on the generic kernel", act=1, null=("b",)),
    _case("wide_fwd", "wf_v_nob", 16, 50, 260, (WF_V,), None, "b = NULL on v4", act=3, null=("b",), ld={"x": 53, "y": 261}),
    _case("wide_fwd", "wf_v_y_off", 4, 64, 64, (WF_V,), None, "m16 -> v4: y off a 16-byte boundary", act=1, off=("y",)),
    _case("wide_fwd", "wf_v_b_off", 4, 64, 64, (WF_V,), None, "m16 -> v4: b off a 16-byte boundary", act=1, off=("b",)),
    _case("wide_fwd", "wf_v_x_off", 4, 128, 64, (WF_V,), None, "m16 -> v4: x off a 16-byte boundary", act=2, off=("x",)),
    _case("wide_fwd", "wf_v_ldy_odd", 4, 64, 128, (WF_V,), None, "m16 -> v4: ldy % 4", act=1, ld={"y": 129}),
    _case("wide_fwd", "wf_g_w_off", 4, 64, 64, (WF_G,), None, "W off a 16-byte boundary", act=1, off=("W",)),
    _case("wide_fwd", "wf_g_n17_in64", 17, 64, 64, (WF_G,), None, "only N > 16 keeps this off the tiled kernels", act=1),
]


def _wb(name, N, in_, out, act, dw, dx, dw0=None, dx0=None, why="", which=("dW", "db", "dx"), **kw):
    """``dw`` / ``dx``: the kernels of the two halves (None: that half is not asked for; ``dx0 = "refused"``: without the MFMA
    tier neither dx kernel has the LDS for in = 256, and the whole call is refused before any launch)."""
    null = set(kw.pop("null", ())) | ({"dW", "db", "dx"} - set(which))
    if act == 0 and kw.pop("noy", False):
        null.add("y")
    build = lambda a, b: EINVAL if b == "refused" else tuple(([a] if a else []) + ([b, DXFINAL] if b else []))
    return _case("wide_bwd", name, N, in_, out, build(dw, dx), build(dw0 or dw, dx0 or dx), why, act=act, null=null, **kw)


def _wide_ld(in_, out, **extra):
    """ldg, ldy, lddx larger than needed."""
    ld = {"g": out + 4, "y": out + 8, "dx": in_ + 4}
    ld.update(extra)
    return ld


WIDE_BWD_CASES = [
    _wb("wb_g_n17", 17, 50, 301, 1, DW_G, DX_G, why="two sample passes; five chunks, the last 45 columns"),
    _wb("wb_g_n36_in200", 36, 200, 70, 2, DW_G, DX_G, why="largest batch inside the generic dx kernel's 60 KB at in = 200"),
    _wb("wb_g_in3", 3, 3, 257, 3, DW_G, DX_G, why="out % 4 and in % 4 both != 0 at N <= 16", ld={"g": 258, "y": 259, "dx": 5}),
    _wb("wb_g_n17_in64", 17, 64, 192, 0, DW_G, DX_G, why="only N > 16 keeps both halves off the tiled kernels", noy=True),
    _wb("wb_g_n36_dxonly", 36, 128, 64, 1, None, DX_G, why="dx only", which=("dx",)),
    _wb("wb_g_n17_dwonly", 17, 50, 301, 2, DW_G, None, why="dW only", which=("dW",)),
    _wb("wb_g_n17_dbonly", 17, 50, 301, 3, DW_G, None, why="db only", which=("db",)),
    _wb("wb_g_n1", 1, 50, 70, 1, DW_G, DX_G, why="one sample"),
    _wb("wb_v_n1_in200", 1, 200, 132, 1, DW_V, DX_V, why="one sample; three chunks, the last 4 columns", ld=_wide_ld(200, 132)),
    _wb("wb_v_in3", 16, 3, 260, 2, DW_V, DX_G, why="fewer weight rows than the four gridDim.y slices; dx generic by in % 4"),
    _wb("wb_v_in50", 3, 50, 132, 3, DW_V, DX_G, why="in = 50: slices of 13, 13, 13, 11 rows", ld=_wide_ld(50, 132)),
    _wb("wb_v_dwonly", 16, 64, 132, 0, DW_V, None, why="dW only", which=("dW",), noy=True),
    _wb("wb_v_dbonly", 16, 64, 132, 1, DW_V, None, why="db only: gridDim.y = 1", which=("db",)),
    _wb("wb_v_dxonly", 16, 64, 132, 2, None, DX_V, why="dx only", which=("dx",)),
    _wb("wb_v_in200_n16", 16, 200, 260, 0, DW_V, DX_V, why="in = 200 at the full tile: 55 KB of LDS for the dx kernel"),
    _wb("wb_v_in256_nodx", 16, 256, 132, 2, DW_V, None, why="in = 256 off the MFMA shape: no dx, so no LDS refusal", which=("dW", "db")),
    _wb("wb_vm_ldx_odd", 9, 128, 192, 1, DW_V, DX_M(2), DW_V, DX_V, "ldx % 4 pushes only the dW half to v4", ld={"x": 129}),
    _wb("wb_gv_ldg_odd", 3, 128, 192, 1, DW_G, DX_V, why="ldg % 4 pushes dW to generic and dx to v4", ld={"g": 193}),
    _wb("wb_gv_ldy_odd", 3, 128, 192, 2, DW_G, DX_V, why="ldy % 4 under an activation does the same", ld={"y": 193}),
    _wb("wb_m_ldy_odd_act0", 3, 128, 192, 0, DW_M(2), DX_M(2), DW_V, DX_V, "ldy % 4 is ignored without an activation", ld={"y": 193}),
    _wb("wb_mv_w_off", 4, 64, 64, 1, DW_M(1), DX_V, DW_V, DX_V, "W off a 16-byte boundary: only dx needs it", off=("W",)),
    _wb("wb_vg_ws_off", 4, 52, 132, 1, DW_V, DX_G, why="workspace off a 16-byte boundary", off=("ws",)),
    _wb("wb_g_dw_off", 4, 64, 64, 2, DW_G, DX_M(1), DW_G, DX_V, "dW off a 16-byte boundary", off=("dW",)),
    _wb("wb_g_db_off", 4, 64, 64, 3, DW_G, DX_M(1), DW_G, DX_V, "db off a 16-byte boundary", off=("db",)),
    _wb("wb_m1_n1", 1, 64, 64, 1, DW_M(1), DX_M(1), DW_V, DX_V, "NR = 1, one sample, ONE chunk: the block's second chunk is off",
        ld=_wide_ld(64, 64)),
    _wb("wb_m2_out192", 3, 128, 192, 2, DW_M(2), DX_M(2), DW_V, DX_V, "NR = 2, three chunks", ld=_wide_ld(128, 192)),
    _wb("wb_m4_out320", 16, 256, 320, 3, DW_M(4), DX_M(4), DW_V, "refused", "NR = 4 (in = 256), five chunks", ld=_wide_ld(256, 320)),
    _wb("wb_m1_out320_noy", 13, 64, 320, 0, DW_M(1), DX_M(1), DW_V, DX_V, "no activation, y = NULL, N = 13", noy=True),
    _wb("wb_m1_out8320", 16, 64, 64 * 130, 1, None, DX_M(1), None, DX_V, "65 slabs: the final kernel's unrolled loop", which=("dx",)),
    _wb("wb_m2_dwonly", 16, 128, 128, 3, DW_M(2), None, DW_V, None, "dW only", which=("dW",)),
    _wb("wb_m2_dbonly", 16, 128, 128, 1, DW_M(2), None, DW_V, None, "db only", which=("db",)),
    _wb("wb_m4_dxonly", 16, 256, 128, 2, None, DX_M(4), None, "refused", "dx only, an even number of chunks", which=("dx",)),
    _wb("wb_m4_n3", 3, 256, 64, 1, DW_M(4), DX_M(4), DW_V, "refused", "NR = 4 at N = 3, one chunk"),
]
for _c in (1, 17, 49, 65, 130):
    WIDE_BWD_CASES.append(_wb("wb_g_chunks%d" % _c, 3, 5, 64 * _c - 3, 1 + _c % 3, DW_G if _c < 49 else None, DX_G,
                              why="generic dx over %d chunks, the last 61 columns" % _c,
                              which=("dW", "db", "dx") if _c < 49 else ("dx",)))

TABLES = {"long_fwd": LONG_FWD_CASES, "long_bwd": LONG_BWD_CASES, "wide_fwd": WIDE_FWD_CASES, "wide_bwd": WIDE_BWD_CASES}
ALL_CASES = [c for t in TABLES.values() for c in t]


# ----------------------------------------------------------------------------------------------------- inputs
def _rng(c, salt=0):
    return np.random.default_rng(zlib.crc32(c["name"].encode()) + salt)


def _y_for(rng, shape, act):
    """A ``y`` a forward could have written: never exactly 0 under leaky / relu; |y| <= tanh(1.25) under tanh, so that the
    cancellation in 1 - y^2 (one float32 rounding of y^2 against a result >= 0.28) stays far inside the sum bar."""
    v = rng.standard_normal(shape).astype(np.float32)
    if act == 3:
        return np.tanh(np.clip(v, -1.25, 1.25)).astype(np.float32)
    v[v == 0] = np.float32(0.5)
    return v


def inputs(c):
    """The arrays of a case (float32, dense), seeded by its name."""
    rng = _rng(c)
    N, in_, out, nmat = c["N"], c["in_"], c["out"], c["nmat"]
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    d = {"x": f(N, in_)}
    if c["entry"] in ("long_fwd", "long_bwd"):
        for m in range(nmat):
            d["W%d" % m] = f(in_, out)
            if c["entry"] == "long_fwd":
                d["b%d" % m] = None if ("b%d" % m) in c["null"] else f(out)
            else:
                d["g%d" % m] = f(N, out)
        return d
    d["W"] = (f(in_, out) / np.float32(np.sqrt(in_))).astype(np.float32)
    if c["entry"] == "wide_fwd":
        d["b"] = None if "b" in c["null"] else f(out)
    else:
        d["g"] = f(N, out)
        d["y"] = None if "y" in c["null"] else _y_for(rng, (N, out), c["act"])
    return d


def reference(c, d, T):
    """dict name -> (value, sum |terms|) of the outputs the case asks for."""
    nmat = c["nmat"]
    if c["entry"] == "long_fwd":
        r = long_fwd_ref(d["x"], [d["W%d" % m] for m in range(nmat)], [d["b%d" % m] for m in range(nmat)], T)
        return {"y%d" % m: r[m] for m in range(nmat)}
    if c["entry"] == "long_bwd":
        r = long_bwd_ref(d["x"], [d["W%d" % m] for m in range(nmat)], [d["g%d" % m] for m in range(nmat)], T)
        return {k: v for k, v in r.items() if k not in c["null"]}
    if c["entry"] == "wide_fwd":
        return {"y": wide_fwd_ref(d["x"], d["W"], d["b"], c["act"], T)}
    r = wide_bwd_ref(d["x"], d["g"], d["y"], c["act"], d["W"], T)
    return {k: v for k, v in r.items() if k not in c["null"]}


def uses_element_bar(c):
    """Wide y behind an activation is held to element_bar; every other output is a bare contraction: sum_bar."""
    return c["entry"] == "wide_fwd" and c["act"] != 0
