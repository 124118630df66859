"""The group-norm kernels of csrc/groupnorm.hip on their own, against float64 restatements (tests/gn_cases.py), through the C entry
points ``cape_groupnorm_fwd`` / ``cape_groupnorm_bwd`` / ``cape_groupnorm_param_reduce_batch`` at the smallest shapes that reach
every row-chunk form of the partial-sum pass, every form of the apply pass and every edge of a channel quad; then the autograd
wrapper ``ops.GroupNormFn`` on its deferred and pass-through paths.

Every operand is a window of a larger buffer: its own leading dimension above round_up(C, 4), its own sample stride above
V * ld.  The pad lanes and all slack of x, dy, dx_add (and what surrounds gamma / beta) are NaN (-1e30 in the two ``bigpad``
cases: fmaxf would drop a NaN from a row bound even where the code forgot that the lane does not count); the pad lanes and all slack of
y, dx, and everything around stats, coef, bcoef, the partials, the workspace and rowmax_out hold a sentinel that must keep its
bits.  Every case runs twice on fresh buffers and gives the same bits.  y, stats, coef, dx, bcoef are held to
kernel_bars.element_bar against the float32 two-pass restatement, dgamma_partial / dbeta_partial per element to
kernel_bars.sum_bar; the backward reference takes ``y_dev > 0`` as its ReLU mask.  rowmax_out[:, 0] equals max_c |stored row|
bit for bit in all three forms, entries 1..3 are +0.  tests/test_gn_cases_host.py proves the table on the CPU.

Measured on an MI355X, worst error in units of the bar (element_bar: error over max(4 x the float32 restatement's error,
4 * 2^-24); sum_bar: over 2e-6 sum |terms|), equal to three digits to the emulation of tests/gn_cases.py:
  partial-sum pass   RB = 16: 0.477 (bcoef, offset_rb16), sums 0.073    RB = 32: 0.193 (dx, rb32_v97), sums 0.147
                     RB = 64: 0.249 (dx, offset_rb64), sums 0.193        RB = 128: 0.243 (dx, cap_fused), sums 0.206
  apply pass         plain 0.332 (y, c3_g3_norm)   fused 0.477 (bcoef, offset_rb16)   rows 0.264 (y, c38_g2_rm)
                     standalone 0.186 (dx, c1028_g257_rm_norelu_add); the constant group's y: 0.298 of its derived bound
Row 0 as an outlier: with the float64 statistics every k in 4, 16, 64, 256 holds the bar at every chunk form (stats at most 0.13
of it).  With the float32 sums the kernel had before, the same cases gave on the MI355X: RB = 16 held k = 4 (0.61) and missed
k = 16 by 1.8 x (5.8e-7); RB = 32, 64 and 128 missed k = 4 already, by 1.9 x, 2.6 x and 2.7 x (9.5e-7, 1.3e-6, 1.7e-6); the
worst was 1.1e-5 (15 x) at k = 16, RB = 128; and six cases of unit-normal data missed too (rb64_v65, rb128_v130 by 4.2 x,
rb128_c4, cap_plain, cap_fused, c4_g4_norm).

Changed on a scratch build, arithmetic only, and caught by: pivot forced to 0 in gn_stat_partial_kernel -- 78 tests, every
offset_* among them; the 2 dp S term dropped in gn_final_kernel -- 77; the lane sum started at l = 2, forward or backward -- 77
each; ``>= 0`` in the backward's mask -- gamma0_c8 and gamma0_c96; gn_quad_bound ignoring ``left`` -- c6_g2_rm_bigpad and
c38_g2_rm_bigpad (NaN pads cannot show it: fmaxf drops them wherever they enter)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gn_cases as GN
import parity_bar
from kernel_bars import element_bar, sum_bar, same_bits, bits, mat_err, TOL

pytestmark = pytest.mark.gpu

SENT = np.float32(-31337.5)
NAN = np.float32(np.nan)
BIG = np.float32(-1e30)
EINVAL, EWORKSPACE = -1, -4
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class Win:
    """A window of ``shape`` with ``strides`` (in floats) inside a 1-D device buffer: 4 floats in front of it, 8 behind its last
    element, everything outside the window = ``pad``."""

    def __init__(self, dev, shape, strides=None, data=None, pad=SENT):
        shape = tuple(int(s) for s in shape)
        if strides is None:
            strides = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
        idx = np.full(shape, 4, np.int64)
        for ax, (n, st) in enumerate(zip(shape, strides)):
            idx += (np.arange(n, dtype=np.int64) * st).reshape([-1 if a == ax else 1 for a in range(len(shape))])
        host = np.full(int(idx.max()) + 1 + 8, pad, np.float32)
        self.idx = idx
        self.outside = np.ones(host.size, bool)
        self.outside[idx.reshape(-1)] = False
        assert int((~self.outside).sum()) == idx.size                          # (no two elements share a slot)
        if data is not None:
            host[idx] = np.asarray(data, np.float32).reshape(shape)
        self.pad_bits = bits(np.full(1, pad, np.float32))[0]
        self.buf = torch.from_numpy(host).to(dev)
        self.t = self.buf[4:]
        assert self.t.data_ptr() % 16 == 0

    def read(self):
        """(the window, whether everything outside it kept its bits)"""
        host = self.buf.cpu().numpy()
        return host[self.idx].copy(), bool((bits(host[self.outside]) == self.pad_bits).all())

    def untouched(self):
        return bool((bits(self.buf.cpu().numpy()) == self.pad_bits).all())


def _act(dev, c, extra, data=None, pad=SENT):
    """[N, V, C] with ld = round_up(C, 4) + extra and a sample stride of V * ld + extra (both multiples of 4)."""
    ld = GN.pad4(c["C"]) + extra
    ss = c["V"] * ld + extra
    w = Win(dev, (c["N"], c["V"], c["C"]), (ss, ld, 1), data=data, pad=pad)
    w.ld, w.ss = ld, ss
    return w


def _table(dev, c, k):
    Cp = GN.pad4(c["C"])
    return Win(dev, (c["N"], k, c["C"]), (k * Cp, Cp, 1))


FWD_OUT, BWD_OUT = ("y", "stats", "coef", "ws", "rm"), ("dx", "dgamma_p", "dbeta_p", "bcoef", "ws2", "rm2")


def execute(dev, c, d, fwd=None, bwd=None):
    """One forward and -- when it returned 0 -- one backward on fresh buffers.  ``fwd`` / ``bwd``: what to falsify in that CALL
    (the buffers stay those of the case): ``over`` scalar arguments, ``null`` pointers passed as NULL, ``off`` pointers moved by
    four bytes.  Returns (rc_fwd, rc_bwd or None, {name: Win})."""
    from cape_amd import ops
    lib, S = ops.lib, ops._stream
    N, V, Cn, G = c["N"], c["V"], c["C"], c["G"]
    need = GN.workspace_bytes(N, V, Cn)
    assert int(lib.cape_groupnorm_workspace_bytes(N, V, Cn)) == need
    PAD = BIG if c["pad"] == "big" else NAN
    w = dict(x=_act(dev, c, 4, d["x"], PAD), gamma=Win(dev, (Cn,), data=d["gamma"], pad=NAN), beta=Win(dev, (Cn,), data=d["beta"], pad=NAN),
             y=_act(dev, c, 8), stats=Win(dev, (N, G, 2)), coef=_table(dev, c, 4), ws=Win(dev, (need // 4,)),
             rm=Win(dev, (N * V, 4)) if c["rm"] else None)

    def ptr(t, name):
        if name in t.get("null", ()) or w[name] is None:
            return None
        return ops._ptr(w[name].t, 1 if name in t.get("off", ()) else 0)

    t = dict(fwd or {})
    a = dict(xs=w["x"].ss, ldx=w["x"].ld, ys=w["y"].ss, ldy=w["y"].ld, G=G, N=N, V=V, C=Cn, ws_bytes=need)
    a.update(t.get("over", {}))
    rc = int(lib.cape_groupnorm_fwd(ptr(t, "x"), a["xs"], a["ldx"], ptr(t, "gamma"), ptr(t, "beta"), float(GN.EPS), a["G"], c["relu"],
                                    ptr(t, "y"), a["ys"], a["ldy"], ptr(t, "stats"), ptr(t, "coef"), a["N"], a["V"], a["C"],
                                    ptr(t, "ws"), a["ws_bytes"], ptr(t, "rm"), S()))
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, w
    w.update(dy=_act(dev, c, 12, d["dy"], PAD), add=_act(dev, c, 8, d["add"], PAD) if c["add"] else None, dx=_act(dev, c, 4),
             dgamma_p=Win(dev, (N, Cn)), dbeta_p=Win(dev, (N, Cn)), bcoef=_table(dev, c, 3), ws2=Win(dev, (need // 4,)),
             rm2=Win(dev, (N * V, 4)) if c["rm"] else None)
    t = dict(bwd or {})
    a = dict(xs=w["x"].ss, ldx=w["x"].ld, dys=w["dy"].ss, lddy=w["dy"].ld, dxs=w["dx"].ss, lddx=w["dx"].ld,
             adds=w["add"].ss if c["add"] else 0, ldadd=w["add"].ld if c["add"] else 0, G=G, N=N, V=V, C=Cn, ws_bytes=need)
    a.update(t.get("over", {}))
    rcb = int(lib.cape_groupnorm_bwd(ptr(t, "x"), a["xs"], a["ldx"], ptr(t, "dy"), a["dys"], a["lddy"], ptr(t, "gamma"), ptr(t, "stats"),
                                     ptr(t, "coef"), a["G"], c["relu"], ptr(t, "dx"), a["dxs"], a["lddx"], ptr(t, "add"), a["adds"],
                                     a["ldadd"], ptr(t, "dgamma_p"), ptr(t, "dbeta_p"), ptr(t, "bcoef"), a["N"], a["V"], a["C"],
                                     ptr(t, "ws2"), a["ws_bytes"], ptr(t, "rm2"), S()))
    torch.cuda.synchronize()
    return rc, rcb, w


# ------------------------------------------------------------------------------------------------- the table of cases
_FWD_REFS, _BWD_REFS = {}, {}
FIGURES = {}                     # (what the case reaches, quantity) -> (worst figure in units of its bar, case)


def _forward_refs(c, d):
    key = (c["seed"], c["relu"])
    if key not in _FWD_REFS:
        _FWD_REFS.clear()                                                       # (one set of large arrays at a time)
        _FWD_REFS[key] = tuple(GN.forward_ref(d["x"], d["gamma"], d["beta"], c["G"], c["relu"], T) for T in (F64, F32))
    return _FWD_REFS[key]


def _backward_refs(c, d, f64, f32, mask):
    key = (c["seed"], c["relu"], c["add"])
    hit = _BWD_REFS.get(key)
    if hit is None or not (mask is None or np.array_equal(hit[0], mask)):
        _BWD_REFS.clear()
        hit = (mask,) + tuple(GN.backward_ref(d["x"], d["dy"], d["gamma"], f["stats"], c["G"], mask, d["add"], T) for f, T in ((f64, F64), (f32, F32)))
        _BWD_REFS[key] = hit
    return hit[1], hit[2]


def _note(c, quantity, fig):
    p = GN.case_plan(c)
    for what in ("RB = %d" % p["RB"], "apply: " + p["form"]):
        if fig >= FIGURES.get((what, quantity), (-1.0, ""))[0]:
            FIGURES[(what, quantity)] = (fig, c["name"])


def run_case(dev, c, judge=True):
    """The case twice; every check of the module docstring.  Returns (failures, {quantity: error in units of its bar})."""
    d = GN.inputs(c)
    fails, figs = [], {}
    rc, rcb, w = execute(dev, c, d)
    rc2, rcb2, w2 = execute(dev, c, d)
    if (rc, rcb, rc2, rcb2) != (0, 0, 0, 0):
        return ["%s: rc %s %s / %s %s (%s)" % (c["name"], rc, rcb, rc2, rcb2, c["why"])], figs
    got = {}
    for k in FWD_OUT + BWD_OUT:
        if w[k] is None:
            continue
        v, ok = w[k].read()
        v2, ok2 = w2[k].read()
        if not (ok and ok2):
            fails.append("%s / %s: wrote outside its window (%s)" % (c["name"], k, c["why"]))
        if k not in ("ws", "ws2"):
            got[k] = v
            if not np.isfinite(v).all():
                fails.append("%s / %s: %d values are not finite (a pad lane leaked)" % (c["name"], k, int((~np.isfinite(v)).sum())))
            if not same_bits(v, v2):
                fails.append("%s / %s: two runs differ" % (c["name"], k))
    if fails:
        return fails, figs
    # ---- row bounds: bit for bit the largest magnitude of the row as stored
    for rk, ok_ in (("rm", "y"), ("rm2", "dx")):
        if w[rk] is None:
            continue
        want = np.abs(got[ok_]).max(axis=2).reshape(-1)
        if not same_bits(got[rk][:, 0].copy(), want):
            bad = np.flatnonzero(bits(got[rk][:, 0].copy()) != bits(want))
            fails.append("%s / %s: %d of %d row bounds are not max |row| (first: row %d has %r, its row %r)"
                         % (c["name"], rk, bad.size, want.size, bad[0], got[rk][bad[0], 0], want[bad[0]]))
        if bits(got[rk][:, 1:].copy()).any():
            fails.append("%s / %s: entries 1..3 are not +0" % (c["name"], rk))
    # ---- the bars
    f64, f32 = _forward_refs(c, d)
    mask = (got["y"] > 0) if c["relu"] else None
    b64, b32 = _backward_refs(c, d, f64, f32, mask)
    dfwd = dict(y=got["y"], stats=got["stats"], coef=got["coef"])
    dbwd = dict(dx=None if c["add"] else got["dx"], dx_add=got["dx"] if c["add"] else None, bcoef=got["bcoef"])
    q64, q32, qd = GN.split(c, f64, b64), GN.split(c, f32, b32), GN.split(c, dfwd, dbwd)
    for k in sorted(q64):
        if k == ("dx_add" if not c["add"] else "dx"):
            continue
        e, e32 = mat_err(qd[k], q64[k]), mat_err(q32[k], q64[k])
        figs[k] = e / min(max(4.0 * e32, parity_bar.FLOOR), TOL)
        print("%s / %s: error %.2e, float32 restatement %.2e: %.2f of the bar" % (c["name"], k, e, e32, figs[k]))
        if judge:
            try:
                element_bar("groupnorm", "%s / %s" % (c["name"], k), qd[k], q32[k], q64[k])
            except AssertionError as e_:
                fails.append("%s / %s (%s): %s" % (c["name"], k, c["why"], str(e_)[:300]))
    for k in GN.SUM_QUANTITIES:
        scale = b64[k.replace("_p", "_abs")]
        figs[k] = GN.sum_fraction(got[k], b64[k], scale)
        if judge:
            try:
                sum_bar("groupnorm", "%s / %s" % (c["name"], k), got[k], b64[k], scale, f32=b32[k])
            except AssertionError as e_:
                fails.append("%s / %s (%s): %s" % (c["name"], k, c["why"], str(e_)[:300]))
    # ---- what the special inputs are there for
    if c["data"] == "zerovar":
        n, g = GN.zerovar_where(c)
        if not (got["stats"][n, g, 0] == GN.ZV_CONST and got["stats"][n, g, 1] == GN.ZV_RSTD):
            fails.append("%s: stats of the constant group are %r, not (%r, %r)" % (c["name"], got["stats"][n, g], GN.ZV_CONST, GN.ZV_RSTD))
        else:
            for k, v in GN.zerovar_fractions(c, d, dfwd, dbwd, b64["dgamma_abs"]).items():
                figs[k] = v
                if not v <= 1.0:
                    fails.append("%s / %s: %.3f of its derived bound" % (c["name"], k, v))
    if c["data"] == "gamma0":
        c0, c1 = GN.gamma0_channels(c)
        if bits(got["y"][:, :, c0].copy()).any() or not (got["y"][:, :, c1] == d["beta"][c1]).all():
            fails.append("%s: y of the gamma = 0 channels is not (+0, beta)" % c["name"])
        if bits(got["dbeta_p"][:, c0].copy()).any() or bits(got["dgamma_p"][:, c0].copy()).any():
            fails.append("%s: the channel with y = 0 everywhere has parameter gradients %r / %r (mask at exactly 0)"
                         % (c["name"], got["dgamma_p"][:, c0], got["dbeta_p"][:, c0]))
    if c["data"] == "relurow":
        r = GN.relu_row(c)
        rows = got["rm"].reshape(c["N"], c["V"], 4)[:, r, 0]
        if bits(got["y"][:, r, :].copy()).any() or bits(rows.copy()).any():
            fails.append("%s: the row ReLU switches off is not +0 with bound +0" % c["name"])
    for k, v in figs.items():
        _note(c, k, v)
    return fails, figs


@pytest.mark.parametrize("c", GN.ALL_CASES, ids=lambda c: c["name"])
def test_case(dev, c):
    """One case of the table: everything the module docstring lists."""
    fails, figs = run_case(dev, c)
    print("%s: %s" % (c["name"], "  ".join("%s %.2f" % kv for kv in sorted(figs.items()))))
    assert not fails, "\n".join(fails)


def test_print_the_worst_figure_of_every_form(dev):
    assert FIGURES, "runs after test_case"
    for (what, k), (v, name) in sorted(FIGURES.items()):
        print("WORST %-18s %-10s %.3f of its bar at %s" % (what, k, v, name))


# ------------------------------------------------------------------------------------------------- parameter reduction
def _seq_sum(p):
    """float32 sum over axis 0 in index order"""
    s = np.zeros(p.shape[1:], F32)
    for n in range(p.shape[0]):
        s = (s + p[n]).astype(F32)
    return s


def _reduce(dev, shapes, seed):
    """cape_groupnorm_param_reduce_batch over items of the given (N, C); every output [C] lies 8 floats from the next one in ONE
    buffer of sentinels."""
    from cape_amd import ops, _lib
    rng = np.random.default_rng(seed)
    parts = [((rng.standard_normal((N, Cn)) * 10 ** rng.uniform(-2, 2)).astype(F32), rng.standard_normal((N, Cn)).astype(F32)) for N, Cn in shapes]
    offs, o = [], 8
    for N, Cn in shapes:
        offs.append((o, o + Cn + 8))
        o += 2 * (Cn + 8)
    out = torch.full((o,), float(SENT), device=dev)
    devp = [(Win(dev, pg.shape, data=pg, pad=NAN), Win(dev, pb.shape, data=pb, pad=NAN)) for pg, pb in parts]
    arr = (_lib.CapeGnParamItem * len(shapes))()
    for a, (N, Cn), (og, ob), (wg, wb) in zip(arr, shapes, offs, devp):
        a.dgamma_partial, a.dbeta_partial = wg.t.data_ptr(), wb.t.data_ptr()
        a.dgamma, a.dbeta = out.data_ptr() + 4 * og, out.data_ptr() + 4 * ob
        a.N, a.C = N, Cn
    rc = int(ops.lib.cape_groupnorm_param_reduce_batch(C.addressof(arr), len(shapes), ops._stream()))
    torch.cuda.synchronize()
    assert rc == 0
    host = out.cpu().numpy()
    keep = np.ones(o, bool)
    for (N, Cn), (og, ob), (pg, pb) in zip(shapes, offs, parts):
        for off, p in ((og, pg), (ob, pb)):
            assert same_bits(host[off:off + Cn].copy(), _seq_sum(p)), (N, Cn)
            keep[off:off + Cn] = False
    assert (bits(host[keep]) == bits(np.full(1, SENT, F32))[0]).all(), "a neighbouring item's output was written beyond C"
    return arr, out


def test_param_reduce_is_the_sequential_float32_sum(dev):
    """One item, then 32 items of mixed C (1, 255, 256, 257, 600) and N (1, 3, 33) in one launch: bit-equal to the float32 sum in
    sample order, nothing written between the outputs."""
    _reduce(dev, [(3, 257)], 1)
    _reduce(dev, [(33, 600)], 2)
    Cs, Ns = (1, 255, 256, 257, 600), (1, 3, 33)
    shapes = [(Ns[(i * 2 + i // 5) % 3], Cs[i % 5]) for i in range(32)]
    assert {s for s in shapes} >= {(n, c_) for n in Ns for c_ in Cs}
    _reduce(dev, shapes, 3)


def test_param_reduce_refuses_bad_arguments(dev):
    from cape_amd import ops, _lib
    arr, out = _reduce(dev, [(3, 5)] * 2, 4)
    lib, S = ops.lib, ops._stream
    out.fill_(float(SENT))
    assert int(lib.cape_groupnorm_param_reduce_batch(None, 1, S())) == EINVAL
    assert int(lib.cape_groupnorm_param_reduce_batch(C.addressof(arr), 0, S())) == EINVAL
    big = (_lib.CapeGnParamItem * 33)(*([arr[0]] * 33))
    assert int(lib.cape_groupnorm_param_reduce_batch(C.addressof(big), 33, S())) == EINVAL
    for field in ("dgamma_partial", "dbeta_partial", "dgamma", "dbeta"):
        bad = (_lib.CapeGnParamItem * 2)(arr[0], arr[1])
        setattr(bad[1], field, None)
        assert int(lib.cape_groupnorm_param_reduce_batch(C.addressof(bad), 2, S())) == EINVAL, field
    for field in ("N", "C"):
        bad = (_lib.CapeGnParamItem * 2)(arr[0], arr[1])
        setattr(bad[1], field, 0)
        assert int(lib.cape_groupnorm_param_reduce_batch(C.addressof(bad), 2, S())) == EINVAL, field
    torch.cuda.synchronize()
    assert (bits(out.cpu().numpy()) == bits(np.full(1, SENT, F32))[0]).all()


# ------------------------------------------------------------------------------------------------- refused before any launch
def _refused(dev, c, d, which, rc_want=EINVAL, **t):
    rc, rcb, w = execute(dev, c, d, **{which: t})
    outs = FWD_OUT if which == "fwd" else BWD_OUT
    assert (rc if which == "fwd" else rcb) == rc_want, (c["name"], which, t, rc, rcb)
    for k in outs:
        assert w[k] is None or w[k].untouched(), (c["name"], which, t, k)


def test_entry_points_refuse_bad_arguments(dev):
    """Every documented refusal of cape_groupnorm_fwd / _bwd: the code, and every output buffer still full of the sentinel."""
    c = GN.by_name("c12_g4_rm_norelu_add")
    d = GN.inputs(c)
    rc, rcb, w = execute(dev, c, d)
    assert (rc, rcb) == (0, 0) and not w["y"].untouched() and not w["dx"].untouched()          # (the base case is accepted)
    Cn, need = c["C"], GN.workspace_bytes(c["N"], c["V"], c["C"])
    for name in ("x", "gamma", "beta", "y", "stats", "coef", "ws"):
        _refused(dev, c, d, "fwd", null=(name,))
    for name in ("x", "dy", "gamma", "stats", "coef", "dx", "dgamma_p", "dbeta_p", "bcoef", "ws2"):
        _refused(dev, c, d, "bwd", null=(name,))
    for which in ("fwd", "bwd"):
        _refused(dev, c, d, which, over=dict(G=5))                                   # C % G != 0
        _refused(dev, c, d, which, over=dict(G=0))
        _refused(dev, c, d, which, over=dict(N=0))
        _refused(dev, c, d, which, over=dict(V=0))
        _refused(dev, c, d, which, over=dict(C=0))
        _refused(dev, c, d, which, over=dict(ldx=Cn - 4))                            # ld < C, a multiple of 4
        _refused(dev, c, d, which, over=dict(ldx=Cn + 5))                            # ld % 4 != 0
        _refused(dev, c, d, which, over=dict(xs=w["x"].ss + 2))                      # sample stride % 4 != 0
        _refused(dev, c, d, which, off=("x",))                                       # pointer off by 4 bytes
        _refused(dev, c, d, which, off=("ws" if which == "fwd" else "ws2",))          # workspace off a 16-byte boundary
        _refused(dev, c, d, which, over=dict(ws_bytes=need - 1), rc_want=EWORKSPACE)
        _refused(dev, c, d, which, over=dict(ws_bytes=0), rc_want=EWORKSPACE)
    _refused(dev, c, d, "fwd", over=dict(ldy=Cn - 4))
    _refused(dev, c, d, "fwd", over=dict(ldy=Cn + 5))
    _refused(dev, c, d, "fwd", over=dict(ys=w["y"].ss + 1))
    _refused(dev, c, d, "fwd", off=("y",))
    for ld, ss, p in (("lddy", "dys", "dy"), ("lddx", "dxs", "dx"), ("ldadd", "adds", "add")):
        _refused(dev, c, d, "bwd", over={ld: Cn - 4})
        _refused(dev, c, d, "bwd", over={ld: Cn + 6})
        _refused(dev, c, d, "bwd", over={ss: w[p].ss + 3})
        _refused(dev, c, d, "bwd", off=(p,))
    # a group wider than 256 channels
    c = GN.by_name("c510_g2_norm")
    d = GN.inputs(c)
    _refused(dev, c, d, "fwd", over=dict(G=1))
    _refused(dev, c, d, "bwd", over=dict(G=1))
    from cape_amd import ops
    assert int(ops.lib.cape_groupnorm_workspace_bytes(0, 1, 1)) == EINVAL == int(ops.lib.cape_groupnorm_workspace_bytes(1, 1, 0))


# ------------------------------------------------------------------------------------------------- the wrapper
def _leaf(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True)


def _np(t):
    return t.detach().cpu().numpy()


def test_deferred_parameter_gradients_equal_the_immediate_ones(dev):
    """Two group norms inside a deferred sweep with g_gamma / g_beta bucket views, then flush_deferred(): the views hold the
    parameter gradients (within sum_bar of float64, like the immediate ``dgb.sum(1)`` path), every float between them keeps its
    bits, and dx is the immediate path's bit for bit."""
    from cape_amd import ops
    assert ops.DEFERRED is None and ops.LAUNCH_LOG is None and not ops.DEFERRED_GN
    cs = [GN.by_name("c96_g32_rm"), GN.by_name("c38_g2_rm")]
    ds = [GN.inputs(c) for c in cs]
    res = {}
    for mode in ("immediate", "deferred"):
        bucket = torch.full((8 + sum(2 * (c["C"] + 8) for c in cs),), float(SENT), device=dev)
        spans, o = [], 8
        for c in cs:
            spans.append((o, o + c["C"] + 8))
            o += 2 * (c["C"] + 8)
        out = []
        ops.DEFERRED = [] if mode == "deferred" else None
        try:
            for c, d, (og, ob) in zip(cs, ds, spans):
                x, g, b = _leaf(dev, d["x"]), _leaf(dev, d["gamma"]), _leaf(dev, d["beta"])
                views = (bucket[og:og + c["C"]], bucket[ob:ob + c["C"]]) if mode == "deferred" else (None, None)
                y = ops.GroupNormFn.apply(x, g, b, c["G"], float(GN.EPS), True, False, *views)
                gx, gg, gb = torch.autograd.grad((y * torch.from_numpy(d["dy"]).to(dev)).sum(), [x, g, b])
                if mode == "deferred":
                    assert gg.data_ptr() == views[0].data_ptr() and gb.data_ptr() == views[1].data_ptr()
                out.append([_np(y), _np(gx), gg, gb])
            if mode == "deferred":
                assert len(ops.DEFERRED_GN) == 2
                assert (bits(bucket.cpu().numpy()) == bits(np.full(1, SENT, F32))[0]).all()          # nothing before the flush
                ops.flush_deferred()
                assert not ops.DEFERRED_GN
            torch.cuda.synchronize()
        finally:
            ops.DEFERRED = None
            ops.DEFERRED_GN[:] = []
        for o_ in out:
            o_[2], o_[3] = _np(o_[2]).copy(), _np(o_[3]).copy()
        res[mode] = out
        if mode == "deferred":
            host = bucket.cpu().numpy()
            keep = np.ones(host.size, bool)
            for c, (og, ob) in zip(cs, spans):
                keep[og:og + c["C"]] = False
                keep[ob:ob + c["C"]] = False
            assert (bits(host[keep]) == bits(np.full(1, SENT, F32))[0]).all()
    for c, d, imm, dfr in zip(cs, ds, res["immediate"], res["deferred"]):
        assert same_bits(imm[0], dfr[0]) and same_bits(imm[1], dfr[1])
        f64 = GN.forward_ref(d["x"], d["gamma"], d["beta"], c["G"], 1, F64)
        b64 = GN.backward_ref(d["x"], d["dy"], d["gamma"], f64["stats"], c["G"], imm[0] > 0, None, F64)
        for who, r in (("immediate", imm), ("deferred", dfr)):
            sum_bar("GroupNormFn " + who, c["name"] + " / dgamma", r[2], b64["dgamma_p"].sum(0), b64["dgamma_abs"].sum(0))
            sum_bar("GroupNormFn " + who, c["name"] + " / dbeta", r[3], b64["dbeta_p"].sum(0), b64["dbeta_abs"].sum(0))


def test_passthrough_alone_hands_its_gradient_back_unchanged(dev):
    """passthrough=True with only the pass-through output used: the backward returns g_pass itself, and no parameter gradient."""
    from cape_amd import ops
    c = GN.by_name("c38_g2_rm")
    d = GN.inputs(c)
    x, g, b = _leaf(dev, d["x"]), _leaf(dev, d["gamma"]), _leaf(dev, d["beta"])
    y, x2 = ops.GroupNormFn.apply(x, g, b, c["G"], float(GN.EPS), True, True)
    gr = torch.from_numpy(d["dy"]).to(dev)
    ops.LAUNCH_LOG = []
    try:
        gx, gg, gb = torch.autograd.grad((x2 * gr).sum(), [x, g, b], allow_unused=True)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert names == [] and gg is None and gb is None
    assert same_bits(_np(gx), d["dy"])
