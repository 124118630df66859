"""The backward-prep kernels of csrc/elementwise.hip on their own, against float64 (tests/bp_cases.py), through the C entry points
``cape_bwd_prep`` / ``cape_bwd_prep_bf16`` / ``cape_bwd_prep_finalize`` at the smallest shapes that reach the generic, the narrow
and both vector kernels, every start of the shuffle ladder (cvn = 1 .. 64), one to eight column passes, read-ahead 1 and 2,
RB = 16 .. 128, the three regimes of the final stage's bias loop and both ways a row bound is produced; then the wrapper
``ops.bwd_prep``.  The last test runs the module again in a child process under CAPE_SPMM_WIDE=0, where ``bp_cases.plan`` (which
reads the knob as the library does) asserts the 4-channel kernels on the wide shapes.

Every operand is a window of a larger buffer with its own leading dimension and sample stride; the pad columns F .. ld, the rows
beyond Mo and all slack of g, y and rowscale are NaN, the dead bits of the mask words are random; everything around dz, the sums,
the workspace and rowmax_out holds a sentinel that must keep its bits.  Per case: ``cape_bwd_prep_plan`` equals the table's tuple;
the case runs twice on fresh buffers and gives the same bits; dz is THE float32 product bit for bit (none / leaky / relu / mask,
the sign of zero included; bf16 storage: its rounding to nearest even) -- tanh goes to kernel_bars.element_bar (bf16: one bf16
rounding on top, the bar of test_gpu_sparse.bf16_bar) --; dbias, dcoef, dcoef_g per element to kernel_bars.sum_bar against
float64 sums of the unrounded float32 products (of g for dcoef_g); rowmax_out entry by entry the bits of max |g| over its column
pass (over the whole row in entry 0 where the bound is standalone), +0 in the entries no pass owns, and the maximum over the four
entries never below max |g| or max |dz| of the row (asked of every fp32 vector case but v4_f32_nobias and v8_f256_sums, which
pass NULL on purpose, and of the scalar forms at F = 3, 32 and 64).  Every output element of every case is judged.

Both defects the issue suspected were real, shown on an MI355X by these cases before the fix:
  1. v4_f1280 (five passes of 256) and v8_f4096 (eight of 512): the vector kernel wrote the bound of pass p >= 4 into entry
     p - 4 of the NEXT row (racing with that row's own store) and, after the last row, behind the buffer: one and four floats of
     the guard held the last row's passes 4.. bit for bit, and 8 / 11 of the 20 rows were bounded below max |g|.  Such shapes
     now take the standalone pass; a row keeps four entries.
  2. gen_f64_off1, gen_f64_ld67, gen_f32_off1_mask, gen_f32_zoff2_tanh, gen_f64_inplace_off1, nar_f3_rm and the wrapper test:
     the standalone pass of the scalar forms ran over dz, so with an activation or a mask the bound lay below max |g| of the
     rows whose largest element is damped (36 of 74 rows of gen_f64_ld67, e.g. 2.106 for a row of 3.342; 0 for the rows of
     nar_f3_rm that relu switches off) -- and ops.bwd_prep attaches it to g as well.  It now runs over g, before the launch
     (in place, g is overwritten).

Measured on an MI355X, worst error in units of the bar (sum_bar: over 2e-6 sum |terms|; dz is bit-exact except tanh):
  family    generic  dbias 0.045  dcoef 0.048  dcoef_g 0.045  tanh dz 0.169      narrow  0.013  0.038  0.025  tanh dz 0.173
            vec4     dbias 0.046  dcoef 0.062  dcoef_g 0.051  tanh dz 0.180      vec8    0.058  0.059  0.038
            (bf16 tanh, v8_f512_bf16_tanh: 0.987 of the bf16 bar -- half an ulp of bf16 just above a power of two)
  cvn       1: 0.017   2: 0.023   4: 0.031   8: 0.045   16: 0.062   32: 0.054   64: 0.059          (the worst of the three sums)
  RB        16: 0.062   32: 0.008   64: 0.010   128: 0.007
  final     idle lanes 0.062   tail only 0.057   unrolled + tail 0.030   unrolled only 0.003
The float32 restatement of tests/bp_cases.py in the kernel's order gives 0.058 / 0.062 / 0.051 on the CPU: the device's sums are
the emulation's to two digits.  The module runs in 7 s, 4 s of them the knob leg.

Changed on a scratch build and caught by (default leg, the finalize and refusal tests left out):
  * the shuffle ladder started at 2 cvn: every vector case with cvn < 64 that has a sum -- v4_f4, v4_f8, v4_f16, v4_f32, v4_f64,
    v4_f128, v8_f256 and 23 more; cvn = 64 has no ladder (v4_f768, v8_f512 pass);
  * read-ahead rows accumulated without ``r < rb`` (stores left masked): 35 cases, rows_rb_plus2, rows_lt_rb, rows_mo1 and
    rows_f4_rlanes among them; the fp32 8-channel cases (read-ahead 1) pass, the bf16 ones (read-ahead 2) fail;
  * ``cgs`` taken as R * F: v4_f32_nobias and ops_rg_only_nobias (R = 0: every sample's dcoef_g lands on sample 0; run on these
    two alone -- with R >= 2 the mutant stores behind the buffer);
  * ``le`` = 4 at cvn = 64 is no mutation: 256 / 64 = 4 row lanes, so ``le`` is 4 there as written, and the per-lane slot
    ``threadIdx.x`` equals the per-wave slot ``(threadIdx.x >> 6) * cvn + q``;
  * the bias loop bound ``i + 16 * NS`` only moves terms from the unrolled loop into the tail: every partial is still summed
    once, the module passes, and rightly so.  (The bound as written is the last one that keeps ``part[(i + 240) * TF + f]``
    inside the slab.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bp_cases as BP
from kernel_bars import element_bar, sum_bar, same_bits, bits, mat_err, TOL
import parity_bar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
SENT = F32(-31337.5)
NAN = F32(np.nan)
EINVAL, EWORKSPACE = -1, -4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def to_raw(a, bf16):
    """float32 values -> the stored integers (int32; bf16: the upper halves as int16 -- the values must be bf16 numbers)"""
    u = np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)
    if not bf16:
        return u.view(np.int32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16).view(np.int16)


def from_raw(r, bf16):
    if not bf16:
        return np.ascontiguousarray(r).view(F32)
    return (np.ascontiguousarray(r).view(np.uint16).astype(np.uint32) << 16).view(F32)


class Win:
    """A window of ``shape`` with ``strides`` (in elements) inside a 1-D device buffer: 16 bytes plus ``off`` elements in front
    of it, 8 elements behind its last one, everything outside the window = ``pad``.  fp32, or bf16 kept as 16-bit integers."""

    def __init__(self, dev, shape, strides=None, data=None, pad=SENT, off=0, bf16=False):
        shape = tuple(int(s) for s in shape)
        if strides is None:
            strides = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
        self.bf16, self.es = bf16, 2 if bf16 else 4
        self.front = 16 // self.es + off
        idx = np.full(shape, self.front, np.int64)
        for ax, (n, st) in enumerate(zip(shape, strides)):
            idx += (np.arange(n, dtype=np.int64) * st).reshape([-1 if a == ax else 1 for a in range(len(shape))])
        padv = F32(pad) if not bf16 else BP.bf16_round(np.full(1, pad, F32))[0]
        self.pad_raw = to_raw(np.full(1, padv, F32), bf16)[0]
        host = np.full(int(idx.max()) + 1 + 8, self.pad_raw)
        self.idx = idx
        self.outside = np.ones(host.size, bool)
        self.outside[idx.reshape(-1)] = False
        assert int((~self.outside).sum()) == idx.size                          # (no two elements share a slot)
        if data is not None:
            host[idx] = to_raw(np.asarray(data, F32).reshape(shape), bf16)
        self.host = host
        self.buf = torch.from_numpy(host).to(dev)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.front * self.es

    def p(self, elems=0):
        return C.c_void_p(self.ptr + self.es * int(elems))

    def read(self):
        """(the window as float32 values, whether everything outside it kept its bits)"""
        host = self.buf.cpu().numpy()
        return from_raw(host[self.idx], self.bf16).copy(), bool((host[self.outside] == self.pad_raw).all())

    def unchanged(self):
        """the whole buffer is what was uploaded"""
        return bool(np.array_equal(self.buf.cpu().numpy(), self.host))


OUTS = ("dz", "dbias", "dcoef", "dcoef_g", "rm")


def _lib():
    from cape_amd import ops
    return ops.lib, ops._stream


def execute(dev, c, d, finalize=1, over=None, null=(), sentinel_dz=False):
    """One cape_bwd_prep[_bf16] on fresh buffers.  ``over``: scalar arguments to falsify in the CALL, ``null``: pointers passed as
    NULL (the buffers stay those of the case).  Returns (rc, {name: Win or None}, the arguments of the call)."""
    lib, S = _lib()
    N, Mo, F, R, bf = c["N"], c["Mo"], c["F"], c["R"], c["dt"] == "bf16"
    st = (c["ss"], c["ld"], 1)
    need = BP.workspace_bytes(N, Mo, F, R)
    assert int(lib.cape_bwd_prep_workspace_bytes(N, Mo, F, R)) == need
    w = dict(g=Win(dev, (N, Mo, F), st, d["g"], NAN, c["off"], bf))
    w["y"] = Win(dev, (N, Mo, F), st, d["y"], NAN, c["off"], bf) if (c["act"] != "none" and not c["mask"]) else None
    w["dz"] = w["g"] if c["alias"] != "no" else Win(dev, (N, Mo, F), st, None, SENT, c["zoff"], bf)
    w["mask"] = None if d["mask"] is None else torch.from_numpy(d["mask"].view(np.int32)).to(dev)
    w["rs"] = Win(dev, (R + 1, Mo), None, d["rowscale"], NAN) if (R or c["rg"]) else None
    w["dbias"] = Win(dev, (F,)) if c["bias"] else None
    if c["joint"]:
        w["joint"] = Win(dev, (N, R + 1, F))
        w["dcoef"] = w["dcoef_g"] = None
        pc, pg, cs = w["joint"].p(), w["joint"].p(R * F), (R + 1) * F
    else:
        w["joint"] = None
        w["dcoef"] = Win(dev, (N, R, F)) if R else None
        w["dcoef_g"] = Win(dev, (N, F)) if c["rg"] else None
        pc, pg, cs = (w["dcoef"].p() if R else None), (w["dcoef_g"].p() if c["rg"] else None), 0
    w["ws"] = Win(dev, (need // 4,))
    w["rm"] = Win(dev, (N * Mo, 4)) if c["rm"] else None
    ptr = dict(g=w["g"].p(), y=w["y"].p() if w["y"] else None, dz=w["dz"].p(), mask=C.c_void_p(w["mask"].data_ptr()) if c["mask"] else None,
               dbias=w["dbias"].p() if c["bias"] else None, rs=w["rs"].p() if w["rs"] else None, dcoef=pc, dcoef_g=pg, ws=w["ws"].p(),
               rm=w["rm"].p() if c["rm"] else None)
    for k in null:
        ptr[k] = None
    a = dict(gs=c["ss"], ldg=c["ld"], ys=c["ss"], ldy=c["ld"], act=BP.ACT[c["act"]], zs=c["ss"], ldz=c["ld"], R=R, rg=R if c["rg"] else 0,
             cs=cs, finalize=finalize, N=N, Mo=Mo, F=F, ws_bytes=need)
    a.update(over or {})
    fn = getattr(lib, "cape_bwd_prep_bf16" if bf else "cape_bwd_prep")
    rc = int(fn(ptr["g"], a["gs"], a["ldg"], ptr["y"], a["ys"], a["ldy"], a["act"], ptr["mask"], ptr["dz"], a["zs"], a["ldz"], ptr["dbias"],
                ptr["rs"], a["R"], ptr["dcoef"], a["rg"], ptr["dcoef_g"], a["cs"], a["finalize"], a["N"], a["Mo"], a["F"], ptr["ws"],
                a["ws_bytes"], ptr["rm"], S()))
    torch.cuda.synchronize()
    return rc, w, dict(ptr=ptr, a=a)


def device_plan(c, w):
    lib, _ = _lib()
    out = (C.c_int32 * 6)()
    fn = getattr(lib, "cape_bwd_prep_plan_bf16" if c["dt"] == "bf16" else "cape_bwd_prep_plan")
    rc = int(fn(w["g"].p(), c["ss"], c["ld"], w["y"].p() if w["y"] else None, c["ss"], c["ld"], BP.ACT[c["act"]],
                C.c_void_p(w["mask"].data_ptr()) if c["mask"] else None, w["dz"].p(), c["ss"], c["ld"], c["N"], c["Mo"], c["F"],
                1 if c["rm"] else 0, out))
    assert rc == 0, (c["name"], rc)
    return tuple(out)


def collect(c, w):
    """(failures, {name: array}) of one finished call: the windows of dz, the sums and the bounds; every guard checked"""
    fails, got = [], {}
    N, Mo, F, R = c["N"], c["Mo"], c["F"], c["R"]
    for k in ("g", "y", "rs"):
        if w[k] is not None and not (k == "g" and c["alias"] == "inplace") and not w[k].unchanged():
            fails.append("%s / %s: an input (or its NaN pad) was written" % (c["name"], k))
    if c["mask"] and not np.array_equal(w["mask"].cpu().numpy(), BP.inputs(c)["mask"].view(np.int32)):
        fails.append("%s / mask: written" % c["name"])
    for k in ("dz", "dbias", "dcoef", "dcoef_g", "joint", "rm", "ws"):
        if w[k] is None:
            continue
        v, ok = w[k].read()
        if not ok:
            fails.append("%s / %s: wrote outside its window (%s)" % (c["name"], k, c["why"]))
        if k == "joint":
            got["dcoef"], got["dcoef_g"] = np.ascontiguousarray(v[:, :R]), np.ascontiguousarray(v[:, R])
        elif k == "rm":
            got[k] = v.reshape(N, Mo, 4)
        elif k != "ws":
            got[k] = v
    return fails, got


# ------------------------------------------------------------------------------------------------- the table of cases
FIGURES = {}                     # (what the case reaches, quantity) -> (worst figure in units of its bar, case)


def _note(c, P, quantity, fig):
    what = ["family " + BP.FAMILY[P[0]], "RB = %d" % P[2], "final: " + BP.final_regime(c["N"], P)]
    if P[0] >= BP.VEC4:
        what += ["cvn = %d" % v for v in set(BP.cvns(P, c["F"]))] + ["read-ahead %d" % P[1]]
    for k in what:
        if fig >= FIGURES.get((k, quantity), (-1.0, ""))[0]:
            FIGURES[(k, quantity)] = (fig, c["name"])


def bf16_bar(name, dev_, f32_, ref):
    """test_gpu_sparse.bf16_bar: one bf16 rounding of an fp32 result that is inside the fp32 bar"""
    dev_, f32_, ref = (np.asarray(v, F64) for v in (dev_, f32_, ref))
    tol = 2.0 ** -8 * np.abs(ref) + 4.0 * np.abs(f32_ - ref).max()
    err = np.abs(dev_ - ref)
    share = float((err / np.where(tol > 0, tol, 1.0)).max())
    print("%s: worst |err| / bf16 bar = %.3f" % (name, share))
    assert np.isfinite(dev_).all() and (err <= tol).all(), (name, share)
    return share


def run_case(dev, c):
    """The case twice; every check of the module docstring.  Returns (failures, {quantity: error in units of its bar})."""
    d = BP.inputs(c)
    figs = {}
    rc, w, _ = execute(dev, c, d)
    P = device_plan(c, w)
    assert P == BP.wanted(c) == BP.case_plan(c), (c["name"], "cape_bwd_prep_plan", P, "table", BP.wanted(c), "plan()", BP.case_plan(c))
    rc2, w2, _ = execute(dev, c, d)
    if (rc, rc2) != (0, 0):
        return ["%s: rc %s / %s (%s)" % (c["name"], rc, rc2, c["why"])], figs
    fails, got = collect(c, w)
    fails2, got2 = collect(c, w2)
    fails += fails2
    for k in got:
        if not same_bits(np.ascontiguousarray(got[k]), np.ascontiguousarray(got2[k])):
            fails.append("%s / %s: two runs differ" % (c["name"], k))
    if c["alias"] == "sums" and not w["g"].unchanged():
        fails.append("%s: the sums-only call wrote dz == g" % c["name"])
    if fails:
        return fails, figs
    ref = BP.reference(c, d)
    # ---- dz
    if ref["store"] is not None:
        fails += BP.judge_dz(c, ref, got["dz"])
        figs["dz"] = 0.0
    elif c["dt"] == "f32":
        e, e32 = mat_err(got["dz"], ref["dz64"]), mat_err(ref["dz32r"], ref["dz64"])
        figs["dz"] = e / min(max(4.0 * e32, parity_bar.FLOOR), TOL)
        try:
            element_bar("bwd_prep", c["name"] + " / dz", got["dz"], ref["dz32r"], ref["dz64"])
        except AssertionError as e_:
            fails.append("%s / dz (%s): %s" % (c["name"], c["why"], str(e_)[:300]))
    else:
        try:
            figs["dz"] = bf16_bar(c["name"] + " / dz", got["dz"], ref["dz32r"], ref["dz64"])
        except AssertionError as e_:
            fails.append("%s / dz (%s): %s" % (c["name"], c["why"], str(e_)[:300]))
    # ---- the sums
    f, sfig = BP.judge_sums(c, ref, got)
    fails += f
    figs.update(sfig)
    emu = BP.emulate_sums(c, d, P)
    for k in sfig:
        try:
            sum_bar("bwd_prep", c["name"] + " / " + k, got[k], ref[k], ref[k + "_abs"], f32=emu[k])
        except AssertionError as e_:
            fails.append("%s / %s (%s): %s" % (c["name"], k, c["why"], str(e_)[:300]))
    # ---- the row bounds
    if c["rm"]:
        fails += BP.judge_bounds(c, d, P, got["rm"], got["dz"])
    for k, v in figs.items():
        _note(c, P, k, v)
    return fails, figs


@pytest.mark.parametrize("c", BP.CASES, ids=lambda c: c["name"])
def test_case(dev, c):
    """One case of the table: everything the module docstring lists."""
    fails, figs = run_case(dev, c)
    print("%s: %s" % (c["name"], "  ".join("%s %.3f" % kv for kv in sorted(figs.items()))))
    assert not fails, "\n".join(fails)


def test_print_the_worst_figure_of_every_form(dev):
    assert FIGURES, "runs after test_case"
    for (what, k), (v, name) in sorted(FIGURES.items()):
        print("WORST %-24s %-8s %.3f of its bar at %s" % (what, k, v, name))


# ------------------------------------------------------------------------------------------------- the deferred final stage
def _item(it, c, w, chunks=0, drop=()):
    it.workspace = w["ws"].ptr
    it.N, it.Mo, it.F, it.R = c["N"], c["Mo"], c["F"], c["R"]
    R, F = c["R"], c["F"]
    it.dbias = w["dbias"].ptr if c["bias"] and "dbias" not in drop else None
    if c["joint"]:
        it.dcoef, it.dcoef_g, it.dcoef_sample_stride = w["joint"].ptr, w["joint"].ptr + 4 * R * F, (R + 1) * F
    else:
        it.dcoef = w["dcoef"].ptr if R and "dcoef" not in drop else None
        it.dcoef_g = w["dcoef_g"].ptr if c["rg"] else None
        it.dcoef_sample_stride = 0
    it.chunks = chunks


BATCH = ["gen_f5", "gen_f36", "gen_f130", "nar_f2", "nar_r4_rg", "v4_f4", "v4_f32", "v4_f64", "v4_f32_nobias", "v8_f256", "v8_f512",
         "rows_mo1", "fin_tail", "fin_unrolled_tail", "ops_separate_dcoef", "ops_rg_only_nobias"]


def _sums_of(c, w):
    fails, got = collect(c, w)
    assert not fails, fails
    return {k: got[k] for k in BP.SUMS if k in got}


def test_finalize_0_then_one_batched_final_equals_finalize_1(dev):
    """16 layers of different N, Mo, F, R -- two without dbias, joint and separate dcoef, one with explicit chunks -- deferred
    with finalize = 0: the outputs still hold their sentinels; one cape_bwd_prep_finalize over the 16 gives the bits of the 16
    undeferred calls, and so does a single-item final of each."""
    from cape_amd import _lib as L
    lib, S = _lib()
    cs = [BP.by_name(n) for n in BATCH]
    assert len(cs) == 16 and {c["bias"] for c in cs} == {0, 1} and {c["joint"] for c in cs} == {0, 1} and len({(c["N"], c["F"], c["R"]) for c in cs}) >= 12
    ds = [BP.inputs(c) for c in cs]
    imm = []
    for c, d in zip(cs, ds):
        rc, w, _ = execute(dev, c, d, finalize=1)
        assert rc == 0
        imm.append(_sums_of(c, w))
    for mode in ("batch", "single"):
        held = []
        for c, d in zip(cs, ds):
            rc, w, _ = execute(dev, c, d, finalize=0)
            assert rc == 0
            for k in ("dbias", "dcoef", "dcoef_g", "joint"):
                assert w[k] is None or w[k].unchanged(), (c["name"], k, "written before the final stage")
            held.append(w)
        if mode == "batch":
            arr = (L.CapeBwdPrepItem * 16)()
            for i, (it, c, w) in enumerate(zip(arr, cs, held)):
                _item(it, c, w, chunks=BP.case_plan(c)[3] if i == 2 else 0)
            assert int(lib.cape_bwd_prep_finalize(arr, 16, S())) == 0
        else:
            for c, w in zip(cs, held):
                arr = (L.CapeBwdPrepItem * 1)()
                _item(arr[0], c, w)
                assert int(lib.cape_bwd_prep_finalize(arr, 1, S())) == 0
        torch.cuda.synchronize()
        for c, w, want in zip(cs, held, imm):
            got = _sums_of(c, w)
            assert set(got) == set(want)
            for k in want:
                assert same_bits(np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])), (mode, c["name"], k)


def test_finalize_refuses_bad_item_lists(dev):
    from cape_amd import _lib as L
    lib, S = _lib()
    c = BP.by_name("gen_f36")
    rc, w, _ = execute(dev, c, BP.inputs(c), finalize=0)
    assert rc == 0
    one = (L.CapeBwdPrepItem * 1)()
    _item(one[0], c, w)
    many = (L.CapeBwdPrepItem * 17)(*([one[0]] * 17))
    assert int(lib.cape_bwd_prep_finalize(many, 17, S())) == EINVAL
    assert int(lib.cape_bwd_prep_finalize(one, 0, S())) == EINVAL
    assert int(lib.cape_bwd_prep_finalize(None, 1, S())) == EINVAL
    bad = (L.CapeBwdPrepItem * 1)(one[0])
    bad[0].workspace = None
    assert int(lib.cape_bwd_prep_finalize(bad, 1, S())) == EINVAL
    bad = (L.CapeBwdPrepItem * 1)(one[0])
    bad[0].dcoef = None                                                          # R = 2 without dcoef
    assert int(lib.cape_bwd_prep_finalize(bad, 1, S())) == EINVAL
    for field in ("N", "Mo", "F"):
        bad = (L.CapeBwdPrepItem * 1)(one[0])
        setattr(bad[0], field, 0)
        assert int(lib.cape_bwd_prep_finalize(bad, 1, S())) == EINVAL, field
    bad = (L.CapeBwdPrepItem * 1)(one[0])
    bad[0].R = 5
    assert int(lib.cape_bwd_prep_finalize(bad, 1, S())) == EINVAL
    torch.cuda.synchronize()
    assert w["joint"].unchanged() and w["dbias"].unchanged()


# ------------------------------------------------------------------------------------------------- refused before any launch
def _refused(dev, c, d, rc_want=EINVAL, **t):
    rc, w, _ = execute(dev, c, d, **t)
    assert rc == rc_want, (c["name"], t, rc)
    for k in ("dz", "dbias", "dcoef", "dcoef_g", "joint", "rm", "ws"):
        if w[k] is not None:
            assert w[k].unchanged(), (c["name"], t, k)


def test_entry_point_refuses_bad_arguments(dev):
    """Every documented refusal of cape_bwd_prep: the code, and every output buffer as it was uploaded."""
    c = BP.by_name("gen_f64_off1")                                              # leaky, R = 1, rg, a bound
    d = BP.inputs(c)
    rc, w, _ = execute(dev, c, d)
    assert rc == 0 and not w["dz"].unchanged()                                   # (the base case is accepted)
    need = BP.workspace_bytes(c["N"], c["Mo"], c["F"], c["R"])
    _refused(dev, c, d, over=dict(ldg=c["F"] - 1))
    _refused(dev, c, d, over=dict(ldz=c["F"] - 1))
    _refused(dev, c, d, over=dict(ldy=c["F"] - 1))
    _refused(dev, c, d, null=("y",))                                            # an activation without y
    _refused(dev, c, d, over=dict(R=5))
    _refused(dev, c, d, over=dict(R=-1))
    _refused(dev, c, d, null=("dcoef",))                                        # R > 0 without dcoef
    _refused(dev, c, d, null=("rs",))
    _refused(dev, c, d, over=dict(R=0), null=("rs", "dcoef"))                   # dcoef_g without rowscale
    _refused(dev, c, d, over=dict(ws_bytes=need - 1), rc_want=EWORKSPACE)
    _refused(dev, c, d, over=dict(ws_bytes=0), rc_want=EWORKSPACE)
    _refused(dev, c, d, over=dict(act=4))
    _refused(dev, c, d, over=dict(act=-1))
    for k in ("g", "dz", "ws"):
        _refused(dev, c, d, null=(k,))
    for k in ("N", "Mo", "F"):
        _refused(dev, c, d, over={k: 0})
    # rowmax_out with bf16 storage
    cb = dict(BP.by_name("gen_f36_bf16"))
    db = BP.inputs(cb)
    cb["rm"] = 1
    _refused(dev, cb, db)
    lib, _ = _lib()
    assert int(lib.cape_bwd_prep_workspace_bytes(0, 1, 1, 0)) == EINVAL == int(lib.cape_bwd_prep_workspace_bytes(1, 1, 1, 5))
    out = (C.c_int32 * 6)()
    assert int(lib.cape_bwd_prep_plan(w["g"].p(), c["ss"], c["F"] - 1, w["y"].p(), c["ss"], c["ld"], 1, None, w["dz"].p(), c["ss"], c["ld"],
                                      c["N"], c["Mo"], c["F"], 1, out)) == EINVAL
    assert int(lib.cape_bwd_prep_plan_bf16(w["g"].p(), c["ss"], c["ld"], w["y"].p(), c["ss"], c["ld"], 1, None, w["dz"].p(), c["ss"], c["ld"],
                                           c["N"], c["Mo"], c["F"], 1, out)) == EINVAL


# ------------------------------------------------------------------------------------------------- the wrapper
def _np(t):
    return t.detach().cpu().numpy()


def test_wrapper_bounds_g_on_an_unaligned_power_of_two_view(dev):
    """Suspect 2 end to end: ops.bwd_prep on a gradient view at a channel offset of one element, F = 64, relu.  The bound it
    attaches to BOTH g and dz is max |g| of every row."""
    from cape_amd import ops
    rng = np.random.default_rng(5)
    N, Mo, F = 2, 37, 64
    base = torch.from_numpy(rng.standard_normal((N, Mo, 72)).astype(F32)).to(dev)
    g = base[:, :, 1:1 + F]
    y = torch.from_numpy(rng.standard_normal((N, Mo, F)).astype(F32)).to(dev)
    assert not ops._vec_ok(g) and ops._want_rm(g), "the two-piece arithmetic is on by default"
    dz, db, _, _ = ops.bwd_prep(g, y=y, act="relu", want_bias=True)
    torch.cuda.synchronize()
    rm_g, rm_z = ops.rm_of(g), ops.rm_of(dz)
    assert rm_g is not None and rm_z is not None and rm_g.data_ptr() == rm_z.data_ptr()
    gh, zh, rm = _np(g), _np(dz), _np(rm_g)
    assert same_bits(np.ascontiguousarray(zh), (gh * (_np(y) > 0).astype(F32)).astype(F32))
    assert same_bits(np.ascontiguousarray(rm[:, :, 0]), np.abs(gh).max(axis=2)) and not bits(np.ascontiguousarray(rm[:, :, 1:])).any()
    assert (np.abs(zh).max(axis=2) < np.abs(gh).max(axis=2)).any(), "some row's largest element is switched off (or the case shows nothing)"


def test_wrapper_deferred_equals_immediate_and_honours_dbias_out(dev):
    """defer=True inside a deferred sweep, then flush_deferred(): dz, dbias, dcoef, dcoef_g are the immediate call's bit for bit;
    dbias lands in the ``dbias_out`` view of a bucket whose other floats keep their bits."""
    from cape_amd import ops
    assert ops.DEFERRED is None
    c = BP.by_name("ops_joint")
    d = BP.inputs(c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    res = {}
    for mode in ("immediate", "deferred"):
        bucket = torch.full((c["F"] + 16,), float(SENT), device=dev)
        view = bucket[8:8 + c["F"]]
        ops.DEFERRED = [] if mode == "deferred" else None
        try:
            dz, db, dc, dcg = ops.bwd_prep(t(d["g"]), y=t(d["y"]), act="leaky", want_bias=True, rowscale=t(d["rowscale"]), R=c["R"], rg=c["R"],
                                           dbias_out=view, joint=True, defer=True)
            assert db.data_ptr() == view.data_ptr()
            if mode == "deferred":
                torch.cuda.synchronize()
                assert len(ops.DEFERRED) == 1 and (bits(_np(bucket)) == bits(np.full(1, SENT, F32))[0]).all()      # nothing before the flush
                ops.flush_deferred()
                assert not ops.DEFERRED
            torch.cuda.synchronize()
        finally:
            ops.DEFERRED = None
        host = _np(bucket)
        assert (bits(host[:8].copy()) == bits(np.full(1, SENT, F32))[0]).all() and (bits(host[8 + c["F"]:].copy()) == bits(np.full(1, SENT, F32))[0]).all()
        res[mode] = [_np(dz).copy(), host[8:8 + c["F"]].copy(), _np(dc).copy()]
    for a, b in zip(res["immediate"], res["deferred"]):
        assert same_bits(a, b)
    ref = BP.reference(c, d)
    assert same_bits(res["immediate"][0], ref["dz32"])
    sum_bar("ops.bwd_prep", "dbias", res["immediate"][1], ref["dbias"], ref["dbias_abs"])
    sum_bar("ops.bwd_prep", "dcoef", res["immediate"][2][:, :c["R"]], ref["dcoef"], ref["dcoef_abs"])
    sum_bar("ops.bwd_prep", "dcoef_g", res["immediate"][2][:, c["R"]], ref["dcoef_g"], ref["dcoef_g_abs"])


# ------------------------------------------------------------------------------------------------- the knob leg
def test_bwd_prep_under_knob_spmm_wide_0():
    """CAPE_SPMM_WIDE is latched at first use: one fresh child process runs every other test of this module with the 4-channel
    kernels on the wide shapes (bp_cases.plan reads the knob, so the table asserts them)."""
    env = dict(os.environ)
    env["CAPE_SPMM_WIDE"] = "0"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_bwd_prep.py"), "-x", "-q", "-m", "gpu", "-k", "not knob"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode()[-2500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
