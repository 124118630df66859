"""The cases of tests/test_gpu_bwd_prep.py: the backward-prep kernels of csrc/elementwise.hip called through ``cape_bwd_prep`` /
``cape_bwd_prep_bf16`` / ``cape_bwd_prep_finalize`` at the smallest shapes that reach every kernel family, every start of the
shuffle ladder, every column-pass count, every row-chunk form, every regime of the final stage's bias loop and both ways a row
bound is produced.  TEST INFRASTRUCTURE ONLY (no GPU needed here; tests/test_bp_cases_host.py checks this file on the CPU).

* ``plan(...)`` restates the host dispatch (``bp_plan`` of elementwise.hip, what ``cape_bwd_prep_plan`` returns): ``bp_rows``,
  ``aligned4`` / ``aligned8`` of csrc/views.h with their element-size rule, the ``256 % (F / VW)`` rule, the mask's ``F % 32``
  rule, ``CAPE_SPMM_WIDE`` read as the library reads it (``atoi`` of the variable, 1 without it), read-ahead 1 for the 8-channel
  kernel on fp32 and 2 otherwise, and the row bound: none / in the kernel (vector form, at most four column passes) /
  standalone.
* ``reference(c, d)``: dz in float64; for none / leaky / relu / mask also as THE float32 value, bit for bit -- one float32
  multiply by fl(0.2f), 1 or 0, or a select, the sign of zero included (a negative gradient times 0 is -0; a masked-out
  element is +0) --; for bf16 storage that float32 value rounded to nearest even as ``cape_st`` rounds it (``bf16_round``, tied
  to sparse_reference.bf16 by the host test).  The three sums in float64 with sum |terms| next to each.  THE TERMS ARE THE
  UNROUNDED float32 ``d`` FOR dbias AND dcoef, AND ``g`` FOR dcoef_g: the kernels accumulate before the store, so in bf16
  storage the sums are those of the float32 products, not of the stored dz (for tanh the terms are the float64 products: the
  kernel's float32 ``g * (1 - y * y)`` is not pinned to the bit).
* ``emulate_sums(c, d)``: the sums in float32 in the kernel's own order -- per chunk and column pass the row lanes of the
  family (4 / 256 / 256 over the column groups), each lane its rows one after the other (fma for the scaled terms), the lanes by
  the xor butterflies and then the waves in index order, then the final stage's 16 lanes over the partials and the 16 lane sums
  in index order.  For the record column of kernel_bars.sum_bar and for the host test's margin; not a bit-for-bit model.
* ``bounds_ref(c, d, P)``: the row bounds [N, Mo, 4]: entry p = max |g| over the columns of pass p in the kernel, entry 0 = max
  over the row by the standalone pass, +0 elsewhere.
* One table of cases; each carries a ``why`` and the exact plan tuple (family, read-ahead, RB, chunks per sample, column passes,
  bound) it must reach, once as the library runs by default and once under CAPE_SPMM_WIDE=0."""
import os
import zlib

import numpy as np

import kernel_bars

F32, F64 = np.float32, np.float64
GENERIC, NARROW, VEC4, VEC8 = 0, 1, 2, 3
FAMILY = {GENERIC: "generic", NARROW: "narrow", VEC4: "vec4", VEC8: "vec8"}
B_NONE, B_KERNEL, B_ALONE = 0, 1, 2
ACT = {"none": 0, "leaky": 1, "relu": 2, "tanh": 3}
LEAK = F32(0.2)
BP_BLOCKS, BP_RB_MAX, BP_RB_MIN, BP_UNROLL = 448, 128, 16, 2
MAXR = 4


# ----------------------------------------------------------------------------------------------------- the dispatch
def bp_rows(N, Mo):
    rb = BP_RB_MAX
    while rb > BP_RB_MIN and N * ((Mo + rb - 1) // rb) < BP_BLOCKS:
        rb >>= 1
    return rb


def spmm_wide():
    """CAPE_SPMM_WIDE as csrc/views.h reads it: atoi() of the variable (leading blanks, a sign, digits; anything else 0)."""
    v = os.environ.get("CAPE_SPMM_WIDE")
    if v is None:
        return True
    s = v.lstrip(" \t\n\v\f\r")
    i = 1 if s[:1] in ("+", "-") else 0
    j = i
    while j < len(s) and s[j] in "0123456789":
        j += 1
    return (int(s[:j]) if j > i else 0) != 0


def aligned4(view, C, es):
    """view = (element offset from a 16-byte boundary, sample stride, leading dimension)"""
    off, ss, ld = view
    return (off * es) % (4 * es) == 0 and ss % 4 == 0 and ld % 4 == 0 and C % 4 == 0


def aligned8(view, C, es):
    off, ss, ld = view
    a = 4 if es == 4 else 8
    return (off * es) % 16 == 0 and ss % a == 0 and ld % a == 0 and C % 8 == 0


def workspace_bytes(N, Mo, F, R):
    RB = bp_rows(N, Mo)
    return N * ((Mo + RB - 1) // RB) * (R + 2) * F * 4


def plan(N, Mo, F, g, dz, y, act, mask, es, rm, wide=None):
    """(family, read-ahead, RB, chunks, passes, bound) of cape_bwd_prep for these views.  ``g`` / ``dz`` / ``y``: views as
    aligned4 takes them (``y`` is looked at only with an activation and no mask); ``act``: its name; ``mask`` / ``rm``: whether
    there is one; ``wide``: CAPE_SPMM_WIDE, None = as the environment has it."""
    wide = spmm_wide() if wide is None else wide
    RB = bp_rows(N, Mo)
    chunks = (Mo + RB - 1) // RB
    need_y = not mask and act != "none"
    vec = (aligned4(g, F, es) and aligned4(dz, F, es) and (not need_y or aligned4(y, F, es))
           and ((F % 256 == 0) if F >= 256 else (256 % (F // 4) == 0)) and (F % 32 == 0 or not mask))
    w8 = (vec and wide and aligned8(g, F, es) and aligned8(dz, F, es) and (not need_y or aligned8(y, F, es))
          and F >= 256 and ((F % 512 == 0) if F >= 512 else (256 % (F // 8) == 0)))
    family = VEC8 if w8 else VEC4 if vec else NARROW if F <= 4 else GENERIC
    depth = 0 if not vec else 1 if (w8 and es == 4) else BP_UNROLL
    fb = {VEC8: 512, VEC4: 256, NARROW: 4, GENERIC: 64}[family]
    passes = (F + fb - 1) // fb
    bound = B_NONE if not rm else B_KERNEL if (vec and passes <= 4) else B_ALONE
    return (family, depth, RB, chunks, passes, bound)


def pass_columns(P, F):
    """[(first column, width)] of the column passes of plan ``P``"""
    fb = {VEC8: 512, VEC4: 256, NARROW: 4, GENERIC: 64}[P[0]]
    return [(b, min(fb, F - b)) for b in range(0, F, fb)]


def cvns(P, F):
    """column groups per pass of a vector plan (the start of the shuffle ladder; 64 = the per-lane LDS layout)"""
    vw = {VEC4: 4, VEC8: 8}[P[0]]
    return [w // vw for _, w in pass_columns(P, F)]


def final_regime(N, P):
    """how the final stage's bias loop runs over the N * chunks partials of a column: 16 sums per lane, then a tail"""
    total = N * P[3]
    return "idle lanes" if total < 16 else "tail only" if total < 256 else "unrolled + tail" if total % 256 else "unrolled only"


# ----------------------------------------------------------------------------------------------------- the cases
DATA_KINDS = ("normal", "binades", "yzero", "tanhedge", "mask0", "mask1")
ALIAS = ("no", "inplace", "sums")


def _case(name, N, Mo, F, why, want, want0=None, dt="f32", act="leaky", mask=0, R=0, rg=0, bias=1, joint=0, alias="no", off=0, zoff=0,
          ld=None, ss_extra=16, data="normal", rm=0):
    """``off`` / ``zoff``: element offset of the g (and y) / dz window from a 16-byte boundary; ``ld``: leading dimension of all
    three views (default: F rounded up to 8, plus 8); ``ss_extra``: elements between the samples beyond Mo * ld.  ``want`` /
    ``want0``: the plan by default / under CAPE_SPMM_WIDE=0 (the same when ``want0`` is None)."""
    assert data in DATA_KINDS and alias in ALIAS and act in ACT and dt in ("f32", "bf16") and 0 <= R <= MAXR
    assert not (joint and not (R and rg)) and not (alias == "sums" and (act != "none" or mask)) and not (rm and dt == "bf16")
    assert not (mask and act != "none")
    ld = ((F + 7) // 8) * 8 + 8 if ld is None else ld
    return dict(name=name, N=N, Mo=Mo, F=F, why=why, want=tuple(want), want0=tuple(want if want0 is None else want0), dt=dt, act=act,
                mask=mask, R=R, rg=rg, bias=bias, joint=joint, alias=alias, off=off, zoff=off if alias != "no" else zoff, ld=ld,
                ss=Mo * ld + ss_extra, data=data, rm=rm, es=4 if dt == "f32" else 2)


def views(c):
    """(g, dz, y) as plan() takes them"""
    return (c["off"], c["ss"], c["ld"]), (c["zoff"], c["ss"], c["ld"]), (c["off"], c["ss"], c["ld"])


def case_plan(c, wide=None):
    g, dz, y = views(c)
    return plan(c["N"], c["Mo"], c["F"], g, dz, y, c["act"], bool(c["mask"]), c["es"], bool(c["rm"]), wide=wide)


def wanted(c, wide=None):
    return c["want"] if (spmm_wide() if wide is None else wide) else c["want0"]


G, Nw, V4, V8 = GENERIC, NARROW, VEC4, VEC8
CASES = [
    # ---- the generic kernel: 64 columns x 4 row lanes per pass
    _case("gen_f5", 1, 19, 5, "F = 5: one pass, 59 idle column lanes", (G, 0, 16, 2, 1, 0), R=0),
    _case("gen_f36", 3, 37, 36, "F = 36 with two condition terms", (G, 0, 16, 3, 1, 0), R=2, rg=1, joint=1),
    _case("gen_f96", 2, 50, 96, "F = 96: 256 % 24 != 0 keeps an aligned view off the vector kernel; relu", (G, 0, 16, 4, 2, 0), act="relu", R=1),
    _case("gen_f130", 2, 140, 130, "F = 130: column passes of 64, 64 and 2", (G, 0, 16, 9, 3, 0), R=3, rg=1),
    _case("gen_f288", 2, 33, 288, "F = 288, [features | condition]: >= 256 and no multiple of 256", (G, 0, 16, 3, 5, 0), R=2, rg=1, joint=1, act="none"),
    _case("gen_f288_tanh", 1, 20, 288, "the same width through tanh", (G, 0, 16, 2, 5, 0), act="tanh", R=1, data="tanhedge"),
    _case("gen_f64_off1", 2, 37, 64, "F = 64 at a channel offset of one element: rows are not 16-byte aligned; the bound is standalone over g (suspect 2)",
          (G, 0, 16, 3, 1, 2), off=1, zoff=1, rm=1, R=1, rg=1),
    _case("gen_f64_ld67", 2, 37, 64, "F = 64 with ld = 67; relu bound must still cover g (suspect 2)", (G, 0, 16, 3, 1, 2), ld=67, ss_extra=5, rm=1, act="relu"),
    _case("gen_f32_off1_mask", 3, 21, 32, "F = 32 at offset 1 under a mask: bound over g, not over the masked dz (suspect 2)", (G, 0, 16, 2, 1, 2),
          off=1, rm=1, mask=1, act="none", R=2),
    _case("gen_f32_zoff2_tanh", 1, 40, 32, "only dz is off alignment; tanh", (G, 0, 16, 3, 1, 2), zoff=2, rm=1, act="tanh", data="tanhedge"),
    _case("gen_f8_mask", 2, 37, 8, "a mask with F = 8 (F % 32 != 0): bit f & 31 of ONE word per row, on the generic kernel", (G, 0, 16, 3, 1, 0),
          mask=1, act="none", R=1, rg=1),
    _case("gen_f40_mask", 2, 20, 40, "a mask of two words per row, the second with 8 live bits", (G, 0, 16, 2, 1, 0), mask=1, act="none"),
    _case("gen_f64_inplace_off1", 2, 37, 64, "in place on the generic kernel; the standalone bound is taken of g before it is overwritten",
          (G, 0, 16, 3, 1, 2), off=1, alias="inplace", rm=1, act="relu"),
    _case("gen_f36_sums", 2, 37, 36, "dz == g without activation on the generic kernel: sums only, nothing stored", (G, 0, 16, 3, 1, 0),
          act="none", alias="sums", R=2, rg=1),
    _case("gen_f36_bf16", 2, 37, 36, "the generic kernel on bf16 storage", (G, 0, 16, 3, 1, 0), dt="bf16", R=1, rg=1),
    _case("gen_f20_yzero", 2, 37, 20, "y exactly 0 and -0: y > 0 is false; leaky", (G, 0, 16, 3, 1, 0), data="yzero", ld=20, ss_extra=0),
    # ---- the narrow kernel: one row per thread
    _case("nar_f1", 3, 37, 1, "F = 1", (Nw, 0, 16, 3, 1, 0), R=1),
    _case("nar_f2", 3, 37, 2, "F = 2; relu", (Nw, 0, 16, 3, 1, 0), act="relu", R=2, rg=1, joint=1),
    _case("nar_f3", 2, 300, 3, "F = 3, the output layer's width: 19 chunks; tanh", (Nw, 0, 16, 19, 1, 0), act="tanh", R=0),
    _case("nar_f3_yzero", 2, 37, 3, "F = 3 with y = +-0; relu", (Nw, 0, 16, 3, 1, 0), act="relu", data="yzero"),
    _case("nar_f4_off1", 2, 37, 4, "F = 4 at an offset of one element: not vector-eligible", (Nw, 0, 16, 3, 1, 0), off=1, zoff=1, R=1),
    _case("nar_mo1", 3, 1, 3, "Mo = 1: 255 idle threads", (Nw, 0, 16, 1, 1, 0), R=1, rg=1),
    _case("nar_f3_mask", 2, 37, 3, "a mask with F = 3: one word per row", (Nw, 0, 16, 3, 1, 0), mask=1, act="none", R=1),
    _case("nar_r4_rg", 2, 37, 3, "R = 4 with rg: all six terms", (Nw, 0, 16, 3, 1, 0), R=4, rg=1, joint=1),
    _case("nar_f3_bf16", 2, 37, 3, "the narrow kernel on bf16 storage", (Nw, 0, 16, 3, 1, 0), dt="bf16", R=1),
    _case("nar_f2_sums", 2, 37, 2, "sums only on the narrow kernel", (Nw, 0, 16, 3, 1, 0), act="none", alias="sums", R=1),
    _case("nar_f3_inplace", 2, 37, 3, "in place on the narrow kernel; leaky", (Nw, 0, 16, 3, 1, 0), alias="inplace", R=1),
    _case("nar_f3_rm", 2, 37, 3, "a bound asked of the narrow kernel: standalone", (Nw, 0, 16, 3, 1, 2), rm=1, act="relu"),
    # ---- the 4-channel vector kernel: the shuffle ladder from each start
    _case("v4_f4", 2, 37, 4, "cvn = 1: 256 row lanes, six shuffle steps", (V4, 2, 16, 3, 1, 1), rm=1, R=1, rg=1),
    _case("v4_f8", 2, 37, 8, "cvn = 2", (V4, 2, 16, 3, 1, 1), rm=1, act="relu", R=2),
    _case("v4_f16", 2, 37, 16, "cvn = 4", (V4, 2, 16, 3, 1, 1), rm=1, act="tanh", R=1, data="tanhedge"),
    _case("v4_f32", 2, 37, 32, "cvn = 8; a mask", (V4, 2, 16, 3, 1, 1), rm=1, mask=1, act="none", R=2, rg=1, joint=1),
    _case("v4_f64", 3, 50, 64, "cvn = 16", (V4, 2, 16, 4, 1, 1), rm=1, R=4, rg=1),
    _case("v4_f128", 2, 37, 128, "cvn = 32: one shuffle step", (V4, 2, 16, 3, 1, 1), rm=1, act="none", R=1, rg=1),
    _case("v4_f256_bf16_ld", 2, 37, 256, "cvn = 64 (per-lane LDS layout) reached as bf16 with ld = F + 4: rows are 8-byte aligned only",
          (V4, 2, 16, 3, 1, 0), dt="bf16", ld=260, ss_extra=4, R=2, rg=1),
    _case("v4_f768", 2, 20, 768, "F = 768: three passes of 256 (768 % 512 != 0 keeps it off the 8-channel kernel)", (V4, 2, 16, 2, 3, 1), rm=1, R=1, rg=1),
    _case("v4_f768_mask", 1, 20, 768, "three passes under a mask: word f >> 5 of 24", (V4, 2, 16, 2, 3, 1), rm=1, mask=1, act="none", R=1),
    _case("v4_f64_inplace", 2, 37, 64, "in place on the vector kernel: the bound is of g as it was", (V4, 2, 16, 3, 1, 1), rm=1, act="relu", alias="inplace", R=1),
    _case("v4_f64_sums", 2, 37, 64, "dz == g, no activation: sums only; the bound is still written", (V4, 2, 16, 3, 1, 1), rm=1, act="none", alias="sums", R=2, rg=1),
    _case("v4_f32_nobias", 2, 37, 32, "no dbias, no dcoef: dcoef_g alone", (V4, 2, 16, 3, 1, 0), bias=0, R=0, rg=1),
    _case("v4_f32_nothing", 2, 37, 32, "no sum at all: dz and its bound only", (V4, 2, 16, 3, 1, 1), bias=0, rm=1, act="relu"),
    _case("v4_f16_yzero", 2, 37, 16, "y = +-0 on the vector kernel; relu", (V4, 2, 16, 3, 1, 1), act="relu", data="yzero", rm=1),
    _case("v4_f64_mask0", 2, 37, 64, "mask words all zero: dz = +0, the bound stays that of g", (V4, 2, 16, 3, 1, 1), mask=1, act="none", data="mask0", rm=1, R=1),
    _case("v4_f64_mask1", 2, 37, 64, "mask words all ones: dz = g bit for bit", (V4, 2, 16, 3, 1, 1), mask=1, act="none", data="mask1", rm=1, R=1),
    _case("v4_f64_binades", 3, 130, 64, "rows over 24 binades and one all-zero row", (V4, 2, 16, 9, 1, 1), data="binades", rm=1, R=2, rg=1),
    _case("v4_f1280", 1, 20, 1280, "F = 1280: five passes of 256; a row has four bound entries, so the bound is standalone (suspect 1)",
          (V4, 2, 16, 2, 5, 2), rm=1, R=1),
    # ---- the 8-channel vector kernel (the 4-channel one under CAPE_SPMM_WIDE=0)
    _case("v8_f256", 2, 37, 256, "cvn = 32 of eight channels; 4-channel leg: cvn = 64 on fp32", (V8, 1, 16, 3, 1, 1), (V4, 2, 16, 3, 1, 1), rm=1, R=2, rg=1),
    _case("v8_f512", 2, 37, 512, "cvn = 64 of eight channels: per-lane LDS layout; 4-channel leg: two passes", (V8, 1, 16, 3, 1, 1), (V4, 2, 16, 3, 2, 1),
          rm=1, act="relu", R=1, rg=1),
    _case("v8_f1024", 1, 20, 1024, "two passes of 512; 4-channel leg: four passes, every bound entry in use", (V8, 1, 16, 2, 2, 1), (V4, 2, 16, 2, 4, 1),
          rm=1, R=1),
    _case("v8_f2048", 1, 20, 2048, "four passes of 512, every bound entry in use; 4-channel leg: eight passes, standalone", (V8, 1, 16, 2, 4, 1),
          (V4, 2, 16, 2, 8, 2), rm=1, act="relu"),
    _case("v8_f4096", 1, 20, 4096, "eight passes of 512: the bound is standalone (suspect 1)", (V8, 1, 16, 2, 8, 2), (V4, 2, 16, 2, 16, 2), rm=1, mask=1, act="none"),
    _case("v8_f256_bf16", 2, 37, 256, "bf16: read-ahead 2 on the 8-channel kernel", (V8, 2, 16, 3, 1, 0), (V4, 2, 16, 3, 1, 0), dt="bf16", R=2, rg=1),
    _case("v8_f512_bf16_tanh", 2, 37, 512, "bf16, cvn = 64, tanh", (V8, 2, 16, 3, 1, 0), (V4, 2, 16, 3, 2, 0), dt="bf16", act="tanh", data="tanhedge", R=1),
    _case("v8_f512_bf16_ld", 2, 37, 512, "bf16 with ld = F + 4: falls back to four channels per thread", (V4, 2, 16, 3, 2, 0), dt="bf16", ld=516, ss_extra=4, R=1),
    _case("v8_f256_mask", 2, 37, 256, "a mask of eight words per row, eight bits per thread", (V8, 1, 16, 3, 1, 1), (V4, 2, 16, 3, 1, 1), rm=1, mask=1, act="none", R=1, rg=1),
    _case("v8_f256_sums", 2, 37, 256, "sums only on the 8-channel kernel", (V8, 1, 16, 3, 1, 0), (V4, 2, 16, 3, 1, 0), act="none", alias="sums", R=1),
    _case("v8_f512_inplace_bf16", 2, 37, 512, "in place, bf16", (V8, 2, 16, 3, 1, 0), (V4, 2, 16, 3, 2, 0), dt="bf16", act="relu", alias="inplace"),
    # ---- rows and chunks
    _case("rows_lt_rb", 3, 5, 64, "Mo = 5 < RB: eleven of sixteen row lanes idle", (V4, 2, 16, 1, 1, 1), rm=1, R=1),
    _case("rows_rb_plus2", 3, 18, 64, "Mo = RB + 2: a last chunk of two rows, shorter than one read-ahead group", (V4, 2, 16, 2, 1, 1), rm=1, R=1, rg=1),
    _case("rows_rb_plus2_v8", 3, 18, 512, "the same on the 8-channel kernel", (V8, 1, 16, 2, 1, 1), (V4, 2, 16, 2, 2, 1), rm=1, R=1),
    _case("rows_rb_plus2_bf16", 3, 18, 256, "the same with read-ahead 2 on eight channels", (V8, 2, 16, 2, 1, 0), (V4, 2, 16, 2, 1, 0), dt="bf16", R=1),
    _case("rows_mult", 3, 48, 32, "Mo = 3 RB", (V4, 2, 16, 3, 1, 1), rm=1, R=1),
    _case("rows_mo1", 3, 1, 128, "Mo = 1 on the vector kernel", (V4, 2, 16, 1, 1, 1), rm=1, R=1, rg=1),
    _case("rows_mo1_gen", 2, 1, 36, "Mo = 1 on the generic kernel", (G, 0, 16, 1, 1, 0), R=1),
    _case("rows_f4_rlanes", 1, 300, 4, "F = 4, 256 row lanes for 16 rows: read-ahead rows all past the chunk", (V4, 2, 16, 19, 1, 1), rm=1, R=1),
    _case("rb32", 16, 897, 4, "RB = 32: 29 chunks, the last of one row", (V4, 2, 32, 29, 1, 1), R=1, ld=4, rm=1),
    _case("rb64", 16, 1729, 4, "RB = 64: 28 chunks, the last of one row", (V4, 2, 64, 28, 1, 1), R=1, rg=1, ld=4, rm=1),
    _case("rb128", 16, 3458, 4, "RB = 128 (16 x 28 = 448 blocks): the last chunk has two rows", (V4, 2, 128, 28, 1, 1), rm=1, R=1, ld=4),
    _case("rb128_nar", 16, 3458, 3, "RB = 128 on the narrow kernel: half of the threads idle", (Nw, 0, 128, 28, 1, 0), R=1, act="relu", ld=3),
    _case("rb128_gen", 16, 3458, 5, "RB = 128 on the generic kernel: 32 rows per row lane", (G, 0, 128, 28, 1, 0), R=1, ld=5),
    # ---- the final stage
    _case("fin_idle", 1, 37, 40, "3 partials per column: 13 of the 16 lanes get nothing; F % 16 = 8", (G, 0, 16, 3, 1, 0), R=1, rg=1),
    _case("fin_tail", 16, 37, 36, "48 partials: tail loop only; F % 16 = 4", (G, 0, 16, 3, 1, 0), R=2, rg=1, joint=1),
    _case("fin_unrolled_tail", 16, 272, 20, "17 chunks of 16 rows, 272 partials: one unrolled group of 256, then a tail of 16", (G, 0, 16, 17, 1, 0), R=1, rg=1),
    _case("fin_unrolled_tail_v4", 16, 272, 16, "the same after the vector kernel", (V4, 2, 16, 17, 1, 1), R=1, act="relu", rm=1),
    _case("fin_unrolled_only", 16, 256, 8, "256 partials: the unrolled loop alone", (V4, 2, 16, 16, 1, 1), R=0, rm=1),
    # ---- operands
    _case("ops_none_r0", 2, 37, 64, "no activation, no sums but dbias, a separate dz", (V4, 2, 16, 3, 1, 1), act="none", rm=1),
    _case("ops_separate_dcoef", 3, 37, 64, "dcoef and dcoef_g in separate buffers (stride 0 = contiguous)", (V4, 2, 16, 3, 1, 1), R=2, rg=1, rm=1),
    _case("ops_joint", 3, 37, 64, "dcoef and dcoef_g as slices of one [N, R + 1, F] buffer", (V4, 2, 16, 3, 1, 1), R=2, rg=1, joint=1, rm=1),
    _case("ops_rg_only_nobias", 3, 37, 36, "dcoef_g without dcoef or dbias on the generic kernel", (G, 0, 16, 3, 1, 0), bias=0, R=0, rg=1),
    _case("ops_wide_stride", 2, 37, 64, "ld = 2 F and a sample stride far beyond Mo * ld", (V4, 2, 16, 3, 1, 1), ld=128, ss_extra=1024, rm=1, R=1),
]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


# ----------------------------------------------------------------------------------------------------- inputs
def bf16_round(a):
    """float32 -> the float32 value of its bfloat16 rounding (nearest even), as cape_st / cape_stv store it (finite inputs)"""
    u = np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(np.shape(a))


def inputs(c):
    """g, y [N, Mo, F] float32 (bf16-representable in a bf16 case), mask words [N, Mo, ceil(F / 32)] uint32 or None (the bits
    beyond F are random), rowscale [R + 1, Mo] float32 (row R is the ``rg`` row): seeded by the case's name."""
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    N, Mo, F = c["N"], c["Mo"], c["F"]
    f = lambda *s: rng.standard_normal(s).astype(F32)
    g, y = f(N, Mo, F), f(N, Mo, F)
    if c["data"] == "binades":
        e = rng.integers(-12, 13, size=(N, Mo, 1))
        g = (g * np.exp2(e)).astype(F32)
        g[:, Mo // 2, :] = 0
    elif c["data"] == "yzero":
        k = rng.integers(0, 3, size=y.shape)
        y = np.where(k == 0, F32(0.0), np.where(k == 1, F32(-0.0), y)).astype(F32)
    elif c["data"] == "tanhedge":
        k = rng.integers(0, 5, size=y.shape)
        y = np.tanh(y).astype(F32)
        y = np.where(k == 0, F32(1.0), np.where(k == 1, F32(-1.0), np.where(k == 2, (y * F32(1e-4)).astype(F32), y))).astype(F32)
    elif c["act"] == "tanh":
        y = np.tanh(y).astype(F32)
    if c["dt"] == "bf16":
        g, y = bf16_round(g), bf16_round(y)
    mask = None
    if c["mask"]:
        words = (F + 31) // 32
        mask = rng.integers(0, 2 ** 32, size=(N, Mo, words), dtype=np.uint64).astype(np.uint32)
        if c["data"] in ("mask0", "mask1"):
            live = np.zeros(words, np.uint32)
            for w in range(words):
                nb = min(32, F - 32 * w)
                live[w] = np.uint32(0xFFFFFFFF if nb == 32 else (1 << nb) - 1)
            mask = (mask & ~live) if c["data"] == "mask0" else (mask | live)          # (the dead bits stay random)
    rowscale = f(c["R"] + 1, Mo)
    return dict(g=g, y=y, mask=mask, rowscale=rowscale)


def mask_bits(mask, F):
    """boolean [N, Mo, F]: bit f & 31 of word f >> 5"""
    f = np.arange(F)
    return ((mask[:, :, f >> 5] >> (f & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


# ----------------------------------------------------------------------------------------------------- references
def reference(c, d):
    """dict: dz64; dz32 (float32, bit for bit; None for tanh) and dz32r (the float32 restatement: dz32, or numpy's float32
    g * (1 - y * y)); store = what the tensor holds (dz32 in fp32, its bf16 rounding otherwise; None for tanh); the sums dbias
    [F], dcoef [N, R, F], dcoef_g [N, F] in float64 with dbias_abs / dcoef_abs / dcoef_g_abs (None where the case has no such
    output)."""
    g, y = d["g"], d["y"]
    g64 = g.astype(F64)
    if c["mask"]:
        keep = mask_bits(d["mask"], c["F"])
        dz32 = np.where(keep, g, F32(0.0)).astype(F32)
        dz64 = np.where(keep, g64, 0.0)
    elif c["act"] == "none":
        dz32, dz64 = g.copy(), g64
    elif c["act"] == "leaky":
        dz32 = (g * np.where(y > 0, F32(1.0), LEAK).astype(F32)).astype(F32)
        dz64 = g64 * np.where(y > 0, 1.0, 0.2)
    elif c["act"] == "relu":
        dz32 = (g * np.where(y > 0, F32(1.0), F32(0.0)).astype(F32)).astype(F32)
        dz64 = g64 * np.where(y > 0, 1.0, 0.0)
    else:
        dz32 = None
        dz64 = g64 * (1.0 - y.astype(F64) ** 2)
    dz32r = dz32 if dz32 is not None else (g * (F32(1.0) - y * y).astype(F32)).astype(F32)
    terms = dz32.astype(F64) if dz32 is not None else dz64
    out = dict(dz64=dz64, dz32=dz32, dz32r=dz32r, store=None if dz32 is None else dz32 if c["dt"] == "f32" else bf16_round(dz32))
    rs = d["rowscale"].astype(F64)
    R = c["R"]
    out["dbias"] = terms.sum((0, 1)) if c["bias"] else None
    out["dbias_abs"] = np.abs(terms).sum((0, 1)) if c["bias"] else None
    out["dcoef"] = np.einsum("jr,nrf->njf", rs[:R], terms) if R else None
    out["dcoef_abs"] = np.einsum("jr,nrf->njf", np.abs(rs[:R]), np.abs(terms)) if R else None
    out["dcoef_g"] = np.einsum("r,nrf->nf", rs[R], g64) if c["rg"] else None
    out["dcoef_g_abs"] = np.einsum("r,nrf->nf", np.abs(rs[R]), np.abs(g64)) if c["rg"] else None
    return out


SUMS = ("dbias", "dcoef", "dcoef_g")


def bounds_ref(c, d, P):
    """[N, Mo, 4] float32 or None: what rowmax_out holds under plan ``P`` (see the module docstring)"""
    if P[5] == B_NONE:
        return None
    a = np.abs(d["g"])
    rm = np.zeros((c["N"], c["Mo"], 4), F32)
    if P[5] == B_ALONE:
        rm[:, :, 0] = a.max(axis=2)
    else:
        for p, (b, w) in enumerate(pass_columns(P, c["F"])):
            rm[:, :, p] = a[:, :, b:b + w].max(axis=2)
    return rm


def fma32(a, b, c_):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c_, F64)).astype(F32)


def _lane_tree(t, family, cvn):
    """[.., lanes, w] float32 lane sums -> [.., w] in the kernel's order"""
    lanes = t.shape[-2]
    if family == GENERIC:                                      # (l0 + l1) + (l2 + l3)
        return ((t[..., 0, :] + t[..., 1, :]).astype(F32) + (t[..., 2, :] + t[..., 3, :]).astype(F32)).astype(F32)
    if family == NARROW:                                       # xor 32 .. 1 inside each wave, then (w0 + w1) + (w2 + w3)
        v = t.reshape(t.shape[:-2] + (4, 64, t.shape[-1]))
        h = 32
        while h >= 1:
            v = (v[..., :h, :] + v[..., h:2 * h, :]).astype(F32)
            h >>= 1
        v = v[..., 0, :]
        return ((v[..., 0, :] + v[..., 1, :]).astype(F32) + (v[..., 2, :] + v[..., 3, :]).astype(F32)).astype(F32)
    if cvn >= 64:                                              # four lanes through LDS, in index order
        s = t[..., 0, :]
        for l in range(1, lanes):
            s = (s + t[..., l, :]).astype(F32)
        return s
    per = lanes // 4                                           # row lanes of one wave: xor cvn, 2 cvn, .. = neighbours first
    v = t.reshape(t.shape[:-2] + (4, per, t.shape[-1]))
    while v.shape[-2] > 1:
        v = (v[..., 0::2, :] + v[..., 1::2, :]).astype(F32)
    v = v[..., 0, :]
    s = v[..., 0, :]
    for w in range(1, 4):
        s = (s + v[..., w, :]).astype(F32)
    return s


def emulate_sums(c, d, P=None):
    """dbias, dcoef, dcoef_g (None where absent) in float32 in the kernel's order (module docstring)"""
    P = case_plan(c) if P is None else P
    family, RB, chunks = P[0], P[2], P[3]
    N, Mo, F, R = c["N"], c["Mo"], c["F"], c["R"]
    ref = reference(c, d)
    dd = ref["dz32r"]
    terms = [(dd, None)] + [(dd, d["rowscale"][j]) for j in range(R)] + [(d["g"], d["rowscale"][R])]
    part = np.zeros((N, chunks, R + 2, F), F32)
    vw = {VEC4: 4, VEC8: 8}.get(family)
    for b, w in pass_columns(P, F):
        cvn = w // vw if vw else None
        lanes = 4 if family == GENERIC else 256 if family == NARROW else 256 // cvn
        steps = (RB + lanes - 1) // lanes
        for ti, (x, sc) in enumerate(terms):
            z = np.zeros((N, chunks * steps * lanes, w), F32)
            s = np.zeros((chunks * steps * lanes,), F32)
            rows = (np.arange(Mo) // RB) * (steps * lanes) + np.arange(Mo) % RB
            z[:, rows] = x[:, :, b:b + w]
            if sc is not None:
                s[rows] = sc
            z = z.reshape(N, chunks, steps, lanes, w)
            s = s.reshape(1, chunks, steps, lanes, 1)
            t = np.zeros((N, chunks, lanes, w), F32)
            for j in range(steps):
                t = (t + z[:, :, j]).astype(F32) if sc is None else fma32(s[:, :, j], z[:, :, j], t)
            part[:, :, ti, b:b + w] = _lane_tree(t, family, cvn)
    out = dict(dbias=None, dcoef=None, dcoef_g=None)

    def lanes16(p):                                            # [total, ..] -> 16 lanes strided over the partials, then in index order
        tot = p.shape[0]
        acc = np.zeros((16,) + p.shape[1:], F32)
        for i in range(tot):
            acc[i % 16] = (acc[i % 16] + p[i]).astype(F32)
        s = np.zeros(p.shape[1:], F32)
        for l in range(16):
            s = (s + acc[l]).astype(F32)
        return s

    if c["bias"]:
        out["dbias"] = lanes16(part[:, :, 0].reshape(N * chunks, F))
    if R:
        out["dcoef"] = np.stack([np.stack([lanes16(part[n, :, 1 + j]) for j in range(R)]) for n in range(N)])
    if c["rg"]:
        out["dcoef_g"] = np.stack([lanes16(part[n, :, R + 1]) for n in range(N)])
    return out


def sum_fraction(got, ref64, abs_terms):
    """the worst error of ``got`` as a fraction of kernel_bars.sum_bar (inf where a sum without terms is not exactly 0)"""
    err = np.abs(np.asarray(got, F64) - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fr = np.where(abs_terms > 0, err / (kernel_bars.SUM_REL * abs_terms), np.where(err > 0, np.inf, 0.0))
    return float(fr.max())


# ----------------------------------------------------------------------------------------------------- the judges
def judge_dz(c, ref, got):
    """``got``: the float32 value of every stored dz element [N, Mo, F].  List of failures (tanh: none here -- it goes to
    kernel_bars.element_bar)."""
    if ref["store"] is None:
        return []
    if kernel_bars.same_bits(np.ascontiguousarray(got), np.ascontiguousarray(ref["store"])):
        return []
    bad = np.argwhere(kernel_bars.bits(np.ascontiguousarray(got)) != kernel_bars.bits(np.ascontiguousarray(ref["store"])))
    i = tuple(bad[0])
    return ["%s / dz: %d of %d elements differ in their bits (first: %r has %r, wants %r)" % (c["name"], len(bad), got.size, i, got[i], ref["store"][i])]


def judge_sums(c, ref, got):
    """``got``: dict of the three sums as the device wrote them.  (failures, {quantity: fraction of kernel_bars.sum_bar})"""
    fails, figs = [], {}
    for k in SUMS:
        if ref[k] is None:
            continue
        figs[k] = sum_fraction(got[k], ref[k], ref[k + "_abs"])
        if not np.isfinite(np.asarray(got[k])).all() or not figs[k] <= 1.0:
            fails.append("%s / %s: %.3g of the sum bar (2e-6 of sum |terms|)" % (c["name"], k, figs[k]))
    return fails, figs


def judge_bounds(c, d, P, rm, dz_stored):
    """``rm`` [N, Mo, 4] as written: entry by entry the bits of bounds_ref; the maximum over the four entries never below the
    row maximum of g and of the stored dz."""
    want = bounds_ref(c, d, P)
    fails = []
    if not kernel_bars.same_bits(np.ascontiguousarray(rm), want):
        bad = np.argwhere(kernel_bars.bits(np.ascontiguousarray(rm)) != kernel_bars.bits(want))
        i = tuple(bad[0])
        fails.append("%s / row bounds: %d of %d entries differ (first: %r has %r, wants %r)" % (c["name"], len(bad), rm.size, i, rm[i], want[i]))
    top = rm.max(axis=2)
    for what, a in (("g", d["g"]), ("dz", dz_stored)):
        low = top < np.abs(a).max(axis=2)
        if low.any() or not np.isfinite(top).all():
            i = tuple(np.argwhere(low)[0]) if low.any() else (0, 0)
            fails.append("%s / row bounds: %d rows are bounded below max |%s| (first: row %r bound %r, row maximum %r)"
                         % (c["name"], int(low.sum()), what, i, top[i], np.abs(a).max(axis=2)[i]))
    return fails
