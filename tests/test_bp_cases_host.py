"""No GPU needed: the cases of tests/test_gpu_bwd_prep.py (tests/bp_cases.py) reach the forms they are named for, the references
are what they claim, the bars keep their margin and the judges reject corrupted results.

* ``plan()`` rests on the constants of csrc/elementwise.hip and csrc/views.h, equals ``cape_bwd_prep_plan`` (a pure host query:
  called here on addresses that are never dereferenced) on every case, and every case carries the tuple it reaches, by default
  and under CAPE_SPMM_WIDE=0.
* The table reaches every family, read-ahead depth, cvn, pass count, RB, final-stage regime and bound mode, every activation and
  the mask on every family that takes it, every operand form and data kind.
* The float32 restatement of the sums in the kernel's order stays under A QUARTER of kernel_bars.sum_bar; the worst share is
  printed.
* Each judge rejects: one dz element one ulp off, a flipped sign of zero, one chunk's partial dropped from each sum, dcoef_g
  summed over dz, a row bound taken from dz, the bound of pass p stored at p + 1 (and at entry p - 4 of the next row), a mask word
  not shifted by f & 31 at F = 8.
* ``ops.bwd_prep``'s own gates (``_vec_ok``, ``_want_rm``, ``_new_rm``) agree with ``plan()``."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import bp_cases as BP
import kernel_bars
import sparse_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_plan_restates_the_dispatch_of_the_source():
    src, views, hdr = _read("cape_amd", "csrc", "elementwise.hip"), _read("cape_amd", "csrc", "views.h"), _read("include", "cape_hip.h")
    assert "constexpr int BP_RB_MAX = %d;" % BP.BP_RB_MAX in src and "#define CAPE_BP_BLOCKS_DEFAULT %d" % BP.BP_BLOCKS in src
    assert "#define CAPE_BP_RB_MIN_DEFAULT %d" % BP.BP_RB_MIN in src and re.search(r"#define CAPE_BP_UNROLL_DEFAULT %d\b" % BP.BP_UNROLL, src)
    assert "while (rb > rbmin && (long long)N * ((Mo + rb - 1) / rb) < want) rb >>= 1;" in src
    assert "(F >= 256 ? (F % 256) == 0 : (256 % (F / 4)) == 0) && ((F & 31) == 0 || !mask);" in src
    assert "F >= 256 && (F >= 512 ? (F % 512) == 0 : (256 % (F / 8)) == 0);" in src
    assert "const int ur = (wide && es == 4) ? 1 : CAPE_BP_UNROLL_DEFAULT;" in src
    assert "(vec && P.passes <= 4) ? CAPE_BP_BOUND_KERNEL : CAPE_BP_BOUND_STANDALONE" in src
    assert "constexpr int FB = 64 * VW;" in src and "for (int fbase = 0; fbase < F; fbase += 64)" in src
    assert "rm_standalone(g, g_sample_stride, ldg, N, Mo, F, rowmax_out, stream)" in src and "rm_standalone(dz" not in src
    assert "constexpr int RSR_MAXR = %d;" % BP.MAXR in src
    assert "& (4 * es - 1)) == 0) && ((ss & 3) == 0) && ((ld & 3) == 0) && ((C & 3) == 0)" in views
    assert "const int a = es == 4 ? 3 : 7;" in views and "& 15) == 0) && ((ss & a) == 0) && ((ld & a) == 0) && ((C & 7) == 0)" in views
    assert 'getenv("CAPE_SPMM_WIDE") ? atoi(getenv("CAPE_SPMM_WIDE")) : CAPE_SPMM_WIDE_DEFAULT' in views and "#define CAPE_SPMM_WIDE_DEFAULT 1" in views
    for name, v in (("GENERIC", BP.GENERIC), ("NARROW", BP.NARROW), ("VEC4", BP.VEC4), ("VEC8", BP.VEC8), ("BOUND_NONE", BP.B_NONE),
                    ("BOUND_KERNEL", BP.B_KERNEL), ("BOUND_STANDALONE", BP.B_ALONE)):
        assert re.search(r"#define CAPE_BP_%s %d\b" % (name, v), hdr), name
    assert "case CAPE_ACT_LEAKY: return y > 0.f ? 1.f : 0.2f;" in _read("cape_amd", "csrc", "common.h")
    assert BP.bp_rows(2, 6890) == 16 and BP.bp_rows(64, 6890) == 128 and BP.bp_rows(16, 1729) == 64 and BP.bp_rows(2, 431) == 16
    assert BP.workspace_bytes(3, 37, 36, 2) == 3 * 3 * 4 * 36 * 4


def test_the_plan_query_is_declared_bound_and_agrees_with_plan():
    """header, _lib.py, the library and the ABI number agree; cape_bwd_prep_plan[_bf16] == plan() on every case (this process
    runs one leg: the knob is latched; the GPU module's child process runs the other)."""
    from cape_amd import _lib
    hdr = _read("include", "cape_hip.h")
    want = int(re.search(r"#define CAPE_ABI_VERSION (\d+)", hdr).group(1))
    assert want == 18 == _lib.lib.cape_abi_version()
    for name in ("cape_bwd_prep_plan", "cape_bwd_prep_plan_bf16"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M) and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "bounds the rows of g AS THEY ARE ON ENTRY" in hdr and "BEFORE they are rounded" in hdr
    base = 1 << 20
    for c in BP.CASES:
        es = c["es"]
        out = (C.c_int32 * 6)()
        fn = getattr(_lib.lib, "cape_bwd_prep_plan_bf16" if es == 2 else "cape_bwd_prep_plan")
        g, z = base + es * c["off"], (base + es * c["off"]) if c["alias"] != "no" else (2 * base + es * c["zoff"])
        y = (3 * base + es * c["off"]) if (c["act"] != "none" and not c["mask"]) else None
        rc = fn(g, c["ss"], c["ld"], y, c["ss"], c["ld"], BP.ACT[c["act"]], (4 * base) if c["mask"] else None, z, c["ss"], c["ld"],
                c["N"], c["Mo"], c["F"], c["rm"], out)
        assert rc == 0 and tuple(out) == BP.case_plan(c) == BP.wanted(c), (c["name"], tuple(out), BP.case_plan(c), BP.wanted(c))
    out = (C.c_int32 * 6)()
    assert _lib.lib.cape_bwd_prep_plan(None, 0, 8, None, 0, 8, 0, None, base, 0, 8, 1, 1, 8, 0, out) == -1
    assert _lib.lib.cape_bwd_prep_plan(base, 0, 8, None, 0, 8, 1, None, base, 0, 8, 1, 1, 8, 0, out) == -1          # an activation without y
    assert _lib.lib.cape_bwd_prep_plan(base, 0, 8, None, 0, 8, 0, None, base, 0, 8, 1, 1, 8, 0, None) == -1


def test_spmm_wide_is_read_as_atoi_reads_it(monkeypatch):
    for v, want in ((None, True), ("0", False), ("1", True), (" 0", False), ("-1", True), ("+0", False), ("", False), ("x", False), ("2x", True), ("00", False)):
        if v is None:
            monkeypatch.delenv("CAPE_SPMM_WIDE", raising=False)
        else:
            monkeypatch.setenv("CAPE_SPMM_WIDE", v)
        assert BP.spmm_wide() is want, v


def test_the_table_reaches_every_form():
    names = [c["name"] for c in BP.CASES]
    assert len(set(names)) == len(names)                                       # (the inputs are seeded by the name)
    assert all(c["why"] for c in BP.CASES)
    for c in BP.CASES:
        assert BP.case_plan(c, wide=True) == c["want"] and BP.case_plan(c, wide=False) == c["want0"], c["name"]
        assert c["N"] in (1, 2, 3, 16) and (c["Mo"] <= 300 or c["name"].startswith("rb")), c["name"]
        assert c["N"] * c["Mo"] * c["ld"] * c["es"] <= 1200 * 1024, c["name"]
    for wide in (True, False):
        plans = [(c, BP.case_plan(c, wide=wide)) for c in BP.CASES]
        fams = {p[0] for _, p in plans}
        assert fams == ({BP.GENERIC, BP.NARROW, BP.VEC4, BP.VEC8} if wide else {BP.GENERIC, BP.NARROW, BP.VEC4})
        assert {(p[0], p[1]) for _, p in plans if p[0] >= BP.VEC4} == ({(BP.VEC4, 2), (BP.VEC8, 1), (BP.VEC8, 2)} if wide else {(BP.VEC4, 2)})
        for fam in fams:
            sub = [(c, p) for c, p in plans if p[0] == fam]
            assert {c["dt"] for c, _ in sub} == {"f32", "bf16"}, fam
            assert {c["act"] for c, _ in sub if not c["mask"]} == set(BP.ACT), fam            # every activation gate ...
            assert any(c["mask"] for c, _ in sub), fam                                         # ... and the mask
            assert {c["alias"] for c, _ in sub} == set(BP.ALIAS), fam
            assert {p[5] for _, p in sub} >= ({BP.B_NONE, BP.B_ALONE} if fam < BP.VEC4 else {BP.B_NONE, BP.B_KERNEL, BP.B_ALONE}), fam
            assert {c["rg"] for c, _ in sub} == {0, 1} and any(c["R"] for c, _ in sub), fam
        cv = {(p[0], v) for c, p in plans if p[0] >= BP.VEC4 for v in BP.cvns(p, c["F"])}
        assert cv >= {(BP.VEC4, v) for v in (1, 2, 4, 8, 16, 32, 64)}
        assert not wide or cv >= {(BP.VEC8, 32), (BP.VEC8, 64)}
        assert {p[4] for _, p in plans if p[0] == BP.VEC4} >= ({1, 2, 3, 5} if wide else {1, 2, 3, 4, 5, 8, 16})
        assert not wide or {p[4] for _, p in plans if p[0] == BP.VEC8} >= {1, 2, 4, 8}
        assert {p[4] for _, p in plans if p[0] == BP.GENERIC} >= {1, 2, 3, 5}
        # every bound entry in use, and the first shape past that
        assert any(p[5] == BP.B_KERNEL and p[4] == 4 for _, p in plans) and any(p[5] == BP.B_ALONE and p[0] >= BP.VEC4 and p[4] > 4 for _, p in plans)
        assert {p[2] for _, p in plans} == {16, 32, 64, 128}
        assert {BP.final_regime(c["N"], p) for c, p in plans} == {"idle lanes", "tail only", "unrolled + tail", "unrolled only"}
        assert any(c["F"] % 16 and BP.final_regime(c["N"], p) == r for c, p in plans for r in ("unrolled + tail",))
        vecs = [(c, p) for c, p in plans if p[0] >= BP.VEC4]
        assert any(c["Mo"] < p[2] for c, p in vecs) and any(c["Mo"] == p[2] + 2 for c, p in vecs) and any(c["Mo"] % p[2] == 0 and p[3] > 1 for c, p in vecs)
        assert any(c["Mo"] == p[2] + 2 and p[1] == 2 for c, p in vecs) and (not wide or any(c["Mo"] == p[2] + 2 and p[1] == 1 for c, p in vecs))
        assert all(p[5] == (BP.B_NONE if not c["rm"] else p[5]) for c, p in plans) and all(c["rm"] for c, p in vecs if c["dt"] == "f32" and c["R"] + c["rg"] + c["bias"] > 1 and c["alias"] == "no" and c["Mo"] <= 300 and c["name"][:3] in ("v4_", "v8_"))
    assert any(c["Mo"] == 1 for c in BP.CASES) and {c["R"] for c in BP.CASES} == {0, 1, 2, 3, 4}
    assert {c["data"] for c in BP.CASES} == set(BP.DATA_KINDS)
    assert {(c["bias"], bool(c["R"]), c["rg"]) for c in BP.CASES} >= {(1, False, 0), (1, True, 1), (0, False, 1), (0, False, 0), (1, True, 0)}
    assert {c["joint"] for c in BP.CASES if c["R"] and c["rg"]} == {0, 1}
    assert any(c["ld"] > c["F"] + 16 and c["ss"] > c["Mo"] * c["ld"] + 512 for c in BP.CASES)
    # the shapes the issue names
    for name, fam in (("gen_f5", 0), ("gen_f36", 0), ("gen_f96", 0), ("gen_f130", 0), ("gen_f288", 0), ("gen_f64_off1", 0), ("gen_f64_ld67", 0),
                      ("nar_f1", 1), ("nar_f2", 1), ("nar_f3", 1), ("nar_f4_off1", 1), ("nar_mo1", 1), ("nar_f3_mask", 1), ("nar_r4_rg", 1),
                      ("v4_f4", 2), ("v4_f8", 2), ("v4_f16", 2), ("v4_f32", 2), ("v4_f64", 2), ("v4_f128", 2), ("v4_f256_bf16_ld", 2), ("v4_f768", 2),
                      ("v8_f256", 3), ("v8_f512", 3), ("v8_f1024", 3), ("v8_f2048", 3), ("v8_f256_bf16", 3), ("v8_f512_bf16_ld", 2),
                      ("v4_f1280", 2), ("v8_f4096", 3)):
        assert BP.by_name(name)["want"][0] == fam, name
    assert BP.by_name("v8_f256")["want0"][:2] == (BP.VEC4, 2) and BP.cvns(BP.by_name("v8_f256")["want0"], 256) == [64]
    assert BP.by_name("v8_f512")["want0"][4] == 2 and BP.by_name("v8_f1024")["want0"][4:] == (4, BP.B_KERNEL)
    assert BP.by_name("v8_f2048")["want"][4:] == (4, BP.B_KERNEL) and BP.by_name("v4_f1280")["want"][4:] == (5, BP.B_ALONE)
    assert BP.by_name("v8_f4096")["want"][4:] == (8, BP.B_ALONE) and (BP.by_name("v8_f4096")["N"], BP.by_name("v8_f4096")["Mo"]) == (1, 20)
    assert BP.by_name("rb128")["want"][2:4] == (128, 28) and BP.by_name("fin_unrolled_tail")["want"][2:4] == (16, 17)
    assert BP.pass_columns(BP.by_name("gen_f130")["want"], 130) == [(0, 64), (64, 64), (128, 2)]
    for name in ("gen_f64_off1", "gen_f64_ld67", "gen_f32_off1_mask", "gen_f32_zoff2_tanh", "nar_f3_rm"):      # suspect 2: a damped g, a bound asked
        c = BP.by_name(name)
        assert c["want"][5] == BP.B_ALONE and (c["mask"] or c["act"] != "none")


def test_the_special_inputs_are_what_they_claim():
    c = BP.by_name("v4_f64_binades")
    d = BP.inputs(c)
    top = np.abs(d["g"]).max(axis=2)
    assert (top == 0).sum() == c["N"] and np.log2(top[top > 0].max() / top[top > 0].min()) > 20
    for name in ("gen_f20_yzero", "nar_f3_yzero", "v4_f16_yzero"):
        c = BP.by_name(name)
        d = BP.inputs(c)
        z, s = d["y"] == 0, np.signbit(d["y"])
        assert (z & s).sum() > 10 and (z & ~s).sum() > 10
        ref = BP.reference(c, d)
        want = BP.LEAK if c["act"] == "leaky" else F32(0)
        assert kernel_bars.same_bits(ref["dz32"][z], (d["g"][z] * want).astype(F32))            # y = +-0: the y > 0 branch is false
        if c["act"] == "relu":
            assert (np.signbit(ref["dz32"][z]) == np.signbit(d["g"][z])).all() and (ref["dz32"][z] == 0).all()      # -0 under a negative gradient
    for name in ("gen_f288_tanh", "v4_f16", "v8_f512_bf16_tanh"):
        y = BP.inputs(BP.by_name(name))["y"]
        assert (y == 1).sum() > 5 and (y == -1).sum() > 5 and ((np.abs(y) < 1e-3) & (y != 0)).sum() > 5 and np.abs(y).max() <= 1
    for name, bit in (("v4_f64_mask0", False), ("v4_f64_mask1", True)):
        c = BP.by_name(name)
        d = BP.inputs(c)
        assert (BP.mask_bits(d["mask"], c["F"]) == bit).all()
    d = BP.inputs(BP.by_name("gen_f40_mask"))
    assert ((d["mask"][:, :, 1] >> 8) != 0).any()                                # dead bits of the last word are set
    for c in BP.CASES:
        if c["dt"] == "bf16":
            d = BP.inputs(c)
            assert kernel_bars.same_bits(d["g"], BP.bf16_round(d["g"])) and kernel_bars.same_bits(d["y"], BP.bf16_round(d["y"]))


def test_the_references_are_the_formulas_of_the_header():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(200000) * np.exp2(rng.integers(-30, 30, 200000))).astype(F32)
    a[:4] = [0.0, -0.0, 1.00390625, -1.01171875]                                # two ties: to even
    assert np.array_equal(BP.bf16_round(a).astype(F64), sparse_reference.bf16(a))
    assert np.array_equal(np.signbit(BP.bf16_round(a)), np.signbit(a))
    for name in ("gen_f36", "v4_f16", "v4_f32", "gen_f96", "ops_none_r0", "v8_f256_bf16"):
        c = BP.by_name(name)
        d = BP.inputs(c)
        ref = BP.reference(c, d)
        g, y = d["g"].astype(F64), d["y"].astype(F64)
        grad = dict(none=1.0, leaky=np.where(y > 0, 1.0, 0.2), relu=(y > 0) * 1.0, tanh=1 - y * y)[c["act"]]
        want = g * (BP.mask_bits(d["mask"], c["F"]) if c["mask"] else grad)
        assert np.abs(ref["dz64"] - want).max() == 0
        dd = ref["dz32r"].astype(F64)
        assert np.abs(dd - want).max() <= 2.0 ** -23 * np.abs(want).max()
        if c["dt"] == "bf16":
            assert np.array_equal(ref["store"].astype(F64), sparse_reference.bf16(ref["dz32"]))
            assert not np.array_equal(ref["store"], ref["dz32"])                 # the sums below are NOT those of the stored dz
        rs = d["rowscale"].astype(F64)
        terms = dd if c["act"] != "tanh" else want
        assert np.allclose(ref["dbias"], terms.sum((0, 1)), rtol=0, atol=1e-12 * ref["dbias_abs"].max())
        for j in range(c["R"]):
            assert np.allclose(ref["dcoef"][:, j], (rs[j][None, :, None] * terms).sum(1), rtol=0, atol=1e-12 * ref["dcoef_abs"].max())
        if c["rg"]:
            assert np.allclose(ref["dcoef_g"], (rs[c["R"]][None, :, None] * g).sum(1), rtol=0, atol=1e-12 * ref["dcoef_g_abs"].max())
        for k in BP.SUMS:
            if ref[k] is not None:
                assert (ref[k + "_abs"] >= np.abs(ref[k]) - 1e-12).all()


WORST = {}


@pytest.mark.parametrize("c", BP.CASES, ids=lambda c: c["name"])
def test_restatement_leaves_three_quarters_of_every_bar(c):
    d = BP.inputs(c)
    ref = BP.reference(c, d)
    for wide in (True, False):
        P = BP.case_plan(c, wide=wide)
        fails, figs = BP.judge_sums(c, ref, BP.emulate_sums(c, d, P))
        for k, v in figs.items():
            key = (BP.FAMILY[P[0]], k)
            if v >= WORST.get(key, (-1.0, ""))[0]:
                WORST[key] = (v, c["name"])
        assert not fails and all(v <= 0.25 for v in figs.values()), (c["name"], wide, figs)
    if ref["dz32"] is not None:                                                 # the float32 dz is within one rounding of float64
        assert np.abs(ref["dz32"].astype(F64) - ref["dz64"]).max() <= 2.0 ** -23 * max(np.abs(ref["dz64"]).max(), 1e-30)


def test_print_the_worst_share_of_the_sum_bar():
    assert WORST, "runs after the parametrised test above"
    for (fam, k), (v, name) in sorted(WORST.items()):
        print("WORST float32 restatement  %-8s %-8s %.3f of the sum bar at %s" % (fam, k, v, name))
    assert max(v for v, _ in WORST.values()) <= 0.25


def _exact(c, d):
    """what a correct device returns: the stored dz, the float32 roundings of the float64 sums, the bounds"""
    ref = BP.reference(c, d)
    P = BP.case_plan(c)
    got = {k: ref[k].astype(F32) for k in BP.SUMS if ref[k] is not None}
    return ref, P, ref["store"], got, BP.bounds_ref(c, d, P)


def test_the_judges_accept_the_exact_result_and_reject_each_mutation():
    for c in BP.CASES:                                                          # nothing is rejected that is right
        d = BP.inputs(c)
        ref, P, dz, got, rm = _exact(c, d)
        assert not BP.judge_sums(c, ref, got)[0], c["name"]
        if dz is not None:
            assert not BP.judge_dz(c, ref, dz)
            if rm is not None:
                assert not BP.judge_bounds(c, d, P, rm, dz), c["name"]
    # ---- one dz element one ulp off; the sign of a zero
    for name in ("v4_f64", "gen_f36_bf16", "v4_f16_yzero"):
        c = BP.by_name(name)
        d = BP.inputs(c)
        ref, P, dz, got, rm = _exact(c, d)
        bad = dz.copy()
        i = tuple(np.argwhere(bad != 0)[-1])
        step = np.spacing(bad[i]) if c["dt"] == "f32" else F32(np.abs(bad[i]) * 2.0 ** -7)
        bad[i] = bad[i] + step
        assert BP.judge_dz(c, ref, bad) and "1 of" in BP.judge_dz(c, ref, bad)[0]
        z = np.argwhere(dz == 0)
        if len(z):
            bad = dz.copy()
            bad[tuple(z[0])] = -bad[tuple(z[0])]
            assert BP.judge_dz(c, ref, bad)
    # ---- one chunk's partial dropped from each sum
    for name in ("gen_f36", "v4_f64", "fin_unrolled_tail", "nar_r4_rg", "rb128"):
        c = BP.by_name(name)
        d = BP.inputs(c)
        ref, P, dz, got, rm = _exact(c, d)
        RB, n, ch = P[2], c["N"] - 1, P[3] - 1
        rows = slice(ch * RB, min(c["Mo"], ch * RB + RB))
        terms, rs = ref["dz32"].astype(F64)[n, rows], d["rowscale"].astype(F64)
        for k in got:
            bad = {q: v.copy() for q, v in got.items()}
            if k == "dbias":
                bad[k] = (ref[k] - terms.sum(0)).astype(F32)
            elif k == "dcoef":
                bad[k][n] = (ref[k][n] - np.einsum("jr,rf->jf", rs[:c["R"], rows], terms)).astype(F32)
            else:
                bad[k][n] = (ref[k][n] - np.einsum("r,rf->f", rs[c["R"], rows], d["g"].astype(F64)[n, rows])).astype(F32)
            f = BP.judge_sums(c, ref, bad)[0]
            assert len(f) == 1 and ("/ %s:" % k) in f[0], (name, k, f)
    # ---- dcoef_g summed over dz instead of g
    for name in ("gen_f36", "v4_f32", "nar_f2", "v8_f512"):
        c = BP.by_name(name)
        d = BP.inputs(c)
        ref, P, dz, got, rm = _exact(c, d)
        bad = dict(got)
        bad["dcoef_g"] = np.einsum("r,nrf->nf", d["rowscale"][c["R"]].astype(F64), ref["dz64"]).astype(F32)
        f = BP.judge_sums(c, ref, bad)[0]
        assert len(f) == 1 and "dcoef_g" in f[0], name
    # ---- a row bound taken from dz
    for name in ("gen_f64_off1", "gen_f64_ld67", "gen_f32_off1_mask", "nar_f3_rm", "v4_f8", "v8_f512", "v4_f64_mask0"):
        c = BP.by_name(name)
        d = BP.inputs(c)
        ref, P, dz, got, rm = _exact(c, d)
        bad = BP.bounds_ref(c, dict(d, g=dz), P)
        f = BP.judge_bounds(c, d, P, bad, dz)
        assert len(f) == 2 and "below max |g|" in f[1], (name, f)
    # ---- the bound of pass p stored at p + 1; at entry p - 4 of the next row (what a fifth pass did)
    for name in ("v8_f1024", "v4_f768", "v8_f2048"):
        c = BP.by_name(name)
        d = BP.inputs(c)
        ref, P, dz, got, rm = _exact(c, d)
        bad = np.roll(rm.reshape(-1), 1).reshape(rm.shape)
        assert BP.judge_bounds(c, d, P, bad, dz), name
    c = BP.by_name("v4_f1280")
    d = BP.inputs(c)
    ref, P, dz, got, rm = _exact(c, d)
    a = np.abs(d["g"])
    flat = np.zeros(c["N"] * c["Mo"] * 4 + 4, F32)
    for r in range(c["Mo"]):                                                     # five entries per row, in row order
        for p in range(5):
            flat[4 * r + p] = a[0, r, 256 * p:256 * p + 256].max()
    f = BP.judge_bounds(c, d, P, flat[:-4].reshape(rm.shape), dz)
    assert f and "entries differ" in f[0]
    # ---- a mask word not shifted by f & 31 at F = 8
    c = BP.by_name("gen_f8_mask")
    d = BP.inputs(c)
    ref, P, dz, got, rm = _exact(c, d)
    bad = np.where((d["mask"][:, :, :1] & 1).astype(bool), d["g"], F32(0)).astype(F32)          # bit 0 for every column
    assert BP.judge_dz(c, ref, bad)
    bad = np.where(((d["mask"][:, :, :1] >> (np.arange(8) & 3).astype(np.uint32)) & 1).astype(bool), d["g"], F32(0)).astype(F32)      # f & 3
    assert BP.judge_dz(c, ref, bad)


def test_plan_agrees_with_the_gates_of_the_wrapper():
    """ops._vec_ok is aligned4 of the three views; ops._want_rm asks for a bound only where F is a power of two >= 32 on fp32, which
    the kernel then writes itself on every aligned view (at most four passes up to F = 1024 / 2048) -- and ops._new_rm has the
    four entries a row of rowmax_out has."""
    import torch
    from cape_amd import ops
    for c in BP.CASES:
        es, F = c["es"], c["F"]
        for off, ld in ((c["off"], c["ld"]), (c["zoff"], c["ld"])):
            base = torch.empty(c["N"] * c["ss"] + 64, dtype=torch.float32 if es == 4 else torch.bfloat16)
            assert base.data_ptr() % 16 == 0
            t = torch.as_strided(base, (c["N"], c["Mo"], F), (c["ss"], ld, 1), off)
            assert ops._vec_ok(t) == BP.aligned4((off, c["ss"], ld), F, es), c["name"]
        t = types.SimpleNamespace(shape=(c["N"], c["Mo"], F), dtype=torch.float32 if es == 4 else torch.bfloat16)
        want = ops._want_rm(t)
        assert want == (bool(ops.H2) and es == 4 and F >= 32 and F & (F - 1) == 0), c["name"]
    for F in (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192):
        v = (0, 20 * (F + 8), F + 8)
        for wide in (True, False):
            P = BP.plan(1, 20, F, v, v, v, "leaky", False, 4, True, wide=wide)
            assert P[0] >= BP.VEC4 and P[5] == (BP.B_KERNEL if P[4] <= 4 else BP.B_ALONE) and (P[4] <= 4) == (F <= (2048 if wide else 1024))
    t = torch.empty((3, 5, 64))
    assert tuple(ops._new_rm(t).shape) == (3, 5, 4) == BP.bounds_ref(dict(N=3, Mo=5, F=64), dict(g=np.zeros((3, 5, 64), F32)), (2, 2, 16, 1, 1, 1)).shape
