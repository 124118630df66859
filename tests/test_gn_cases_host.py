"""No GPU needed: the cases of tests/test_gpu_groupnorm.py (tests/gn_cases.py) reach the forms they are named for, the float64
references are the reference's group norm, and the bars keep their margin.

* The table reaches every value of every field of ``plan()``: each row chunk, each apply form, capped and uncapped grids of
  both apply kernels, ``CL`` above and below ``chunks``, a column tile of one quad, channel counts off a quad.
* ``forward_ref`` / ``backward_ref`` in float64 equal ``oracle.torch_twin.group_norm`` under autograd to 1e-12.
* The float32 restatement and the emulation of the kernel's own formulation stay under HALF of each bar of every required case
  (kernel_bars.element_bar / sum_bar): the condition under which the GPU test may hold the kernels to the whole bar.
* ``plan()`` agrees with ``ops.group_count``, ``ops._want_rm(..., any_width=True)`` and ``ops._pad4`` where the wrapper decides."""
import os
import re
import types

import numpy as np
import pytest

import gn_cases as GN
import kernel_bars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64

KERNELS = ["gn_stat_partial_kernel", "gn_partial_kernel", "gn_final_kernel", "gn_apply_kernel", "gn_apply_rows_kernel",
           "gn_bwd_final_kernel", "gn_bwd_apply_kernel", "gn_bwd_apply_rows_kernel", "gn_param_reduce_batch_kernel"]


def _source():
    with open(os.path.join(ROOT, "cape_amd", "csrc", "groupnorm.hip")) as f:
        return f.read()


def test_the_kernel_list_is_the_source_file():
    src = _source()
    defined = set(re.findall(r"__global__\s+__launch_bounds__\(\d+\)\s+void\s+(\w+)\s*\(", src))
    assert defined == set(KERNELS) and len(defined) == 9
    assert set(re.findall(r"CAPE_LAUNCH\((\w+)", src)) == set(KERNELS)


def test_plan_restates_the_dispatch_of_the_source():
    """The constants plan() rests on, read from groupnorm.hip, and the (N, V) pairs of the chunk forms."""
    src = _source()
    assert "int rb = 128;" in src and "while (rb > 16 && (long long)N * ((V + rb - 1) / rb) < 1024) rb >>= 1;" in src
    assert "if (b > 8192) b = 8192;" in src and "return c4 <= 64 && (c4 & (c4 - 1)) == 0;" in src
    assert src.count("rowmax_out && !gn_rm_fused(C) && C <= 1024") == 2 and "return C / G <= 256;" in src
    m = re.search(r"constexpr int GN_ROWS_MAX = (\d+);", src)
    assert m and src.count("__shared__ unsigned mx[GN_ROWS_MAX];") == 2
    # the rows form runs for every c4 that is no power of two: its blocks hold at most 256 / 3 rows
    most = max(GN.plan(1, 1, C, C, True)["block_rows"] or 0 for C in range(1, 1025))
    assert most == 85 == int(m.group(1))
    for rb, (N, V) in GN.CHUNK_SHAPES.items():
        assert GN.gn_rows(N, V) == rb
    assert GN.gn_rows(2, 6890) == GN.gn_rows(32, 431) == GN.gn_rows(4, 862) == 16          # what the older tests reach
    assert "(int64_t)sizeof(double);" in src and GN.workspace_bytes(3, 37, 38) == 3 * 3 * 2 * 40 * 8


def test_the_table_reaches_every_form():
    plans = [(c, GN.case_plan(c)) for c in GN.CASES]
    names = [c["name"] for c in GN.CASES + GN.PIVOT_CASES]
    assert len(set(names)) == len(names)                                       # (the inputs are seeded by the name)
    assert all(c["why"] for c in GN.CASES)
    assert {p["RB"] for _, p in plans} == {16, 32, 64, 128}
    for rb in (16, 32, 64, 128):                                               # each chunk form with a ragged last chunk
        assert any(p["RB"] == rb and p["chunks"] > 1 and p["last_chunk_rows"] < rb for _, p in plans), rb
    assert {p["form"] for _, p in plans} == {"plain", "fused", "rows", "standalone"}
    for form in ("fused", "rows", "standalone"):                               # each bound form with and without ReLU / dx_add
        sub = [c for c, p in plans if p["form"] == form]
        assert {c["relu"] for c in sub} == {0, 1} and {c["add"] for c in sub} == {0, 1}, form
        C = {c["C"] for c in sub}
        assert any(c["rm"] == 0 and c["C"] in C for c in GN.CASES), form      # the same width with rowmax_out = NULL
    assert {(p["form"], p["capped"]) for _, p in plans} >= {("plain", True), ("plain", False), ("fused", True), ("fused", False),
                                                             ("rows", True), ("rows", False)}
    assert any(p["CL"] > p["chunks"] for _, p in plans) and any(p["CL"] < p["chunks"] and p["chunks"] > 1 for _, p in plans)
    assert {p["CL"] for _, p in plans} >= {1, 8, 64, 256} and {p["cp"] for _, p in plans} >= {1, 4, 32, 256}
    assert {p["Cg"] for _, p in plans} >= {1, 3, 17, 19, 255, 256}
    tiles = [t for _, p in plans for t in p["tiles"]]
    assert any(t["c4n"] == 1 and t["idle_lanes"] > 0 for t in tiles)           # more lanes than rows
    assert any(t["c4n"] == 1 and t["cbase"] == 256 for t in tiles)             # ... as the SECOND tile
    assert any(t["rows_per_lane"] > 1 for t in tiles) and any(t["lanes"] == 4 for t in tiles)
    assert max(len(p["tiles"]) for _, p in plans) == 5                         # C = 1028
    assert {c["C"] % 4 for c in GN.CASES} == {0, 2, 3}
    assert {p["block_rows"] for _, p in plans if p["form"] == "rows"} >= {85, 51, 10, 3, 1}
    assert any(c["V"] == 1 for c in GN.CASES) and any(1 < c["V"] < GN.case_plan(c)["RB"] for c in GN.CASES)
    assert any(c["N"] == 1 for c in GN.CASES)
    assert {c["data"] for c in GN.CASES} == set(GN.DATA_KINDS) - {"pivot"}
    assert {GN.case_plan(c)["RB"] for c in GN.CASES if c["data"] == "offset"} == {16, 32, 64, 128}
    for k in GN.PIVOT_KS:
        assert {GN.case_plan(c)["RB"] for c in GN.PIVOT_CASES if c["k"] == k} == {16, 32, 64, 128}
    # the shapes the issue names
    want = {("rb16_v37", 16, 5), ("rb32_v97", 32, 1), ("rb64_v65", 64, 1), ("rb128_v130", 128, 2)}
    assert {(c["name"], p["RB"], p["last_chunk_rows"]) for c, p in plans if c["name"].startswith("rb") and "_v" in c["name"]} == want
    p = GN.case_plan(GN.by_name("rb128_v130"))
    assert p["tiles"] == [dict(cbase=0, c4n=8, lanes=32, rows_per_lane=4, idle_lanes=0)]
    assert GN.case_plan(GN.by_name("c12_g4_rm"))["block_rows"] == 85 and GN.case_plan(GN.by_name("c20_g5_rm"))["block_rows"] == 51
    assert GN.case_plan(GN.by_name("c260_g2_rm"))["block_rows"] == 3 and GN.case_plan(GN.by_name("c1024_g32_rm"))["block_rows"] == 1
    assert GN.case_plan(GN.by_name("cap_plain"))["capped"] and GN.case_plan(GN.by_name("cap_rows"))["capped"]
    assert GN.case_plan(GN.by_name("c1028_g257_rm"))["form"] == "standalone"


def test_plan_agrees_with_the_wrapper():
    import torch
    from cape_amd import ops
    for c in GN.CASES:
        assert ops._pad4(c["C"]) == GN.case_plan(c)["Cp"]
    for C, G in ((3, 3), (4, 4), (12, 12), (38, 38), (48, 48), (64, 32), (96, 32), (256, 32), (544, 32), (1024, 32)):
        assert ops.group_count(2, C) == G
        assert any(c["C"] == C and c["G"] == G for c in GN.CASES) or C in (12, 38)          # (the table takes wider groups there)
    with pytest.raises(ValueError):
        ops.group_count(2, 260)
    for C in sorted({c["C"] for c in GN.CASES}):
        t = types.SimpleNamespace(shape=(3, 37, C), dtype=torch.float32)
        want = ops._want_rm(t, any_width=True)
        assert want == (bool(ops.H2) and C % 32 == 0)
        form = GN.plan(3, 37, C, C, want)["form"]
        assert form == "plain" if not want else form in ("fused", "rows")
        # the wrapper never asks for bounds at c4 = 3; only a caller of the C entry points reaches that block size
        assert not (want and GN.plan(3, 37, C, C, True)["block_rows"] == 85)


@pytest.mark.parametrize("name", ["c3_g1_rm", "c38_g2_norm", "c96_g32_rm", "c260_g2_norm", "v1", "offset_rb16", "gamma0_c8"])
def test_float64_references_are_the_twin_under_autograd(name):
    import torch
    from oracle import torch_twin as tt
    c = GN.by_name(name)
    d = GN.inputs(c)
    N, V, C, G = c["N"], c["V"], c["C"], c["G"]
    tx, tg, tb = (torch.tensor(d[k].astype(F64), requires_grad=True) for k in ("x", "gamma", "beta"))
    if G == min(32, C):
        ty = tt.group_norm(tx, tg, tb, eps=float(GN.EPS))
    else:                                                                        # the twin's lines with the case's G
        xg = tx.permute(0, 2, 1).reshape(-1, G, C // G, V)
        mean = xg.mean(dim=(2, 3), keepdim=True)
        var = ((xg - mean) ** 2).mean(dim=(2, 3), keepdim=True)
        ty = (((xg - mean) / torch.sqrt(var + float(GN.EPS))).reshape(-1, C, V) * tg.reshape(1, C, 1) + tb.reshape(1, C, 1)).permute(0, 2, 1)
    pre = ty
    if c["relu"]:
        ty = torch.relu(ty)
    loss = (ty * torch.tensor(d["dy"].astype(F64))).sum()
    if d["add"] is not None:
        loss = loss + (tx * torch.tensor(d["add"].astype(F64))).sum()
    loss.backward()
    fwd = GN.forward_ref(d["x"], d["gamma"], d["beta"], G, c["relu"], F64)
    mask = (pre.detach().numpy() > 0) if c["relu"] else None
    bwd = GN.backward_ref(d["x"], d["dy"], d["gamma"], fwd["stats"], G, mask, d["add"], F64)
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert close(fwd["y"], ty.detach().numpy())
    assert close(bwd["dx_add"] if d["add"] is not None else bwd["dx"], tx.grad.numpy())
    assert close(bwd["dgamma_p"].sum(0), tg.grad.numpy()) and close(bwd["dbeta_p"].sum(0), tb.grad.numpy())
    # the tables are what they are named: y from coef, dx from bcoef
    a, b, r, mr = (fwd["coef"][:, i:i + 1] for i in range(4))
    y2 = a * d["x"] + b
    assert close(np.maximum(y2, 0) if c["relu"] else y2, fwd["y"])
    A, B, Cc = (bwd["bcoef"][:, i:i + 1] for i in range(3))
    dm = d["dy"].astype(F64) * (mask if mask is not None else 1.0)
    assert close(A * dm - (B + (d["x"] * r - mr) * Cc), bwd["dx"])
    assert (bwd["dgamma_abs"] >= np.abs(bwd["dgamma_p"]) - 1e-12).all() and (bwd["dbeta_abs"] >= np.abs(bwd["dbeta_p"]) - 1e-12).all()


def margins(c):
    """{quantity: (fraction of its bar the float32 restatement uses, the same of the kernel-order emulation)}"""
    d = GN.inputs(c)
    G, relu = c["G"], c["relu"]
    f64 = GN.forward_ref(d["x"], d["gamma"], d["beta"], G, relu, F64)
    f32 = GN.forward_ref(d["x"], d["gamma"], d["beta"], G, relu, F32)
    emu = GN.emu_forward(d["x"], d["gamma"], d["beta"], G, relu)
    mask = (emu["y"] > 0) if relu else None                                    # the mask of the path under test, as on the GPU
    b64 = GN.backward_ref(d["x"], d["dy"], d["gamma"], f64["stats"], G, mask, d["add"], F64)
    b32 = GN.backward_ref(d["x"], d["dy"], d["gamma"], f32["stats"], G, mask, d["add"], F32)
    bem = GN.emu_backward(d["x"], d["dy"], d["gamma"], emu["stats"], emu["coef"], G, relu, d["add"])
    if relu:
        assert np.array_equal(GN.fma32(emu["coef"][:, 0:1], d["x"], emu["coef"][:, 1:2]) > 0, mask)
    q64, q32, qem = GN.split(c, f64, b64), GN.split(c, f32, b32), GN.split(c, emu, bem)
    deg = GN.degenerate_channels(c)
    out = {}
    for k in q64:
        assert q32[k].dtype == F32 and qem[k].dtype == F32 and q64[k].dtype == F64, k
        out[k] = (GN.element_fraction(q32[k], q32[k], q64[k]), GN.element_fraction(qem[k], q32[k], q64[k]))
    for k in GN.SUM_QUANTITIES:
        scale = b64[k.replace("_p", "_abs")]
        out[k] = (GN.sum_fraction(b32[k], b64[k], scale), GN.sum_fraction(bem[k], b64[k], scale))
    if deg.any():
        z32 = GN.zerovar_fractions(c, d, f32, b32, b64["dgamma_abs"])
        zem = GN.zerovar_fractions(c, d, emu, bem, b64["dgamma_abs"])
        out.update({k: (z32[k], zem[k]) for k in zem})
    return out


WORST = {}


@pytest.mark.parametrize("c", GN.ALL_CASES, ids=lambda c: c["name"])
def test_restatement_and_emulation_leave_half_of_every_bar(c):
    m = margins(c)
    for k, (f32, emu) in m.items():
        for who, v in (("float32 restatement", f32), ("kernel-order emulation", emu)):
            if v >= WORST.get((who, k), (-1.0, ""))[0]:
                WORST[(who, k)] = (v, c["name"])
    line = "  ".join("%s %.2f/%.2f" % (k, a, b) for k, (a, b) in m.items())
    print("%s (float32 / emulation, fractions of the bar): %s" % (c["name"], line))
    bad = {k: v for k, v in m.items() if max(v) > 0.5}
    assert not bad, (c["name"], bad)


def test_print_the_worst_fraction_of_each_bar():
    assert WORST, "runs after the parametrised test above"
    for (who, k), (v, name) in sorted(WORST.items()):
        print("WORST %-24s %-18s %.3f of its bar at %s" % (who, k, v, name))
    assert max(v for v, _ in WORST.values()) <= 0.5


def test_the_special_inputs_are_what_they_claim():
    c = GN.by_name("gamma0_c8")
    d = GN.inputs(c)
    c0, c1 = GN.gamma0_channels(c)
    assert d["gamma"][c0] == 0 and d["beta"][c0] == 0 and d["gamma"][c1] == 0 and d["beta"][c1] > 0
    y = GN.emu_forward(d["x"], d["gamma"], d["beta"], c["G"], 1)["y"]
    assert (y[:, :, c0] == 0).all() and (y[:, :, c1] == d["beta"][c1]).all()
    for name in ("relurow_c12", "relurow_c64", "relurow_c1028"):
        c = GN.by_name(name)
        d = GN.inputs(c)
        assert (d["gamma"] > 0.5).all()
        for y in (GN.emu_forward(d["x"], d["gamma"], d["beta"], c["G"], 1)["y"], GN.forward_ref(d["x"], d["gamma"], d["beta"], c["G"], 1, F64)["y"]):
            assert (y[:, GN.relu_row(c), :] == 0).all() and (y.max(axis=2) > 0).sum() == c["N"] * (c["V"] - 1)
    c = GN.by_name("offset_rb16")
    d = GN.inputs(c)
    st = GN.forward_ref(d["x"], d["gamma"], d["beta"], c["G"], 0, F64)["stats"]
    assert (np.abs(np.abs(st[..., 0]) - 50) < 1).all() and (np.abs(st[..., 1] - 1) < 0.3).all()      # 50 sigma off, sigma 1
    c = GN.by_name("zerovar_relu")
    d = GN.inputs(c)
    n, g = GN.zerovar_where(c)
    assert (d["x"][n, :, g * 3:(g + 1) * 3] == GN.ZV_CONST).all() and d["x"][n].std() > 0.5


def test_every_outlier_pivot_leaves_half_of_the_bar():
    """The family of the module docstring of gn_cases: PIVOT_REQUIRED are exactly the k whose emulated rstd stays under half of
    its bar at every chunk form -- all four with the float64 sums of the kernel, none with the float32 sums it had before."""
    for acc, want in ((F64, set(GN.PIVOT_REQUIRED)), (F32, set())):
        rows = GN.pivot_survey(acc=acc)
        for r in rows:
            print("pivot k = %3d RB = %3d, %s sums: emulated rstd error %.2e, float32 restatement %.2e, half of the bar %.2e"
                  % (r[:2] + (acc.__name__,) + r[2:]))
        assert {k for k in GN.PIVOT_KS if all(e <= half for kk, rb, e, e32, half in rows if kk == k)} == want
    assert set(GN.PIVOT_REQUIRED) == set(GN.PIVOT_KS) and not GN.MEASURED_PIVOT_CASES


def test_the_emulation_of_the_lane_split_on_a_hand_case():
    """_partials against the loop of the kernel written out for one sample and one column tile."""
    rng = np.random.default_rng(3)
    V, C, RB = 37, 12, 16
    e = (rng.standard_normal((1, V, C)) * 1000).astype(F32)
    f = rng.standard_normal((1, V, C)).astype(F32)
    s0, s1 = GN._partials(e, e, f, RB, F32)
    lanes = 256 // 3
    for ch in range(3):
        t0, t1 = np.zeros((lanes, C), F32), np.zeros((lanes, C), F32)
        for rl in range(lanes):
            for r in range(ch * RB + rl, min(V, ch * RB + RB), lanes):
                t0[rl] = t0[rl] + e[0, r]
                t1[rl] = GN.fma32(e[0, r], f[0, r], t1[rl])
        a0, a1 = t0[0].copy(), t1[0].copy()
        for l in range(1, lanes):
            a0, a1 = (a0 + t0[l]).astype(F32), (a1 + t1[l]).astype(F32)
        assert kernel_bars.same_bits(a0, s0[0, ch]) and kernel_bars.same_bits(a1, s1[0, ch])
