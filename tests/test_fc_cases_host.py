"""No GPU needed: the cases of tests/test_gpu_fc.py (tests/fc_cases.py) reach the kernels they are named for, name every kernel
and every template instantiation of csrc/fc.hip and csrc/fc_mfma.h, and leave the bars their margin.

* ``tier()`` agrees with the tier every case states, with the MFMA tier on and off.
* The kernels of the two source files are exactly the ones listed here, and each is named by at least one case.
* The float32 restatement of every case stays within a quarter of the bar the GPU test applies: 0.25 * 2e-6 * sum |terms| per
  element for the bare contractions (kernel_bars.sum_bar), 0.25 * 2e-5 max-abs over max-abs for the wide forward behind an
  activation (kernel_bars.element_bar).  The inputs alone must not eat the margin.
* No ``y`` a backward case hands over is exactly 0 under leaky / relu (float32 and float64 then agree on every sign)."""
import os
import re

import numpy as np
import pytest

import fc_cases as F
import kernel_bars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# written out: every kernel of csrc/fc.hip and csrc/fc_mfma.h, every instantiation the dispatcher launches
KERNELS = [
    "fc_long_partial_kernel", "fc_long_final_kernel", "fc_long_bwd_kernel", "fc_wide_fwd_kernel", "fc_wide_bwd_dw_kernel",
    "fc_wide_bwd_dx_partial_kernel", "fc_wide_bwd_dx_final_kernel",
    "fc_long_partial_v4_kernel", "fc_long_bwd_v4_kernel", "fc_wide_fwd_v4_kernel", "fc_wide_bwd_dw_v4_kernel", "fc_wide_bwd_dx_partial_v4_kernel",
    "fc_long_partial_m16_kernel<1>", "fc_long_partial_m16_kernel<2>",
    "fc_long_bwd_m16_kernel<1,1>", "fc_long_bwd_m16_kernel<1,2>", "fc_long_bwd_m16_kernel<2,1>",
    "fc_wide_fwd_m16_kernel<1>", "fc_wide_fwd_m16_kernel<2>", "fc_wide_fwd_m16_kernel<4>",
    "fc_wide_bwd_dw_m16_kernel<1>", "fc_wide_bwd_dw_m16_kernel<2>", "fc_wide_bwd_dw_m16_kernel<4>",
    "fc_wide_bwd_dx_m16_kernel<1>", "fc_wide_bwd_dx_m16_kernel<2>", "fc_wide_bwd_dx_m16_kernel<4>",
]


def _source(name):
    with open(os.path.join(ROOT, "cape_amd", "csrc", name)) as f:
        return f.read()


def test_the_kernel_list_is_the_source_files():
    src = _source("fc.hip") + _source("fc_mfma.h")
    defined = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", src))
    assert defined == {k.split("<")[0] for k in KERNELS}
    launched = set()
    for m in re.finditer(r"CAPE_LAUNCH\(\(?(\w+)(?:<([\d, ]+)>)?", src):
        launched.add(m.group(1) + ("<%s>" % m.group(2).replace(" ", "") if m.group(2) else ""))
    assert launched == set(KERNELS)
    assert sorted(KERNELS) == F.ALL_KERNELS


@pytest.mark.parametrize("c", F.ALL_CASES, ids=lambda c: c["name"])
def test_case_reaches_its_kernel(c):
    assert F.case_tier(c, mfma=True) == c["tier"], (c["name"], c["why"])
    assert F.case_tier(c, mfma=False) == c["tier0"], (c["name"], c["why"])
    assert not any("m16" in k for k in c["tier0"])
    assert c["why"]


def test_the_cases_name_every_kernel():
    named = {k for c in F.ALL_CASES for k in c["tier"]}
    assert named == set(KERNELS)
    off = {k for c in F.ALL_CASES for k in c["tier0"]} - {F.EINVAL[0]}
    assert off == {k for k in KERNELS if "m16" not in k}
    # an MFMA case must move with the knob; the refused ones are the in = 256 data gradients alone
    for c in F.ALL_CASES:
        if any("m16" in k for k in c["tier"]):
            assert c["tier0"] != c["tier"]
        if c["tier0"] == F.EINVAL:
            assert c["entry"] == "wide_bwd" and c["in_"] == 256 and "dx" not in c["null"]
    names = [c["name"] for c in F.ALL_CASES]
    assert len(set(names)) == len(names)                    # (the inputs are seeded by the name)


def test_the_knob_is_read_like_atoi(monkeypatch):
    for v, on in ((None, True), ("1", True), ("0", False), (" 0", False), ("0x1", False), ("off", False), ("2", True), ("-1", True)):
        if v is None:
            monkeypatch.delenv("CAPE_FC_MFMA", raising=False)
        else:
            monkeypatch.setenv("CAPE_FC_MFMA", v)
        assert F.mfma_on() is on, v
    monkeypatch.setenv("CAPE_FC_MFMA", "0")
    c = next(c for c in F.LONG_BWD_CASES if c["name"] == "lb_m12_all")
    assert F.case_tier(c) == c["tier0"] == F.expected_tier(c) == (F.LB_V,)


def test_tier_refuses_what_the_entry_points_refuse():
    t = F.tier
    assert t("long_fwd", 0, 8, 8) == t("long_fwd", 65, 8, 8) == t("long_fwd", 4, 0, 8) == t("long_fwd", 4, 8, 0) == F.EINVAL
    assert t("long_fwd", 4, 8, 8, ld={"x": 7}) == t("long_fwd", 4, 8, 8, nmat=3) == t("long_bwd", 4, 8, 8, nmat=0) == F.EINVAL
    assert t("long_bwd", 4, 8, 8, ld={"dx": 7}) == F.EINVAL and t("long_bwd", 4, 8, 8, ld={"dx": 7}, null=("dx",)) != F.EINVAL
    assert t("long_bwd", 59, 8192, 64, nmat=2) == F.EINVAL and t("long_bwd", 58, 8192, 64, nmat=2) == (F.LB_G,)
    assert t("wide_fwd", 4, 8, 8, act=4) == t("wide_fwd", 4, 8, 8, act=-1) == t("wide_fwd", 4, 8, 8, ld={"y": 7}) == F.EINVAL
    assert t("wide_fwd", 64, 193, 8) == F.EINVAL and t("wide_fwd", 64, 192, 8) == (F.WF_G,)
    assert t("wide_bwd", 4, 8, 8, act=1, null=("y",)) == t("wide_bwd", 4, 8, 8, ld={"g": 7}) == t("wide_bwd", 4, 8, 8, null=("ws",)) == F.EINVAL
    assert t("wide_bwd", 37, 200, 8192) == F.EINVAL and t("wide_bwd", 36, 200, 8192) == (F.DW_G, F.DX_G, F.DXFINAL)
    assert t("wide_bwd", 37, 200, 8192, null=("dx",)) == (F.DW_G,)


def _margin(c):
    d = F.inputs(c)
    ref, f32 = F.reference(c, d, np.float64), F.reference(c, d, np.float32)
    assert sorted(ref) == sorted(f32) and ref
    worst = 0.0
    for k in ref:
        v64, scale = ref[k]
        v32 = f32[k][0]
        assert v32.dtype == np.float32 and v64.dtype == np.float64 and v32.shape == v64.shape == scale.shape, (c["name"], k)
        if F.uses_element_bar(c):
            worst = max(worst, kernel_bars.mat_err(v32, v64) / kernel_bars.TOL)
        else:
            err = np.abs(v32.astype(np.float64) - v64)
            assert (scale > 0).any() and (err[scale == 0] == 0).all(), (c["name"], k)       # (relu can switch a whole sum off)
            worst = max(worst, float((err / np.where(scale > 0, scale, 1.0)).max()) / kernel_bars.SUM_REL)
    return worst


@pytest.mark.parametrize("c", F.ALL_CASES, ids=lambda c: c["name"])
def test_float32_restatement_leaves_three_quarters_of_the_bar(c):
    assert _margin(c) <= 0.25, c["name"]


def test_no_backward_y_is_zero_where_the_sign_matters():
    seen = 0
    for c in F.WIDE_BWD_CASES:
        d = F.inputs(c)
        if c["act"] == 0:
            continue
        y = d["y"]
        assert y is not None and y.dtype == np.float32 and np.isfinite(y).all()
        if c["act"] in (1, 2):
            assert (y != 0).all(), c["name"]
            seen += 1
        else:
            assert (np.abs(y) < 1).all(), c["name"]
    assert seen >= 10


def test_references_on_a_hand_case():
    x = np.array([[1.0, -2.0]], np.float32)
    W = np.array([[3.0, 0.5], [1.0, -1.0]], np.float32)
    b = np.array([0.25, -8.0], np.float32)
    (y, a), = F.long_fwd_ref(x, [W], [b], np.float64)
    assert np.array_equal(y, [[1.25, -5.5]]) and np.array_equal(a, [[5.25, 10.5]])
    for act, want in ((0, [1.25, -5.5]), (1, [1.25, -1.1]), (2, [1.25, 0.0]), (3, np.tanh([1.25, -5.5]))):
        yv, av = F.wide_fwd_ref(x, W, b, act, np.float64)
        assert np.allclose(yv, [want], rtol=1e-15, atol=0) and np.array_equal(av, a)
    g = np.array([[2.0, 4.0]], np.float32)
    yin = np.array([[0.5, -0.5]], np.float32)
    for act, dz in ((0, [2.0, 4.0]), (1, [2.0, 0.8]), (2, [2.0, 0.0]), (3, [1.5, 3.0])):
        r = F.wide_bwd_ref(x, g, yin, act, W, np.float64)
        dz = np.array([dz])
        assert np.allclose(r["dW"][0], x.T.astype(np.float64) @ dz, rtol=1e-15)
        assert np.allclose(r["db"][0], dz[0], rtol=1e-15)
        assert np.allclose(r["dx"][0], dz @ W.T.astype(np.float64), rtol=1e-15)
        assert np.allclose(r["dx"][1], np.abs(dz) @ np.abs(W.T.astype(np.float64)), rtol=1e-15)
    r = F.long_bwd_ref(x, [W, W], [g, -g], np.float64)
    assert np.array_equal(r["dx"][0], [[0.0, 0.0]]) and np.array_equal(r["dx"][1], [[16.0, 12.0]])
    assert np.array_equal(r["dW1"][0], -(x.T.astype(np.float64) @ g)) and np.array_equal(r["db0"][0], [2.0, 4.0])


def test_the_python_gates_admit_only_what_the_entry_points_serve():
    """ops._fc_long_ok / ops._fc_wide_ok against tier(): whatever the alignment of the gradient views and the MFMA knob, a call
    the gates admit is not refused by cape_fc_long_bwd / cape_fc_wide_bwd (the forwards refuse nothing the gates admit)."""
    import types
    from cape_amd import ops
    fake = lambda *shape: types.SimpleNamespace(is_cuda=True, dim=lambda: 2, shape=shape)
    admitted = refused = 0
    for N in range(1, 65):
        for out in (5, 18, 20, 64, 70, 128):
            for nmat in (1, 2):
                ok = ops._fc_long_ok(fake(N, 8192), [fake(8192, out)] * nmat)
                admitted, refused = admitted + ok, refused + (not ok)
                for off in ((), ("dW0",), ("W0", "g0", "dx")):
                    for mfma in (True, False):
                        served = F.tier("long_bwd", N, 8192, out, nmat=nmat, off=off, mfma=mfma) != F.EINVAL
                        assert served or not ok, (N, out, nmat, off, mfma)
        for kin in (3, 50, 64, 128, 192, 200):
            ok = ops._fc_wide_ok(fake(N, kin), kin, 8192)
            admitted, refused = admitted + ok, refused + (not ok)
            for off in ((), ("ws",), ("W", "g", "y", "dW")):
                for mfma in (True, False):
                    for act in (0, 1):
                        served = F.tier("wide_bwd", N, kin, 8192, act=act, off=off, mfma=mfma) != F.EINVAL
                        fwd = F.tier("wide_fwd", N, kin, 8192, act=act, off=off, mfma=mfma) != F.EINVAL
                        assert (served and fwd) or not ok, (N, kin, off, mfma, act)
    assert admitted > 500 and refused > 50
    # the shipped pair (nz = 64) up to batch 58, the shipped decoder input (nz + condition = 128) at every batch
    assert ops._fc_long_ok(fake(58, 55168), [fake(55168, 64)] * 2) and not ops._fc_long_ok(fake(59, 55168), [fake(55168, 64)] * 2)
    assert ops._fc_long_ok(fake(64, 55168), [fake(55168, 64)])
    assert ops._fc_wide_ok(fake(64, 128), 128, 55168) and ops._fc_wide_ok(fake(36, 200), 200, 55168) and not ops._fc_wide_ok(fake(37, 200), 200, 55168)
