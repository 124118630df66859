"""No GPU needed: the cases of tests/test_gpu_contractions.py (tests/contraction_cases.py) reach the kernels they are named for, the
tables cover every form the host path can launch, and the judges can tell a wrong result from a right one.

* Plans: every case is put to cape_gconv_fwd_plan[_bf16] / cape_gconv_dw_plan[_bf16] with placeholder pointers and must report the
  tuple it names.  The plans are those of the default environment: when a kernel-selection knob is set in this process they are
  queried in a child process without it.
* Coverage: the union of the forward cases' (family, BM, BN, layout, dual, storage) is contraction_cases.FWD_FORMS; the union of
  the weight-gradient cases' (storage, id, ct, ft) is tools/record_dw_plans.py EXPECT_TILES without the two-piece kernel, plus the
  plain 128 x 128 tile in both storage types.
* Judges: the float32 restatement of every case passes (bf16 forward: rounded to bf16); results with a chunk dropped, weights
  swapped, a 4-channel tail dropped, the second weight set on the wrong source, a row range left out, dz for dz2, overwrite for
  accumulate, the mid plane dropped, a truncating store or a shifted sign-mask word do not."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import contraction_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c["name"]: c for c in K.all_cases()}


@functools.lru_cache(maxsize=None)
def default_plans():
    if not any(k in os.environ for k in K.PLAN_KNOBS):
        return K.host_plans()
    env = {k: v for k, v in os.environ.items() if k not in K.PLAN_KNOBS}
    r = subprocess.run([sys.executable, "-m", "tests.contraction_cases", "--plans"], env=env, cwd=ROOT, stdout=subprocess.PIPE, timeout=120)
    assert r.returncode == 0
    return json.loads(r.stdout.decode().splitlines()[-1])


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_case_reaches_its_kernel(name):
    case = BY_NAME[name]
    want, got = K.expected_host_plan(case), list(default_plans()[name])
    assert got[:len(want)] == want, (name, got, want)
    if case["kind"] == "fwd":
        if case["not_family"] is not None:
            assert got[0] != case["not_family"], (name, got)
        # a launch the narrow kernel declines: the query answers 4 all the same, and the case names what runs instead
        assert (case["runs"] is not None) == (got[0] == 4 and bool(case["deint"] or case["rank"] or case["bias_off"] or case["ypad"])), name
        if case["runs"] is not None:                         # gemm_plain.h gp_tile: 128 x 32 up to 32 columns, else 64 x 64
            assert case["runs"] == ("plain 128x32" if case["F"] <= 32 else "plain 64x64"), name


def test_the_forward_cases_cover_every_form():
    cases = [c for c in K.FWD_CASES if c["not_family"] is None]
    assert {K.fwd_form(c) for c in cases} == K.FWD_FORMS
    # every family and storage type has a view case
    assert {(c["plan"][0], c["storage"]) for c in K.VIEW_CASES} == {(1, "fp32"), (4, "fp32"), (2, "fp32"), (2, "bf16"), (0, "bf16"), (0, "fp32")}
    # family 1: the edges the table is for
    plain = K.PLAIN_CASES
    assert {1, 3, 30, 33, 48, 70} <= {c["F"] for c in plain}
    assert {1, 65, 129} <= {c["Mo"] for c in plain}
    chunks = {sum(-(-ch // 32) for ch, _ in c["srcs"]) for c in plain}
    assert {1, 2, 3, 8} <= chunks
    assert any(len(c["srcs"]) == 8 for c in plain) and any(ch == 36 for c in plain for ch, _ in c["srcs"])
    assert any(ch % 4 and ld > ch for c in plain for ch, ld in c["srcs"])
    assert {(c["w2"] == 0, c["w2"] == len(c["srcs"]) - 1) for c in plain if c["dual"]} == {(True, False), (False, True)}
    for tile in ((64, 64), (128, 32)):
        mine = [c for c in plain if c["plan"][1:] == tile and not c["dual"]]
        assert any(c["rank"] for c in mine) and any(c["bias"] == "vertex" for c in mine) and any(c["act"] == "tanh" for c in mine), tile
    assert {c["deint"] for c in plain} >= {2, 3} and any(c["dual"] and c["to2"] for c in plain)
    assert sum(1 for c in K.NARROW_CASES if c["runs"]) == 4 and sum(1 for c in K.NARROW_CASES if c["not_family"] == 4) == 2
    assert "tanh" not in {c["act"] for c in K.FWD_CASES if c["storage"] == "bf16"}


def test_the_weight_gradient_cases_cover_every_form():
    import record_dw_plans as R
    want = {(s, k, t) for (s, k), tiles in R.EXPECT_TILES.items() if k != 4 for t in tiles} | {("fp32", 1, (128, 128)), ("bf16", 1, (128, 128))}
    assert {(c["storage"], c["kid"], c["tile"]) for c in K.ALL_DW_CASES} == want
    kernels = {("fp32", k) for k in (K.GENERIC, K.PLAIN, K.PACKED, K.SPLIT, K.NARROW_IN, K.NARROW_OUT)} | \
              {("bf16", k) for k in (K.GENERIC, K.PLAIN, K.PACKED, K.SPLIT)}
    for storage, kid in kernels:
        mine = [c for c in K.ALL_DW_CASES if (c["storage"], c["kid"]) == (storage, kid)]
        assert any((c["N"], c["Mo"], c["slabs"]) == (3, 300, 9) for c in mine), (storage, kid)
        assert any(c["slabs"] is not None and c["N"] > c["slabs"] for c in mine), (storage, kid)       # more samples than groups
        assert any(c["accumulate"] for c in mine) and any(c["lead"] for c in mine), (storage, kid)
        if kid in (K.GENERIC, K.PLAIN, K.SPLIT):
            assert any(c["dz2"] and len(c["srcs"]) == 2 for c in mine), (storage, kid)
    big = [c for c in K.ALL_DW_CASES if c["aligned"] and sum(ch for ch, _ in c["srcs"]) * c["F"] >= 262144]
    assert {c["accumulate"] for c in big if c["storage"] == "fp32"} == {False, True}


def test_plans_command_lists_every_case(capsys):
    assert K.main(["--plans"]) == 0
    listed = json.loads(capsys.readouterr().out.splitlines()[-1])
    assert sorted(listed) == sorted(BY_NAME) and all(len(p) == 4 for p in listed.values())


def test_case_names_are_unique():
    names = [c["name"] for c in K.all_cases()]
    assert len(set(names)) == len(names)                     # (the inputs are seeded by the name)


@functools.lru_cache(maxsize=None)
def _built(name):
    case = BY_NAME[name]
    if case["kind"] == "fwd":
        op = K.fwd_operands(case)
        return case, op, K.fwd_reference(case, op)
    op = K.dw_operands(case)
    return case, op, (K.dw_compute(case, op), K.dw_compute(case, op, np.float32))


def _restated(case, op, store=K.bf16_round):
    y, v = K.fwd_compute(case, op, np.float32)
    if case["storage"] == "bf16":
        y = store(y)
    return y, v


@pytest.mark.parametrize("name", [c["name"] for c in K.FWD_CASES])
def test_forward_judge_accepts_the_float32_restatement(name):
    case = BY_NAME[name]
    op = K.fwd_operands(case)
    ref = K.fwd_reference(case, op)
    y, v = _restated(case, op)
    worst = K.judge_fwd(case, ref, y, K.pack_mask(v > 0) if case["dual"] else None)
    assert 0 < worst <= (1.0 if case["storage"] == "bf16" else K.kernel_bars.TOL)
    if case["dual"]:
        assert K.dual_mask_caps(case, ref) <= 0.01           # judge_mask's cap on unjudged positions


@pytest.mark.parametrize("name", [c["name"] for c in K.FWD_CASES if c["storage"] == "bf16"])
def test_bf16_operands_need_both_weight_planes(name):
    case, op, ref = _built(name)
    for x in op["xs"]:
        assert np.array_equal(K.bf16_round(x), x)
    for W in op["Ws"] + ([op["Wa"]] if case["dual"] else []):
        hi, mid = K.weight_planes(W)
        assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64), W.astype(np.float64))
        assert (mid != 0).mean() > 0.9


def _zeroed(xs, k, sl):
    xs = [x.copy() for x in xs]
    xs[k][:, :, sl] = 0
    return xs


def _corrupted(case, op, how):
    """The float32 restatement of a kernel that is wrong in one way."""
    last = len(op["xs"]) - 1
    store = K.bf16_round
    if how == "last_chunk_dropped":
        C = case["srcs"][0][0]
        case2, op2 = case, dict(op, xs=_zeroed(op["xs"], 0, slice((C - 1) // 32 * 32, None)))
    elif how == "weights_swapped":
        assert op["Ws"][0].shape == op["Ws"][last].shape and last > 0
        Ws = list(op["Ws"])
        Ws[0], Ws[last] = Ws[last], Ws[0]
        case2, op2 = case, dict(op, Ws=Ws)
    elif how == "tail_dropped":
        k = next(i for i, (ch, _) in enumerate(case["srcs"]) if ch == 36)
        case2, op2 = case, dict(op, xs=_zeroed(op["xs"], k, slice(32, 36)))
    elif how == "w2_on_wrong_source":
        assert op["xs"][0].shape == op["xs"][last].shape and last > 0
        case2, op2 = dict(case, w2=last - case["w2"]), op
    elif how == "mid_plane_dropped":
        case2, op2 = case, dict(op, Ws=[K.weight_planes(W)[0] for W in op["Ws"]])
    else:
        assert how == "truncating_store"
        case2, op2, store = case, op, K.bf16_trunc
    return _restated(case2, op2, store)


REJECTED = [
    ("plain_64x64_nc_F72", "last_chunk_dropped"), ("plain_64x64_nc_F72", "weights_swapped"), ("plain_64x64_nc_F72", "tail_dropped"),
    ("plain_64x64_kc_F70", "tail_dropped"), ("plain_128x32_kc_F3", "weights_swapped"), ("plain_128x32_nc_padded", "weights_swapped"),
    ("plain_8src_F33", "last_chunk_dropped"), ("plain_64x64_rank", "tail_dropped"),
    ("plain_dual128x32_nc_F32", "w2_on_wrong_source"), ("plain_dual128x64_kc_F48", "w2_on_wrong_source"),
    ("plain_dual128x64_nc_F72", "tail_dropped"), ("narrow_lpr8_idle_quads", "weights_swapped"),
    ("split_64x64_kc", "last_chunk_dropped"), ("split_128x128_nc", "weights_swapped"), ("split_dual128x64_nc", "last_chunk_dropped"),
    ("split_64x64_kc_bf16", "last_chunk_dropped"), ("split_128x128_nc_bf16", "weights_swapped"),
    ("split_64x64_kc_bf16", "mid_plane_dropped"), ("split_64x64_nc_bf16", "mid_plane_dropped"), ("split_128x128_kc_bf16", "mid_plane_dropped"),
    ("split_dual128x64_nc_bf16", "mid_plane_dropped"), ("generic_64x128_bf16", "mid_plane_dropped"),
    ("split_64x64_kc_bf16", "truncating_store"), ("split_64x64_nc_bf16", "truncating_store"), ("split_128x128_kc_bf16", "truncating_store"),
    ("generic_128x32_bf16", "truncating_store"), ("generic_64x128_bf16", "tail_dropped"), ("view_split_bf16", "truncating_store"),
]


@pytest.mark.parametrize("name,how", REJECTED)
def test_forward_judge_rejects_a_wrong_result(name, how):
    case, op, ref = _built(name)
    y, v = _corrupted(case, op, how)
    assert np.isfinite(y).all() and not np.array_equal(y, _restated(case, op)[0])
    with pytest.raises(AssertionError):
        K.judge_fwd(case, ref, y, K.pack_mask(ref["v"] > 0) if case["dual"] else None)


@pytest.mark.parametrize("name", ["plain_dual128x64_nc_F72", "split_dual128x64_nc", "generic_dual128x64_bf16"])
def test_judge_rejects_a_shifted_mask_word(name):
    case, op, ref = _built(name)
    y, v = _restated(case, op)
    words = K.pack_mask(v > 0)
    assert np.array_equal(K.unpack_mask(words)[:, :, :case["F"]], v > 0)
    n, r = case["N"] - 1, case["Mo"] // 2
    bad = words.copy()
    bad[n, r, 0] = words[n, r, 1]                            # the word of the next 32-column block
    assert bad[n, r, 0] != words[n, r, 0]
    with pytest.raises(AssertionError, match="sign bits"):
        K.judge_fwd(case, ref, y, bad)
    bad = words.copy()
    bad[0, 0, -1] |= np.uint32(1 << 31)                      # F = 72: the upper 24 bits of word 2 belong to no column
    with pytest.raises(AssertionError, match="columns >= F"):
        K.judge_fwd(case, ref, y, bad)


@pytest.mark.parametrize("name", [c["name"] for c in K.ALL_DW_CASES])
def test_weight_gradient_judge_accepts_the_float32_restatement(name):
    case, op, (want, f32) = _built(name)
    if case["storage"] == "bf16":
        for a in [op["dz"]] + op["xs"] + ([op["dz2"]] if case["dz2"] else []):
            assert np.array_equal(K.bf16_round(a), a)
    assert 0 <= K.judge_dw(case, want, f32, f32) < K.kernel_bars.TOL


@pytest.mark.parametrize("name", ["dw_generic_64x64", "dw_plain_64x64", "dw_packed_128x32", "dw_split_64x64", "dw_narrow_in_64x64",
                                  "dw_narrow_out_64x64", "dw_split_64x64_bf16", "dw_packed_128x32_F31_bf16"])
def test_weight_gradient_judge_rejects_a_missing_row_range_and_an_overwrite(name):
    case, op, (want, f32) = _built(name)
    assert (case["N"], case["Mo"], case["slabs"], case["accumulate"]) == (3, 300, 9, True)
    for lo, hi in ((0, 128), (128, 256), (256, 300), (288, 300)):                   # each row range; the last one's 12-row chunk
        rows = np.ones(300, bool)
        rows[lo:hi] = False
        with pytest.raises(AssertionError):
            K.judge_dw(case, want, f32, K.dw_compute(case, op, np.float32, rows=rows))
    with pytest.raises(AssertionError):
        K.judge_dw(case, want, f32, K.dw_compute(dict(case, accumulate=False), op, np.float32))


@pytest.mark.parametrize("name", ["dw_plain_128x64_dz2", "dw_split_128x64_dz2", "dw_generic_dz2", "dw_split_dz2_accumulate_bf16"])
def test_weight_gradient_judge_rejects_dz_for_dz2(name):
    case, op, (want, f32) = _built(name)
    with pytest.raises(AssertionError):
        K.judge_dw(case, want, f32, K.dw_compute(dict(case, dz2=False), op, np.float32))
