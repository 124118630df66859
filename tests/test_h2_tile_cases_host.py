"""No GPU needed: the cases of tests/test_gpu_h2_tiles.py (tests/h2_cases.py) reach the kernels they are named for, and their
judges can tell a wrong chunk from a right one.

* Plans: every forward / data-gradient case of the default leg is put to cape_gconv_fwd_plan_h2 with placeholder pointers (as
  tests/test_host_and_abi.py does) and must report (3, BM, BN, 1); the launch whose row bounds are 20 wide must report another
  family; every weight-gradient case must report (4, ct, ft) from cape_gconv_dw_plan_h2.  The plans are those of the default
  environment: when a kernel-selection knob is set in this process they are queried in a child process without it.
* Judges: the float32 restatement of a case passes; a result with the last chunk of a source dropped, a chunk multiplied from the
  stage three chunks earlier, two sources' weights swapped, one row split with a bound 2^6 too small, or one sign-mask word
  taken from the next column block does not."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import h2_cases as H
from tests.test_h2_numerics import scale_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def default_plans():
    if not any(k in os.environ for k in H.PLAN_KNOBS):
        return H.host_plans()
    env = {k: v for k, v in os.environ.items() if k not in H.PLAN_KNOBS}
    r = subprocess.run([sys.executable, "-m", "tests.h2_cases", "--plans"], env=env, cwd=ROOT, stdout=subprocess.PIPE, timeout=120)
    assert r.returncode == 0
    return json.loads(r.stdout.decode().splitlines()[-1])


@pytest.mark.parametrize("name", sorted(H.expected_host_plans()))
def test_case_reaches_its_kernel(name):
    want, got = H.expected_host_plans()[name], default_plans()[name]
    if want is None:
        assert got[0] != 3, (name, got)                      # row bounds wider than the kernel reads: declined
    else:
        assert list(got[:len(want)]) == want, (name, got, want)


def test_the_cases_cover_every_tile_form():
    """Union of the asserted plan tuples over the default process and the three knob legs."""
    fwd = {(c["tile"], c["dual"]) for c in H.FWD_CASES + H.VIEW_CASES + [c for leg in H.LEG_CASES.values() for c in leg]}
    fwd |= {(c["tile"], False) for c in H.BWD_CASES}
    assert fwd == {((128, 256), False), ((128, 128), False), ((128, 64), False), ((64, 128), False), ((64, 64), False), ((128, 64), True)}
    assert {c["tile"] for c in H.DW_CASES} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert sorted(H.LEG_CASES) == sorted(H.LEG_ENV)
    names = [c["name"] for c in H.FWD_CASES + H.VIEW_CASES + H.BWD_CASES + H.CHAIN_CASES + H.DW_CASES] + \
            [c["name"] for leg in H.LEG_CASES.values() for c in leg]
    assert len(set(names)) == len(names)                     # (the inputs are seeded by the name)


def _case(name):
    return next(c for c in H.FWD_CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _built(name):
    case = _case(name)
    op = H.fwd_operands(case)
    return case, op, H.fwd_reference(case, op)


def _chunks(case):
    """(source, first channel) of every 32-channel chunk in the order the kernels walk them."""
    return [(k, c0) for k in range(case["K"]) for c0 in range(0, case["Ch"], 32)]


def _contrib(case, op, chunk):
    k, c0 = chunk
    return op["xs"][k][:, :, c0:c0 + 32] @ op["W"][k::case["K"]][c0:c0 + 32]


def _corrupted(case, op, how):
    K = case["K"]
    mod = dict(op)
    delta = None
    if how == "last_chunk_dropped":
        xs = [x.copy() for x in op["xs"]]
        xs[K - 2][:, :, -32:] = 0
        mod["xs"] = xs
    elif how == "stale_stage":
        ch = _chunks(case)
        i = len(ch) - 2
        delta = _contrib(case, op, ch[i - 3]) - _contrib(case, op, ch[i])
    elif how == "weights_swapped":
        W = op["W"].copy()
        W[0::K], W[1::K] = op["W"][1::K], op["W"][0::K]
        mod["W"] = W
    elif how == "row_bound_too_small":
        n, r = case["N"] - 1, 100
        bound = max(float(np.abs(x[n, r]).max()) for x in op["xs"])
        s, _ = scale_of(np.float32(bound))
        lim = np.float32(65504.0 / (64.0 * float(s)))        # x * (64 s) saturates at the largest fp16 number
        xs = [x.copy() for x in op["xs"]]
        for x in xs:
            x[n, r] = np.clip(x[n, r], -lim, lim)
        mod["xs"] = xs
    else:
        assert how == "restatement"
    return H.fwd_compute(case, mod, np.float32, acc_delta=delta)


CORRUPTIONS = ["last_chunk_dropped", "stale_stage", "weights_swapped", "row_bound_too_small"]


@pytest.mark.parametrize("name", ["wide_3src_9chunks_F264", "t64_6chunks", "dual_has2_flips_at_3"])
def test_judge_accepts_the_float32_restatement(name):
    case, op, ref = _built(name)
    y, v = _corrupted(case, op, "restatement")
    worst = H.judge_fwd(case, ref, y, H.pack_mask(v > 0) if case["dual"] else None)
    assert 0 < worst < H.BAR


@pytest.mark.parametrize("how", CORRUPTIONS)
@pytest.mark.parametrize("name", ["wide_3src_9chunks_F264", "t64_6chunks"])
def test_judge_rejects_a_wrong_result(name, how):
    case, op, ref = _built(name)
    y, _ = _corrupted(case, op, how)
    assert np.isfinite(y).all() and not np.array_equal(y, _corrupted(case, op, "restatement")[0])
    with pytest.raises(AssertionError):
        H.judge_fwd(case, ref, y)


def test_judge_rejects_a_shifted_mask_word():
    case, op, ref = _built("dual_has2_flips_at_3")
    y, v = _corrupted(case, op, "restatement")
    words = H.pack_mask(v > 0)
    assert np.array_equal(H.unpack_mask(words)[:, :, :case["F"]], v > 0)
    bad = words.copy()
    bad[1, 100, 0] = words[1, 100, 1]                        # the word of the next 32-column block
    assert bad[1, 100, 0] != words[1, 100, 0]
    with pytest.raises(AssertionError, match="sign bits"):
        H.judge_fwd(case, ref, y, bad)
    # bits beyond F (72 columns: the upper 24 bits of word 2) must be zero
    bad = words.copy()
    bad[0, 0, 2] |= np.uint32(1 << 31)
    with pytest.raises(AssertionError, match="columns >= F"):
        H.judge_fwd(case, ref, y, bad)


def test_weight_gradient_and_row_bound_judges():
    case = next(c for c in H.DW_CASES if c["name"] == "dw_128x128_dz2_accumulate")
    op = H.dw_operands(case)
    want = H.dw_compute(case, op)
    f32 = H.dw_compute(case, op, np.float32)
    assert 0 < H.judge_dw(case, want, f32) < H.BAR
    # the second source contracted against dz instead of dz2; the gradient overwritten instead of accumulated
    for wrong in (dict(case, dz2_src=None), dict(case, accumulate=False)):
        op2 = dict(op, g0=op["g0"] if wrong["accumulate"] else None)
        with pytest.raises(AssertionError):
            H.judge_dw(case, want, H.dw_compute(wrong, op2, np.float32))
    # row bounds: the exact four-row maxima pass; a bound from the first 31 columns of a block, or one row's own maximum
    # replaced by a larger one, does not
    rng = np.random.default_rng(0)
    y = rng.standard_normal((2, 11, 70)).astype(np.float32)

    def bounds(cols):
        rm = np.zeros((2, 11, 4), dtype=np.float32)
        for j in range(3):
            blk = np.abs(y[:, :, 32 * j:32 * j + cols]).max(-1)
            g = np.zeros((2, 12), dtype=np.float32)
            g[:, :11] = blk
            rm[:, :, j] = np.repeat(g.reshape(2, 3, 4).max(-1), 4, axis=1)[:, :11]
        return rm

    H.judge_rm(bounds(32), y, 70)
    y[0, 5, 31] = 9.0
    with pytest.raises(AssertionError):
        H.judge_rm(bounds(31), y, 70)
    rm = bounds(32)
    rm[1, 2, 1] *= 4.0
    with pytest.raises(AssertionError):
        H.judge_rm(rm, y, 70)
