"""Cases, operand builders, float64 / float32 references and judges of the direct tests of the contraction kernels AROUND the fp16
two-piece family (tests/h2_cases.py holds that one).  TEST INFRASTRUCTURE ONLY -- not collected by pytest.

    forward            gemm_plain_kernel (family 1), gemm_split_kernel (family 2, fp32 and bf16 storage), fwd_narrow_in_kernel
                       (family 4), gconv_fwd_kernel (family 0: bf16 storage, and the fp32 128 x 128 tile)
    weight gradient    the generic kernel, dw_plain, dw_packed, dw_split (both storage types), dw_narrow_in, dw_narrow_out, and
                       both slab reductions (dw_reduce_kernel, dw_reduce_vec_kernel)

    tests/test_gpu_contractions.py          runs every case on the device (run_fwd / run_dw)
    tests/test_contraction_cases_host.py    pins every case's kernel plan without a GPU and feeds the judges corrupted results
    python -m tests.contraction_cases --plans    the host plan of every case as one JSON line

A case is a dict; every run_* asserts the EXACT plan tuple the library reports (ops.PLAN_LOG) before it judges, and every judge takes
the device result as a plain numpy array.  Inputs are seeded by the case's name.

Operands.  A source (C, ld) is the slice [lead, lead + C) of a buffer of row pitch ld whose other columns hold NaN -- the pad lane
of a (3, 4) source, the columns an edge tile overhangs, the neighbours of a view.  The output is a slice of a sentinel-filled
buffer: everything outside the output's (row-padded) columns must come back bit for bit; for the view cases everything outside the
view itself.  Weight gradients are views of one sentinel-filled bucket at odd offsets.

Bars (none is new):
  fp32 forward   tests/h2_cases.py's measures -- worst row on its own norm where the epilogue scales with the row, worst row on
                 the tensor's largest row norm for additive terms, max-norm for tanh -- judged with parity_bar.check against the
                 float32 numpy restatement of the same op order, also_below = kernel_bars.TOL.  Rows whose reference is exactly zero
                 must be exactly zero (at most 1 % of the rows).  DUAL cases also go through h2_cases.judge_mask.
  dW             the output is fp32 and the products of bf16 operands are exact, so in both storage types every gradient block
                 gets parity_bar.check on max|got - want| / max|want| against the float32 restatement, also_below = TOL.
  bf16 forward   per element |got - want64| <= half_ulp_bf16(|want64|) + kernel_bars.SUM_REL * sum|terms|: what a correctly
                 rounded store may cost plus the project's figure for a fixed-order fp32 sum.  Elements whose terms are all zero
                 must be exactly zero.  Activations are exact bf16 numbers and weights have at most 16 significant bits
                 (hi + mid, the two planes the kernel stages), so a kernel that drops the second plane cannot pass.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, _HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kernel_bars  # noqa: E402
import parity_bar  # noqa: E402
from tests.h2_cases import (DEV, MASK_FILL, PLAN_KNOBS, _per_row_err, _row_scales, _tensor_err, judge_mask, pack_mask,  # noqa: E402,F401
                            rng_of, unpack_mask)

SENTINEL = -12345.678
DW_SENTINEL = -7.25e33


def _padq(c, q=4):
    return (int(c) + q - 1) // q * q


# --------------------------------------------------------------------------------------------------------------------------
# bf16 number formats on the host
# --------------------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """float32 -> the nearest bf16 number (ties to even), as float32."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000))
    return r.view(np.float32)


def bf16_trunc(a):
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (b & np.uint32(0xFFFF0000)).view(np.float32)


def weight_planes(w):
    """The two planes the bf16-storage kernels stage a float32 weight as: hi = its top 16 bits, mid = the remainder rounded to
    bf16."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    hi = bf16_trunc(w)
    return hi, bf16_round(w - hi)


def weights16(w):
    """``w`` with at most 16 significant bits: hi + mid of its planes (exact in float32)."""
    hi, mid = weight_planes(w)
    return (hi + mid).astype(np.float32)


def half_ulp_bf16(v):
    v = np.abs(np.asarray(v, dtype=np.float64))
    out = np.zeros_like(v)
    nz = v > 0
    out[nz] = 2.0 ** (np.floor(np.log2(v[nz])) - 8)
    return out


# --------------------------------------------------------------------------------------------------------------------------
# forward cases
# --------------------------------------------------------------------------------------------------------------------------
def fwd_case(name, srcs, shape, layout, plan, storage="fp32", w2=None, act=None, bias=None, rank=0, to2=0, deint=0, lead=0, view=False,
             runs=None, bias_off=False, ypad=None, not_family=None):
    """srcs: [(C, ld)]; shape: (N, Mo, F); plan: the first three entries of the plan query (family, BM, BN; family 4: rows per
    pass, F); w2: index of the source that carries the second weight set (DUAL); lead: channel offset of every source in its
    buffer; view: the output is a strict view (nothing outside its F columns may be written); runs: the kernel a launch runs
    that the narrow kernel declines; not_family: a neighbour that must NOT plan this family (plan = what it plans instead)."""
    N, Mo, F = shape
    return dict(kind="fwd", name=name, srcs=[tuple(s) for s in srcs], N=N, Mo=Mo, F=F, layout=layout, plan=tuple(plan), storage=storage,
                w2=w2, dual=w2 is not None, act=act, bias=bias, rank=rank, to2=to2, deint=deint, lead=lead, view=view, runs=runs,
                bias_off=bias_off, ypad=ypad, not_family=not_family)


S32, S36, S64 = (32, 32), (36, 36), (64, 64)
P128, P64, PD32, PD64 = (1, 128, 32), (1, 64, 64), (1, 128, 32), (1, 128, 64)

# ---- family 1: gemm_plain_kernel, 32 channels per chunk
PLAIN_CASES = [
    # the eight forms
    fwd_case("plain_128x32_kc_F3", [S32, S32], (2, 129, 3), "kc", P128),                            # two chunks, last row tile of one row
    fwd_case("plain_128x32_nc_F32", [S64], (2, 129, 32), "nc", P128),
    fwd_case("plain_128x32_nc_padded", [(3, 4), (6, 8), (3, 4)], (2, 129, 12), "nc", P128),       # NaN pad lanes, a source change per chunk
    fwd_case("plain_64x64_nc_F72", [S36, S36], (2, 65, 72), "nc", P64),                             # chunk tails of 4 channels
    fwd_case("plain_64x64_kc_F70", [S36], (2, 65, 70), "kc", P64),
    fwd_case("plain_64x64_nc_F48", [S64], (2, 65, 48), "nc", P64),
    fwd_case("plain_dual128x32_nc_F32", [S32, S32], (2, 129, 32), "nc", PD32, w2=0),                # has2 ends at the source change
    fwd_case("plain_dual128x32_kc_F30", [S32, S32], (2, 129, 30), "kc", PD32, w2=1),                # has2 begins at the source change
    fwd_case("plain_dual128x64_nc_F72", [S36, S36], (2, 129, 72), "nc", PD64, w2=0),
    fwd_case("plain_dual128x64_kc_F48", [S64, S64], (2, 129, 48), "kc", PD64, w2=1),
    # pipeline lengths and edges
    # (F = 1 with a bias: a row of ONE column has no norm of its own to be judged on -- where its 32 terms cancel, the relative
    # error of a correct float32 sum is unbounded -- so the case takes the measure of the additive terms)
    fwd_case("plain_one_chunk_F1", [S32], (2, 129, 1), "kc", P128, bias="channel"),                 # the loop body runs without a load
    fwd_case("plain_one_chunk_Mo1", [(3, 4)], (2, 1, 12), "nc", P128),
    fwd_case("plain_8src_F33", [S32] * 8, (2, 65, 33), "kc", P64),                                  # eight one-chunk sources
    fwd_case("plain_Mo1_F70", [S36, S36], (2, 1, 70), "kc", P64),
    # the general epilogue, once per tile
    fwd_case("plain_64x64_rank", [S36, S36], (2, 65, 72), "nc", P64, rank=2),
    fwd_case("plain_128x32_rank", [S32, S32], (2, 129, 30), "kc", P128, rank=2),
    fwd_case("plain_64x64_vbias_leaky", [S36], (2, 65, 70), "kc", P64, bias="vertex", act="leaky"),
    fwd_case("plain_128x32_vbias_relu", [S64], (2, 129, 32), "nc", P128, bias="vertex", act="relu"),
    fwd_case("plain_64x64_cbias_tanh", [S64], (2, 65, 48), "nc", P64, bias="channel", act="tanh"),
    fwd_case("plain_128x32_cbias_tanh", [S32, S32], (2, 129, 3), "kc", P128, bias="channel", act="tanh"),
    fwd_case("plain_dual128x32_rank_to_acc2", [S32, S32], (2, 129, 32), "nc", PD32, w2=0, rank=2, to2=2),
    fwd_case("plain_dual128x64_rank_to_acc2", [S36, S36], (2, 129, 72), "nc", PD64, w2=1, rank=2, to2=1),
    fwd_case("plain_64x64_deint2", [S36], (2, 65, 72), "kc", P64, deint=2),
    fwd_case("plain_128x32_deint3", [S32, S32], (2, 129, 30), "kc", P128, deint=3),
]

# ---- family 4: fwd_narrow_in_kernel (plan[1] = rows per pass, plan[2] = F)
NARROW_CASES = [
    fwd_case("narrow_lpr4", [(3, 4)], (2, 70, 16), "nc", (4, 64, 16)),
    fwd_case("narrow_lpr8_idle_quads", [(3, 4), (3, 4)], (2, 70, 20), "nc", (4, 32, 20)),
    fwd_case("narrow_lpr64_grid_stride", [(4, 4), (4, 4)], (3, 6890, 256), "nc", (4, 4, 256)),      # 20670 rows > 1024 blocks x 16 rows
    fwd_case("narrow_lpr64_idle_quads", [(3, 4), (5, 8)], (1, 37, 132), "nc", (4, 4, 132)),
    fwd_case("narrow_cbias", [(4, 4), (4, 4)], (2, 70, 256), "nc", (4, 4, 256), bias="channel"),
    fwd_case("narrow_cbias_leaky", [(3, 4)], (2, 70, 16), "nc", (4, 64, 16), bias="channel", act="leaky"),
    fwd_case("narrow_cbias_relu", [(3, 4), (3, 4)], (2, 70, 20), "nc", (4, 32, 20), bias="channel", act="relu"),
    fwd_case("narrow_cbias_tanh", [(3, 4), (5, 8)], (1, 37, 132), "nc", (4, 4, 132), bias="channel", act="tanh"),
    fwd_case("narrow_vbias", [(3, 4)], (2, 70, 16), "nc", (4, 64, 16), bias="vertex"),
    # launches the narrow kernel declines: the plan query still answers 4, gconv_fwd_impl runs gemm_plain_kernel
    fwd_case("narrow_declined_deint2", [(4, 4)], (2, 70, 64), "kc", (4, 16, 64), deint=2, runs="plain 64x64"),
    fwd_case("narrow_declined_rank", [(3, 4)], (2, 70, 16), "nc", (4, 64, 16), rank=2, runs="plain 128x32"),
    fwd_case("narrow_declined_bias_off", [(3, 4)], (2, 70, 16), "nc", (4, 64, 16), bias="channel", bias_off=True, runs="plain 128x32"),
    fwd_case("narrow_declined_ldy", [(3, 4), (3, 4)], (2, 70, 20), "nc", (4, 32, 20), ypad=5, runs="plain 128x32"),
    # neighbours that must not plan 4
    fwd_case("narrow_neighbour_9_channels", [(4, 4), (5, 8)], (2, 70, 16), "nc", P128, not_family=4),
    fwd_case("narrow_neighbour_F260", [(3, 4)], (2, 70, 260), "nc", P64, not_family=4),
]

# ---- family 2: gemm_split_kernel; the same shapes in both storage types
_SPLIT = [
    ("split_64x64_nc", [S32], (2, 65, 64), "nc", (2, 64, 64), {}),
    ("split_64x64_kc", [S64, (96, 96)], (3, 203, 72), "kc", (2, 64, 64), {}),
    ("split_128x128_nc", [S32, S32], (16, 1409, 256), "nc", (2, 128, 128), {}),
    ("split_128x128_kc", [S64], (16, 1409, 200), "kc", (2, 128, 128), {}),
    ("split_dual128x64_nc", [S32, S64], (3, 257, 72), "nc", (2, 128, 64), dict(w2=0)),
    ("split_dual128x64_kc", [S32, S64], (3, 257, 72), "kc", (2, 128, 64), dict(w2=1)),
]
SPLIT_CASES = [fwd_case(n, s, sh, lay, pl, **kw) for n, s, sh, lay, pl, kw in _SPLIT] + [
    fwd_case("split_64x64_rank", [S64, (96, 96)], (3, 203, 72), "kc", (2, 64, 64), rank=2),
    fwd_case("split_64x64_vbias_leaky", [S32], (2, 65, 64), "nc", (2, 64, 64), bias="vertex", act="leaky"),
    fwd_case("split_64x64_cbias_tanh", [S64, (96, 96)], (3, 203, 72), "kc", (2, 64, 64), bias="channel", act="tanh"),
    fwd_case("split_dual_rank_to_acc2", [S32, S64], (3, 257, 72), "nc", (2, 128, 64), w2=0, rank=2, to2=2),
    fwd_case("split_128x128_deint2", [S64], (16, 1409, 256), "kc", (2, 128, 128), deint=2),
]
SPLIT_BF16_CASES = [fwd_case(n + "_bf16", s, sh, lay, pl, storage="bf16", **kw) for n, s, sh, lay, pl, kw in _SPLIT] + [
    fwd_case("split_64x64_rank_bf16", [S64, (96, 96)], (3, 203, 72), "kc", (2, 64, 64), storage="bf16", rank=2),
    fwd_case("split_64x64_vbias_leaky_bf16", [S32], (2, 65, 64), "nc", (2, 64, 64), storage="bf16", bias="vertex", act="leaky"),
    fwd_case("split_128x128_deint2_bf16", [S64], (16, 1409, 256), "kc", (2, 128, 128), storage="bf16", deint=2),
]

# ---- family 0: gconv_fwd_kernel in bf16 storage (F < 64, or channels that are no multiple of 32), and the fp32 128 x 128 tile
GENERIC_CASES = [
    fwd_case("generic_128x32_bf16", [S32], (2, 70, 3), "kc", (0, 128, 32), storage="bf16"),
    fwd_case("generic_128x64_bf16", [S64], (2, 70, 48), "nc", (0, 128, 64), storage="bf16"),
    fwd_case("generic_64x128_bf16", [(36, 40)], (2, 70, 136), "nc", (0, 64, 128), storage="bf16"),
    fwd_case("generic_128x128_bf16", [(36, 40)], (16, 2561, 136), "nc", (0, 128, 128), storage="bf16"),          # 16 * 21 * 2 = 672 >= 640
    fwd_case("generic_dual128x32_bf16", [(36, 40)], (2, 70, 30), "kc", (0, 128, 32), storage="bf16", w2=0),
    fwd_case("generic_dual128x64_bf16", [(36, 40)], (2, 70, 72), "nc", (0, 128, 64), storage="bf16", w2=0),
    # two bf16 launches the split kernel must decline
    fwd_case("generic_declines_3_channels_bf16", [(3, 8)], (2, 70, 72), "nc", (0, 64, 128), storage="bf16"),
    fwd_case("generic_declines_ld36_bf16", [(32, 36)], (2, 70, 72), "nc", (0, 64, 128), storage="bf16"),
    fwd_case("generic_cbias_leaky_bf16", [(36, 40)], (2, 70, 136), "nc", (0, 64, 128), storage="bf16", bias="channel", act="leaky"),
    # fp32: sources 4 bytes off a 16-byte boundary
    fwd_case("generic_128x128_fp32", [(36, 40)], (16, 2561, 136), "nc", (0, 128, 128), lead=1),
]

# ---- channel-offset views next to NaN, output views of a sentinel-filled buffer
VIEW_CASES = [
    fwd_case("view_plain", [(36, 48), (36, 48)], (2, 65, 72), "nc", P64, lead=4, view=True),
    fwd_case("view_plain_dual", [(32, 44), (32, 44)], (2, 129, 32), "nc", PD32, w2=1, lead=4, view=True),
    fwd_case("view_narrow", [(3, 8), (4, 8)], (2, 70, 20), "nc", (4, 32, 20), lead=4, view=True),
    fwd_case("view_split", [(32, 44), (64, 76)], (3, 203, 72), "kc", (2, 64, 64), lead=4, view=True),
    fwd_case("view_split_dual", [(32, 44), (64, 76)], (3, 257, 72), "nc", (2, 128, 64), w2=0, lead=4, view=True),
    fwd_case("view_split_bf16", [(32, 48), (64, 80)], (3, 203, 72), "kc", (2, 64, 64), storage="bf16", lead=8, view=True),
    fwd_case("view_generic_bf16", [(36, 48)], (2, 70, 136), "nc", (0, 64, 128), storage="bf16", lead=3, view=True),
    fwd_case("view_generic_fp32", [(36, 40)], (16, 2561, 136), "nc", (0, 128, 128), lead=3, view=True),
]

FWD_TABLES = dict(plain=PLAIN_CASES, narrow=NARROW_CASES, split=SPLIT_CASES, split_bf16=SPLIT_BF16_CASES, generic=GENERIC_CASES,
                  view=VIEW_CASES)
FWD_CASES = [c for t in FWD_TABLES.values() for c in t]

# the forms the host path can launch outside family 3: (family, BM, BN, layout, dual, storage); family 4 = (4, rows per pass, 0, 0)
FWD_FORMS = {(1, bm, bn, lay, d, "fp32") for (bm, bn, d) in ((128, 32, False), (64, 64, False), (128, 32, True), (128, 64, True))
             for lay in (0, 1)}
FWD_FORMS |= {(2, bm, bn, lay, d, st) for (bm, bn, d) in ((64, 64, False), (128, 128, False), (128, 64, True)) for lay in (0, 1)
              for st in ("fp32", "bf16")}
FWD_FORMS |= {(4, rows, 0, 0, False, "fp32") for rows in (64, 32, 16, 4)}
FWD_FORMS |= {(0, bm, bn, 0, d, "bf16") for (bm, bn, d) in ((128, 32, False), (128, 64, False), (64, 128, False), (128, 128, False),
                                                            (128, 32, True), (128, 64, True))}
FWD_FORMS |= {(0, 128, 128, 0, False, "fp32")}


def fwd_form(case):
    fam, bm, bn = case["plan"]
    lay = 1 if case["layout"] == "kc" else 0
    if fam == 4:
        return (4, bm, 0, 0, False, case["storage"])
    return (fam, bm, bn, lay if fam else 0, case["dual"], case["storage"])


def fwd_plan_tuple(case):
    """What ops.PLAN_LOG must hold after the case's launch."""
    fam, bm, bn = case["plan"]
    lay = (1 if case["layout"] == "kc" else 0) if fam else 0
    return ("fwd", fam, bm, bn, lay, int(case["dual"])) + (("bf16",) if case["storage"] == "bf16" else ())


def additive(case):
    return bool(case["bias"]) or bool(case["rank"])


def fwd_bar_kind(case):
    return "element" if case["act"] == "tanh" else "tensor" if additive(case) else "row"


def _scales(N, Mo, rng, add):
    s = _row_scales(N, Mo, rng, binades=8 if add else 24, large_row=not add)
    if N * Mo < 100:                                         # one exactly-zero row would be more than 1 % of the rows
        s[s == 0] = 1.0
    return s


def fwd_operands(case):
    N, Mo, F = case["N"], case["Mo"], case["F"]
    rng = rng_of(case["name"])
    bf = case["storage"] == "bf16"
    op = {}
    col = 2.0 ** (-rng.integers(0, 12, (1, F))).astype(np.float64)                  # weight columns of different size
    op["Ws"] = [(rng.standard_normal((c, F)) * 0.3 * col).astype(np.float32) for c, _ in case["srcs"]]
    op["Wa"] = (rng.standard_normal((case["srcs"][case["w2"]][0], F)) * 0.2).astype(np.float32) if case["dual"] else None
    scales = _scales(N, Mo, rng, additive(case))
    op["xs"] = [(rng.standard_normal((N, Mo, c)) * scales[:, :, None]).astype(np.float32) for c, _ in case["srcs"]]
    if bf:
        op["Ws"] = [weights16(w) for w in op["Ws"]]
        op["Wa"] = weights16(op["Wa"]) if case["dual"] else None
        op["xs"] = [bf16_round(x) for x in op["xs"]]
    op["bias"] = None
    if case["bias"] == "channel":
        op["bias"] = (rng.standard_normal(F) * 0.5).astype(np.float32)
    elif case["bias"] == "vertex":
        op["bias"] = (rng.standard_normal((Mo, F)) * 0.5).astype(np.float32)
    R = case["rank"]
    op["rowscale"] = rng.standard_normal((R, Mo)).astype(np.float32) if R else None
    op["coef"] = (rng.standard_normal((N, R, F)) * 0.3).astype(np.float32) if R else None
    return op


def _deinterleave(case, full):
    K, F = case["deint"], case["F"]
    stride = _padq(F // K)
    out = np.zeros(full.shape[:2] + (K * stride,), dtype=full.dtype)
    for k in range(K):
        out[:, :, k * stride:k * stride + F // K] = full[:, :, k::K]                # column j = c*K + k -> channel k*stride + c
    return out


def fwd_compute(case, op, dtype=np.float64, absolute=False):
    """The operation in ``dtype``: matmuls summed in source order, then the epilogue.  Returns (y, v): v = what the DUAL form takes
    the sign of (None otherwise).  ``absolute``: the sum of the absolute values of every element's terms instead (float64)."""
    A = (lambda a: np.abs(a.astype(np.float64))) if absolute else (lambda a: a.astype(dtype))
    acc = None
    for x, W in zip(op["xs"], op["Ws"]):
        t = A(x) @ A(W)
        acc = t if acc is None else acc + t
    v, add2 = acc, None
    for j in range(case["rank"]):
        t = A(op["rowscale"][j])[None, :, None] * A(op["coef"][:, j])[:, None, :]
        if absolute:
            t = np.abs(t)
        if case["dual"] and (case["to2"] >> j) & 1:
            add2 = t if add2 is None else add2 + t
        else:
            v = v + t
    if case["dual"]:
        a2 = A(op["xs"][case["w2"]]) @ A(op["Wa"])
        if absolute:
            return v + a2 + (add2 if add2 is not None else 0), v
        y = np.maximum(v, 0) + a2
        if add2 is not None:
            y = y + add2
        return y, v
    if op["bias"] is not None:
        b = A(op["bias"])
        v = v + (b if case["bias"] == "channel" else b[None])
    if absolute:
        y = v
    else:
        act = case["act"]
        y = np.where(v > 0, v, dtype(0.2) * v) if act == "leaky" else np.maximum(v, 0) if act == "relu" else np.tanh(v) if act == "tanh" else v
    if case["deint"]:
        y = _deinterleave(case, y)
    return y, None


def fwd_reference(case, op):
    want, v = fwd_compute(case, op)
    ref = dict(want=want, v=v, f32=fwd_compute(case, op, np.float32)[0], vscale=None, terms=None)
    if case["dual"] or case["storage"] == "bf16":
        ref["terms"], ref["vscale"] = fwd_compute(case, op, absolute=True)
    return ref


def _measure(kind, got, want):
    if kind == "row":
        return _per_row_err(got, want)
    if kind == "tensor":
        return _tensor_err(got, want)
    return float(kernel_bars.mat_err(got, want))


def judge_fwd(case, ref, got, mask=None):
    """``got``: the device result as a numpy array, ``mask``: the DUAL form's sign words.  Returns the worst figure: the error in
    the case's measure (fp32 storage), the largest used share of the allowance (bf16 storage)."""
    got = np.asarray(got, dtype=np.float64)
    want = ref["want"]
    name = case["name"]
    assert got.shape == want.shape and np.isfinite(got).all(), name
    if case["storage"] == "bf16":
        terms = ref["terms"]
        assert np.all(got[terms == 0] == 0), name                                   # (the zero pads of a de-interleaved output too)
        allow = half_ulp_bf16(want) + kernel_bars.SUM_REL * terms
        err = np.abs(got - want)
        nz = terms > 0
        worst = float((err[nz] / allow[nz]).max())
        assert worst <= 1.0, "%s: %d of %d elements beyond half a bf16 ulp + %g sum|terms| (worst %.3f of the allowance)" % (
            name, int((err > allow).sum()), err.size, kernel_bars.SUM_REL, worst)
    else:
        kind = fwd_bar_kind(case)
        if kind == "row":
            n = np.sqrt((want ** 2).sum(-1))
            assert (n == 0).mean() <= 0.01, "more than 1 % exactly-zero rows"
        worst = _measure(kind, got, want)
        parity_bar.check("contractions[%s]" % name, kind, worst, _measure(kind, np.asarray(ref["f32"], np.float64), want),
                         also_below=kernel_bars.TOL)
    if case["dual"]:
        assert mask is not None
        judge_mask(ref["v"], ref["vscale"], mask, want.shape[2])
    return worst


def dual_mask_caps(case, ref):
    """The share of positions judge_mask leaves unjudged on the reference (it asserts its 1 % cap)."""
    return judge_mask(ref["v"], ref["vscale"], pack_mask(ref["v"] > 0), case["F"])


def report(name, tile, worst, kind):
    line = "%-44s %-12s %s %.3e" % (name, "%dx%d" % tuple(tile), kind, worst)
    print(line, flush=True)
    return line


def _dev_operand(a, ld, lead, dtype):
    """``a`` [N, M, C] as the slice [lead, lead + C) of a NaN-filled buffer of row pitch ``ld``."""
    import torch
    N, M, Cn = a.shape
    assert lead + Cn <= ld
    buf = torch.full((N, M, ld), float("nan"), device=DEV, dtype=dtype)
    v = buf[:, :, lead:lead + Cn]
    v.copy_(torch.tensor(a))
    return v


def _dev_out(N, Mo, width, lead, strict, dtype, ypad=None):
    """A [N, Mo, width] view at column ``lead`` of a sentinel-filled buffer, zeroed.  Returns (buffer, view, (lo, hi)): the columns
    outside [lo, hi) must stay the sentinel -- the view itself when ``strict``, else the view with its row padding."""
    import torch
    q = 4 if dtype == torch.float32 else 8
    wpad = width if strict else _padq(width, q)
    buf = torch.full((N, Mo, lead + wpad + (q if ypad is None else ypad)), SENTINEL, device=DEV, dtype=dtype)
    buf[:, :, lead:lead + wpad] = 0
    return buf, buf[:, :, lead:lead + width], (lead, lead + wpad)


def _outside_intact(buf, lo, hi, sentinel=SENTINEL):
    import torch
    b = buf.cpu()
    it = torch.int32 if b.dtype == torch.float32 else torch.int16
    out = torch.cat([b[..., :lo], b[..., hi:]], dim=-1).contiguous()
    return bool(torch.equal(out.view(it), torch.full_like(out, sentinel).view(it)))


def _dev_weight(W, layout):
    import torch
    if layout == "nc":
        t = torch.tensor(W, device=DEV)
        return t, (t, 0, W.shape[1], 1)
    t = torch.tensor(np.ascontiguousarray(W.T), device=DEV)                         # [F, C]
    return t, (t, 0, 1, W.shape[0])


def run_fwd(case):
    import torch
    from cape_amd import _lib, ops
    N, Mo, F = case["N"], case["Mo"], case["F"]
    op = fwd_operands(case)
    dtype = torch.bfloat16 if case["storage"] == "bf16" else torch.float32
    entries, keep = [], []
    for i, ((c, ld), x, W) in enumerate(zip(case["srcs"], op["xs"], op["Ws"])):
        hW, w = _dev_weight(W, case["layout"])
        e = dict(x=_dev_operand(x, ld, case["lead"], dtype), w=w)
        if case["w2"] == i:
            hWa, e["w2"] = _dev_weight(op["Wa"], case["layout"])
            keep.append(hWa)
        entries.append(e)
        keep.append(hW)
    K = case["deint"]
    width = K * _padq(F // K) if K else F
    ybuf, y, (lo, hi) = _dev_out(N, Mo, width, 4 if case["view"] and dtype == torch.float32 else 8 if case["view"] else 0, case["view"],
                                 dtype, case["ypad"])
    mask = torch.full((N, Mo, (F + 31) // 32), MASK_FILL, device=DEV, dtype=torch.int32) if case["dual"] else None
    bias = None
    if op["bias"] is not None:
        if case["bias_off"]:                                                        # 4 bytes off a 16-byte boundary
            bbuf = torch.zeros(F + 4, device=DEV)
            bias = bbuf[1:1 + F]
            bias.copy_(torch.tensor(op["bias"]))
            assert bias.data_ptr() % 16 == 4
        else:
            bias = torch.tensor(op["bias"], device=DEV)
    rank = None
    if case["rank"]:
        rank = (torch.tensor(op["rowscale"], device=DEV), torch.tensor(op["coef"], device=DEV), case["to2"])
    ops.PLAN_LOG = set()
    try:
        ops.gconv_fwd(entries, y, bias=bias, bias_mode=_lib.BIAS_VERTEX if case["bias"] == "vertex" else _lib.BIAS_CHANNEL,
                      act=case["act"] or "none", mask=mask, rank=rank, deinterleave=K, F=F)
        torch.cuda.synchronize()
        plans = set(ops.PLAN_LOG)
    finally:
        ops.PLAN_LOG = None
    assert plans == {fwd_plan_tuple(case)}, (case["name"], plans)
    got = y.float().cpu().numpy()
    worst = judge_fwd(case, fwd_reference(case, op), got, mask.cpu().numpy() if mask is not None else None)
    assert _outside_intact(ybuf, lo, hi), "%s: columns outside the output were written" % case["name"]
    return report(case["name"], case["plan"][1:], worst, "allowance" if case["storage"] == "bf16" else fwd_bar_kind(case))


def plan_fwd_host(case):
    """The case's launch put to cape_gconv_fwd_plan / _bf16 with placeholder pointers (never dereferenced)."""
    from cape_amd import _lib
    bf = case["storage"] == "bf16"
    es = 2 if bf else 4
    n = len(case["srcs"])
    arr = (_lib.CapeSrc * n)()
    for i, (s, (c, ld)) in enumerate(zip(arr, case["srcs"])):
        base = 0x10000000 * (i + 1)
        s.x, s.x_sample_stride, s.ldx, s.C = base + es * case["lead"], case["Mo"] * ld, ld, c
        rs, cs = (case["F"], 1) if case["layout"] == "nc" else (1, c)
        s.w, s.w_rs, s.w_cs = base + 0x4000000, rs, cs
        s.w2, s.w2_rs, s.w2_cs = None, 0, 0
        if case["w2"] == i:
            s.w2, s.w2_rs, s.w2_cs = base + 0x7000000, rs, cs
    out = (C.c_int32 * 4)()
    fn = _lib.lib.cape_gconv_fwd_plan_bf16 if bf else _lib.lib.cape_gconv_fwd_plan
    assert fn(arr, n, case["N"], case["Mo"], case["F"], out) == 0
    return list(out)


# --------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases
# --------------------------------------------------------------------------------------------------------------------------
GENERIC, PLAIN, PACKED, SPLIT, NARROW_IN, NARROW_OUT = 0, 1, 2, 3, 5, 6


def dw_case(name, kid, tile, srcs, F, shape=(2, 70), storage="fp32", slabs=None, dz2=False, accumulate=False, lead=0, lddz=None,
            aligned=False):
    """srcs: [(C, ld)]; shape: (N, Mo); slabs: plan[3] where the case pins it; dz2: the LAST source contracts against dz2; lead:
    channel offset of every operand in its NaN-filled buffer; aligned: gradient blocks at 16-byte offsets (the float4 reduction)."""
    N, Mo = shape
    return dict(kind="dw", name=name, kid=kid, tile=tuple(tile), srcs=[tuple(s) for s in srcs], F=F, N=N, Mo=Mo, storage=storage,
                slabs=slabs, dz2=dz2, accumulate=accumulate, lead=lead, lddz=_padq(F) if lddz is None else lddz,
                aligned=aligned)


NINE = dict(shape=(3, 300), slabs=9)                         # three sample groups x row ranges of 128 / 128 / 44 rows
DW_CASES = [
    # ---- fp32: one case per (kernel, tile) of tools/record_dw_plans.py EXPECT_TILES, plus plain 128 x 128
    dw_case("dw_generic_64x64", GENERIC, (64, 64), [(5, 5)], 8, accumulate=True, **NINE),
    dw_case("dw_generic_128x128", GENERIC, (128, 128), [(70, 70)], 130, lddz=130),
    dw_case("dw_generic_64x128", GENERIC, (64, 128), [(5, 5)], 130, lddz=130),
    dw_case("dw_generic_128x64", GENERIC, (128, 64), [(70, 70)], 9, lddz=9),
    dw_case("dw_plain_64x64", PLAIN, (64, 64), [(3, 4)], 10, accumulate=True, **NINE),
    dw_case("dw_plain_64x128", PLAIN, (64, 128), [(6, 8)], 67),
    dw_case("dw_plain_128x64_dz2", PLAIN, (128, 64), [(128, 128)], 3, dz2=True),
    dw_case("dw_plain_128x128", PLAIN, (128, 128), [(68, 68)], 67),
    dw_case("dw_packed_128x32", PACKED, (128, 32), [S32, S32], 32, accumulate=True, **NINE),
    dw_case("dw_packed_64x64", PACKED, (64, 64), [S32, S32], 64),
    dw_case("dw_packed_128x64", PACKED, (128, 64), [S32] * 3, 64),
    dw_case("dw_packed_128x64_mixed", PACKED, (128, 64), [S32, S64, (4, 4)], 36),
    dw_case("dw_split_64x64", SPLIT, (64, 64), [S64], 64, accumulate=True, **NINE),
    dw_case("dw_split_64x128", SPLIT, (64, 128), [S32, S64], 130, lddz=132),
    dw_case("dw_split_128x64_dz2", SPLIT, (128, 64), [(68, 68), (68, 68)], 34, dz2=True),
    dw_case("dw_split_128x128", SPLIT, (128, 128), [(160, 160)], 192),
    dw_case("dw_narrow_in_64x64", NARROW_IN, (64, 64), [(3, 4)], 16, accumulate=True, **NINE),
    dw_case("dw_narrow_in_64x128", NARROW_IN, (64, 128), [(4, 4), (4, 4)], 256),
    dw_case("dw_narrow_in_64x128_padded", NARROW_IN, (64, 128), [(3, 4), (5, 8)], 132),
    dw_case("dw_narrow_out_64x64", NARROW_OUT, (64, 64), [(16, 16)], 3, accumulate=True, **NINE),
    dw_case("dw_narrow_out_128x32", NARROW_OUT, (128, 32), [S32, S32], 3),
    dw_case("dw_narrow_out_128x64_F4", NARROW_OUT, (128, 64), [(256, 256)], 4),
    dw_case("dw_narrow_out_128x64_F1", NARROW_OUT, (128, 64), [(160, 160)], 1),
    dw_case("dw_narrow_out_128x32_F2", NARROW_OUT, (128, 32), [(12, 12), (8, 8)], 2),
    # ---- fp32: more samples than groups (two samples per group)
    dw_case("dw_split_two_samples_per_group", SPLIT, (128, 128), [(256, 256)] * 8, 512, shape=(16, 40), slabs=8),
    dw_case("dw_generic_two_samples_per_group", GENERIC, (128, 128), [(70, 70)] * 8, 514, shape=(16, 40), slabs=8, lddz=514),
    dw_case("dw_plain_two_samples_per_group", PLAIN, (128, 128), [(68, 68)] * 8, 515, shape=(16, 40), slabs=8),
    dw_case("dw_packed_two_samples_per_group", PACKED, (128, 32), [S32, S32], 32, shape=(1024, 3), slabs=512),
    dw_case("dw_narrow_in_two_samples_per_group", NARROW_IN, (64, 64), [(3, 4)], 16, shape=(1024, 3), slabs=512),
    dw_case("dw_narrow_out_two_samples_per_group", NARROW_OUT, (64, 64), [(16, 16)], 3, shape=(1024, 3), slabs=512),
    # ---- fp32: dz2 on the last of two sources
    dw_case("dw_generic_dz2", GENERIC, (64, 64), [(5, 5), (5, 5)], 8, dz2=True),
    dw_case("dw_plain_dz2", PLAIN, (64, 64), [(3, 4), (3, 4)], 10, dz2=True),
    dw_case("dw_split_dz2_accumulate", SPLIT, (64, 64), [S64, S64], 64, dz2=True, accumulate=True),
    # ---- fp32: operands as channel-offset views whose neighbours hold NaN (the columns an edge tile overhangs)
    dw_case("dw_generic_nan_view", GENERIC, (128, 128), [(70, 81)], 130, lead=3, lddz=141),
    dw_case("dw_plain_nan_view", PLAIN, (64, 128), [(6, 16)], 67, lead=4, lddz=80),
    dw_case("dw_packed_nan_view", PACKED, (128, 32), [(32, 44), (32, 44)], 32, lead=4, lddz=44),
    dw_case("dw_split_nan_view", SPLIT, (128, 128), [(160, 172)], 192, lead=4, lddz=204),
    dw_case("dw_narrow_in_nan_view", NARROW_IN, (64, 64), [(3, 12)], 16, lead=4, lddz=28),
    dw_case("dw_narrow_out_nan_view", NARROW_OUT, (64, 64), [(16, 28)], 3, lead=4, lddz=12),
    # ---- both reductions: C * F >= 262144 at 16-byte block offsets sums its slabs in dw_reduce_vec_kernel, all else in dw_reduce_kernel
    dw_case("dw_reduce_vec", SPLIT, (128, 128), [(512, 512)], 512, shape=(2, 300), aligned=True),
    dw_case("dw_reduce_vec_accumulate", SPLIT, (128, 128), [(512, 512)], 512, shape=(2, 300), aligned=True, accumulate=True),
    dw_case("dw_reduce_scalar_large", SPLIT, (128, 128), [(512, 512)], 512, shape=(2, 300)),
]
B = dict(storage="bf16")
DW_BF16_CASES = [
    # ---- bf16 storage: built from what cape_gconv_dw_plan_bf16 answers (no narrow forms; the split kernel before the packed one)
    dw_case("dw_generic_64x64_bf16", GENERIC, (64, 64), [(5, 5)], 8, accumulate=True, **NINE, **B),
    dw_case("dw_generic_128x128_bf16", GENERIC, (128, 128), [(70, 70)], 130, lddz=130, **B),
    dw_case("dw_generic_64x128_bf16", GENERIC, (64, 128), [(5, 5)], 130, lddz=130, **B),
    dw_case("dw_generic_128x64_bf16", GENERIC, (128, 64), [(70, 70)], 9, lddz=9, **B),
    dw_case("dw_plain_64x64_bf16", PLAIN, (64, 64), [(3, 4)], 10, accumulate=True, **NINE, **B),
    dw_case("dw_plain_64x128_bf16", PLAIN, (64, 128), [(6, 8)], 67, **B),
    dw_case("dw_plain_128x64_dz2_bf16", PLAIN, (128, 64), [(128, 128)], 3, dz2=True, **B),
    dw_case("dw_plain_128x128_bf16", PLAIN, (128, 128), [(68, 68)], 67, **B),
    dw_case("dw_packed_128x32_bf16", PACKED, (128, 32), [S32, S32], 3, **B),
    dw_case("dw_packed_128x32_F31_bf16", PACKED, (128, 32), [S32, S32], 31, accumulate=True, **NINE, **B),
    dw_case("dw_split_64x64_bf16", SPLIT, (64, 64), [S64], 64, accumulate=True, **NINE, **B),
    dw_case("dw_split_64x64_was_packed_bf16", SPLIT, (64, 64), [S32, S32], 32, **B),
    dw_case("dw_split_64x128_bf16", SPLIT, (64, 128), [S32, S64], 130, lddz=132, **B),
    dw_case("dw_split_128x64_dz2_bf16", SPLIT, (128, 64), [(68, 68), (68, 68)], 34, dz2=True, **B),
    dw_case("dw_split_128x128_bf16", SPLIT, (128, 128), [(160, 160)], 192, **B),
    dw_case("dw_split_was_narrow_out_bf16", SPLIT, (128, 64), [(256, 256)], 4, **B),
    dw_case("dw_plain_was_narrow_in_bf16", PLAIN, (64, 64), [(3, 4)], 16, **B),
    dw_case("dw_split_two_samples_per_group_bf16", SPLIT, (128, 128), [(256, 256)] * 8, 512, shape=(16, 40), slabs=8, **B),
    dw_case("dw_generic_two_samples_per_group_bf16", GENERIC, (128, 128), [(70, 70)] * 8, 514, shape=(16, 40), slabs=8, lddz=514, **B),
    dw_case("dw_plain_two_samples_per_group_bf16", PLAIN, (128, 128), [(68, 68)] * 8, 515, shape=(16, 40), slabs=8, **B),
    dw_case("dw_packed_two_samples_per_group_bf16", PACKED, (128, 32), [S32, S32], 31, shape=(1024, 3), slabs=512, **B),
    dw_case("dw_generic_dz2_bf16", GENERIC, (64, 64), [(5, 5), (5, 5)], 8, dz2=True, **B),
    dw_case("dw_plain_dz2_bf16", PLAIN, (64, 64), [(3, 4), (3, 4)], 10, dz2=True, **B),
    dw_case("dw_split_dz2_accumulate_bf16", SPLIT, (64, 64), [S64, S64], 64, dz2=True, accumulate=True, **B),
    dw_case("dw_generic_nan_view_bf16", GENERIC, (128, 128), [(70, 81)], 130, lead=3, lddz=141, **B),
    dw_case("dw_plain_nan_view_bf16", PLAIN, (64, 128), [(6, 24)], 67, lead=8, lddz=88, **B),
    dw_case("dw_packed_nan_view_bf16", PACKED, (128, 32), [(32, 48), (32, 48)], 31, lead=8, lddz=48, **B),
    dw_case("dw_split_nan_view_bf16", SPLIT, (128, 128), [(160, 176)], 192, lead=8, lddz=208, **B),
    dw_case("dw_reduce_vec_bf16", SPLIT, (128, 128), [(512, 512)], 512, shape=(2, 300), aligned=True, accumulate=True, **B),
]
ALL_DW_CASES = DW_CASES + DW_BF16_CASES


def dw_plan_tuple(case):
    return ("dw", case["kid"]) + case["tile"] + (("bf16",) if case["storage"] == "bf16" else ())


def dw_operands(case):
    N, Mo, F = case["N"], case["Mo"], case["F"]
    rng = rng_of(case["name"])
    op = {}
    sc = 2.0 ** (-rng.integers(0, 6, (N, Mo, 1))).astype(np.float64)                # per-row scales over 6 binades
    op["dz"] = (rng.standard_normal((N, Mo, F)) * sc).astype(np.float32)
    op["dz2"] = (rng.standard_normal((N, Mo, F)) * sc[:, ::-1] * 0.5).astype(np.float32) if case["dz2"] else None
    op["xs"] = [(rng.standard_normal((N, Mo, c)) * sc[::-1]).astype(np.float32) for c, _ in case["srcs"]]
    if case["storage"] == "bf16":
        op["dz"], op["xs"] = bf16_round(op["dz"]), [bf16_round(x) for x in op["xs"]]
        op["dz2"] = bf16_round(op["dz2"]) if case["dz2"] else None
    op["g0"] = None
    if case["accumulate"]:
        # a gradient already in the blocks, of the size of what is added to it
        rms = float(np.sqrt(((sc * sc[::-1]) ** 2).sum()))
        op["g0"] = [(rng.standard_normal((c, F)) * rms).astype(np.float32) for c, _ in case["srcs"]]
    return op


def dw_compute(case, op, dtype=np.float64, rows=None):
    """Per source the gradient block in ``dtype``.  ``rows``: a boolean [Mo] mask of the rows that take part (host corruptions)."""
    out = []
    last = len(op["xs"]) - 1
    for i, x in enumerate(op["xs"]):
        z = op["dz2"] if case["dz2"] and i == last else op["dz"]
        if rows is not None:
            x, z = x[:, rows], z[:, rows]
        w = x.reshape(-1, x.shape[2]).astype(dtype).T @ z.reshape(-1, z.shape[2]).astype(dtype)
        if case["accumulate"]:
            w = w + op["g0"][i].astype(dtype)
        out.append(w)
    return out


def judge_dw(case, want, f32, got):
    worst = 0.0
    for i, (g, w, r) in enumerate(zip(got, want, f32)):
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == w.shape and np.isfinite(g).all(), case["name"]
        err = float(np.abs(g - w).max() / np.abs(w).max())
        e32 = float(np.abs(np.asarray(r, np.float64) - w).max() / np.abs(w).max())
        parity_bar.check("contractions[%s]" % case["name"], "dW_%d" % i, err, e32, also_below=kernel_bars.TOL)
        worst = max(worst, err)
    return worst


def dw_blocks(case):
    """(offset, C) of every gradient block in the bucket, and the bucket's size: odd offsets unless the case wants 16 bytes."""
    blocks, off = [], 8 if case["aligned"] else 7
    for k, (c, _) in enumerate(case["srcs"]):
        blocks.append((off, c))
        off += c * case["F"] + (5 if k % 2 == 0 else 8)
        if case["aligned"]:
            off = _padq(off)
    return blocks, off + 3


def run_dw(case):
    import torch
    from cape_amd import ops
    N, Mo, F = case["N"], case["Mo"], case["F"]
    op = dw_operands(case)
    dtype = torch.bfloat16 if case["storage"] == "bf16" else torch.float32
    hdz = _dev_operand(op["dz"], case["lddz"], case["lead"], dtype)
    hdz2 = _dev_operand(op["dz2"], case["lddz"], case["lead"], dtype) if case["dz2"] else None
    blocks, size = dw_blocks(case)
    bucket = torch.full((size,), DW_SENTINEL, device=DEV, dtype=torch.float32)
    ent = []
    for i, ((c, ld), x, (off, _)) in enumerate(zip(case["srcs"], op["xs"], blocks)):
        if case["accumulate"]:
            bucket[off:off + c * F] = torch.tensor(op["g0"][i].ravel(), device=DEV)
        ent.append(dict(x=_dev_operand(x, ld, case["lead"], dtype), w=(bucket, off, F, 1), use_dz2=case["dz2"] and i == len(blocks) - 1))
    if case["aligned"]:
        assert all((bucket.data_ptr() + 4 * off) % 16 == 0 for off, _ in blocks)
    # the slab count is not part of ops.PLAN_LOG: the same query, made here
    plan = (C.c_int32 * 4)()
    p, ss, ld = ops._v(hdz)
    mask = (1 << (len(ent) - 1)) if case["dz2"] else 0
    ops.check(ops._fn("cape_gconv_dw_plan", hdz)(ops._mk_srcs(ent), len(ent), p, ss, ld, ops._v(hdz2)[0] if case["dz2"] else None, mask,
                                                 N, Mo, F, plan), "cape_gconv_dw_plan")
    keep = ops.DEFERRED, ops.PLAN_LOG
    ops.DEFERRED, ops.PLAN_LOG = None, set()
    try:
        ops.gconv_dw(ent, hdz, accumulate=case["accumulate"], dz2=hdz2)
        torch.cuda.synchronize()
        plans = set(ops.PLAN_LOG)
    finally:
        ops.DEFERRED, ops.PLAN_LOG = keep
    assert plans == {dw_plan_tuple(case)} and list(plan)[:3] == [case["kid"]] + list(case["tile"]), (case["name"], plans, list(plan))
    if case["slabs"] is not None:
        assert plan[3] == case["slabs"], (case["name"], list(plan))
    b = bucket.cpu().numpy()
    inside = np.zeros(size, bool)
    got = []
    for off, c in blocks:
        inside[off:off + c * F] = True
        got.append(b[off:off + c * F].reshape(c, F))
    worst = judge_dw(case, dw_compute(case, op), dw_compute(case, op, np.float32), got)
    out = b[~inside]
    assert np.array_equal(out.view(np.int32), np.full_like(out, DW_SENTINEL).view(np.int32)), "%s: the bucket was written outside its blocks" % case["name"]
    return report(case["name"], case["tile"], worst, "dw")


def plan_dw_host(case):
    """The case's launch put to cape_gconv_dw_plan / _bf16 with placeholder pointers (tools/record_dw_plans.py make_case)."""
    import record_dw_plans as R
    _lib, lib = R._load()
    es = 2 if case["storage"] == "bf16" else 4
    srcs, dz, dzs, dz2, mask, h2, keep = R.make_case(_lib, case["storage"], 0, 1 if case["dz2"] else 0, es * case["lead"], case["srcs"],
                                                     case["F"], case["lddz"], case["N"], case["Mo"])
    rc, plan = R.plan_of(lib, case["storage"], srcs, len(case["srcs"]), dz, dzs, case["lddz"], dz2, mask, case["N"], case["Mo"], case["F"], None)
    assert rc == 0, (case["name"], rc)
    return plan


# --------------------------------------------------------------------------------------------------------------------------
# host plan queries
# --------------------------------------------------------------------------------------------------------------------------
def all_cases():
    return FWD_CASES + ALL_DW_CASES


def host_plans():
    """name -> plan of every case, as the library reports it under the environment of this process."""
    return {c["name"]: (plan_fwd_host(c) if c["kind"] == "fwd" else plan_dw_host(c)) for c in all_cases()}


def expected_host_plan(case):
    """The leading plan entries the case names (forward: family, BM, BN, layout; dW: kernel id, ct, ft[, slabs])."""
    if case["kind"] == "fwd":
        return list(fwd_plan_tuple(case)[1:5])
    return [case["kid"]] + list(case["tile"]) + ([case["slabs"]] if case["slabs"] is not None else [])


def main(argv):
    if argv == ["--plans"]:
        print(json.dumps(host_plans()))
        return 0
    sys.stderr.write("usage: python -m tests.contraction_cases --plans\n")
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
