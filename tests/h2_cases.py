"""Cases, operand builders, float64 references and judges of the direct tests of the fp16 two-piece contractions
(cape_amd/csrc/gemm_h2.h, gemm_h2x.h).  TEST INFRASTRUCTURE ONLY -- not collected by pytest.

    tests/test_gpu_h2_tiles.py          runs every case on the device (run_fwd / run_bwd / run_chain / run_dw) and the knob legs
    tests/test_h2_tile_cases_host.py    pins every case's kernel plan without a GPU and feeds the judges corrupted results
    python -m tests.h2_cases LEG        the cases of one knob leg (LEG_ENV) in a process that was started with the leg's knobs:
                                        one line per case (name, tile, worst figure), non-zero exit on the first failure
    python -m tests.h2_cases --plans    the host plan of every default-leg case as one JSON line

A case is a dict; every run_* asserts the EXACT plan tuple the library reports (ops.PLAN_LOG) before it judges the result, and
every judge takes the device result as a plain numpy array.  Inputs are seeded by the case's name.  With CAPE_H2_MARGINS=<file>
every judged case appends its line to that file (profiles/r07_h2_tile_margins.txt).

Bars (none is new):
  row      plain / ReLU / leaky without an additive term, all data gradients: tests/test_gpu_h2.py's 2e-6 of EVERY row's own
           norm against float64; rows whose reference is exactly zero must come back exactly zero and are at most 1 % of the rows.
  tensor   an additive term that does not scale with the row (channel / vertex bias, rank-1 terms): 2e-6 of the tensor's largest
           row norm; the rows are drawn from 8 binades and the 6e4 row is left out, so that the largest row norm stays within
           2^8 of the typical one and an error on an ordinary row remains visible.
  element  tanh, and the launch the two-piece kernel declines: kernel_bars.element_bar (factor 4 on the float32 restatement of
           the same op order, backstop 2e-5).
  dw       per source max|got - want| / max|want| < 2e-6 (test_dw_h2).
  mask     bit == (v > 0) for v = accumulator 1 + its rank-1 terms, wherever |v| > 1e-4 max|v| -- and ALSO wherever
           |v| > 1e-4 sum|terms of v|: the rows span 40 binades and the weight columns 12, so the tensor-wide maximum alone would
           leave most positions unjudged; the kernel's error at a position is <= ~2^-20 of the sum of its terms' absolute values
           (22-bit pieces, fp32 accumulation), two orders below that threshold.  Unjudged positions: at most 1 % (asserted on the
           reference).  Bits of columns >= F are zero.
"""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kernel_bars  # noqa: E402
from tests.test_h2_numerics import scale_of  # noqa: E402

DEV = "cuda:0"
BAR = 2e-6
SENTINEL = -12345.678
MASK_FILL = 0x5A5A5A5A
# environment of the knob legs (the library latches them at first use: one fresh process per leg)
LEG_ENV = {
    "h2x2": dict(CAPE_H2X="2"),
    "tile128": dict(CAPE_H2_TILE="128x128", CAPE_H2X="0"),
    "tile64x128": dict(CAPE_H2_TILE="64x128", CAPE_H2X="0"),
}
# knobs that move a kernel plan (the host test queries the plans with these removed)
PLAN_KNOBS = ("CAPE_H2", "CAPE_GEMM_H2", "CAPE_DW_H2", "CAPE_H2X", "CAPE_H2_TILE", "CAPE_GEMM_PLAIN", "CAPE_DW_PLAIN", "CAPE_GEMM_BF16X6",
              "CAPE_GEMM_BF16X6_DUAL", "CAPE_DW_BF16X6", "CAPE_DW_V4", "CAPE_NARROW")


# --------------------------------------------------------------------------------------------------------------------------
# shared helpers (tests/test_gpu_h2.py imports these back)
# --------------------------------------------------------------------------------------------------------------------------
def _act(a):
    import torch
    from cape_amd import ops
    t = ops.alloc_act(a.shape[0], a.shape[1], a.shape[2], torch.device(DEV))
    t.copy_(torch.tensor(a, dtype=torch.float32))
    return t


def _row_scales(N, M, rng, binades=24, large_row=True):
    s = 2.0 ** (-rng.integers(0, binades, (N, M))).astype(np.float64)
    s[0, min(3, M - 1)] = 0.0
    s[0, min(5, M - 1)] = 1e-30
    if large_row:
        s[-1, min(7, M - 1)] = 6e4
    return s


def _per_row_err(got, want):
    """largest relative L2 error of a row judged on that row's own norm (rows that are exactly zero must be exactly zero)."""
    n = np.sqrt((want ** 2).sum(-1))
    e = np.sqrt(((got - want) ** 2).sum(-1))
    assert np.all(e[n == 0] == 0)
    return float((e[n > 0] / n[n > 0]).max())


def _tensor_err(got, want):
    """largest L2 error of a row on the tensor's largest row norm (the ``with_bias`` branch of tests/test_gpu_h2.py)."""
    return float(np.sqrt(((got - want) ** 2).sum(-1)).max() / np.sqrt((want ** 2).sum(-1)).max())


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def unpack_mask(words):
    """[N, Mo, nw] int32 / uint32 words -> [N, Mo, 32 nw] bits (bit b of word j = column 32 j + b)."""
    w = np.ascontiguousarray(words).view(np.uint32)
    return ((w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(w.shape[0], w.shape[1], -1).astype(bool)


def pack_mask(pos):
    """[N, Mo, F] booleans -> [N, Mo, ceil(F / 32)] uint32 words."""
    N, Mo, F = pos.shape
    nw = (F + 31) // 32
    b = np.zeros((N, Mo, nw * 32), dtype=np.uint64)
    b[:, :, :F] = pos
    return (b.reshape(N, Mo, nw, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def report(name, tile, worst, kind):
    line = "%-44s %-12s %s %.3e" % (name, "%dx%d" % tuple(tile) if tile else "-", kind, worst)
    print(line, flush=True)
    path = os.environ.get("CAPE_H2_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    return line


def judge_rm(rm, y, F):
    """The epilogue's row bounds: >= the true maximum of every 32-column block, <= the maximum over the block's aligned
    four-row group, zero beyond ceil(F / 32)."""
    N, Mo = y.shape[0], y.shape[1]
    nb = (F + 31) // 32
    a = np.abs(y)
    Mp = (Mo + 3) // 4 * 4
    for j in range(nb):
        blk = a[:, :, 32 * j:32 * j + 32].max(-1)
        assert np.all(rm[:, :, j] >= blk), j
        grp = np.zeros((N, Mp), dtype=blk.dtype)
        grp[:, :Mo] = blk
        grp = np.repeat(grp.reshape(N, Mp // 4, 4).max(-1), 4, axis=1)[:, :Mo]
        assert np.all(rm[:, :, j] <= grp), j
    assert np.all(rm[:, :, nb:] == 0)


def judge_mask(v, vscale, words, F):
    """``v``: float64 reference of what the sign is taken of, ``vscale``: sum of the absolute values of its terms."""
    bits = unpack_mask(words)
    assert not bits[:, :, F:].any(), "bits of columns >= F must be zero"
    a = np.abs(v)
    judged = (a > 1e-4 * a.max()) | (a > 1e-4 * vscale)
    skipped = 1.0 - judged.mean()
    assert skipped <= 0.01, skipped
    wrong = int((bits[:, :, :F][judged] != (v[judged] > 0)).sum())
    assert wrong == 0, "%d sign bits differ from the reference" % wrong
    return skipped


# --------------------------------------------------------------------------------------------------------------------------
# forward cases
# --------------------------------------------------------------------------------------------------------------------------
def fwd_case(name, shape, tile, dual=False, act=None, bias=None, rank=0, to2=0, leg="default", view=False):
    N, Mo, Ch, K, F = shape
    return dict(kind="fwd", name=name, N=N, Mo=Mo, Ch=Ch, K=K, F=F, tile=tile, dual=dual, act=act, bias=bias, rank=rank, to2=to2,
                leg=leg, view=view)


WIDE, T128, T64, D128 = (128, 256), (128, 128), (64, 64), (128, 64)
FWD_CASES = [
    # ---- wide 128 x 256: ten row tiles, the last of one row
    fwd_case("wide_8src_8chunks", (16, 1153, 32, 8, 200), WIDE),                        # eight one-chunk sources
    fwd_case("wide_3src_9chunks_F264", (8, 1153, 96, 3, 264), WIDE),                    # source changes at 3 and 6; column tile of 8
    fwd_case("wide_2src_10chunks", (16, 1153, 160, 2, 256), WIDE, act="leaky"),
    fwd_case("wide_1src_11chunks_F192", (16, 1153, 352, 1, 192), WIDE, act="relu"),
    fwd_case("wide_general_rank", (16, 1153, 128, 2, 200), WIDE, rank=2),
    fwd_case("wide_general_vbias_leaky", (16, 1153, 128, 2, 200), WIDE, bias="vertex", act="leaky"),
    fwd_case("wide_general_cbias_tanh", (16, 1153, 128, 2, 200), WIDE, bias="channel", act="tanh"),
    # ---- 128 x 128
    fwd_case("t128_16chunks", (16, 1409, 256, 2, 160), T128),
    fwd_case("t128_17chunks", (16, 1409, 544, 1, 136), T128, act="leaky"),
    # ---- 64 x 64 at every pipeline length
    fwd_case("t64_4chunks", (2, 203, 32, 4, 136), T64),
    fwd_case("t64_5chunks", (3, 203, 32, 5, 136), T64, act="leaky"),
    fwd_case("t64_6chunks", (2, 203, 96, 2, 136), T64),
    fwd_case("t64_7chunks", (2, 203, 32, 7, 136), T64, act="relu"),
    fwd_case("t64_9chunks_F72", (2, 203, 96, 3, 72), T64),
    fwd_case("t64_4chunks_rank", (2, 203, 32, 4, 136), T64, rank=2),
    fwd_case("t64_4chunks_vbias", (2, 203, 32, 4, 136), T64, bias="vertex"),
    # ---- DUAL 128 x 64 (second weight set on source 0 only)
    fwd_case("dual_has2_flips_at_3", (3, 257, 96, 3, 72), D128, dual=True),
    fwd_case("dual_has2_chunk0_only", (2, 131, 32, 8, 72), D128, dual=True),
    fwd_case("dual_rank_to_acc2", (3, 257, 96, 3, 72), D128, dual=True, rank=2, to2=2),
]
VIEW_CASES = [
    fwd_case("view_wide", (8, 1153, 96, 3, 264), WIDE, view=True),
    fwd_case("view_t64", (2, 203, 96, 2, 136), T64, view=True),
    fwd_case("view_dual", (3, 257, 96, 3, 72), D128, dual=True, view=True),
]
LEG_CASES = {
    "h2x2": [fwd_case("h2x2_4chunks", (1, 129, 32, 4, 200), WIDE, leg="h2x2"),
             fwd_case("h2x2_5chunks", (2, 129, 160, 1, 192), WIDE, leg="h2x2"),
             fwd_case("h2x2_6chunks", (1, 257, 96, 2, 264), WIDE, leg="h2x2"),
             fwd_case("h2x2_7chunks", (2, 129, 32, 7, 200), WIDE, leg="h2x2")],
    "tile128": [fwd_case("tile128_6chunks", (2, 203, 96, 2, 136), T128, leg="tile128"),
                fwd_case("tile128_9chunks_F72", (2, 203, 96, 3, 72), (128, 64), leg="tile128")],
    "tile64x128": [fwd_case("tile64x128_6chunks", (2, 203, 96, 2, 136), (64, 128), leg="tile64x128"),
                   fwd_case("tile64x128_6chunks_F264", (1, 257, 96, 2, 264), (64, 128), leg="tile64x128")],
}


def additive(case):
    return bool(case.get("bias")) or bool(case.get("rank"))


def fwd_bar_kind(case):
    return "element" if case.get("act") == "tanh" else "tensor" if additive(case) else "row"


def fwd_operands(case):
    N, Mo, Ch, K, F = (case[k] for k in ("N", "Mo", "Ch", "K", "F"))
    rng = rng_of(case["name"])
    op = {}
    op["W"] = (rng.standard_normal((Ch * K, F)) * 0.3 * 2.0 ** (-rng.integers(0, 12, (1, F)))).astype(np.float32)   # columns of different size
    op["Wa"] = (rng.standard_normal((Ch, F)) * 0.2).astype(np.float32) if case["dual"] else None
    add = additive(case)
    scales = _row_scales(N, Mo, rng, binades=8 if add else 24, large_row=not add)
    op["xs"] = [(rng.standard_normal((N, Mo, Ch)) * scales[:, :, None]).astype(np.float32) for _ in range(K)]
    op["bias"] = None
    if case["bias"] == "channel":
        op["bias"] = (rng.standard_normal(F) * 0.5).astype(np.float32)
    elif case["bias"] == "vertex":
        op["bias"] = (rng.standard_normal((Mo, F)) * 0.5).astype(np.float32)
    R = case["rank"]
    op["rowscale"] = rng.standard_normal((R, Mo)).astype(np.float32) if R else None
    op["coef"] = (rng.standard_normal((N, R, F)) * 0.3).astype(np.float32) if R else None
    return op


def fwd_compute(case, op, dtype=np.float64, acc_delta=None):
    """The operation in ``dtype``: matmuls summed in source order, then the epilogue.  Returns (y, v): v = what the DUAL form
    takes the ReLU sign of (None otherwise).  ``acc_delta`` is added to the accumulator (the host test's corruptions)."""
    K = case["K"]
    acc = None
    for k in range(K):
        t = op["xs"][k].astype(dtype) @ op["W"][k::K].astype(dtype)                  # rows c*K + k
        acc = t if acc is None else acc + t
    if acc_delta is not None:
        acc = acc + acc_delta.astype(dtype)
    v, add2 = acc, None
    for j in range(case["rank"]):
        t = op["rowscale"][j].astype(dtype)[None, :, None] * op["coef"][:, j].astype(dtype)[:, None, :]
        if case["dual"] and (case["to2"] >> j) & 1:
            add2 = t if add2 is None else add2 + t
        else:
            v = v + t
    if case["dual"]:
        y = np.maximum(v, 0) + op["xs"][0].astype(dtype) @ op["Wa"].astype(dtype)
        if add2 is not None:
            y = y + add2
        return y, v
    if op["bias"] is not None:
        v = v + (op["bias"].astype(dtype) if case["bias"] == "channel" else op["bias"].astype(dtype)[None])
    act = case["act"]
    y = np.where(v > 0, v, dtype(0.2) * v) if act == "leaky" else np.maximum(v, 0) if act == "relu" else np.tanh(v) if act == "tanh" else v
    return y, None


def fwd_reference(case, op):
    want, v = fwd_compute(case, op)
    ref = dict(want=want, v=v, f32=None, vscale=None)
    if fwd_bar_kind(case) == "element":
        ref["f32"] = fwd_compute(case, op, np.float32)[0]
    if case["dual"]:
        K = case["K"]
        s = sum(np.abs(op["xs"][k].astype(np.float64)) @ np.abs(op["W"][k::K].astype(np.float64)) for k in range(K))
        for j in range(case["rank"]):
            if not (case["to2"] >> j) & 1:
                s = s + np.abs(op["rowscale"][j].astype(np.float64)[None, :, None] * op["coef"][:, j].astype(np.float64)[:, None, :])
        ref["vscale"] = s
    return ref


def judge_fwd(case, ref, got, mask=None, kind=None):
    """``got``: the device result [N, Mo, F] as a numpy array, ``mask``: the DUAL form's sign words.  Returns the worst figure."""
    got = np.asarray(got, dtype=np.float64)
    want = ref["want"]
    assert got.shape == want.shape and np.isfinite(got).all(), case["name"]
    kind = kind or fwd_bar_kind(case)
    if kind == "row":
        n = np.sqrt((want ** 2).sum(-1))
        assert (n == 0).mean() <= 0.01, "more than 1 % exactly-zero rows"
        worst = _per_row_err(got, want)
        assert worst < BAR, (case["name"], worst)
    elif kind == "tensor":
        worst = _tensor_err(got, want)
        assert worst < BAR, (case["name"], worst)
    else:
        kernel_bars.element_bar("h2_cases", case["name"], got, ref["f32"], want)
        worst = kernel_bars.mat_err(got, want)
    if case.get("dual"):
        assert mask is not None
        judge_mask(ref["v"], ref["vscale"], mask, want.shape[2])
    return worst


def fwd_geometry(case):
    """What the plan query needs of the launch run_fwd makes: per source (C, ldx, w_rs, w_cs, piece pitch, second weight set,
    row-bound width)."""
    Ch, K, F = case["Ch"], case["K"], case["F"]
    ldx = Ch + 12 if case["view"] else Ch
    specs = [dict(C=Ch, ldx=ldx, w_rs=K * F, w_cs=1, pitch=Ch, w2=(F, 1, Ch) if case["dual"] and k == 0 else None, rmw=4) for k in range(K)]
    return specs, case["N"], case["Mo"], F


def _plan_of(log, what):
    return {p for p in log if p[0] == what}


def _nan_view(x, lead=4, tail=8):
    """``x`` [N, M, C] as the slice [:, :, lead:lead + C] of a buffer whose other columns hold NaN."""
    import torch
    buf = torch.full((x.shape[0], x.shape[1], x.shape[2] + lead + tail), float("nan"), device=DEV, dtype=torch.float32)
    v = buf[:, :, lead:lead + x.shape[2]]
    v.copy_(torch.as_tensor(x, dtype=torch.float32))
    return v


def _sentinel_out(N, Mo, F):
    import torch
    buf = torch.full((N, Mo, F + 8), SENTINEL, device=DEV, dtype=torch.float32)
    return buf, buf[:, :, 4:4 + F]


def _sentinel_intact(buf, F):
    b = buf.cpu().numpy()
    s = np.float32(SENTINEL)
    return kernel_bars.same_bits(np.ascontiguousarray(b[:, :, :4]), np.full_like(b[:, :, :4], s)) and \
        kernel_bars.same_bits(np.ascontiguousarray(b[:, :, 4 + F:]), np.full_like(b[:, :, 4 + F:], s))


def run_fwd(case):
    import torch
    from cape_amd import _lib, ops
    N, Mo, Ch, K, F, dual = (case[k] for k in ("N", "Mo", "Ch", "K", "F", "dual"))
    op = fwd_operands(case)
    dev = torch.device(DEV)
    hW = torch.tensor(op["W"], device=DEV)
    hWa = torch.tensor(op["Wa"], device=DEV) if dual else None
    P = ops.pieces_for(hW, Ch, K, pair=(hWa, 1) if dual else None)
    Pa = ops.pieces_for(hWa, Ch, 1, pair=(hW, K)) if dual else None
    entries = []
    for k in range(K):
        if case["view"]:
            hx = _nan_view(op["xs"][k])
            rm = ops.rowmax(_act(op["xs"][k]))                                  # bounds of a contiguous copy
        else:
            hx = _act(op["xs"][k])
            rm = ops.rowmax(hx)
        e = dict(x=hx, w=(hW, k * F, K * F, 1), p=P.fwd(k), rm=rm)
        if dual and k == 0:
            e["w2"], e["p2"] = (hWa, 0, F, 1), Pa.fwd(0)
        entries.append(e)
    ybuf = None
    if case["view"]:
        ybuf, y = _sentinel_out(N, Mo, F)
    else:
        y = ops.alloc_act(N, Mo, F, dev)
    rm_y = ops.alloc_rm(y)
    mask = torch.full((N, Mo, (F + 31) // 32), MASK_FILL, device=DEV, dtype=torch.int32) if dual else None
    bias = torch.tensor(op["bias"], device=DEV) if op["bias"] is not None else None
    rank = None
    if case["rank"]:
        rank = (torch.tensor(op["rowscale"], device=DEV), torch.tensor(op["coef"], device=DEV), case["to2"])
    ops.PLAN_LOG = set()
    try:
        ops.gconv_fwd(entries, y, bias=bias, bias_mode=_lib.BIAS_VERTEX if case["bias"] == "vertex" else _lib.BIAS_CHANNEL,
                      act=case["act"] or "none", mask=mask, rank=rank, wsi=ops._ptr(P.fsi), wsi2=ops._ptr(Pa.fsi) if dual else None,
                      rm_out=rm_y)
        plans = set(ops.PLAN_LOG)
    finally:
        ops.PLAN_LOG = None
    assert plans == {("fwd", 3, case["tile"][0], case["tile"][1], 1, int(dual))}, (case["name"], plans)
    y32 = y.cpu().numpy()
    worst = judge_fwd(case, fwd_reference(case, op), y32, mask.cpu().numpy() if dual else None)
    judge_rm(rm_y.cpu().numpy(), y32, F)
    if ybuf is not None:
        assert _sentinel_intact(ybuf, F), "columns outside the output view were written"
    return report(case["name"], case["tile"], worst, fwd_bar_kind(case))


# --------------------------------------------------------------------------------------------------------------------------
# data-gradient cases (contraction over the Fout columns)
# --------------------------------------------------------------------------------------------------------------------------
BWD_CASES = [
    # one launch for all orders, de-interleaving epilogue: 288 output columns = two column tiles, 11 chunks
    dict(kind="bwd", name="bwd_wide_deint_11chunks", N=8, Mo=1153, Ch=96, K=3, Fo=352, form="deint", aff=False, tile=WIDE),
    # one source per order + the affine term: three sources of 160 = 15 chunks
    dict(kind="bwd", name="bwd_wide_multi_affine_15chunks", N=16, Mo=1153, Ch=192, K=2, Fo=160, form="multi", aff=True, tile=WIDE),
]


def bwd_operands(case):
    N, Mo, Ch, K, Fo = (case[k] for k in ("N", "Mo", "Ch", "K", "Fo"))
    rng = rng_of(case["name"])
    op = {}
    op["W"] = (rng.standard_normal((Ch * K, Fo)) * 0.3 * 2.0 ** (-rng.integers(0, 10, (Ch, 1)).repeat(K, 0))).astype(np.float32)
    op["Wa"] = (rng.standard_normal((Ch, Fo)) * 0.2).astype(np.float32) if case["aff"] else None
    scales = _row_scales(N, Mo, rng)
    nt = 1 if case["form"] == "deint" else K + (1 if case["aff"] else 0)
    op["ts"] = [(rng.standard_normal((N, Mo, Fo)) * scales[:, :, None]).astype(np.float32) for _ in range(nt)]
    return op


def bwd_compute(case, op, dtype=np.float64):
    Ch, K = case["Ch"], case["K"]
    if case["form"] == "deint":
        full = op["ts"][0].astype(dtype) @ op["W"].astype(dtype).T                  # column j = c*K + k
        ChP = (Ch + 3) // 4 * 4
        want = np.zeros(full.shape[:2] + (K * ChP,), dtype=dtype)
        for k in range(K):
            want[:, :, k * ChP:k * ChP + Ch] = full[:, :, k::K]
        return want
    want = None
    for k in range(K):
        t = op["ts"][k].astype(dtype) @ op["W"][k::K].astype(dtype).T
        want = t if want is None else want + t
    if case["aff"]:
        want = want + op["ts"][K].astype(dtype) @ op["Wa"].astype(dtype).T
    return want


def judge_bwd(case, want, got):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), case["name"]
    n = np.sqrt((want ** 2).sum(-1))
    assert (n == 0).mean() <= 0.01
    worst = _per_row_err(got, want)
    assert worst < BAR, (case["name"], worst)
    return worst


def bwd_geometry(case):
    Ch, K, Fo = case["Ch"], case["K"], case["Fo"]
    if case["form"] == "deint":
        return [dict(C=Fo, ldx=Fo, w_rs=1, w_cs=Fo, pitch=Fo, w2=None, rmw=4)], case["N"], case["Mo"], K * Ch
    specs = [dict(C=Fo, ldx=Fo, w_rs=1, w_cs=K * Fo, pitch=K * Fo, w2=None, rmw=4) for _ in range(K)]
    if case["aff"]:
        specs.append(dict(C=Fo, ldx=Fo, w_rs=1, w_cs=Fo, pitch=Fo, w2=None, rmw=4))
    return specs, case["N"], case["Mo"], Ch


def run_bwd(case):
    import torch
    from cape_amd import ops
    N, Mo, Ch, K, Fo, aff = (case[k] for k in ("N", "Mo", "Ch", "K", "Fo", "aff"))
    op = bwd_operands(case)
    dev = torch.device(DEV)
    hW = torch.tensor(op["W"], device=DEV)
    hWa = torch.tensor(op["Wa"], device=DEV) if aff else None
    P = ops.pieces_for(hW, Ch, K, pair=(hWa, 1) if aff else None)
    Pa = ops.pieces_for(hWa, Ch, 1, pair=(hW, K)) if aff else None
    hT = [_act(t) for t in op["ts"]]
    ops.PLAN_LOG = set()
    try:
        if case["form"] == "deint":
            ChP = (Ch + 3) // 4 * 4
            out = ops.alloc_act(N, Mo, K * ChP, dev, zero=True)
            ops.gconv_fwd([dict(x=hT[0], w=(hW, 0, 1, Fo), p=(P.b_hi.data_ptr(), P.b_lo.data_ptr(), Fo), rm=ops.rowmax(hT[0]))], out,
                          deinterleave=K, F=K * Ch, wsi=ops._ptr(P.bsi))
        else:
            ent = [dict(x=hT[k], w=(hW, k * Fo, 1, K * Fo), p=P.bwd(k), rm=ops.rowmax(hT[k])) for k in range(K)]
            if aff:
                ent.append(dict(x=hT[K], w=(hWa, 0, 1, Fo), p=Pa.bwd(0), rm=ops.rowmax(hT[K])))
                assert torch.equal(P.bsc, Pa.bsc)                                # the paired tensors share their channel scales
            out = ops.alloc_act(N, Mo, Ch, dev)
            ops.gconv_fwd(ent, out, wsi=ops._ptr(P.bsc))
        plans = set(ops.PLAN_LOG)
    finally:
        ops.PLAN_LOG = None
    assert plans == {("fwd", 3, case["tile"][0], case["tile"][1], 1, 0)}, (case["name"], plans)
    worst = judge_bwd(case, bwd_compute(case, op), out.cpu().numpy())
    return report(case["name"], case["tile"], worst, "row")


# --------------------------------------------------------------------------------------------------------------------------
# row-bound chain: a producing epilogue writes bounds of width 8 / 12 / 16 / 20, the consumer reads them
# --------------------------------------------------------------------------------------------------------------------------
CHAIN_N, CHAIN_MO, CHAIN_K, CHAIN_F = 2, 203, 2, 136
CHAIN_CASES = [dict(kind="chain", name="chain_w%d" % w, FA=FA, prod="h2", Ch=64, width=w, consume=True)
               for FA, w in ((160, 8), (288, 12), (416, 16), (544, 20))]
CHAIN_CASES += [dict(kind="chain", name="chain_producer_family%d" % f, FA=160, prod="fam%d" % f, Ch=48 if f == 1 else 64, width=8,
                     consume=False) for f in (0, 1, 2)]


def chain_operands(case):
    N, Mo, K, FA, Ch = CHAIN_N, CHAIN_MO, CHAIN_K, case["FA"], case["Ch"]
    rng = rng_of(case["name"])
    op = {}
    WA = rng.standard_normal((Ch * K, FA)) * 0.3
    WA[:, (FA - 1) // 32 * 32:] *= 64.0                     # the LAST 32-column block is 2^6 larger: its bound entry must be read
    op["WA"] = WA.astype(np.float32)
    g = 2.0 ** (-rng.integers(0, 12, (N, (Mo + 3) // 4))).astype(np.float64)      # constant within aligned groups of four rows
    scales = np.repeat(g, 4, axis=1)[:, :Mo]
    op["xs"] = [(rng.standard_normal((N, Mo, Ch)) * scales[:, :, None]).astype(np.float32) for _ in range(K)]
    op["Wc"] = (rng.standard_normal((FA, CHAIN_F)) * 0.3 * 2.0 ** (-rng.integers(0, 12, (1, CHAIN_F)))).astype(np.float32)
    return op


def chain_producer(case, op, dtype=np.float64):
    K = CHAIN_K
    acc = None
    for k in range(K):
        t = op["xs"][k].astype(dtype) @ op["WA"][k::K].astype(dtype)
        acc = t if acc is None else acc + t
    return acc


def chain_geometry(case, stage):
    """stage 'producer' (h2 producers only) or 'consumer'."""
    FA, Ch, K = case["FA"], case["Ch"], CHAIN_K
    if stage == "producer":
        return [dict(C=Ch, ldx=Ch, w_rs=K * FA, w_cs=1, pitch=Ch, w2=None, rmw=4) for _ in range(K)], CHAIN_N, CHAIN_MO, FA
    return [dict(C=FA, ldx=FA, w_rs=CHAIN_F, w_cs=1, pitch=FA, w2=None, rmw=case["width"])], CHAIN_N, CHAIN_MO, CHAIN_F


def judge_chain_consumer(case, want, f32, got):
    """Widths up to 16 run on the two-piece kernel (row bar); width 20 is declined and held to element_bar."""
    fake = dict(name=case["name"], dual=False)
    return judge_fwd(fake, dict(want=want, f32=f32), got, kind="row" if case["width"] <= 16 else "element")


def run_chain(case):
    import torch
    from cape_amd import ops
    N, Mo, K, FA, Ch = CHAIN_N, CHAIN_MO, CHAIN_K, case["FA"], case["Ch"]
    op = chain_operands(case)
    dev = torch.device(DEV)
    hWA = torch.tensor(op["WA"], device=DEV)
    prod = case["prod"]
    PA = ops.pieces_for(hWA, Ch, K) if prod == "h2" else None
    entries = []
    for k in range(K):
        if prod == "fam0":
            # a source view whose base is not 16-byte aligned: the generic staging kernel
            buf = torch.zeros((N, Mo, Ch + 4), device=DEV, dtype=torch.float32)
            hx = buf[:, :, 1:1 + Ch]
            hx.copy_(torch.tensor(op["xs"][k]))
        else:
            hx = _act(op["xs"][k])
        e = dict(x=hx, w=(hWA, k * FA, K * FA, 1))
        if prod == "h2":
            e["p"], e["rm"] = PA.fwd(k), ops.rowmax(hx)
        entries.append(e)
    yA = ops.alloc_act(N, Mo, FA, dev)
    rmA = ops.alloc_rm(yA)
    assert rmA.shape[2] == case["width"]
    ops.PLAN_LOG = set()
    try:
        ops.gconv_fwd(entries, yA, wsi=ops._ptr(PA.fsi) if prod == "h2" else None, rm_out=rmA)
        plans = set(ops.PLAN_LOG)
    finally:
        ops.PLAN_LOG = None
    fam = {"h2": 3, "fam0": 0, "fam1": 1, "fam2": 2}[prod]
    assert {p[1] for p in plans} == {fam} and len(plans) == 1, (case["name"], plans)
    if prod == "h2":
        assert plans == {("fwd", 3, 64, 64, 1, 0)}, plans
    yA32 = yA.cpu().numpy()
    wantA = chain_producer(case, op)
    if prod == "h2":
        worst = judge_fwd(dict(name=case["name"] + "/producer", dual=False), dict(want=wantA), yA32, kind="row")
    else:
        assert np.isfinite(yA32).all()
        worst = kernel_bars.mat_err(yA32, wantA)
        assert worst < kernel_bars.TOL, worst
    judge_rm(rmA.cpu().numpy(), yA32, FA)
    tile = next(iter(plans))[2:4]
    lines = [report(case["name"] + "/producer", tile, worst, "row" if prod == "h2" else "matrix")]
    if not case["consume"]:
        return lines
    hWc = torch.tensor(op["Wc"], device=DEV)
    Pc = ops.pieces_for(hWc, FA, 1)
    y = ops.alloc_act(N, Mo, CHAIN_F, dev)
    ops.PLAN_LOG = set()
    try:
        ops.gconv_fwd([dict(x=yA, w=(hWc, 0, CHAIN_F, 1), p=Pc.fwd(0), rm=rmA)], y, wsi=ops._ptr(Pc.fsi))
        plans = set(ops.PLAN_LOG)
    finally:
        ops.PLAN_LOG = None
    assert len(plans) == 1, plans
    plan = next(iter(plans))
    if case["width"] <= 16:
        assert plan == ("fwd", 3, 64, 64, 1, 0), plan
    else:
        assert plan[1] != 3, plan                           # declined, not mis-run
    want = yA32.astype(np.float64) @ op["Wc"].astype(np.float64)                    # judged on the input it actually got
    f32 = yA32 @ op["Wc"]
    worst = judge_chain_consumer(case, want, f32, y.cpu().numpy())
    lines.append(report(case["name"] + "/consumer", plan[2:4], worst, "row" if case["width"] <= 16 else "element"))
    return lines


# --------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases
# --------------------------------------------------------------------------------------------------------------------------
def dw_case(name, N, Mo, Cs, F, tile, dz2_src=None, accumulate=False, view=False):
    return dict(kind="dw", name=name, N=N, Mo=Mo, Cs=Cs, F=F, tile=tile, dz2_src=dz2_src, accumulate=accumulate, view=view)


DW_CASES = [
    # (two 64-channel sources into 64 columns pack into ONE tile of the packed exact-fp32 kernel; three do not)
    dw_case("dw_64x64", 3, 333, [64, 64, 64], 64, (64, 64)),
    dw_case("dw_128x64_F40", 3, 333, [128], 40, (128, 64)),
    dw_case("dw_128x128_dz2", 2, 300, [128, 128], 128, (128, 128), dz2_src=1),
    dw_case("dw_128x128_dz2_accumulate", 2, 300, [128, 128], 128, (128, 128), dz2_src=1, accumulate=True),
] + [dw_case("dw_64x128_Mo%d" % Mo, 2, Mo, [64], 136, (64, 128)) for Mo in (1, 31, 33, 65)] + [
    dw_case("dw_128x128_nan_views", 3, 333, [96], 160, (128, 128), view=True),
]


def dw_operands(case):
    N, Mo, Cs, F = (case[k] for k in ("N", "Mo", "Cs", "F"))
    rng = rng_of(case["name"])
    op = {}
    # rows of very different size inside every workgroup's range: the slab-uniform scales must cope
    sc = 2.0 ** (-rng.integers(0, 12, (N, Mo, 1))).astype(np.float64)
    op["dz"] = (rng.standard_normal((N, Mo, F)) * sc).astype(np.float32)
    op["dz2"] = (rng.standard_normal((N, Mo, F)) * sc * 0.5).astype(np.float32) if case["dz2_src"] is not None else None
    op["xs"] = [(rng.standard_normal((N, Mo, C_)) * sc[::-1]).astype(np.float32) for C_ in Cs]
    op["g0"] = None
    if case["accumulate"]:
        # a gradient already in the buffers, of the size of what is added to it
        rms = float(np.sqrt(((sc * sc[::-1]) ** 2).sum()))
        op["g0"] = [(rng.standard_normal((C_, F)) * rms).astype(np.float32) for C_ in Cs]
    return op


def dw_compute(case, op, dtype=np.float64):
    out = []
    for i, x in enumerate(op["xs"]):
        z = op["dz2"] if case["dz2_src"] == i else op["dz"]
        w = x.reshape(-1, x.shape[2]).astype(dtype).T @ z.reshape(-1, z.shape[2]).astype(dtype)
        if op["g0"] is not None:
            w = w + op["g0"][i].astype(dtype)
        out.append(w)
    return out


def judge_dw(case, want, got):
    worst = 0.0
    for g, w in zip(got, want):
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == w.shape and np.isfinite(g).all(), case["name"]
        err = float(np.abs(g - w).max() / np.abs(w).max())
        assert err < BAR, (case["name"], err)
        worst = max(worst, err)
    return worst


def run_dw(case):
    import torch
    from cape_amd import ops
    N, Mo, Cs, F = (case[k] for k in ("N", "Mo", "Cs", "F"))
    op = dw_operands(case)

    def operand(a):
        if case["view"]:
            t = _nan_view(a)                                                    # channel offset 4, pitch a multiple of 4
            ops.set_rm(t, ops.rowmax(_act(a)))
        else:
            t = _act(a)
            ops.rowmax(t)
        return t

    hdz = operand(op["dz"])
    hdz2 = operand(op["dz2"]) if op["dz2"] is not None else None
    ent = []
    for i, x in enumerate(op["xs"]):
        dW = torch.tensor(op["g0"][i], device=DEV) if op["g0"] is not None else torch.zeros((x.shape[2], F), device=DEV)
        ent.append(dict(x=operand(x), w=(dW, 0, F, 1), use_dz2=case["dz2_src"] == i))
    ops.PLAN_LOG = set()
    try:
        ops.gconv_dw(ent, hdz, accumulate=case["accumulate"], dz2=hdz2)
        plans = set(ops.PLAN_LOG)
    finally:
        ops.PLAN_LOG = None
    assert plans == {("dw", 4, case["tile"][0], case["tile"][1])}, (case["name"], plans)
    worst = judge_dw(case, dw_compute(case, op), [e["w"][0].cpu().numpy() for e in ent])
    return report(case["name"], case["tile"], worst, "dw")


# --------------------------------------------------------------------------------------------------------------------------
# host plan queries (pure host logic: placeholder pointers, never dereferenced)
# --------------------------------------------------------------------------------------------------------------------------
def plan_fwd_host(geometry):
    from cape_amd import _lib
    specs, N, Mo, F = geometry
    n = len(specs)
    arr = (_lib.CapeSrc * n)()
    hs = (_lib.CapeH2Src * n)()
    dual = False
    for i, (s, h, g) in enumerate(zip(arr, hs, specs)):
        base = 0x10000000 * (i + 1)
        s.x, s.x_sample_stride, s.ldx, s.C = base + (16 if g["ldx"] != g["C"] else 0), Mo * g["ldx"], g["ldx"], g["C"]
        s.w, s.w_rs, s.w_cs = base + 0x4000000, g["w_rs"], g["w_cs"]
        s.w2, s.w2_rs, s.w2_cs = None, 0, 0
        h.w_hi, h.w_lo, h.w_pitch = base + 0x5000000, base + 0x6000000, g["pitch"]
        if g["w2"] is not None:
            dual = True
            s.w2, s.w2_rs, s.w2_cs = base + 0x7000000, g["w2"][0], g["w2"][1]
            h.w2_hi, h.w2_lo, h.w2_pitch = base + 0x8000000, base + 0x9000000, g["w2"][2]
        h.rowmax, h.rowmax_w = base + 0xA000000, g["rmw"]
    h2 = _lib.CapeH2()
    h2.src = C.addressof(hs)
    h2.wscale_inv = 0xA0000000
    h2.w2scale_inv = 0xB0000000 if dual else None
    out = (C.c_int32 * 4)()
    assert _lib.lib.cape_gconv_fwd_plan_h2(arr, n, N, Mo, F, C.byref(h2), out) == 0
    return list(out)


def plan_dw_host(case):
    from cape_amd import _lib
    N, Mo, Cs, F = (case[k] for k in ("N", "Mo", "Cs", "F"))
    pad = 12 if case["view"] else 0
    off = 16 if case["view"] else 0
    n = len(Cs)
    arr = (_lib.CapeSrc * n)()
    h2 = _lib.CapeH2Dw()
    for i, (s, Cn) in enumerate(zip(arr, Cs)):
        base = 0x10000000 * (i + 1)
        s.x, s.x_sample_stride, s.ldx, s.C = base + off, Mo * (Cn + pad), Cn + pad, Cn
        s.w, s.w_rs, s.w_cs = base + 0x4000000, F, 1
        s.w2, s.w2_rs, s.w2_cs = None, 0, 0
        h2.src_rowmax[i], h2.src_rowmax_w[i] = base + 0x8000000, 4
    h2.dz_rowmax, h2.dz_rowmax_w = 0xA0000000, 4
    dz2, mask = None, 0
    if case["dz2_src"] is not None:
        dz2, mask = C.c_void_p(0xC0000000 + off), 1 << case["dz2_src"]
        h2.dz2_rowmax, h2.dz2_rowmax_w = 0xD0000000, 4
    ldz = (F + 3) // 4 * 4 + pad
    out = (C.c_int32 * 4)()
    assert _lib.lib.cape_gconv_dw_plan_h2(arr, n, C.c_void_p(0xB0000000 + off), Mo * ldz, ldz, dz2, mask, N, Mo, F, C.byref(h2), out) == 0
    return list(out)


def host_plans():
    """name -> plan of every case of the default leg (forward, views, data gradient, chain, weight gradient)."""
    plans = {}
    for c in FWD_CASES + VIEW_CASES:
        plans[c["name"]] = plan_fwd_host(fwd_geometry(c))
    for c in BWD_CASES:
        plans[c["name"]] = plan_fwd_host(bwd_geometry(c))
    for c in CHAIN_CASES:
        if c["prod"] == "h2":
            plans[c["name"] + "/producer"] = plan_fwd_host(chain_geometry(c, "producer"))
        if c["consume"]:
            plans[c["name"] + "/consumer"] = plan_fwd_host(chain_geometry(c, "consumer"))
    for c in DW_CASES:
        plans[c["name"]] = plan_dw_host(c)
    return plans


def expected_host_plans():
    """What host_plans() must report under the default environment (None: any family but 3)."""
    want = {}
    for c in FWD_CASES + VIEW_CASES + BWD_CASES:
        want[c["name"]] = [3, c["tile"][0], c["tile"][1], 1]
    for c in CHAIN_CASES:
        if c["prod"] == "h2":
            want[c["name"] + "/producer"] = [3, 64, 64, 1]
        if c["consume"]:
            want[c["name"] + "/consumer"] = [3, 64, 64, 1] if c["width"] <= 16 else None
    for c in DW_CASES:
        want[c["name"]] = [4, c["tile"][0], c["tile"][1]]
    return want


RUNNERS = dict(fwd=run_fwd, bwd=run_bwd, chain=run_chain, dw=run_dw)


def main(argv):
    if len(argv) == 1 and argv[0] == "--plans":
        print(json.dumps(host_plans()))
        return 0
    if len(argv) != 1 or argv[0] not in LEG_CASES:
        sys.stderr.write("usage: python -m tests.h2_cases {%s} | --plans\n" % " | ".join(sorted(LEG_CASES)))
        return 2
    leg = argv[0]
    for k, v in LEG_ENV[leg].items():
        if os.environ.get(k) != v:
            sys.stderr.write("leg %s needs %s=%s in the environment of this process\n" % (leg, k, v))
            return 2
    for case in LEG_CASES[leg]:
        RUNNERS[case["kind"]](case)                          # an assertion ends the process with a traceback and status 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
