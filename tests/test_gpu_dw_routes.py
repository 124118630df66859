"""The three routes to a weight gradient agree bit for bit, for every kernel the dW host path can choose:

    now        ops.gconv_dw: contraction and slab reduction at once (cape_gconv_dw_stage*, stage 0)
    deferred   ops.gconv_dw(defer=True) in a deferred sweep, then flush_deferred(): contraction at once (stage 1), the reduction
               at the flush (cape_gconv_dw_reduce_batch); CAPE_DW_BATCH = 0
    batched    the same with CAPE_DW_BATCH at its default: a launch of dw_h2_kernel<128, 128, true> leaves its contraction to the
               flush as well (cape_gconv_dw_batch); every other launch is refused there and contracts at once

One case per kernel id and storage type, the smallest shapes that reach it: N = 2, Mo = 70 (no multiple of the 32-row chunk).
Each case first asserts through ops.PLAN_LOG that it reaches the kernel it is named for.  The gradient blocks are views of one
sentinel-filled bucket at odd offsets: the routes' buckets are equal bit for bit, sentinel included.  The "now" route of every
case is held to the project's bar against a float64 einsum (tests/parity_bar.py, as tests/test_gpu_dw_batch.py); the bf16 cases on
the bf16-rounded operands the device holds, whose products are exact in float32.  Every (storage, kernel, tile) form, the slab
splits and both reductions are judged in tests/test_gpu_contractions.py (tests/contraction_cases.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_bar                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25e33
N, MO = 2, 70

# name: (storage, kernel id, [(C, ld, use_dz2)], F, lddz, row bounds, batchable, (ct, ft))
CASES = {
    "generic": ("fp32", 0, [(5, 5, False)], 8, 8, False, False, (64, 64)),
    "plain": ("fp32", 1, [(3, 4, False)], 10, 12, False, False, (64, 64)),
    "packed": ("fp32", 2, [(32, 32, False), (32, 32, False)], 32, 32, False, False, (128, 32)),
    "split": ("fp32", 3, [(64, 64, False)], 64, 64, False, False, (64, 64)),
    "h2": ("fp32", 4, [(64, 64, False)], 64, 64, True, False, (64, 64)),
    "h2_v4": ("fp32", 4, [(128, 128, False)], 128, 128, True, True, (128, 128)),
    "h2_v4_dz2": ("fp32", 4, [(128, 128, False), (128, 128, True)], 128, 128, True, True, (128, 128)),
    "narrow_in": ("fp32", 5, [(3, 4, False)], 16, 16, False, False, (64, 64)),
    "narrow_out": ("fp32", 6, [(16, 16, False)], 3, 4, False, False, (64, 64)),
    "split_bf16": ("bf16", 3, [(64, 64, False)], 64, 64, False, False, (64, 64)),
    # (F = 31, not 32: bf16 storage tries the split kernel before it packs, and takes it for any even F -- with F = 32 the plan
    # query reports kernel 3.  31 is the nearest width that packs: the same 128 x 32 tile, lddz stays 32.)
    "packed_bf16": ("bf16", 2, [(32, 32, False), (32, 32, False)], 31, 32, False, False, (128, 32)),
    "plain_bf16": ("bf16", 1, [(3, 4, False)], 10, 12, False, False, (64, 64)),
    "generic_bf16": ("bf16", 0, [(5, 5, False)], 8, 8, False, False, (64, 64)),
}


def _dev(a, ld, dtype, bounds):
    """``a`` [N, Mo, C] on the device in rows of pitch ``ld``, with its row bounds attached when ``bounds``."""
    from cape_amd import ops
    buf = torch.zeros((a.shape[0], a.shape[1], ld), device=DEV, dtype=dtype)
    t = buf[:, :, :a.shape[2]] if ld != a.shape[2] else buf
    t.copy_(torch.tensor(a))
    if bounds:
        ops.rowmax(t)
    return t


def _bf16_round(a):
    return torch.tensor(a).to(torch.bfloat16).to(torch.float32).numpy()


def _mat_err(a, ref):
    return np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max()


@pytest.fixture(scope="module")
def data():
    """Per case: host operands (what the device holds, exactly), the bucket layout, per block the float64 result and its float32
    restatement.  Computed once and left unchanged."""
    out = {}
    for k, (name, (storage, kid, srcs, F, lddz, bounds, batchable, tile)) in enumerate(CASES.items()):
        rng = np.random.default_rng(20260000 + k)
        sc = 2.0 ** (-rng.integers(0, 6, (N, MO, 1))).astype(np.float64)
        dz = (rng.standard_normal((N, MO, F)) * sc).astype(np.float32)
        two = any(u for _, _, u in srcs)
        dz2 = (rng.standard_normal((N, MO, F)) * sc[:, ::-1]).astype(np.float32) if two else None
        x0 = (rng.standard_normal((N, MO, srcs[0][0])) * sc[::-1]).astype(np.float32)
        # (with dz2: ONE source, contracted against dz by the first entry and against dz2 by the second)
        xs = [x0 if i == 0 or two else (rng.standard_normal((N, MO, c)) * sc).astype(np.float32) for i, (c, _, _) in enumerate(srcs)]
        if storage == "bf16":
            dz, xs = _bf16_round(dz), [_bf16_round(x) for x in xs]
        blocks, off = [], 7
        for (c, ld, use2), xh in zip(srcs, xs):
            g = dz2 if use2 else dz
            w64 = np.einsum('nrc,nrf->cf', xh.astype(np.float64), g.astype(np.float64))
            w32 = xh.reshape(-1, c).T @ g.reshape(-1, F)
            blocks.append(dict(off=off, C=c, F=F, w64=w64, w32=w32))
            off += c * F + (5 if len(blocks) % 2 else 8)
        out[name] = dict(dz=dz, dz2=dz2, xs=xs, blocks=blocks, size=off + 3)
    return out


def _run(name, d, route):
    """One gradient through ``route``; returns (bucket on the host, the plan tuples logged, was the contraction deferred)."""
    from cape_amd import ops
    storage, kid, srcs, F, lddz, bounds, batchable, tile = CASES[name]
    dtype = torch.bfloat16 if storage == "bf16" else torch.float32
    bucket = torch.full((d["size"],), SENTINEL, device=DEV, dtype=torch.float32)
    hdz = _dev(d["dz"], lddz, dtype, bounds)
    hdz2 = _dev(d["dz2"], lddz, dtype, bounds) if d["dz2"] is not None else None
    hx, ent = {}, []
    for (c, ld, use2), xh, b in zip(srcs, d["xs"], d["blocks"]):
        if id(xh) not in hx:
            hx[id(xh)] = _dev(xh, ld, dtype, bounds)
        ent.append(dict(x=hx[id(xh)], w=(bucket, b["off"], F, 1), use_dz2=use2))
    keep = ops.DW_BATCH, ops.DEFERRED, ops.PLAN_LOG
    ops.PLAN_LOG = set()
    batched = False
    try:
        if route == "now":
            ops.DEFERRED = None
            ops.gconv_dw(ent, hdz, dz2=hdz2)
        else:
            ops.DW_BATCH, ops.DEFERRED = (1 if route == "batched" else 0), []
            ops.gconv_dw(ent, hdz, dz2=hdz2, defer=True)
            assert len(ops.DEFERRED_DW) == 1
            batched = bool(ops.DEFERRED_DW[0][5])
            ops.flush_deferred()
        torch.cuda.synchronize()
        log = set(ops.PLAN_LOG)
    finally:
        ops.DW_BATCH, ops.DEFERRED, ops.PLAN_LOG = keep
        ops.DEFERRED_DW[:] = []
    return bucket.cpu().numpy(), log, batched


@pytest.mark.parametrize("name", list(CASES))
def test_routes_write_the_same_bits(data, name):
    storage, kid, srcs, F, lddz, bounds, batchable, tile = CASES[name]
    d = data[name]
    want_plan = {("dw", kid) + tile + (("bf16",) if storage == "bf16" else ())}
    got = {}
    for route in ("now", "deferred", "batched"):
        got[route], log, batched = _run(name, d, route)
        assert log == want_plan, (name, route, log, want_plan)          # the kernel this case is named for
        assert batched == (route == "batched" and batchable), (name, route, batched)
    now = got["now"]
    inside = np.zeros(d["size"], bool)
    for i, b in enumerate(d["blocks"]):
        sl = slice(b["off"], b["off"] + b["C"] * b["F"])
        inside[sl] = True
        w = now[sl].reshape(b["C"], b["F"])
        assert np.isfinite(w).all(), (name, i)
        e_hip, e_f32 = _mat_err(w, b["w64"]), _mat_err(b["w32"], b["w64"])
        print("%s block %d (%d x %d): err %.3e, float32 restatement %.3e" % (name, i, b["C"], b["F"], e_hip, e_f32))
        parity_bar.check("test_gpu_dw_routes[%s]" % name, "dW_%d" % i, e_hip, e_f32)
    assert np.array_equal(now[~inside].view(np.int32), np.full((~inside).sum(), SENTINEL, np.float32).view(np.int32)), name
    for route in ("deferred", "batched"):
        assert np.array_equal(got[route].view(np.int32), now.view(np.int32)), (name, route)
