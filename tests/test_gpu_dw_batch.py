"""Weight gradients per phase (cape_gconv_dw_batch): the deferred contractions of several launches of dw_h2_kernel<128, 128, true> run
at the flush as ONE grid, every item cut exactly as its own launch cuts it.  Four items in one batch, on synthetic operands with
their row bounds attached:

    A  N = 2, Mo = 431 (no multiple of the 32-row chunk), sources C = [128, 128], F = 128
    B  N = 2, Mo = 862, source C = [128], F = 256, contracted against dz AND (a second entry, the use_dz2 mask) against dz2
    C  N = 2, Mo = 431, C = [128], F = 128, accumulate = 1 onto a non-zero block
    D  N = 2, Mo = 431, C = [160], F = 192: partial 128-tiles on both axes

The gradient blocks are views of one flat bucket pre-filled with a sentinel.  Every block is held to the project's bar
(tests/parity_bar.py: error against a float64 einsum <= 4 x that of the float32 restatement), on the batched path and on the
per-layer path (CAPE_DW_BATCH=0) alike; the batched path writes the same partial slabs, so the two buckets are also equal bit for
bit.  The bucket outside the blocks keeps the sentinel, two runs agree bit for bit, and an operand written in place between
queueing and flush is refused."""
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

# name: (N, Mo, F, [(C, use_dz2)], accumulate)
ITEMS = [("A", 2, 431, 128, [(128, False), (128, False)], False),
         ("B", 2, 862, 256, [(128, False), (128, True)], False),
         ("C", 2, 431, 128, [(128, False)], True),
         ("D", 2, 431, 192, [(160, False)], False)]


def _act(a):
    from cape_amd import ops
    t = ops.alloc_act(a.shape[0], a.shape[1], a.shape[2], torch.device(DEV))
    t.copy_(torch.tensor(a, dtype=torch.float32))
    ops.rowmax(t)
    return t


def _mat_err(a, ref):
    return np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max()


@pytest.fixture(scope="module")
def case():
    """Host operands, the bucket layout, and per block the float64 result and its float32 restatement (computed once)."""
    rng = np.random.default_rng(20240611)
    items, blocks, off = [], [], 7                       # (odd gaps: the blocks start at every alignment)
    for name, N, Mo, F, srcs, acc in ITEMS:
        sc = 2.0 ** (-rng.integers(0, 6, (N, Mo, 1))).astype(np.float64)
        dz = (rng.standard_normal((N, Mo, F)) * sc).astype(np.float32)
        dz2 = (rng.standard_normal((N, Mo, F)) * sc[:, ::-1]).astype(np.float32) if any(u for _, u in srcs) else None
        x = (rng.standard_normal((N, Mo, srcs[0][0])) * sc[::-1]).astype(np.float32)      # (B: one source, two entries)
        xs = [x if i == 0 or name == "B" else (rng.standard_normal((N, Mo, c)) * sc).astype(np.float32) for i, (c, _) in enumerate(srcs)]
        ent = []
        for (c, use2), xh in zip(srcs, xs):
            g = dz2 if use2 else dz
            prior = (rng.standard_normal((c, F)) * 3.0).astype(np.float32) if acc else None
            w64 = np.einsum('nrc,nrf->cf', xh.astype(np.float64), g.astype(np.float64))
            w32 = xh.reshape(-1, c).T @ g.reshape(-1, F)                                     # float32 throughout
            if acc:
                w64, w32 = w64 + prior.astype(np.float64), (w32 + prior).astype(np.float32)
            ent.append(dict(x=xh, use2=use2, block=len(blocks)))
            blocks.append(dict(item=name, off=off, C=c, F=F, prior=prior, w64=w64, w32=w32))
            off += c * F + (5 if len(blocks) % 2 else 8)
        items.append(dict(name=name, dz=dz, dz2=dz2, ent=ent, acc=acc))
    return dict(items=items, blocks=blocks, size=off + 3)


def _run(case, batch):
    """Queue the four items as the backward sweep does and flush; returns (bucket on the host, how many were batched)."""
    from cape_amd import ops
    bucket = torch.full((case["size"],), SENTINEL, device=DEV, dtype=torch.float32)
    for b in case["blocks"]:
        if b["prior"] is not None:
            bucket[b["off"]:b["off"] + b["C"] * b["F"]] = torch.tensor(b["prior"]).reshape(-1)
    keep_batch, keep_def = ops.DW_BATCH, ops.DEFERRED
    ops.DW_BATCH, ops.DEFERRED = batch, []
    try:
        for it in case["items"]:
            hdz = _act(it["dz"])
            hdz2 = _act(it["dz2"]) if it["dz2"] is not None else None
            hx = {}
            ent = []
            for e in it["ent"]:
                t = hx.setdefault(id(e["x"]), None)
                if t is None:
                    t = hx[id(e["x"])] = _act(e["x"])
                b = case["blocks"][e["block"]]
                ent.append(dict(x=t, w=(bucket, b["off"], b["F"], 1), use_dz2=e["use2"]))
            ops.gconv_dw(ent, hdz, accumulate=it["acc"], dz2=hdz2, defer=True)
        nbatched = sum(1 for q in ops.DEFERRED_DW if q[5])
        assert len(ops.DEFERRED_DW) == len(case["items"])
        ops.flush_deferred()
        torch.cuda.synchronize()
    finally:
        ops.DW_BATCH, ops.DEFERRED = keep_batch, keep_def
        ops.DEFERRED_DW[:] = []
    return bucket.cpu().numpy(), nbatched


def _check_bucket(case, got, tag):
    inside = np.zeros(case["size"], bool)
    for i, b in enumerate(case["blocks"]):
        sl = slice(b["off"], b["off"] + b["C"] * b["F"])
        inside[sl] = True
        w = got[sl].reshape(b["C"], b["F"])
        assert np.isfinite(w).all(), (tag, b["item"], i)
        e_hip, e_f32 = _mat_err(w, b["w64"]), _mat_err(b["w32"], b["w64"])
        print("%s block %d (item %s, %d x %d): err %.3e, float32 restatement %.3e" % (tag, i, b["item"], b["C"], b["F"], e_hip, e_f32))
        parity_bar.check("test_gpu_dw_batch[%s]" % tag, "dW_%s_%d" % (b["item"], i), e_hip, e_f32)
    assert np.array_equal(got[~inside].view(np.int32), np.full((~inside).sum(), SENTINEL, np.float32).view(np.int32)), tag


def test_batched_contractions_against_float64(case):
    got, nbatched = _run(case, 1)
    assert nbatched == len(ITEMS)                         # every item is one the batch takes (D's partial tiles included)
    _check_bucket(case, got, "batch")
    again, _ = _run(case, 1)
    assert np.array_equal(got.view(np.int32), again.view(np.int32))      # fixed summation order: bit for bit


def test_batch_equals_the_per_layer_launches_bit_for_bit(case):
    """One grid, but every item cut exactly as its own launch cuts it -- the same slabs, the same scales, the same reduction."""
    got, nbatched = _run(case, 1)
    ref, n0 = _run(case, 0)
    assert nbatched == len(ITEMS) and n0 == 0
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))


def test_per_layer_path_is_held_to_the_same_bar(case):
    got, nbatched = _run(case, 0)
    assert nbatched == 0
    _check_bucket(case, got, "per_layer")


def test_operand_written_between_queue_and_flush_is_refused(case):
    from cape_amd import ops
    it = case["items"][0]
    for victim in ("dz", "x"):
        keep = ops.DEFERRED
        ops.DEFERRED = []
        try:
            hdz = _act(it["dz"])
            hx = _act(it["ent"][0]["x"])
            dW = torch.zeros((128, 128), device=DEV)
            ops.gconv_dw([dict(x=hx, w=(dW, 0, 128, 1))], hdz, defer=True)
            assert ops.DEFERRED_DW[-1][5]
            (hdz if victim == "dz" else hx).add_(1)
            with pytest.raises(RuntimeError, match="written in place"):
                ops.flush_deferred()
            assert not ops.DEFERRED_DW
        finally:
            ops.DEFERRED = keep
            ops.DEFERRED_DW[:] = []
        torch.cuda.synchronize()
