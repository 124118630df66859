"""The streaming sparse-operator kernels (csrc/sparse.hip: spmm_kernel, spmm_multi_kernel with its fused activation-gradient
epilogue, spmm_combine_kernel, bwd_prep_spmm_kernel, spmm_multi_prep_kernel and the gather helpers below them) on small synthetic
operators (tests/sparse_reference.py): every ELL width with empty rows and rows of exactly 4, 5, 8, 9 and 12 entries, operators
that must stay CSR, stored zeros, tail blocks, one and several blocks, both branches of the block mapping (N % 8), the chunked
(`rpb` 2 and 3) reductions with a wholly dead last group, 4- and 8-wide and scalar forms, fp32 and bf16 storage.

Every output is held to the float64 formula of include/cape_hip.h with tests/kernel_bars.py (element_bar: 4 x the float32
restatement, backstop 2e-5; sum_bar: 2e-6 of sum |terms|); whatever the headers call bit-identical (ELL against CSR, the fused
forms against the launches they replace, row bounds against the stored output) is compared bit for bit.  bf16 storage: per element
|dev - ref64| <= 2^-8 |ref64| + 4 x (max error of the float32 restatement) -- one bf16 rounding of the fp32 result.

The last test runs this module again in child processes under the kernel-selection knobs (CAPE_SPMM_WIDE / _ELL / _UNROLL)."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sparse_reference as R
from kernel_bars import element_bar, sum_bar, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = os.environ.get("CAPE_SPMM_WIDE") is None or int(os.environ["CAPE_SPMM_WIDE"]) != 0      # csrc/views.h spmm_wide()
SHAPES = [(37, 190), (300, 53), (37, 53), (300, 190)]            # (Mo, Mi): below one block of 256 work items / not a multiple
NS = [1, 3, 8, 16]                                               # 8, 16: the N % 8 == 0 branch of cape_map_block
F32, BF16 = torch.float32, torch.bfloat16
EINVAL, EWORKSPACE = -1, -4
WORST = dict(element=0.0, sum=0.0, bf16=0.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield torch.device("cuda:0")
    print("\ntest_gpu_sparse worst figures: element_bar ratio %.3f, sum_bar %.2e, bf16 bar share %.3f" % (WORST["element"], WORST["sum"], WORST["bf16"]))


def _ops():
    from cape_amd import ops
    return ops


_OPERATORS = {}


def operator(family, rows, cols, dev, seed=0):
    """(scipy matrix, DeviceCSR) of one synthetic operator; asserts the ELL width its family names."""
    from cape_amd.graph import HostCSR
    key = (family, rows, cols, seed)
    if key not in _OPERATORS:
        S = R.synth_operator(np.random.default_rng([rows, cols, seed, R.FAMILIES.index(family)]), rows, cols, family)
        csr = _ops().DeviceCSR(HostCSR(S), dev)
        assert csr.ell_w == R.expected_ell_w(family), (family, csr.ell_w)
        assert family != "ell4" or csr.max_row <= 4
        _OPERATORS[key] = (S, csr)
    return _OPERATORS[key]


def view(a, dev, dt=F32, off=0, pad=0, ld=None):
    """Device view [N, M, C] of ``a`` at channel offset ``off`` inside a zeroed buffer of row length ``ld``."""
    N, M, Cn = a.shape
    q = 4 if dt == F32 else 8
    ld = (Cn + off + pad + q - 1) // q * q if ld is None else ld
    buf = torch.zeros((N, M, ld), device=dev, dtype=dt)
    v = buf[:, :, off:off + Cn]
    v.copy_(torch.tensor(np.asarray(a), dtype=torch.float32).to(dt))
    return v


def n64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def n32(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def ell_mode(on):
    ops = _ops()
    saved = ops.SPMM_ELL
    ops.SPMM_ELL = on                    # read at call time (DeviceCSR.operands)
    try:
        yield
    finally:
        ops.SPMM_ELL = saved


def ebar(test, quantity, dev_, f32_, ref):
    r = element_bar(test, quantity, dev_, f32_, ref)
    WORST["element"] = max(WORST["element"], r)
    print("%s / %s: element_bar ratio %.3f" % (test, quantity, r))


def sbar(test, quantity, dev_, ref, abs_terms):
    WORST["sum"] = max(WORST["sum"], sum_bar(test, quantity, dev_, ref, abs_terms))


def bf16_bar(test, quantity, dev_, f32_, ref):
    """One bf16 rounding of an fp32 result that is inside the fp32 bar: bf16 keeps 8 significant bits, so round-to-nearest is off by
    at most half an ulp, which just above a power of two is 2^-8 of the value (the measured worst share of this bar is 0.995)."""
    dev_, f32_, ref = (np.asarray(v, np.float64) for v in (dev_, f32_, ref))
    assert dev_.shape == ref.shape and np.isfinite(dev_).all(), (test, quantity)
    tol = 2.0 ** -8 * np.abs(ref) + 4.0 * np.abs(f32_ - ref).max()
    err = np.abs(dev_ - ref)
    share = float((err / np.where(tol > 0, tol, 1.0)).max())
    WORST["bf16"] = max(WORST["bf16"], share)
    print("%s / %s: worst |err| / bf16 bar = %.3f" % (test, quantity, share))
    assert (err <= tol).all(), (test, quantity, share)


def check_rowbound(rm, y32, what):
    """[N, Mo, 4] row bounds: entry 0 = max |y| of the stored row exactly, entries 1..3 zero."""
    rm = n32(rm)
    assert same_bits(np.ascontiguousarray(rm[:, :, 0]), np.abs(y32).max(axis=2).astype(np.float32)), what
    assert np.all(rm[:, :, 1:] == 0), what


def spmm_rc(x, csr, y, alpha=1.0, z=None, beta=0.0, rm=None, operands=None):
    """cape_spmm[_bf16] called directly: returns the return code."""
    ops = _ops()
    xp, xs, xl = ops._v(x)
    yp, ys, yl = ops._v(y)
    zp, zs, zl = ops._v(z) if z is not None else (None, 0, 0)
    if operands is None:
        operands = csr.operands() if ops._vec_ok(x, y, z) else (csr.rowptr_t.data_ptr(), csr.colidx_t.data_ptr(), csr.vals_t.data_ptr(), 0)
    rp, ci, va, ew = operands
    N, _, Cn = x.shape
    return ops._fn("cape_spmm", x)(xp, xs, xl, C.c_void_p(rp), C.c_void_p(ci), C.c_void_p(va), int(csr.max_row), ew, float(alpha), zp, zs, zl,
                                   float(beta), yp, ys, yl, N, csr.shape[0], Cn, ops._ptr(rm), ops._stream())


def term_array(xs, csrs, ys=None, scales=None, rms=None):
    """cape_spmm_term_t array for direct calls (csrs[k] None = identity)."""
    from cape_amd import _lib
    ops = _ops()
    arr = (_lib.CapeSpmmTerm * len(xs))()
    for k, t in enumerate(arr):
        xp, t.x_sample_stride, t.ldx = ops._v(xs[k])
        t.x = xp.value
        t.scale = 1.0 if scales is None else float(scales[k])
        if csrs[k] is None:
            t.rowptr = t.colidx = t.vals = None
        else:
            t.rowptr, t.colidx, t.vals, t.ell_width = csrs[k].operands()
        if ys is not None:
            yp, t.y_sample_stride, t.ldy = ops._v(ys[k])
            t.y = yp.value
        if rms is not None and rms[k] is not None:
            t.rowmax_out = rms[k].data_ptr()
    return arr


# ---- cape_spmm ---------------------------------------------------------------------------------------------------------------
SPMM_C = [1, 3, 6, 4, 12, 36, 8, 24, 64, 264]      # scalar | 4-wide | 8-wide | cq = 33: the standalone row-bound pass


@pytest.mark.parametrize("Cn", SPMM_C)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_spmm(family, Cn, dev):
    ops = _ops()
    idx = R.FAMILIES.index(family) + SPMM_C.index(Cn)
    Mo, Mi = SHAPES[idx % 4]
    N = NS[(idx // 2) % 4] if Cn < 264 else 3
    S, csr = operator(family, Mo, Mi, dev)
    rng = np.random.default_rng(idx)
    x, z = R.inputs(rng, N, Mi, Cn), R.inputs(rng, N, Mo, Cn)
    alpha, beta = 1.3, -0.7
    g64, g32 = R.gather(S, x, np.float64), R.gather(S, x, np.float32)
    ref = dict(plain=(g64, g32), axpby=(R.spmm_from_gather(g64, alpha, z, beta, np.float64), R.spmm_from_gather(g32, alpha, z, beta, np.float32)))
    scalar = Cn % 4 != 0
    out = {}
    for ell in (1, 0):
        with ell_mode(ell):
            hx, hz = view(x, dev), view(z, dev)
            assert ops._vec_ok(hx) == (not scalar)
            if not scalar:
                assert csr.operands()[3] == (csr.ell_w if ell else 0)          # the leg the family names is the one that runs
            o = dict(plain=ops.spmm(hx, csr), axpby=ops.spmm(hx, csr, alpha=alpha, z=hz, beta=beta))
            if not scalar:
                xo = view(x, dev, off=4, pad=4)                                # a channel slice of a wider buffer: still a vector form
                assert ops._vec_ok(xo)
                o["slice4"] = ops.spmm(xo, csr)
            xo = view(x, dev, off=2, pad=2)                                    # offset 2: the scalar kernel, which reads CSR only --
            assert not ops._vec_ok(xo)                                         # the call succeeds, so no ELL operands were handed over
            o["slice2"] = ops.spmm(xo, csr)
            hy = view(z, dev)                                                  # in place: z aliases y
            assert ops.spmm(hx, csr, y=hy, alpha=alpha, z=hy, beta=beta) is hy
            o["inplace"] = hy
            rm = torch.full((N, Mo, 4), -1.0, device=dev)
            yb = ops.alloc_act(N, Mo, Cn, dev)
            assert spmm_rc(hx, csr, yb, alpha, hz, beta, rm) == 0
            torch.cuda.synchronize()
            check_rowbound(rm, n32(yb), (family, Cn, ell))
            o["bound"] = yb
            out[ell] = {k: n32(v) for k, v in o.items()}
    tag = "spmm[%s,C%d,N%d,Mo%d]" % (family, Cn, N, Mo)
    for k in out[1]:
        assert same_bits(out[1][k], out[0][k]), (tag, k, "ELL differs from CSR")
    o = out[1]
    for k in ("slice4", "slice2"):
        assert k not in o or same_bits(o[k], o["plain"]), (tag, k)
    assert same_bits(o["inplace"], o["axpby"]) and same_bits(o["bound"], o["axpby"]), tag
    ebar(tag, "S x", o["plain"], *ref["plain"][::-1])
    ebar(tag, "alpha S x + beta z", o["axpby"], *ref["axpby"][::-1])
    empty = R.degrees(S) == 0
    assert empty.any()
    assert same_bits(o["plain"][:, empty], np.zeros((N, int(empty.sum()), Cn), np.float32)), tag          # +0.0
    assert same_bits(o["axpby"][:, empty], (np.float32(beta) * z[:, empty].astype(np.float32)).astype(np.float32)), tag


# ---- cape_spmm_multi ---------------------------------------------------------------------------------------------------------
MULTI_LAYOUTS = [      # families (None = identity term), scales
    (["ell12"], [1.0]),
    ([None, "ell8"], [1.3, -0.7]),
    (["ell8", "csr", None], [1.0, 2.5, 0.3]),                  # an ELL and a CSR operator in one launch
    ([None, "ell4", "zeros_inside", None], [0.9, 1.0, -1.1, 1.7]),
]


@pytest.mark.parametrize("sum_mode", [False, True], ids=["separate", "sum"])
@pytest.mark.parametrize("Cn", [3, 6, 12, 36, 8, 64])
def test_spmm_multi(Cn, sum_mode, dev):
    ops = _ops()
    for li, (fams, scales) in enumerate(MULTI_LAYOUTS):
        idx = li + Cn + sum_mode
        Mo, Mi = SHAPES[idx % 4]
        N = NS[(idx // 2) % 4]
        rng = np.random.default_rng(100 * Cn + li)
        pairs = [(None, None) if f is None else operator(f, Mo, Mi, dev, seed=k) for k, f in enumerate(fams)]
        xs = [R.inputs(rng, N, Mo if f is None else Mi, Cn) for f in fams]
        terms = [(p[0], x, s) for p, x, s in zip(pairs, xs, scales)]
        r64, r32 = R.spmm_multi(terms, sum_mode, np.float64), R.spmm_multi(terms, sum_mode, np.float32)
        out = {}
        for ell in (1, 0):
            with ell_mode(ell):
                hx = [view(x, dev, pad=4 * k) for k, x in enumerate(xs)]            # inputs with different ld
                assert len({ops._v(h)[2] for h in hx}) == len(hx)
                y = ops.spmm_multi(hx, [p[1] for p in pairs], sum=sum_mode, scales=scales)
                torch.cuda.synchronize()
                ys = [y] if sum_mode else y
                for t in ys:                                                   # row bounds of the sum / of every term
                    if ops.rm_of(t) is not None:
                        check_rowbound(ops.rm_of(t), n32(t), (Cn, li, ell))
                assert (ops.rm_of(ys[0]) is not None) == (Cn == 64 and bool(ops.H2))
                out[ell] = [n32(t) for t in ys]
        tag = "spmm_multi[%s,C%d,layout%d,N%d,Mo%d]" % ("sum" if sum_mode else "separate", Cn, li, N, Mo)
        for k, (a, b) in enumerate(zip(out[1], out[0])):
            assert same_bits(a, b), (tag, k, "ELL differs from CSR")
            ebar(tag, "y" if sum_mode else "y%d" % k, a, r32 if sum_mode else r32[k], r64 if sum_mode else r64[k])


# ---- cape_spmm_multi_actgrad -------------------------------------------------------------------------------------------------
def _actgrad_case(Cn, storage, act, dev):
    idx = [64, 128, 256, 512].index(Cn) if Cn >= 64 else Cn // 8
    Mo, Mi = [(37, 53), (300, 190)][(idx + (act == "relu")) % 2]
    N = [3, 8][idx % 2] if Cn < 512 else 3
    dt = F32 if storage == "fp32" else BF16
    q = (lambda a: a) if dt == F32 else R.bf16
    rng = np.random.default_rng(Cn + len(storage))
    fams, scales = ["ell12", None, "ell8"], [1.0, 1.0, -0.5]
    pairs = [(None, None) if f is None else operator(f, Mo, Mi, dev, seed=k) for k, f in enumerate(fams)]
    xs = [q(R.inputs(rng, N, Mo if f is None else Mi, Cn)) for f in fams]
    ax = q(R.inputs(rng, N, Mo, Cn))
    ax[:, ::5, ::3], ax[:, 1::7, 1::2] = 0.0, -0.0                      # exact zeros of both signs next to negative values
    terms = [(p[0], x, s) for p, x, s in zip(pairs, xs, scales)]
    hx = [view(x, dev, dt) for x in xs]
    hax = view(ax, dev, dt, ld=Cn + 4) if storage == "bf16_w4" else view(ax, dev, dt)      # ld % 8 == 4: the 4-wide bf16 form
    assert np.array_equal(np.signbit(n64(hax)), np.signbit(ax))
    return dict(N=N, Mo=Mo, terms=terms, scales=scales, csrs=[p[1] for p in pairs], hx=hx, ax=ax, hax=hax, dt=dt,
                cq=Cn // (8 if (WIDE and storage != "bf16_w4") else 4))


@pytest.mark.parametrize("act", ["leaky", "relu"])
@pytest.mark.parametrize("storage", ["fp32", "bf16", "bf16_w4"])
@pytest.mark.parametrize("Cn", [64, 128, 256, 512])
def test_spmm_multi_actgrad(Cn, storage, act, dev):
    """y = (sum_k scale_k S_k x_k) * act'(act_x) and the bias-gradient partials; act' at an output of +0.0 / -0.0 is the slope
    (include/cape_hip.h, cape_act_grad_from_out: 1 only where the output is > 0)."""
    from cape_amd import _lib
    ops = _ops()
    c = _actgrad_case(Cn, storage, act, dev)
    N, Mo, cq = c["N"], c["Mo"], c["cq"]
    if not 8 <= cq <= 64:          # (CAPE_SPMM_WIDE=0 or the 4-wide bf16 layout at 512 channels: 128 lanes per row) refused, not launched
        with pytest.raises(_lib.CapeHipError):
            ops.spmm_multi(c["hx"], c["csrs"], sum=True, scales=c["scales"], act_x=c["hax"], act=act)
        return
    for ell in (1, 0):
        with ell_mode(ell):
            y, part, chunks = ops.spmm_multi(c["hx"], c["csrs"], sum=True, scales=c["scales"], act_x=c["hax"], act=act)
            db = torch.empty(Cn, device=dev)
            ops._finalize_bwd_prep([dict(ws=part, N=N, Mo=Mo, F=Cn, R=0, dbias=db, dcoef=None, dcoef_g=None, cstride=0, chunks=chunks)])
            torch.cuda.synchronize()
            if ell:
                y1, part1, db1 = y, part, db
            else:
                assert torch.equal(y, y1) and torch.equal(part[:, :, 0], part1[:, :, 0]) and torch.equal(db, db1)
    y64, db64 = R.actgrad(c["terms"], c["ax"], act, np.float64)
    y32, _ = R.actgrad(c["terms"], c["ax"], act, np.float32)
    tag = "actgrad[C%d,%s,%s,N%d,Mo%d]" % (Cn, storage, act, N, Mo)
    if storage == "fp32":
        ebar(tag, "y", n32(y1), y32, y64)
        if ops.rm_of(y1) is not None:
            check_rowbound(ops.rm_of(y1), n32(y1), tag)
    else:
        bf16_bar(tag, "y", n64(y1), y32, y64)
    assert chunks == (Mo * cq + 255) // 256 and tuple(part1.shape) == (N, chunks, 2, Cn)
    # the terms of these sums are the products v * x the rows are made of (times act'), not the finished y: a y that is small by
    # cancellation inside its row carries the rounding error of its products (the float32 restatement measures 1.5e-4 of sum |y|
    # on these inputs, 2e-7 of sum |products|)
    leaf = R.abs_terms(c["terms"]) * R.act_grad_from_out(c["ax"], act)
    sbar(tag, "bias partials", n64(part1[:, :, 0]), R.block_partials(y64, cq), R.block_partials(leaf, cq))
    sbar(tag, "dbias", n64(db1), db64, leaf.sum(axis=(0, 1)))


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("Cn", [8, 16, 32])
def test_spmm_multi_actgrad_refuses_fewer_than_eight_lanes_per_row(Cn, storage, dev):
    """The block reduction of the bias sums starts at the 8-lane rotation: with 1, 2 or 4 work items per row (C = 8, 16, 32 in the
    8-wide form; the 4-wide form has 2, 4 and 8) it would leave rows out.  Measured before the entry refused these sizes, fp32, 8-wide,
    C = 32, N = 3, Mo = 37: every partial held rows 0 and 2 of every four only (equal to that sum to 5e-8), dbias off by up to 0.31 of
    sum |terms| (C = 16: 0.33; C = 8 at N = 8, Mo = 300: 0.041) against the bar of 2e-6, y itself right to 1.2e-7.  Both the launch and the _chunks query now return CAPE_EINVAL and nothing is written."""
    ops = _ops()
    c = _actgrad_case(Cn, storage, "leaky", dev)
    N, Mo = c["N"], c["Mo"]
    y = ops.alloc_act(N, Mo, Cn, dev, dtype=c["dt"])
    y.fill_(7.0)
    part = torch.full((N, 64, 2, Cn), 7.0, device=dev)
    yp, ys, yl = ops._v(y)
    ap, as_, al = ops._v(c["hax"])
    legal = c["cq"] >= 8                                     # CAPE_SPMM_WIDE=0 at C = 32: eight 4-channel work items per row
    chunks = int(ops._fn("cape_spmm_multi_actgrad_chunks", y)(yp, ys, yl, ap, as_, al, Mo, Cn))
    arr = term_array(c["hx"], c["csrs"], scales=c["scales"])
    rc = ops._fn("cape_spmm_multi_actgrad", y)(arr, 3, yp, ys, yl, N, Mo, Cn, None, ap, as_, al, 1, ops._ptr(part), ops._stream())
    torch.cuda.synchronize()
    if not legal:
        assert chunks == EINVAL and rc == EINVAL
        assert bool((y == 7.0).all()) and bool((part == 7.0).all())
        return
    assert rc == 0 and chunks == (Mo * c["cq"] + 255) // 256
    part = part.flatten()[:N * chunks * 2 * Cn].view(N, chunks, 2, Cn)          # the layout the launch wrote
    y64, _ = R.actgrad(c["terms"], c["ax"], "leaky", np.float64)
    leaf = R.abs_terms(c["terms"]) * R.act_grad_from_out(c["ax"], "leaky")
    sbar("actgrad[C%d,%s]" % (Cn, storage), "bias partials", n64(part[:, :, 0]), R.block_partials(y64, c["cq"]), R.block_partials(leaf, c["cq"]))


# ---- cape_bwd_prep_spmm ------------------------------------------------------------------------------------------------------
def _g_and_bits(rng, N, M, F, q):
    g = q(R.inputs(rng, N, M, F))
    g[0, 5] = 0.0                                            # an all-zero row
    bits = rng.random((N, M, F)) < 0.55
    bits[0, 1, :32], bits[0, 2, :32] = False, True           # one all-zero and one all-ones word
    return g, bits


def _prep_spmm_checks(tag, family, N, Mo, F, storage, variants, dev, expect_chunks=None):
    ops = _ops()
    dt = F32 if storage == "fp32" else BF16
    q = (lambda a: a) if dt == F32 else R.bf16
    S, csr = operator(family, Mo, Mo, dev)
    rng = np.random.default_rng(Mo + F)
    g, bits = _g_and_bits(rng, N, Mo, F, q)
    rs = R.f32(rng.standard_normal((3, Mo)))
    hm = torch.tensor(R.sign_words(bits).view(np.int32), device=dev)
    hrs = torch.tensor(rs, dtype=torch.float32, device=dev)
    hg = view(g, dev, dt, ld=F + 4) if storage == "bf16_w4" else view(g, dev, dt)
    r64 = R.bwd_prep_spmm(S, g, bits, rs, 2, 2, np.float64)
    t1_32 = R.gather(S, r64["dz"], np.float32)
    cq = F // (8 if (WIDE and storage != "bf16_w4") else 4)
    if expect_chunks is not None:
        d0, d1 = ops.alloc_act(N, Mo, F, dev, dtype=dt), ops.alloc_act(N, Mo, F, dev, dtype=dt)
        got = int(ops._fn("cape_bwd_prep_spmm_chunks", hg)(*ops._v(hg), *ops._v(d0), *ops._v(d1), N, Mo, F))
        bps = (Mo * cq + 255) // 256
        rpb = 3 if N * bps >= 1536 else 2 if N * bps >= 1024 else 1
        assert got == (bps + rpb - 1) // rpb and rpb > 1, (got, bps, rpb)
        if WIDE:
            assert got == expect_chunks and bps % rpb != 0           # the last chunk ends in a wholly dead group
    first = None
    for R_, rg, joint in variants:
        for ell in (1, 0):
            with ell_mode(ell):
                kw = dict(rowscale=hrs if (R_ or rg is not None) else None, R=R_, rg=rg, joint=joint)
                ops.drop_rm(hg)                        # (each launch bounds the rows of g itself)
                dz_a, _, dc_a, dg_a = ops.bwd_prep(hg, mask=hm, **kw)
                t1_a = ops.spmm(dz_a, csr)
                ops.drop_rm(hg)
                g2 = hg
                out = ops.bwd_prep_spmm(g2, hm, csr, **kw)
                assert out is not None
                dz_b, t1_b, dc_b, dg_b = out
                torch.cuda.synchronize()
                vt = "%s R%d rg%s joint%d ell%d" % (tag, R_, rg, joint, ell)
                assert torch.equal(dz_a, dz_b) and torch.equal(t1_a, t1_b), vt                # the two launches it replaces, bit for bit
                assert np.array_equal(n64(dz_b), r64["dz"]) and np.array_equal(np.signbit(n64(dz_b)), np.signbit(r64["dz"])), vt
                if first is None:
                    first = t1_b
                assert torch.equal(t1_b, first), vt                                          # ELL = CSR, and no variant changes T1
                if dt == F32 and ops.H2:
                    check_rowbound(ops.rm_of(dz_b), n32(g2), vt + " rm_g")
                    check_rowbound(ops.rm_of(t1_b), n32(t1_b), vt + " rm_t1")
                    assert ops.rm_of(g2) is ops.rm_of(dz_b)
                if R_:
                    assert (rg is not None and joint) == (dc_b.shape[1] == R_ + 1)
                    sbar(vt, "dcoef", n64(dc_b[:, :R_]), r64["dcoef"][:, :R_], r64["dcoef_abs"][:, :R_])
                if rg is not None:
                    ref_g = np.einsum("r,nrf->nf", rs[rg], g)
                    sbar(vt, "dcoef_g", n64(dg_b), ref_g, np.einsum("r,nrf->nf", np.abs(rs[rg]), np.abs(g)))
    if dt == F32:
        ebar(tag, "T1", n32(first), t1_32, r64["t1"])
    else:
        bf16_bar(tag, "T1", n64(first), t1_32, r64["t1"])


PREP_VARIANTS = [(0, None, False), (1, 1, False), (1, 1, True), (2, 2, False), (2, 2, True), (2, None, False)]
PREP_CASES = [(f, F, "fp32") for f in ("ell8", "ell12", "csr") for F in (32, 64, 128, 256)] + \
             [("ell12", 64, "bf16"), ("ell8", 256, "bf16"), ("ell12", 64, "bf16_w4"), ("csr", 256, "bf16_w4")]


@pytest.mark.parametrize("family,F,storage", PREP_CASES)
def test_bwd_prep_spmm(family, F, storage, dev):
    idx = PREP_CASES.index((family, F, storage))
    Mo = (37, 300)[idx % 2]
    N = NS[(idx // 2) % 4]
    _prep_spmm_checks("bwd_prep_spmm[%s,F%d,%s,N%d,Mo%d]" % (family, F, storage, N, Mo), family, N, Mo, F, storage, PREP_VARIANTS, dev)


@pytest.mark.parametrize("Mo", [520, 777])
def test_bwd_prep_spmm_chunked_reduction_with_a_dead_last_group(Mo, dev):
    """N = 16, F = 256 (8-wide: 32 lanes per row): Mo = 520 -> 65 groups of 256 work items per sample, 1040 in all, two per block,
    the last block one live and one wholly dead group; Mo = 777 -> 98 groups, 1568 in all, three per block, the last block two live
    groups and one dead.  33 partial chunks per sample either way."""
    _prep_spmm_checks("bwd_prep_spmm[rpb,Mo%d]" % Mo, "ell12", 16, Mo, 256, "fp32", [(2, 2, True)], dev, expect_chunks=33)


# ---- cape_spmm_multi_prep ----------------------------------------------------------------------------------------------------
def _multi_prep_direct(hg, hm, csrs, masked, N, Mo, Mf, F, dev):
    """One term: below what ops.spmm_multi_prep takes; the C entry is called directly and finished with cape_bwd_prep_finalize."""
    ops = _ops()
    n = len(csrs)
    ys = [ops.alloc_act(N, Mo, F, dev, dtype=hg.dtype) for _ in csrs]
    rms = [ops._new_rm(y) if hg.dtype == F32 else None for y in ys]
    arr = term_array([hg] * n, csrs, ys=ys, rms=rms)
    chunks = int(ops._fn("cape_spmm_multi_prep_chunks", hg)(arr, n, N, Mo, F))
    assert chunks > 0
    part = torch.empty((N, chunks, n + 1, F), device=dev)
    bits = sum(1 << k for k, m in enumerate(masked) if m)
    rc = ops._fn("cape_spmm_multi_prep", hg)(arr, n, bits, ops._ptr(hm), Mf, N, Mo, F, ops._ptr(part), part.numel() * 4, ops._stream())
    assert rc == 0
    dcoef = torch.empty((N, max(n - 1, 1), F), device=dev)
    dg = torch.empty((N, F), device=dev)
    ops._finalize_bwd_prep([dict(ws=part, N=N, Mo=Mo, F=F, R=n - 1, dbias=None, dcoef=dcoef if n > 1 else None, dcoef_g=dg, cstride=0, chunks=chunks)])
    return ys, rms, dcoef, dg, chunks


def _multi_prep_checks(tag, family, N, Mo, F, storage, layouts, dev, expect_chunks=None):
    ops = _ops()
    dt = F32 if storage == "fp32" else BF16
    q = (lambda a: a) if dt == F32 else R.bf16
    Mf = 2 * Mo + 3
    ops3 = [operator(family, Mo, Mf, dev, seed=k) for k in range(3)]
    rng = np.random.default_rng(3 * Mo + F)
    g, bits = _g_and_bits(rng, N, Mf, F, q)
    hm = torch.tensor(R.sign_words(bits).view(np.int32), device=dev)
    hg = view(g, dev, dt, ld=F + 4) if storage == "bf16_w4" else view(g, dev, dt)
    cq = F // (8 if (WIDE and storage != "bf16_w4") else 4)
    cache, dz = {}, np.where(bits, g, 0.0)
    for which, masked in layouts:
        Ss, csrs = [ops3[k][0] for k in which], [ops3[k][1] for k in which]
        n = len(which)
        for k, m in zip(which, masked):                      # (one gather per operator, mask state and precision)
            for p in (np.float64, np.float32):
                if (k, bool(m), p) not in cache:
                    cache[k, bool(m), p] = R.gather(ops3[k][0], dz if m else g, p)
        T64 = [cache[k, bool(m), np.float64] for k, m in zip(which, masked)]
        T32 = [cache[k, bool(m), np.float32] for k, m in zip(which, masked)]
        for k, m in zip(which, masked):                      # sum |products| of every column sum (see test_spmm_multi_actgrad)
            if (k, bool(m), "abs") not in cache:
                cache[k, bool(m), "abs"] = R.abs_terms([(ops3[k][0], dz if m else g, 1.0)]).sum(axis=1)
        s64, sabs = [T.sum(axis=1) for T in T64], [cache[k, bool(m), "abs"] for k, m in zip(which, masked)]
        first = None
        for ell in (1, 0):
            with ell_mode(ell):
                vt = "%s terms%s masked%s ell%d" % (tag, which, masked, ell)
                dz_a = ops.bwd_prep(hg, mask=hm)[0]
                ops.drop_rm(hg)
                Ts_a = ops.spmm_multi([dz_a if m else hg for m in masked], csrs)
                if n >= 2:
                    out = ops.spmm_multi_prep(hg, hm, csrs, masked, joint=bool(ell))
                    assert out is not None, vt
                    Ts_b, dc, dg = out
                    rms = [ops.rm_of(t) for t in Ts_b]
                else:
                    Ts_b, rms, dc, dg, chunks = _multi_prep_direct(hg, hm, csrs, masked, N, Mo, Mf, F, dev)
                torch.cuda.synchronize()
                for k in range(n):
                    assert torch.equal(Ts_a[k], Ts_b[k]), (vt, k)                            # bwd_prep + spmm_multi, bit for bit
                    if dt == F32 and rms[k] is not None:
                        check_rowbound(rms[k], n32(Ts_b[k]), (vt, k))
                    ref_s, ref_a = s64[k], sabs[k]
                    got = dg if k == n - 1 else dc[:, k]
                    sbar(vt, "column sums of T%d" % k, n64(got), ref_s, ref_a)
                assert dt != F32 or not ops.H2 or all(r is not None for r in rms)
                if first is None:
                    first = Ts_b
                for a, b in zip(first, Ts_b):
                    assert torch.equal(a, b), vt                                             # ELL = CSR
        for k in range(n):
            (ebar if dt == F32 else bf16_bar)("%s terms%s" % (tag, which), "T%d" % k, (n32 if dt == F32 else n64)(first[k]), T32[k], T64[k])
    if expect_chunks is not None:
        arr = term_array([hg] * 3, [ops3[0][1], ops3[1][1], ops3[0][1]], ys=[ops.alloc_act(N, Mo, F, dev) for _ in range(3)])
        got = int(ops._fn("cape_spmm_multi_prep_chunks", hg)(arr, 3, N, Mo, F))
        bps = (Mo * cq + 255) // 256
        rpb = 3 if N * bps >= 1536 else 2 if N * bps >= 1024 else 1
        assert got == (bps + rpb - 1) // rpb and rpb > 1
        if WIDE:
            assert got == expect_chunks and bps % rpb != 0


MP_LAYOUTS = [([0, 1, 0], [1, 1, 0]),        # the `pair` leg: one set of gathers for terms 0 and 2
              ([0, 1, 2], [1, 0, 1]),        # three distinct operators: no pair
              ([0, 1], [0, 1]),
              ([0, 0], [1, 0]),              # two terms that pair
              ([1], [1])]
MP_CASES = [(f, F, "fp32") for f in ("ell4", "ell12", "csr") for F in (32, 64, 128, 256)] + \
           [("ell12", 64, "bf16"), ("ell4", 256, "bf16"), ("ell12", 64, "bf16_w4"), ("csr", 128, "bf16_w4")]


@pytest.mark.parametrize("family,F,storage", MP_CASES)
def test_spmm_multi_prep(family, F, storage, dev):
    idx = MP_CASES.index((family, F, storage))
    Mo = (37, 300)[(idx + 1) % 2]
    N = NS[(idx // 2 + 1) % 4]
    _multi_prep_checks("multi_prep[%s,F%d,%s,N%d,Mo%d]" % (family, F, storage, N, Mo), family, N, Mo, F, storage, MP_LAYOUTS, dev)


@pytest.mark.parametrize("Mo", [520, 777])
def test_spmm_multi_prep_chunked_reduction_with_a_dead_last_group(Mo, dev):
    _multi_prep_checks("multi_prep[rpb,Mo%d]" % Mo, "ell12", 16, Mo, 256, "fp32", MP_LAYOUTS[:1], dev, expect_chunks=33)


# ---- cape_spmm_combine -------------------------------------------------------------------------------------------------------
def _run_combine(c, dev, dt, dual, F, ld=None):
    ops = _ops()
    N, Mo = c["N"], c["Mo"]
    csrs = []
    from cape_amd.graph import HostCSR
    for m in c["S"]:
        csrs.append(ops.DeviceCSR(HostCSR(m), dev))
    hz = [view(z, dev, dt, ld=ld) for z in c["Z"]]
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).contiguous()
    y = ops.alloc_act(N, Mo, F, dev, dtype=dt)
    mask = None
    if dual:
        mask = torch.zeros((N, Mo, F // 32), device=dev, dtype=torch.int32) if F % 32 == 0 else None
        ops.spmm_combine(hz, csrs, y, to_acc2=0b100, rank=(t(c["rowscale"]), t(c["coef"]), 0b11), dual=True, mask=mask)
    else:
        from cape_amd import _lib
        ops.spmm_combine(hz, csrs, y, rank=(t(c["rowscale"]), t(c["coef"]), 0), bias=t(c["bias"]), bias_mode=_lib.BIAS_VERTEX, act="leaky")
    torch.cuda.synchronize()
    return y, mask, csrs


@pytest.mark.parametrize("dual", [False, True], ids=["single", "dual"])
@pytest.mark.parametrize("F", [6, 36, 64, 96])                     # scalar | 4-wide | 8-wide, mask words assembled from 4 lanes
@pytest.mark.parametrize("shape", [(37, 53), (300, 190)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", ["ell8", "ell12"])
def test_spmm_combine(family, shape, F, dual, dev):
    ops = _ops()
    c = R.combine_case(family, F, dual, Mo=shape[0], Mi=shape[1])
    y64, a1 = R.combine(prec=np.float64, **c["args"])
    y32, _ = R.combine(prec=np.float32, **c["args"])
    out = {}
    for ell in (1, 0):
        with ell_mode(ell):
            y, mask, csrs = _run_combine(c, dev, F32, dual, F)
            assert all(s.ell_w == R.expected_ell_w(family) and (R.degrees(m) == 0).any() for s, m in zip(csrs, c["S"]))
            if ops.rm_of(y) is not None:
                check_rowbound(ops.rm_of(y), n32(y), (family, F, dual, ell))
            assert (ops.rm_of(y) is not None) == (F == 64 and bool(ops.H2))
            out[ell] = (n32(y), None if mask is None else mask.cpu().numpy())
    tag = "combine[%s,%dx%d,F%d,%s]" % (family, shape[0], shape[1], F, "dual" if dual else "single")
    assert same_bits(out[1][0], out[0][0]), tag
    ebar(tag, "y", out[1][0], y32, y64)
    if out[1][1] is not None:
        assert np.array_equal(out[1][1], out[0][1]), tag
        got = R.unpack_words(out[1][1], F)
        unsure = R.uncertain_signs(a1)
        assert unsure.mean() <= 0.005, tag
        assert (a1 == 0).any() and np.array_equal(got[~unsure], (a1 > 0)[~unsure]), tag       # exact zeros (empty rows) included


# ---- bf16 storage of the unfused entries -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["w8", "w4"])
def test_bf16_storage_of_spmm_multi_and_combine(layout, dev):
    """cape_spmm_bf16 / cape_spmm_multi_bf16 / cape_spmm_combine_bf16 at C = 64: 8 channels per work item, and 4 (inputs in a buffer
    with ld % 8 == 4).  fp32 accumulation, one rounding of the result."""
    ops = _ops()
    Cn, N, Mo, Mi = 64, 3, 300, 53
    ld = Cn if layout == "w8" else Cn + 4
    rng = np.random.default_rng(64 + len(layout))
    S, csr = operator("ell12", Mo, Mi, dev)
    S2, csr2 = operator("csr", Mo, Mi, dev, seed=1)
    x, x2, xi = (R.bf16(R.inputs(rng, N, m, Cn)) for m in (Mi, Mi, Mo))
    terms = [(S, x, 1.0), (S2, x2, -0.5), (None, xi, 1.0)]
    c = R.combine_case("ell8", Cn, False, Mo=Mo, Mi=Mi)
    c["Z"] = [R.bf16(z) for z in c["Z"]]
    c["args"]["terms"] = [(s, z, 1.0) for s, z in zip(c["S"], c["Z"])]
    out = {}
    for ell in (1, 0):
        with ell_mode(ell):
            hx, hx2, hxi = (view(a, dev, BF16, ld=ld) for a in (x, x2, xi))
            o = [ops.spmm(hx, csr), ops.spmm_multi([hx, hx2, hxi], [csr, csr2, None], sum=True, scales=[1.0, -0.5, 1.0])]
            o += ops.spmm_multi([hx, hx2, hxi], [csr, csr2, None], scales=[1.0, -0.5, 1.0])
            o.append(_run_combine(c, dev, BF16, False, Cn, ld=ld)[0])
            torch.cuda.synchronize()
            out[ell] = [n64(t) for t in o]
    for a, b in zip(out[1], out[0]):
        assert np.array_equal(a, b)
    refs = [(R.gather(S, x, p),) for p in (np.float32, np.float64)]
    refs = [r + (R.spmm_multi(terms, True, p),) + tuple(R.spmm_multi(terms, False, p)) + (R.combine(prec=p, **c["args"])[0],)
            for r, p in zip(refs, (np.float32, np.float64))]
    for k, name in enumerate(["spmm", "multi sum", "multi 0", "multi 1", "multi 2", "combine"]):
        bf16_bar("bf16[%s]" % layout, name, out[1][k], refs[0][k], refs[1][k])


# ---- refused arguments: return codes only, nothing is launched ---------------------------------------------------------------
def test_refused_arguments(dev):
    ops = _ops()
    N, Mo, Mi, Cn = 2, 37, 53, 8
    S, csr = operator("ell8", Mo, Mi, dev)
    rng = np.random.default_rng(0)
    x = R.inputs(rng, N, Mi, Cn)
    y = ops.alloc_act(N, Mo, Cn, dev)
    y.fill_(7.0)
    ell = (csr.rowptr_t.data_ptr(), csr.ell_col_t.data_ptr(), csr.ell_val_t.data_ptr(), 8)
    assert spmm_rc(view(x, dev, off=2, pad=2), csr, y, operands=ell) == EINVAL           # ELL operands with an unaligned view
    for w in (5, 16):
        assert spmm_rc(view(x, dev), csr, y, operands=ell[:3] + (w,)) == EINVAL
    assert spmm_rc(view(x, dev), csr, y, operands=(ell[0], ell[1] + 4, ell[2], 8)) == EINVAL   # ELL arrays off their 16-byte alignment
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    # F = 96 (12 / 24 work items per row) in the fused forms: the caller keeps the two launches
    Sq, csq = operator("ell8", Mo, Mo, dev)
    g, bits = _g_and_bits(rng, N, Mo, 96, lambda a: a)
    hg, hm = view(g, dev), torch.tensor(R.sign_words(bits).view(np.int32), device=dev)
    hrs = torch.tensor(R.f32(rng.standard_normal((3, Mo))), dtype=torch.float32, device=dev)
    assert ops.bwd_prep_spmm(hg, hm, csq, rowscale=hrs, R=2, rg=2) is None
    Sc, csc = operator("ell4", 17, Mo, dev)
    assert ops.spmm_multi_prep(hg, hm, [csc, csc], [True, False]) is None
    # a partials buffer one byte short
    F = 32
    hg = view(g[:, :, :F], dev)
    hm = torch.tensor(R.sign_words(bits[:, :, :F]).view(np.int32), device=dev)
    dz, t1 = ops.alloc_act(N, Mo, F, dev), ops.alloc_act(N, Mo, F, dev)
    dz.fill_(7.0)
    chunks = int(ops.lib.cape_bwd_prep_spmm_chunks(*ops._v(hg), *ops._v(dz), *ops._v(t1), N, Mo, F))
    part = torch.empty((N, chunks, 4, F), device=dev)
    rp, ci, va, ew = csq.operands()
    call = lambda nbytes: ops.lib.cape_bwd_prep_spmm(*ops._v(hg), ops._ptr(hm), C.c_void_p(rp), C.c_void_p(ci), C.c_void_p(va), ew, *ops._v(dz),
                                                     *ops._v(t1), ops._ptr(hrs), 2, 2, N, Mo, F, ops._ptr(part), nbytes, None, None, ops._stream())
    assert call(part.numel() * 4 - 1) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((dz == 7.0).all())
    assert call(part.numel() * 4) == 0
    ys = [ops.alloc_act(N, 17, F, dev) for _ in range(2)]
    arr = term_array([hg, hg], [csc, csc], ys=ys)
    ch = int(ops.lib.cape_spmm_multi_prep_chunks(arr, 2, N, 17, F))
    part = torch.empty((N, ch, 3, F), device=dev)
    assert ops.lib.cape_spmm_multi_prep(arr, 2, 1, ops._ptr(hm), Mo, N, 17, F, ops._ptr(part), part.numel() * 4 - 1, ops._stream()) == EWORKSPACE
    assert ops.lib.cape_spmm_multi_prep(arr, 2, 1, ops._ptr(hm), Mo, N, 17, F, ops._ptr(part), part.numel() * 4, ops._stream()) == 0
    torch.cuda.synchronize()


# ---- the knob legs -----------------------------------------------------------------------------------------------------------
KNOBS = [dict(CAPE_SPMM_WIDE="0"),       # the 4-wide instantiations of every kernel, the fused fp32 ones included (cq = 64 at F = 256,
                                         # cq = 8 at F = 32: the 8-lane rotation); the activation-gradient form refuses 512 channels
         dict(CAPE_SPMM_ELL="0"),
         dict(CAPE_SPMM_UNROLL="0"),     # entry loop as written
         dict(CAPE_SPMM_UNROLL="8")]     # entries in groups of 8


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "+".join("%s=%s" % kv for kv in sorted(k.items())))
def test_sparse_kernels_under_knob(knobs):
    """The knobs are latched at first use: one fresh child process per setting runs every other test of this module."""
    env = dict(os.environ)
    env.update(knobs)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_sparse.py"), "-x", "-q", "-m", "gpu", "-k", "not knob"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    tail = r.stdout.decode()[-2500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
