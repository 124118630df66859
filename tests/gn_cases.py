"""The cases of tests/test_gpu_groupnorm.py: the eight kernels of csrc/groupnorm.hip called through ``cape_groupnorm_fwd`` /
``cape_groupnorm_bwd`` at the smallest shapes that reach every chunk form of the partial-sum pass, every form of the apply
pass and every edge of a channel quad.  TEST INFRASTRUCTURE ONLY (no GPU needed here; tests/test_gn_cases_host.py checks
this file on the CPU).

* ``plan(N, V, C, G, rowmax)`` restates the host dispatch: the row chunk ``RB`` of ``gn_rows``, the column tiles of the
  partial-sum pass with their lane split, ``cp`` / ``CL`` of the two final kernels, the form of the apply pass and its grid.
* ``forward_ref`` / ``backward_ref`` are plain-numpy restatements in a precision ``T``: float64 is the reference, float32 the
  reference's own order (two-pass mean / variance, ``(x - mean) * rstd * gamma + beta``) that kernel_bars.element_bar measures
  against.  The backward takes the ReLU mask as an ARGUMENT: the GPU test hands it ``y_dev > 0``, which pins the kernel's claim
  that the mask it re-derives from the same fma is the forward's decision.
* ``emu_forward`` / ``emu_backward`` restate the KERNEL's formulation in its own order: pivot row 0, sums per lane (rows
  ``rl, rl + lanes, ..``) and then over the lanes in index order -- float64 from the difference on in the forward, float32
  sums in the backward --, float64 combine, coefficient form ``fma(a, x, b)``.  The host test holds them to half of
  every bar the GPU test applies: the formulation alone must not eat the margin.  (On the MI355X the figures of the device
  equal the emulation's to three digits.)
* One table of cases; each names the form it exists for.

Row 0 as an outlier (the pivot of the single-pass variance is ``x[n, 0, c]``; every channel of row 0 set to k sigma, k in 4,
16, 64, 256; C = 32 in 4 groups at the four chunk shapes).  Emulated error of rstd over max rstd, as the worst over the four k,
next to half of its bar (4 x the two-pass float32 restatement's error, at least 4 * 2^-24):

    chunk   float64 from the difference on (the kernel)   half of the bar        float32 differences, sums and partials (before)
    RB  16  3.8e-08                                       1.2e-07 .. 2.4e-07     2.7e-07 (k = 4) .. 1.1e-06 (k = 256)
    RB  32  5.7e-08                                       2.5e-07 .. 3.2e-07     9.5e-07 (k = 4) .. 5.4e-06 (k = 64)
    RB  64  5.9e-08                                       2.5e-07 .. 3.7e-07     1.3e-06 (k = 4) .. 7.7e-06 (k = 64)
    RB 128  5.9e-08                                       3.1e-07 .. 3.9e-07     1.7e-06 (k = 4) .. 1.6e-05 (k = 64)

With float32 sums NO k stayed under half of the bar at every chunk form (and unit-normal data with one or two channels per
group did not either: a 4-sigma first row turns up by chance; on the MI355X rb128_v130 missed the whole bar by 4.2 x); with
float64 sums all four do, so all four are required cases (PIVOT_REQUIRED).  ``emu_forward(acc=F32)`` still restates the former
arithmetic; tests/test_gn_cases_host.py prints both."""
import zlib

import numpy as np

import kernel_bars
import parity_bar

EPS = np.float32(1e-5)
F32 = np.float32
F64 = np.float64


# ----------------------------------------------------------------------------------------------------- the dispatch
def gn_rows(N, V):
    rb = 128
    while rb > 16 and N * ((V + rb - 1) // rb) < 1024:
        rb >>= 1
    return rb


def pad4(C):
    return (C + 3) & ~3


def workspace_bytes(N, V, C):
    RB = gn_rows(N, V)
    return N * ((V + RB - 1) // RB) * 2 * pad4(C) * 8          # float64 partials of the forward (the backward's are float32)


def plan(N, V, C, G, rowmax):
    """What cape_groupnorm_fwd / _bwd launch for this shape (both take the same decisions)."""
    assert N >= 1 and V >= 1 and C >= 1 and G >= 1 and C % G == 0 and C // G <= 256
    RB = gn_rows(N, V)
    chunks = (V + RB - 1) // RB
    Cp = pad4(C)
    c4 = Cp >> 2
    tiles = []
    for cbase in range(0, Cp, 256):
        c4n = min(256, Cp - cbase) >> 2
        lanes = 256 // c4n
        tiles.append(dict(cbase=cbase, c4n=c4n, lanes=lanes, rows_per_lane=(RB + lanes - 1) // lanes, idle_lanes=max(0, lanes - RB)))
    Cg = C // G
    cp = 1
    while cp < Cg:
        cp <<= 1
    CL = 256 // cp
    if not rowmax:
        form = "plain"                                       # gn_apply_kernel / gn_bwd_apply_kernel, rm = NULL
    elif c4 <= 64 and (c4 & (c4 - 1)) == 0:
        form = "fused"                                       # the same kernels bound each row inside a lane group
    elif C <= 1024:
        form = "rows"                                        # gn_apply_rows_kernel / gn_bwd_apply_rows_kernel
    else:
        form = "standalone"                                  # plain apply, then cape_rowmax
    if form == "rows":
        block_rows = 256 // c4
        blocks = (N * V + block_rows - 1) // block_rows
    else:
        block_rows = None
        blocks = (N * V * c4 + 255) // 256
    return dict(RB=RB, chunks=chunks, last_chunk_rows=V - (chunks - 1) * RB, Cp=Cp, c4=c4, tiles=tiles, Cg=Cg, cp=cp, CL=CL,
                form=form, block_rows=block_rows, grid=max(1, min(blocks, 8192)), capped=blocks > 8192,
                partial_grid=N * chunks, final_grid=N * G)


# ----------------------------------------------------------------------------------------------------- references
def _per_channel(v, Cg):
    """[N, G] -> [N, 1, C]"""
    return np.repeat(v, Cg, axis=1)[:, None, :]


def _group_rows(a, G):
    """[N, V, C] -> contiguous [N, G, V * Cg] (so that numpy's float32 sums over the last axis are pairwise)."""
    N, V, C = a.shape
    return np.ascontiguousarray(a.reshape(N, V, G, C // G).transpose(0, 2, 1, 3)).reshape(N, G, V * (C // G))


def _sum_rows(a, T):
    """sum over V of [N, V, C] -> [N, C], over a contiguous axis"""
    return np.ascontiguousarray(a.transpose(0, 2, 1)).sum(-1, dtype=T)


def forward_ref(x, gamma, beta, G, relu, T, eps=EPS):
    """dict y [N, V, C], stats [N, G, 2] = (mean, rstd), coef [N, 4, C] = (a, b, rstd, mean * rstd) in precision ``T``:
    population variance, eps inside the root, two passes."""
    N, V, C = x.shape
    Cg = C // G
    xt, gt, bt = x.astype(T), gamma.astype(T), beta.astype(T)
    xg = _group_rows(xt, G)
    mean = xg.mean(-1, dtype=T)
    var = ((xg - mean[..., None]) ** 2).mean(-1, dtype=T)
    rstd = (T(1) / np.sqrt(var + T(eps))).astype(T)
    mc, rc = _per_channel(mean, Cg), _per_channel(rstd, Cg)
    y = ((xt - mc) * rc * gt + bt).astype(T)
    if relu:
        y = np.where(y > 0, y, T(0)).astype(T)
    a = (rc * gt).astype(T)
    coef = np.concatenate([a, bt - mc * a, rc + 0 * gt, mc * rc + 0 * gt], axis=1).astype(T)
    return dict(y=y, stats=np.stack([mean, rstd], axis=-1), coef=coef)


def backward_ref(x, dy, gamma, stats, G, mask, add, T):
    """dict dx, dx_add (None without ``add``), bcoef [N, 3, C] = (A_c, B_g, C_g), dgamma_p / dbeta_p [N, C] and the sum of
    |terms| of each of those sums.  ``stats`` in precision T from forward_ref; ``mask``: boolean [N, V, C] or None (no ReLU).
    The terms of dgamma are d' x rstd and d' mean rstd, counted one by one: xhat is itself a difference, and the cancellation
    inside it belongs on the condition-aware scale like the cancellation between terms (with the mean 50 sigma off zero every
    float32 evaluation of xhat, the reference's own order included, carries 50 roundings of xhat)."""
    N, V, C = x.shape
    Cg = C // G
    xt, gt = x.astype(T), gamma.astype(T)
    mc, rc = _per_channel(stats[..., 0].astype(T), Cg), _per_channel(stats[..., 1].astype(T), Cg)
    xhat = ((xt - mc) * rc).astype(T)
    d = dy.astype(T)
    if mask is not None:
        d = np.where(mask, d, T(0)).astype(T)
    dbeta, dgamma = _sum_rows(d, T), _sum_rows(d * xhat, T)
    Tn = T(V * Cg)
    S1 = (dbeta * gt).reshape(N, G, Cg).sum(-1, dtype=T)
    S2 = (dgamma * gt).reshape(N, G, Cg).sum(-1, dtype=T)
    rstd = stats[..., 1].astype(T)
    A = (rc * gt).astype(T)
    B, Cc = _per_channel(rstd * S1 / Tn, Cg), _per_channel(rstd * S2 / Tn, Cg)
    dx = (A * d - (B + xhat * Cc)).astype(T)
    return dict(dx=dx, dx_add=None if add is None else (dx + add.astype(T)).astype(T),
                bcoef=np.concatenate([A, B + 0 * gt, Cc + 0 * gt], axis=1).astype(T),
                dgamma_p=dgamma, dbeta_p=dbeta, dgamma_abs=_sum_rows(np.abs(d) * (np.abs(xt) + np.abs(mc)) * rc, T),
                dbeta_abs=_sum_rows(np.abs(d), T))


# ------------------------------------------------------------------------------------- the kernel's own formulation
def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64, one float64 sum, one rounding to float32 (a double rounding
    in about one result in 2^29: an emulation, not a bit-for-bit model)."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _partials(e0, f1a, f1b, RB, acc):
    """gn_partial_kernel: per (sample, chunk, channel) t0 = sum e0, t1 = sum f1a * f1b in the kernel's order -- per column tile
    of 256 floats ``lanes = 256 / c4n`` row lanes, lane rl adds rows rl, rl + lanes, .. of the chunk one after the other in
    precision ``acc`` (t1 by fma), then lane 0 adds the other lanes in index order.  Returns two ``acc`` arrays [N, chunks, C]:
    F64 is gn_stat_partial_kernel (the inputs are float64 differences), F32 gn_partial_kernel of the backward."""
    N, V, C = e0.shape
    chunks = (V + RB - 1) // RB
    out0, out1 = np.zeros((N, chunks, C), acc), np.zeros((N, chunks, C), acc)
    for cbase in range(0, pad4(C), 256):
        c4n = min(256, pad4(C) - cbase) >> 2
        lanes = 256 // c4n
        rpl = (RB + lanes - 1) // lanes
        cs = slice(cbase, min(C, cbase + 256))
        cw = cs.stop - cs.start

        def lay(a):                                           # [N, chunks, rpl, lanes, cw], row of the chunk = j * lanes + rl
            z = np.zeros((N, chunks * RB, cw), a.dtype)
            z[:, :V] = a[:, :, cs]
            z = z.reshape(N, chunks, RB, cw)
            if rpl * lanes != RB:
                z = np.concatenate([z, np.zeros((N, chunks, rpl * lanes - RB, cw), a.dtype)], axis=2)
            return z.reshape(N, chunks, rpl, lanes, cw)

        E0, A1, B1 = lay(e0), lay(f1a), lay(f1b)
        t0, t1 = np.zeros((N, chunks, lanes, cw), acc), np.zeros((N, chunks, lanes, cw), acc)
        for j in range(rpl):
            t0 = (t0 + E0[:, :, j]).astype(acc)
            t1 = fma32(A1[:, :, j], B1[:, :, j], t1) if acc is F32 else A1[:, :, j] * B1[:, :, j] + t1     # (no fma: an emulation)
        s0, s1 = t0[:, :, 0], t1[:, :, 0]
        for l in range(1, min(lanes, RB)):                    # (the lanes past the chunk's rows hold zeros)
            s0 = (s0 + t0[:, :, l]).astype(acc)
            s1 = (s1 + t1[:, :, l]).astype(acc)
        out0[:, :, cs], out1[:, :, cs] = s0, s1
    return out0, out1


def emu_forward(x, gamma, beta, G, relu, eps=EPS, RB=None, acc=F64):
    """cape_groupnorm_fwd restated: float32 y, stats, coef as forward_ref lays them out.  ``RB``: force a chunk form; ``acc``:
    F32 restates the pass as it was with float32 sums and partials (the module docstring quotes it)."""
    N, V, C = x.shape
    Cg = C // G
    RB = gn_rows(N, V) if RB is None else RB
    x, gamma, beta = x.astype(F32), gamma.astype(F32), beta.astype(F32)
    p = x[:, :1, :]
    d = (x - p).astype(F32) if acc is F32 else x.astype(F64) - p.astype(F64)
    S, Q = _partials(d, d, d, RB, acc)
    S, Q = S.astype(F64).sum(1), Q.astype(F64).sum(1)        # gn_final_kernel: float64 from here
    p64 = p[:, 0, :].astype(F64)
    Tn = float(V) * float(Cg)
    mean = (S + V * p64).reshape(N, G, Cg).sum(-1) / Tn
    dp = p64 - np.repeat(mean, Cg, axis=1)
    m2 = (Q + 2.0 * dp * S + V * dp * dp).reshape(N, G, Cg).sum(-1)
    var = np.maximum(m2 / Tn, 0.0)
    rstd = (1.0 / np.sqrt(var + F64(eps))).astype(F32)
    mean32 = mean.astype(F32)
    mc, rc = _per_channel(mean32, Cg), _per_channel(rstd, Cg)
    a = (rc * gamma).astype(F32)
    b = fma32(-mc, a, beta + 0 * a)
    coef = np.concatenate([a, b, rc + 0 * a, (mc * rc).astype(F32) + 0 * a], axis=1).astype(F32)
    y = fma32(a, x, b)
    if relu:
        y = np.where(y > 0, y, F32(0)).astype(F32)
    return dict(y=y, stats=np.stack([mean32, rstd], axis=-1), coef=coef)


def emu_backward(x, dy, gamma, stats, coef, G, relu, add, RB=None):
    """cape_groupnorm_bwd restated on the float32 stats / coef of the forward; the mask is fma(a, x, b) > 0."""
    N, V, C = x.shape
    Cg = C // G
    RB = gn_rows(N, V) if RB is None else RB
    x, gamma = x.astype(F32), gamma.astype(F32)
    a, b, rr, mr = (coef[:, i:i + 1, :].astype(F32) for i in range(4))
    d = dy.astype(F32)
    if relu:
        d = np.where(fma32(a, x, b) > 0, d, F32(0)).astype(F32)
    xh = fma32(x, rr, -mr)
    s1, s2 = _partials(d, d, xh, RB, F32)
    a1, a2 = s1.astype(F64).sum(1), s2.astype(F64).sum(1)
    Tn = float(V) * float(Cg)
    rstd = stats[..., 1].astype(F32)
    S1 = (a1 * gamma.astype(F64)).reshape(N, G, Cg).sum(-1)
    S2 = (a2 * gamma.astype(F64)).reshape(N, G, Cg).sum(-1)
    B = _per_channel((rstd.astype(F64) * S1 / Tn).astype(F32), Cg)
    Cc = _per_channel((rstd.astype(F64) * S2 / Tn).astype(F32), Cg)
    A = (_per_channel(rstd, Cg) * gamma).astype(F32)
    inner = fma32(xh, Cc, B)
    dx = (A.astype(F64) * d.astype(F64) - inner.astype(F64)).astype(F32)          # (contracted: one rounding)
    return dict(dx=dx, dx_add=None if add is None else (dx + add.astype(F32)).astype(F32),
                bcoef=np.concatenate([A, B + 0 * A, Cc + 0 * A], axis=1).astype(F32),
                dgamma_p=a2.astype(F32), dbeta_p=a1.astype(F32))


# ----------------------------------------------------------------------------------------------------- the cases
DATA_KINDS = ("normal", "offset", "zerovar", "gamma0", "relurow", "pivot")
ZV_CONST = F32(1.5)                     # the constant of the zero-variance group (no power of two: mean * rstd is rounded)
OFFSET = F32(50.0)
RELU_ROW = F32(-6.0)


def _case(name, N, V, C, G, why, relu=0, rm=0, add=0, data="normal", k=0, seed=None, pad="nan"):
    """``seed``: the name whose inputs the case uses (two cases that differ in rowmax_out alone share their references).
    ``pad``: what the GPU test puts into the pad lanes and the slack of x, dy, dx_add -- NaN, or ("big") -1e30: inside
    gn_quad_bound a NaN lane is dropped by fmaxf whether or not the lane counts, a large finite one is not."""
    assert data in DATA_KINDS and pad in ("nan", "big")
    return dict(name=name, N=N, V=V, C=C, G=G, relu=relu, rm=rm, add=add, data=data, k=k, why=why, seed=seed or name, pad=pad)


def case_plan(c):
    return plan(c["N"], c["V"], c["C"], c["G"], bool(c["rm"]))


CHUNK_SHAPES = {16: (2, 37), 32: (256, 97), 64: (512, 65), 128: (1024, 130)}

CASES = [
    # ---- the four row-chunk forms of the partial-sum pass
    _case("rb16_v37", 2, 37, 8, 2, "RB = 16, last chunk 5 rows, 128 lanes for 16 rows", relu=1, rm=1),
    _case("rb32_v97", 256, 97, 8, 2, "RB = 32, last chunk 1 row", relu=1, add=1),
    _case("rb64_v65", 512, 65, 8, 2, "RB = 64, last chunk 1 row", rm=1),
    _case("rb128_v130", 1024, 130, 32, 32, "RB = 128: four rows per lane, last chunk 2 rows; Cg = 1", relu=1, rm=1, add=1),
    _case("rb128_c4", 1024, 130, 4, 1, "RB = 128 with c4n = 1: 256 lanes, 128 of them idle", relu=1),
    _case("v1", 5, 1, 64, 4, "V = 1: statistics over the channels only, the pivot is the data", relu=1, rm=1, add=1),
    _case("v3", 5, 3, 20, 5, "V = 3 < RB", relu=0, rm=1),
    _case("n1_c4", 1, 37, 4, 4, "one sample, one quad, c4n = 1; Cg = 1", relu=1, rm=1),
    # ---- grid caps: the stride loops of the apply kernels
    _case("cap_plain", 1024, 130, 64, 32, "plain apply over more than 8192 x 256 quads", relu=1, add=1),
    _case("cap_fused", 1024, 130, 64, 32, "the same grid with the row bound inside the stride loop", relu=1, rm=1, add=1, seed="cap_plain"),
    _case("cap_rows", 64, 130, 1024, 32, "rows form over more than 8192 one-row groups", relu=1, rm=1),
]

# ---- channel forms, each with (bound, ReLU, no dx_add) and (no bound, no ReLU, dx_add)
for _C, _G, _why in [
        (3, 3, "C % 4 != 0, one quad, Cg = 1"),
        (3, 1, "C % 4 != 0, one quad, one group"),
        (4, 4, "one quad"),
        (6, 2, "two quads, the second with two lanes; Cg = 3 in cp = 4"),
        (12, 4, "c4 = 3: rows form with 85 rows per block (the LDS maxima had 64 slots)"),
        (20, 5, "rows form, 51 rows per block"),
        (38, 2, "C % 4 = 2 in ten quads; Cg = 19 in cp = 32"),
        (48, 48, "Cg = 1: CL = 256 chunk lanes for 3 chunks"),
        (64, 32, "fused, 16 lanes per row"),
        (96, 32, "rows form, 24 lanes per row; Cg = 3"),
        (256, 32, "fused, one wave per row"),
        (256, 1, "Cg = 256: cp = 256, CL = 1 below 3 chunks"),
        (260, 2, "second column tile of ONE quad (256 lanes); rows form with 3 rows per block; a group across both tiles"),
        (510, 2, "Cg = 255 in cp = 256; C % 4 = 2 in the second tile"),
        (544, 32, "[features | condition] of the GraphCMR blocks: Cg = 17, three column tiles"),
        (1024, 32, "rows form with ONE row per block"),
        (1028, 257, "C > 1024: plain apply, then cape_rowmax")]:
    CASES.append(_case("c%d_g%d_rm" % (_C, _G), 3, 37, _C, _G, _why, relu=1, rm=1, add=0))
    CASES.append(_case("c%d_g%d_norm" % (_C, _G), 3, 37, _C, _G, _why, relu=0, rm=0, add=1))

CASES += [
    _case("c12_g4_rm_norelu_add", 3, 37, 12, 4, "c4 = 3 rows form without ReLU, with dx_add", relu=0, rm=1, add=1),
    _case("c64_g32_rm_norelu_add", 3, 37, 64, 32, "fused without ReLU, with dx_add", relu=0, rm=1, add=1),
    _case("c1028_g257_rm_norelu_add", 3, 37, 1028, 257, "standalone bound without ReLU, with dx_add", relu=0, rm=1, add=1),
    _case("c96_g32_relu_norm_add", 3, 37, 96, 32, "ReLU without a bound, with dx_add", relu=1, rm=0, add=1),
    _case("c6_g2_rm_bigpad", 3, 37, 6, 2, "fused bound, pad lanes of -1e30: only ``left`` keeps them out of the bound", relu=1, rm=1, add=1, pad="big"),
    _case("c38_g2_rm_bigpad", 3, 37, 38, 2, "rows-form bound, pad lanes of -1e30", relu=1, rm=1, add=1, pad="big"),
]

# ---- data
for _rb, (_N, _V) in sorted(CHUNK_SHAPES.items()):
    _C, _G = (32, 4) if _rb == 128 else (8, 2)
    CASES.append(_case("offset_rb%d" % _rb, _N, _V, _C, _G, "every channel 50 sigma off zero at RB = %d: the pivot shift" % _rb,
                       relu=1, rm=1, add=1, data="offset"))
CASES += [
    _case("offset_c38", 3, 37, 38, 2, "50 sigma off zero with pad lanes", relu=0, rm=0, data="offset"),
    _case("zerovar_relu", 3, 37, 12, 4, "one (sample, group) is constant: var = 0, rstd = 1 / sqrt(eps)", relu=1, rm=1, data="zerovar"),
    _case("zerovar_norelu", 3, 37, 12, 4, "the same without ReLU", relu=0, add=1, data="zerovar"),
    _case("gamma0_c8", 3, 37, 8, 2, "gamma = 0 with beta = 0 (mask at exactly 0) and with beta > 0", relu=1, rm=1, data="gamma0"),
    _case("gamma0_c96", 3, 37, 96, 32, "the same in the rows form", relu=1, rm=1, add=1, data="gamma0"),
    _case("relurow_c12", 3, 37, 12, 4, "a row ReLU switches off entirely: bound exactly 0 (rows form)", relu=1, rm=1, data="relurow"),
    _case("relurow_c64", 3, 37, 64, 32, "the same in the fused form", relu=1, rm=1, data="relurow"),
    _case("relurow_c1028", 3, 37, 1028, 257, "the same through cape_rowmax", relu=1, rm=1, data="relurow"),
]

PIVOT_KS = (4, 16, 64, 256)
PIVOT_REQUIRED = PIVOT_KS               # see the module docstring
PIVOT_CASES = []
for _k in PIVOT_KS:
    for _rb, (_N, _V) in sorted(CHUNK_SHAPES.items()):
        PIVOT_CASES.append(_case("pivot_k%d_rb%d" % (_k, _rb), _N, _V, 32, 4, "row 0 at %d sigma, RB = %d" % (_k, _rb),
                                 relu=1, rm=1, data="pivot", k=_k))
REQUIRED_PIVOT_CASES = [c for c in PIVOT_CASES if c["k"] in PIVOT_REQUIRED]
MEASURED_PIVOT_CASES = [c for c in PIVOT_CASES if c["k"] not in PIVOT_REQUIRED]

ALL_CASES = CASES + REQUIRED_PIVOT_CASES


def by_name(name):
    return next(c for c in CASES + PIVOT_CASES if c["name"] == name)


# ----------------------------------------------------------------------------------------------------- inputs
def zerovar_where(c):
    """(sample, group) of the constant group of a ``zerovar`` case"""
    return c["N"] - 1, c["G"] - 1


def gamma0_channels(c):
    """(channel with gamma = 0 and beta = 0, channel with gamma = 0 and beta = 0.3)"""
    return 1, c["C"] - 3


def relu_row(c):
    return c["V"] // 2


def inputs(c):
    """x, dy, add (None when the case has no dx_add) [N, V, C], gamma, beta [C]: float32, dense, seeded by the case's name."""
    rng = np.random.default_rng(zlib.crc32(c["seed"].encode()))
    N, V, C, G = c["N"], c["V"], c["C"], c["G"]
    Cg = C // G
    f = lambda *s: rng.standard_normal(s).astype(F32)
    x, dy = f(N, V, C), f(N, V, C)
    add = f(N, V, C) if c["add"] else None
    gamma = (1 + 0.1 * np.clip(f(C), -4, 4)).astype(F32)                     # positive
    beta = (0.1 * f(C)).astype(F32)
    if c["data"] == "offset":                                                 # equal inside a group, so that its sigma stays 1
        x = (x + OFFSET * np.repeat(np.where(np.arange(G) % 2 == 0, 1, -1), Cg).astype(F32)).astype(F32)
    elif c["data"] == "zerovar":
        n, g = zerovar_where(c)
        x[n, :, g * Cg:(g + 1) * Cg] = ZV_CONST
    elif c["data"] == "gamma0":
        c0, c1 = gamma0_channels(c)
        gamma[c0], beta[c0] = 0, 0
        gamma[c1], beta[c1] = 0, F32(0.3)
    elif c["data"] == "relurow":
        x[:, relu_row(c), :] = RELU_ROW
    elif c["data"] == "pivot":
        x[:, 0, :] = F32(c["k"])
    return dict(x=x, dy=dy, add=add, gamma=gamma, beta=beta)


# ----------------------------------------------------------------------------------------------------- the bars
ELEMENT_QUANTITIES = ("y", "stats", "coef", "dx", "dx_add", "bcoef")
SUM_QUANTITIES = ("dgamma_p", "dbeta_p")


def split(c, fwd, bwd):
    """The arrays kernel_bars.element_bar is applied to: dict name -> array.  In a ``zerovar`` case the entries that have bounds
    of their own (y and C_g of the constant group: zerovar_bounds) are set to 0 in every party."""
    deg = degenerate_channels(c)
    q = {}
    if fwd is not None:
        q.update(y=np.where(deg[:, None, :], 0, fwd["y"]).astype(fwd["y"].dtype), stats=fwd["stats"], coef=fwd["coef"])
    if bwd is not None:
        q["dx"] = bwd["dx"]
        if bwd["dx_add"] is not None:
            q["dx_add"] = bwd["dx_add"]
        bc = bwd["bcoef"].copy()
        bc[:, 2][deg] = 0
        q["bcoef"] = bc
    return q


def element_fraction(got, f32, ref64):
    """The error of ``got`` as a fraction of kernel_bars.element_bar: of max(4 x the float32 restatement's error, the floor) and
    of the backstop, whichever is tighter."""
    e, e32 = kernel_bars.mat_err(got, ref64), kernel_bars.mat_err(f32, ref64)
    return max(e / max(4.0 * e32, parity_bar.FLOOR), e / kernel_bars.TOL)


def sum_fraction(got, ref64, abs_terms):
    """The worst error of ``got`` as a fraction of kernel_bars.sum_bar (inf where a sum without terms is not exactly 0)."""
    err = np.abs(np.asarray(got, F64) - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fr = np.where(abs_terms > 0, err / (kernel_bars.SUM_REL * abs_terms), np.where(err > 0, np.inf, 0.0))
    return float(fr.max())


def degenerate_channels(c):
    """Boolean [N, C]: the channels of the constant group of a ``zerovar`` case.  There xhat is exactly 0 in the reference, so
    y = beta and C_g = 0 hold exactly and a relative measure has no scale: they get the bounds of zerovar_fractions."""
    m = np.zeros((c["N"], c["C"]), bool)
    if c["data"] == "zerovar":
        n, g = zerovar_where(c)
        Cg = c["C"] // c["G"]
        m[n, g * Cg:(g + 1) * Cg] = True
    return m


ZV_RSTD = F32(1.0 / np.sqrt(F64(EPS)))          # fl(1 / sqrt(eps)), the root taken in float64 as the kernel takes it


def zerovar_fractions(c, d, fwd, bwd, dgamma_abs):
    """The constant group of a ``zerovar`` case against its derived bounds, as fractions of them; stats must be exact.
    * y: with x = mean, b = fl(beta - mean a) and y = fl(a x + b) are two roundings of quantities below |a x| + |beta|:
      |y - beta| <= 2^-23 (|a x| + |beta|); ReLU moves neither side apart.
    * C_g = rstd sum_c gamma_c dgamma_c / T with every dgamma_c inside kernel_bars.sum_bar of its exact value 0."""
    n, g = zerovar_where(c)
    Cg = c["C"] // c["G"]
    cs = slice(g * Cg, (g + 1) * Cg)
    assert fwd["stats"][n, g, 0] == ZV_CONST and fwd["stats"][n, g, 1] == ZV_RSTD, fwd["stats"][n, g]
    gam, bet = d["gamma"][cs].astype(F64), d["beta"][cs].astype(F64)
    want = np.maximum(bet, 0) if c["relu"] else bet
    bound = 2.0 ** -23 * (np.abs(float(ZV_RSTD) * gam * float(ZV_CONST)) + np.abs(bet))
    out = {"zerovar y": float((np.abs(fwd["y"][n][:, cs].astype(F64) - want) / bound).max())}
    if bwd is not None:
        cg = float(ZV_RSTD) * float((np.abs(gam) * kernel_bars.SUM_REL * dgamma_abs[n, cs]).sum()) / (c["V"] * Cg)
        out["zerovar C_g"] = float(np.abs(bwd["bcoef"][n, 2, cs].astype(F64)).max() / cg)
    return out


def pivot_survey(ks=PIVOT_KS, acc=F64):
    """[(k, RB, emulated rstd error, float32 restatement's, half of the bar)] over the four chunk forms."""
    rows = []
    for k in ks:
        for rb in sorted(CHUNK_SHAPES):
            c = by_name("pivot_k%d_rb%d" % (k, rb))
            d = inputs(c)
            r64 = forward_ref(d["x"], d["gamma"], d["beta"], c["G"], 0, F64)["stats"][..., 1]
            r32 = forward_ref(d["x"], d["gamma"], d["beta"], c["G"], 0, F32)["stats"][..., 1]
            emu = emu_forward(d["x"], d["gamma"], d["beta"], c["G"], 0, acc=acc)["stats"][..., 1]
            e, e32 = kernel_bars.mat_err(emu, r64), kernel_bars.mat_err(r32, r64)
            rows.append((k, rb, e, e32, 0.5 * min(max(4.0 * e32, parity_bar.FLOOR), kernel_bars.TOL)))
    return rows
