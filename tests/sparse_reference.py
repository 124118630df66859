"""Synthetic sparse operators and restatements of the streaming sparse-operator entry points (csrc/sparse.hip: cape_spmm,
cape_spmm_multi[_actgrad], cape_bwd_prep_spmm, cape_spmm_multi_prep, cape_spmm_combine) for tests/test_gpu_sparse.py and
tests/test_sparse_reference_host.py.  TEST INFRASTRUCTURE ONLY, no GPU.

Every restatement takes ``prec``: np.float64 evaluates the formula written in include/cape_hip.h; np.float32 accumulates in the
kernels' own order -- the entries of a row in CSR order with one fused multiply-add each, the terms in order, ``scale`` after
the gather, the rank-1 terms after the operator terms.  (fmaf is restated as float32(float64(a) * float64(b) + float64(c)): the
product of two float32 is exact in float64.)  Operator values and inputs are float32-representable float64 arrays, so the
float64 result is the exact arithmetic of what the device holds."""
import numpy as np
import scipy.sparse as sp

FAMILIES = ("ell4", "ell8", "ell12", "csr", "zeros_inside", "zero_group")
# family -> (largest drawn degree, degrees that must occur, expected DeviceCSR.ell_w)
_SPEC = {
    "ell4": (4, [4, 3, 2, 1, 0], 4),
    "ell8": (8, [4, 5, 8, 0, 0], 8),
    "ell12": (12, [8, 9, 12, 0, 0, 0], 12),
    "csr": (12, [8, 9, 12, 0, 0, 0, 13, 40], 0),
    "zeros_inside": (12, [8, 9, 12, 0, 0, 0], 12),
    "zero_group": (12, [8, 9, 12, 0, 0, 0, 10], 0),
}


def expected_ell_w(family):
    return _SPEC[family][2]


def f32(a):
    """float32-representable float64 copy of ``a``."""
    return np.asarray(a, np.float32).astype(np.float64)


def synth_operator(rng, rows, cols, family):
    """scipy CSR (float64, float32-representable values, columns sorted and distinct inside a row) with the degrees of ``family``;
    column 0 and column cols-1 are both used; stored zeros are kept."""
    hi, need, _ = _SPEC[family]
    need = [min(d, cols) for d in need]         # (a square 37-row operator: its long row is 37 entries, not 40)
    assert rows >= len(need) + 4 and cols >= 13
    deg = rng.integers(0, hi + 1, size=rows)
    where = rng.choice(np.arange(1, rows - 1), size=len(need), replace=False)
    deg[where] = need
    if family == "ell4":
        deg[0] = deg[-1] = 0
    else:
        deg[-1] = max(deg[-1], 2)               # the row the dead lanes of a tail block are clamped to gathers something
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = np.concatenate([np.sort(rng.choice(cols, size=d, replace=False)) for d in deg] + [np.zeros(0, np.int64)]).astype(np.int64)
    data = f32(rng.standard_normal(indices.size) * np.exp2(rng.integers(-3, 3, size=indices.size)))
    data[data == 0] = 1.0
    r2 = int(np.flatnonzero(deg >= 2)[0])       # one row reaches both ends of the input
    indices[indptr[r2]], indices[indptr[r2 + 1] - 1] = 0, cols - 1
    indices[indptr[r2] + 1:indptr[r2 + 1] - 1] = np.sort(rng.choice(np.arange(1, cols - 1), size=deg[r2] - 2, replace=False))
    if family == "zeros_inside":                # one stored 0.0 in a group of four that keeps another non-zero entry
        for r in np.flatnonzero(deg >= 2)[::2]:
            j = int(rng.integers(0, deg[r]))
            lo = 4 * (j // 4)
            if min(deg[r], lo + 4) - lo >= 2:
                data[indptr[r] + j] = 0.0
    if family == "zero_group":                  # stored entries 4..7 all zero in front of a non-zero entry 8
        r = int(where[_SPEC[family][1].index(10)])
        data[indptr[r] + 4:indptr[r] + 8] = 0.0
    return sp.csr_matrix((data, indices, indptr), shape=(rows, cols))


def degrees(S):
    return np.diff(S.indptr)


def padded(S):
    """(cols [rows, w], vals [rows, w]) with w = the longest row; slots past a row's end are (0, 0.0)."""
    deg = degrees(S)
    w = max(int(deg.max()), 1)
    cols = np.zeros((S.shape[0], w), np.int64)
    vals = np.zeros((S.shape[0], w), np.float64)
    rr = np.repeat(np.arange(S.shape[0]), deg)
    slot = np.arange(S.nnz) - np.repeat(S.indptr[:-1], deg)
    cols[rr, slot], vals[rr, slot] = S.indices, S.data
    return cols, vals


def fma(a, b, c, prec):
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    return (a * b + c).astype(prec).astype(np.float64)


def rnd(a, prec):
    return np.asarray(a, np.float64).astype(prec).astype(np.float64)


def gather(S, x, prec):
    """acc[n, r, :] = sum_e vals[e] * x[n, colidx[e], :], entries in CSR order, one fma each.  x: [N, Mi, C]."""
    cols, vals = padded(S)
    deg = degrees(S)
    acc = np.zeros((x.shape[0], S.shape[0], x.shape[2]))
    for j in range(int(deg.max())):
        sel = np.flatnonzero(deg > j)                       # (the rows that still have an entry: a slot past the end adds nothing)
        acc[:, sel] = fma(vals[None, sel, j, None], x[:, cols[sel, j], :], acc[:, sel], prec)
    return acc


def rowbound(y):
    return np.abs(y).max(axis=2)


def spmm(S, x, alpha=1.0, z=None, beta=0.0, prec=np.float64):
    """y = alpha * S x + beta * z (cape_spmm): the gather, then ``* alpha``, then one fma with z."""
    acc = rnd(gather(S, x, prec) * np.float64(np.float32(alpha)), prec)
    if z is not None:
        acc = fma(np.float64(np.float32(beta)), z, acc, prec)
    return acc


def spmm_multi(terms, sum_mode, prec=np.float64):
    """``terms``: [(S or None = identity, x, scale)].  Separate mode: [scale_k * S_k x_k]; sum mode: their sum, terms in order."""
    outs = []
    for S, x, scale in terms:
        acc = x.copy() if S is None else gather(S, x, prec)
        outs.append(rnd(acc * np.float64(np.float32(scale)), prec))
    if not sum_mode:
        return outs
    tot = np.zeros_like(outs[0])
    for o in outs:
        tot = rnd(tot + o, prec)
    return tot


def act_grad_from_out(y, act):
    """include/cape_hip.h / csrc/common.h cape_act_grad_from_out: 1 where the OUTPUT is > 0, else the slope (0.2 leaky, 0 relu);
    an output of +0.0 or -0.0 is not > 0."""
    return np.where(np.asarray(y) > 0, 1.0, {"leaky": np.float64(np.float32(0.2)), "relu": 0.0}[act])


def actgrad(terms, act_x, act, prec=np.float64):
    """cape_spmm_multi_actgrad: (y, dbias) with y = (sum_k scale_k S_k x_k) * act'(act_x), dbias[c] = sum_{n,r} y (float64 sum)."""
    y = rnd(spmm_multi(terms, True, prec) * act_grad_from_out(act_x, act), prec)
    return y, y.sum(axis=(0, 1))


def abs_terms(terms):
    """sum_k |scale_k| |S_k| |x_k|: the sum of the absolute values of the products a summed application adds up -- the scale of
    its rounding error, whatever cancels inside a row (sum_bar's condition-aware scale)."""
    tot = 0.0
    for S, x, scale in terms:
        a = np.abs(x) if S is None else gather(abs(S).tocsr(), np.abs(x), np.float64)
        tot = tot + abs(np.float64(np.float32(scale))) * a
    return tot


def block_partials(y, cq, rpb=1):
    """The partial sums one launch leaves for cape_bwd_prep_finalize, reduced in float64: [N, chunks, C] where chunk t holds the
    rows of the work items [t * rpb * 256, (t + 1) * rpb * 256) -- a work item is (row, one of the cq lanes of that row)."""
    N, Mo, C = y.shape
    rows = rpb * 256 // cq
    chunks = (Mo + rows - 1) // rows
    out = np.zeros((N, chunks, C))
    for t in range(chunks):
        out[:, t] = y[:, t * rows:(t + 1) * rows].sum(axis=1)
    return out


def sign_words(bits):
    """[N, M, F] booleans -> [N, M, ceil(F / 32)] uint32 words, bit b of word w = channel 32 w + b."""
    N, M, F = bits.shape
    words = np.zeros((N, M, (F + 31) // 32), dtype=np.uint32)
    for b in range(32):
        sl = bits[:, :, b::32]
        words[:, :, :sl.shape[2]] |= sl.astype(np.uint32) << np.uint32(b)
    return words


def unpack_words(words, F):
    w = np.asarray(words).view(np.uint32).astype(np.int64)
    return (((w[..., None] >> np.arange(32)) & 1).reshape(w.shape[0], w.shape[1], -1)[:, :, :F]) == 1


def bwd_prep_spmm(S, g, bits, rowscale, R, rg, prec=np.float64):
    """cape_bwd_prep_spmm: dz = bit ? g : 0;  t1 = S dz;  dcoef[n, j] = sum_r rowscale[j, r] dz[n, r] (j < R);
    dcoef_g[n] = sum_r rowscale[rg, r] g[n, r].  Returns dict with the sums in float64 and the sums of |terms| next to them."""
    dz = np.where(bits, g, 0.0)
    out = dict(dz=dz, t1=gather(S, dz, prec))
    if R:
        out["dcoef"] = np.einsum("jr,nrf->njf", rowscale[:R], dz)
        out["dcoef_abs"] = np.einsum("jr,nrf->njf", np.abs(rowscale[:R]), np.abs(dz))
    if rg is not None:
        out["dcoef_g"] = np.einsum("r,nrf->nf", rowscale[rg], g)
        out["dcoef_g_abs"] = np.einsum("r,nrf->nf", np.abs(rowscale[rg]), np.abs(g))
    return out


def multi_prep(Ss, g, bits, masked, prec=np.float64):
    """cape_spmm_multi_prep: T_k = S_k (masked[k] ? dz : g) and the column sums of every T_k (float64) with their sum |terms|."""
    dz = np.where(bits, g, 0.0)
    Ts = [gather(S, dz if m else g, prec) for S, m in zip(Ss, masked)]
    return Ts, [T.sum(axis=1) for T in Ts], [np.abs(T).sum(axis=1) for T in Ts]


def act_fwd(v, act, prec):
    if act == "none":
        return v
    if act == "relu":
        return np.where(v > 0, v, 0.0)
    if act == "leaky":
        return np.where(v > 0, v, rnd(v * np.float64(np.float32(0.2)), prec))
    raise ValueError(act)


def combine(terms, to2=0, rank=None, bias=None, act="none", dual=False, prec=np.float64):
    """cape_spmm_combine.  ``terms``: [(S or None, x, scale)]; ``rank``: (rowscale [R, Mo], coef [N, R, F], rank_to2) or None;
    ``bias``: broadcastable to [N, Mo, F].  Returns (y, a1): single: y = act(a1 + bias);  dual: y = relu(a1) + a2, sign = a1 > 0."""
    a = [None, None]
    for k, (S, x, scale) in enumerate(terms):
        acc = x.copy() if S is None else gather(S, x, prec)
        i = (to2 >> k) & 1
        a[i] = fma(np.float64(np.float32(scale)), acc, 0.0 if a[i] is None else a[i], prec)
    if rank is not None:
        rowscale, coef, rto2 = rank
        for j in range(coef.shape[1]):
            i = (rto2 >> j) & 1
            a[i] = fma(rowscale[j][None, :, None], coef[:, j][:, None, :], 0.0 if a[i] is None else a[i], prec)
    a1 = a[0] if a[0] is not None else np.zeros_like(a[1])
    a2 = a[1] if a[1] is not None else np.zeros_like(a1)
    if dual:
        return rnd(np.where(a1 > 0, a1, 0.0) + a2, prec), a1
    v = a1 if bias is None else rnd(a1 + bias, prec)
    return act_fwd(v, act, prec), a1


def bf16(a):
    """Round to bfloat16 (nearest even), back as float64."""
    import torch
    return torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def spmm_from_gather(acc, alpha, z, beta, prec):
    acc = rnd(acc * np.float64(np.float32(alpha)), prec)
    return acc if z is None else fma(np.float64(np.float32(beta)), z, acc, prec)


def uncertain_signs(a1):
    """Elements whose sign bit is not asserted: neither exactly zero nor at least 1e-4 of the largest magnitude."""
    a = np.abs(a1)
    return (a != 0) & (a < 1e-4 * a.max())


def inputs(rng, *shape):
    """float32-representable normal values with a power-of-two scale per row."""
    return f32(rng.standard_normal(shape) * np.exp2(rng.integers(-3, 3, size=shape[:-1] + (1,))))


def combine_case(family, F, dual, N=3, Mo=37, Mi=53):
    """Inputs of one cape_spmm_combine case (shared by the host and the GPU test): three operators of ``family`` with empty rows,
    two rank-1 terms.  single: everything on acc1, per-vertex bias, leaky.  dual: operator 2 and both rank-1 terms on acc2, so an
    empty row of operators 0 and 1 leaves acc1 exactly 0."""
    rng = np.random.default_rng(1000 * F + 10 * FAMILIES.index(family) + dual)
    S = [synth_operator(rng, Mo, Mi, family) for _ in range(3)]
    if dual:                                                  # one row empty in both acc1 operators
        for k in range(2):
            m, r = S[k], Mo // 2
            keep = np.ones(m.nnz, bool)
            keep[m.indptr[r]:m.indptr[r + 1]] = False
            deg = degrees(m)
            deg[r] = 0
            S[k] = sp.csr_matrix((m.data[keep], m.indices[keep], np.concatenate([[0], np.cumsum(deg)])), shape=m.shape)
    Z = [f32(rng.standard_normal((N, Mi, F))) for _ in range(3)]    # (no row scales: few sums come out near 0 by chance)
    rowscale, coef = f32(rng.standard_normal((2, Mo))), f32(rng.standard_normal((N, 2, F)))
    bias = f32(rng.standard_normal((Mo, F)))
    terms = [(S[k], Z[k], 1.0) for k in range(3)]
    if dual:
        args = dict(terms=terms, to2=0b100, rank=(rowscale, coef, 0b11), dual=True)
    else:
        args = dict(terms=terms, rank=(rowscale, coef, 0), bias=bias[None], act="leaky")
    return dict(N=N, Mo=Mo, Mi=Mi, S=S, Z=Z, rowscale=rowscale, coef=coef, bias=bias, args=args)
