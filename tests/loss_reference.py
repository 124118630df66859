"""References of the loss kernels (cape_amd/csrc/loss.hip) in plain numpy, dtype-generic, no autograd.  TEST INFRASTRUCTURE ONLY.

The gradients are analytic, so the kernel's convention d||d||/dd = 0 at d = 0 (TF gives NaN there) is part of the reference
instead of a hole in it.

recon_edge    recon = sum w * l(pred - gt) / (N * sum w)          (unweighted: mean over the 3 N V coordinates)
              edge  = mean over (n, e) of || ((pred+ref)_a - (pred+ref)_b) - ((gt+ref)_a - (gt+ref)_b) ||
              dpred = d (w_recon * recon + w_edge * edge) / d pred, the edge part scattered with np.add.at
  definition64   everything in float64 from the fp32 inputs
  rounded64      the two differences the kernel takes -- pred - gt and the edge vector above -- formed in float32, one rounding
                 per operation (adds and subtracts only: nothing there can be contracted or reordered), everything after them in
                 float64.  THE reference of the device in every regime: where the residual is small against the coordinates the
                 float32 differences cancel, and definition64 drifts away from any float32 evaluation by orders of magnitude
  restate32      the kernel in float32, operation for operation (separate multiply and add where the kernel has fmaf): the
                 vertex gather walks graph.vertex_edge_table in its order, the sums are per-thread partials over the grid-stride
                 trips and then a tree.  Its error against rounded64 sets the bar of the gradient.  ``mut``: the corruptions of
                 tests/test_loss_cases_host.py
gan_bce       gan_g, gan_d, scale * both and the two gradients [Nf + Nr, M] as documented above gan_bce_kernel; float64 from
              bce = max(x, 0) - x t + log1p(exp(-|x|)) and sigmoid - t, float32 with the kernel's single exponential and its two
              sigmoid branches.  The targets are the kernel's in both: t_real = float32(1) - float32(smooth), t_fake = float32(smooth)"""
import types

import numpy as np

F32, F64 = np.float32, np.float64
KINDS = ("l1", "huber", "l2")
HUBER_DELTA = F32(0.1)
LB, GRID_CAP, GAN_LB = 256, 1024, 1024          # csrc/loss.hip: block size, cape_grid_blocks' cap, the GAN kernel's one block


def pointwise(d, kind, delta=HUBER_DELTA, sign0=0.0):
    """(l(d), l'(d)) in d's dtype.  ``sign0``: the l1 slope at d == 0 (0: TF's sign, the kernel's)."""
    dt = d.dtype.type
    if kind == "l1":
        s = np.sign(d)
        if sign0:
            s = np.where(d == 0, dt(sign0), s)
        return np.abs(d), s.astype(d.dtype)
    if kind == "huber":
        th, a = dt(delta), np.abs(d)
        return np.where(a <= th, dt(0.5) * a * a, th * a - dt(0.005)).astype(d.dtype), np.clip(d, -th, th)
    assert kind == "l2", kind
    return d * d, dt(2) * d


def _differences(pred, gt, ref, edges, dtype, rounded, no_ref=False):
    """(pred - gt [N, V, 3], edge vectors [N, E, 3]) in ``dtype``; ``rounded``: formed in float32 first, in the kernel's order."""
    pred, gt, ref = (np.asarray(v) for v in (pred, gt, ref))
    assert pred.dtype == gt.dtype == ref.dtype == F32 and pred.shape == gt.shape and ref.shape == pred.shape[1:]
    w = F32 if rounded else dtype
    p, g, r = pred.astype(w), gt.astype(w), ref.astype(w)[None]
    a, b = np.asarray(edges)[:, 0], np.asarray(edges)[:, 1]
    P, G = (p, g) if no_ref else (p + r, g + r)
    dv = (P[:, a] - P[:, b]) - (G[:, a] - G[:, b])
    return (p - g).astype(dtype), dv.astype(dtype)


def _units(dv):
    ln = np.sqrt(dv[..., 0] * dv[..., 0] + dv[..., 1] * dv[..., 1] + dv[..., 2] * dv[..., 2])
    with np.errstate(divide="ignore"):
        inv = np.where(ln > 0, dv.dtype.type(1) / ln, dv.dtype.type(0)).astype(dv.dtype)
    return ln, dv * inv[..., None]


def weight_sum(weights):
    """sum of one sample's weights as the wrapper forms it (float64 of the fp32 values)"""
    return float(np.asarray(weights, F32).astype(F64).sum())


def _result(**kw):
    return types.SimpleNamespace(**kw)


def _recon_edge64(pred, gt, ref, edges, w_recon, w_edge, weights, kind, rounded, delta):
    N, V, _ = pred.shape
    E = len(edges)
    d, dv = _differences(pred, gt, ref, edges, F64, rounded)
    l, dl = pointwise(d, kind, delta)
    if weights is None:
        assert kind == "l1", "the unweighted kernel is l1 only"
        w, inv_v = np.ones((V, 3)), 1.0 / (3.0 * N * V)
    else:
        w = np.asarray(weights, F32).astype(F64)
        inv_v = 1.0 / (N * weight_sum(weights))
    wr, we = float(F32(w_recon)), float(F32(w_edge))
    terms = w[None] * l
    ln, unit = _units(dv)
    scat = np.zeros((N, V, 3))
    for n in range(N):
        np.add.at(scat[n], edges[:, 0], unit[n])
        np.add.at(scat[n], edges[:, 1], -unit[n])
    return _result(recon=terms.sum() * inv_v, edge=ln.sum() / (N * E), dpred=wr * inv_v * (w[None] * dl) + we / (N * E) * scat,
                   recon_terms=terms * inv_v, edge_terms=ln / (N * E), recon_abs=np.abs(terms).sum() * inv_v,
                   edge_abs=np.abs(ln).sum() / (N * E))


def definition64(pred, gt, ref, edges, w_recon, w_edge, weights=None, kind="l1", delta=HUBER_DELTA):
    return _recon_edge64(pred, gt, ref, edges, w_recon, w_edge, weights, kind, False, delta)


def rounded64(pred, gt, ref, edges, w_recon, w_edge, weights=None, kind="l1", delta=HUBER_DELTA):
    return _recon_edge64(pred, gt, ref, edges, w_recon, w_edge, weights, kind, True, delta)


def recon_edge(pred, gt, ref, edges, w_recon, w_edge, weights=None, kind="l1", dtype=F64):
    """the definition in float64, the kernel's operations in float32"""
    fn = definition64 if dtype == F64 else restate32
    return fn(pred, gt, ref, edges, w_recon, w_edge, weights, kind)


def recon_scale32(N, V, w_recon, weights=None):
    """(cr, inv_v) of the kernel: the float32 scale of the point-wise slope, the reciprocal that turns the vertex sum into recon"""
    if weights is None:
        nm3 = F32(N) * F32(V) * F32(3.0)
        return F32(w_recon) / nm3, F32(1.0) / nm3
    inv = F32(1.0 / (N * weight_sum(weights)))
    return F32(w_recon) * inv, inv


def _grid_sum32(terms, rows):
    """float32 sum of terms [rows, k] as the two passes take it: each thread adds its rows' terms over the grid-stride trips,
    then a tree over the threads of a block and over the blocks"""
    blocks = min((rows + LB - 1) // LB, GRID_CAP)
    threads = blocks * LB
    acc = np.zeros(threads, F32)
    for start in range(0, rows, threads):
        part = terms[start:start + threads]
        for k in range(part.shape[1]):
            acc[:len(part)] = acc[:len(part)] + part[:, k]
    return np.sum(np.sum(acc.reshape(blocks, LB), axis=1, dtype=F32), dtype=F32)


def restate32(pred, gt, ref, edges, w_recon, w_edge, weights=None, kind="l1", mut=None):
    from cape_amd.graph import vertex_edge_table
    mut = mut or {}
    N, V, _ = pred.shape
    E = len(edges)
    d, dv = _differences(pred, gt, ref, edges, F32, True, no_ref=mut.get("no_ref", False))
    ln, unit = _units(dv)
    if "zero_unit" in mut:                                         # what the unit vector of a zero-length edge is taken to be
        unit[ln == 0] = np.asarray(mut["zero_unit"], F32)
    l, dl = pointwise(d, kind, sign0=mut.get("sign0", 0.0))
    cr, inv_v = recon_scale32(N, V, w_recon, weights)
    if weights is None:
        assert kind == "l1", "the unweighted kernel is l1 only"
        terms, g = l, cr * dl
    else:
        w = np.asarray(weights, F32)[None]
        terms, g = w * l, cr * (w * dl)
    g = np.ascontiguousarray(g, F32)
    ce = F32(w_edge) / (F32(N) * F32(mut.get("ce_edges", E)))
    vptr, vidx = mut["table"] if "table" in mut else vertex_edge_table(edges, V)
    deg = np.diff(vptr)
    for t in range(int(deg.max()) if len(deg) else 0):             # the gather, every vertex's list in the table's order
        vs = np.nonzero(deg > t)[0]
        code = vidx[vptr[vs] + t]
        sg = np.where(code & 1, -ce, ce).astype(F32)
        g[:, vs] = g[:, vs] + sg[None, :, None] * unit[:, code >> 1]
    terms, lens = terms.reshape(N * V, 3).astype(F32), ln.reshape(N * E, 1)
    limit = mut.get("rows_limit")                                  # a grid-stride loop that never takes its second trip
    if limit is not None:
        g.reshape(N * V, 3)[limit:] = 0
        terms, lens = terms[:limit], lens[:limit]
    s, t = _grid_sum32(terms, len(terms)), _grid_sum32(lens, len(lens))
    return _result(recon=s * inv_v, edge=t * (F32(1.0) / (F32(N) * F32(E))), dpred=g, cr=cr, ce=ce)


def recon_slope32(pred, gt, w_recon, weights=None, kind="l1"):
    """cr * dl, cr * (w * dl): the float32 value of the gradient where no edge contributes"""
    N, V, _ = pred.shape
    _, dl = pointwise(np.asarray(pred, F32) - np.asarray(gt, F32), kind)
    cr, _ = recon_scale32(N, V, w_recon, weights)
    return (cr * dl if weights is None else cr * (np.asarray(weights, F32)[None] * dl)).astype(F32)


def total64(recon, edge, w_recon, w_edge, term_a=None, w_a=0.0, term_b=None):
    """(total, sum |terms|) in float64 from float32 values: what loss_final_kernel adds up"""
    terms = [float(F32(w_recon)) * float(recon), float(F32(w_edge)) * float(edge)]
    if term_a is not None:
        terms.append(float(F32(w_a)) * float(term_a))
    if term_b is not None:
        terms.append(float(term_b))
    return sum(terms), sum(abs(t) for t in terms)


# ---- adversarial losses ----------------------------------------------------------------------------------------------------

def gan_targets(smooth, dtype):
    s = F32(smooth)
    return dtype(F32(1.0) - s), dtype(s)


def gan_bce(fake, real, smooth, scale, dtype=F64, mut=None):
    """fake [Nf, M], real [Nr, M] fp32 logits.  float32: the kernel's operations; float64: the definition."""
    mut = mut or {}
    fake, real = np.asarray(fake), np.asarray(real)
    assert fake.dtype == real.dtype == F32 and fake.ndim == real.ndim == 2 and fake.shape[1] == real.shape[1]
    Nf, Nr, M = fake.shape[0], real.shape[0], fake.shape[1]
    tr, tf = gan_targets(smooth, dtype)
    xf, xr = fake.astype(dtype), real.astype(dtype)

    def parts(x):
        e = np.exp(-np.abs(x))
        sp = np.maximum(x, dtype(0)) + (e if mut.get("log1p_as_e") else np.log1p(e))
        if dtype == F32:
            neg = dtype(1) / (dtype(1) + e) if mut.get("neg_branch_pos") else e / (dtype(1) + e)
            sig = np.where(x >= 0, dtype(1) / (dtype(1) + e), neg)
        else:
            sig = 0.5 * (1.0 + np.tanh(0.5 * x))
        return sp.astype(dtype), sig.astype(dtype)

    spf, sigf = parts(xf)
    spr, sigr = parts(xr)
    bg, bdf, bdr = spf - xf * tr, spf - xf * tf, spr - xr * tr
    if dtype == F32:
        nf, nr = F32(Nf) * F32(M), F32(Nr) * F32(M)
        if mut.get("swap_div"):
            nf, nr = nr, nf
        cf, cr = F32(scale) / nf, F32(scale) / nr

        def total(b):                                              # one block: strided per-thread sums, then a tree
            flat = b.reshape(-1)
            acc = np.zeros(GAN_LB, F32)
            for start in range(0, len(flat), GAN_LB):
                part = flat[start:start + GAN_LB]
                acc[:len(part)] = acc[:len(part)] + part
            return np.sum(acc, dtype=F32)
        g, d = total(bg) / nf, total(bdr) / nr + total(bdf) / nf
        sc = F32(scale)
    else:
        nf, nr = float(Nf * M), float(Nr * M)
        cf, cr = float(F32(scale)) / nf, float(F32(scale)) / nr
        g, d = bg.sum() / nf, bdr.sum() / nr + bdf.sum() / nf
        sc = float(F32(scale))
    ga = np.concatenate([cf * (sigf - tr), np.zeros((Nr, M), dtype)]).astype(dtype)
    if mut.get("ga_real_nonzero"):
        ga[Nf:] = cr * (sigr - tr)
    gb = np.concatenate([cf * (sigf - tf), cr * (sigr - tr)]).astype(dtype)
    return _result(gan_g=g, gan_d=d, scaled_g=sc * g, scaled_d=sc * d, ga=ga, gb=gb,
                   g_abs=float(np.abs(bg.astype(F64)).sum() / (Nf * M)),
                   d_abs=float(np.abs(bdr.astype(F64)).sum() / (Nr * M) + np.abs(bdf.astype(F64)).sum() / (Nf * M)))
