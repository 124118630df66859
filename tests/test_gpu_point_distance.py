"""Mesh-to-scan distance on the device (cape_amd/point_distance.py, csrc/scan/point_distance.hip) against the float64 brute force
of tests/point_distance_reference.py, under tests/parity_bar.py's bar: each measure of the HIP path may be at most 4x the same
measure of the fp32 restatement (the brute force evaluated in float32), floor 4 * 2^-24.  R is the largest absolute coordinate
of a case; every query is compared, none is left out, and no index is compared with the reference's except where a test says so
(where two points tie either is right):
  1 distance        max |sqrt(d2) - sqrt(d2_min(fp64))| / R
  2 index validity  max (sqrt(d2_fp64(q, p[the path's index])) - sqrt(d2_min)) / R
  3 gradient        vertex_err and whole-tensor relative L2 of dq and dp against the float64 formulas ON THE PATH'S OWN INDICES, for
                    a random fp32 seed g
The restatement's own indices are used for its measures."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import point_distance_reference as P    # noqa: E402
import scan_distance_reference as R     # noqa: E402
from parity_bar import check            # noqa: E402

pytestmark = pytest.mark.gpu

PT = 512           # point_distance.hip PT: points per LDS tile          (include/cape_hip.h documents the three)
QB = 512           # point_distance.hip QB: queries per workgroup
SPLIT_MAX = 16     # point_distance.hip SPLIT_MAX
DEV = "cuda"


def vertex_err(a, ref):
    """max per-row error norm / max per-row reference norm, as tests/test_gpu_vertex_normals.py defines it."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, ref.shape[-1])
    r = np.asarray(ref, dtype=np.float64).reshape(-1, ref.shape[-1])
    return np.sqrt(((a - r) ** 2).sum(-1)).max() / max(np.sqrt((r * r).sum(-1)).max(), 1e-30)


def rel_l2(a, ref):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.sqrt(((a - r) ** 2).sum() / max((r * r).sum(), 1e-300))


def _pd():
    from cape_amd.point_distance import PointDistance
    return PointDistance()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a, order="C", copy=True), dtype=dtype).to(DEV)      # a copy: canonical strides for N = 1 too


def _run(pd, q, p, count=None, g=None):
    """forward (+ backward with the seed g) on numpy inputs [N, Q, 3] / [N, M, 3]: dict of numpy outputs."""
    qt, pt = _dev(q), _dev(p)
    with torch.no_grad():
        d2, index = pd.forward(qt, pt, count)
        out = dict(d2=d2.cpu().numpy(), index=index.cpu().numpy())
        if g is not None:
            dq, dp = pd.backward(qt, pt, index, _dev(g), count)
            out.update(dq=dq.cpu().numpy(), dp=dp.cpu().numpy())
    return out


def _reference(q, p):
    """Per query set [Q, 3] and cloud [M, 3] (fp32 inputs): the float64 minimum and the fp32 restatement's own results."""
    i64, d64 = P.brute_force(q, p)
    i32, d32 = P.brute_force(q, p, np.float32)
    return dict(i64=i64, d64=d64, i32=i32, d32=d32)


def _measures(tag, q, p, out, g, ref=None, n=0):
    """Measures 1-3 of sample ``n`` of a run against the references of its queries q [Q, 3] and points p [M, 3]; returns the
    path's measure 2."""
    ref = ref or _reference(q, p)
    Rm = float(max(np.abs(q).max(), np.abs(p).max()))
    index, d2 = out["index"][n].astype(np.int64), out["d2"][n].astype(np.float64)
    assert (index >= 0).all() and (index < len(p)).all() and np.isfinite(d2).all()
    assert (ref["i32"] >= 0).all()
    r64 = np.sqrt(ref["d64"])
    q64, p64, g64 = q.astype(np.float64), p.astype(np.float64), g[n].astype(np.float64)
    errs = [np.abs(np.sqrt(d2) - r64).max() / Rm, (np.sqrt(P.own_d2(q64, p64, index)) - r64).max() / Rm]
    errs32 = [np.abs(np.sqrt(ref["d32"].astype(np.float64)) - r64).max() / Rm,
              (np.sqrt(P.own_d2(q64, p64, ref["i32"])) - r64).max() / Rm]
    names = ["distance", "index validity"]
    dq64, dp64 = P.gradients(q64, p64, index, g64)
    dq64r, dp64r = P.gradients(q64, p64, ref["i32"], g64)
    dq32, dp32 = P.gradients(q, p, ref["i32"], g[n], np.float32)
    for name, mine, want, mine32, want32 in (("dq", out["dq"][n], dq64, dq32, dq64r), ("dp", out["dp"][n], dp64, dp32, dp64r)):
        assert np.isfinite(mine).all()
        errs += [vertex_err(mine, want), rel_l2(mine, want)]
        errs32 += [vertex_err(mine32, want32), rel_l2(mine32, want32)]
        names += [name + " (vertex_err)", name + " (rel L2)"]
    print("%s[%d] R %.2f: " % (tag, n, Rm) + "; ".join("%s %.2e [fp32 %.2e]" % t for t in zip(names, errs, errs32)))
    for name, e, e32 in zip(names, errs, errs32):
        check(tag, name, e, e32)
    return errs[1]


def _small_cloud(x, faces, M, seed):
    """fp32 points around the small mesh: near the surface on both sides, a quarter anywhere in the inflated box."""
    rng = np.random.default_rng(seed)
    p, nrm = R.surface_samples(rng, x.astype(np.float64), faces, M)
    p = p + rng.uniform(-0.05, 0.1, M)[:, None] * nrm
    far = rng.permutation(M)[:M // 4]
    p[far] = rng.uniform(x.min(0) - 0.3, x.max(0) + 0.3, (len(far), 3))
    return p.astype(np.float32)


def _small_batch(N, Q, M, seed):
    """N different small meshes (the octahedron scaled, moved and perturbed per sample): its vertices repeated to Q rows with
    a perturbation per row as queries [N, Q, 3], a cloud [N, M, 3] around each."""
    rng = np.random.default_rng(seed)
    x0, f0 = R.octahedron()
    qs, ps = [], []
    for n in range(N):
        x = (x0 * rng.uniform(0.5, 1.5) + 0.01 * rng.standard_normal(x0.shape) + rng.uniform(-0.5, 0.5, 3)).astype(np.float32)
        rows = x[np.arange(Q) % len(x)].astype(np.float64) + 0.01 * rng.standard_normal((Q, 3))
        qs.append(rows.astype(np.float32))
        ps.append(_small_cloud(x, f0, M, seed + 100 + n))
    return np.stack(qs), np.stack(ps)


def _check_case(tag, qs, ps, seed=0):
    g = np.random.default_rng(seed).standard_normal(qs.shape[:2]).astype(np.float32)
    out = _run(_pd(), qs, ps, None, g)
    for n in range(qs.shape[0]):
        _measures(tag, qs[n], ps[n], out, g, n=n)
    return out


# ---- tile edges --------------------------------------------------------------------------------------------------------------

def test_plan_is_what_the_header_documents():
    pd = _pd()
    assert pd.plan(1, QB, SPLIT_MAX * PT) == (SPLIT_MAX, PT, QB)
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    assert "plan[1] = points per LDS tile (%d); plan[2] = queries per workgroup (%d)" % (PT, QB) in hdr
    assert "at most %d and at most the number of point tiles" % SPLIT_MAX in hdr


@pytest.mark.parametrize("M,Q,N", [(1, 1, 1), (PT, QB - 1, 1), (PT + 1, QB, 3), (128, QB + 1, 3), (PT + 1, 1, 3)])
def test_tile_edges_on_the_small_mesh(M, Q, N):
    qs, ps = _small_batch(N, Q, M, seed=M + Q)
    assert _pd().plan(N, Q, M)[1:] == (PT, QB)
    _check_case("point_small_M%d_Q%d_N%d" % (M, Q, N), qs, ps)


def test_point_split_factors_give_the_same_bits():
    """The split is a function of the sizes: one sample of 16 point tiles with QB, 128 QB and 600 QB queries selects 16, 8 and 1
    parts; the first QB queries are the same in all three and must come back bit for bit, and be right."""
    M = SPLIT_MAX * PT
    pd = _pd()
    sizes = (QB, 128 * QB, 600 * QB)
    assert [pd.plan(1, Q, M)[0] for Q in sizes] == [SPLIT_MAX, 8, 1]
    q0, p = _small_batch(1, QB, M, seed=8)
    rng = np.random.default_rng(9)
    q = (rng.standard_normal((1, sizes[-1], 3)) * 0.4).astype(np.float32)
    q[0, :QB] = q0[0]
    outs = [_run(pd, q[:, :Q], p) for Q in sizes]
    for k in ("index", "d2"):
        assert outs[0][k].tobytes() == outs[1][k][:, :QB].tobytes() == outs[2][k][:, :QB].tobytes(), k
        assert outs[1][k].tobytes() == outs[2][k][:, :sizes[1]].tobytes(), k
    g = np.random.default_rng(1).standard_normal((1, QB)).astype(np.float32)
    full = _run(pd, q[:, :QB], p, None, g)
    assert full["d2"].tobytes() == outs[0]["d2"].tobytes() and full["index"].tobytes() == outs[0]["index"].tobytes()
    _measures("point_split", q[0, :QB], p[0], full, g)


# ---- counts, wide rows -------------------------------------------------------------------------------------------------------

def test_ragged_counts():
    M, Q = 40, 70
    qs, ps = _small_batch(4, Q, M, seed=2)
    count = np.array([M, 1, 0, 7], np.int32)
    for n in range(4):
        ps[n, count[n]:] = np.nan                          # padding is never read
    pd = _pd()
    g = np.random.default_rng(3).standard_normal((4, Q)).astype(np.float32)
    out = _run(pd, qs, ps, count, g)
    for n in range(4):
        c = count[n]
        assert not out["dp"][n, c:].any() and np.isfinite(out["dp"][n]).all()
        alone = _run(pd, qs[n:n + 1], ps[n:n + 1, :max(c, 1)], None if c else np.zeros(1, np.int32), g[n:n + 1])
        for k in ("index", "d2", "dq"):
            assert out[k][n].tobytes() == alone[k][0].tobytes(), (n, k)
        assert out["dp"][n, :c].tobytes() == alone["dp"][0, :c].tobytes(), n
        if c:
            assert (out["index"][n] < c).all()
            sub = dict(index=out["index"][n:n + 1], d2=out["d2"][n:n + 1], dq=out["dq"][n:n + 1], dp=out["dp"][n:n + 1, :c])
            _measures("point_ragged", qs[n], ps[n, :c], sub, g[n:n + 1])
    assert (out["index"][2] == -1).all() and np.isnan(out["d2"][2]).all() and not out["dq"][2].any()
    # count on the device, and count = None against a full count
    dev_count = _run(pd, qs, ps, torch.as_tensor(count).to(DEV), g)
    full = np.nan_to_num(ps)
    a, b = _run(pd, qs, full, None, g), _run(pd, qs, full, np.full(4, M, np.int32), g)
    for k in out:
        assert out[k].tobytes() == dev_count[k].tobytes() and a[k].tobytes() == b[k].tobytes(), k
    with pytest.raises(ValueError):
        pd.forward(_dev(qs), _dev(full), np.array([M, 1, 0, M + 1]))


def test_wide_rows():
    N, M, Q = 2, 37, 45
    qs, ps = _small_batch(N, Q, M, seed=4)
    pd = _pd()
    g = np.random.default_rng(5).standard_normal((N, Q)).astype(np.float32)
    want = _run(pd, qs, ps, None, g)
    q4, p5 = np.full((N, Q, 4), np.nan, np.float32), np.full((N, M, 5), np.nan, np.float32)
    q4[:, :, :3], p5[:, :, :3] = qs, ps
    qt, pt = _dev(q4)[:, :, :3], _dev(p5)[:, :, :3]
    dq4, dp6 = torch.full((N, Q, 4), 7.0, device=DEV), torch.full((N, M, 6), 7.0, device=DEV)
    with torch.no_grad():
        d2, index = pd.forward(qt, pt)
        pd.backward(qt, pt, index, _dev(g), dq=dq4[:, :, :3], dp=dp6[:, :, :3])
    got = dict(d2=d2, index=index, dq=dq4[:, :, :3], dp=dp6[:, :, :3])
    for k, v in got.items():
        assert v.cpu().numpy().tobytes() == want[k].tobytes(), k
    assert (dq4[:, :, 3] == 7.0).all() and (dp6[:, :, 3:] == 7.0).all()                  # padding never written


# ---- non-finite input --------------------------------------------------------------------------------------------------------

def test_non_finite_points_never_win():
    M, Q = PT + 10, 130
    qs, ps = _small_batch(1, Q, M, seed=6)
    pd = _pd()
    g = np.random.default_rng(7).standard_normal((1, Q)).astype(np.float32)
    base = _run(pd, qs, ps, None, g)
    at = np.array([5, PT - 1])                            # rows 5 and PT of the new cloud: the second opens the second tile
    rows = np.array([[0.1, np.nan, 0.2], [np.inf, 0.0, 0.0]], np.float32)
    bad = np.insert(ps[0], at, rows, axis=0)[None]
    pos = at + np.arange(2)
    assert not np.isfinite(bad[0, pos]).all(1).any() and np.isfinite(np.delete(bad[0], pos, 0)).all()
    out = _run(pd, qs, bad, None, g)
    assert not np.isin(out["index"], pos).any()
    shifted = out["index"] - (out["index"] > pos[0]) - (out["index"] > pos[1])
    assert np.array_equal(shifted, base["index"])
    for k in ("d2", "dq"):
        assert out[k].tobytes() == base[k].tobytes(), k
    assert np.delete(out["dp"][0], pos, 0).tobytes() == base["dp"][0].tobytes() and not out["dp"][0, pos].any()
    # nothing but NaN
    none = _run(pd, qs, np.full_like(ps, np.nan), None, g)
    assert (none["index"] == -1).all() and np.isnan(none["d2"]).all() and not none["dq"].any() and not none["dp"].any()


def test_a_query_with_a_non_finite_coordinate():
    M, Q = 90, 130
    qs, ps = _small_batch(1, Q, M, seed=8)
    pd = _pd()
    g = np.random.default_rng(9).standard_normal((1, Q)).astype(np.float32)
    bad = qs.copy()
    bad[0, 70, 1] = np.nan
    bad[0, 5, 2] = np.inf
    out = _run(pd, bad, ps, None, g)
    for j in (70, 5):
        assert out["index"][0, j] == -1 and np.isnan(out["d2"][0, j]) and not out["dq"][0, j].any()
    g0 = g.copy()
    g0[0, [70, 5]] = 0.0                                   # the same sums without the two: they add nothing to dp
    base = _run(pd, qs, ps, None, g0)
    keep = np.setdiff1d(np.arange(Q), (70, 5))            # the neighbours in the wave are unaffected
    for k in ("index", "d2", "dq"):
        assert out[k][0, keep].tobytes() == base[k][0, keep].tobytes(), k
    assert np.isfinite(out["dp"]).all() and out["dp"].tobytes() == base["dp"].tobytes()


# ---- ties, determinism -------------------------------------------------------------------------------------------------------

def test_ties_and_determinism():
    rng = np.random.default_rng(10)
    M, Q = 2 * (PT + 30), 200                              # the second copy lies in the tiles after the first's
    qs, half = _small_batch(2, Q, M // 2, seed=11)
    ps = np.concatenate([half, half], 1)                  # rows i and i + M / 2 identical: identical fp32 values, whatever the rounding
    qs[:, 100:] = half[:, :100]                           # queries that are cloud points themselves
    pd = _pd()
    g = rng.standard_normal((2, Q)).astype(np.float32)
    out = _run(pd, qs, ps, None, g)
    assert (out["index"] >= 0).all() and (out["index"] < M // 2).all()
    assert not out["d2"][:, 100:].any()                   # exactly zero
    for n in range(2):
        _measures("point_doubled", qs[n], ps[n], out, g, n=n)
    again = _run(pd, qs, ps, None, g)
    swapped = _run(pd, qs[::-1], ps[::-1], None, g[::-1])
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k
        assert out[k].tobytes() == swapped[k][::-1].tobytes(), k
    # mirrored ties: queries on the plane x = 0 of a cloud that is symmetric in it -- the fp32 values of a pair are equal, but
    # which of the two comes first is the cloud's order, so these are held to the measures only
    side = rng.uniform(0.1, 0.6, (60, 3)).astype(np.float32)
    side[:, 1:] -= 0.3
    cloud = np.concatenate([side, side * np.array([-1, 1, 1], np.float32)])[rng.permutation(120)][None]
    qm = rng.uniform(-0.5, 0.5, (1, 80, 3)).astype(np.float32)
    qm[0, :, 0] = 0.0
    gm = rng.standard_normal((1, 80)).astype(np.float32)
    _measures("point_mirrored", qm[0], cloud[0], _run(pd, qm, cloud, None, gm), gm)


# ---- the template ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _template_reference(seed, shift, M):
    x, _, p = R.template_case(seed, shift, M)
    ref = _reference(x, p)
    for a in (x, p) + tuple(ref.values()):
        a.setflags(write=False)
    return x, p, ref


@pytest.mark.parametrize("seed,shift", [(3, 0.0), (5, 3.0)])
def test_template_recipes(seed, shift):
    """The 6890 template vertices against the recipe's 2049 points; shift 3.0 is the translated body, which the difference form
    searches in raw coordinates without loss.  At shift 0 the reference arithmetic picks the float64 winner for every vertex
    (checked on the CPU when the kernel was specified), so measure 2 must be exactly 0 there."""
    x, p, ref = _template_reference(seed, shift, 2049)
    g = np.random.default_rng(13).standard_normal((1, len(x))).astype(np.float32)
    out = _run(_pd(), x[None], p[None], None, g)
    validity = _measures("point_template_shift%g" % shift, x, p, out, g, ref=ref)
    if shift == 0.0:
        assert validity == 0.0


# ---- autograd ----------------------------------------------------------------------------------------------------------------

def test_diff_matches_forward_and_the_backward_entry():
    N, M, Q = 2, 50, 60
    qs, ps = _small_batch(N, Q, M, seed=14)
    pd = _pd()
    g = np.random.default_rng(15).standard_normal((N, Q)).astype(np.float32)
    want = _run(pd, qs, ps, None, g)
    qt, pt = _dev(qs).requires_grad_(True), _dev(ps).requires_grad_(True)
    d2, index = pd.diff(qt, pt, return_selection=True)
    assert d2.requires_grad and not index.requires_grad
    d2.backward(_dev(g))
    got = dict(d2=d2.detach(), index=index, dq=qt.grad, dp=pt.grad)
    for k, v in got.items():
        assert v.cpu().numpy().tobytes() == want[k].tobytes(), k
    # only the queries: no dp is produced; a loss downstream of d2
    q2, p2 = _dev(qs).requires_grad_(True), _dev(ps)
    (pd.diff(q2, p2) * _dev(g)).sum().backward()
    assert q2.grad.cpu().numpy().tobytes() == want["dq"].tobytes() and p2.grad is None
    with torch.no_grad():
        dq, dp = pd.backward(_dev(qs), p2, index, _dev(g), want_dp=False)
    assert dp is None and dq.cpu().numpy().tobytes() == want["dq"].tobytes()
    # only the points
    p3 = _dev(ps).requires_grad_(True)
    pd.diff(_dev(qs), p3).backward(_dev(g))
    assert p3.grad.cpu().numpy().tobytes() == want["dp"].tobytes()
    with pytest.raises(RuntimeError):
        pd.forward(qt, _dev(ps))
    with pytest.raises(RuntimeError):
        pd.forward(_dev(qs), pt)


def test_gradient_against_float64_finite_differences():
    """8 queries 0.05 from one point each of a grid with spacing 0.5 (every other point at least 0.45 away): the selection is
    unique and stable under the perturbation.  There d2 is a quadratic, so central differences of the float64 reference with
    h = 1e-5 are exact up to 1e-16 / h, about 1e-10 of the gradient; the device's fp32 results carry a few 2^-24.  Held to 1e-5
    of the largest gradient entry (the argument of tests/test_gpu_scan_distance.py's finite-difference test)."""
    rng = np.random.default_rng(16)
    grid = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(2), indexing="ij"), -1).reshape(-1, 3) * 0.5 + 0.1
    p = grid.astype(np.float32).astype(np.float64)
    pick = rng.permutation(len(p))[:8]
    u = rng.standard_normal((8, 3))
    q = (p[pick] + 0.05 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    i64, _ = P.brute_force(q, p)
    assert np.array_equal(i64, pick)
    dist = np.sqrt(((q[:, None] - p[None]) ** 2).sum(-1))
    dist[np.arange(8), pick] = np.inf
    assert dist.min() >= 0.2
    g = rng.uniform(0.5, 1.5, 8).astype(np.float32)
    loss = lambda qq, pp: float((g.astype(np.float64) * P.brute_force(qq, pp)[1]).sum())
    qt, pt = _dev(q[None]).requires_grad_(True), _dev(p[None]).requires_grad_(True)
    _pd().diff(qt, pt).backward(_dev(g[None]))
    dq, dp = qt.grad.cpu().numpy()[0].astype(np.float64), pt.grad.cpu().numpy()[0].astype(np.float64)
    h = 1e-5
    fd_q, fd_p = np.zeros_like(q), np.zeros_like(p)
    for idx in np.ndindex(*q.shape):
        e = np.zeros_like(q)
        e[idx] = h
        fd_q[idx] = (loss(q + e, p) - loss(q - e, p)) / (2 * h)
    for idx in np.ndindex(*p.shape):
        e = np.zeros_like(p)
        e[idx] = h
        fd_p[idx] = (loss(q, p + e) - loss(q, p - e)) / (2 * h)
    print("finite differences: dq %.2e, dp %.2e of the largest entry" % (np.abs(dq - fd_q).max() / np.abs(fd_q).max(),
                                                                         np.abs(dp - fd_p).max() / np.abs(fd_p).max()))
    assert np.abs(dq - fd_q).max() <= 1e-5 * np.abs(fd_q).max()
    assert np.abs(dp - fd_p).max() <= 1e-5 * np.abs(fd_p).max()
    assert not np.delete(dp, pick, axis=0).any()


# ---- refusals, wrappers ------------------------------------------------------------------------------------------------------

def test_wrong_device_dtype_or_shape_is_refused_and_nothing_is_launched():
    qs, ps = _small_batch(1, 9, 11, seed=17)
    pd = _pd()
    qt, pt = _dev(qs), _dev(ps)
    sentinel = (torch.full((1, 9), 5.0, device=DEV), torch.full((1, 9), 5, dtype=torch.int32, device=DEV))
    for bq, bp in ((qt.cpu(), pt), (qt, pt.cpu()), (qt.double(), pt), (qt, pt.double()), (qt[0], pt), (qt, pt[:, :, :2]),
                   (qt[:, :, :2], pt), (qs, pt), (qt, ps), (qt, torch.cat([pt, pt])), (qt[:, :0], pt), (qt, pt[:, :0])):
        with pytest.raises(ValueError):
            pd.forward(bq, bp, out=sentinel)
        with pytest.raises(ValueError):
            pd.diff(bq, bp)
    for bad_out in ((sentinel[0], sentinel[1].long()), (sentinel[0].double(), sentinel[1]), (sentinel[0].cpu(), sentinel[1]),
                    (sentinel[0], torch.full((1, 10), 5, dtype=torch.int32, device=DEV)), (sentinel[0],),
                    (torch.full((9, 2), 5.0, device=DEV).t()[:1], sentinel[1])):
        with pytest.raises(ValueError):
            pd.forward(qt, pt, out=bad_out)
    index = torch.zeros((1, 9), dtype=torch.int32, device=DEV)
    gt = torch.ones((1, 9), device=DEV)
    dq = torch.full((1, 9, 3), 5.0, device=DEV)
    for kw in (dict(index=index.long()), dict(index=index[:, :8]), dict(g=gt[:, :8]), dict(dq=torch.full((1, 8, 3), 5.0, device=DEV)),
               dict(dp=torch.full((1, 10, 3), 5.0, device=DEV)), dict(dq=dq.cpu()), dict(count=[12])):
        a = dict(index=index, g=gt, dq=dq)
        a.update(kw)
        with pytest.raises(ValueError):
            pd.backward(qt, pt, a.pop("index"), a.pop("g"), **a)
    torch.cuda.synchronize()
    assert all(bool((t == 5).all()) for t in sentinel) and bool((dq == 5).all())


def test_smpl_wrappers_equal_the_class():
    import smpl_synth as synth
    from cape_amd import smpl
    from cape_amd.scan_distance import pad_points
    m = synth.smpl_like()
    body = smpl.SMPL(m)
    assert body._point is None
    faces = np.asarray(m["f"], dtype=np.int64)
    rng = np.random.default_rng(18)
    xs = (m["v_template"][None] + 0.003 * rng.standard_normal((2, body.V, 3))).astype(np.float32)
    pts = [R.surface_samples(rng, xs[n].astype(np.float64), faces, m_n)[0].astype(np.float32) + np.float32(0.01)
           for n, m_n in enumerate((90, 33))]
    pd = _pd()
    want = pd.np(xs, pts)
    got = body.point_distance_np(xs, pts)
    assert body._point is not None and body._scan is None
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert (got[1][1] < 33).all() and (got[1] >= 0).all() and got[0].shape == (2, body.V)
    padded, count = pad_points(pts)
    xt, pt = _dev(xs), _dev(padded)
    dev_out = body.point_distance(xt, pt, count)
    assert dev_out[0].cpu().numpy().tobytes() == want[0].tobytes() and dev_out[1].cpu().numpy().tobytes() == want[1].tobytes()
    xg = xt.clone().requires_grad_(True)
    d2 = body.point_distance_diff(xg, pt, count)
    assert d2.detach().cpu().numpy().tobytes() == want[0].tobytes()
    d2.sum().backward()
    with torch.no_grad():
        dq, _ = pd.backward(xt, pt, dev_out[1], torch.ones_like(d2), count, want_dp=False)
    assert torch.equal(xg.grad, dq) and float(xg.grad.abs().max()) > 0
