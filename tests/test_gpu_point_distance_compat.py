"""Mesh-to-scan distance with normal compatibility on the device (PointDistance's ``query_normals`` / ``point_normals`` /
``cos_min``) against tests/compat_distance_reference.py, under tests/parity_bar.py's bar.  The measures are those of
tests/test_gpu_scan_distance_compat.py with points for faces:
  1 distance    max (sqrt(d2) - sqrt(sure)) / R and max (sqrt(maybe) - sqrt(d2)) / R against the float32 restatement's
  2 selection   the path's own point has c64 >= cos_min - DELTA and its float64 distance is the returned d2; no point in the
                maybe-set: index -1, d2 NaN; a point in the sure-set: a winner
  3 dq, dp      on the path's own indices, as tests/test_gpu_point_distance.py measures them
CONDITION: at most 1 % of a case's queries may be ambiguous (sure != maybe) -- asserted."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compat_distance_reference as C   # noqa: E402
import point_distance_reference as P    # noqa: E402
import scan_distance_reference as R     # noqa: E402
from parity_bar import check            # noqa: E402
from test_gpu_point_distance import DEV, PT, QB, SPLIT_MAX, _dev, _pd, rel_l2, vertex_err   # noqa: E402
from test_gpu_scan_distance_compat import COS30, COS60, _gap, _normals_off_every_face, _sheets   # noqa: E402

pytestmark = pytest.mark.gpu


def _run(pd, q, p, qn=None, pn=None, cos_min=None, count=None, g=None):
    """forward (+ the plain backward entry with the seed g) on numpy inputs: dict of numpy outputs."""
    qt, pt = _dev(q), _dev(p)
    kw = {} if qn is None else dict(query_normals=_dev(qn), point_normals=_dev(pn), cos_min=cos_min)
    with torch.no_grad():
        d2, index = pd.forward(qt, pt, count, **kw)
        out = dict(d2=d2.cpu().numpy(), index=index.cpu().numpy())
        if g is not None:
            dq, dp = pd.backward(qt, pt, index, _dev(g), count)
            out.update(dq=dq.cpu().numpy(), dp=dp.cpu().numpy())
    return out


def _measures(tag, q, p, qn, pn, cos_min, out, g, n=0, tables=None):
    ref = C.point_search(tables or C.point_tables(q, p, qn, pn), cos_min)
    Q = len(q)
    assert ref["ambiguous"].sum() <= 0.01 * Q, "%s: %d of %d queries are ambiguous" % (tag, ref["ambiguous"].sum(), Q)
    Rm = float(max(np.abs(q).max(), np.nanmax(np.abs(p))))
    index, d2 = out["index"][n].astype(np.int64), out["d2"][n].astype(np.float64)
    none, must, has, has32 = ref["maybe_id"] < 0, ref["sure_id"] >= 0, index >= 0, ref["id32"] >= 0
    assert (index < len(p)).all() and (index[none] == -1).all() and has[must].all() and has32[must].all()
    assert np.isfinite(d2[has]).all() and np.isnan(d2[~has]).all()
    assert (ref["c64"][np.arange(Q), np.maximum(index, 0)][has] >= cos_min - C.DELTA).all()
    q64, p64 = q.astype(np.float64), p.astype(np.float64)
    d_own, d_own32, d32 = P.own_d2(q64, p64, index), P.own_d2(q64, p64, ref["id32"]), ref["d32"].astype(np.float64)
    names = ["distance above sure", "distance below maybe", "own distance"]
    errs = [_gap(d2, ref["sure"], must & has) / Rm, _gap(ref["maybe"], d2, has) / Rm,
            max(_gap(d_own, d2, has), _gap(d2, d_own, has)) / Rm]
    errs32 = [_gap(d32, ref["sure"], must & has32) / Rm, _gap(ref["maybe"], d32, has32) / Rm,
              max(_gap(d_own32, d32, has32), _gap(d32, d_own32, has32)) / Rm]
    if g is not None:
        g64 = g[n].astype(np.float64)
        assert not out["dq"][n][~has].any()
        p0 = np.nan_to_num(p64)                                                          # padding rows: never selected
        dq64, dp64 = P.gradients(q64, p0, index, g64)
        dq64r, dp64r = P.gradients(q64, p0, ref["id32"], g64)
        dq32, dp32 = P.gradients(q, np.nan_to_num(p), ref["id32"], g[n], np.float32)
        for name, mine, want, mine32, want32 in (("dq", out["dq"][n], dq64, dq32, dq64r), ("dp", out["dp"][n], dp64, dp32, dp64r)):
            assert np.isfinite(mine).all()
            errs += [vertex_err(mine, want), rel_l2(mine, want)]
            errs32 += [vertex_err(mine32, want32), rel_l2(mine32, want32)]
            names += [name + " (vertex_err)", name + " (rel L2)"]
    print("%s[%d] cos_min %.4f R %.2f, %d ambiguous, %d without a point: " % (tag, n, cos_min, Rm, ref["ambiguous"].sum(), (~has).sum())
          + "; ".join("%s %.2e [fp32 %.2e]" % t for t in zip(names, errs, errs32)))
    for name, e, e32 in zip(names, errs, errs32):
        check(tag, name, e, e32)
    return ref


def _small_case(N, Q, M, seed):
    """N different small meshes (the octahedron scaled, moved and perturbed per sample): its vertices repeated to Q rows with a
    perturbation per row as queries, their vertex normals through the recipe's noise; a cloud of M points near the surface on
    both sides with normals by the same recipe.  (qs [N, Q, 3], ps [N, M, 3], qn, pn) float32."""
    rng = np.random.default_rng(seed)
    x0, f0 = R.octahedron()
    qs, ps, qn, pn = [], [], [], []
    for n in range(N):
        x = (x0 * rng.uniform(0.5, 1.5) + 0.01 * rng.standard_normal(x0.shape) + rng.uniform(-0.5, 0.5, 3)).astype(np.float32)
        vn = C.vertex_normals(x, f0)
        rows = np.arange(Q) % len(x)
        qs.append((x[rows].astype(np.float64) + 0.01 * rng.standard_normal((Q, 3))).astype(np.float32))
        qn.append(C.noisy_normals(rng, vn[rows]).astype(np.float32))
        p, nrm = R.surface_samples(rng, x.astype(np.float64), f0, M)
        ps.append((p + rng.uniform(-0.05, 0.1, M)[:, None] * nrm).astype(np.float32))
        pn.append(C.noisy_normals(rng, nrm).astype(np.float32))
    return np.stack(qs), np.stack(ps), np.stack(qn), np.stack(pn)


def _check_case(tag, qs, ps, qn, pn, cos_min, seed=0):
    g = np.random.default_rng(seed).standard_normal(qs.shape[:2]).astype(np.float32)
    out = _run(_pd(), qs, ps, qn, pn, cos_min, None, g)
    for n in range(qs.shape[0]):
        _measures(tag, qs[n], ps[n], qn[n], pn[n], cos_min, out, g, n=n)
    return out


# ---- the template ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _template(seed, shift, M=2049):
    x, faces, p, pn = C.template_case(seed, shift, M)
    vn = C.vertex_normals(x, faces).astype(np.float32)
    tables = C.point_tables(x, p, vn, pn)
    for a in (x, p, vn, pn) + tables:
        a.setflags(write=False)
    return x, p, vn, pn, tables


@pytest.mark.parametrize("cos_min", [COS30, COS60, 0.0])
@pytest.mark.parametrize("seed,shift", [(3, 0.0), (5, 3.0)])
def test_template_recipes(seed, shift, cos_min):
    """The 6890 template vertices with their float64 vertex normals against the recipe's 2049 points and normals."""
    x, p, vn, pn, tables = _template(seed, shift)
    g = np.random.default_rng(13).standard_normal((1, len(x))).astype(np.float32)
    pd = _pd()
    out = _run(pd, x[None], p[None], vn[None], pn[None], cos_min, None, g)
    _measures("compat_point_template_shift%g" % shift, x, p, vn, pn, cos_min, out, g, tables=tables)
    plain = _run(pd, x[None], p[None])
    changed = int((out["d2"].view(np.uint32) != plain["d2"].view(np.uint32)).sum())
    print("the filter changes %d of %d vertices" % (changed, len(x)))
    assert changed >= 1000                                 # the recipe filters: the plain search fails this test
    if cos_min == 0.0:
        for c in (-2.0, -float("inf")):
            same = _run(pd, x[None], p[None], vn[None], pn[None], c)
            assert same["index"].tobytes() == plain["index"].tobytes() and same["d2"].tobytes() == plain["d2"].tobytes()


# ---- tile edges, the split ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,Q,N", [(1, 1, 1), (PT, QB - 1, 1), (PT + 1, QB, 3), (128, QB + 1, 3), (PT + 1, 1, 3), (PT - 1, 40, 1)])
def test_tile_edges_on_the_small_mesh(M, Q, N):
    qs, ps, qn, pn = _small_case(N, Q, M, seed=M + Q)
    _check_case("compat_point_small_M%d_Q%d_N%d" % (M, Q, N), qs, ps, qn, pn, 0.0 if M == 1 else 0.5)


def test_point_split_factors_give_the_same_bits():
    """One sample of 16 point tiles with QB and 600 QB queries selects 16 parts and 1; the first QB queries are the same in both
    and must come back bit for bit, and be right."""
    M = SPLIT_MAX * PT
    pd = _pd()
    sizes = (QB, 600 * QB)
    assert [pd.plan(1, Q, M)[0] for Q in sizes] == [SPLIT_MAX, 1]
    q0, p, qn0, pn = _small_case(1, QB, M, seed=8)
    rng = np.random.default_rng(9)
    q = (rng.standard_normal((1, sizes[-1], 3)) * 0.4).astype(np.float32)
    qn = rng.standard_normal(q.shape)
    qn = (qn / np.linalg.norm(qn, axis=2, keepdims=True)).astype(np.float32)
    q[0, :QB], qn[0, :QB] = q0[0], qn0[0]
    g = np.random.default_rng(1).standard_normal((1, QB)).astype(np.float32)
    for cos_min in (COS60, 0.0):
        few, many = _run(pd, q[:, :QB], p, qn[:, :QB], pn, cos_min, None, g), _run(pd, q, p, qn, pn, cos_min)
        for k in ("index", "d2"):
            assert few[k].tobytes() == many[k][:, :QB].tobytes(), k
        _measures("compat_point_split", q[0, :QB], p[0], qn[0, :QB], pn[0], cos_min, few, g)


# ---- a sleeve ----------------------------------------------------------------------------------------------------------------

def test_a_sleeve_takes_the_sheet_that_faces_the_same_way():
    """The corners of two sheets 2 mm apart as the cloud, each with its sheet's normal; queries straight below corners of the
    front sheet, 0.5 mm from the back one, with the front's normal."""
    x, _, _ = _sheets(k=8)
    nv = len(x) // 2
    pn = np.concatenate([np.tile(np.float32([0, 0, 1]), (nv, 1)), np.tile(np.float32([0, 0, -1]), (nv, 1))])
    q = x[:nv].copy()
    q[:, 2] = np.float32(-0.5e-3)
    qn = np.tile(np.float32([0, 0, 1]), (nv, 1))
    pd = _pd()
    g = np.random.default_rng(20).standard_normal((1, nv)).astype(np.float32)
    plain = _run(pd, q[None], x[None])
    assert (plain["index"][0] == np.arange(nv) + nv).all()
    out = _run(pd, q[None], x[None], qn[None], pn[None], 0.0, None, g)
    assert (out["index"][0] == np.arange(nv)).all()
    _measures("compat_point_sleeve", q, x, qn, pn, 0.0, out, g)
    print("sleeve: largest |sqrt(d2) - 1.5 mm| %.2e" % np.abs(np.sqrt(out["d2"].astype(np.float64)) - 1.5e-3).max())
    assert np.abs(np.sqrt(out["d2"].astype(np.float64)) - 1.5e-3).max() <= 4 * 2.0 ** -24 * 0.05   # the bar's floor at R = 0.05


# ---- no compatible point, bad normals ----------------------------------------------------------------------------------------

def test_no_compatible_point():
    Q, M = 130, 128
    qs, ps, _, _ = _small_case(1, Q, M, seed=21)
    x0, f0 = R.octahedron()
    fn = C.face_normals(x0, f0)                                                           # one point normal per face normal
    pn = fn.astype(np.float32)[None]
    qn = _normals_off_every_face(np.random.default_rng(22), fn, Q)[None]
    g = np.random.default_rng(23).standard_normal((1, Q)).astype(np.float32)
    out = _run(_pd(), qs, ps, qn, pn, 0.9999, None, g)
    assert (out["index"] == -1).all() and np.isnan(out["d2"]).all() and not out["dq"].any() and not out["dp"].any()
    _measures("compat_point_none", qs[0], ps[0], qn[0], pn[0], 0.9999, out, g)


def test_bad_normals():
    Q, M = 130, PT + 10
    qs, ps, qn, pn = _small_case(1, Q, M, seed=8)
    pd = _pd()
    g = np.random.default_rng(9).standard_normal((1, Q)).astype(np.float32)
    base = _run(pd, qs, ps, qn, pn, -2.0, None, g)
    assert (base["index"] >= 0).all()
    bad = qn.copy()
    bad[0, 70, 1] = np.nan
    bad[0, 5, 2] = np.inf
    bad[0, 6, 0] = -np.inf
    out = _run(pd, qs, ps, bad, pn, -2.0, None, g)
    for j in (70, 5, 6):
        assert out["index"][0, j] == -1 and np.isnan(out["d2"][0, j]) and not out["dq"][0, j].any()
    keep = np.setdiff1d(np.arange(Q), (70, 5, 6))         # the neighbours in the wave are unaffected
    for k in ("index", "d2", "dq"):
        assert out[k][0, keep].tobytes() == base[k][0, keep].tobytes(), k
    # a point with such a normal never wins: the result without the point
    at = np.array([3, PT - 1])
    badp = pn.copy()
    badp[0, at[0], 0], badp[0, at[1], 2] = np.nan, np.inf
    out = _run(pd, qs, ps, qn, badp, -2.0)
    without = _run(pd, qs, np.delete(ps, at, 1), qn, np.delete(pn, at, 1), -2.0)
    assert not np.isin(out["index"], at).any()
    shifted = out["index"] - (out["index"] > at[0]) - (out["index"] > at[1])
    assert np.array_equal(shifted, without["index"]) and out["d2"].tobytes() == without["d2"].tobytes()


# ---- counts, wide rows, determinism --------------------------------------------------------------------------------------------

def test_ragged_counts():
    M, Q = 40, 70
    qs, ps, qn, pn = _small_case(4, Q, M, seed=2)
    count = np.array([M, 1, 0, 7], np.int32)
    for n in range(4):
        ps[n, count[n]:] = np.nan                          # padding is never read: points and normals
        pn[n, count[n]:] = np.nan
    pd = _pd()
    g = np.random.default_rng(3).standard_normal((4, Q)).astype(np.float32)
    out = _run(pd, qs, ps, qn, pn, 0.0, count, g)
    for n in range(4):
        c = count[n]
        m = max(c, 1)
        assert not out["dp"][n, c:].any() and np.isfinite(out["dp"][n]).all()
        alone = _run(pd, qs[n:n + 1], ps[n:n + 1, :m], qn[n:n + 1], pn[n:n + 1, :m], 0.0, None if c else np.zeros(1, np.int32),
                     g[n:n + 1])
        for k in ("index", "d2", "dq"):
            assert out[k][n].tobytes() == alone[k][0].tobytes(), (n, k)
        assert out["dp"][n, :c].tobytes() == alone["dp"][0, :c].tobytes(), n
        assert (out["index"][n] < max(c, 0)).all()
    assert (out["index"][2] == -1).all() and np.isnan(out["d2"][2]).all() and not out["dq"][2].any()
    _measures("compat_point_ragged", qs[0], ps[0], qn[0], pn[0], 0.0, out, g)
    sub = dict(index=out["index"][3:4], d2=out["d2"][3:4], dq=out["dq"][3:4], dp=out["dp"][3:4, :7])
    _measures("compat_point_ragged", qs[3], ps[3, :7], qn[3], pn[3, :7], 0.0, sub, g[3:4])


def test_wide_rows():
    N, M, Q = 2, 37, 45
    qs, ps, qn, pn = _small_case(N, Q, M, seed=4)
    pd = _pd()
    want = _run(pd, qs, ps, qn, pn, 0.5)
    assert (want["index"] >= 0).any()
    q4, p5 = np.full((N, Q, 4), np.nan, np.float32), np.full((N, M, 5), np.nan, np.float32)
    q4[:, :, :3], p5[:, :, :3] = qn, pn
    with torch.no_grad():
        d2, index = pd.forward(_dev(qs), _dev(ps), query_normals=_dev(q4)[:, :, :3], point_normals=_dev(p5)[:, :, :3], cos_min=0.5)
    assert d2.cpu().numpy().tobytes() == want["d2"].tobytes() and index.cpu().numpy().tobytes() == want["index"].tobytes()


def test_determinism():
    qs, ps, qn, pn = _small_case(2, 300, PT + 30, seed=10)
    pd = _pd()
    g = np.random.default_rng(11).standard_normal((2, 300)).astype(np.float32)
    out = _run(pd, qs, ps, qn, pn, COS60, None, g)
    again = _run(pd, qs, ps, qn, pn, COS60, None, g)
    swapped = _run(pd, qs[::-1], ps[::-1], qn[::-1], pn[::-1], COS60, None, g[::-1])
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k
        assert out[k].tobytes() == swapped[k][::-1].tobytes(), k


# ---- autograd, refusals, the SMPL wrappers -------------------------------------------------------------------------------------

def test_diff_matches_forward_and_the_backward_entry():
    N, M, Q = 2, 50, 60
    qs, ps, qn, pn = _small_case(N, Q, M, seed=14)
    pd = _pd()
    g = np.random.default_rng(15).standard_normal((N, Q)).astype(np.float32)
    want = _run(pd, qs, ps, qn, pn, 0.5, None, g)
    assert (want["index"] >= 0).any() and (want["index"] != _run(pd, qs, ps)["index"]).any()
    qt, pt = _dev(qs).requires_grad_(True), _dev(ps).requires_grad_(True)
    d2, index = pd.diff(qt, pt, return_selection=True, query_normals=_dev(qn), point_normals=_dev(pn), cos_min=0.5)
    assert d2.requires_grad and not index.requires_grad
    d2.backward(_dev(g))
    got = dict(d2=d2.detach(), index=index, dq=qt.grad, dp=pt.grad)
    for k, v in got.items():
        assert v.cpu().numpy().tobytes() == want[k].tobytes(), k


def test_refusals_launch_nothing():
    qs, ps, qn, pn = _small_case(1, 9, 11, seed=17)
    pd = _pd()
    qt, pt, at, bt = _dev(qs), _dev(ps), _dev(qn), _dev(pn)
    sentinel = (torch.full((1, 9), 5.0, device=DEV), torch.full((1, 9), 5, dtype=torch.int32, device=DEV))
    good = dict(query_normals=at, point_normals=bt, cos_min=0.5)
    bads = [dict(query_normals=at, point_normals=bt), dict(cos_min=0.5), dict(query_normals=at, cos_min=0.5),
            dict(point_normals=bt, cos_min=0.5), dict(good, cos_min=float("nan")), dict(good, query_normals=at.cpu()),
            dict(good, point_normals=bt.double()), dict(good, query_normals=at[:, :8]), dict(good, point_normals=bt[:, :, :2]),
            dict(good, point_normals=pn), dict(good, query_normals=bt)]
    for kw in bads:
        with pytest.raises(ValueError):
            pd.forward(qt, pt, out=sentinel, **kw)
        with pytest.raises(ValueError):
            pd.diff(qt, pt, **kw)
    for name in ("query_normals", "point_normals"):
        kw = dict(good)
        kw[name] = kw[name].clone().requires_grad_(True)
        with pytest.raises(RuntimeError):
            pd.forward(qt, pt, out=sentinel, **kw)
        with pytest.raises(RuntimeError):
            pd.diff(qt, pt, **kw)
    torch.cuda.synchronize()
    assert all(bool((t == 5).all()) for t in sentinel)


def test_smpl_wrappers_equal_the_class_fed_the_vertex_normals():
    import smpl_synth as synth
    from cape_amd import smpl
    from cape_amd.scan_distance import pad_normals, pad_points
    m = synth.smpl_like()
    body = smpl.SMPL(m)
    faces = np.asarray(m["f"], dtype=np.int64)
    rng = np.random.default_rng(18)
    xs = (m["v_template"][None] + 0.003 * rng.standard_normal((2, body.V, 3))).astype(np.float32)
    pts, nrm = [], []
    for n, m_n in enumerate((90, 33)):
        p, nn = R.surface_samples(rng, xs[n].astype(np.float64), faces, m_n)
        pts.append(p.astype(np.float32) + np.float32(0.01)), nrm.append(C.noisy_normals(rng, nn).astype(np.float32))
    pd = _pd()
    vn = body.vertex_normals_np(xs)
    want = pd.np(xs, pts, query_normals=vn, point_normals=nrm, cos_min=COS60)
    plain = pd.np(xs, pts)
    assert (want[1] != plain[1]).any() and (want[1] >= 0).any()
    got = body.point_distance_np(xs, pts, point_normals=nrm, cos_min=COS60)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    padded, count = pad_points(pts)
    nt = _dev(pad_normals("point_normals", nrm, padded, count))
    xt, pt = _dev(xs), _dev(padded)
    dev_out = body.point_distance(xt, pt, count, point_normals=nt, cos_min=COS60)
    assert dev_out[0].cpu().numpy().tobytes() == want[0].tobytes() and dev_out[1].cpu().numpy().tobytes() == want[1].tobytes()
    cls_out = pd.forward(xt, pt, count, query_normals=body.vertex_normals(xt), point_normals=nt, cos_min=COS60)
    assert torch.equal(cls_out[1], dev_out[1])
    xg = xt.clone().requires_grad_(True)
    d2 = body.point_distance_diff(xg, pt, count, point_normals=nt, cos_min=COS60)
    assert d2.detach().cpu().numpy().tobytes() == want[0].tobytes()
    d2.nan_to_num().sum().backward()
    with torch.no_grad():
        dq, _ = pd.backward(xt, pt, dev_out[1], torch.isfinite(d2.detach()).float(), count, want_dp=False)
    assert torch.equal(xg.grad, dq) and float(xg.grad.abs().max()) > 0
