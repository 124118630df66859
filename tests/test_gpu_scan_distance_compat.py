"""Scan-to-mesh distance with normal compatibility on the device (ScanDistance's ``normals`` / ``cos_min``) against
tests/compat_distance_reference.py, under tests/parity_bar.py's bar.  The device decides compatibility in fp32, the reference
in float64 with a band DELTA: ``sure`` is the float64 minimum over the faces compatible whatever the rounding, ``maybe`` over
every face the device may have accepted.  R is the largest absolute coordinate of a case; every point is compared:
  1 distance    max (sqrt(d2) - sqrt(sure)) / R and max (sqrt(maybe) - sqrt(d2)) / R, each against the same measure of the float32
                restatement (which filters at cos_min itself): for an unambiguous point the distance is pinned from both sides
  2 selection   the path's own face has c64 >= cos_min - DELTA and its float64 distance is the returned d2 (within the bar); no
                face in the maybe-set: face -1, d2 NaN, bary 0; a face in the sure-set: a winner
  3 foot, dx, dp  on the path's own faces, as tests/test_gpu_scan_distance.py measures them
CONDITION: at most 1 % of a case's points may be ambiguous (sure != maybe) -- asserted, so no case passes by being all band."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compat_distance_reference as C   # noqa: E402
import scan_distance_reference as R     # noqa: E402
from parity_bar import check            # noqa: E402
from test_gpu_scan_distance import B, DEV, SPLIT_MAX, T, _dev, _sd, rel_l2, vertex_err   # noqa: E402

pytestmark = pytest.mark.gpu

COS30, COS60 = float(np.cos(np.deg2rad(30.0))), float(np.cos(np.deg2rad(60.0)))


def _run(sd, x, p, nrm=None, cos_min=None, count=None, g=None):
    """forward (+ the plain backward entry with the seed g) on numpy inputs: dict of numpy outputs."""
    xt, pt = _dev(x), _dev(p)
    kw = {} if nrm is None else dict(normals=_dev(nrm), cos_min=cos_min)
    with torch.no_grad():
        d2, face, bary = sd.forward(xt, pt, count, **kw)
        out = dict(d2=d2.cpu().numpy(), face=face.cpu().numpy(), bary=bary.cpu().numpy())
        if g is not None:
            dx, dp = sd.backward(xt, pt, face, bary, _dev(g))
            out.update(dx=dx.cpu().numpy(), dp=dp.cpu().numpy())
    return out


def _gap(a, b, where):
    """max over ``where`` of sqrt(a) - sqrt(b), at least 0."""
    with np.errstate(invalid="ignore"):
        d = np.sqrt(a.astype(np.float64)) - np.sqrt(b.astype(np.float64))
    return float(np.max(np.where(where, d, 0.0), initial=0.0))


def _measures(tag, x, faces, p, nrm, cos_min, out, g, n=0, tables=None):
    """Measures 1-3 and the condition for sample ``n`` of a run; returns the reference's dict."""
    ref = C.scan_search(tables or C.scan_tables(x, faces, p, nrm), cos_min)
    M = len(p)
    assert ref["ambiguous"].sum() <= 0.01 * M, "%s: %d of %d points are ambiguous" % (tag, ref["ambiguous"].sum(), M)
    Rm = float(max(np.nanmax(np.abs(x)), np.abs(p).max()))
    face, bary, d2 = out["face"][n].astype(np.int64), out["bary"][n].astype(np.float64), out["d2"][n].astype(np.float64)
    none, must, has, has32 = ref["maybe_id"] < 0, ref["sure_id"] >= 0, face >= 0, ref["id32"] >= 0
    assert (face < len(faces)).all() and (face[none] == -1).all() and has[must].all() and has32[must].all()
    assert np.isfinite(d2[has]).all() and np.isnan(d2[~has]).all() and np.isfinite(bary).all() and not bary[~has].any()
    assert (ref["c64"][np.arange(M), np.maximum(face, 0)][has] >= cos_min - C.DELTA).all()
    x64, p64 = x.astype(np.float64), p.astype(np.float64)
    d_own, d_own32 = np.full(M, np.nan), np.full(M, np.nan)
    foot_own, foot_own32 = np.zeros((M, 3)), np.zeros((M, 3))
    _, _, foot_own[has], d_own[has] = R.on_face(x64, faces, p64[has], face[has])
    _, _, foot_own32[has32], d_own32[has32] = R.on_face(x64, faces, p64[has32], ref["id32"][has32])
    d32 = ref["d32"].astype(np.float64)
    foot = np.zeros((M, 3))
    foot[has] = (bary[has][:, :, None] * x64[faces[face[has]]]).sum(1)
    names = ["distance above sure", "distance below maybe", "own distance", "foot"]
    errs = [_gap(d2, ref["sure"], must & has) / Rm, _gap(ref["maybe"], d2, has) / Rm,
            max(_gap(d_own, d2, has), _gap(d2, d_own, has)) / Rm, np.abs(foot - foot_own).max() / Rm]
    errs32 = [_gap(d32, ref["sure"], must & has32) / Rm, _gap(ref["maybe"], d32, has32) / Rm,
              max(_gap(d_own32, d32, has32), _gap(d32, d_own32, has32)) / Rm,
              np.abs(np.where(has32[:, None], ref["foot32"].astype(np.float64), 0.0) - foot_own32).max() / Rm]
    if g is not None:
        g64 = g[n].astype(np.float64)
        assert not out["dp"][n][~has].any()
        dx64, dp64 = R.gradients(x64, faces, p64, face, g64)
        dx64r, dp64r = R.gradients(x64, faces, p64, ref["id32"], g64)
        dx32, dp32 = R.gradients(x, faces, p, ref["id32"], g[n], np.float32)
        for name, mine, want, mine32, want32 in (("dx", out["dx"][n], dx64, dx32, dx64r), ("dp", out["dp"][n], dp64, dp32, dp64r)):
            assert np.isfinite(mine).all()
            errs += [vertex_err(mine, want), rel_l2(mine, want)]
            errs32 += [vertex_err(mine32, want32), rel_l2(mine32, want32)]
            names += [name + " (vertex_err)", name + " (rel L2)"]
    print("%s[%d] cos_min %.4f R %.2f, %d ambiguous, %d without a face: " % (tag, n, cos_min, Rm, ref["ambiguous"].sum(), (~has).sum())
          + "; ".join("%s %.2e [fp32 %.2e]" % t for t in zip(names, errs, errs32)))
    for name, e, e32 in zip(names, errs, errs32):
        check(tag, name, e, e32)
    return ref


def _small_case(N, M, F, seed):
    """N different small meshes (the octahedron scaled, moved and perturbed per sample, its faces repeated up to F rows), points
    near the surface on both sides, a quarter anywhere in the inflated box, and normals by the recipe of the template cases."""
    rng = np.random.default_rng(seed)
    x0, f0 = R.octahedron()
    faces = np.concatenate([f0] * (F // len(f0) + 1))[:F]
    xs, ps, ns = [], [], []
    for n in range(N):
        x = (x0 * rng.uniform(0.5, 1.5) + 0.01 * rng.standard_normal(x0.shape) + rng.uniform(-0.5, 0.5, 3)).astype(np.float32)
        p, nrm = R.surface_samples(rng, x.astype(np.float64), f0, M)
        p = p + rng.uniform(-0.05, 0.1, M)[:, None] * nrm
        far = rng.permutation(M)[:M // 4]
        p[far] = rng.uniform(x.min(0) - 0.3, x.max(0) + 0.3, (len(far), 3))
        xs.append(x), ps.append(p.astype(np.float32)), ns.append(C.noisy_normals(rng, nrm).astype(np.float32))
    return np.stack(xs), faces, np.stack(ps), np.stack(ns)


def _check_case(tag, xs, faces, ps, ns, cos_min, seed=0):
    g = np.random.default_rng(seed).standard_normal(ps.shape[:2]).astype(np.float32)
    out = _run(_sd(faces, xs.shape[1]), xs, ps, ns, cos_min, None, g)
    for n in range(xs.shape[0]):
        _measures(tag, xs[n], faces, ps[n], ns[n], cos_min, out, g, n=n)
    return out


# ---- the template ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _template(seed, shift, M=256):
    x, faces, p, nrm = C.template_case(seed, shift, M)
    tables = C.scan_tables(x, faces, p, nrm)
    for a in (x, faces, p, nrm) + tables:
        a.setflags(write=False)
    return x, faces, p, nrm, tables


@pytest.mark.parametrize("cos_min", [COS30, COS60, 0.0])
@pytest.mark.parametrize("seed,shift", [(3, 0.0), (5, 3.0)])
def test_template_recipes(seed, shift, cos_min):
    x, faces, p, nrm, tables = _template(seed, shift)
    g = np.random.default_rng(13).standard_normal((1, len(p))).astype(np.float32)
    sd = _sd(faces, x.shape[0])
    out = _run(sd, x[None], p[None], nrm[None], cos_min, None, g)
    _measures("compat_scan_template_shift%g" % shift, x, faces, p, nrm, cos_min, out, g, tables=tables)
    plain = _run(sd, x[None], p[None])
    changed = int((out["d2"].view(np.uint32) != plain["d2"].view(np.uint32)).sum())
    print("the filter changes %d of %d points" % (changed, len(p)))
    assert changed >= 40                                   # the recipe filters: the plain search fails this test


@pytest.mark.parametrize("seed,shift", [(3, 0.0), (5, 3.0)])
def test_no_filtering_returns_the_plain_entrys_bits_on_the_template(seed, shift):
    x, faces, p, nrm, _ = _template(seed, shift)
    sd = _sd(faces, x.shape[0])
    plain = _run(sd, x[None], p[None])
    for cos_min in (-2.0, -float("inf")):
        out = _run(sd, x[None], p[None], nrm[None], cos_min)
        for k in ("face", "bary", "d2"):
            assert out[k].tobytes() == plain[k].tobytes(), (k, cos_min)


# ---- tile edges, the split ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F,M,N", [(128, 1, 1), (T, B - 1, 1), (T + 1, B, 3), (128, B + 1, 3), (T + 1, 1, 3)])
def test_tile_edges_on_the_small_mesh(F, M, N):
    xs, faces, ps, ns = _small_case(N, M, F, seed=F + M)
    _check_case("compat_scan_small_F%d_M%d_N%d" % (F, M, N), xs, faces, ps, ns, 0.5)


def test_face_split_factors_give_the_same_bits():
    """One mesh of 16 face tiles with 512 and 300 * 512 points selects 16 parts and 1; the first 512 points are the same in both
    and must come back bit for bit, and be right."""
    x, faces = R.octahedron(5)
    assert len(faces) == SPLIT_MAX * T
    x = x.astype(np.float32)[None]
    sd = _sd(faces, x.shape[1])
    sizes = (B, 300 * B)
    assert [sd.plan(1, M)[0] for M in sizes] == [SPLIT_MAX, 1]
    rng = np.random.default_rng(8)
    p = (rng.standard_normal((1, sizes[-1], 3)) * 0.4).astype(np.float32)
    nrm = rng.standard_normal(p.shape)
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    p0, n0 = R.surface_samples(rng, x[0].astype(np.float64), faces, B)
    p[0, :B] = p0 + rng.uniform(-0.05, 0.1, B)[:, None] * n0
    nrm[0, :B] = C.noisy_normals(rng, n0)
    g = np.random.default_rng(1).standard_normal((1, B)).astype(np.float32)
    for cos_min in (COS60, 0.0):
        few, many = _run(sd, x, p[:, :B], nrm[:, :B], cos_min, None, g), _run(sd, x, p, nrm, cos_min)
        for k in ("face", "bary", "d2"):
            assert few[k].tobytes() == many[k][:, :B].tobytes(), k
        _measures("compat_scan_split", x[0], faces, p[0, :B], nrm[0, :B], cos_min, few, g)


# ---- a sleeve ----------------------------------------------------------------------------------------------------------------

def _sheets(k=4, gap=2e-3, side=0.1):
    """Two parallel square sheets of k x k quads ``gap`` apart: the front at z = +gap / 2 with normal +z, the back at
    z = -gap / 2 with normal -z.  (x [V, 3] float32, faces, unit face normals [F, 3])."""
    u = np.linspace(-side / 2, side / 2, k + 1)
    gx, gy = np.meshgrid(u, u, indexing="ij")
    flat = np.stack([gx.ravel(), gy.ravel()], 1)
    idx = lambda i, j: i * (k + 1) + j
    quads = [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)) for i in range(k) for j in range(k)]
    front = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]                  # counter-clockwise seen from +z
    nv = len(flat)
    back = [(a + nv, c + nv, b + nv) for a, b, c in front]
    x = np.concatenate([np.c_[flat, np.full(nv, gap / 2)], np.c_[flat, np.full(nv, -gap / 2)]]).astype(np.float32)
    faces = np.array(front + back, dtype=np.int64)
    return x, faces, C.face_normals(x, faces)


def test_a_sleeve_takes_the_sheet_that_faces_the_same_way():
    x, faces, fn = _sheets()
    nf = len(faces) // 2
    assert (fn[:nf, 2] == 1.0).all() and (fn[nf:, 2] == -1.0).all()
    rng = np.random.default_rng(20)
    M = 200
    p = np.c_[rng.uniform(-0.04, 0.04, (M, 2)), np.full(M, -0.5e-3)].astype(np.float32)   # 0.5 mm from the back, 1.5 from the front
    nrm = np.tile(np.float32([0, 0, 1]), (M, 1))
    sd = _sd(faces, x.shape[0])
    g = rng.standard_normal((1, M)).astype(np.float32)
    plain = _run(sd, x[None], p[None])
    assert (plain["face"] >= nf).all() and np.abs(np.sqrt(plain["d2"]) - 0.5e-3).max() < 1e-8
    out = _run(sd, x[None], p[None], nrm[None], 0.0, None, g)
    assert (out["face"] >= 0).all() and (out["face"] < nf).all()
    _measures("compat_scan_sleeve", x, faces, p, nrm, 0.0, out, g)
    print("sleeve: largest |sqrt(d2) - 1.5 mm| %.2e" % np.abs(np.sqrt(out["d2"]) - 1.5e-3).max())
    assert np.abs(np.sqrt(out["d2"].astype(np.float64)) - 1.5e-3).max() <= 4 * 2.0 ** -24 * 0.05   # the bar's floor at R = 0.05


# ---- degenerate faces, no compatible face, bad normals -------------------------------------------------------------------------

def test_degenerate_faces():
    M = 128                                                # point 3 is ambiguous by construction (c = 0 = cos_min): 1 of 128
    xs, faces, ps, ns = _small_case(1, M, 2 * T + 7, seed=6)
    where = ps[0, 3].astype(np.float64) + 1e-4
    xc, fc = R.append_face(xs[0], faces, "collapsed", at=T + 100, where=where)
    xn, fn = R.append_face(xc, fc, "nan")
    V = xn.shape[0]
    sd = _sd(fn, V)
    plain = _run(sd, xn[None], ps)
    assert (plain["face"][0] == T + 100).nonzero()[0].tolist() == [3]
    # every point carries the normal of its own nearest face: the collapsed face, whose c = 0 lies in the band of cos_min = 0 for
    # every point, is then nearer than a compatible face for point 3 alone
    ns = C.face_normals(xs[0], faces)[_run(_sd(faces, 66), xs, ps)["face"][0]].astype(np.float32)[None]
    # nothing filtered: the plain entry's bits, whatever the degenerate faces
    out = _run(sd, xn[None], ps, ns, -2.0)
    for k in ("face", "bary", "d2"):
        assert out[k].tobytes() == plain[k].tobytes(), k
    # a collapsed face has the normal (0, 0, 0): c = 0, compatible iff cos_min <= 0
    g = np.random.default_rng(7).standard_normal((1, M)).astype(np.float32)
    out = _run(sd, xn[None], ps, ns, 0.0, None, g)
    assert out["face"][0, 3] == T + 100
    assert (out["face"] != len(fn) - 1).all()                                            # the NaN face never wins
    _measures("compat_scan_collapsed", xn, fn, ps[0], ns[0], 0.0, out, g)
    out = _run(sd, xn[None], ps, ns, 0.5, None, g)
    assert (out["face"] != T + 100).all() and (out["face"] != len(fn) - 1).all()
    _measures("compat_scan_collapsed_0.5", xn, fn, ps[0], ns[0], 0.5, out, g)


def _normals_off_every_face(rng, fn, M, degrees=3.0):
    """Unit normals [M, 3] at least ``degrees`` off every face normal."""
    out = np.empty((0, 3))
    while len(out) < M:
        n = rng.standard_normal((4 * M, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        out = np.concatenate([out, n[(n @ fn.T).max(1) <= np.cos(np.deg2rad(degrees))]])
    return out[:M].astype(np.float32)


def test_no_compatible_face():
    M = 130
    xs, faces, ps, _ = _small_case(1, M, 128, seed=21)
    ns = _normals_off_every_face(np.random.default_rng(22), C.face_normals(xs[0], faces), M)[None]
    g = np.random.default_rng(23).standard_normal((1, M)).astype(np.float32)
    out = _run(_sd(faces, 66), xs, ps, ns, 0.9999, None, g)
    assert (out["face"] == -1).all() and np.isnan(out["d2"]).all() and not out["bary"].any()
    assert not out["dx"].any() and not out["dp"].any()
    _measures("compat_scan_none", xs[0], faces, ps[0], ns[0], 0.9999, out, g)


def test_bad_normals():
    M = 130
    xs, faces, ps, ns = _small_case(1, M, 128, seed=8)
    sd = _sd(faces, 66)
    base = _run(sd, xs, ps, ns, 0.0)
    bad = ns.copy()
    bad[0, 70, 1] = np.nan
    bad[0, 5, 2] = np.inf
    bad[0, 6, 0] = -np.inf
    out = _run(sd, xs, ps, bad, 0.0)
    for i in (70, 5, 6):
        assert out["face"][0, i] == -1 and np.isnan(out["d2"][0, i]) and not out["bary"][0, i].any()
    keep = np.setdiff1d(np.arange(M), (70, 5, 6))          # the neighbours in the wave are unaffected
    assert (base["face"][0, [70, 5, 6]] >= 0).all()
    for k in ("face", "bary", "d2"):
        assert out[k][0, keep].tobytes() == base[k][0, keep].tobytes(), k


# ---- counts, wide rows, determinism --------------------------------------------------------------------------------------------

def test_ragged_counts():
    M = 40
    xs, faces, ps, ns = _small_case(4, M, 128, seed=2)
    count = np.array([M, 1, 0, 7], np.int32)
    for n in range(4):
        ps[n, count[n]:] = np.nan                          # padding is never read: points and normals
        ns[n, count[n]:] = np.nan
    sd = _sd(faces, 66)
    g = np.random.default_rng(3).standard_normal((4, M)).astype(np.float32)
    out = _run(sd, xs, ps, ns, 0.5, count, g)
    for n in range(4):
        c = count[n]
        assert (out["face"][n, c:] == -1).all() and not out["d2"][n, c:].any() and not out["bary"][n, c:].any()
        assert not out["dp"][n, c:].any()
        m = max(c, 1)
        alone = _run(sd, xs[n:n + 1], ps[n:n + 1, :m], ns[n:n + 1, :m], 0.5, None if c else np.zeros(1, np.int32), g[n:n + 1, :m])
        for k in ("face", "bary", "d2", "dp"):
            assert out[k][n, :c].tobytes() == alone[k][0, :c].tobytes(), (n, k)
        assert out["dx"][n].tobytes() == alone["dx"][0].tobytes()
    assert not out["dx"][2].any()
    _measures("compat_scan_ragged", xs[0], faces, ps[0], ns[0], 0.5, out, g)


def test_wide_rows():
    N, M = 2, 37
    xs, faces, ps, ns = _small_case(N, M, 128, seed=4)
    sd = _sd(faces, 66)
    want = _run(sd, xs, ps, ns, 0.5)
    assert (want["face"] >= 0).any()
    for width in (4, 5):
        n4 = np.full((N, M, width), np.nan, np.float32)
        n4[:, :, :3] = ns
        with torch.no_grad():
            got = sd.forward(_dev(xs), _dev(ps), normals=_dev(n4)[:, :, :3], cos_min=0.5)
        for k, v in zip(("d2", "face", "bary"), got):
            assert v.cpu().numpy().tobytes() == want[k].tobytes(), (k, width)


def test_determinism():
    xs, faces, ps, ns = _small_case(2, 300, 128, seed=10)
    sd = _sd(faces, 66)
    g = np.random.default_rng(11).standard_normal((2, 300)).astype(np.float32)
    out = _run(sd, xs, ps, ns, COS60, None, g)
    again = _run(sd, xs, ps, ns, COS60, None, g)
    swapped = _run(sd, xs[::-1], ps[::-1], ns[::-1], COS60, None, g[::-1])
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k
        assert out[k].tobytes() == swapped[k][::-1].tobytes(), k


# ---- autograd, refusals, the SMPL wrappers -------------------------------------------------------------------------------------

def test_diff_matches_forward_and_the_backward_entry():
    N, M = 2, 50
    xs, faces, ps, ns = _small_case(N, M, 128, seed=14)
    sd = _sd(faces, 66)
    g = np.random.default_rng(15).standard_normal((N, M)).astype(np.float32)
    want = _run(sd, xs, ps, ns, 0.5, None, g)
    assert (want["face"] >= 0).any() and (want["face"] != _run(sd, xs, ps)["face"]).any()
    xt, pt = _dev(xs).requires_grad_(True), _dev(ps).requires_grad_(True)
    d2, face, bary = sd.diff(xt, pt, return_selection=True, normals=_dev(ns), cos_min=0.5)
    assert d2.requires_grad and not face.requires_grad and not bary.requires_grad
    d2.backward(_dev(g))
    got = dict(d2=d2.detach(), face=face, bary=bary, dx=xt.grad, dp=pt.grad)
    for k, v in got.items():
        assert v.cpu().numpy().tobytes() == want[k].tobytes(), k


def test_refusals_launch_nothing():
    xs, faces, ps, ns = _small_case(1, 9, 128, seed=17)
    sd = _sd(faces, 66)
    xt, pt, nt = _dev(xs), _dev(ps), _dev(ns)
    sentinel = (torch.full((1, 9), 5.0, device=DEV), torch.full((1, 9), 5, dtype=torch.int32, device=DEV),
                torch.full((1, 9, 3), 5.0, device=DEV))
    for kw in (dict(normals=nt), dict(cos_min=0.5), dict(normals=nt, cos_min=float("nan")), dict(normals=nt.cpu(), cos_min=0.5),
               dict(normals=nt.double(), cos_min=0.5), dict(normals=nt[:, :8], cos_min=0.5), dict(normals=nt[:, :, :2], cos_min=0.5),
               dict(normals=ns, cos_min=0.5), dict(normals=torch.cat([nt, nt]), cos_min=0.5)):
        with pytest.raises(ValueError):
            sd.forward(xt, pt, out=sentinel, **kw)
        with pytest.raises(ValueError):
            sd.diff(xt, pt, **kw)
    for call in (lambda **kw: sd.forward(xt, pt, out=sentinel, **kw), lambda **kw: sd.diff(xt, pt, **kw)):
        with pytest.raises(RuntimeError):
            call(normals=nt.clone().requires_grad_(True), cos_min=0.5)
    torch.cuda.synchronize()
    assert all(bool((t == 5).all()) for t in sentinel)
    with pytest.raises(ValueError):
        sd.np(xs, ps, normals=ns[:, :8], cos_min=0.5)
    with pytest.raises(ValueError):
        sd.np(xs, [ps[0]], normals=[ns[0, :8]], cos_min=0.5)


def test_smpl_wrappers_equal_the_class_on_the_models_faces():
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
    sd = _sd(faces, body.V)
    want = sd.np(xs, pts, normals=nrm, cos_min=COS60)
    plain = sd.np(xs, pts)
    assert (want[1] != plain[1]).any() and (want[1][0] >= 0).any()
    got = body.scan_distance_np(xs, pts, normals=nrm, cos_min=COS60)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    padded, count = pad_points(pts)
    nt = _dev(pad_normals("normals", nrm, padded, count))
    xt, pt = _dev(xs), _dev(padded)
    dev_out = body.scan_distance(xt, pt, count, normals=nt, cos_min=COS60)
    assert dev_out[0].cpu().numpy().tobytes() == want[0].tobytes() and dev_out[1].cpu().numpy().tobytes() == want[1].tobytes()
    xg = xt.clone().requires_grad_(True)
    d2 = body.scan_distance_diff(xg, pt, count, normals=nt, cos_min=COS60)
    assert d2.detach().cpu().numpy().tobytes() == want[0].tobytes()
    d2.nan_to_num().sum().backward()
    seed = torch.isfinite(d2.detach()).float()
    with torch.no_grad():
        dx, _ = sd.backward(xt, pt, dev_out[1], dev_out[2], seed, want_dp=False)
    assert torch.equal(xg.grad, dx) and float(xg.grad.abs().max()) > 0
