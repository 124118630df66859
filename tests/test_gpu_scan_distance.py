"""Scan-to-mesh distance on the device (cape_amd/scan_distance.py, csrc/scan/scan_distance.hip) against the float64 brute force
of tests/scan_distance_reference.py, under tests/parity_bar.py's bar: each measure of the HIP path may be at most 4x the same
measure of the fp32 restatement (the brute force evaluated in float32), floor 4 * 2^-24.  R is the largest absolute coordinate
of a case; every point is compared, none is left out, and no face index is ever compared with the reference's (where two faces
tie either is right):
  1 distance       max |sqrt(d2) - sqrt(d2_min(fp64))| / R
  2 face validity  max (sqrt(d2_fp64(p, the path's face)) - sqrt(d2_min)) / R
  3 foot           max |bary . corners - foot_fp64 on the path's own face| / R
  4 gradient       vertex_err and whole-tensor relative L2 of dx and dp against the float64 formulas ON THE PATH'S OWN FACES, for a
                   random fp32 seed g
The restatement's own faces are used for its measures 3 and 4."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_distance_reference as R     # noqa: E402
from parity_bar import check            # noqa: E402

pytestmark = pytest.mark.gpu

T = 512            # scan_distance.hip FT: faces per LDS tile
B = 512            # scan_distance.hip PB: points per workgroup
SPLIT_MAX = 16     # scan_distance.hip SPLIT_MAX
DEV = "cuda"


def vertex_err(a, ref):
    """max per-row error norm / max per-row reference norm, as tests/test_gpu_vertex_normals.py defines it."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, ref.shape[-1])
    r = np.asarray(ref, dtype=np.float64).reshape(-1, ref.shape[-1])
    return np.sqrt(((a - r) ** 2).sum(-1)).max() / max(np.sqrt((r * r).sum(-1)).max(), 1e-30)


def rel_l2(a, ref):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.sqrt(((a - r) ** 2).sum() / max((r * r).sum(), 1e-300))


def _sd(faces, V):
    from cape_amd.scan_distance import ScanDistance
    return ScanDistance(faces, V)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a, order="C", copy=True), dtype=dtype).to(DEV)      # a copy: canonical strides for N = 1 too


def _run(sd, x, p, count=None, g=None):
    """forward (+ backward with the seed g) on numpy inputs [N, V, 3] / [N, M, 3]: dict of numpy outputs."""
    xt, pt = _dev(x), _dev(p)
    with torch.no_grad():
        d2, face, bary = sd.forward(xt, pt, count)
        out = dict(d2=d2.cpu().numpy(), face=face.cpu().numpy(), bary=bary.cpu().numpy())
        if g is not None:
            dx, dp = sd.backward(xt, pt, face, bary, _dev(g))
            out.update(dx=dx.cpu().numpy(), dp=dp.cpu().numpy())
    return out


def _reference(x, faces, p):
    """Per mesh [V, 3] and points [M, 3] (fp32 inputs): the float64 minimum and the fp32 restatement's own results."""
    f64, _, d64 = R.brute_force(x, faces, p)
    f32, foot32, d32 = R.brute_force(x, faces, p, np.float32)
    return dict(d64=d64, f64=f64, f32=f32, foot32=foot32, d32=d32)


@functools.lru_cache(maxsize=None)
def _template_reference(seed, shift, M):
    x, faces, p = R.template_case(seed, shift, M)
    ref = _reference(x, faces, p)
    for a in (x, faces, p) + tuple(ref.values()):
        a.setflags(write=False)
    return x, faces, p, ref


def _measures(tag, x, faces, p, out, g, ref=None, n=0):
    """Measures 1-4 of sample ``n`` of a run against the references of its mesh x [V, 3] and points p [M, 3]."""
    ref = ref or _reference(x, faces, p)
    Rm = float(max(np.nanmax(np.abs(x)), np.abs(p).max()))
    face, bary, d2 = out["face"][n].astype(np.int64), out["bary"][n].astype(np.float64), out["d2"][n].astype(np.float64)
    assert (face >= 0).all() and (face < len(faces)).all() and np.isfinite(d2).all() and np.isfinite(bary).all()
    assert (ref["f32"] >= 0).all()
    r64 = np.sqrt(ref["d64"])
    x64, p64 = x.astype(np.float64), p.astype(np.float64)
    _, _, foot_own, d_own = R.on_face(x64, faces, p64, face)
    _, _, foot_own32, d_own32 = R.on_face(x64, faces, p64, ref["f32"])
    errs = [np.abs(np.sqrt(d2) - r64).max() / Rm, (np.sqrt(d_own) - r64).max() / Rm,
            np.abs((bary[:, :, None] * x64[faces[face]]).sum(1) - foot_own).max() / Rm]
    errs32 = [np.abs(np.sqrt(ref["d32"].astype(np.float64)) - r64).max() / Rm, (np.sqrt(d_own32) - r64).max() / Rm,
              np.abs(ref["foot32"].astype(np.float64) - foot_own32).max() / Rm]
    names = ["distance", "face validity", "foot"]
    dx64, dp64 = R.gradients(x64, faces, p64, face, g[n].astype(np.float64))
    dx64r, dp64r = R.gradients(x64, faces, p64, ref["f32"], g[n].astype(np.float64))
    dx32, dp32 = R.gradients(x, faces, p, ref["f32"], g[n], np.float32)
    for name, mine, want, mine32, want32 in (("dx", out["dx"][n], dx64, dx32, dx64r), ("dp", out["dp"][n], dp64, dp32, dp64r)):
        assert np.isfinite(mine).all()
        errs += [vertex_err(mine, want), rel_l2(mine, want)]
        errs32 += [vertex_err(mine32, want32), rel_l2(mine32, want32)]
        names += [name + " (vertex_err)", name + " (rel L2)"]
    print("%s[%d] R %.2f: " % (tag, n, Rm) + "; ".join("%s %.2e [fp32 %.2e]" % t for t in zip(names, errs, errs32)))
    for name, e, e32 in zip(names, errs, errs32):
        check(tag, name, e, e32)


def _check_case(tag, xs, faces, ps, seed=0):
    """A batch of meshes xs [N, V, 3] and points ps [N, M, 3] (fp32) through all measures, sample by sample."""
    g = np.random.default_rng(seed).standard_normal(ps.shape[:2]).astype(np.float32)
    out = _run(_sd(faces, xs.shape[1]), xs, ps, None, g)
    for n in range(xs.shape[0]):
        _measures(tag, xs[n], faces, ps[n], out, g, n=n)
    return out


def _small_points(x, faces, M, seed):
    """fp32 points around the small mesh: near the surface on both sides, a quarter anywhere in the inflated box."""
    rng = np.random.default_rng(seed)
    p, nrm = R.surface_samples(rng, x.astype(np.float64), faces, M)
    p = p + rng.uniform(-0.05, 0.1, M)[:, None] * nrm
    far = rng.permutation(M)[:M // 4]
    p[far] = rng.uniform(x.min(0) - 0.3, x.max(0) + 0.3, (len(far), 3))
    return p.astype(np.float32)


def _small_batch(N, M, F, seed):
    """N different small meshes (the octahedron scaled, moved and perturbed per sample) with the faces repeated up to F rows."""
    rng = np.random.default_rng(seed)
    x0, f0 = R.octahedron()
    faces = np.concatenate([f0] * (F // len(f0) + 1))[:F]
    xs = np.stack([(x0 * rng.uniform(0.5, 1.5) + 0.01 * rng.standard_normal(x0.shape) + rng.uniform(-0.5, 0.5, 3)).astype(np.float32)
                   for _ in range(N)])
    ps = np.stack([_small_points(xs[n], f0, M, seed + 100 + n) for n in range(N)])
    return xs, faces, ps


# ---- tile edges --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F,M,N", [(128, 1, 1), (T, B - 1, 1), (T + 1, B, 3), (128, B + 1, 3), (T + 1, 1, 3)])
def test_tile_edges_on_the_small_mesh(F, M, N):
    xs, faces, ps = _small_batch(N, M, F, seed=F + M)
    assert _sd(faces, 66).plan(N, M)[1:] == (T, B)
    _check_case("scan_small_F%d_M%d_N%d" % (F, M, N), xs, faces, ps)


def test_face_split_factors_give_the_same_bits():
    """The split is a function of the sizes: one mesh of 16 face tiles with 512, 200 * 512 and 300 * 512 points selects 16, 2
    and 1 parts; the first 512 points are the same in all three and must come back bit for bit, and be right."""
    x, faces = R.octahedron(5)
    assert len(faces) == SPLIT_MAX * T
    x = x.astype(np.float32)[None]
    sd = _sd(faces, x.shape[1])
    sizes = (B, 200 * B, 300 * B)
    assert [sd.plan(1, M)[0] for M in sizes] == [SPLIT_MAX, 2, 1]
    rng = np.random.default_rng(8)
    p = (rng.standard_normal((1, sizes[-1], 3)) * 0.4).astype(np.float32)
    p[0, :B] = _small_points(x[0], faces, B, 9)
    outs = [_run(sd, x, p[:, :M]) for M in sizes]
    for k in ("face", "bary", "d2"):
        assert outs[0][k].tobytes() == outs[1][k][:, :B].tobytes() == outs[2][k][:, :B].tobytes(), k
        assert outs[1][k].tobytes() == outs[2][k][:, :sizes[1]].tobytes(), k
    g = np.random.default_rng(1).standard_normal((1, B)).astype(np.float32)
    full = _run(sd, x, p[:, :B], None, g)
    assert full["d2"].tobytes() == outs[0]["d2"].tobytes()
    _measures("scan_split", x[0], faces, p[0, :B], full, g)


# ---- counts, wide rows -------------------------------------------------------------------------------------------------------

def test_ragged_counts():
    M = 40
    xs, faces, ps = _small_batch(4, M, 128, seed=2)
    count = np.array([M, 1, 0, 7], np.int32)
    for n in range(4):
        ps[n, count[n]:] = np.nan                          # padding is never read
    sd = _sd(faces, 66)
    g = np.random.default_rng(3).standard_normal((4, M)).astype(np.float32)
    out = _run(sd, xs, ps, count, g)
    for n in range(4):
        c = count[n]
        assert (out["face"][n, c:] == -1).all() and not out["d2"][n, c:].any() and not out["bary"][n, c:].any()
        assert not out["dp"][n, c:].any()
        alone = _run(sd, xs[n:n + 1], ps[n:n + 1, :max(c, 1)], None if c else np.zeros(1, np.int32), g[n:n + 1, :max(c, 1)])
        for k in ("face", "bary", "d2", "dp"):
            assert out[k][n, :c].tobytes() == alone[k][0, :c].tobytes(), (n, k)
        assert out["dx"][n].tobytes() == alone["dx"][0].tobytes()
        if c:
            sub = {k: v[n:n + 1, :c] if k != "dx" else v[n:n + 1] for k, v in out.items()}
            _measures("scan_ragged", xs[n], faces, ps[n, :c], sub, g[n:n + 1, :c])
    assert not out["dx"][2].any()
    # count on the device, and count = None against a full count
    dev_count = _run(sd, xs, ps, torch.as_tensor(count).to(DEV), g)
    full = np.nan_to_num(ps)
    a, b = _run(sd, xs, full, None, g), _run(sd, xs, full, np.full(4, M, np.int32), g)
    for k in out:
        assert out[k].tobytes() == dev_count[k].tobytes() and a[k].tobytes() == b[k].tobytes(), k
    with pytest.raises(ValueError):
        sd.forward(_dev(xs), _dev(full), np.array([M, 1, 0, M + 1]))


def test_wide_rows():
    N, M = 2, 37
    xs, faces, ps = _small_batch(N, M, 128, seed=4)
    sd = _sd(faces, 66)
    g = np.random.default_rng(5).standard_normal((N, M)).astype(np.float32)
    want = _run(sd, xs, ps, None, g)
    x4, p4 = np.full((N, 66, 4), np.nan, np.float32), np.full((N, M, 5), np.nan, np.float32)
    x4[:, :, :3], p4[:, :, :3] = xs, ps
    xt, pt = _dev(x4)[:, :, :3], _dev(p4)[:, :, :3]
    dx4, dp4 = torch.full((N, 66, 4), 7.0, device=DEV), torch.full((N, M, 6), 7.0, device=DEV)
    with torch.no_grad():
        d2, face, bary = sd.forward(xt, pt)
        sd.backward(xt, pt, face, bary, _dev(g), dx=dx4[:, :, :3], dp=dp4[:, :, :3])
    got = dict(d2=d2, face=face, bary=bary, dx=dx4[:, :, :3], dp=dp4[:, :, :3])
    for k, v in got.items():
        assert v.cpu().numpy().tobytes() == want[k].tobytes(), k
    assert (dx4[:, :, 3] == 7.0).all() and (dp4[:, :, 3:] == 7.0).all()                  # padding never written


# ---- degenerate faces, non-finite points -------------------------------------------------------------------------------------

def test_degenerate_faces_never_win():
    M = 64
    xs, faces, ps = _small_batch(1, M, 2 * T + 7, seed=6)
    sd = _sd(faces, 66)
    g = np.random.default_rng(7).standard_normal((1, M)).astype(np.float32)
    base = _run(sd, xs, ps, None, g)
    for at in (None, T + 100):                             # appended, and in the middle of the second tile
        xn, fn = R.append_face(xs[0], faces, "nan", at=at)
        out = _run(_sd(fn, 69), xn[None], ps, None, g)
        pos = len(faces) if at is None else at
        assert (out["face"] != pos).all()
        assert np.array_equal(np.where(out["face"] > pos, out["face"] - 1, out["face"]), base["face"])
        for k in ("bary", "d2", "dp"):
            assert out[k].tobytes() == base[k].tobytes(), k
        assert out["dx"][0, :66].tobytes() == base["dx"].tobytes() and not out["dx"][0, 66:].any()
    # a collapsed face is the point it sits on (the rule's vertex region): right where it is closest, by the measures
    xc, fc = R.append_face(xs[0], faces, "collapsed", at=T + 100, where=ps[0, 3].astype(np.float64) + 1e-4)
    out = _run(_sd(fc, 69), xc[None], ps, None, g)
    assert out["face"][0, 3] == T + 100
    _measures("scan_collapsed", xc, fc, ps[0], out, g)
    # nothing but degenerate faces
    xa = np.full_like(xs, np.nan)
    xa[0, 0] = 0.0
    out = _run(sd, xa, ps, None, g)
    assert (out["face"] == -1).all() and np.isnan(out["d2"]).all() and not out["bary"].any()
    assert not out["dx"].any() and not out["dp"].any()


def test_a_point_with_a_nan_coordinate():
    M = 130
    xs, faces, ps = _small_batch(1, M, 128, seed=8)
    sd = _sd(faces, 66)
    g = np.random.default_rng(9).standard_normal((1, M)).astype(np.float32)
    base = _run(sd, xs, ps, None, g)
    bad = ps.copy()
    bad[0, 70, 1] = np.nan
    bad[0, 5, 2] = np.inf
    out = _run(sd, xs, bad, None, g)
    for i in (70, 5):
        assert out["face"][0, i] == -1 and np.isnan(out["d2"][0, i]) and not out["bary"][0, i].any() and not out["dp"][0, i].any()
    keep = np.setdiff1d(np.arange(M), (70, 5))            # the neighbours in the wave are unaffected
    for k in ("face", "bary", "d2", "dp"):
        assert out[k][0, keep].tobytes() == base[k][0, keep].tobytes(), k
    face = out["face"][0].astype(np.int64)
    dx64, _ = R.gradients(xs[0], faces, np.nan_to_num(bad[0], posinf=0.0), face, g[0])
    # the two points add nothing and poison nothing: fp32 results of fp64 sums, 2^-24 each, held to 1e-5
    assert np.isfinite(out["dx"]).all() and vertex_err(out["dx"][0], dx64) <= 1e-5


# ---- ties, determinism -------------------------------------------------------------------------------------------------------

def test_ties_and_determinism():
    x0, faces = R.octahedron()
    x = x0.astype(np.float32)
    rng = np.random.default_rng(10)
    planes = (rng.uniform(-0.8, 0.8, (60, 3)) * 1.0).astype(np.float32)
    planes[np.arange(60), np.arange(60) % 3] = 0.0          # on a symmetry plane: mirrored faces tie exactly
    planes[:6] *= np.eye(3, dtype=np.float32)[np.arange(6) % 3 - 1]   # on an axis: four or more faces tie
    ps = np.concatenate([planes, x])[None]                # and every mesh vertex itself
    M = ps.shape[1]
    xs2 = np.stack([x, (1.25 * x0 + 0.125).astype(np.float32)])
    ps2 = np.stack([ps[0], (1.25 * ps[0].astype(np.float64) + 0.125).astype(np.float32)])
    sd = _sd(faces, 66)
    g = rng.standard_normal((2, M)).astype(np.float32)
    out = _run(sd, xs2, ps2, None, g)
    for n in range(2):
        _measures("scan_ties", xs2[n], faces, ps2[n], out, g, n=n)
    at_vertex = slice(60, M)
    assert not out["d2"][0, at_vertex].any()               # exactly zero, and the barycentrics a unit vector
    assert np.abs(np.sort(out["bary"][0, at_vertex], 1) - np.array([0, 0, 1])).max() <= 2.0 ** -23
    again = _run(sd, xs2, ps2, None, g)
    swapped = _run(sd, xs2[::-1], ps2[::-1], None, g[::-1])
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k
        assert out[k].tobytes() == swapped[k][::-1].tobytes(), k


# ---- the template ------------------------------------------------------------------------------------------------------------

def _template_batch(seeds, shift, M=256):
    cases = [_template_reference(seed, shift, M) for seed in seeds]
    xs, ps = np.stack([c[0] for c in cases]), np.stack([c[2] for c in cases])
    return xs, cases[0][1], ps, [c[3] for c in cases]


@pytest.mark.parametrize("seeds,shift", [((3, 11), 0.0), ((5, 12), 3.0)])
def test_template_recipes(seeds, shift):
    """shift 3.0 is the translated body: a search in raw fp32 coordinates loses there; the sample-local one does not."""
    xs, faces, ps, refs = _template_batch(seeds, shift)
    g = np.random.default_rng(13).standard_normal(ps.shape[:2]).astype(np.float32)
    out = _run(_sd(faces, xs.shape[1]), xs, ps, None, g)
    for n in range(2):
        _measures("scan_template_shift%g" % shift, xs[n], faces, ps[n], out, g, ref=refs[n], n=n)
    on_surface = np.sqrt(out["d2"]) < 1e-6
    assert on_surface.sum() >= 20                          # points exactly on the surface are part of the recipe


# ---- autograd ----------------------------------------------------------------------------------------------------------------

def test_diff_matches_forward_and_the_backward_entry():
    N, M = 2, 50
    xs, faces, ps = _small_batch(N, M, 128, seed=14)
    sd = _sd(faces, 66)
    g = np.random.default_rng(15).standard_normal((N, M)).astype(np.float32)
    want = _run(sd, xs, ps, None, g)
    xt, pt = _dev(xs).requires_grad_(True), _dev(ps).requires_grad_(True)
    d2, face, bary = sd.diff(xt, pt, return_selection=True)
    assert d2.requires_grad and not face.requires_grad and not bary.requires_grad
    d2.backward(_dev(g))
    got = dict(d2=d2.detach(), face=face, bary=bary, dx=xt.grad, dp=pt.grad)
    for k, v in got.items():
        assert v.cpu().numpy().tobytes() == want[k].tobytes(), k
    # only the vertices: no dp is asked for; a loss downstream of d2
    x2 = _dev(xs).requires_grad_(True)
    (sd.diff(x2, _dev(ps)) * _dev(g)).sum().backward()
    assert x2.grad.cpu().numpy().tobytes() == want["dx"].tobytes()
    with pytest.raises(RuntimeError):
        sd.forward(xt, _dev(ps))
    with pytest.raises(RuntimeError):
        sd.forward(_dev(xs), pt)


def test_gradient_against_float64_finite_differences():
    """8 points 0.05 above the centroids of 8 faces of the small mesh: interior region, no tie near.  There d2 is smooth, so
    central differences of the float64 reference with h = 1e-5 are exact to h^2 |d2'''| + 1e-16 / h, about 1e-9 of the
    gradient; the device's fp32 results carry a few 2^-24.  Held to 1e-5 of the largest gradient entry."""
    x0, faces = R.octahedron()
    x = x0.astype(np.float32).astype(np.float64)
    pick = np.arange(8) * 16 + 3
    tri = x[faces[pick]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    p = (tri.mean(1) + 0.05 * nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    f64, _, _ = R.brute_force(x, faces, p)
    assert np.array_equal(f64, pick) and not R.on_face(x, faces, p, f64)[0].any()
    g = np.random.default_rng(16).uniform(0.5, 1.5, 8).astype(np.float32)
    loss = lambda xx, pp: float((g.astype(np.float64) * R.brute_force(xx, faces, pp)[2]).sum())
    xt, pt = _dev(x[None]).requires_grad_(True), _dev(p[None]).requires_grad_(True)
    sd = _sd(faces, 66)
    sd.diff(xt, pt).backward(_dev(g[None]))
    dx, dp = xt.grad.cpu().numpy()[0].astype(np.float64), pt.grad.cpu().numpy()[0].astype(np.float64)
    h = 1e-5
    fd_p, fd_x = np.zeros_like(p), np.zeros_like(x)
    for idx in np.ndindex(*p.shape):
        e = np.zeros_like(p)
        e[idx] = h
        fd_p[idx] = (loss(x, p + e) - loss(x, p - e)) / (2 * h)
    used = np.unique(faces[pick])
    for v in used:
        for k in range(3):
            e = np.zeros_like(x)
            e[v, k] = h
            fd_x[v, k] = (loss(x + e, p) - loss(x - e, p)) / (2 * h)
    print("finite differences: dp %.2e, dx %.2e of the largest entry" % (np.abs(dp - fd_p).max() / np.abs(fd_p).max(),
                                                                         np.abs(dx - fd_x).max() / np.abs(fd_x).max()))
    assert np.abs(dp - fd_p).max() <= 1e-5 * np.abs(fd_p).max()
    assert np.abs(dx - fd_x).max() <= 1e-5 * np.abs(fd_x).max()
    assert not np.delete(dx, used, axis=0).any()


def test_wrong_device_or_dtype_is_refused_and_nothing_is_launched():
    xs, faces, ps = _small_batch(1, 9, 128, seed=17)
    sd = _sd(faces, 66)
    xt, pt = _dev(xs), _dev(ps)
    sentinel = (torch.full((1, 9), 5.0, device=DEV), torch.full((1, 9), 5, dtype=torch.int32, device=DEV),
                torch.full((1, 9, 3), 5.0, device=DEV))
    for bx, bp in ((xt.cpu(), pt), (xt, pt.cpu()), (xt.double(), pt), (xt, pt.double()), (xt[:, :60], pt), (xt, pt[:, :, :2]),
                   (xs, pt), (xt, torch.cat([pt, pt]))):
        with pytest.raises(ValueError):
            sd.forward(bx, bp, out=sentinel)
        with pytest.raises(ValueError):
            sd.diff(bx, bp)
    with pytest.raises(ValueError):
        sd.forward(xt, pt, out=(sentinel[0], sentinel[1].long(), sentinel[2]))
    torch.cuda.synchronize()
    assert all(bool((t == 5).all()) for t in sentinel)


def test_smpl_wrappers_equal_the_class_on_the_models_faces():
    import smpl_synth as synth
    from cape_amd import smpl
    m = synth.smpl_like()
    body = smpl.SMPL(m)
    assert body._scan is None
    faces = np.asarray(m["f"], dtype=np.int64)
    rng = np.random.default_rng(18)
    xs = (m["v_template"][None] + 0.003 * rng.standard_normal((2, body.V, 3))).astype(np.float32)
    pts = [R.surface_samples(rng, xs[n].astype(np.float64), faces, m_n)[0].astype(np.float32) + np.float32(0.01)
           for n, m_n in enumerate((90, 33))]
    sd = _sd(faces, body.V)
    want = sd.np(xs, pts)
    got = body.scan_distance_np(xs, pts)
    assert body._scan is not None
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert (got[1][1, 33:] == -1).all() and (got[1][0] >= 0).all()
    from cape_amd.scan_distance import pad_points
    padded, count = pad_points(pts)
    xt, pt = _dev(xs), _dev(padded)
    dev_out = body.scan_distance(xt, pt, count)
    assert dev_out[0].cpu().numpy().tobytes() == want[0].tobytes()
    xg = xt.clone().requires_grad_(True)
    d2 = body.scan_distance_diff(xg, pt, count)
    assert d2.detach().cpu().numpy().tobytes() == want[0].tobytes()
    d2.sum().backward()
    with torch.no_grad():
        dx, _ = sd.backward(xt, pt, dev_out[1], dev_out[2], torch.ones_like(d2), want_dp=False)
    assert torch.equal(xg.grad, dx) and float(xg.grad.abs().max()) > 0
