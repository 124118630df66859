"""Scan-to-mesh distance on the host: the brute-force reference the GPU tests use (tests/scan_distance_reference.py) against
``closest_points_on_mesh`` and against torch autograd, the C-ABI's declarations and argument checks (decided before any launch),
and what ``ScanDistance`` and its argument handling refuse.  None of this needs a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_distance_reference as R     # noqa: E402

ENTRIES = ("cape_scan_distance_workspace_bytes", "cape_scan_distance_plan", "cape_scan_nearest_fwd", "cape_scan_nearest_bwd")


def _points_near(x, faces, M, seed):
    rng = np.random.default_rng(seed)
    p, nrm = R.surface_samples(rng, x, faces, M)
    p = p + rng.uniform(-0.05, 0.1, M)[:, None] * nrm
    p[::4] = rng.uniform(x.min(0) - 0.3, x.max(0) + 0.3, (len(p[::4]), 3))
    return p


# ---- the references themselves -----------------------------------------------------------------------------------------------

def _assert_equals_kdtree(x, faces, p):
    from cape_amd.mesh_operators import closest_points_on_mesh
    face, foot, d2 = R.brute_force(x, faces, p)
    kf, kpart, kfoot = closest_points_on_mesh(x, faces, p)
    kd = np.sqrt(((p - kfoot) ** 2).sum(-1))
    assert np.abs(np.sqrt(d2) - kd).max() <= 1e-12 and np.abs(foot - kfoot).max() <= 1e-9
    part, bary, ofoot, od2 = R.on_face(x, faces, p, face)
    assert np.abs(ofoot - foot).max() <= 1e-12 and np.abs(od2 - d2).max() <= 1e-14
    assert np.abs(bary.sum(1) - 1).max() <= 1e-12 and bary.min() >= -1e-12
    same = kf == face                                     # where both picked one face the region must agree too
    assert same.mean() > 0.5 and np.array_equal(part[same], kpart[same])
    return part


def test_brute_force_equals_closest_points_on_mesh_small_mesh():
    x, faces = R.octahedron()
    assert x.shape == (66, 3) and faces.shape == (128, 3)
    part = _assert_equals_kdtree(x, faces, np.concatenate([_points_near(x, faces, 400, 1), 1.3 * x]))   # 1.3 x: beyond a vertex
    assert set(np.unique(part)) == set(range(7))          # every region occurs


def test_brute_force_equals_closest_points_on_mesh_template():
    x, faces, p = R.template_case(3, 0.0, 64)
    _assert_equals_kdtree(x.astype(np.float64), faces, p.astype(np.float64))


def test_fp32_restatement_is_close_and_degenerate_faces_never_win():
    x, faces = R.octahedron()
    x = x.astype(np.float32)                                # every path sees the same fp32 inputs
    p = _points_near(x.astype(np.float64), faces, 200, 2).astype(np.float32)
    f64, _, d64 = R.brute_force(x, faces, p)
    f32, foot32, d32 = R.brute_force(x, faces, p, np.float32)
    assert d32.dtype == np.float32 and foot32.dtype == np.float32
    assert np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(d64)).max() <= 1e-6
    xn, fn = R.append_face(x, faces, "nan", at=40)
    fa, _, da = R.brute_force(xn, fn, p.astype(np.float64))
    assert (fa != 40).all() and np.array_equal(np.where(fa > 40, fa - 1, fa), f64) and np.array_equal(da, d64)
    none, _, dn = R.brute_force(np.full((3, 3), np.nan), np.array([[0, 1, 2]]), p[:5])
    assert (none == -1).all() and np.isnan(dn).all()
    xc, fc = R.append_face(x, faces, "collapsed", where=p[7])          # a collapsed face IS a point: it wins where it is
    fw, _, dw = R.brute_force(xc, fc, p[7:8].astype(np.float64))
    assert fw[0] == len(faces) and dw[0] == 0.0


def test_gradient_formulas_equal_autograd_with_the_selection_fixed():
    x, faces = R.octahedron()
    p = np.concatenate([_points_near(x, faces, 300, 3), 1.3 * x])
    face, _, _ = R.brute_force(x, faces, p)
    part, _, _, _ = R.on_face(x, faces, p, face)
    assert set(np.unique(part)) == set(range(7))
    g = np.random.default_rng(4).standard_normal(len(p))
    dx, dp = R.gradients(x, faces, p, face, g)
    xt, pt = torch.tensor(x, requires_grad=True), torch.tensor(p, requires_grad=True)
    tri = xt[torch.as_tensor(faces[face])]
    _, _, _, d2 = R.rule(tri[:, 0], tri[:, 1], tri[:, 2], pt, part=torch.as_tensor(part))
    (d2 * torch.as_tensor(g)).sum().backward()
    assert np.abs(xt.grad.numpy() - dx).max() <= 1e-12 * np.abs(dx).max()
    assert np.abs(pt.grad.numpy() - dp).max() <= 1e-12 * np.abs(dp).max()
    # a point without a face adds nothing
    face[5] = -1
    dx2, dp2 = R.gradients(x, faces, p, face, g)
    assert not dp2[5].any() and np.abs(dx2 - dx).max() > 0


# ---- C-ABI -------------------------------------------------------------------------------------------------------------------

def test_entries_declared_bound_and_exported():
    from cape_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    assert int(re.search(r"#define CAPE_ABI_VERSION (\d+)", hdr).group(1)) == 18 and _lib.lib.cape_abi_version() == 18
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    assert _lib.SIGNATURES[ENTRIES[0]][0] is ctypes.c_int64
    assert all(_lib.SIGNATURES[n][0] is ctypes.c_int for n in ENTRIES[1:])
    mk = open(os.path.join(ROOT, "cape_amd", "csrc", "Makefile")).read()
    assert "scan/scan_distance.o" in mk and os.path.exists(os.path.join(ROOT, "cape_amd", "csrc", "scan", "scan_distance.hip"))


def _plan(N, F, M):
    from cape_amd._lib import lib
    out = (ctypes.c_int32 * 3)()
    assert lib.cape_scan_distance_plan(N, F, M, out) == 0
    return tuple(out)


def test_workspace_bytes_and_plan():
    from cape_amd._lib import lib
    wb = lib.cape_scan_distance_workspace_bytes
    N, V, F, M = 2, 6890, 13776, 20000
    split, T, B = _plan(N, F, M)
    assert (T, B) == (512, 512) and split >= 1
    # forward: a 64-byte record per (sample, face) and 8 bytes per (part, point); backward: 64 bytes per point
    assert wb(N, V, F, M) == max(N * F * 64 + split * N * M * 8, N * M * 64)
    assert wb(1, 3, 1, 1000) == max(64 + 8000, 64000)                                  # the backward's share decides
    for bad in ((0, V, F, M), (N, 0, F, M), (N, V, 0, M), (N, V, F, 0), (-1, V, F, M)):
        assert wb(*bad) == -1, bad
    assert wb(65536, 1, 1, 32768) == -1 and wb(65536, 1, 1, 32767) > 0                 # N M = 2^31
    assert wb(65536, 32768, 1, 1) == -1                                                # N V = 2^31
    assert wb(1, 3, 715827883, 1) == -1 and wb(1, 3, 715827882, 1) > 0                 # 3 F = 2^31 + 1 / 2^31 - 2
    out = (ctypes.c_int32 * 3)()
    assert lib.cape_scan_distance_plan(0, F, M, out) == -1 and lib.cape_scan_distance_plan(1, F, M, None) == -1
    # the split is a function of the sizes: few workgroups -> the faces are shared out, many -> one walk
    assert _plan(1, F, 8)[0] == 14 and _plan(1, 16 * 512, 8)[0] == 16 and _plan(1, 16 * 512, 200 * 512)[0] == 2 and _plan(1, 16 * 512, 300 * 512)[0] == 1
    assert _plan(1, 128, 8)[0] == 1 and _plan(1, 513, 8)[0] == 2 and _plan(16, F, 20000)[0] == 1


def test_entries_reject_bad_arguments_before_launching():
    from cape_amd._lib import lib
    P = ctypes.c_void_p
    N, V, F, M = 2, 6890, 13776, 1000
    need = int(lib.cape_scan_distance_workspace_bytes(N, V, F, M))

    def fwd(**kw):
        a = dict(x=P(0x100000), ldx=4, faces=P(0x200000), points=P(0x300000), ldp=3, count=None, N=N, V=V, F=F, M=M,
                 face=P(0x400000), bary=P(0x500000), d2=P(0x600000), ws=P(0x800000), need=need)
        a.update(kw)
        return lib.cape_scan_nearest_fwd(a["x"], a["ldx"], a["faces"], a["points"], a["ldp"], a["count"], a["N"], a["V"], a["F"],
                                         a["M"], a["face"], a["bary"], a["d2"], a["ws"], a["need"], None)

    def bwd(**kw):
        a = dict(x=P(0x100000), ldx=4, faces=P(0x200000), points=P(0x300000), ldp=3, face=P(0x400000), bary=P(0x500000),
                 g=P(0x600000), N=N, V=V, F=F, M=M, dx=P(0x700000), ldd=3, dp=None, lddp=3, ws=P(0x800000), need=need)
        a.update(kw)
        return lib.cape_scan_nearest_bwd(a["x"], a["ldx"], a["faces"], a["points"], a["ldp"], a["face"], a["bary"], a["g"], a["N"],
                                         a["V"], a["F"], a["M"], a["dx"], a["ldd"], a["dp"], a["lddp"], a["ws"], a["need"], None)

    for name in ("x", "faces", "points", "face", "bary", "d2", "ws"):
        assert fwd(**{name: None}) == -1, name
    for name in ("x", "faces", "points", "face", "bary", "g", "dx", "ws"):
        assert bwd(**{name: None}) == -1, name
    for call in (fwd, bwd):
        for size in ("N", "V", "F", "M"):
            assert call(**{size: 0}) == -1 and call(**{size: -1}) == -1, size
        assert call(ldx=2) == -1 and call(ldp=2) == -1
        assert call(N=65536, M=32768) == -1                                                # N M = 2^31
        assert call(N=65536, V=32768, M=1) == -1                                           # N V = 2^31
        assert call(F=715827883) == -1                                                     # 3 F = 2^31 + 1
        assert call(ws=P(0x800008)) == -1                                                  # not 16-byte aligned
        assert call(need=0) == -1
    assert fwd(need=N * F * 64 + N * M * 8 - 8) == -1                                      # a short workspace
    assert bwd(need=N * M * 64 - 8) == -1
    assert bwd(ldd=2) == -1 and bwd(dp=P(0x900000), lddp=2) == -1


# ---- ScanDistance ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["shape", "float", "negative", "too_large", "repeated", "empty"])
def test_bad_faces(bad):
    from cape_amd.scan_distance import ScanDistance
    _, f = R.octahedron(1)
    f = f.copy()
    if bad == "shape":
        f = f[:, :2]
    elif bad == "float":
        f = f.astype(np.float64)
    elif bad == "negative":
        f[5, 1] = -1
    elif bad == "too_large":
        f[7, 2] = 18
    elif bad == "repeated":
        f[3, 2] = f[3, 0]
    else:
        f = f[:0]
    with pytest.raises(ValueError):
        ScanDistance(f, 18)


def test_bad_count_and_bad_points():
    from cape_amd.scan_distance import _count, _points, pad_points
    cpu = torch.device("cpu")
    host, dev = _count([3, 0, 5], 3, 5, cpu)
    assert host.dtype == np.int32 and dev.dtype == torch.int32 and dev.tolist() == [3, 0, 5]
    assert _count(None, 3, 5, cpu) == (None, None)
    assert _count(torch.tensor([1, 2, 3], dtype=torch.int32), 3, 5, cpu)[1].tolist() == [1, 2, 3]
    for bad in ([3, 0, 6], [3, -1, 5], [3, 0], [[3, 0, 5]], [3.0, 0.0, 5.0], torch.tensor([1, 2, 9])):
        with pytest.raises(ValueError):
            _count(bad, 3, 5, cpu)
    t = torch.zeros(2, 7, 3)
    assert _points("points", t, 2, cpu) == (7, 3)
    assert _points("points", torch.zeros(2, 7, 4)[:, :, :3], 2, cpu) == (7, 4)
    for bad, dev in ((t, torch.device("cuda", 0)), (t.double(), cpu), (t.numpy(), cpu), (t[:1], cpu), (t[:, :0], cpu), (t[0], cpu),
                     (torch.zeros(2, 3, 7).transpose(1, 2), cpu), (torch.zeros(4, 7, 3)[::2], cpu)):
        with pytest.raises(ValueError):
            _points("points", bad, 2, dev)
    pts, count = pad_points([np.zeros((4, 3)), np.ones((1, 3)), np.ones((6, 3))])
    assert pts.shape == (3, 6, 3) and pts.dtype == np.float32 and count.tolist() == [4, 1, 6]
    assert pts[1, 0].tolist() == [1, 1, 1] and not pts[1, 1:].any()
    assert pad_points(np.zeros((2, 5, 3)))[1] is None
    for bad in ([], [np.zeros((4, 3)), np.zeros((0, 3))], [np.zeros((4, 2))], [np.zeros(3)], np.zeros((2, 0, 3)), np.zeros((5, 3)),
                np.zeros((2, 5, 4))):
        with pytest.raises(ValueError):
            pad_points(bad)


def test_tables_and_wrappers_are_built_lazily():
    import smpl_synth as synth
    from cape_amd import smpl
    from cape_amd.scan_distance import ScanDistance
    _, f = R.octahedron(1)
    sd = ScanDistance(f, 18)
    assert sd.faces.dtype == np.int32 and np.array_equal(sd.faces, f) and (sd.V, sd.F) == (18, 32) and sd._dev is None
    assert sd.plan(1, 8) == (1, 512, 512)
    m = dict(synth.small())
    m["f"] = np.zeros((4, 3), np.int64)                   # no triangle list: nothing looks until a distance is asked for
    body = smpl.SMPL(m)
    assert body._scan is None
    with pytest.raises(ValueError):
        body.scan_distance_np(np.zeros((1, body.V, 3), np.float32), np.zeros((1, 4, 3), np.float32))


def test_no_cpu_fallback(monkeypatch):
    from cape_amd._lib import CapeHipError
    from cape_amd.scan_distance import ScanDistance
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x, f = R.octahedron(1)
    sd = ScanDistance(f, 18)
    xt, pt = torch.tensor(x[None], dtype=torch.float32), torch.zeros(1, 4, 3)
    with pytest.raises(CapeHipError):
        sd.forward(xt, pt)
    with pytest.raises(CapeHipError):
        sd.diff(xt.requires_grad_(True), pt)
    with pytest.raises(CapeHipError):
        sd.np(x, np.zeros((4, 3)))
