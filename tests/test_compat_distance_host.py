"""Host-side checks of the normal-compatible searches: tests/compat_distance_reference.py against the plain brute
forces and on a hand-made case, the ambiguity condition of the GPU tests' template recipes (so a bad recipe is caught without a
GPU), the C-ABI's declarations and argument checks (decided before any launch), and what the Python layer decides before it
touches the device."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compat_distance_reference as C   # noqa: E402
import point_distance_reference as P    # noqa: E402
import scan_distance_reference as R     # noqa: E402

ENTRIES = ("cape_scan_distance_compat_workspace_bytes", "cape_scan_nearest_compat_fwd", "cape_point_nearest_compat_fwd")
COS = [float(np.cos(np.deg2rad(a))) for a in (30.0, 60.0)] + [0.0]


# ---- the reference -------------------------------------------------------------------------------------------------------------

def _small(seed, M=40):
    rng = np.random.default_rng(seed)
    x0, faces = R.octahedron()
    x = (x0 + 0.01 * rng.standard_normal(x0.shape)).astype(np.float32)
    p, nrm = R.surface_samples(rng, x.astype(np.float64), faces, M)
    p = (p + rng.uniform(-0.05, 0.1, M)[:, None] * nrm).astype(np.float32)
    return x, faces, p, C.noisy_normals(rng, nrm).astype(np.float32)


def test_without_a_filter_the_reference_is_the_plain_brute_force():
    x, faces, p, nrm = _small(1)
    xn, fn = R.append_face(*R.append_face(x, faces, "collapsed", at=5, where=p[3].astype(np.float64)), "nan")
    for xx, ff in ((x, faces), (xn, fn)):
        ref = C.scan_search(C.scan_tables(xx, ff, p, nrm), -2.0)
        f64, _, d64 = R.brute_force(xx, ff, p)
        f32, foot32, d32 = R.brute_force(xx, ff, p, np.float32)
        assert np.array_equal(ref["sure_id"], f64) and np.array_equal(ref["maybe_id"], f64) and np.array_equal(ref["sure"], d64)
        assert np.array_equal(ref["id32"], f32) and np.array_equal(ref["d32"], d32) and np.array_equal(ref["foot32"], foot32)
        assert not ref["ambiguous"].any()
    vn = C.vertex_normals(x, faces).astype(np.float32)
    ref = C.point_search(C.point_tables(x, p, vn, nrm), -2.0)
    i64, e64 = P.brute_force(x, p)
    i32, e32 = P.brute_force(x, p, np.float32)
    assert np.array_equal(ref["sure_id"], i64) and np.array_equal(ref["sure"], e64) and np.array_equal(ref["maybe"], e64)
    assert np.array_equal(ref["id32"], i32) and np.array_equal(ref["d32"], e32)


def test_the_band_on_three_faces():
    """Three parallel triangles 1, 2 and 3 below the point, all with the normal +z: the point's normal sets one cosine for the
    three; then cosines per face -- about 0.2, one within the band of the threshold 0.5 or just outside it, and 0.9."""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    p = np.array([[0.2, 0.2, 0.0]], np.float32)
    x = np.concatenate([tri - [0, 0, k + 1.0] for k in range(3)]).astype(np.float32)
    faces = np.arange(9).reshape(3, 3)
    assert np.array_equal(C.face_normals(x, faces), np.tile([0.0, 0, 1], (3, 1)))
    for c, (sure, maybe) in ((0.95, (0, 0)), (0.5 + 5e-6, (-1, 0)), (0.5 - 5e-6, (-1, 0)), (0.5 + 2e-5, (0, 0)), (0.5 - 2e-5, (-1, -1))):
        ref = C.scan_search(C.scan_tables(x, faces, p, np.array([[np.sqrt(1 - c * c), 0.0, c]])), 0.5)
        assert (ref["sure_id"][0], ref["maybe_id"][0]) == (sure, maybe), c
        assert ref["ambiguous"][0] == (sure != maybe)
        if sure == 0:
            assert ref["sure"][0] == 1.0
    # per-face cosines: face 0 incompatible, face 1 in the band, face 2 compatible -- sure takes 2, maybe takes 1
    d = np.array([[1.0, 4.0, 9.0]])
    for c_mid, want in ((0.5 + 5e-6, (2, 1, True)), (0.5 + 2e-5, (1, 1, False)), (0.5 - 2e-5, (2, 2, False))):
        c64 = np.array([[0.2, c_mid, 0.9]])
        ref = C._search(d, c64, d.astype(np.float32), c64.astype(np.float32), 0.5, C.DELTA)
        assert (ref["sure_id"][0], ref["maybe_id"][0], bool(ref["ambiguous"][0])) == want, c_mid
        assert ref["maybe"][0] <= ref["sure"][0]
    # a NaN or inf normal on either side is compatible with nothing, whatever the threshold
    bad = C.cosines(np.array([[np.nan, 0, 1], [np.inf, 0, 0], [0, 0, 1.0]]), np.array([[0, 0, 1.0], [0, -np.inf, 0]]))
    assert np.isnan(bad[:2]).all() and np.isnan(bad[2, 1]) and bad[2, 0] == 1.0
    assert C.masked_min(np.ones((3, 2)), bad >= -np.inf)[0].tolist() == [-1, -1, 0]
    # a collapsed and a NaN face have the normal (0, 0, 0)
    xz = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    assert not C.face_normals(xz, np.array([[0, 1, 2], [3, 4, 5]])).any()


@pytest.mark.parametrize("seed,shift", [(3, 0.0), (5, 3.0)])
def test_the_template_recipes_are_not_all_band(seed, shift):
    """The condition the GPU tests assert, here at the ten times wider band 1e-4: next to no query is ambiguous, and the filter
    changes the result of many."""
    x, faces, p, nrm = C.template_case(seed, shift, 256)
    x2, faces2, p2 = R.template_case(seed, shift, 256)
    assert np.array_equal(x, x2) and np.array_equal(p, p2) and np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-6
    tables = C.scan_tables(x, faces, p, nrm)
    _, _, plain = R.brute_force(x, faces, p)
    for cos_min in COS:
        ref = C.scan_search(tables, cos_min, 1e-4)
        changed = int((ref["sure"] != plain).sum())
        print("scan-to-mesh seed %d cos_min %.3f: %d ambiguous, %d changed" % (seed, cos_min, ref["ambiguous"].sum(), changed))
        assert ref["ambiguous"].sum() == 0 and 40 <= changed <= 200
    x, faces, p, pn = C.template_case(seed, shift, 2049)
    vn = C.vertex_normals(x, faces).astype(np.float32)
    tables = C.point_tables(x, p, vn, pn)
    _, plain = P.brute_force(x, p)
    for cos_min in COS:
        ref = C.point_search(tables, cos_min, 1e-4)
        changed = int((ref["sure"] != plain).sum())
        print("mesh-to-scan seed %d cos_min %.3f: %d ambiguous, %d changed" % (seed, cos_min, ref["ambiguous"].sum(), changed))
        assert ref["ambiguous"].sum() <= 20 and 1000 <= changed <= 6000


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
    # the plain entries' arguments plus (normals, ldn, cos_min) and (query_normals, ldqn, point_normals, ldpn, cos_min)
    assert len(_lib.SIGNATURES["cape_scan_nearest_compat_fwd"][1]) == len(_lib.SIGNATURES["cape_scan_nearest_fwd"][1]) + 3
    assert len(_lib.SIGNATURES["cape_point_nearest_compat_fwd"][1]) == len(_lib.SIGNATURES["cape_point_nearest_fwd"][1]) + 5
    mk = open(os.path.join(ROOT, "cape_amd", "csrc", "Makefile")).read()
    for obj in ("scan/scan_distance.o", "scan/point_distance.o"):
        assert re.search(r"^%s:.*scan/nearest\.h" % re.escape(obj), mk, re.M), obj


def test_the_compat_workspace_holds_80_byte_records():
    from cape_amd._lib import lib
    wb, wc = lib.cape_scan_distance_workspace_bytes, lib.cape_scan_distance_compat_workspace_bytes
    plan = (ctypes.c_int32 * 3)()
    for N, V, F, M in ((1, 66, 128, 1), (3, 6890, 13776, 256), (1, 4098, 8192, 512), (2, 66, 513, 100000)):
        assert lib.cape_scan_distance_plan(N, F, M, plan) == 0
        fwd, bwd = N * F * 80 + 8 * plan[0] * N * M, N * M * 64
        assert wc(N, V, F, M) == max(fwd, bwd), (N, V, F, M)
        assert wc(N, V, F, M) >= wb(N, V, F, M)                                            # the plain backward fits
    for bad in ((0, 5, 5, 5), (5, 0, 5, 5), (5, 5, 0, 5), (5, 5, 5, 0), (65536, 5, 5, 32768)):
        assert wc(*bad) == -1, bad


def test_entries_reject_bad_arguments_before_launching():
    """No device here: a launch would fail with another code, so -1 shows the refusal came first."""
    from cape_amd._lib import lib
    A = ctypes.c_void_p
    N, V, F, M, Q = 2, 66, 1024, 100, 66
    need = int(lib.cape_scan_distance_compat_workspace_bytes(N, V, F, M))
    plain = int(lib.cape_scan_distance_workspace_bytes(N, V, F, M))
    assert plain < need

    def scan(**kw):
        a = dict(x=A(0x100000), ldx=3, faces=A(0x200000), points=A(0x300000), ldp=3, normals=A(0x500000), ldn=4, cos_min=0.5,
                 count=None, N=N, V=V, F=F, M=M, face=A(0x400000), bary=A(0x600000), d2=A(0x700000), ws=A(0x800000), need=need)
        a.update(kw)
        return lib.cape_scan_nearest_compat_fwd(a["x"], a["ldx"], a["faces"], a["points"], a["ldp"], a["normals"], a["ldn"],
                                                a["cos_min"], a["count"], a["N"], a["V"], a["F"], a["M"], a["face"], a["bary"],
                                                a["d2"], a["ws"], a["need"], None)

    for name in ("x", "faces", "points", "normals", "face", "bary", "d2", "ws"):
        assert scan(**{name: None}) == -1, name
    for size in ("N", "V", "F", "M"):
        assert scan(**{size: 0}) == -1 and scan(**{size: -1}) == -1, size
    assert scan(ldx=2) == -1 and scan(ldp=2) == -1 and scan(ldn=2) == -1
    assert scan(cos_min=float("nan")) == -1
    assert scan(N=65536, M=32768) == -1                                                    # N M = 2^31
    assert scan(ws=A(0x800008)) == -1 and scan(need=0) == -1 and scan(need=need - 8) == -1
    assert scan(need=plain) == -1                                                          # the plain entry's workspace is short

    pneed = int(lib.cape_point_distance_workspace_bytes(N, Q, M))
    plan = (ctypes.c_int32 * 3)()
    assert lib.cape_point_distance_plan(N, Q, M, plan) == 0

    def point(**kw):
        a = dict(q=A(0x100000), ldq=4, points=A(0x300000), ldp=3, qn=A(0x200000), ldqn=3, pn=A(0x500000), ldpn=5, cos_min=0.0,
                 count=None, N=N, Q=Q, M=M, index=A(0x400000), d2=A(0x600000), ws=A(0x800000), need=pneed)
        a.update(kw)
        return lib.cape_point_nearest_compat_fwd(a["q"], a["ldq"], a["points"], a["ldp"], a["qn"], a["ldqn"], a["pn"], a["ldpn"],
                                                 a["cos_min"], a["count"], a["N"], a["Q"], a["M"], a["index"], a["d2"], a["ws"],
                                                 a["need"], None)

    for name in ("q", "points", "qn", "pn", "index", "d2", "ws"):
        assert point(**{name: None}) == -1, name
    for size in ("N", "Q", "M"):
        assert point(**{size: 0}) == -1 and point(**{size: -1}) == -1, size
    assert point(ldq=2) == -1 and point(ldp=2) == -1 and point(ldqn=2) == -1 and point(ldpn=2) == -1
    assert point(cos_min=float("nan")) == -1
    assert point(N=65536, Q=32768, M=1) == -1 and point(N=65536, Q=1, M=32768) == -1
    assert point(ws=A(0x800008)) == -1 and point(need=0) == -1 and point(need=8 * plan[0] * N * Q - 8) == -1


# ---- the Python layer, before the device ---------------------------------------------------------------------------------------

def test_a_list_of_normal_arrays_is_padded_as_the_points_are():
    from cape_amd.scan_distance import pad_normals, pad_points
    rng = np.random.default_rng(0)
    pts = [rng.standard_normal((m, 3)) for m in (5, 2, 9)]
    nrm = [rng.standard_normal((m, 3)) for m in (5, 2, 9)]
    padded, count = pad_points(pts)
    out = pad_normals("normals", nrm, padded, count)
    want, count2 = pad_points(nrm)
    assert out.dtype == np.float32 and out.tobytes() == want.tobytes() and np.array_equal(count, count2)
    for n, m in enumerate((5, 2, 9)):
        assert np.array_equal(out[n, :m], nrm[n].astype(np.float32)) and not out[n, m:].any()
    # an array for a list of equal lengths and the reverse; one sample as [M, 3]
    same = [rng.standard_normal((4, 3)) for _ in range(2)]
    p2, c2 = pad_points(same)
    assert pad_normals("normals", np.stack(same), p2, c2).tobytes() == p2.tobytes()
    p3, c3 = pad_points(np.stack(same))
    assert c3 is None and pad_normals("normals", same, p3, c3).tobytes() == p3.tobytes()
    assert pad_normals("normals", same[0], p3[:1], None).shape == (1, 4, 3)
    for bad in (nrm[:2], [nrm[0], nrm[1], nrm[2][:8]], [nrm[1], nrm[0], nrm[2]], np.zeros((3, 9, 3)), np.zeros((3, 9, 2)),
                [a[:, :2] for a in nrm], []):
        with pytest.raises(ValueError, match="normals"):
            pad_normals("normals", bad, padded, count)


def test_all_of_the_filter_or_none_is_decided_before_the_device():
    from cape_amd.point_distance import PointDistance
    from cape_amd.scan_distance import NearestDistance, ScanDistance
    n = torch.zeros(1, 5, 3)
    assert NearestDistance._compat(None, normals=None) is None
    assert NearestDistance._compat(0.5, normals=n)[0] == 0.5 and NearestDistance._compat(-float("inf"), normals=n)[1] is n
    for kw in (dict(normals=n), dict(cos_min=0.5), dict(normals=n, cos_min=float("nan"))):
        with pytest.raises(ValueError):
            NearestDistance._compat(kw.get("cos_min"), normals=kw.get("normals"))
    with pytest.raises(RuntimeError):
        NearestDistance._compat(0.5, normals=n.clone().requires_grad_(True))
    x0, faces = R.octahedron()
    sd, pd = ScanDistance(faces, 66), PointDistance()
    xt, pt = torch.zeros(1, 66, 3), torch.zeros(1, 5, 3)
    for call in (sd.forward, sd.diff, sd):
        with pytest.raises(ValueError):
            call(xt, pt, normals=n)
        with pytest.raises(ValueError):
            call(xt, pt, cos_min=0.0)
    for call in (pd.forward, pd.diff, pd):
        for kw in (dict(query_normals=xt), dict(point_normals=n), dict(cos_min=0.0), dict(query_normals=xt, point_normals=n),
                   dict(query_normals=xt, cos_min=0.0), dict(point_normals=n, cos_min=0.0)):
            with pytest.raises(ValueError):
                call(xt, pt, **kw)
    assert sd._dev is None and pd._dev is None                                             # nothing touched the device
    with pytest.raises(ValueError):
        sd.np(x0, np.zeros((5, 3)), normals=np.zeros((5, 3)))
    with pytest.raises(ValueError):
        pd.np(x0, np.zeros((5, 3)), point_normals=np.zeros((5, 3)), cos_min=0.0)


def test_fit_scan_refuses_the_normal_arguments_before_anything_else():
    from cape_amd.models import CAPE
    me = types.SimpleNamespace(batch_size=2, nz=4)           # no device, no variables
    body = types.SimpleNamespace(V=6)
    scan = np.zeros((2, 5, 3), np.float32)
    nrm = np.zeros((2, 5, 3), np.float32)
    ragged = [np.zeros((5, 3), np.float32), np.zeros((3, 3), np.float32)]
    for s, kw in ((scan, dict(scan_normals=nrm)), (scan, dict(normal_angle=60.0)), (scan, dict(scan_normals=nrm, normal_angle=0.0)),
                  (scan, dict(scan_normals=nrm, normal_angle=180.0)), (scan, dict(scan_normals=nrm, normal_angle=-5.0)),
                  (scan, dict(scan_normals=nrm, normal_angle=float("nan"))), (scan, dict(scan_normals=nrm[:1], normal_angle=60.0)),
                  (scan, dict(scan_normals=nrm[:, :4], normal_angle=60.0)), (ragged, dict(scan_normals=nrm, normal_angle=60.0)),
                  (ragged, dict(scan_normals=ragged[::-1], normal_angle=60.0)), (scan, dict(scan_normals=ragged, normal_angle=60.0))):
        with pytest.raises(ValueError, match="normal"):
            CAPE.fit_scan(me, s, None, None, None, body, None, None, None, **kw)
