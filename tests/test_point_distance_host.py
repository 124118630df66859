"""Mesh-to-scan distance on the host: the brute-force reference the GPU tests use (tests/point_distance_reference.py) against a
KD-tree and against torch autograd, the C-ABI's declarations and argument checks (decided before any launch), and what
``PointDistance`` and ``CAPE.fit_scan``'s new arguments refuse before a device is touched.  None of this needs a device."""
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
import point_distance_reference as P     # noqa: E402

ENTRIES = ("cape_point_distance_workspace_bytes", "cape_point_distance_plan", "cape_point_nearest_fwd", "cape_point_nearest_bwd")
PT, QB, SPLIT_MAX = 512, 512, 16        # what include/cape_hip.h documents


# ---- the references themselves -----------------------------------------------------------------------------------------------

def test_brute_force_equals_a_kdtree():
    rng = np.random.default_rng(1)
    try:
        from scipy.spatial import cKDTree
        sizes = ((300, 1), (257, 1000), (1, 77))
        nearest = lambda q, p: cKDTree(p).query(q)
    except ImportError:                                      # a plain double loop on a small case
        sizes = ((40, 1), (33, 50))

        def nearest(q, p):
            d = np.array([[np.sqrt(((a - b) ** 2).sum()) for b in p] for a in q])
            return d.min(1), d.argmin(1)
    for Q, M in sizes:
        q, p = rng.standard_normal((Q, 3)), rng.standard_normal((M, 3))
        index, d2 = P.brute_force(q, p)
        kd, ki = nearest(q, p)
        assert np.abs(np.sqrt(d2) - kd).max() <= 1e-12
        assert np.array_equal(index, ki)                      # random clouds have no ties
        assert np.array_equal(P.own_d2(q, p, index), d2)
        i_small, d_small = P.brute_force(q, p, chunk=7)       # the chunking changes nothing
        assert np.array_equal(i_small, index) and np.array_equal(d_small, d2)


def test_brute_force_ties_non_finite_and_the_fp32_restatement():
    rng = np.random.default_rng(2)
    q = rng.standard_normal((50, 3)).astype(np.float32)
    half = rng.standard_normal((20, 3)).astype(np.float32)
    p = np.concatenate([half, half])                         # every point twice: the lowest index wins
    i64, d64 = P.brute_force(q, p)
    i32, d32 = P.brute_force(q, p, np.float32)
    assert (i64 < 20).all() and (i32 < 20).all() and d32.dtype == np.float32
    assert np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(d64)).max() <= 1e-6
    bad = np.concatenate([[[np.nan, 0, 0], [np.inf, 0, 0]], p]).astype(np.float32)
    ib, db = P.brute_force(q, bad)
    assert np.array_equal(ib - 2, i64) and np.array_equal(db, d64)
    qn = q.copy()
    qn[3, 1] = np.nan
    qn[4, 2] = -np.inf
    for dt in (np.float64, np.float32):
        i, d = P.brute_force(qn, p, dt)
        assert list(i[3:5]) == [-1, -1] and np.isnan(d[3:5]).all() and np.array_equal(np.delete(i, (3, 4)), np.delete(i64, (3, 4)))
        i, d = P.brute_force(q, np.full((5, 3), np.nan), dt)
        assert (i == -1).all() and np.isnan(d).all()
        i, d = P.brute_force(q, np.zeros((0, 3)), dt)
        assert (i == -1).all() and np.isnan(d).all()


def test_gradient_formulas_equal_autograd_with_the_index_held():
    rng = np.random.default_rng(3)
    q, p = rng.standard_normal((200, 3)), rng.standard_normal((30, 3))       # several queries share a point
    index, _ = P.brute_force(q, p)
    assert len(np.unique(index)) < len(index)
    g = rng.standard_normal(len(q))
    dq, dp = P.gradients(q, p, index, g)
    qt, pt = torch.tensor(q, requires_grad=True), torch.tensor(p, requires_grad=True)
    d2 = ((qt - pt[torch.as_tensor(index)]) ** 2).sum(-1)
    (d2 * torch.as_tensor(g)).sum().backward()
    assert np.abs(qt.grad.numpy() - dq).max() <= 1e-12 * np.abs(dq).max()
    assert np.abs(pt.grad.numpy() - dp).max() <= 1e-12 * np.abs(dp).max()
    index[5] = -1                                             # a query without a point adds nothing
    dq2, dp2 = P.gradients(q, p, index, g)
    assert not dq2[5].any() and np.abs(dp2 - dp).max() > 0
    dq32, dp32 = P.gradients(q.astype(np.float32), p.astype(np.float32), index, g.astype(np.float32), np.float32)
    assert dq32.dtype == np.float32 and dp32.dtype == np.float32


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
    assert "scan/point_distance.o" in mk and os.path.exists(os.path.join(ROOT, "cape_amd", "csrc", "scan", "point_distance.hip"))


def _plan(N, Q, M):
    from cape_amd._lib import lib
    out = (ctypes.c_int32 * 3)()
    assert lib.cape_point_distance_plan(N, Q, M, out) == 0
    return tuple(out)


def test_workspace_bytes_and_plan():
    from cape_amd._lib import lib
    wb = lib.cape_point_distance_workspace_bytes
    for N, Q, M in ((16, 6890, 20000), (1, 6890, 20000), (2, 5, 9), (1, QB, SPLIT_MAX * PT), (1, 1, 100000)):
        split, pt, qb = _plan(N, Q, M)
        assert (pt, qb) == (PT, QB) and 1 <= split <= min(SPLIT_MAX, -(-M // PT)), (N, Q, M)
        # forward: 8 bytes per (part, query); backward: three doubles per query
        assert wb(N, Q, M) == max(8 * split * N * Q, 24 * N * Q), (N, Q, M)
    assert _plan(1, 1, 100000)[0] == SPLIT_MAX and wb(1, 1, 100000) == 8 * SPLIT_MAX     # the forward's share decides
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5)):
        assert wb(*bad) == -1, bad
    assert wb(65536, 32768, 1) == -1 and wb(65536, 32767, 1) > 0                        # N Q = 2^31
    assert wb(65536, 1, 32768) == -1 and wb(65536, 1, 32767) > 0                        # N M = 2^31
    out = (ctypes.c_int32 * 3)()
    assert lib.cape_point_distance_plan(0, 5, 5, out) == -1 and lib.cape_point_distance_plan(1, 5, 5, None) == -1
    assert lib.cape_point_distance_plan(65536, 32768, 1, out) == -1
    # the split is a function of the sizes: few workgroups -> the points are shared out, many -> one walk
    assert _plan(1, QB, SPLIT_MAX * PT)[0] == SPLIT_MAX          # one query tile over SPLIT_MAX point tiles
    assert _plan(1, QB, 64 * PT)[0] == SPLIT_MAX                 # capped
    assert _plan(1, QB, 3 * PT)[0] == 3 and _plan(1, QB, PT)[0] == 1 and _plan(1, QB, PT + 1)[0] == 2
    assert _plan(1, 128 * QB, SPLIT_MAX * PT)[0] == 8 and _plan(1, 600 * QB, SPLIT_MAX * PT)[0] == 1
    assert _plan(2048, 5, 100000)[0] == 1                        # a large grid


def test_entries_reject_bad_arguments_before_launching():
    """No device here: a launch would fail with another code, so -1 shows the refusal came first."""
    from cape_amd._lib import lib
    A = ctypes.c_void_p
    N, Q, M = 2, 6890, 1000
    need = int(lib.cape_point_distance_workspace_bytes(N, Q, M))

    def fwd(**kw):
        a = dict(q=A(0x100000), ldq=4, points=A(0x300000), ldp=3, count=None, N=N, Q=Q, M=M, index=A(0x400000), d2=A(0x600000),
                 ws=A(0x800000), need=need)
        a.update(kw)
        return lib.cape_point_nearest_fwd(a["q"], a["ldq"], a["points"], a["ldp"], a["count"], a["N"], a["Q"], a["M"], a["index"],
                                          a["d2"], a["ws"], a["need"], None)

    def bwd(**kw):
        a = dict(q=A(0x100000), ldq=4, points=A(0x300000), ldp=3, count=None, index=A(0x400000), g=A(0x600000), N=N, Q=Q, M=M,
                 dq=A(0x700000), lddq=3, dp=None, lddp=3, ws=A(0x800000), need=need)
        a.update(kw)
        return lib.cape_point_nearest_bwd(a["q"], a["ldq"], a["points"], a["ldp"], a["count"], a["index"], a["g"], a["N"], a["Q"],
                                          a["M"], a["dq"], a["lddq"], a["dp"], a["lddp"], a["ws"], a["need"], None)

    for name in ("q", "points", "index", "d2", "ws"):
        assert fwd(**{name: None}) == -1, name
    for name in ("q", "points", "index", "g", "dq", "ws"):
        assert bwd(**{name: None}) == -1, name
    for call in (fwd, bwd):
        for size in ("N", "Q", "M"):
            assert call(**{size: 0}) == -1 and call(**{size: -1}) == -1, size
        assert call(ldq=2) == -1 and call(ldp=2) == -1
        assert call(N=65536, Q=32768, M=1) == -1                                           # N Q = 2^31
        assert call(N=65536, Q=1, M=32768) == -1                                           # N M = 2^31
        assert call(ws=A(0x800008)) == -1                                                  # not 16-byte aligned
        assert call(need=0) == -1
    assert fwd(need=8 * _plan(N, Q, M)[0] * N * Q - 8) == -1                               # a short workspace
    assert bwd(need=24 * N * Q - 8) == -1
    assert bwd(lddq=2) == -1 and bwd(dp=A(0x900000), lddp=2) == -1


# ---- PointDistance -----------------------------------------------------------------------------------------------------------

def test_point_distance_is_built_lazily_and_shares_the_scan_helpers():
    import smpl_synth as synth
    from cape_amd import point_distance, scan_distance, smpl
    assert point_distance._points is scan_distance._points and point_distance._count is scan_distance._count
    assert point_distance.pad_points is scan_distance.pad_points
    pd = point_distance.PointDistance()
    assert pd._dev is None and pd.plan(1, QB, SPLIT_MAX * PT) == (SPLIT_MAX, PT, QB)
    body = smpl.SMPL(synth.small())
    assert body._point is None and body._scan is None
    cpu = torch.device("cpu")
    assert point_distance._queries("queries", torch.zeros(2, 7, 4)[:, :, :3], cpu) == (2, 7, 4)
    for bad in (np.zeros((2, 7, 3), np.float32), torch.zeros(7, 3), torch.zeros(2, 7, 3).double(), torch.zeros(2, 0, 3),
                torch.zeros(0, 7, 3), torch.zeros(2, 7, 2), torch.zeros(2, 3, 7).transpose(1, 2)):
        with pytest.raises(ValueError):
            point_distance._queries("queries", bad, cpu)


def test_no_cpu_fallback(monkeypatch):
    from cape_amd._lib import CapeHipError
    from cape_amd.point_distance import PointDistance
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pd = PointDistance()
    qt, pt = torch.zeros(1, 5, 3), torch.zeros(1, 4, 3)
    with pytest.raises(CapeHipError):
        pd.forward(qt, pt)
    with pytest.raises(CapeHipError):
        pd.diff(qt.clone().requires_grad_(True), pt)
    with pytest.raises(CapeHipError):
        pd.backward(qt, pt, torch.zeros(1, 5, dtype=torch.int32), torch.zeros(1, 5))
    with pytest.raises(CapeHipError):
        pd.np(np.zeros((5, 3)), np.zeros((4, 3)))


# ---- fit_scan: what is decided before the device is touched --------------------------------------------------------------------

def test_fit_scan_refuses_the_new_arguments_before_anything_else():
    """lambda_mesh and mesh_max_dist are judged first, mesh_weights as soon as the sizes are known: a stand-in for the model
    without a device, a decoder or a body beyond its vertex count is enough to get there."""
    from cape_amd.models import CAPE

    class Untouchable(object):
        def __getattr__(self, name):
            raise AssertionError("fit_scan touched %s before it refused" % name)

    scan = np.zeros((2, 5, 3), np.float32)
    for kw in (dict(lambda_mesh=-1.0), dict(lambda_mesh=float("nan")), dict(lambda_mesh=float("inf")),
               dict(lambda_mesh=1.0, mesh_max_dist=-0.1), dict(lambda_mesh=1.0, mesh_max_dist=float("nan")),
               dict(mesh_max_dist=-0.1)):
        with pytest.raises(ValueError):
            CAPE.fit_scan(Untouchable(), scan, None, None, None, Untouchable(), None, None, None, **kw)
    me = types.SimpleNamespace(batch_size=2, nz=4)           # no device, no variables
    body = types.SimpleNamespace(V=6)
    for w in (np.ones(5), np.ones((6, 1)), np.zeros(6), np.array([1, 1, 1, -1, -1, -1.0]), np.array([1, np.nan, 1, 1, 1, 1.0])):
        with pytest.raises(ValueError, match="mesh_weights"):
            CAPE.fit_scan(me, scan, None, None, None, body, None, None, None, lambda_mesh=1.0, mesh_weights=w)
