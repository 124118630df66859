"""Vertex normals on the host: the torch restatement the GPU tests use (tests/vertex_normals_reference.py) against the literal
sparse form and against the hand-derived gradient of DESIGN 7h in numpy loops, the C-ABI's declarations and argument checks
(decided before any launch), and what ``VertexNormals`` refuses.  None of this needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cape_vertex_normals_workspace_bytes", "cape_vertex_normals_fwd", "cape_vertex_normals_bwd")


def _small_mesh():
    """9 vertices, 8 faces: an open patch with valences 1..4, one collinear (degenerate) face, one pair of faces that cancel
    on a vertex of their own, and vertex 8 in no face.  Dyadic coordinates."""
    rng = np.random.default_rng(5)
    x = np.round(rng.standard_normal((2, 9, 3)) * 64) / 64
    x[:, 5] = 0.5 * (x[:, 4] + x[:, 6])                      # 4, 5, 6 collinear: face (4, 5, 6) is degenerate
    faces = np.array([[0, 1, 2], [2, 1, 3], [0, 2, 4], [3, 1, 0], [4, 5, 6], [2, 3, 6], [7, 0, 1], [7, 1, 0]])
    return x, faces


# ---- the restatement itself ----------------------------------------------------------------------------------------------

def test_reference_equals_the_sparse_form():
    """normalize(ftov @ unit_face_normals), the way psbody.mesh and the reference write it, with scipy in float64."""
    import scipy.sparse as sp
    import vertex_normals_reference as R
    x, faces = _small_mesh()
    V, F = x.shape[1], len(faces)
    n64, _, s_len, m_len = R.evaluate(x, faces, np.zeros_like(x), torch.float64)
    ftov = sp.csr_matrix((np.ones(3 * F), (faces.reshape(-1), np.repeat(np.arange(F), 3))), shape=(V, F))
    for i in range(x.shape[0]):
        m = np.cross(x[i, faces[:, 1]] - x[i, faces[:, 0]], x[i, faces[:, 2]] - x[i, faces[:, 0]])
        ss = (m * m).sum(1, keepdims=True)
        u = m / np.sqrt(ss + (ss == 0))
        s = ftov @ u
        ss = (s * s).sum(1, keepdims=True)
        want = s / np.sqrt(ss + (ss == 0))
        assert np.abs(n64[i] - want).max() <= 1e-14
        assert np.abs(s_len[i] - np.sqrt(ss[:, 0])).max() <= 1e-14 and np.abs(m_len[i] - np.linalg.norm(m, axis=1)).max() <= 1e-14
    assert (m_len[:, 4] == 0).all() and (s_len[:, 7] == 0).all() and (s_len[:, 8] == 0).all()
    assert (n64[:, 7] == 0).all() and (n64[:, 8] == 0).all() and (n64[:, 5] == 0).all()      # 5: its only face is degenerate
    assert np.abs(np.linalg.norm(n64[:, :5], axis=-1) - 1).max() < 1e-14


def _numpy_loops(x, faces, gbar):
    """Normals and gradient by the formulas of DESIGN 7h -- the two passes of the backward kernels -- one vertex at a time,
    float64, over the vertex -> incident-corner table in list order."""
    from cape_amd.graph import vertex_face_table
    N, V, _ = x.shape
    vptr, vidx = vertex_face_table(faces, V)
    guard = lambda a: np.sqrt(a @ a + (1.0 if a @ a == 0 else 0.0))

    def unit(xs, f):
        m = np.cross(xs[faces[f, 1]] - xs[faces[f, 0]], xs[faces[f, 2]] - xs[faces[f, 0]])
        r = guard(m)
        return m / r, r

    n, h, dx = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    for i in range(N):
        for v in range(V):
            s = np.zeros(3)
            for code in vidx[vptr[v]:vptr[v + 1]]:
                s += unit(x[i], code // 3)[0]
            r = guard(s)
            n[i, v] = s / r
            h[i, v] = (gbar[i, v] - n[i, v] * (n[i, v] @ gbar[i, v])) / r
        for v in range(V):
            for code in vidx[vptr[v]:vptr[v + 1]]:
                f, k = code // 3, code % 3
                u, r = unit(x[i], f)
                G = h[i, faces[f, 0]] + h[i, faces[f, 1]] + h[i, faces[f, 2]]
                gamma = (G - u * (u @ G)) / r
                dx[i, v] += np.cross(gamma, x[i, faces[f, (k + 2) % 3]] - x[i, faces[f, (k + 1) % 3]])
    return n, dx


def test_reference_gradient_equals_the_derived_formulas():
    import vertex_normals_reference as R
    x, faces = _small_mesh()
    gbar = np.random.default_rng(6).standard_normal(x.shape)
    n64, g64, _, _ = R.evaluate(x, faces, gbar, torch.float64)
    n, dx = _numpy_loops(x, faces, gbar)
    assert np.abs(n - n64).max() <= 1e-14
    assert np.isfinite(g64).all() and np.abs(dx - g64).max() <= 1e-12 * max(1.0, np.abs(g64).max())
    assert np.abs(g64[:, 5]).max() > 0           # the degenerate face passes its G on unscaled: the guards are constants
    assert not g64[:, 8].any()


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------

def test_entries_declared_bound_and_exported():
    from cape_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    assert int(re.search(r"#define CAPE_ABI_VERSION (\d+)", hdr).group(1)) == 18 and _lib.lib.cape_abi_version() == 18
    assert hdr.count("lib/losses.py:54-80") >= 2
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    assert _lib.SIGNATURES[ENTRIES[0]][0] is ctypes.c_int64
    assert _lib.SIGNATURES[ENTRIES[1]][0] is ctypes.c_int and _lib.SIGNATURES[ENTRIES[2]][0] is ctypes.c_int


def test_entries_reject_bad_arguments_before_launching():
    from cape_amd._lib import lib
    P = ctypes.c_void_p
    N, V, F = 2, 6890, 13776
    need = int(lib.cape_vertex_normals_workspace_bytes(N, V))
    assert need == N * V * 3 * 4
    assert lib.cape_vertex_normals_workspace_bytes(0, V) == -1 and lib.cape_vertex_normals_workspace_bytes(N, 0) == -1
    assert lib.cape_vertex_normals_workspace_bytes(65536, 32768) == -1                   # N V = 2^31
    assert lib.cape_vertex_normals_workspace_bytes(65536, 32767) == 65536 * 32767 * 12

    def fwd(**kw):
        a = dict(x=P(0x100000), ldx=4, faces=P(0x200000), vptr=P(0x300000), vidx=P(0x400000), N=N, V=V, F=F, out=P(0x500000),
                 ldn=3)
        a.update(kw)
        return lib.cape_vertex_normals_fwd(a["x"], a["ldx"], a["faces"], a["vptr"], a["vidx"], a["N"], a["V"], a["F"], a["out"],
                                           a["ldn"], None)

    def bwd(**kw):
        a = dict(x=P(0x100000), ldx=4, g=P(0x600000), ldg=3, faces=P(0x200000), vptr=P(0x300000), vidx=P(0x400000), N=N, V=V, F=F,
                 dx=P(0x700000), ldd=4, ws=P(0x800000), need=need)
        a.update(kw)
        return lib.cape_vertex_normals_bwd(a["x"], a["ldx"], a["g"], a["ldg"], a["faces"], a["vptr"], a["vidx"], a["N"], a["V"],
                                           a["F"], a["dx"], a["ldd"], a["ws"], a["need"], None)

    for name in ("x", "faces", "vptr", "vidx", "out"):
        assert fwd(**{name: None}) == -1, name
    for name in ("x", "g", "faces", "vptr", "vidx", "dx", "ws"):
        assert bwd(**{name: None}) == -1, name
    for call in (fwd, bwd):
        assert call(N=0) == -1 and call(N=-1) == -1 and call(V=0) == -1 and call(F=0) == -1
        assert call(ldx=2) == -1
        assert call(N=65536, V=32768) == -1                                                # N V = 2^31
        assert call(F=715827883) == -1                                                     # 3 F = 2^31 + 1
    assert fwd(ldn=2) == -1
    assert bwd(ldg=2) == -1 and bwd(ldd=2) == -1
    assert bwd(need=need - 4) == -1 and bwd(need=0) == -1                                  # a short workspace


# ---- VertexNormals -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["shape", "flat", "float", "negative", "too_large", "repeated", "empty"])
def test_bad_faces(bad):
    from cape_amd.vertex_normals import VertexNormals
    _, f = _small_mesh()
    f = f.copy()
    if bad == "shape":
        f = f[:, :2]
    elif bad == "flat":
        f = f.reshape(-1)
    elif bad == "float":
        f = f.astype(np.float64)
    elif bad == "negative":
        f[5, 1] = -1
    elif bad == "too_large":
        f[7, 2] = 9
    elif bad == "repeated":
        f[3, 2] = f[3, 0]
    else:
        f = f[:0]
    with pytest.raises(ValueError):
        VertexNormals(f, 9)


def test_tables_are_built_on_the_host_and_smpl_builds_them_lazily():
    import smpl_synth as synth
    from cape_amd import smpl
    from cape_amd.graph import vertex_face_table
    from cape_amd.vertex_normals import VertexNormals
    _, f = _small_mesh()
    vn = VertexNormals(f.astype(np.int64), 9)
    assert vn.faces.dtype == np.int32 and np.array_equal(vn.faces, f) and (vn.V, vn.F) == (9, 8)
    ptr, idx = vertex_face_table(f, 9)
    assert np.array_equal(vn.vptr, ptr) and np.array_equal(vn.vidx, idx)
    # an SMPL with faces that are no triangle list still constructs: nothing looks at them until normals are asked for
    m = dict(synth.small())
    m["f"] = np.zeros((4, 3), np.int64)
    body = smpl.SMPL(m)
    assert body._normals is None
    with pytest.raises(ValueError):
        body.vertex_normals_np(np.zeros((1, body.V, 3), np.float32))


def test_row_check_refuses_what_the_kernels_must_not_see():
    """The one check between a tensor and the kernels, on the host: another device, dtype, shape or row layout is a ValueError."""
    from cape_amd.vertex_normals import _rows
    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    t = torch.zeros(2, 9, 3)
    assert _rows("verts", t, 9, cpu) == 3
    assert _rows("verts", torch.zeros(2, 9, 4)[:, :, :3], 9, cpu) == 4
    for bad, dev in ((t, gpu), (t.double(), cpu), (t.numpy(), cpu), (t[:, :8], cpu), (t[0], cpu), (t[:0], cpu),
                     (torch.zeros(2, 3, 9).transpose(1, 2), cpu), (torch.zeros(4, 9, 3)[::2], cpu)):
        with pytest.raises(ValueError):
            _rows("verts", bad, 9, dev)


def test_no_cpu_fallback(monkeypatch):
    from cape_amd._lib import CapeHipError
    from cape_amd.vertex_normals import VertexNormals
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x, f = _small_mesh()
    vn = VertexNormals(f, 9)
    xt = torch.tensor(x, dtype=torch.float32)
    with pytest.raises(CapeHipError):
        vn.forward(xt)
    with pytest.raises(CapeHipError):
        vn.diff(xt.requires_grad_(True))
    with pytest.raises(CapeHipError):
        vn.np(x)
