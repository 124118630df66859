"""lambda_normal on the host: the vertex -> incident-corner table, how the constructor resolves the option and the faces, the
argument checks of cape_face_normal_loss_fwd_bwd (decided before any launch), and the torch restatement the GPU tests use
(tests/normal_loss_reference.py) against a plain numpy double loop.  None of this needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
V = 6890


def _faces():
    return np.load(os.path.join(GOLDEN, "template_faces.npy"))


@pytest.fixture(scope="module")
def make_model(mesh_ops):
    from cape_amd.configs import cape_params
    from cape_amd.models import CAPE
    m = mesh_ops

    def make(**kw):
        return CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], **dict(cape_params(p=m["p"], batch_size=2), **kw))
    return make


# ---- vertex_face_table ---------------------------------------------------------------------------------------------------

def _check_table(faces, num_verts):
    from cape_amd.graph import vertex_face_table
    ptr, idx = vertex_face_table(faces, num_verts)
    F = faces.shape[0]
    assert ptr.dtype == np.int32 and idx.dtype == np.int32
    assert ptr.shape == (num_verts + 1,) and idx.shape == (3 * F,)
    assert ptr[0] == 0 and ptr[-1] == 3 * F
    assert np.array_equal(np.diff(ptr), np.bincount(faces.reshape(-1), minlength=num_verts))
    assert np.array_equal(np.sort(idx), np.arange(3 * F))                 # every (face, corner) exactly once
    brute = [[] for _ in range(num_verts)]                                # brute-force inversion, in code order
    for f in range(F):
        for k in range(3):
            brute[faces[f, k]].append(3 * f + k)
    for v in range(num_verts):
        lst = idx[ptr[v]:ptr[v + 1]].tolist()
        assert lst == sorted(lst) and lst == brute[v], v
    return ptr, idx


def test_vertex_face_table_on_the_template():
    faces = _faces()
    assert faces.shape == (13776, 3)
    ptr, _ = _check_table(faces, V)
    deg = np.diff(ptr)
    assert deg.min() >= 3 and deg.max() <= 9 and abs(deg.mean() - 6.0) < 0.01


def test_vertex_face_table_on_a_random_mesh_with_an_unused_vertex():
    rng = np.random.default_rng(3)
    nv = 40
    faces = np.stack([rng.choice(nv - 1, 3, replace=False) for _ in range(97)])      # vertex nv - 1 is in no face
    ptr, _ = _check_table(faces, nv)
    assert ptr[nv] == ptr[nv - 1]


# ---- constructor ---------------------------------------------------------------------------------------------------------

def _write_obj(path, faces, slashes=False):
    pack_v = np.zeros((V, 3))
    with open(path, "w") as fh:
        fh.write("# template\n")
        for v in pack_v:
            fh.write("v %.1f %.1f %.1f\n" % tuple(v))
        for i, f in enumerate(faces):
            if slashes and i % 2:
                fh.write("f %d/%d/%d %d/%d/%d %d//%d\n" % (f[0] + 1, 7, 8, f[1] + 1, 9, 1, f[2] + 1, 4))
            elif slashes:
                fh.write("f %d/%d %d/%d %d/%d\n" % (f[0] + 1, 3, f[1] + 1, 2, f[2] + 1, 1))
            else:
                fh.write("f %d %d %d\n" % (f[0] + 1, f[1] + 1, f[2] + 1))


def test_lambda_normal_zero_reads_nothing_and_builds_nothing(tmp_path, make_model):
    for kw in (dict(), dict(lambda_normal=0), dict(lambda_normal=0.0, faces=_faces())):
        model = make_model(project_dir=str(tmp_path), **kw)              # no template under project_dir
        assert model.lambda_normal == 0.0 and model._faces is None
        assert not hasattr(model, '_face_dev')


def test_explicit_faces_win_over_the_file(tmp_path, make_model):
    (tmp_path / "data").mkdir()
    _write_obj(str(tmp_path / "data" / "template_mesh.obj"), _faces()[:10])
    model = make_model(lambda_normal=0.5, faces=_faces(), project_dir=str(tmp_path))
    assert model.lambda_normal == 0.5
    assert model._faces.dtype == np.int32 and np.array_equal(model._faces, _faces())


@pytest.mark.parametrize("slashes", [False, True], ids=["plain", "a/b/c"])
def test_faces_from_the_template_obj(tmp_path, make_model, slashes):
    from cape_amd.models import base_model
    (tmp_path / "data").mkdir()
    obj = str(tmp_path / "data" / "template_mesh.obj")
    _write_obj(obj, _faces(), slashes)
    assert np.array_equal(base_model._obj_faces(obj), _faces())
    # (the constructor reads vertices and edges from project_dir only when edges_smpl.npy is there too: not needed here)
    model = make_model(lambda_normal=1.0, project_dir=str(tmp_path))
    assert np.array_equal(model._faces, _faces())


def test_missing_faces_name_both_ways(tmp_path, make_model):
    with pytest.raises(FileNotFoundError) as e:
        make_model(lambda_normal=1.0, project_dir=str(tmp_path))
    msg = str(e.value)
    assert "faces=" in msg and os.path.join(str(tmp_path), "data", "template_mesh.obj") in msg


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), -float("inf")])
def test_bad_lambda_normal(bad, make_model):
    with pytest.raises(ValueError):
        make_model(lambda_normal=bad, faces=_faces())


@pytest.mark.parametrize("bad", ["shape", "flat", "float", "negative", "too_large", "repeated"])
def test_bad_faces(bad, make_model):
    f = _faces().copy()
    if bad == "shape":
        f = f[:, :2]
    elif bad == "flat":
        f = f.reshape(-1)
    elif bad == "float":
        f = f.astype(np.float64)
    elif bad == "negative":
        f[5, 1] = -1
    elif bad == "too_large":
        f[7, 2] = V
    else:
        f[9, 2] = f[9, 0]
    with pytest.raises(ValueError):
        make_model(lambda_normal=1.0, faces=f)


def test_lambda_normal_needs_three_channels(make_model):
    with pytest.raises(ValueError):
        make_model(lambda_normal=1.0, faces=_faces(), nn_input_channel=6)
    make_model(lambda_normal=0.0, nn_input_channel=6)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------

def test_abi_version_18():
    from cape_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    assert int(re.search(r"#define CAPE_ABI_VERSION (\d+)", hdr).group(1)) == 18
    assert _lib.lib.cape_abi_version() == 18
    assert "cape_face_normal_loss_fwd_bwd" in hdr and "cape_face_normal_loss_workspace_bytes" in hdr


def test_normal_entry_rejects_bad_arguments_before_launching():
    from cape_amd._lib import lib
    P = ctypes.c_void_p
    N, M, F = 2, 6890, 13776
    need = int(lib.cape_face_normal_loss_workspace_bytes(N, M, F))
    assert need >= N * F * 3 * 4                                          # room for one 3-vector per (sample, face)
    assert lib.cape_face_normal_loss_workspace_bytes(0, M, F) == -1
    assert lib.cape_face_normal_loss_workspace_bytes(N, 0, F) == -1
    assert lib.cape_face_normal_loss_workspace_bytes(N, M, 0) == -1

    def call(**kw):
        a = dict(pred=P(0x100000), ldp=4, gt=P(0x200000), ref=P(0x300000), faces=P(0x400000), fptr=P(0x500000),
                 fidx=P(0x600000), N=N, M=M, F=F, w=1.0, out=P(0x800000), total=P(0x810000), term=P(0x820000),
                 dpred=P(0x900000), ldd=4, ws=P(0xa00000), need=need)
        a.update(kw)
        return lib.cape_face_normal_loss_fwd_bwd(a["pred"], a["ldp"], a["gt"], a["ref"], a["faces"], a["fptr"], a["fidx"], a["N"],
                                                 a["M"], a["F"], a["w"], a["out"], a["total"], a["term"], a["dpred"], a["ldd"],
                                                 a["ws"], a["need"], None)

    for name in ("pred", "gt", "ref", "faces", "out", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(N=0) == -1 and call(M=0) == -1 and call(F=-3) == -1
    assert call(ldp=2) == -1
    assert call(ldd=2) == -1
    assert call(fptr=None) == -1 and call(fidx=None) == -1              # tables are needed for the gradient ...
    assert call(w=float("nan")) == -1 and call(w=float("inf")) == -1
    assert call(total=None) == -1                                       # term_in without total_out
    assert call(need=need - 4) == -4                                    # workspace too small
    assert call(need=need - 4, dpred=None, fptr=None, fidx=None, ldd=0) == -4      # ... and not for the value alone


# ---- the restatement itself ----------------------------------------------------------------------------------------------

def _numpy_loops(pred, gt, ref, faces):
    """Value and gradient by the formulas of DESIGN 7d, one face at a time, float64."""
    N, nv, _ = pred.shape
    F = len(faces)
    x, y = pred + ref, gt + ref
    val, grad = 0.0, np.zeros_like(pred)

    def unit(m):
        ss = float(m @ m)
        return m / np.sqrt(ss + (1.0 if ss == 0 else 0.0)), np.sqrt(ss + (1.0 if ss == 0 else 0.0))

    for n in range(N):
        for (i0, i1, i2) in faces:
            a, b = x[n, i1] - x[n, i0], x[n, i2] - x[n, i0]
            nx, lm = unit(np.cross(a, b))
            ny, _ = unit(np.cross(y[n, i1] - y[n, i0], y[n, i2] - y[n, i0]))
            c = float(nx @ ny)
            val += 1 - abs(c)
            g = -np.sign(c) * (ny - c * nx) / lm
            d1, d2 = np.cross(b, g), np.cross(g, a)
            grad[n, i1] += d1
            grad[n, i2] += d2
            grad[n, i0] -= d1 + d2
    return val / (N * F), grad / (N * F)


def test_reference_against_numpy_loops():
    import normal_loss_reference as R
    rng = np.random.default_rng(2)
    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 0], [5, 2, 4], [1, 5, 3]])
    grid = lambda shape, q: np.round(rng.standard_normal(shape) * q) / q   # dyadic values: the shifts below are exact
    ref = grid((6, 3), 8.0)
    pred = grid((3, 6, 3), 1024.0)
    gt = pred + grid((3, 6, 3), 4096.0)
    gt[1] = -gt[1] - 2 * ref                                              # y = -(...): some cosines negative
    pred[2, 1] = pred[2, 2] + ref[2] - ref[1]                             # x[1] == x[2] in sample 2: degenerate predicted faces
    gt[0, 4] = gt[0, 0] + ref[0] - ref[4]                                 # y[4] == y[0] in sample 0: degenerate target faces
    val, grad, c = R.evaluate(pred, gt, ref, faces, torch.float64)
    want_val, want_grad = _numpy_loops(pred, gt, ref, faces)
    assert (c < -0.1).any() and (c > 0.1).any()
    assert (c[2, [0, 1]] == 0).all() and c[0, 2] == 0 and (c != 0).sum() == c.size - 3        # degenerate faces: c = 0, their term is 1
    assert np.isfinite(grad).all()
    assert abs(val - want_val) < 1e-13
    assert np.abs(grad - want_grad).max() < 1e-12 * max(1.0, np.abs(want_grad).max())
    # all faces degenerate in pred: the value is exactly 1 and the gradient exactly 0
    val1, grad1, _ = R.evaluate(np.zeros((1, 6, 3)), gt[:1], np.zeros((6, 3)), faces, torch.float32)
    assert val1 == 1.0 and not grad1.any()
