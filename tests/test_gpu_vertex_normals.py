"""Vertex normals on the device (cape_amd/csrc/mesh/vertex_normals.hip; cape_amd.vertex_normals.VertexNormals, the SMPL
wrappers, CAPE.decode_posed(return_normals=True), CAPE.fit_posed(lambda_vnormal=...)) against fp64 torch autograd of the
definition (tests/vertex_normals_reference.py; the reference's lib/losses.py:54-80).

Bars: SURVEY 8(c) through tests/parity_bar.check -- the device's error against fp64 may be at most 4 x the error of the fp32
restatement on the same inputs and measure (floor 4 * 2^-24): (a) the normals' max absolute component error (components lie
in [-1, 1]), (b) the gradient's vertex_err (max per-vertex error norm / max per-vertex gradient norm) and its whole-tensor
relative L2, as tests/test_gpu_normal_loss.py defines them.  Both zero guards are discontinuities, so every parity case first
asserts, on the CPU references alone, that fp64 min |s_v| >= 5e-3 over the vertices that have faces and min |m_f| >= 1e-8 (the
exact-zero cases: that every length is exactly 0 in both precisions or above those thresholds).  No vertex is ever left out of
a comparison."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
V = 6890
MIN_S, MIN_M = 5e-3, 1e-8
GRID_CAP_THREADS = 1024 * 256          # vertex_normals.hip: MAXB blocks of LB threads, the rest by the grid-stride loop


def vertex_err(a, ref):
    a = np.asarray(a, dtype=np.float64).reshape(-1, ref.shape[-1])
    r = np.asarray(ref, dtype=np.float64).reshape(-1, ref.shape[-1])
    return np.sqrt(((a - r) ** 2).sum(-1)).max() / max(np.sqrt((r * r).sum(-1)).max(), 1e-30)


def rel_l2(a, ref):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.sqrt(((a - r) ** 2).sum() / max((r * r).sum(), 1e-300))


def max_abs(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max())


@functools.lru_cache(maxsize=None)
def _faces():
    return np.load(os.path.join(GOLD, "template_faces.npy"))


def _template():
    from cape_amd.load_data import load_pack
    return np.asarray(load_pack()["template_verts"], dtype=np.float64)


def _recipe(seed, base, sc, N=2):
    """The issue's input recipe: float32 x and gbar."""
    rng = np.random.default_rng(seed)
    x = (base * _template() + sc * rng.standard_normal((N, V, 3))).astype(np.float32)
    gbar = rng.standard_normal((N, V, 3)).astype(np.float32)
    return x, gbar


RECIPES = {"rng7_5e-4": (7, 1, 5e-4), "rng7_5e-3": (7, 1, 5e-3), "rng13_noise": (13, 0, 1)}


@functools.lru_cache(maxsize=None)
def _template_case(recipe, N=2):
    """(x, gbar, fp64 reference, fp32 restatement) of a template recipe, computed once and shared (nothing writes to them)."""
    x, gbar = _recipe(*RECIPES[recipe], N=N)
    return (x, gbar) + _references(x, _faces(), gbar)


def _references(x, faces, gbar, exact_zeros=False):
    """((n, grad) fp64, (n, grad) fp32) after the condition on the inputs, CPU references only."""
    import vertex_normals_reference as R
    n64, g64, s64, m64 = R.evaluate(x, faces, gbar, torch.float64)
    n32, g32, s32, m32 = R.evaluate(x, faces, gbar, torch.float32)
    used = np.zeros(x.shape[1], bool)
    used[np.asarray(faces).reshape(-1)] = True
    if exact_zeros:          # every length is exactly zero in both precisions, or clear of the guard
        for l64, l32, bar in ((s64[:, used], s32[:, used], MIN_S), (m64, m32, MIN_M)):
            assert np.array_equal(l64 == 0, l32 == 0) and (l64[l64 != 0] >= bar).all(), "input condition (exact zeros)"
    else:
        assert s64[:, used].min() >= MIN_S, "input condition: fp64 min |s_v| = %.3g" % s64[:, used].min()
        assert m64.min() >= MIN_M, "input condition: fp64 min |m_f| = %.3g" % m64.min()
    assert not s64[:, ~used].any()
    return (n64, g64), (n32, g32)


def _device(vn, x, gbar, rows="dense"):
    """(normals, d <n, gbar> / d x, the input's pad gradient or None) through VertexNormals.diff; with rows4 the input, the
    incoming gradient and forward's output live in 16-byte rows whose padding holds 1e9."""
    dev = vn.device
    N, nv, _ = x.shape
    xt, gt = torch.tensor(x, device=dev), torch.tensor(gbar, device=dev)
    if rows == "dense":
        leaf = xt.requires_grad_(True)
        view, gview = leaf, gt
    else:
        leaf = torch.full((N, nv, 4), 1e9, dtype=torch.float32, device=dev)
        leaf[:, :, :3] = xt
        leaf.requires_grad_(True)
        view = leaf[:, :, :3]
        g4 = torch.full((N, nv, 4), 1e9, dtype=torch.float32, device=dev)
        g4[:, :, :3] = gt
        gview = g4[:, :, :3]
    n = vn.diff(view)
    assert n.shape == (N, nv, 3) and n.requires_grad
    n.backward(gview)
    torch.cuda.synchronize()
    with torch.no_grad():                                    # forward on the same rows: the same bits, padding untouched
        if rows == "dense":
            n2 = vn.forward(view.detach())
        else:
            out4 = torch.full((N, nv, 4), 1e9, dtype=torch.float32, device=dev)
            n2 = vn.forward(view.detach(), out=out4[:, :, :3])
            assert n2.data_ptr() == out4.data_ptr() and bool((out4[:, :, 3] == 1e9).all())
            assert bool((leaf.detach()[:, :, 3] == 1e9).all()) and bool((g4[:, :, 3] == 1e9).all())
        assert torch.equal(n2, n.detach())
    g = leaf.grad.cpu().numpy()
    return n.detach().cpu().numpy(), g[:, :, :3], (g[:, :, 3] if rows != "dense" else None)


def _judge(tag, n, g, ref64, ref32):
    from parity_bar import check
    (n64, g64), (n32, g32) = ref64, ref32
    errs = (max_abs(n, n64), vertex_err(g, g64), rel_l2(g, g64))
    errs32 = (max_abs(n32, n64), vertex_err(g32, g64), rel_l2(g32, g64))
    print("%s: normals max abs err %.2e [fp32 %.2e]; gradient vertex_err %.2e [fp32 %.2e], rel L2 %.2e [fp32 %.2e]"
          % (tag, errs[0], errs32[0], errs[1], errs32[1], errs[2], errs32[2]))
    assert np.isfinite(n).all() and np.isfinite(g).all()
    check(tag, "vertex normals (max abs)", errs[0], errs32[0])
    check(tag, "vertex normal gradient (vertex_err)", errs[1], errs32[1])
    check(tag, "vertex normal gradient (rel L2)", errs[2], errs32[2])


@functools.lru_cache(maxsize=None)
def _template_normals():
    from cape_amd.vertex_normals import VertexNormals
    return VertexNormals(_faces(), V)


# ---- 1. the template ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", ["dense", "rows4"])
@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_template_recipes(recipe, rows):
    x, gbar, ref64, ref32 = _template_case(recipe)
    n, g, pad = _device(_template_normals(), x, gbar, rows)
    _judge("vnormals[%s,%s]" % (recipe, rows), n, g, ref64, ref32)
    if rows == "rows4":
        assert float(np.abs(pad).max()) == 0.0


# ---- 2. small synthetic meshes --------------------------------------------------------------------------------------------

def _tetrahedron():
    return 4, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def _fan12():
    """A closed fan: hub 0 with valence 12, rim 1..12 with valence 2."""
    return 13, np.array([[0, i, i % 12 + 1] for i in range(1, 13)])


def _grid6_plus_one():
    """A 6 x 6 vertex grid, each of its 25 cells cut into two triangles, and vertex 36 that no face uses."""
    idx = np.arange(36).reshape(6, 6)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return 37, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])


SMALL = {"tetrahedron": (_tetrahedron, 4, 4), "fan12": (_fan12, 13, 12), "grid6_plus_one": (_grid6_plus_one, 37, 50)}


def _small_inputs(mesh, N):
    nv, faces = SMALL[mesh][0]()
    rng = np.random.default_rng(100 + N)
    x = rng.standard_normal((N, nv, 3)).astype(np.float32)
    if mesh == "grid6_plus_one":         # a height field over the grid: a surface, not 37 points thrown into space
        gx, gy = np.meshgrid(np.arange(6.0), np.arange(6.0), indexing="ij")
        x[:, :36, 0], x[:, :36, 1] = gx.ravel() + 0.2 * x[:, :36, 0], gy.ravel() + 0.2 * x[:, :36, 1]
    return nv, faces, x, rng.standard_normal((N, nv, 3)).astype(np.float32)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("mesh", sorted(SMALL))
def test_small_meshes(mesh, N):
    from cape_amd.vertex_normals import VertexNormals
    nv, faces, x, gbar = _small_inputs(mesh, N)
    assert (nv, len(faces)) == SMALL[mesh][1:]
    valence = np.bincount(faces.reshape(-1), minlength=nv)
    ref64, ref32 = _references(x, faces, gbar)
    n, g, _ = _device(VertexNormals(faces, nv), x, gbar)
    _judge("vnormals[%s,N=%d]" % (mesh, N), n, g, ref64, ref32)
    if mesh == "fan12":
        assert valence[0] == 12
    if mesh == "grid6_plus_one":
        assert valence[36] == 0 and not n[:, 36].any() and not g[:, 36].any()


# ---- 3. exact zeros -------------------------------------------------------------------------------------------------------

def test_exact_zeros():
    """Small integer coordinates: every cross product is exact in fp32 and fp64 alike.  Vertex 0's only face (0, 1, 2) lies on
    three collinear points: its normal is exactly 0.  Vertices 5, 6, 7 carry the faces (5, 6, 7) and (5, 7, 6), whose unit
    normals cancel exactly: all three normals are exactly 0.  The gradient is that of the expression as written (the guards
    pass the incoming gradient on unscaled): finite, and under the bar against autograd."""
    from cape_amd.vertex_normals import VertexNormals
    x = np.array([[[0, 0, 0], [1, 1, 2], [2, 2, 4], [0, 3, 1], [2, 0, -1], [1, 0, 0], [0, 2, 0], [0, 0, 3]]], np.float32)
    x = np.concatenate([x, x[:, :, [1, 2, 0]] * np.float32(2)], 0)                  # a second sample: permuted axes, doubled
    faces = np.array([[0, 1, 2], [1, 3, 2], [1, 2, 4], [5, 6, 7], [5, 7, 6]])
    gbar = np.random.default_rng(9).standard_normal(x.shape).astype(np.float32)
    ref64, ref32 = _references(x, faces, gbar, exact_zeros=True)
    assert not ref64[0][:, [0, 5, 6, 7]].any()
    assert np.abs(ref64[1][:, 0]).max() > 0               # the degenerate face passes a gradient on (the guard is a constant)
    n, g, _ = _device(VertexNormals(faces, 8), x, gbar)
    assert not n[:, [0, 5, 6, 7]].any()
    assert np.abs(np.linalg.norm(n[:, [1, 2, 3, 4]], axis=-1) - 1).max() < 1e-6
    _judge("vnormals[exact zeros]", n, g, ref64, ref32)


# ---- 4. the grid-stride loop ----------------------------------------------------------------------------------------------

def test_more_items_than_one_launch_has_threads():
    N = 39
    assert N * V == 268710 > GRID_CAP_THREADS == 262144        # the last 6566 items are second turns of the stride loop
    x, gbar, ref64, ref32 = _template_case("rng7_5e-3", N)
    n, g, _ = _device(_template_normals(), x, gbar)
    _judge("vnormals[rng7_5e-3,N=39]", n, g, ref64, ref32)


# ---- 5. repeatability, selective gradients --------------------------------------------------------------------------------

def test_backward_is_bitwise_repeatable_and_only_an_input_that_asks_gets_a_gradient():
    vn = _template_normals()
    x, gbar, _, _ = _template_case("rng13_noise")
    runs = [_device(vn, x, gbar) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    xt = torch.tensor(x, device=vn.device)
    n = vn.diff(xt)                                                  # nobody asks: no graph, no backward
    assert not n.requires_grad and n.grad_fn is None
    assert n.cpu().numpy().tobytes() == runs[0][0].tobytes()
    # two inputs feed the vertices, one asks
    a, b = xt.clone().requires_grad_(True), torch.zeros_like(xt)
    vn.diff(a + b).backward(torch.tensor(gbar, device=vn.device))
    assert b.grad is None and a.grad.cpu().numpy().tobytes() == runs[0][1].tobytes()
    with pytest.raises(RuntimeError):
        vn.forward(a)                                                # forward carries no gradient and says so, as SMPL.forward


def test_tensors_off_the_device_are_refused_before_any_launch(monkeypatch):
    """A host tensor (or a host ``out``) has a pointer the kernels must never see: ValueError, and no entry is called."""
    from cape_amd import _lib
    from cape_amd.vertex_normals import VertexNormals
    nv, faces = _tetrahedron()
    vn = VertexNormals(faces, nv)
    x = torch.randn(2, nv, 3)
    on_dev = x.to(vn.device)
    want = vn.forward(on_dev).clone()
    calls = []
    for name in ("cape_vertex_normals_fwd", "cape_vertex_normals_bwd"):
        real = getattr(_lib.lib, name)
        monkeypatch.setattr(_lib.lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    for bad in (lambda: vn.forward(x), lambda: vn(x), lambda: vn.forward(on_dev, out=torch.empty(2, nv, 3)),
                lambda: vn.forward(x, out=torch.empty_like(on_dev)), lambda: vn.diff(x.clone().requires_grad_(True)),
                lambda: vn.forward(on_dev.double()), lambda: vn.forward(on_dev[:1], out=torch.empty_like(on_dev))):
        with pytest.raises(ValueError):
            bad()
    assert calls == []
    # a gradient that arrives on the host is brought to the device, not handed to the kernel as it is
    leaf = on_dev.clone().requires_grad_(True)
    g = torch.randn(2, nv, 3)
    vn.diff(leaf).backward(g.to(vn.device))
    first = leaf.grad.clone()
    assert calls == ["cape_vertex_normals_fwd", "cape_vertex_normals_bwd"]
    assert torch.equal(vn._backward(on_dev, g), first) and torch.equal(vn.forward(on_dev), want)


def test_backward_entry_with_padded_rows_never_touches_the_padding():
    """cape_vertex_normals_bwd itself with ldx = ldg = ldd = 4 (VertexNormals always hands it a dense dx): the result is the
    dense call's bit for bit, the 1e9 in the padding of x and gbar is never read and the 1e9 in dx's padding never written."""
    import ctypes as C
    from cape_amd import _lib
    vn = _template_normals()
    dev, faces, vptr, vidx = vn._upload()
    x, gbar, _, _ = _template_case("rng7_5e-3")
    N = x.shape[0]
    _, want, _ = _device(vn, x, gbar)
    P = lambda t: C.c_void_p(t.data_ptr())

    def padded(a):
        t = torch.full((N, V, 4), 1e9, dtype=torch.float32, device=dev)
        if a is not None:
            t[:, :, :3] = torch.tensor(a, device=dev)
        return t

    x4, g4, dx4 = padded(x), padded(gbar), padded(None)
    need = int(_lib.lib.cape_vertex_normals_workspace_bytes(N, V))
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    rc = _lib.lib.cape_vertex_normals_bwd(P(x4), 4, P(g4), 4, P(faces), P(vptr), P(vidx), N, V, vn.F, P(dx4), 4, P(ws), need,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert dx4[:, :, :3].cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()
    for t in (x4, g4, dx4):
        assert bool((t[:, :, 3] == 1e9).all())


# ---- 6. the SMPL wrappers -------------------------------------------------------------------------------------------------

def _smpl_with_template_faces(seed=0):
    import smpl_synth as synth
    from cape_amd import smpl
    m = dict(synth.smpl_like(seed=seed))
    m["f"] = _faces()
    return m, smpl.SMPL(m)


def test_smpl_wrappers_equal_vertex_normals():
    _, body = _smpl_with_template_faces()
    vn = _template_normals()
    x, gbar, _, _ = _template_case("rng7_5e-3")
    want, want_g, _ = _device(vn, x, gbar)
    assert body._normals is None                                     # nothing built before the first use
    xt = torch.tensor(x, device=body.device)
    assert body.vertex_normals(xt).cpu().numpy().tobytes() == want.tobytes()
    out = torch.empty_like(xt)
    assert body.vertex_normals(xt, out=out) is out and out.cpu().numpy().tobytes() == want.tobytes()
    assert body.vertex_normals_np(x).tobytes() == want.tobytes()
    assert body.vertex_normals_np(x[0]).shape == (V, 3)
    leaf = xt.clone().requires_grad_(True)
    body.vertex_normals_diff(leaf).backward(torch.tensor(gbar, device=body.device))
    assert leaf.grad.cpu().numpy().tobytes() == want_g.tobytes()
    assert body._normals is body._vertex_normals()                   # built once


# ---- 7. decode_posed ------------------------------------------------------------------------------------------------------

def _posed_inputs(model, size, seed):
    rng = np.random.default_rng(seed)
    cond, cond2 = rng.standard_normal((size, model.nz_cond)), rng.standard_normal((size, model.nz_cond2))
    z = rng.standard_normal((size, model.nz))
    pose = np.load(os.path.join(GOLD, "demo_pose_params.npz"))["pose"][rng.integers(0, 6, size)]
    st = np.load(os.path.join(GOLD, "trainset_stats.npz"))
    idx = np.load(os.path.join(GOLD, "clothing_verts_idx.npy"))
    return cond, cond2, z, pose, (st["mean"], st["std"], idx)


def _normals_of(posed, dtype):
    import vertex_normals_reference as R
    n, _, s, m = R.evaluate(posed, _faces(), np.zeros_like(posed), dtype)
    return n, s, m


def test_decode_posed_with_normals(mesh_ops):
    from parity_bar import check
    from test_gpu_smpl import _cape_model
    model = _cape_model(mesh_ops, batch_size=4)                      # size 5: the last batch is padded
    _, body = _smpl_with_template_faces(seed=0)
    cond, cond2, z, pose, dress = _posed_inputs(model, 5, 5)
    # the synthetic model's seeded skinning weights fold the surface under the demo poses as they are: the posed meshes then
    # have fp64 min |s_v| = 0.002 - 0.005 whatever the clothing (measured), short of the input condition.  At 0.35 x the
    # rotations this body keeps min |s_v| = 0.012 (the unposed clothed meshes: 0.08).
    pose = 0.35 * pose
    zt = np.concatenate([z, cond, cond2], 1)
    posed0, clothed0 = model.decode_posed(zt, cond, cond2, pose, body, *dress)
    res = model.decode_posed(zt, cond, cond2, pose, body, *dress, return_normals=True)
    assert len(res) == 3
    posed, clothed, normals = res
    assert posed.tobytes() == posed0.tobytes() and clothed.tobytes() == clothed0.tobytes()
    assert normals.dtype == np.float32 and normals.shape == (5, V, 3)
    n64, s64, m64 = _normals_of(posed, torch.float64)
    n32, _, _ = _normals_of(posed, torch.float32)
    print("decode_posed normals: fp64 min |s| %.3g, min |m| %.3g; max abs err %.2e [fp32 %.2e]"
          % (s64.min(), m64.min(), max_abs(normals, n64), max_abs(n32, n64)))
    assert s64.min() >= MIN_S and m64.min() >= MIN_M, "input condition"
    check("decode_posed_normals", "vertex normals (max abs)", max_abs(normals, n64), max_abs(n32, n64))


# ---- 8. fit_posed ---------------------------------------------------------------------------------------------------------
SIZE = 5


@pytest.fixture(scope="module")
def fit_setup(mesh_ops):
    """test_gpu_smpl_grad's fit_setup with the template's triangles on the body model."""
    from test_gpu_smpl import _cape_model
    model = _cape_model(mesh_ops, batch_size=4)                      # size 5: the last batch is padded
    m, body = _smpl_with_template_faces(seed=6)
    rng = np.random.default_rng(21)
    cond, cond2 = rng.standard_normal((SIZE, model.nz_cond)), rng.standard_normal((SIZE, model.nz_cond2))
    z_true = rng.standard_normal((SIZE, model.nz))
    pose = np.load(os.path.join(GOLD, "demo_pose_params.npz"))["pose"][rng.integers(0, 6, SIZE)]
    st = np.load(os.path.join(GOLD, "trainset_stats.npz"))
    idx = np.load(os.path.join(GOLD, "clothing_verts_idx.npy"))
    dress_args = (st["mean"], st["std"], idx)
    target, _ = model.decode_posed(np.concatenate([z_true, cond, cond2], 1), cond, cond2, pose, body, *dress_args)
    return dict(model=model, m=m, body=body, cond=cond, cond2=cond2, z_true=z_true, pose=pose, dress=dress_args, target=target)


def _normal_term(posed, target, dtype, w=None):
    """sum_v w_v (1 - n_v(posed) . n_v(target)) / sum_v w_v per sample, evaluated in ``dtype``."""
    import vertex_normals_reference as R
    f = _faces()
    w = torch.ones(posed.shape[1], dtype=dtype) if w is None else torch.tensor(w, dtype=dtype)
    n = R.vertex_normals(torch.tensor(posed, dtype=dtype), f)[0]
    t = R.vertex_normals(torch.tensor(target, dtype=dtype), f)[0]
    return ((w[None] * (1 - (n * t).sum(-1))).sum(1) / w.sum()).double().numpy()


def test_fit_posed_without_steps_reports_the_normal_term(fit_setup):
    from parity_bar import check
    s = fit_setup
    model = s["model"]
    z0 = 0.3 * np.random.default_rng(1).standard_normal((SIZE, model.nz))
    args = (s["target"], s["pose"], s["cond"], s["cond2"], s["body"]) + tuple(s["dress"])
    w = np.random.default_rng(3).uniform(0.0, 2.0, V).astype(np.float32)
    w[::5] = 0.0
    zt = np.concatenate([z0, s["cond"], s["cond2"]], 1)
    posed0, _ = model.decode_posed(zt, s["cond"], s["cond2"], s["pose"], s["body"], *s["dress"])
    for tag, weights in (("ones", None), ("weighted", w)):
        plain = model.fit_posed(*args, z0=z0, steps=0, weights=weights)
        res = model.fit_posed(*args, z0=z0, steps=0, weights=weights, lambda_vnormal=0.5)
        assert "normal" not in plain and res["normal"].shape == (1, SIZE) and res["normal"].dtype == np.float32
        assert sorted(set(res) - {"normal"}) == sorted(plain)
        for k in plain:                                              # every other output: the bits of the call without it
            assert (res[k] is None and plain[k] is None) or res[k].tobytes() == plain[k].tobytes(), k
        assert res["posed"].tobytes() == posed0.tobytes()
        t64, t32 = _normal_term(posed0, s["target"], torch.float64, weights), _normal_term(posed0, s["target"], torch.float32, weights)
        err, err32 = max_abs(res["normal"][0], t64), max_abs(t32, t64)
        print("fit_posed normal[0] (%s): %s; max abs err %.2e [fp32 %.2e]" % (tag, res["normal"][0], err, err32))
        assert t64.min() > 1e-5                                      # z0 is not the target's code: the term is in effect
        check("fit_posed_normal0_%s" % tag, "vertex-normal term (abs)", err, err32)


def test_fit_posed_lambda_vnormal_zero_is_todays_fit(fit_setup):
    s = fit_setup
    model = s["model"]
    args = (s["target"], s["pose"], s["cond"], s["cond2"], s["body"]) + tuple(s["dress"])
    today = model.fit_posed(*args, steps=3)
    res = model.fit_posed(*args, steps=3, lambda_vnormal=0.0)
    assert "normal" not in res and sorted(res) == sorted(today)
    assert res["z"].tobytes() == today["z"].tobytes() and res["loss"].tobytes() == today["loss"].tobytes()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            model.fit_posed(*args, steps=0, lambda_vnormal=bad)


LAMBDA_VNORMAL = 0.5


def test_fit_posed_normal_term_is_per_sample_and_leaves_the_model_alone(fit_setup):
    """test_gpu_smpl_grad's edge-term test for the vertex-normal term, with its reasoning: the term is normalised per sample,
    so a sample fitted alone (a batch with one live row) and the same sample in a full batch of four take the same steps.
    Adam's step lr g / (|g| + eps) moves by at most lr / 4 times the relative error of g; kernels that sum a batch in another
    order give g to about 1e-6, so three steps agree to a few 1e-7 lr: held to 1e-4 lr.  A batch mean left in the term, or
    target normals of the wrong rows, would move the steps by a share of lr -- as the term itself does against a fit without
    it (held to more than 1e-2 lr, so that the first comparison shows something)."""
    s = fit_setup
    model, lr = s["model"], 0.1
    before = {k: (v.detach().clone(), v.requires_grad) for k, v in model._vars.items()}
    din = (np.concatenate([s["z_true"], s["cond"], s["cond2"]], 1), s["cond"], s["cond2"])
    dout = model.decode(din[0], cond=din[1], cond2=din[2])
    args = lambda sl: (s["target"][sl], s["pose"][sl], s["cond"][sl], s["cond2"][sl], s["body"]) + tuple(s["dress"])
    kw = dict(steps=3, lr=lr, lambda_vnormal=LAMBDA_VNORMAL)
    full = model.fit_posed(*args(slice(0, SIZE)), **kw)
    alone = model.fit_posed(*args(slice(0, 1)), **kw)
    plain = model.fit_posed(*args(slice(0, 1)), steps=3, lr=lr)
    assert full["normal"].shape == (4, SIZE) and alone["normal"].shape == (4, 1) and np.isfinite(full["normal"]).all()
    d_same, d_term = float(np.abs(alone["z"][0] - full["z"][0]).max()), float(np.abs(alone["z"][0] - plain["z"][0]).max())
    print("vertex-normal term (lambda %.2g): alone vs in a batch %.3e, with vs without the term %.3e; normal rows %s -> %s"
          % (LAMBDA_VNORMAL, d_same, d_term, full["normal"][0], full["normal"][-1]))
    assert d_same <= 1e-4 * lr
    assert d_term > 1e-2 * lr, "the vertex-normal term does not move the fit: the comparison above shows nothing"
    # the sign of the term's gradient: the target is a decoded mesh, so the term can reach 0, and at lambda 0.5 it carries the
    # objective (about 5e-4 next to a data term of squared millimetres, 1e-6 .. 1e-5); three Adam steps of lr 0.1 from z = 0
    # lower it for every sample, where a gradient of the wrong sign would raise it
    assert np.all(full["normal"][-1] < full["normal"][0]), full["normal"][[0, -1]]
    for k, v in model._vars.items():
        assert torch.equal(v.detach(), before[k][0]) and v.grad is None and v.requires_grad == before[k][1], k
    assert model.decode(din[0], cond=din[1], cond2=din[2]).tobytes() == dout.tobytes()
