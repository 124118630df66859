"""CAPE.fit_scan with the mesh-to-scan term (``lambda_mesh``, ``mesh_weights``, ``mesh_max_dist``): the two-sided objective
through cape_amd/point_distance.py next to the scan-to-mesh distance.  Model, body and scans as tests/test_gpu_fit_scan.py
builds them; three samples in batches of two, so the last batch is padded."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_distance_reference as R     # noqa: E402
import smpl_synth as synth              # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
SIZE = 3
COUNTS = (512, 300, 1)
STEPS, LR = 30, 0.1                     # tests/test_gpu_fit_scan.py's


@pytest.fixture(scope="module")
def scan_setup(mesh_ops):
    from cape_amd import smpl
    from test_gpu_smpl import _cape_model
    model = _cape_model(mesh_ops, batch_size=2)
    m = synth.smpl_like(seed=6)
    body = smpl.SMPL(m)
    rng = np.random.default_rng(31)
    cond, cond2 = rng.standard_normal((SIZE, model.nz_cond)), rng.standard_normal((SIZE, model.nz_cond2))
    z_true = rng.standard_normal((SIZE, model.nz)).astype(np.float32)
    pose = np.load(os.path.join(GOLD, "demo_pose_params.npz"))["pose"][rng.integers(0, 6, SIZE)]
    st = np.load(os.path.join(GOLD, "trainset_stats.npz"))
    idx = np.load(os.path.join(GOLD, "clothing_verts_idx.npy"))
    dress = (st["mean"], st["std"], idx)
    posed, _ = model.decode_posed(np.concatenate([z_true, cond, cond2], 1), cond, cond2, pose, body, *dress)
    faces = np.asarray(m["f"], dtype=np.int64)
    scan = [R.surface_samples(rng, posed[n].astype(np.float64), faces, m_n)[0].astype(np.float32)
            for n, m_n in enumerate(COUNTS)]
    z0 = (z_true + rng.standard_normal(z_true.shape)).astype(np.float32)
    # a partial scan of sample 0: surface samples from the faces whose centroid lies above the body's median height
    x0 = posed[0].astype(np.float64)
    upper = faces[x0[faces].mean(1)[:, 1] > np.median(x0[:, 1])]
    partial = R.surface_samples(rng, x0, upper, 600)[0].astype(np.float32)
    return dict(model=model, body=body, faces=faces, cond=cond, cond2=cond2, z_true=z_true, z0=z0, pose=pose, dress=dress,
                posed=posed, scan=scan, partial=partial)


def _fit(s, scan, sl=slice(0, SIZE), **kw):
    return s["model"].fit_scan(scan, s["pose"][sl], s["cond"][sl], s["cond2"][sl], s["body"], *s["dress"], **kw)


def _weighted_mean(e2, w, limit=np.inf):
    e2 = e2.astype(np.float64)
    return float((w * (e2 <= limit) * e2).sum() / w.sum())


def test_lambda_mesh_zero_is_todays_fit_and_builds_nothing(scan_setup):
    s = scan_setup
    body = s["body"]
    body._point = None                                     # whatever ran before: the default path must not build one
    kw = dict(z0=s["z0"], steps=3, lr=LR, max_dist=0.5)
    plain = _fit(s, s["scan"], **kw)
    explicit = _fit(s, s["scan"], lambda_mesh=0.0, mesh_weights=np.ones(body.V), mesh_max_dist=0.05, **kw)
    assert body._point is None                             # SMPL's PointDistance is never constructed
    assert set(plain) == set(explicit) == {"z", "pose", "transl", "posed", "clothed", "loss", "inliers"}
    for k in plain:
        if plain[k] is None:
            assert explicit[k] is None
        else:
            assert plain[k].tobytes() == explicit[k].tobytes() and plain[k].dtype == explicit[k].dtype, k


def test_a_scan_of_the_meshs_own_vertices_has_no_distance(scan_setup):
    s = scan_setup
    V = s["posed"].shape[1]
    res = _fit(s, s["posed"], z0=s["z_true"], steps=0, lambda_mesh=1.0)
    assert res["mesh_loss"].shape == (1, SIZE) and res["mesh_inliers"].shape == (1, SIZE)
    print("mesh_loss of a scan of the own vertices:", res["mesh_loss"][0])
    assert np.all(res["mesh_loss"][0] <= 1e-12) and np.all(res["mesh_inliers"][0] == V)
    assert np.all(res["loss"][0] <= 1e-12) and res["posed"].tobytes() == s["posed"].tobytes()


def test_two_sided_fit_lowers_the_mesh_term_and_leaves_the_model_alone(scan_setup):
    from test_gpu_smpl_grad import _assert_model_untouched, _snapshot
    s = scan_setup
    model, body = s["model"], s["body"]
    V = body.V
    before = _snapshot(model)
    views = model._grad_views
    din = (np.concatenate([s["z_true"], s["cond"], s["cond2"]], 1), s["cond"], s["cond2"])
    dout = model.decode(din[0], cond=din[1], cond2=din[2])
    res = _fit(s, s["scan"], z0=s["z0"], steps=STEPS, lr=LR, lambda_mesh=1.0)
    assert res["mesh_loss"].shape == (STEPS + 1, SIZE) and res["mesh_inliers"].shape == (STEPS + 1, SIZE)
    print("fit_scan two-sided: mesh_loss before %s after %s; loss before %s after %s"
          % (res["mesh_loss"][0], res["mesh_loss"][-1], res["loss"][0], res["loss"][-1]))
    assert np.isfinite(res["mesh_loss"]).all() and np.all(res["mesh_loss"][-1] < res["mesh_loss"][0])
    assert np.isfinite(res["loss"]).all()
    assert np.array_equal(res["mesh_inliers"], np.full((STEPS + 1, SIZE), V))
    assert np.array_equal(res["inliers"], np.broadcast_to(COUNTS, (STEPS + 1, SIZE)))
    # the returned leaves as decode_posed evaluates them: the same bits
    zt = np.concatenate([res["z"], s["cond"], s["cond2"]], 1)
    posed, clothed = model.decode_posed(zt, s["cond"], s["cond2"], s["pose"], body, *s["dress"])
    assert np.array_equal(res["posed"], posed) and np.array_equal(res["clothed"], clothed)
    # and the last row is the weighted mean (weights: ones) of their distance to the scans
    e2, index = body.point_distance_np(res["posed"], s["scan"])
    assert all((index[n] >= 0).all() and (index[n] < m).all() for n, m in enumerate(COUNTS))
    want = np.array([_weighted_mean(e2[n], np.ones(V)) for n in range(SIZE)])
    assert np.abs(res["mesh_loss"][-1] - want).max() <= 1e-6 * want.max()
    _assert_model_untouched(model, before, din, dout)
    assert model._grad_views is views
    # the term must matter: without it the fit ends elsewhere
    one_sided = _fit(s, s["scan"], z0=s["z0"], steps=STEPS, lr=LR)
    assert "mesh_loss" not in one_sided
    moved = np.abs(res["z"] - one_sided["z"]).max(1)
    print("two-sided vs one-sided fit, max |dz| per sample:", moved)
    assert np.all(moved > 1e-2 * LR), "the mesh-to-scan term does not reach the gradient: the comparison shows nothing"
    assert res["loss"][0].tobytes() == one_sided["loss"][0].tobytes()      # loss keeps its meaning: the scan-to-mesh term only


def test_mesh_weights(scan_setup):
    s = scan_setup
    V = s["body"].V
    w = np.ones(V, np.float32)
    w[np.random.default_rng(5).permutation(V)[:V // 2]] = 0.0
    w[w > 0] = np.random.default_rng(6).uniform(0.5, 2.0, int((w > 0).sum()))
    res = _fit(s, s["scan"], z0=s["z0"], steps=0, lambda_mesh=0.5, mesh_weights=w)
    e2, _ = s["body"].point_distance_np(res["posed"], s["scan"])
    want = np.array([_weighted_mean(e2[n], w.astype(np.float64)) for n in range(SIZE)])
    assert np.abs(res["mesh_loss"][0] - want).max() <= 1e-6 * want.max()
    assert np.all(res["mesh_inliers"][0] == int((w > 0).sum()))
    plain = _fit(s, s["scan"], z0=s["z0"], steps=0, lambda_mesh=0.5)
    assert np.abs(plain["mesh_loss"][0] - want).max() > 1e-3 * want.max()          # the weights are not ignored


def test_mesh_max_dist_on_a_partial_scan(scan_setup):
    s = scan_setup
    body = s["body"]
    V = body.V
    sl = slice(0, 1)
    res = _fit(s, [s["partial"]], sl, z0=s["z0"][sl], steps=0, lambda_mesh=1.0, mesh_max_dist=0.05)
    e2, _ = body.point_distance_np(res["posed"], [s["partial"]])
    near = e2[0].astype(np.float64) <= 0.05 ** 2           # steps = 0: the row comes from the same kernels on the same bits
    print("partial scan: %d of %d vertices within 0.05" % (near.sum(), V))
    assert 0 < near.sum() < V and res["mesh_inliers"][0, 0] == near.sum()
    want = _weighted_mean(e2[0], np.ones(V), 0.05 ** 2)
    assert abs(res["mesh_loss"][0, 0] - want) <= 1e-6 * want
    # the step-0 gradient through the primitive alone: the masked seed against the same seed with the far vertices' weights
    # set to zero (what fit_scan seeds with mesh_weights = the mask, up to the normalisation)
    pts = torch.as_tensor(s["partial"][None]).cuda()
    grads = []
    for masked in (True, False):
        x = torch.as_tensor(res["posed"]).cuda().requires_grad_(True)
        d2 = body.point_distance_diff(x, pts)
        mask = (d2.detach() <= 0.05 ** 2).float()
        assert int(mask.sum()) == near.sum()
        seed = mask / V if masked else torch.as_tensor(near[None].astype(np.float32)).cuda() / V
        d2.backward(seed)
        grads.append(x.grad.cpu().numpy().astype(np.float64))
    rel = np.sqrt(((grads[0] - grads[1]) ** 2).sum() / (grads[1] ** 2).sum())
    print("step-0 gradient, far vertices masked vs weighted out: relative L2 %.2e" % rel)
    assert rel <= 1e-6 and not grads[0][0, ~near].any() and grads[0][0, near].any()
    # and through fit_scan: the mask and the zero weights take the same first steps
    kw = dict(z0=s["z0"][sl], steps=2, lr=LR, lambda_mesh=1.0)
    cut = _fit(s, [s["partial"]], sl, mesh_max_dist=0.05, **kw)
    uncut = _fit(s, [s["partial"]], sl, **kw)
    assert cut["mesh_inliers"][0, 0] == near.sum() and uncut["mesh_inliers"][0, 0] == V
    assert np.abs(cut["z"] - uncut["z"]).max() > 1e-2 * LR, "the far vertices do not move the fit: the comparison shows nothing"


def test_samples_are_independent(scan_setup):
    """A sample fitted alone and in a batch takes the same steps: the bar of tests/test_gpu_fit_scan.py, 1e-4 lr."""
    s = scan_setup
    kw = dict(steps=3, lr=LR, lambda_mesh=1.0)
    full = _fit(s, s["scan"], z0=s["z0"], **kw)
    for n in (0, 2):                                         # 2: alone in its padded batch already; 0: shares one with 1
        alone = _fit(s, [s["scan"][n]], slice(n, n + 1), z0=s["z0"][n:n + 1], **kw)
        d = float(np.abs(alone["z"][0] - full["z"][n]).max())
        print("sample %d alone vs in a batch: %.3e" % (n, d))
        assert d <= 1e-4 * LR
        assert abs(alone["mesh_loss"][0, 0] - full["mesh_loss"][0, n]) <= 1e-5 * full["mesh_loss"][0, n]


def test_argument_refusals(scan_setup):
    s = scan_setup
    good, V = s["scan"], s["body"].V
    for kw in (dict(lambda_mesh=-1.0), dict(lambda_mesh=float("nan")), dict(lambda_mesh=float("inf")),
               dict(lambda_mesh=1.0, mesh_max_dist=-0.1), dict(lambda_mesh=1.0, mesh_max_dist=float("nan")),
               dict(lambda_mesh=1.0, mesh_weights=np.ones(V - 1)), dict(lambda_mesh=1.0, mesh_weights=np.ones((V, 3))),
               dict(lambda_mesh=1.0, mesh_weights=np.zeros(V)), dict(mesh_weights=np.zeros(V))):
        with pytest.raises(ValueError):
            _fit(s, good, steps=0, **kw)
    with pytest.raises(TypeError):
        _fit(s, good, steps=0, lambda_mesh=1.0, weights=np.ones(V))     # the scan-to-mesh side still has no per-vertex weights
