"""CAPE.fit_scan: latent fitting to raw scans -- points without correspondence -- through the scan-to-mesh distance on the device
(cape_amd/scan_distance.py).  Model and body as the fit_posed tests of tests/test_gpu_smpl_grad.py build them; three samples in
batches of two, so the last batch is padded."""
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
STEPS, LR = 30, 0.1                     # test_fit_posed_lowers_the_data_term_and_leaves_the_model_alone's


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
            for n, m_n in enumerate((512, 300, 1))]
    z0 = (z_true + rng.standard_normal(z_true.shape)).astype(np.float32)
    return dict(model=model, body=body, faces=faces, cond=cond, cond2=cond2, z_true=z_true, z0=z0, pose=pose, dress=dress,
                posed=posed, scan=scan)


def _fit(s, scan, sl=slice(0, SIZE), **kw):
    return s["model"].fit_scan(scan, s["pose"][sl], s["cond"][sl], s["cond2"][sl], s["body"], *s["dress"], **kw)


def test_a_scan_of_the_meshs_own_vertices_has_no_distance(scan_setup):
    s = scan_setup
    res = _fit(s, s["posed"], z0=s["z_true"], steps=0)
    assert res["loss"].shape == (1, SIZE) and res["inliers"].shape == (1, SIZE) and res["transl"] is None
    print("loss of a scan of the own vertices:", res["loss"][0])
    assert np.all(res["loss"][0] <= 1e-12) and np.all(res["inliers"][0] == s["posed"].shape[1])
    assert np.array_equal(res["z"], s["z_true"]) and res["posed"].tobytes() == s["posed"].tobytes()


def test_fit_scan_lowers_the_distance_and_leaves_the_model_alone(scan_setup):
    from test_gpu_smpl_grad import _assert_model_untouched, _snapshot
    s = scan_setup
    model = s["model"]
    before = _snapshot(model)
    views = model._grad_views
    din = (np.concatenate([s["z_true"], s["cond"], s["cond2"]], 1), s["cond"], s["cond2"])
    dout = model.decode(din[0], cond=din[1], cond2=din[2])
    res = _fit(s, s["scan"], z0=s["z0"], steps=STEPS, lr=LR)
    assert res["z"].shape == (SIZE, model.nz) and res["loss"].shape == (STEPS + 1, SIZE)
    print("fit_scan: loss before %s after %s (ratio %s)" % (res["loss"][0], res["loss"][-1], res["loss"][-1] / res["loss"][0]))
    assert np.isfinite(res["loss"]).all() and np.all(res["loss"][-1] < res["loss"][0])
    assert np.all(np.abs(res["z"] - s["z0"]).max(1) > 0)
    assert np.array_equal(res["inliers"], np.broadcast_to([512, 300, 1], (STEPS + 1, SIZE)))
    assert np.array_equal(res["pose"], s["pose"].astype(np.float32))
    # the returned leaves as decode_posed evaluates them: the same bits
    zt = np.concatenate([res["z"], s["cond"], s["cond2"]], 1)
    posed, clothed = model.decode_posed(zt, s["cond"], s["cond2"], s["pose"], s["body"], *s["dress"])
    assert np.array_equal(res["posed"], posed) and np.array_equal(res["clothed"], clothed)
    # and the last loss row is their distance
    d2, _, _ = s["body"].scan_distance_np(posed, s["scan"])
    want = np.array([d2[n, :m].astype(np.float64).mean() for n, m in enumerate((512, 300, 1))])
    assert np.abs(res["loss"][-1] - want).max() <= 1e-6 * want.max()
    _assert_model_untouched(model, before, din, dout)
    assert model._grad_views is views
    # pose and translation as leaves: they move, and the bookkeeping holds
    res_p = _fit(s, s["scan"], z0=s["z0"], steps=3, lr=LR, optimize_pose=True, optimize_transl=True)
    assert res_p["transl"].shape == (SIZE, 3) and np.all(np.abs(res_p["transl"]).max(1) > 0)
    assert np.all(np.abs(res_p["pose"] - s["pose"].astype(np.float32)).max(1) > 0)
    _assert_model_untouched(model, before, din, dout)


def test_max_dist_drops_the_outliers(scan_setup):
    s = scan_setup
    clean = s["scan"][0]
    m = len(clean)
    outliers = clean[:50].copy()
    outliers[:, 0] = s["posed"][0][:, 0].max() + 1.0          # 1 m beyond the body
    dirty = np.concatenate([clean, outliers])
    sl = slice(0, 1)
    kw = dict(z0=s["z0"][sl], steps=3, lr=LR)
    cut = _fit(s, [dirty], sl, max_dist=0.1, **kw)
    assert np.array_equal(cut["inliers"][:, 0], np.full(4, m))
    assert np.all(_fit(s, [dirty], sl, **kw)["inliers"][:, 0] == m + 50)
    plain = _fit(s, [clean], sl, **kw)
    uncut = _fit(s, [dirty], sl, **kw)
    assert np.abs(uncut["z"] - plain["z"]).max() > 1e-2 * LR, "the outliers do not move the fit: the comparison shows nothing"
    # the data term counts the inliers only, normalised by all m + 50 points
    assert np.abs(cut["loss"][0] * (m + 50) / m - plain["loss"][0]).max() <= 1e-5 * plain["loss"][0].max()
    # the step-0 gradient through the primitive alone: the masked seed 1 / (m + 50) on the dirty scan against the same seed on
    # the clean one (what fit_scan seeds, up to the normalisation m / (m + 50))
    body = s["body"]
    zt = np.concatenate([s["z0"][sl], s["cond"][sl], s["cond2"][sl]], 1)
    posed0, _ = s["model"].decode_posed(zt, s["cond"][sl], s["cond2"][sl], s["pose"][sl], body, *s["dress"])
    grads = []
    for pts in (dirty, clean):
        x = torch.as_tensor(posed0).cuda().requires_grad_(True)
        d2 = body.scan_distance_diff(x, torch.as_tensor(pts[None]).cuda())
        mask = (d2.detach() <= 0.1 ** 2).float()
        assert int(mask.sum()) == m
        d2.backward(mask / (m + 50))
        grads.append(x.grad.cpu().numpy().astype(np.float64))
    rel = np.sqrt(((grads[0] - grads[1]) ** 2).sum() / (grads[1] ** 2).sum())
    print("step-0 gradient, outliers masked vs absent: relative L2 %.2e" % rel)
    assert rel <= 1e-6


def test_samples_are_independent(scan_setup):
    """A sample fitted alone and in a batch takes the same steps: fit_posed's bar of 1e-4 lr (its edge-term test has the
    argument: Adam's step moves by at most lr / 4 times the relative error of the gradient)."""
    s = scan_setup
    kw = dict(steps=3, lr=LR)
    full = _fit(s, s["scan"], z0=s["z0"], **kw)
    for n in (0, 2):                                         # 2: alone in its padded batch already; 0: shares one with 1
        alone = _fit(s, [s["scan"][n]], slice(n, n + 1), z0=s["z0"][n:n + 1], **kw)
        d = float(np.abs(alone["z"][0] - full["z"][n]).max())
        print("sample %d alone vs in a batch: %.3e" % (n, d))
        assert d <= 1e-4 * LR
        assert abs(alone["loss"][0, 0] - full["loss"][0, n]) <= 1e-5 * full["loss"][0, n]


def test_argument_refusals(scan_setup):
    s = scan_setup
    good = s["scan"]
    for bad in (np.zeros((SIZE, 10, 2), np.float32), np.zeros((SIZE, 0, 3), np.float32), np.zeros((10, 3), np.float32), [],
                [good[0], good[1], np.zeros((0, 3), np.float32)], [good[0], good[1], np.zeros((4, 2), np.float32)]):
        with pytest.raises(ValueError):
            _fit(s, bad, steps=0)
    with pytest.raises(ValueError):
        _fit(s, good[:2], steps=0)                           # two scans for three poses
    with pytest.raises(ValueError):
        _fit(s, good, steps=0, max_dist=-0.1)
    with pytest.raises(ValueError):
        _fit(s, good, steps=0, max_dist=float("nan"))
    with pytest.raises(ValueError):
        _fit(s, good, steps=0, z0=np.zeros((SIZE, s["model"].nz + 1), np.float32))
    with pytest.raises(TypeError):
        _fit(s, good, steps=0, weights=np.ones(6890))        # no correspondences: no per-vertex weights
