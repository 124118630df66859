"""CAPE.fit_scan with normal-compatible correspondences (``scan_normals``, ``normal_angle``): the filter on the
scan-to-mesh term and, with ``lambda_mesh``, on the mesh-to-scan term.  Model, body and scans as tests/test_gpu_fit_scan.py
builds them (the same random stream, so the same scans), with the normal of the face every scan point was sampled on; three
samples in batches of two, so the last batch is padded."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_distance_reference as R     # noqa: E402
import smpl_synth as synth              # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
SIZE = 3
COUNTS = (512, 300, 1)
STEPS, LR = 30, 0.1                     # tests/test_gpu_fit_scan.py's
COS60 = float(np.cos(np.deg2rad(60.0)))


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
    samples = [R.surface_samples(rng, posed[n].astype(np.float64), faces, m_n) for n, m_n in enumerate(COUNTS)]
    scan, normals = [a.astype(np.float32) for a, _ in samples], [b.astype(np.float32) for _, b in samples]
    z0 = (z_true + rng.standard_normal(z_true.shape)).astype(np.float32)
    return dict(model=model, body=body, faces=faces, cond=cond, cond2=cond2, z_true=z_true, z0=z0, pose=pose, dress=dress,
                posed=posed, scan=scan, normals=normals)


def _fit(s, scan, sl=slice(0, SIZE), **kw):
    return s["model"].fit_scan(scan, s["pose"][sl], s["cond"][sl], s["cond2"][sl], s["body"], *s["dress"], **kw)


def test_without_scan_normals_it_is_todays_fit_and_builds_nothing(scan_setup):
    s = scan_setup
    body = s["body"]
    body._normals = None                                   # whatever ran before: the default path must not build one
    kw = dict(z0=s["z0"], steps=3, lr=LR, max_dist=0.5, lambda_mesh=1.0)
    plain = _fit(s, s["scan"], **kw)
    explicit = _fit(s, s["scan"], scan_normals=None, normal_angle=None, **kw)
    assert body._normals is None                           # no vertex normals without the filter
    assert set(plain) == set(explicit) == {"z", "pose", "transl", "posed", "clothed", "loss", "inliers", "mesh_loss", "mesh_inliers"}
    for k in plain:
        if plain[k] is None:
            assert explicit[k] is None
        else:
            assert plain[k].tobytes() == explicit[k].tobytes() and plain[k].dtype == explicit[k].dtype, k
    filtered = _fit(s, s["scan"], scan_normals=s["normals"], normal_angle=60.0, **kw)
    assert set(filtered) == set(plain) and body._normals is not None
    assert filtered["loss"].tobytes() != plain["loss"].tobytes() or filtered["mesh_loss"].tobytes() != plain["mesh_loss"].tobytes()


def test_a_scan_of_the_meshs_own_vertices_with_its_own_normals(scan_setup):
    """A vertex normal is the normalised sum of its faces' unit normals, so it has a positive dot product with at least one of
    them: at 90 degrees every vertex keeps a face it is a corner of, at distance exactly 0."""
    s = scan_setup
    V = s["posed"].shape[1]
    own = s["body"].vertex_normals_np(s["posed"])
    res = _fit(s, s["posed"], z0=s["z_true"], steps=0, scan_normals=own, normal_angle=90.0)
    print("loss of a scan of the own vertices with the own normals:", res["loss"][0], res["inliers"][0])
    assert np.all(res["loss"][0] == 0.0) and np.all(res["inliers"][0] == V)
    assert np.array_equal(res["z"], s["z_true"]) and res["posed"].tobytes() == s["posed"].tobytes()
    # every normal negated: a vertex now finds the far side of a sheet or a limb, or nothing
    plain = _fit(s, s["posed"], z0=s["z_true"], steps=0, max_dist=0.01)
    flipped = _fit(s, s["posed"], z0=s["z_true"], steps=0, max_dist=0.01, scan_normals=-own, normal_angle=90.0)
    print("negated normals: loss %s (plain %s), inliers %s (plain %s)"
          % (flipped["loss"][0], plain["loss"][0], flipped["inliers"][0], plain["inliers"][0]))
    assert np.all(flipped["loss"][0] > plain["loss"][0]) and np.all(flipped["inliers"][0] < plain["inliers"][0])


def test_filtered_fit_lowers_the_distance_and_leaves_the_model_alone(scan_setup):
    from test_gpu_smpl_grad import _assert_model_untouched, _snapshot
    s = scan_setup
    model, body = s["model"], s["body"]
    before = _snapshot(model)
    views = model._grad_views
    din = (np.concatenate([s["z_true"], s["cond"], s["cond2"]], 1), s["cond"], s["cond2"])
    dout = model.decode(din[0], cond=din[1], cond2=din[2])
    res = _fit(s, s["scan"], z0=s["z0"], steps=STEPS, lr=LR, scan_normals=s["normals"], normal_angle=60.0)
    assert set(res) == {"z", "pose", "transl", "posed", "clothed", "loss", "inliers"}
    print("filtered fit_scan: loss before %s after %s, inliers before %s after %s"
          % (res["loss"][0], res["loss"][-1], res["inliers"][0], res["inliers"][-1]))
    assert np.isfinite(res["loss"]).all() and np.all(res["loss"][-1] < res["loss"][0])
    assert np.all(res["inliers"] <= np.array(COUNTS)[None])
    zt = np.concatenate([res["z"], s["cond"], s["cond2"]], 1)
    posed, clothed = model.decode_posed(zt, s["cond"], s["cond2"], s["pose"], body, *s["dress"])
    assert np.array_equal(res["posed"], posed) and np.array_equal(res["clothed"], clothed)
    # the last row: the mean over the points with a compatible face, times their share
    d2, face, _ = body.scan_distance_np(posed, s["scan"], normals=s["normals"], cos_min=COS60)
    want = np.zeros(SIZE)
    for n, m in enumerate(COUNTS):
        ok = np.isfinite(d2[n, :m])
        assert np.array_equal(ok, face[n, :m] >= 0) and res["inliers"][-1, n] == ok.sum()
        want[n] = d2[n, :m][ok].astype(np.float64).mean() * ok.sum() / m if ok.any() else 0.0
    assert np.abs(res["loss"][-1] - want).max() <= 1e-6 * want.max()
    _assert_model_untouched(model, before, din, dout)
    assert model._grad_views is views
    # the filter must matter: without it the fit ends elsewhere
    plain = _fit(s, s["scan"], z0=s["z0"], steps=STEPS, lr=LR)
    assert np.abs(res["z"] - plain["z"]).max() > 1e-2 * LR, "the filter does not reach the gradient: the comparison shows nothing"


def test_the_mesh_term_is_filtered_too(scan_setup):
    s = scan_setup
    body = s["body"]
    V = body.V
    kw = dict(z0=s["z0"], steps=3, lr=LR, lambda_mesh=1.0)
    res = _fit(s, s["scan"], scan_normals=s["normals"], normal_angle=60.0, **kw)
    plain = _fit(s, s["scan"], **kw)
    assert np.all(res["mesh_inliers"] <= plain["mesh_inliers"]) and np.all(res["mesh_inliers"][:, 2] < V)
    e2, index = body.point_distance_np(res["posed"], s["scan"], point_normals=s["normals"], cos_min=COS60)
    want = np.zeros(SIZE)
    for n in range(SIZE):
        ok = np.isfinite(e2[n])
        assert np.array_equal(ok, index[n] >= 0) and res["mesh_inliers"][-1, n] == ok.sum()
        want[n] = e2[n][ok].astype(np.float64).sum() / V
    print("filtered mesh term: mesh_loss %s, mesh_inliers %s of %d" % (res["mesh_loss"][-1], res["mesh_inliers"][-1], V))
    assert np.abs(res["mesh_loss"][-1] - want).max() <= 1e-6 * want.max()
    d2, _, _ = body.scan_distance_np(res["posed"], s["scan"], normals=s["normals"], cos_min=COS60)
    near = np.array([np.nansum(d2[n, :m].astype(np.float64)) / m for n, m in enumerate(COUNTS)])
    assert np.abs(res["loss"][-1] - near).max() <= 1e-6 * near.max()


def test_samples_are_independent(scan_setup):
    """A sample fitted alone and in a batch takes the same steps: the bar of tests/test_gpu_fit_scan.py, 1e-4 lr."""
    s = scan_setup
    kw = dict(steps=3, lr=LR, lambda_mesh=1.0, normal_angle=60.0)
    full = _fit(s, s["scan"], z0=s["z0"], scan_normals=s["normals"], **kw)
    for n in (0, 2):                                         # 2: alone in its padded batch already; 0: shares one with 1
        alone = _fit(s, [s["scan"][n]], slice(n, n + 1), z0=s["z0"][n:n + 1], scan_normals=[s["normals"][n]], **kw)
        d = float(np.abs(alone["z"][0] - full["z"][n]).max())
        print("sample %d alone vs in a batch: %.3e" % (n, d))
        assert d <= 1e-4 * LR
        assert alone["inliers"][0, 0] == full["inliers"][0, n] and alone["mesh_inliers"][0, 0] == full["mesh_inliers"][0, n]


def test_argument_refusals(scan_setup):
    s = scan_setup
    good, nrm = s["scan"], s["normals"]
    for kw in (dict(scan_normals=nrm), dict(normal_angle=60.0), dict(scan_normals=nrm, normal_angle=0.0),
               dict(scan_normals=nrm, normal_angle=180.0), dict(scan_normals=nrm, normal_angle=-1.0),
               dict(scan_normals=nrm, normal_angle=float("nan")), dict(scan_normals=nrm[:2], normal_angle=60.0),
               dict(scan_normals=[nrm[0], nrm[1][:299], nrm[2]], normal_angle=60.0),
               dict(scan_normals=[nrm[1], nrm[0], nrm[2]], normal_angle=60.0),
               dict(scan_normals=[a[:, :2] for a in nrm], normal_angle=60.0)):
        with pytest.raises(ValueError):
            _fit(s, good, steps=0, **kw)
