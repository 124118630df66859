"""CPU checks of SMPL posing (cape_amd.smpl, include/cape_hip.h "SMPL posing"): analytic pins of the numpy formulation the
GPU tests hold the kernels to, the model loader, the host argument checks of the C entries, and the smplx-compatible
object demos.py drives."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smpl_reference as ref    # noqa: E402
import smpl_synth as synth      # noqa: E402


def _pose(rng, N, J, scale=0.4):
    return scale * rng.standard_normal((N, 3 * J))


def test_zero_pose_gives_the_template():
    m = synth.small()
    v, j = ref.forward(m, m["v_template"][None], np.zeros((2, 15)))
    np.testing.assert_allclose(v, np.broadcast_to(m["v_template"], v.shape), atol=1e-13)
    np.testing.assert_allclose(j[0], m["J_regressor"].toarray() @ m["v_template"], atol=1e-13)
    assert np.array_equal(ref.rodrigues(np.zeros(3)), np.eye(3))


def test_root_only_rotation_is_a_rigid_motion_about_joint_0():
    m = synth.smpl_like()
    r0 = np.array([0.3, -1.1, 0.7])
    pose = np.zeros((1, 72))
    pose[0, :3] = r0
    tr = np.array([[0.1, -0.2, 0.05]])
    v, _ = ref.forward(m, m["v_template"][None], pose, transl=tr)
    R = ref.rodrigues(r0)
    J0 = m["J_regressor"].toarray()[0] @ m["v_template"]
    want = (m["v_template"] - J0) @ R.T + J0 + tr
    np.testing.assert_allclose(v[0], want, atol=1e-12)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
    # the small-angle series meets the closed form
    for r in (np.array([3e-4, 0, 0]), np.array([1e-3, 2e-4, -5e-4])):
        t = np.linalg.norm(r)
        K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / t
        np.testing.assert_allclose(ref.rodrigues(r), np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K, atol=1e-15)


def test_pose_blend_is_linear_in_the_pose_feature():
    m = synth.small()
    m["weights"] = np.zeros_like(m["weights"])
    m["weights"][:, 0] = 1.0                     # every vertex on the root, root unrotated: output = v_posed
    rng = np.random.default_rng(3)
    pa, pb = _pose(rng, 1, 5), _pose(rng, 1, 5)
    pa[0, :3] = pb[0, :3] = 0
    T = m["v_template"][None]
    oa, ob = (ref.forward(m, T, p, full=True) for p in (pa, pb))
    np.testing.assert_allclose(oa["vertices"], oa["v_posed"], atol=1e-13)
    off = lambda pf: np.einsum("vck,nk->nvc", m["posedirs"], pf)
    np.testing.assert_allclose(oa["v_posed"] - T, off(oa["pf"]), atol=1e-14)
    np.testing.assert_allclose(off(oa["pf"] + ob["pf"]), (oa["v_posed"] - T) + (ob["v_posed"] - T), atol=1e-14)


def test_pose_feature_index_order_matches_the_posedirs_layout():
    """pf[(j-1)*9 + 3r + c] = R_j[r, c] - delta_rc: rotate joint j alone, give posedirs a single nonzero column."""
    m = synth.small()
    m["weights"] = np.zeros_like(m["weights"])
    m["weights"][:, 0] = 1.0
    j, r, c = 3, 1, 2
    pose = np.zeros((1, 15))
    pose[0, 3 * j:3 * j + 3] = [0.2, -0.5, 0.9]
    m["posedirs"] = np.zeros_like(m["posedirs"])
    m["posedirs"][:, :, (j - 1) * 9 + 3 * r + c] = 1.0
    v, _ = ref.forward(m, m["v_template"][None], pose)
    want = ref.rodrigues(pose[0, 3 * j:3 * j + 3])[r, c]
    np.testing.assert_allclose(v[0] - m["v_template"], want, atol=1e-14)


def test_loader_round_trips_npz_and_pkl(tmp_path):
    from cape_amd import smpl
    m = synth.small()
    a = smpl.load_smpl_model(synth.write_npz(m, str(tmp_path / "m.npz")), num_betas=4)
    b = smpl.load_smpl_model(synth.write_pkl(m, str(tmp_path / "m.pkl")), num_betas=4)
    for x in (a, b):
        assert (x.J, x.V, x.num_betas) == (5, 37, 4)
        assert list(x.parents) == list(ref.parents_of(m)) and x.parents[0] == -1
        np.testing.assert_allclose(x.host["J_regressor"].toarray(), m["J_regressor"].toarray())
        basis = x.layouts["basis"][0]
        assert basis.shape == (4 + 9 * 4, 3, 37)
        np.testing.assert_array_equal(basis[4:], m["posedirs"].transpose(2, 1, 0))
        np.testing.assert_array_equal(basis[:4], m["shapedirs"][:, :, :4].transpose(2, 1, 0))
        # ELL of the skinning weights reproduces the dense matrix
        ej, ew = x.layouts["ell_j"][0], x.layouts["ell_w"][0]
        dense = np.zeros((37, 5))
        for w in range(x.ell_width):
            np.add.at(dense, (np.arange(37), ej[w]), ew[w])
        np.testing.assert_allclose(dense, m["weights"], atol=1e-7)
        assert x.ell_width <= 4


def test_loader_rejects_unordered_trees_and_chumpy(tmp_path):
    from cape_amd import smpl
    m = synth.small()
    m["kintree_table"] = m["kintree_table"].copy()
    m["kintree_table"][0, 2] = 3
    with pytest.raises(ValueError, match="parent-ordered"):
        smpl.SMPL(m)
    # a pickle that needs chumpy: its class lives in a module that is not installed
    path = tmp_path / "SMPL_MALE.pkl"
    path.write_bytes(b"\x80\x02cchumpy.ch\nCh\nq\x00.")
    with pytest.raises(ValueError, match="chumpy"):
        smpl.read_model_file(str(path))


def test_create_follows_the_smplx_path_convention(tmp_path):
    from cape_amd import smpl
    m = synth.smpl_like()
    synth.write_pkl(m, str(tmp_path / "smpl" / "SMPL_FEMALE.pkl"))
    layer = smpl.body_models.create(model_type='smpl', model_path=str(tmp_path), gender='female')
    import torch
    for name, shape in (("v_template", (6890, 3)), ("body_pose", (1, 69)), ("global_orient", (1, 3)), ("transl", (1, 3)),
                        ("betas", (1, 10))):
        t = getattr(layer, name)
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == shape and t.device.type == "cpu"
    assert layer.faces.shape == m["f"].shape
    np.testing.assert_allclose(layer.v_template.numpy(), m["v_template"], rtol=1e-6)
    layer.body_pose[:] = torch.from_numpy(np.ones(69))           # demos.py:268-269 writes float64 rows in place
    layer.global_orient[:] = torch.from_numpy(np.ones(3))
    with pytest.raises(FileNotFoundError):
        smpl.create(str(tmp_path), gender='male')
    with pytest.raises(ValueError):
        smpl.create(str(tmp_path), model_type='smplx', gender='female')


def test_smpl_entry_points_reject_bad_arguments_before_launching():
    """J > 64, a tree that is not parent-ordered and NULL operands return their CAPE_E* code without a launch."""
    from cape_amd._lib import lib
    P = C.c_void_p
    p = [P(0x100000 + 0x1000 * i) for i in range(12)]
    smpl_parents = synth.SMPL_PARENTS

    def joints(J=24, parents=None, T=p[0], pose=p[4], coef=p[8], G=p[9], B=10, betas=p[5]):
        par = (C.c_int32 * max(J, 1))(*(parents if parents is not None else ([-1] + [0] * (J - 1))))
        return lib.cape_smpl_joints(T, 0, p[1], p[2], p[3], pose, betas, B, p[6], None, par, J, 6890, 4, coef, G, None, None)

    assert joints(J=24, parents=smpl_parents, T=None) == -1          # NULL rest vertices
    assert joints(J=65) == -1                                        # more than 64 joints
    assert joints(J=0) == -1
    bad = list(smpl_parents)
    bad[5] = 7
    assert joints(J=24, parents=bad) == -3                           # parents[j] >= j
    bad = list(smpl_parents)
    bad[0] = 0
    assert joints(J=24, parents=bad) == -3                           # root without parent -1
    assert joints(J=24, parents=smpl_parents, pose=None) == -1
    assert joints(J=24, parents=smpl_parents, betas=None) == -1      # B > 0 without betas
    assert lib.cape_smpl_joints(p[0], 0, p[1], p[2], p[3], p[4], None, 0, None, None, None, 24, 6890, 4, p[8], p[9], None,
                                None) == -1                          # NULL parent table

    def skin(J=24, K=217, T=p[0], out=p[10], W=4, N=4):
        return lib.cape_smpl_skin(T, 0, p[1], K, p[2], p[3], p[4], p[5], W, None, J, 6890, N, out, 3 * 6890, None)

    assert skin(J=65) == -1
    assert skin(T=None) == -1
    assert skin(out=None) == -1
    assert skin(W=0) == -1
    assert skin(N=0) == -1
    assert lib.cape_smpl_dress(None, 3 * 6890, p[1], p[2], p[3], p[4], p[5], 3 * 6890, 2, 6890, None) == -1
    assert lib.cape_smpl_dress(p[0], 3 * 6890, p[1], p[2], p[3], p[4], None, 3 * 6890, 2, 6890, None) == -1
    # samples per skinning workgroup: 16 for SMPL (K = 10 + 9 * 23), fewer where 16 of them do not fit
    assert lib.cape_smpl_skin_tile(217, 24) == 16
    assert 1 <= lib.cape_smpl_skin_tile(10 + 9 * 63, 64) < 16
    assert lib.cape_smpl_skin_tile(217, 65) == -1


def test_fixtures_have_the_shapes_demos_py_reads():
    g = os.path.join(ROOT, "tests", "golden")
    pp = np.load(os.path.join(g, "demo_pose_params.npz"))
    assert pp["pose"].shape == (6, 72)
    st = np.load(os.path.join(g, "trainset_stats.npz"))
    assert st["mean"].shape == st["std"].shape == (6890, 3)
    idx = np.load(os.path.join(g, "clothing_verts_idx.npy"))
    assert idx.ndim == 1 and 0 <= idx.min() and idx.max() < 6890
    d = np.random.default_rng(0).standard_normal((2, 6890, 3))
    minimal = synth.template()
    T = ref.dress(d, st["mean"], st["std"], idx, minimal)
    out = np.setdiff1d(np.arange(6890), idx)
    np.testing.assert_array_equal(T[:, out], np.broadcast_to(minimal[out], (2, len(out), 3)))
