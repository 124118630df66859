"""CPU checks of unposing (cape_amd.smpl.SMPL.unpose / undress, include/cape_hip.h "SMPL posing, inverse"): the numpy
oracle of tests/smpl_unpose_reference.py against the forward oracle it inverts, analytic pins, the array the loader adds,
and the host argument checks of the four C entries."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smpl_reference as ref            # noqa: E402
import smpl_synth as synth              # noqa: E402
import smpl_unpose_reference as uref    # noqa: E402


def _case(m, N, scale, seed, shape=True):
    rng = np.random.default_rng(seed)
    V, J = m["v_template"].shape[0], len(ref.parents_of(m))
    pose = scale * rng.standard_normal((N, 3 * J))
    pose[0] = 0
    T = m["v_template"][None] + 0.01 * rng.standard_normal((N, V, 3))
    betas = 0.8 * rng.standard_normal((N, 10)) if shape else None
    transl = 0.3 * rng.standard_normal((N, 3)) if shape else None
    return T, pose, betas, transl


@pytest.mark.parametrize("which,scale", [("small", 0.3), ("smpl_like", 0.3), ("j52", 0.2)])
def test_oracle_recovers_the_rest_body_from_the_forward_oracle(which, scale):
    m = getattr(synth, which)()
    for shape in (True, False):
        T, pose, betas, transl = _case(m, 3, scale, 103, shape)
        P, joints = ref.forward(m, T, pose, betas, transl)                     # unrounded
        o = uref.unpose(m, P, pose, betas, transl, full=True)
        extent = float(np.ptp(T.reshape(-1, 3), 0).max())
        assert np.abs(o["rest"] - T).max() < 1e-10 * max(extent, 1.0)
        assert np.abs(o["joints"] - joints).max() < 1e-10
        shaped = T if betas is None else T + np.einsum("vck,nk->nvc", m["shapedirs"], betas)
        np.testing.assert_allclose(o["rest_joints"], np.einsum("jv,nvc->njc", m["J_regressor"].toarray(), shaped), atol=1e-10)
        assert o["cond_system"][0] == pytest.approx(1.0, abs=1e-9)             # zero pose: Q L = 0
        assert (o["det_min"] > 0).all() and o["det_min"][0] == pytest.approx(1.0, abs=1e-12)


def test_translation_operator_is_the_chain():
    """G_j.t = (L Jn)_j for the operator the system is built from, on a random tree."""
    m = synth.small()
    parents = ref.parents_of(m)
    rng = np.random.default_rng(5)
    R = ref.rodrigues(0.7 * rng.standard_normal((2, 5, 3)))
    Wr = uref._world_rotations(R, parents, np.float64)
    Jn = rng.standard_normal((2, 5, 3))
    G, _ = uref._transforms(Wr, Jn, parents)
    L = uref.translation_operator(Wr, parents)
    np.testing.assert_allclose((L @ Jn.reshape(2, 15, 1)).reshape(2, 5, 3), G[..., 3], atol=1e-13)


def test_oracle_with_explicit_joints_inverts_the_forward_run_with_them():
    m = synth.smpl_like()
    T, pose, betas, transl = _case(m, 2, 0.3, 7)
    JF = m["v_template"][None]
    P, joints = uref.forward(m, T, pose, betas, transl, joints_from=JF)
    Tb, Jn = uref.unpose(m, P, pose, betas, transl, joints_from=JF)
    assert np.abs(Tb - T).max() < 1e-12
    np.testing.assert_allclose(Jn, np.einsum("jv,nvc->njc", m["J_regressor"].toarray(),
                                             JF + np.einsum("vck,nk->nvc", m["shapedirs"], betas)), atol=1e-13)
    # joints from the body itself is the plain forward; the shortcut against the plain forward is off by centimetres
    P0, _ = ref.forward(m, T, pose, betas, transl)
    np.testing.assert_allclose(uref.forward(m, T, pose, betas, transl, joints_from=T)[0], P0, atol=1e-13)
    off = np.abs(uref.unpose(m, P0, pose, betas, transl, joints_from=JF)[0] - T).max()
    assert 1e-3 < off < 5e-2


def test_zero_pose_unposes_to_the_posed_body_minus_shape_and_translation():
    m = synth.small()
    rng = np.random.default_rng(2)
    P = rng.standard_normal((2, 37, 3))
    betas, transl = rng.standard_normal((2, 10)), rng.standard_normal((2, 3))
    T, Jn = uref.unpose(m, P, np.zeros((2, 15)), betas, transl)
    want = P - transl[:, None] - np.einsum("vck,nk->nvc", m["shapedirs"], betas)
    np.testing.assert_allclose(T, want, atol=1e-13)
    np.testing.assert_allclose(Jn, np.einsum("jv,nvc->njc", m["J_regressor"].toarray(), P - transl[:, None]), atol=1e-13)


def test_undress_inverts_dress_on_the_clothing_vertices():
    g = os.path.join(ROOT, "tests", "golden")
    st = np.load(os.path.join(g, "trainset_stats.npz"))
    idx = np.load(os.path.join(g, "clothing_verts_idx.npy"))
    minimal = synth.template()
    d = np.random.default_rng(0).standard_normal((2, 6890, 3))
    T = ref.dress(d, st["mean"], st["std"], idx, minimal)
    back = uref.undress(T, st["mean"], st["std"], idx, minimal)
    np.testing.assert_allclose(back[:, idx], d[:, idx], atol=1e-12)
    out = np.setdiff1d(np.arange(6890), idx)
    np.testing.assert_allclose(back[:, out], np.broadcast_to((-st["mean"] / st["std"])[out], (2, len(out), 3)), atol=1e-12)
    # right-inverse: dress(undress(T)) = minimal + mask (T - minimal), for any T
    T2 = minimal[None] + 0.02 * np.random.default_rng(1).standard_normal((2, 6890, 3))
    again = ref.dress(uref.undress(T2, st["mean"], st["std"], idx, minimal), st["mean"], st["std"], idx, minimal)
    np.testing.assert_allclose(again[:, idx], T2[:, idx], atol=1e-12)
    np.testing.assert_allclose(again[:, out], np.broadcast_to(minimal[out], (2, len(out), 3)), atol=1e-15)
    every = uref.undress(T2, st["mean"], st["std"], None, minimal)
    np.testing.assert_allclose(every * st["std"] + st["mean"] + minimal, T2, atol=1e-12)


def test_loader_builds_jposedirs_and_forward_diff_refuses_joints_from():
    from cape_amd import smpl
    m = synth.small()
    model = smpl.SMPL(m)
    jpd, dt = model.layouts["jposedirs"]
    assert jpd.shape == (9 * 4, 5, 3) and dt == np.float32
    np.testing.assert_allclose(jpd, np.einsum("jv,vck->kjc", m["J_regressor"].toarray(), m["posedirs"]), atol=1e-15)
    with pytest.raises(NotImplementedError):
        model.forward_diff(None, None, joints_from=object())


def test_the_entries_are_declared_bound_and_leave_the_abi_version_alone():
    from cape_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    for name in ("cape_smpl_unpose_workspace_bytes", "cape_smpl_unpose_joints", "cape_smpl_unpose_skin", "cape_smpl_undress"):
        assert re.search(r"^\s*(?:int|int64_t)\s+%s\s*\(" % name, hdr, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.cape_abi_version() == 18


def test_unpose_entry_points_reject_bad_arguments_before_launching():
    """NULL operands, N < 1, strides below 3V, J > 64, a tree that is not parent-ordered, a short or misaligned workspace and
    element indices beyond 32 bits return their CAPE_E* code without a launch."""
    from cape_amd._lib import lib
    P = C.c_void_p
    p = [P(0x100000 + 0x1000 * i) for i in range(16)]
    V = 6890

    assert lib.cape_smpl_unpose_workspace_bytes(24, 16) == 8 * 16 * 72 * 73
    assert lib.cape_smpl_unpose_workspace_bytes(64, 1) == 8 * 192 * 193
    assert lib.cape_smpl_unpose_workspace_bytes(65, 1) == -1
    assert lib.cape_smpl_unpose_workspace_bytes(0, 1) == -1
    assert lib.cape_smpl_unpose_workspace_bytes(24, 0) == -1

    def joints(J=24, parents=None, posed=p[0], stride=3 * V, pose=p[6], betas=p[7], B=10, jpd=p[8], ws=p[9], ws_bytes=None, coef=p[10],
               G=p[11], N=4, W=4, ell_j=p[4], Vn=V):
        par = (C.c_int32 * max(J, 1))(*(parents if parents is not None else ([-1] + [0] * (J - 1))))
        if ws_bytes is None:
            ws_bytes = max(lib.cape_smpl_unpose_workspace_bytes(J, N), 0)
        return lib.cape_smpl_unpose_joints(posed, stride, p[1], p[2], p[3], ell_j, p[5], W, pose, betas, B, jpd, None, par, J, Vn, N,
                                           ws, ws_bytes, coef, G, None, None, None, None)

    assert joints(posed=None) == -1
    assert joints(pose=None) == -1
    assert joints(coef=None) == -1
    assert joints(G=None) == -1
    assert joints(ell_j=None) == -1
    assert joints(jpd=None) == -1                                    # J > 1 needs jposedirs
    assert joints(betas=None) == -1                                  # B > 0 without betas
    assert joints(B=-1) == -1
    assert joints(J=65) == -1
    assert joints(J=0) == -1
    assert joints(N=0) == -1
    assert joints(stride=3 * V - 1) == -1                            # samples would overlap
    assert joints(W=0) == -1
    assert joints(W=25) == -1
    assert joints(ws=None) == -1
    assert joints(ws=P(0x900004)) == -1                              # fp64 workspace, 8-byte aligned
    assert joints(ws_bytes=8 * 4 * 72 * 73 - 8) == -1                # one word short
    assert joints(Vn=1 << 29, W=4, stride=3 << 29) == -1             # ell_width * V reaches 2^31
    bad = list(synth.SMPL_PARENTS)
    bad[5] = 7
    assert joints(parents=bad) == -3                                 # parents[j] >= j
    bad = list(synth.SMPL_PARENTS)
    bad[0] = 0
    assert joints(parents=bad) == -3
    assert lib.cape_smpl_unpose_joints(p[0], 3 * V, p[1], p[2], p[3], p[4], p[5], 4, p[6], None, 0, p[8], None, None, 24, V, 4, p[9],
                                       1 << 30, p[10], p[11], None, None, None, None) == -1       # NULL parent table

    def skin(J=24, K=217, posed=p[0], stride=3 * V, out=p[10], ostride=3 * V, W=4, N=4, G=p[3], Vn=V, coef=p[2]):
        return lib.cape_smpl_unpose_skin(posed, stride, p[1], K, coef, G, p[4], p[5], W, None, J, Vn, N, out, ostride, None, None)

    assert skin(J=65) == -1
    assert skin(posed=None) == -1
    assert skin(out=None) == -1
    assert skin(G=None) == -1
    assert skin(coef=None) == -1
    assert skin(W=0) == -1
    assert skin(N=0) == -1
    assert skin(stride=3 * V - 1) == -1
    assert skin(stride=0) == -1                                      # no broadcast of the posed input
    assert skin(ostride=3 * V - 1) == -1
    assert skin(Vn=1 << 22, stride=3 << 22, ostride=3 << 22) == -1   # 3 K V reaches 2^31

    def undress(T=p[0], mean=p[1], std=p[2], minimal=p[4], d=p[5], N=2, ts=3 * V, ds=3 * V, Vn=V):
        return lib.cape_smpl_undress(T, ts, mean, std, None, minimal, d, ds, N, Vn, None)

    assert undress(T=None) == -1
    assert undress(mean=None) == -1
    assert undress(std=None) == -1
    assert undress(minimal=None) == -1
    assert undress(d=None) == -1
    assert undress(N=0) == -1
    assert undress(N=65536) == -1
    assert undress(ts=3 * V - 1) == -1
    assert undress(ds=3 * V - 1) == -1
    assert undress(Vn=0) == -1
