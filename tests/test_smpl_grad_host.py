"""CPU-only checks of the differentiable SMPL posing (cape_amd.smpl.forward_diff / dress_diff): the torch twin that the GPU
tests take their gradients from (tests/smpl_torch_twin.py) against the numpy oracle and torch's gradcheck, the argument
checks of the backward entry points, and the transposed joint-regressor table built at model load."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smpl_reference as ref     # noqa: E402
import smpl_synth as synth       # noqa: E402
import smpl_torch_twin as twin   # noqa: E402


def _inputs(m, N, seed, B=10):
    rng = np.random.default_rng(seed)
    J = len(ref.parents_of(m))
    V = m["v_template"].shape[0]
    T = m["v_template"][None] + 0.01 * rng.standard_normal((N, V, 3))
    pose = 0.5 * rng.standard_normal((N, 3 * J))
    pose[0] = 0.0                                   # an exactly-zero pose row
    if N > 1:
        pose[1, 3:6] = [4e-4 / np.sqrt(3)] * 3      # |r| = 4e-4: below the series threshold |r|^2 = 1e-6
        pose[1, 6:9] = [0.0, 1.001e-3, 0.0]         # just above it
    return T, pose, rng.standard_normal((N, B)), rng.standard_normal((N, 3))


def test_twin_forward_equals_the_numpy_reference_in_float64():
    for m in (synth.small(), synth.smpl_like()):
        T, pose, betas, transl = _inputs(m, 3, 1)
        tw = twin.Twin(m, torch.float64)
        for b, t, shared in ((betas, transl, False), (None, None, True), (betas[:, :4], None, False)):
            Tn = T[:1] if shared else T
            v, j = tw.forward(tw.tensor(Tn), tw.tensor(pose), tw.tensor(b), tw.tensor(t))
            f32 = lambda a: None if a is None else np.asarray(a, np.float32)
            v64, j64 = ref.forward(m, f32(Tn), f32(pose), f32(b), f32(t))
            assert np.abs(v.numpy() - v64).max() <= 1e-12 and np.abs(j.numpy() - j64).max() <= 1e-12


def test_twin_passes_gradcheck_with_zero_and_below_threshold_rotations():
    m = synth.small()
    T, pose, betas, transl = _inputs(m, 2, 2)
    tw = twin.Twin(m, torch.float64)
    d = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    ins = (d(T), d(pose), d(betas), d(transl))
    assert float((pose[0] ** 2).sum()) == 0.0 and 0 < float((pose[1, 3:6] ** 2).sum()) < 1e-6
    assert torch.autograd.gradcheck(lambda *a: tw.forward(*a), ins, eps=1e-6, atol=1e-6, rtol=1e-5)
    g = twin.gradients(m, torch.float64, T, pose, betas, transl, np.ones((2, 37, 3)), np.ones((2, 5, 3)))
    assert all(np.isfinite(v).all() for v in g.values()) and set(g) == {"T", "pose", "betas", "transl"}


def test_backward_entry_points_reject_bad_arguments_before_launching():
    """NULL operands, J > 64, a tree that is not parent-ordered, short strides, a short workspace and extents beyond the
    32-bit element index return their CAPE_E* code without a launch."""
    from cape_amd._lib import lib
    P = C.c_void_p
    p = [P(0x100000 + 0x1000 * i) for i in range(16)]
    V, J, K, N = 6890, 24, 217, 4
    plan = (C.c_int32 * 3)()
    assert lib.cape_smpl_skin_bwd_plan(K, J, V, N, plan) == 0
    assert list(plan) == [16, 108, K + 12 * J + 3]              # one wave per workgroup below 256 workgroups
    assert lib.cape_smpl_skin_bwd_plan(K, J, V, 256, plan) == 0 and list(plan)[:2] == [16, 27]
    assert lib.cape_smpl_skin_bwd_plan(10 + 9 * 51, 52, V, 15, plan) == 0 and plan[0] == 14     # the LDS tile of the 52-joint model
    assert lib.cape_smpl_skin_bwd_plan(K, 65, V, N, plan) == -1
    assert lib.cape_smpl_skin_bwd_plan(K, J, V, N, None) == -1
    need = lib.cape_smpl_skin_bwd_workspace_bytes(K, J, V, N)
    assert need == 4 * N * 108 * (K + 12 * J + 3)
    assert lib.cape_smpl_skin_bwd_workspace_bytes(K, J, 0, N) == -1 and lib.cape_smpl_skin_bwd_workspace_bytes(K, 0, V, N) == -1

    def skin(T=p[0], gV=p[6], ws=p[8], wsb=need, J=J, Kk=K, W=4, N=N, Vv=V, gss=3 * V, q=p[7], qss=3 * V):
        return lib.cape_smpl_skin_bwd(T, 0, p[1], Kk, p[2], p[3], p[4], p[5], W, gV, gss, J, Vv, N, 1, q, qss, ws, wsb, None)

    assert skin(T=None) == -1 and skin(gV=None) == -1 and skin(ws=None) == -1
    assert skin(wsb=need - 4) == -1                              # workspace one float short
    assert skin(J=65) == -1 and skin(W=0) == -1 and skin(N=0) == -1
    assert skin(gss=3 * V - 1) == -1 and skin(qss=1) == -1
    big = 1 << 22                                                # 3 * K * V beyond the 32-bit element index
    assert skin(Vv=big, gss=3 * big, qss=3 * big, wsb=1 << 62) == -1

    def joints(J=J, parents=None, T=p[0], pose=p[4], betas=p[5], B=10, gJ=p[6], part=p[7], blocks=108, cv=1, dpose=p[8],
               dbetas=p[9], dtransl=p[10], dJn=p[11]):
        par = (C.c_int32 * max(J, 1))(*(parents if parents is not None else ([-1] + [0] * (J - 1))))
        return lib.cape_smpl_joints_bwd(T, 0, p[1], p[2], p[3], pose, betas, B, p[12], par, J, V, N, gJ, part, blocks, cv, dpose,
                                        dbetas, dtransl, dJn, None)

    assert joints(T=None) == -1 and joints(pose=None) == -1 and joints(betas=None) == -1
    assert joints(J=65) == -1 and joints(J=0) == -1
    bad = list(synth.SMPL_PARENTS)
    bad[5] = 7
    assert joints(parents=bad) == -3
    assert joints(gJ=None, part=None) == -1                       # no gradient at all
    assert joints(blocks=0) == -1
    assert joints(cv=0) == -1                                     # pose gradient from records without their gcoef words
    assert joints(dpose=None, dbetas=None, dtransl=None, dJn=None) == -1

    def jreg(q=p[0], cp=p[1], dJn=p[4], dT=p[5], J=J, N=N, shared=0, qss=3 * V, tss=3 * V):
        return lib.cape_smpl_jreg_bwd(q, qss, cp, p[2], p[3], dJn, J, V, N, shared, dT, tss, None)

    assert jreg(cp=None) == -1 and jreg(dJn=None) == -1 and jreg(dT=None) == -1
    assert jreg(J=65) == -1 and jreg(N=0) == -1 and jreg(qss=3) == -1 and jreg(tss=0) == -1
    assert lib.cape_smpl_dress_bwd(None, 3 * V, p[1], p[2], p[3], 3 * V, 2, V, None) == -1
    assert lib.cape_smpl_dress_bwd(p[0], 3 * V, p[1], p[2], None, 3 * V, 2, V, None) == -1
    assert lib.cape_smpl_dress_bwd(p[0], 3 * V - 1, p[1], p[2], p[3], 3 * V, 2, V, None) == -1
    assert lib.cape_smpl_weighted_l2(None, 3 * V, p[1], 3 * V, p[2], 1.0, 2, V, p[3], p[4], 3 * V, None) == -1
    assert lib.cape_smpl_weighted_l2(p[0], 3 * V, p[1], 3 * V, p[2], 1.0, 2, V, None, p[4], 3 * V, None) == -1
    assert lib.cape_smpl_weighted_l2(p[0], 3 * V, p[1], 3, p[2], 1.0, 2, V, p[3], p[4], 3 * V, None) == -1


def test_transposed_regressor_table_reproduces_the_transpose():
    from cape_amd import smpl
    for m in (synth.small(), synth.smpl_like(), synth.j52()):
        x = smpl.SMPL(m)
        cp, ri, va = (x.layouts[k][0] for k in ("jt_colptr", "jt_rowidx", "jt_vals"))
        assert len(cp) == x.V + 1 and cp[0] == 0 and cp[-1] == len(ri) == len(va)
        dense = np.zeros((x.V, x.J))
        for v in range(x.V):
            r = ri[cp[v]:cp[v + 1]]
            assert np.all(np.diff(r) > 0) and np.all((0 <= r) & (r < x.J))
            dense[v, r] = va[cp[v]:cp[v + 1]]
        assert np.array_equal(dense, m["J_regressor"].toarray().T)
