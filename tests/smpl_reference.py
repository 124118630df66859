"""The SMPL forward pass in numpy, parametrised by dtype: float64 is the oracle, float32 the restatement of the reference's
fp32 CPU path (smplx, demos.py:267-283) that tests/parity_bar.py uses as the yardstick.  Op order of the published
formulation: shape blend, joints from the shaped rest body, Rodrigues, pose feature, pose blend, kinematic chain, blended
transforms applied to [v; 1].  TEST INFRASTRUCTURE ONLY."""
import numpy as np


def rodrigues(r, dtype=np.float64):
    """[..., 3] axis-angle -> [..., 3, 3]; exactly I at 0 (series below |r|^2 = 1e-6)."""
    r = np.asarray(r, dtype=dtype)
    t2 = (r * r).sum(-1)
    small = t2 < 1e-6
    t = np.sqrt(np.where(small, 1, t2)).astype(dtype)
    s = np.where(small, 1 - t2 / 6, np.sin(t) / t).astype(dtype)
    h = np.sin(dtype(0.5) * t) / t
    c = np.where(small, dtype(0.5) - t2 / 24, 2 * h * h).astype(dtype)
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    zero = np.zeros_like(x)
    K = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(r.shape[:-1] + (3, 3))
    K2 = r[..., :, None] * r[..., None, :] - t2[..., None, None] * np.eye(3, dtype=dtype)
    return (np.eye(3, dtype=dtype) + s[..., None, None] * K + c[..., None, None] * K2).astype(dtype)


def parents_of(model):
    p = np.asarray(model["kintree_table"])[0].astype(np.int64)
    p[p == 4294967295] = -1
    return p


def forward(model, T, pose, betas=None, transl=None, dtype=np.float64, full=False):
    """T [N or 1, V, 3], pose [N, 3J], betas [N, B] or None, transl [N, 3] or None -> vertices [N,V,3], joints [N,J,3]."""
    f = lambda a: np.asarray(a.toarray() if hasattr(a, "toarray") else a, dtype=dtype)
    pose = f(pose)
    N = pose.shape[0]
    T = np.broadcast_to(f(T), (N,) + np.shape(T)[1:])
    parents = parents_of(model)
    J = len(parents)
    jreg, W, posedirs = f(model["J_regressor"]), f(model["weights"]), f(model["posedirs"])
    v_shaped = T
    if betas is not None:
        betas = f(betas)
        v_shaped = T + np.einsum("vck,nk->nvc", f(model["shapedirs"])[:, :, :betas.shape[1]], betas)
    Jn = np.einsum("jv,nvc->njc", jreg, v_shaped)
    R = rodrigues(pose.reshape(N, J, 3), dtype)
    pf = (R[:, 1:] - np.eye(3, dtype=dtype)).reshape(N, -1)
    v_posed = v_shaped + np.einsum("vck,nk->nvc", posedirs, pf)
    A = np.zeros((N, J, 3, 4), dtype)
    A[:, 0, :, :3], A[:, 0, :, 3] = R[:, 0], Jn[:, 0]
    for j in range(1, J):
        p = parents[j]
        A[:, j, :, :3] = A[:, p, :, :3] @ R[:, j]
        A[:, j, :, 3] = (A[:, p, :, :3] @ (Jn[:, j] - Jn[:, p])[..., None])[..., 0] + A[:, p, :, 3]
    G = A.copy()
    G[..., 3] = A[..., 3] - (A[..., :3] @ Jn[..., None])[..., 0]
    M = np.einsum("vj,njab->nvab", W, G)
    verts = (M[..., :3] @ v_posed[..., None])[..., 0] + M[..., 3]
    joints = A[..., 3].copy()
    if transl is not None:
        verts = verts + f(transl)[:, None]
        joints = joints + f(transl)[:, None]
    if full:
        return dict(vertices=verts, joints=joints, pf=pf, v_posed=v_posed, G=G, Jn=Jn)
    return verts, joints


def dress(disp, mean, std, clothing_idx, minimal, dtype=np.float64):
    """demos.py:155-161."""
    pred = np.asarray(disp, dtype) * np.asarray(std, dtype) + np.asarray(mean, dtype)
    masked = np.zeros_like(pred)
    masked[:, clothing_idx] = pred[:, clothing_idx]
    return masked + np.asarray(minimal, dtype)
