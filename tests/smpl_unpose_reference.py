"""The inverse of the SMPL forward pass of tests/smpl_reference.py in numpy, parametrised by dtype like that file: float64
is the oracle, float32 the restatement tests/parity_bar.py uses as the yardstick.  Given posed vertices P and the pose, the
rest body T with forward(T) = P.  The joints the forward regresses from the rest body are part of the unknown; for a fixed
pose the map is affine in T and the unknown enters through the 3J rest-joint coordinates only, so the exact inverse is one
dense 3J x 3J solve per sample (np.linalg.solve) and a 3x3 inverse per vertex (np.linalg.inv).  With ``joints_from`` the
joints come from that body instead and no system is solved.  Also ``forward`` with that option and the inverse of ``dress``.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import smpl_reference as ref


def _arrays(model, dtype):
    f = lambda a: np.asarray(a.toarray() if hasattr(a, "toarray") else a, dtype=dtype)
    return f, f(model["J_regressor"]), f(model["weights"]), f(model["posedirs"]), ref.parents_of(model)


def _world_rotations(R, parents, dtype):
    N, J = R.shape[:2]
    Wr = np.zeros((N, J, 3, 3), dtype)
    Wr[:, 0] = R[:, 0]
    for j in range(1, J):
        Wr[:, j] = Wr[:, parents[j]] @ R[:, j]
    return Wr


def _transforms(Wr, Jn, parents):
    """G [N,J,3,4] and the chain's translations A.t [N,J,3] for world rotations Wr and rest joints Jn."""
    N, J = Jn.shape[:2]
    At = np.zeros_like(Jn)
    At[:, 0] = Jn[:, 0]
    for j in range(1, J):
        p = parents[j]
        At[:, j] = (Wr[:, p] @ (Jn[:, j] - Jn[:, p])[..., None])[..., 0] + At[:, p]
    G = np.concatenate([Wr, (At - (Wr @ Jn[..., None])[..., 0])[..., None]], -1)
    return G, At


def translation_operator(Wr, parents):
    """L [N, 3J, 3J] with G_j.t = (L . Jn)_j, from the chain's definition: A_0.t = Jn_0,
    A_j.t = A_p.t + W_p (Jn_j - Jn_p), G_j.t = A_j.t - W_j Jn_j."""
    N, J = Wr.shape[:2]
    E = np.eye(3 * J, dtype=Wr.dtype).reshape(J, 3, 3 * J)
    At = np.zeros((N, J, 3, 3 * J), Wr.dtype)
    At[:, 0] = E[0]
    for j in range(1, J):
        p = parents[j]
        At[:, j] = At[:, p] + Wr[:, p] @ (E[j] - E[p])
    return (At - Wr @ E[None]).reshape(N, 3 * J, 3 * J)


def forward(model, T, pose, betas=None, transl=None, joints_from=None, dtype=np.float64):
    """smpl_reference.forward, with ``joints_from`` [N or 1, V, 3] the rest joints regressed from that body (plus the shape
    term) instead of from T: (vertices [N,V,3], joints [N,J,3])."""
    if joints_from is None:
        return ref.forward(model, T, pose, betas, transl, dtype=dtype)
    f, jreg, W, posedirs, parents = _arrays(model, dtype)
    pose = f(pose)
    N, J = pose.shape[0], len(parents)
    T = np.broadcast_to(f(T), (N,) + np.shape(T)[1:])
    JF = np.broadcast_to(f(joints_from), (N,) + np.shape(joints_from)[1:])
    shape = 0
    if betas is not None:
        shape = np.einsum("vck,nk->nvc", f(model["shapedirs"])[:, :, :np.shape(betas)[1]], f(betas))
    Jn = np.einsum("jv,nvc->njc", jreg, JF + shape)
    R = ref.rodrigues(pose.reshape(N, J, 3), dtype)
    pf = (R[:, 1:] - np.eye(3, dtype=dtype)).reshape(N, -1)
    v_posed = T + shape + np.einsum("vck,nk->nvc", posedirs, pf)
    G, At = _transforms(_world_rotations(R, parents, dtype), Jn, parents)
    M = np.einsum("vj,njab->nvab", W, G)
    verts = (M[..., :3] @ v_posed[..., None])[..., 0] + M[..., 3]
    if transl is not None:
        verts, At = verts + f(transl)[:, None], At + f(transl)[:, None]
    return verts, At


def unpose(model, P, pose, betas=None, transl=None, joints_from=None, dtype=np.float64, full=False):
    """P [N, V, 3] posed vertices, the other arguments as ``forward`` -> (rest vertices T [N,V,3], rest joints Jn [N,J,3]).
    ``full``: a dict with, besides, the posed joints, min_v |det Mrot_v| per sample, and (joints_from None) the condition
    numbers of I + QL and the largest one of Mrot_v per sample."""
    f, jreg, W, posedirs, parents = _arrays(model, dtype)
    pose, P = f(pose), f(P)
    N, J = pose.shape[0], len(parents)
    R = ref.rodrigues(pose.reshape(N, J, 3), dtype)
    pf = (R[:, 1:] - np.eye(3, dtype=dtype)).reshape(N, -1)
    Wr = _world_rotations(R, parents, dtype)
    acc = np.einsum("vck,nk->nvc", posedirs, pf)
    shape = 0
    if betas is not None:
        shape = np.einsum("vck,nk->nvc", f(model["shapedirs"])[:, :, :np.shape(betas)[1]], f(betas))
    X = P if transl is None else P - f(transl)[:, None]
    Mrot = np.einsum("vj,njab->nvab", W, Wr)
    Minv = np.linalg.inv(Mrot)
    out = {}
    if joints_from is None:
        # (I + Q L) Jn = c over the vertices the regressor touches
        cols = np.flatnonzero((jreg != 0).any(0))
        y = (Minv[:, cols] @ X[:, cols, :, None])[..., 0]
        c = np.einsum("jv,nvc->njc", jreg[:, cols], y) - np.einsum("jv,nvc->njc", jreg[:, cols], acc[:, cols])
        wm = (W[cols][None, :, :, None, None] * Minv[:, cols][:, :, None]).reshape(N, len(cols), 9 * J)
        Q = (jreg[:, cols] @ wm).reshape(N, J, J, 3, 3).transpose(0, 1, 3, 2, 4).reshape(N, 3 * J, 3 * J)
        A = np.eye(3 * J, dtype=dtype) + Q @ translation_operator(Wr, parents)
        Jn = np.linalg.solve(A, c.reshape(N, 3 * J, 1)).reshape(N, J, 3).astype(dtype)
        out["cond_system"] = np.linalg.cond(A.astype(np.float64))
    else:
        JF = np.broadcast_to(f(joints_from), (N,) + np.shape(joints_from)[1:])
        Jn = np.einsum("jv,nvc->njc", jreg, JF + shape)
    G, At = _transforms(Wr, Jn, parents)
    Mt = np.einsum("vj,njc->nvc", W, G[..., 3])
    T = (Minv @ (X - Mt)[..., None])[..., 0] - acc - shape
    if not full:
        return T, Jn
    sv = np.linalg.svd(Mrot.astype(np.float64), compute_uv=False)
    out.update(rest=T, rest_joints=Jn, joints=At if transl is None else At + f(transl)[:, None],
               det_min=np.abs(np.linalg.det(Mrot)).min(1), cond_mrot=(sv[..., 0] / sv[..., -1]).max(1))
    return out


def undress(T, mean, std, clothing_idx, minimal, dtype=np.float64):
    """The right-inverse of smpl_reference.dress (reference lib/prep_data.py:74 packs v_cano - minimal the same way):
    d = (mask (T - minimal) - mean) / std; ``clothing_idx`` None: every vertex."""
    d = np.asarray(T, dtype) - np.asarray(minimal, dtype)
    if clothing_idx is not None:
        masked = np.zeros_like(d)
        masked[:, clothing_idx] = d[:, clothing_idx]
        d = masked
    return (d - np.asarray(mean, dtype)) / np.asarray(std, dtype)
