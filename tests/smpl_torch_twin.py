"""tests/smpl_reference.forward restated in torch, parametrised by dtype, so that torch autograd gives the gradients of SMPL
posing independently of the hand-derived backward kernels: float64 is the oracle, float32 the restatement whose error sets
tests/parity_bar.py's bar.  Same op order as the numpy reference; Rodrigues uses its ``where(small, 1, t2)`` guard, so the
branch that is not taken cannot put a NaN into the gradient.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import smpl_reference as ref


def rodrigues(r):
    """[..., 3] axis-angle -> [..., 3, 3]; exactly I at 0 (series below |r|^2 = 1e-6)."""
    dt = r.dtype
    t2 = (r * r).sum(-1)
    small = t2 < 1e-6
    t = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
    s = torch.where(small, 1 - t2 / 6, torch.sin(t) / t)
    h = torch.sin(0.5 * t) / t
    c = torch.where(small, 0.5 - t2 / 24, 2 * h * h)
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(r.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=dt, device=r.device)
    K2 = r[..., :, None] * r[..., None, :] - t2[..., None, None] * eye
    return eye + s[..., None, None] * K + c[..., None, None] * K2


class Twin(object):
    """The model's arrays as CPU (or ``device``) tensors of ``dtype``; ``forward`` takes and returns tensors."""

    def __init__(self, model, dtype=torch.float64, device="cpu"):
        f = lambda a: torch.tensor(np.asarray(a.toarray() if hasattr(a, "toarray") else a, dtype=np.float64), dtype=dtype,
                                   device=device)
        self.dtype, self.device = dtype, device
        self.parents = [int(p) for p in ref.parents_of(model)]
        self.J = len(self.parents)
        self.jreg, self.W, self.posedirs, self.shapedirs = (f(model[k]) for k in ("J_regressor", "weights", "posedirs", "shapedirs"))

    def tensor(self, a, requires_grad=False):
        """An input as this twin sees it: the float32 value every path gets, in the twin's dtype."""
        if a is None:
            return None
        t = torch.tensor(np.asarray(a, dtype=np.float32), dtype=self.dtype, device=self.device)
        return t.requires_grad_(requires_grad)

    def forward(self, T, pose, betas=None, transl=None):
        """T [N or 1, V, 3], pose [N, 3J], betas [N, B] or None, transl [N, 3] or None -> vertices [N,V,3], joints [N,J,3]."""
        N, J = pose.shape[0], self.J
        T = T.expand(N, -1, -1)
        v_shaped = T
        if betas is not None:
            v_shaped = T + torch.einsum("vck,nk->nvc", self.shapedirs[:, :, :betas.shape[1]], betas)
        Jn = torch.einsum("jv,nvc->njc", self.jreg, v_shaped)
        R = rodrigues(pose.reshape(N, J, 3))
        pf = (R[:, 1:] - torch.eye(3, dtype=self.dtype, device=self.device)).reshape(N, -1)
        v_posed = v_shaped + torch.einsum("vck,nk->nvc", self.posedirs, pf)
        rot, t = [R[:, 0]], [Jn[:, 0]]
        for j in range(1, J):
            p = self.parents[j]
            rot.append(rot[p] @ R[:, j])
            t.append((rot[p] @ (Jn[:, j] - Jn[:, p])[..., None])[..., 0] + t[p])
        Ar, At = torch.stack(rot, 1), torch.stack(t, 1)                   # [N,J,3,3], [N,J,3]
        Gt = At - (Ar @ Jn[..., None])[..., 0]
        G = torch.cat([Ar, Gt[..., None]], -1)                            # [N,J,3,4]
        M = torch.einsum("vj,njab->nvab", self.W, G)
        verts = (M[..., :3] @ v_posed[..., None])[..., 0] + M[..., 3]
        joints = At
        if transl is not None:
            verts = verts + transl[:, None]
            joints = joints + transl[:, None]
        return verts, joints

    def dress(self, disp, mean, std, clothing_idx, minimal):
        """smpl_reference.dress's formula on a tensor ``disp``; the other arguments host arrays."""
        c = lambda a: torch.tensor(np.asarray(a, dtype=np.float64).reshape(-1, 3), dtype=self.dtype, device=self.device)
        mask = torch.zeros(disp.shape[1], dtype=self.dtype, device=self.device)
        mask[torch.as_tensor(np.asarray(clothing_idx, dtype=np.int64), device=self.device)] = 1
        return (disp * c(std) + c(mean)) * mask[None, :, None] + c(minimal)


def gradients(model, dtype, T, pose, betas, transl, gV, gJ, device="cpu"):
    """d/d(inputs) of (vertices . gV).sum() + (joints . gJ).sum() by autograd on the twin of ``dtype``: a dict of float64 numpy
    arrays for the inputs given (gV / gJ None: that term is absent)."""
    tw = Twin(model, dtype, device)
    ins = dict(T=tw.tensor(T, True), pose=tw.tensor(pose, True), betas=tw.tensor(betas, True), transl=tw.tensor(transl, True))
    v, j = tw.forward(ins["T"], ins["pose"], ins["betas"], ins["transl"])
    loss = 0
    if gV is not None:
        loss = loss + (v * tw.tensor(gV)).sum()
    if gJ is not None:
        loss = loss + (j * tw.tensor(gJ)).sum()
    loss.backward()
    return {k: t.grad.detach().cpu().double().numpy() for k, t in ins.items() if t is not None and t.grad is not None}
