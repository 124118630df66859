"""TEST INFRASTRUCTURE: the face-normal loss as torch operations, dtype-generic (float64 = the reference the device is judged
against, float32 = the restatement whose own error sets the bar, tests/parity_bar.py).  The definition, in the reference's op
order (lib/losses.py:27-52 on lib/utils.py:119-135 TriNormalsScaled / NormalizedNx3), over ALL samples and faces:

    x = pred + verts_ref, y = gt + verts_ref
    m(x) = (x[i1] - x[i0]) x (x[i2] - x[i0]);  n(x) = m / sqrt(ss + [ss == 0]), ss = m.m;  c = n(x).n(y)
    normal = mean(1 - |c|)

torch's abs has gradient sign(c) with sign(0) = 0, and a degenerate face has n = 0 and a zero gradient through the guard,
so autograd of this function is the gradient of DESIGN 7d without a special case."""
import numpy as np
import torch


def face_cosines(pred, gt, verts_ref, faces):
    """c [N, F] for pred, gt [N, V, 3], verts_ref [V, 3] (tensors of one dtype) and faces [F, 3] (integers; an array, or a
    tensor on the inputs' device)."""
    f = faces.long() if torch.is_tensor(faces) else torch.as_tensor(np.asarray(faces), dtype=torch.long)

    def unit_normals(x):
        x0, x1, x2 = x[:, f[:, 0]], x[:, f[:, 1]], x[:, f[:, 2]]
        m = torch.cross(x1 - x0, x2 - x0, dim=-1)
        ss = (m * m).sum(-1, keepdim=True)
        return m / torch.sqrt(ss + (ss == 0).to(m.dtype))

    return (unit_normals(pred + verts_ref) * unit_normals(gt + verts_ref)).sum(-1)


def normal_loss(pred, gt, verts_ref, faces):
    return (1 - face_cosines(pred, gt, verts_ref, faces).abs()).mean()


def evaluate(pred, gt, verts_ref, faces, dtype):
    """(value, d value / d pred [N, V, 3], c [N, F]) as numpy float64, computed in ``dtype`` from numpy inputs."""
    p = torch.tensor(np.asarray(pred), dtype=dtype, requires_grad=True)
    g = torch.tensor(np.asarray(gt), dtype=dtype)
    r = torch.tensor(np.asarray(verts_ref), dtype=dtype)
    c = face_cosines(p, g, r, faces)
    val = (1 - c.abs()).mean()
    val.backward()
    return float(val.detach()), p.grad.double().numpy(), c.detach().double().numpy()
