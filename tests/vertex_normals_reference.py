"""TEST INFRASTRUCTURE: per-vertex normals as torch operations, dtype-generic (float64 = the reference the device is judged
against, float32 = the restatement whose own error sets the bar, tests/parity_bar.py).  The definition (the reference's
estimate_vertex_normals, lib/losses.py:54-80 on lib/utils.py:119-135 TriNormals / NormalizedNx3), per sample:

    m_f = (x[f1] - x[f0]) x (x[f2] - x[f0]);  u_f = m_f / sqrt(m_f.m_f + [m_f.m_f == 0])
    s_v = sum of u_f over the faces that use v (uniform weights);  n_v = s_v / sqrt(s_v.s_v + [s_v.s_v == 0])

Both guards are comparisons, constants to autograd, so autograd of this function is the gradient of DESIGN 7h without a
special case: a degenerate face has u = 0 and passes G_f on unscaled, a vertex with s = 0 passes gbar on unscaled."""
import numpy as np
import torch


def _guarded_unit(a):
    ss = (a * a).sum(-1, keepdim=True)
    return a / torch.sqrt(ss + (ss == 0).to(a.dtype))


def vertex_normals(x, faces):
    """(n [N, V, 3], s [N, V, 3], m [N, F, 3]) for x [N, V, 3] (a tensor) and faces [F, 3] (integers)."""
    f = faces.long() if torch.is_tensor(faces) else torch.as_tensor(np.asarray(faces), dtype=torch.long)
    x0, x1, x2 = x[:, f[:, 0]], x[:, f[:, 1]], x[:, f[:, 2]]
    m = torch.cross(x1 - x0, x2 - x0, dim=-1)
    u = _guarded_unit(m)
    s = torch.zeros_like(x)
    for k in range(3):                                       # corner by corner: index_add sums duplicates of one index
        s = s.index_add(1, f[:, k], u)
    return _guarded_unit(s), s, m


def evaluate(x, faces, gbar, dtype):
    """(n, d <n, gbar> / d x, |s_v| [N, V], |m_f| [N, F]) as numpy float64, computed in ``dtype`` from numpy inputs; the
    lengths are the true ones (0 where a guard acts)."""
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    g = torch.tensor(np.asarray(gbar), dtype=dtype)
    n, s, m = vertex_normals(xt, faces)
    (n * g).sum().backward()
    d = lambda t: t.detach().double().numpy()
    return d(n), d(xt.grad), d(torch.sqrt((s * s).sum(-1))), d(torch.sqrt((m * m).sum(-1)))
