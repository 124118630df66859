"""CPU references for the scan-to-mesh distance (cape_amd/scan_distance.py).  TEST INFRASTRUCTURE ONLY.

  brute_force(x, faces, p, dtype)    the closest point over ALL faces with cape_amd.mesh_operators._closest_on_triangles evaluated
                                     in ``dtype``: float64 is the reference, float32 the restatement whose error sets the bar
  on_face(x, faces, p, face)         float64 (part, bary, foot, d2) of GIVEN faces (torch: ``rule`` is differentiable)
  gradients(x, faces, p, face, g)    the float64 gradient formulas of d2 for given faces and seed g
  octahedron(levels) / append_face   a small closed mesh and degenerate faces for it
  template_case(seed, shift, M)      the template recipe of the GPU tests
"""
import os

import numpy as np
import torch

from cape_amd.mesh_operators import _closest_on_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(x, faces, p, dtype=np.float64, chunk=None):
    """(face [M] int64, foot [M, 3], d2 [M]) of points p [M, 3] on the mesh x [V, 3]: every (point, face) pair through
    _closest_on_triangles in ``dtype``; the lowest face among equal distances; -1 / NaN where no face evaluates finite."""
    x, p = np.asarray(x, dtype=dtype), np.asarray(p, dtype=dtype)
    faces = np.asarray(faces, dtype=np.int64)
    F, M = len(faces), len(p)
    tri = x[faces]
    chunk = chunk or max(1, (1 << 20) // F)
    face, foot, d2 = np.full(M, -1, np.int64), np.full((M, 3), np.nan, dtype), np.full(M, np.nan, dtype)
    with np.errstate(all="ignore"):
        for i0 in range(0, M, chunk):
            q = p[i0:i0 + chunk]
            m = len(q)
            rep = lambda k: np.broadcast_to(tri[None, :, k], (m, F, 3)).reshape(-1, 3)
            _, ft, dist = _closest_on_triangles(rep(0), rep(1), rep(2), np.repeat(q, F, axis=0))
            dist = dist.reshape(m, F)
            best = np.argmin(dist, 1)
            ok = np.isfinite(dist[np.arange(m), best])
            face[i0:i0 + m] = np.where(ok, best, -1)
            foot[i0:i0 + m][ok] = ft.reshape(m, F, 3)[np.arange(m), best][ok]
            d2[i0:i0 + m][ok] = dist[np.arange(m), best][ok]
    return face, foot, d2


def rule(a, b, c, p, part=None):
    """The seven-region rule on torch tensors [n, 3], row by row: (part, bary [n, 3], foot, d2).  ``part`` given: that region's
    expression whatever the tests say (the selection held constant, for autograd)."""
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    dot = lambda u, v: (u * v).sum(-1)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    denom = va + vb + vc
    t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
    vw = {0: (vb / denom, vc / denom), 1: (t_ab, zero), 2: (1 - t_bc, t_bc), 3: (zero, t_ac), 4: (zero, zero), 5: (one, zero),
          6: (zero, one)}
    if part is None:
        conds = [((d1 <= 0) & (d2 <= 0), 4), ((d3 >= 0) & (d4 <= d3), 5), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1),
                 ((d6 >= 0) & (d5 <= d6), 6), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 3),
                 ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), 2)]
        part = torch.zeros(d1.shape, dtype=torch.int64)
        for cond, code in reversed(conds):                                   # the first that holds wins
            part = torch.where(cond, torch.full_like(part, code), part)
    v, w = zero, zero
    for code, (vv, ww) in vw.items():
        v, w = torch.where(part == code, vv, v), torch.where(part == code, ww, w)
    bary = torch.stack((1 - v - w, v, w), -1)
    foot = bary[:, 0:1] * a + bary[:, 1:2] * b + bary[:, 2:3] * c
    return part, bary, foot, ((p - foot) ** 2).sum(-1)


def on_face(x, faces, p, face, dtype=np.float64):
    """numpy (part, bary, foot, d2) of points p [M, 3] on the GIVEN faces ``face`` [M] of the mesh x [V, 3], in ``dtype``."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=dtype))
    tri = np.asarray(x, dtype=dtype)[np.asarray(faces, dtype=np.int64)[np.asarray(face, dtype=np.int64)]]
    return tuple(r.numpy() for r in rule(t(tri[:, 0]), t(tri[:, 1]), t(tri[:, 2]), t(p)))


def gradients(x, faces, p, face, g, dtype=np.float64):
    """(dx [V, 3], dp [M, 3]) of sum_i g_i d2_i with the faces held, in ``dtype``: dx[corner k] += -2 g b_k (p - foot),
    dp = 2 g (p - foot).  Points with face < 0 add nothing."""
    x, p, g = np.asarray(x, dtype), np.asarray(p, dtype), np.asarray(g, dtype)
    faces, face = np.asarray(faces, np.int64), np.asarray(face, np.int64)
    dx, dp = np.zeros_like(x), np.zeros_like(p)
    ok = face >= 0
    _, bary, foot, _ = on_face(x, faces, p[ok], face[ok], dtype)
    r = p[ok] - foot
    two = dtype(2.0)
    dp[ok] = two * g[ok, None] * r
    for k in range(3):
        np.add.at(dx, faces[face[ok], k], -two * (g[ok] * bary[:, k])[:, None] * r)
    return dx, dp


def octahedron(levels=2, radius=0.5):
    """(x [V, 3] float64, faces [F, 3]) of an octahedron subdivided ``levels`` times onto a sphere: closed, symmetric in the
    three coordinate planes; levels = 2: V = 66, F = 128."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(q, dtype=np.float64) for q in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                q = v[i] + v[j]
                v.append(q / np.linalg.norm(q))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    return radius * np.array(v), np.array(f, dtype=np.int64)


def append_face(x, faces, kind, at=None, where=None):
    """(x', faces') with one more face on three NEW vertices, inserted at row ``at`` of faces (default: appended).  kind "nan":
    the corners have no finite coordinate, the face evaluates to nothing finite and must never win; "collapsed": the three
    corners are the one position ``where``, which the rule evaluates as that point (region vertex a)."""
    x = np.asarray(x)
    V = x.shape[0]
    new = np.full((3, 3), np.nan) if kind == "nan" else np.tile(np.asarray(where, dtype=np.float64), (3, 1))
    row = np.array([[V, V + 1, V + 2]], dtype=faces.dtype)
    at = len(faces) if at is None else at
    return np.concatenate([x, new.astype(x.dtype)]), np.concatenate([faces[:at], row, faces[at:]])


def template():
    from cape_amd.load_data import load_pack
    return (np.asarray(load_pack()["template_verts"], dtype=np.float64),
            np.load(os.path.join(ROOT, "tests", "golden", "template_faces.npy")).astype(np.int64))


def surface_samples(rng, x, faces, M):
    """(points [M, 3], unit face normals [M, 3]) float64: a random face, Dirichlet(1, 1, 1) barycentrics."""
    f = rng.integers(0, len(faces), M)
    b = rng.dirichlet((1.0, 1.0, 1.0), M)
    tri = x[faces[f]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return (b[:, :, None] * tri).sum(1), nrm


def template_case(seed, shift, M):
    """(x [V, 3] float32, faces, points [M, 3] float32): the template moved 5 mm along a random normal field and by ``shift``;
    points on random faces -0.01 .. 0.03 m along the face normal, an eighth of them replaced by uniform points in the bounding
    box inflated by 0.2 m, an eighth of the rest left exactly on the surface."""
    verts, faces = template()
    rng = np.random.default_rng(seed)
    x = (verts + 5e-3 * rng.standard_normal(verts.shape) + shift).astype(np.float32)
    x64 = x.astype(np.float64)
    p, nrm = surface_samples(rng, x64, faces, M)
    off = rng.uniform(-0.01, 0.03, M)
    far = rng.permutation(M)[:M // 8]
    rest = np.setdiff1d(np.arange(M), far)
    off[rng.permutation(rest)[:len(rest) // 8]] = 0.0
    p = p + off[:, None] * nrm
    lo, hi = x64.min(0) - 0.2, x64.max(0) + 0.2
    p[far] = rng.uniform(lo, hi, (len(far), 3))
    return x, faces, p.astype(np.float32)
