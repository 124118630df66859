"""Seeded synthetic SMPL-format models (no real SMPL file is available to the suite): arrays with the key names, shapes and
sparsity of an SMPL file on the shipped 6890-vertex template (SMPL's 24-joint tree), plus a small generic model (J = 5,
V = 37) and a 52-joint one.  TEST INFRASTRUCTURE ONLY."""
import os
import pickle

import numpy as np
import scipy.sparse as sp

SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]


def template():
    from cape_amd.load_data import load_pack
    return np.asarray(load_pack()["template_verts"], dtype=np.float64)


def _faces(V, rng):
    return np.stack([np.arange(V), (np.arange(V) + 1) % V, (np.arange(V) + 2) % V], 1).astype(np.int64)


def make_model(parents=None, verts=None, num_betas=10, seed=0, J=None, V=None):
    """An SMPL-format dict: joints at seeded cluster centres of the vertices, a sparse row-normalised J_regressor over each
    centre's nearest vertices, at most 4 nonzero skinning weights per vertex, small random posedirs / shapedirs."""
    rng = np.random.default_rng(seed)
    if verts is None:
        verts = rng.standard_normal((V, 3)) * 0.3
    V = len(verts)
    if parents is None:
        parents = [-1] + [int(rng.integers(0, j)) for j in range(1, J)]
    J = len(parents)
    centres = verts[rng.choice(V, J, replace=False)]
    d2 = ((verts[:, None, :] - centres[None]) ** 2).sum(-1)          # [V, J]
    jreg = np.zeros((J, V))
    for j in range(J):
        near = np.argsort(d2[:, j])[:min(V, 20)]
        w = rng.uniform(0.2, 1.0, len(near))
        jreg[j, near] = w / w.sum()
    W = np.zeros((V, J))
    order = np.argsort(d2, 1)[:, :min(J, 4)]
    for v in range(V):
        k = int(rng.integers(1, order.shape[1] + 1))
        w = rng.uniform(0.1, 1.0, k)
        W[v, order[v, :k]] = w / w.sum()
    kin = np.zeros((2, J), np.uint32)
    kin[0] = np.array(parents, np.int64).astype(np.uint32)         # parents[0] = -1 -> 4294967295, as the files store it
    kin[1] = np.arange(J)
    return dict(v_template=verts, J_regressor=sp.csc_matrix(jreg), weights=W,
                posedirs=rng.standard_normal((V, 3, 9 * (J - 1))) * 2e-3,
                shapedirs=rng.standard_normal((V, 3, num_betas)) * 1e-2,
                kintree_table=kin, f=_faces(V, rng))


def smpl_like(seed=0):
    return make_model(SMPL_PARENTS, template(), seed=seed)


def small(seed=1):
    return make_model(J=5, V=37, seed=seed)


def j52(seed=2):
    return make_model(J=52, verts=template(), seed=seed)


def write_npz(d, path):
    a = dict(d)
    a["J_regressor"] = a["J_regressor"].toarray()
    np.savez(path, **a)
    return path


def write_pkl(d, path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fh:
        pickle.dump(d, fh, protocol=2)
    return path
