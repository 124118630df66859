"""loss_mask on the host (reference lib/models.py:47-52): how the constructor resolves the option, and the argument checks
of the weighted loss entry point (cape_masked_recon_edge_loss_fwd_bwd), none of which need a device."""
import ctypes
import os
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
V = 6890


@pytest.fixture(scope="module")
def make_model(mesh_ops):
    from cape_amd.configs import cape_params
    from cape_amd.models import CAPE
    m = mesh_ops

    def make(**kw):
        return CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], **dict(cape_params(p=m["p"], batch_size=2), **kw))
    return make


def _project(tmp_path, sub):
    d = tmp_path.joinpath(*sub)
    d.mkdir(parents=True)
    shutil.copyfile(os.path.join(GOLDEN, "loss_mask_binary.npy"), str(d / "loss_mask_binary.npy"))
    return str(tmp_path)


def test_binary_mask_builds_the_documented_weights(tmp_path, make_model):
    model = make_model(loss_mask='binary', project_dir=_project(tmp_path, ("data",)))
    w = model.loss_mask
    assert isinstance(w, np.ndarray) and w.shape == (2, V, 3) and w.dtype == np.float32
    assert np.array_equal(w[0], w[1])
    clothing = np.load(os.path.join(GOLDEN, "clothing_verts_idx.npy"))
    assert (w[:, clothing, :] == 1.0).all()
    assert set(np.unique(w).tolist()) == {np.float32(0.1), np.float32(1.0)}
    assert (w[:, :, 0] == w[:, :, 1]).all() and (w[:, :, 0] == w[:, :, 2]).all()
    assert np.allclose(w.astype(np.float64).sum(1), 4671.5, rtol=1e-6, atol=0)       # per sample and coordinate
    assert int((w[0, :, 0] == 1.0).sum()) == 4425


def test_binary_mask_falls_back_to_lib_data_and_names_both_paths(tmp_path, make_model):
    model = make_model(loss_mask='binary', project_dir=_project(tmp_path / "a", ("lib", "data")))
    assert model.loss_mask.shape == (2, V, 3)
    empty = tmp_path / "b"
    empty.mkdir()
    with pytest.raises(FileNotFoundError) as e:
        make_model(loss_mask='binary', project_dir=str(empty))
    msg = str(e.value)
    assert os.path.join(str(empty), "data", "loss_mask_binary.npy") in msg
    assert os.path.join(str(empty), "lib", "data", "loss_mask_binary.npy") in msg


@pytest.mark.parametrize("shape", [(V,), (V, 1), (V, 3)])
def test_custom_mask_shapes(shape, make_model):
    rng = np.random.default_rng(0)
    w = rng.uniform(0.0, 2.0, shape)
    w[:100] = 0.0                                                   # zeros are allowed
    model = make_model(loss_mask=w)
    full = np.broadcast_to(w.reshape(V, -1), (V, 3)).astype(np.float32)
    assert model.loss_mask.shape == (2, V, 3) and np.array_equal(model.loss_mask[1], full)
    assert np.isclose(model._loss_mask_sum, full.astype(np.float64).sum())


@pytest.mark.parametrize("bad", ["wrong_v", "nan", "inf", "negative", "all_zero", "wrong_cols"])
def test_custom_mask_rejects_bad_weights(bad, make_model):
    w = np.ones((V, 3))
    if bad == "wrong_v":
        w = np.ones(V - 1)
    elif bad == "nan":
        w[5, 1] = np.nan
    elif bad == "inf":
        w[7, 0] = np.inf
    elif bad == "negative":
        w[3, 2] = -0.5
    elif bad == "all_zero":
        w[:] = 0.0
    else:
        w = np.ones((V, 2))
    with pytest.raises(ValueError):
        make_model(loss_mask=w)


@pytest.mark.parametrize("value", [None, '', 'none', 'Binary'])
def test_other_values_keep_the_unmasked_loss(tmp_path, value, make_model):
    model = make_model(loss_mask=value, project_dir=_project(tmp_path, ("data",)))
    assert model.loss_mask == 1.0 and model._loss_mask_w is None
    assert not hasattr(model, '_loss_mask_sum') and not hasattr(model, '_loss_mask_t')


def test_masked_entry_rejects_bad_arguments_before_launching():
    from cape_amd._lib import lib
    P = ctypes.c_void_p
    N, M, E = 2, 6890, 20664
    need = int(lib.cape_masked_recon_edge_workspace_bytes(N, M, E))
    assert need == int(lib.cape_recon_edge_workspace_bytes(N, M, E))
    assert lib.cape_masked_recon_edge_workspace_bytes(0, M, E) == -1

    def call(**kw):
        a = dict(pred=P(0x100000), ldp=4, gt=P(0x200000), ref=P(0x300000), edges=P(0x400000), vptr=P(0x500000),
                 vidx=P(0x600000), weights=P(0x700000), kind=0, inv=1.0 / (N * 3 * 4671.5), out=P(0x800000),
                 dpred=P(0x900000), ldd=4, ws=P(0xa00000), need=need)
        a.update(kw)
        return lib.cape_masked_recon_edge_loss_fwd_bwd(a["pred"], a["ldp"], a["gt"], a["ref"], a["edges"], a["vptr"], a["vidx"],
                                                       N, M, E, a["weights"], a["kind"], a["inv"], 1.0, 1.0, a["out"], None,
                                                       None, 0.0, None, a["dpred"], a["ldd"], a["ws"], a["need"], None)

    assert call(weights=None) == -1
    assert call(kind=3) == -1 and call(kind=-1) == -1
    assert call(ldp=2) == -1
    assert call(ldd=2) == -1
    assert call(vptr=None) == -1
    assert call(pred=None) == -1 and call(out=None) == -1
    assert call(inv=0.0) == -1 and call(inv=float("inf")) == -1 and call(inv=float("nan")) == -1
    assert call(need=need - 4) == -4                                # workspace too small
