"""CAPE's inference drivers share one padded-batch loop (cape_amd/models.py: _batches / _padded, _decoded, _generated): what
that sharing promises, on the small model at batch 4 with sizes 5 and 9 -- one and two full batches followed by a batch of
one row.  The decoder treats samples independently, so one condition row and the same row repeated per sample decode to the
same bits; decode_posed dresses decode's output; predict and test_errors run the same pass under the same seed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_reference as R       # noqa: E402
import parity_bar                # noqa: E402
import smpl_synth as synth       # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
SIZES = [5, 9]


@pytest.fixture(scope="module")
def setup(mesh_ops):
    from cape_amd import smpl
    from test_gpu_smpl import _cape_model
    model = _cape_model(mesh_ops, batch_size=4)
    st = np.load(os.path.join(GOLD, "trainset_stats.npz"))
    idx = np.load(os.path.join(GOLD, "clothing_verts_idx.npy"))
    return dict(model=model, body=smpl.SMPL(synth.smpl_like(seed=6)), mean=st["mean"], std=st["std"], idx=idx,
                poses=np.load(os.path.join(GOLD, "demo_pose_params.npz"))["pose"])


def _codes(model, size):
    rng = np.random.default_rng(40 + size)
    z = rng.standard_normal((size, model.nz + model.nz_cond + model.nz_cond2))
    return z, rng.standard_normal((size, model.nz_cond)), rng.standard_normal((size, model.nz_cond2)), rng


@pytest.mark.parametrize("size", SIZES)
def test_one_condition_row_decodes_like_the_row_repeated(setup, size):
    model = setup["model"]
    z, cond, cond2, _ = _codes(model, size)
    one = model.decode(z, cond[:1], cond2[:1])
    per_sample = model.decode(z, np.repeat(cond[:1], size, 0), np.repeat(cond2[:1], size, 0))
    assert one.shape == (size, 6890, 3) and one.dtype == np.float32 and np.isfinite(one).all()
    assert np.array_equal(one, per_sample)


@pytest.mark.parametrize("size", SIZES)
def test_decode_posed_dresses_what_decode_returns(setup, size):
    from cape_amd import smpl
    s = setup
    model = s["model"]
    z, cond, cond2, rng = _codes(model, size)
    pose = s["poses"][rng.integers(0, 6, size)]
    posed, clothed = model.decode_posed(z, cond, cond2, pose, s["body"], s["mean"], s["std"], s["idx"])
    x = torch.tensor(model.decode(z, cond, cond2), device="cuda")
    want = smpl.dress(x, s["mean"], s["std"], s["idx"], model.verts_ref).cpu().numpy()
    assert clothed.shape == (size, 6890, 3) and posed.shape == clothed.shape
    assert np.array_equal(clothed, want)


@pytest.mark.parametrize("size", SIZES)
def test_predict_and_test_errors_run_the_same_pass(setup, size):
    import test_gpu_model as T
    s = setup
    model = s["model"]
    x, gt, _, cond, _, clo, _, _ = T._inputs(size, model.nz, seed=4)
    torch.manual_seed(7)
    preds, lr_, ll_, le_ = model.predict(x, cond, clo, gt)
    torch.manual_seed(7)
    res = model.test_errors(x, cond, clo, gt, std=s["std"], clothing_idx=s["idx"], return_distances=True)
    assert preds.shape == (size, 6890, 3) and np.isfinite([lr_, ll_, le_]).all()
    assert (res["recon"], res["latent"], res["edge"]) == (lr_, ll_, le_)
    # the distances against float64 on predict's predictions, under test_gpu_eval_errors.py's bar for this comparison
    d = res["distances"]
    assert d.shape == (size, len(s["idx"])) and d.dtype == np.float32
    gt32, std32 = gt.astype(np.float32), s["std"].astype(np.float32)          # what the device holds
    d64 = R.distances(preds, gt32, std32, s["idx"], np.float64)
    assert d64.min() >= 1e-6
    err_f32 = R.rel_err(R.distances(preds, gt32, std32, s["idx"], np.float32), d64)
    err_hip = R.rel_err(d, d64)
    print("drivers size %d distances: max rel err hip %.3e, fp32 restatement %.3e" % (size, err_hip, err_f32))
    parity_bar.check("test_predict_and_test_errors_run_the_same_pass[%d]" % size, "distance", err_hip, err_f32)
