"""test_errors on the device (cape_amd/csrc/eval/vertex_error.hip): the distance pass against the float64
restatement of its definition (tests/eval_reference.py) under the parity bar, the statistics of buffers uploaded directly
(order statistics bit-equal to np.sort, moments against math.fsum), and CAPE.test_errors against predict + numpy."""
import math
import os

import numpy as np
import pytest
import torch

import eval_reference as R
import parity_bar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
V = 6890
U53 = 2.0 ** -53
QS = (0, 0.25, 0.5, 1)


def _fixtures():
    std = np.load(os.path.join(GOLDEN, "trainset_stats.npz"))["std"]
    idx = np.load(os.path.join(GOLDEN, "clothing_verts_idx.npy"))
    assert std.shape == (V, 3) and idx.shape == (3627,)
    return std, idx


def _dev(a, dt=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")


# ---- 1. distance parity --------------------------------------------------------------------------------------------------

def _case(name):
    rng = np.random.default_rng(31 if name == "synthetic" else 32)
    if name == "synthetic":
        nv, N = 70, 3
        idx = rng.permutation(nv)[:37]                                    # unsorted, unique
        std = rng.uniform(5e-4, 2.4e-2, (nv, 3))                          # the range of the shipped statistics
    else:
        nv, N = V, 2
        std, idx = _fixtures()
    std = std.astype(np.float32)
    pred = rng.standard_normal((N, nv, 3)).astype(np.float32)
    gt = (pred + 0.2 * rng.standard_normal((N, nv, 3))).astype(np.float32)
    return pred, gt, std, idx


@pytest.mark.parametrize("rows", ["dense", "rows4"])
@pytest.mark.parametrize("name", ["synthetic", "fixtures"])
def test_vertex_error_parity(name, rows):
    from cape_amd import ops
    pred, gt, std, idx = _case(name)
    N, nv, Vc = pred.shape[0], pred.shape[1], len(idx)
    d64 = R.distances(pred, gt, std, idx, np.float64)
    d32 = R.distances(pred, gt, std, idx, np.float32)
    assert d64.min() >= 1e-6                                              # input condition, on the CPU references alone
    err_f32 = R.rel_err(d32, d64)
    if rows == "dense":
        hp = _dev(pred)
    else:                                                                 # the decoder's 16-byte rows, padding never read
        buf = torch.full((N, nv, 4), 1e9, dtype=torch.float32, device="cuda:0")
        buf[:, :, :3] = _dev(pred)
        hp = buf[:, :, :3]
    S, row0, sentinel = N + 3, 2, -7.0
    dist = torch.full((S, Vc), sentinel, dtype=torch.float32, device="cuda:0")
    hstd, hidx = _dev(std), _dev(idx, torch.int32)
    ops.vertex_error(hp, _dev(gt), hstd, hidx, dist, row0=row0)
    torch.cuda.synchronize()
    out = dist.cpu().numpy()
    err_hip = R.rel_err(out[row0:row0 + N], d64)
    print("vertex_error %s/%s: max rel err hip %.3e (%.2f x 2^-24), fp32 restatement %.3e (%.2f x 2^-24)"
          % (name, rows, err_hip, err_hip * 2 ** 24, err_f32, err_f32 * 2 ** 24))
    parity_bar.check("test_vertex_error_parity[%s-%s]" % (name, rows), "distance", err_hip, err_f32)
    outside = np.r_[out[:row0].reshape(-1), out[row0 + N:].reshape(-1)]
    assert outside.size == 3 * Vc and (outside.view(np.uint32) == np.float32(sentinel).view(np.uint32)).all()
    # a sample whose prediction equals its ground truth: +0 everywhere, as a bit pattern
    ops.vertex_error(hp[:1], _dev(pred[:1]), hstd, hidx, dist, row0=S - 1)
    torch.cuda.synchronize()
    out2 = dist.cpu().numpy()
    assert (out2[S - 1].view(np.uint32) == 0).all()
    assert np.array_equal(out2[:S - 1].view(np.uint32), out[:S - 1].view(np.uint32))


def test_vertex_error_single_vertex_in_padded_rows():
    """V = 1 with several samples in 16-byte rows: a row stride says nothing there, the sample stride does."""
    from cape_amd import ops
    rng = np.random.default_rng(33)
    pred = rng.standard_normal((3, 1, 3)).astype(np.float32)
    gt = (pred + 0.2 * rng.standard_normal((3, 1, 3))).astype(np.float32)
    std = rng.uniform(5e-4, 2.4e-2, (1, 3)).astype(np.float32)
    buf = torch.full((3, 1, 4), 1e9, dtype=torch.float32, device="cuda:0")
    buf[:, :, :3] = _dev(pred)
    hstd, hidx = _dev(std), _dev(np.zeros(1), torch.int32)
    got = [ops.vertex_error(p, _dev(gt), hstd, hidx, torch.zeros((3, 1), dtype=torch.float32, device="cuda:0")).cpu().numpy()
           for p in (buf[:, :, :3], _dev(pred))]
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    d64 = R.distances(pred, gt, std, [0], np.float64)
    assert R.rel_err(got[0], d64) <= 4 * 2.0 ** -24


# ---- 2. statistics of buffers uploaded directly --------------------------------------------------------------------------

SHAPES = [(1, 1), (4, 37), (5, 37), (3, 3627), (64, 3627)]
CONTENTS = ["exp", "five", "equal", "zero", "ulps"]


def _buffer(shape, content):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + len(content))
    n = shape[0] * shape[1]
    if content == "exp":                                                  # every digit of the pattern varies
        b = np.exp(rng.uniform(-20, 5, n)).astype(np.float32)
    elif content == "five":                                               # heavy ties across the ranks
        b = np.exp(rng.uniform(-20, 5, 5)).astype(np.float32)[rng.integers(0, 5, n)]
    elif content == "equal":
        b = np.full(n, np.float32(0.0123456), dtype=np.float32)
    elif content == "zero":
        b = np.zeros(n, dtype=np.float32)
    else:                                                                 # base + k ulps: only the last digit pass tells them apart
        b = (np.float32(1.0).view(np.uint32) + rng.integers(0, 1000, n).astype(np.uint32)).view(np.float32)
    return np.ascontiguousarray(b.reshape(shape))


def _check_order(res, buf):
    srt = np.sort(buf.reshape(-1))
    want = srt[np.asarray(res["order_ranks"])]
    assert np.array_equal(res["order_values"].view(np.uint32), want.view(np.uint32)), (res["order_ranks"], res["order_values"], want)
    return srt


def _check_moments(res, buf):
    S, Vc = buf.shape
    n = S * Vc
    b64 = buf.astype(np.float64)
    near = lambda got, want, m: abs(got - want) <= m * U53 * abs(want)
    assert res["count"] == n and res["nonfinite"] == 0
    assert near(res["euclidean_mean"], R.fsum_mean(b64), n)
    pv = np.array([math.fsum(c) / S for c in b64.T.tolist()])
    ps = np.array([math.fsum(r) / Vc for r in b64.tolist()])
    assert res["per_vertex_mean"].shape == (Vc,) and res["per_sample_mean"].shape == (S,)
    assert (np.abs(res["per_vertex_mean"] - pv) <= S * U53 * np.abs(pv)).all()
    assert (np.abs(res["per_sample_mean"] - ps) <= Vc * U53 * np.abs(ps)).all()


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_error_statistics(shape, content):
    from cape_amd import ops
    buf = _buffer(shape, content)
    n = buf.size
    res = ops.error_statistics(_dev(buf), QS)
    assert sorted(set(r for q in QS for r in ops.quantile_ranks(n, q)[:2])) == res["order_ranks"]
    srt = _check_order(res, buf)
    _check_moments(res, buf)
    var = res["euclidean_var"]
    if content in ("equal", "zero"):
        assert var == 0.0 and res["euclidean_std"] == 0.0
    else:                                                                 # every random buffer, "ulps" included: the one content
        want = R.two_pass_var(buf)                                        # a one-pass E[x^2] - mean^2 would miss by 1e3 .. 1e6
        assert abs(var - want) <= 4 * n * U53 * want, (var, want)         # (want == 0 at 1x1: exactly 0)
        assert res["euclidean_std"] == math.sqrt(var)
    for q in QS:                                                          # the interpolation, from the exact order statistics
        lo, hi, frac = ops.quantile_ranks(n, q)
        assert res["quantiles"][float(q)] == float(srt[lo]) + (float(srt[hi]) - float(srt[lo])) * frac
    want_med = float(np.median(buf.astype(np.float64)))
    assert abs(res["euclidean_median"] - want_med) <= 4 * U53 * abs(want_med)


@pytest.mark.parametrize("shape", [(5, 37), (64, 3627)], ids=["5x37", "64x3627"])
def test_eight_ranks_and_an_unaligned_buffer(shape):
    """Four quantiles at fractional positions ask for eight distinct ranks (the most one call takes); the same buffer
    at an address that is no multiple of 16 bytes takes the scalar loads and must give the same bits."""
    from cape_amd import ops
    buf = _buffer(shape, "exp")
    qs = (0.1, 0.3, 0.6, 0.9)
    res = ops.error_statistics(_dev(buf), qs)
    assert len(res["order_ranks"]) == 8
    _check_order(res, buf)
    _check_moments(res, buf)
    flat = torch.empty(buf.size + 1, dtype=torch.float32, device="cuda:0")
    shifted = flat[1:].view(shape)
    shifted.copy_(_dev(buf))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    res2 = ops.error_statistics(shifted, qs)
    assert np.array_equal(res2["order_values"].view(np.uint32), res["order_values"].view(np.uint32))
    _check_moments(res2, buf)
    assert abs(res2["euclidean_var"] - res["euclidean_var"]) <= 8 * buf.size * U53 * res["euclidean_var"]


def test_nonfinite_values_are_counted():
    from cape_amd import ops
    buf = _buffer((4, 37), "exp")
    buf[1, 5], buf[3, 36] = np.nan, np.inf
    res = ops.error_statistics(_dev(buf), QS)
    assert res["nonfinite"] == 2 and res["count"] == 4 * 37
    assert math.isnan(res["euclidean_mean"]) and math.isnan(res["euclidean_std"])
    assert all(math.isnan(v) for v in res["quantiles"].values()) and math.isnan(res["euclidean_median"])


def test_two_calls_return_identical_bits():
    from cape_amd import ops
    hb = _dev(_buffer((64, 3627), "exp"))
    a, b = ops.error_statistics(hb, QS), ops.error_statistics(hb, QS)
    bits = lambda x: np.asarray(x, dtype=np.float64).view(np.uint64)
    for k in ("euclidean_mean", "euclidean_var", "euclidean_std", "per_vertex_mean", "per_sample_mean"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["order_values"].view(np.uint32), b["order_values"].view(np.uint32))
    assert a["quantiles"] == b["quantiles"]


# ---- 3. model ------------------------------------------------------------------------------------------------------------

def _model(mesh_ops, **overrides):
    from cape_amd.models import CAPE
    from oracle.configs import cape_params
    m = mesh_ops
    P = cape_params("affine_nz64", 2)
    P.update(overrides)
    model = CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], p=m["p"], **P)
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='train')
    model.load_variables({}, strict=False)                    # the initial weights count as loaded: no checkpoint is looked for
    return P, model


def _numpy_statistics_agree(res, d):
    n = d.size
    d64 = d.astype(np.float64)
    mean = R.fsum_mean(d64)
    std = math.sqrt(R.two_pass_var(d))
    med = float(np.median(d64))
    assert abs(res["euclidean_mean"] - mean) <= n * U53 * mean
    assert abs(res["euclidean_std"] - std) <= 2 * n * U53 * std            # the variance's 4 n 2^-53, halved by the root
    assert abs(res["euclidean_median"] - med) <= 4 * U53 * med
    assert abs(res["euclidean_mean"] - float(d64.mean())) <= 1e-12 * mean and abs(res["euclidean_std"] - float(d64.std())) <= 1e-12 * std
    assert (np.abs(res["per_vertex_mean"] - d64.mean(0)) <= 1e-12 * d64.mean(0)).all()
    assert (np.abs(res["per_sample_mean"] - d64.mean(1)) <= 1e-12 * d64.mean(1)).all()


def test_model_test_errors(mesh_ops):
    """Five samples at batch 2 (2 + 2 + a padded 1) with the shipped std and clothing vertices, seeded like
    test_predict_and_evaluate_report_the_weighted_recon: the losses are predict's bit for bit, the distances meet the parity
    bar against float64 recomputed from predict's predictions, the statistics equal numpy on the returned distances."""
    import test_gpu_model as T
    P, model = _model(mesh_ops)
    std, idx = _fixtures()
    x, gt, xd, cond, cond_d, clo, clo_d, eps = T._inputs(5, P["nz"], seed=4)
    torch.manual_seed(7)
    preds, lr_, ll_, le_ = model.predict(x, cond, clo, labels=gt, sess=model)
    torch.manual_seed(7)
    res = model.test_errors(x, cond, clo, labels=gt, std=std, clothing_idx=idx, quantiles=(0.5,), return_distances=True)
    assert (res["recon"], res["latent"], res["edge"]) == (lr_, ll_, le_)
    assert res["count"] == 5 * 3627 and res["nonfinite"] == 0
    d = res["distances"]
    assert d.shape == (5, 3627) and d.dtype == np.float32
    assert res["per_vertex_mean"].shape == (3627,) and res["per_sample_mean"].shape == (5,)
    gt32, std32 = gt.astype(np.float32), std.astype(np.float32)             # what the device holds
    d64 = R.distances(preds, gt32, std32, idx, np.float64)
    assert d64.min() >= 1e-6
    err_f32 = R.rel_err(R.distances(preds, gt32, std32, idx, np.float32), d64)
    err_hip = R.rel_err(d, d64)
    print("test_errors distances: max rel err hip %.3e, fp32 restatement %.3e" % (err_hip, err_f32))
    parity_bar.check("test_model_test_errors", "distance", err_hip, err_f32)
    _numpy_statistics_agree(res, d)
    assert list(res["quantiles"]) == [0.5] and res["quantiles"][0.5] == res["euclidean_median"]

    # labels default to data, every vertex, std of ones
    torch.manual_seed(7)
    full = model.test_errors(x, cond, clo, quantiles=(0.25, 0.5))
    assert full["count"] == 5 * V and full["per_vertex_mean"].shape == (V,) and "distances" not in full
    torch.manual_seed(7)
    preds_x, lrx, llx, lex = model.predict(x, cond, clo, labels=x, sess=model)
    assert (full["recon"], full["latent"], full["edge"]) == (lrx, llx, lex)
    want = float(np.sqrt(((preds_x.astype(np.float64) - x.astype(np.float32)) ** 2).sum(-1)).mean())
    assert abs(full["euclidean_mean"] - want) <= 1e-6 * want

    # a NaN in the labels shows in the count, and the statistics are NaN
    bad = gt.copy()
    bad[3, idx[10], 1] = np.nan
    torch.manual_seed(7)
    nan = model.test_errors(x, cond, clo, labels=bad, std=std, clothing_idx=idx)
    assert nan["nonfinite"] > 0 and nan["count"] == 5 * 3627
    assert math.isnan(nan["euclidean_mean"]) and math.isnan(nan["euclidean_std"]) and math.isnan(nan["euclidean_median"])


def test_model_test_errors_bf16_storage(mesh_ops):
    """act_dtype='bf16': the statistics equal numpy on the run's own distances."""
    import test_gpu_model as T
    P, model = _model(mesh_ops, act_dtype='bf16')
    std, idx = _fixtures()
    x, gt, xd, cond, cond_d, clo, clo_d, eps = T._inputs(5, P["nz"], seed=4)
    torch.manual_seed(7)
    res = model.test_errors(x, cond, clo, labels=gt, std=std, clothing_idx=idx, return_distances=True)
    d = res["distances"]
    assert d.shape == (5, 3627) and res["nonfinite"] == 0 and np.isfinite([res["recon"], res["latent"], res["edge"]]).all()
    _numpy_statistics_agree(res, d)
