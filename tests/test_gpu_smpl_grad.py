"""Differentiable SMPL posing on the device (cape_amd.smpl.SMPL.forward_diff / dress_diff; csrc/smpl/smpl_bwd.hip) and
CAPE.fit_posed on top of it.  Gradients are held against torch autograd on the float64 twin of the numpy oracle
(tests/smpl_torch_twin.py) under tests/parity_bar.py's bar: each gradient is divided by the float64 gradient's max-abs, and
the HIP path's max-abs error may be at most 4x that of the float32 twin on the CPU (floor 4 * 2^-24).  Every path sees the
same fp32 inputs; seeded synthetic SMPL-format models (tests/smpl_synth.py)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity_bar                # noqa: E402
import smpl_reference as ref     # noqa: E402
import smpl_synth as synth       # noqa: E402
import smpl_torch_twin as twin   # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("T", "pose", "betas", "transl")


@functools.lru_cache(maxsize=None)
def _model(which):
    from cape_amd import smpl
    m = getattr(synth, which)()
    return m, smpl.SMPL(m)


def _inputs(m, N, seed, shared, B, transl, gV, gJ):
    """fp32 inputs with the edge cases of Rodrigues' formula: an all-zero pose row, a joint at |r| = 4e-4 (the series
    branch) and one just above the threshold |r|^2 = 1e-6."""
    rng = np.random.default_rng(seed)
    J, V = len(ref.parents_of(m)), m["v_template"].shape[0]
    T = m["v_template"][None] + 0.01 * rng.standard_normal((1 if shared else N, V, 3))
    pose = 0.5 * rng.standard_normal((N, 3 * J))
    r = N - 1                                        # N = 1: the small rotations share the only row
    if N > 1:
        pose[0] = 0.0
    pose[r, 3:6] = np.array([1.0, -2.0, 2.0]) * (4e-4 / 3.0)
    pose[r, 6:9] = [0.0, 1.001e-3, 0.0]
    pose[r, 9:12] = 0.0
    f32 = lambda a: np.asarray(a, np.float32)
    return dict(T=f32(T), pose=f32(pose), betas=f32(0.8 * rng.standard_normal((N, B))) if B else None,
                transl=f32(0.3 * rng.standard_normal((N, 3))) if transl else None,
                gV=f32(rng.standard_normal((N, V, 3))) if gV else None, gJ=f32(rng.standard_normal((N, J, 3))) if gJ else None)


def _nerr(a, g64):
    return float(np.abs(np.asarray(a, np.float64) - g64).max() / np.abs(g64).max())


def _hip_gradients(model, x, need):
    dev = lambda k: None if x[k] is None else torch.tensor(x[k], device="cuda").requires_grad_(k in need)
    ins = {k: dev(k) for k in NAMES}
    v, j = model.forward_diff(ins["T"], ins["pose"], ins["betas"], ins["transl"])
    with torch.no_grad():                                                   # the plain forward on the same values
        plain = model.forward(*[None if t is None else t.detach() for t in ins.values()])
    assert torch.equal(v, plain[0]) and torch.equal(j, plain[1])
    loss = 0
    if x["gV"] is not None:
        loss = loss + (v * torch.tensor(x["gV"], device="cuda")).sum()
    if x["gJ"] is not None:
        loss = loss + (j * torch.tensor(x["gJ"], device="cuda")).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {k: None if (t is None or t.grad is None) else t.grad.cpu().numpy() for k, t in ins.items()}


def _check_case(tag, which, N, shared=False, B=10, transl=True, gV=True, gJ=True, need=NAMES):
    m, model = _model(which)
    x = _inputs(m, N, len(tag) + N, shared, B, transl, gV, gJ)
    args = (x["T"], x["pose"], x["betas"], x["transl"], x["gV"], x["gJ"])
    g64 = twin.gradients(m, torch.float64, *args)
    g32 = twin.gradients(m, torch.float32, *args)
    hip = _hip_gradients(model, x, need)
    for k in NAMES:
        if x[k] is None or k not in need:
            assert hip[k] is None, "%s: %s got a gradient it did not ask for" % (tag, k)
            continue
        assert hip[k].shape == x[k].shape and np.isfinite(hip[k]).all(), (tag, k)
        parity_bar.check(tag, "d" + k, _nerr(hip[k], g64[k]), _nerr(g32[k], g64[k]))
    return hip


@pytest.mark.parametrize("N", [1, 3, 17])
def test_gradients_small_model(N):
    _check_case("grad_small_N%d_per_sample" % N, "small", N)
    _check_case("grad_small_N%d_shared_T_betas4" % N, "small", N, shared=True, B=4, transl=False)
    _check_case("grad_small_N%d_no_betas_gV_only" % N, "small", N, B=0, gJ=False)
    _check_case("grad_small_N%d_shared_T_gJ_only" % N, "small", N, shared=True, gV=False)


@pytest.mark.parametrize("N,shared,B,transl", [(1, False, 10, True), (17, False, 10, True), (17, True, 4, False)])
def test_gradients_smpl_sized_model(N, shared, B, transl):
    """N = 17 crosses the 16-sample tile and leaves a one-sample tail."""
    _check_case("grad_smpl24_N%d_%s_betas%d" % (N, "shared_T" if shared else "per_sample", B), "smpl_like", N, shared=shared, B=B,
                transl=transl)


def test_gradients_across_the_lds_tile_of_the_52_joint_model():
    """K = 469 coefficients: 14 samples per workgroup, N = 15 leaves a one-sample tail."""
    _, model = _model("j52")
    plan = (C.c_int32 * 3)()
    from cape_amd._lib import lib
    assert lib.cape_smpl_skin_bwd_plan(10 + 9 * 51, 52, model.V, 15, plan) == 0 and plan[0] == 14
    _check_case("grad_j52_N15", "j52", 15)


def test_gradients_with_four_wave_workgroups():
    """From ten tiles of samples on, the vertex pass runs 256-thread workgroups: the partial sums cross the waves in LDS."""
    _, model = _model("smpl_like")
    plan = (C.c_int32 * 3)()
    from cape_amd._lib import lib
    assert lib.cape_smpl_skin_bwd_plan(10 + 9 * 23, 24, model.V, 146, plan) == 0 and list(plan)[:2] == [16, 27]
    _check_case("grad_smpl24_N146_shared_T", "smpl_like", 146, shared=True)


@pytest.mark.parametrize("which,N", [("small", 17), ("smpl_like", 17)])
def test_only_the_inputs_that_ask_get_a_gradient(which, N):
    """Subsets of the inputs requiring grad; without pose and betas the vertex pass skips its gcoef sums."""
    _check_case("grad_%s_subset_pose_transl" % which, which, N, need=("pose", "transl"))
    _check_case("grad_%s_subset_T" % which, which, N, need=("T",))
    _check_case("grad_%s_subset_T_transl_shared" % which, which, N, shared=True, need=("T", "transl"))
    _check_case("grad_%s_subset_betas_gJ_only" % which, which, N, gV=False, need=("betas",))


def test_backward_is_bitwise_repeatable():
    m, model = _model("smpl_like")
    x = _inputs(m, 19, 3, False, 10, True, True, True)
    a = _hip_gradients(model, x, NAMES)
    b = _hip_gradients(model, x, NAMES)
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)
    x = _inputs(m, 19, 4, True, 10, True, True, True)
    a, b = _hip_gradients(model, x, NAMES), _hip_gradients(model, x, NAMES)
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)


def _dress_fixtures():
    st = np.load(os.path.join(GOLD, "trainset_stats.npz"))
    return st["mean"], st["std"], np.load(os.path.join(GOLD, "clothing_verts_idx.npy")), synth.template()


def test_dress_diff_gradient_is_mask_times_std():
    from cape_amd import smpl
    mean, std, idx, minimal = _dress_fixtures()
    rng = np.random.default_rng(5)
    d = rng.standard_normal((5, 6890, 3)).astype(np.float32)
    g = rng.standard_normal((5, 6890, 3)).astype(np.float32)
    disp = torch.tensor(d, device="cuda", requires_grad=True)
    T = smpl.dress_diff(disp, mean, std, idx, minimal)
    assert torch.equal(T, smpl.dress(disp.detach(), mean, std, idx, minimal))
    (T * torch.tensor(g, device="cuda")).sum().backward()
    mask = np.zeros((6890, 1))
    mask[idx] = 1.0
    std3 = np.reshape(std, (6890, 3))
    g64 = mask * std3.astype(np.float64) * g
    g32 = mask.astype(np.float32) * std3.astype(np.float32) * g
    parity_bar.check("smpl_dress_diff", "d_disp", _nerr(disp.grad.cpu().numpy(), g64), _nerr(g32, g64))


def _weighted_l2(posed, target, w):
    """cape_smpl_weighted_l2 on device tensors: (loss [N], grad [N,V,3])."""
    from cape_amd._lib import lib, check
    N, V = posed.shape[0], posed.shape[1]
    loss, grad = torch.empty(N, device="cuda"), torch.empty_like(posed)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(lib.cape_smpl_weighted_l2(p(posed), 3 * V, p(target), 3 * V, p(w), 1.0 / float(w.double().sum()), N, V, p(loss), p(grad),
                                    3 * V, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "cape_smpl_weighted_l2")
    return loss, grad


def test_composed_chain_dress_pose_weighted_l2():
    """dress_diff -> forward_diff -> weighted L2 to a target: the gradient arriving at the displacements, against the float64
    twin composed with smpl_reference.dress's formula -- the whole new chain without the decoder."""
    from cape_amd import smpl
    m, model = _model("smpl_like")
    mean, std, idx, minimal = _dress_fixtures()
    rng = np.random.default_rng(8)
    N, V = 5, 6890
    f32 = lambda a: np.asarray(a, np.float32)
    d = f32(rng.standard_normal((N, V, 3)))
    pose = f32(0.5 * rng.standard_normal((N, 72)))
    transl = f32(0.3 * rng.standard_normal((N, 3)))
    w = f32(rng.uniform(0.0, 2.0, V))
    target = f32(ref.forward(m, ref.dress(f32(0.9 * d), mean, std, idx, minimal), pose, None, transl)[0]
                 + 0.01 * rng.standard_normal((N, V, 3)))

    def by_twin(dtype):
        tw = twin.Twin(m, dtype)
        disp = tw.tensor(d, True)
        cast = (lambda a: np.asarray(a, np.float32)) if dtype == torch.float32 else (lambda a: a)
        v, _ = tw.forward(tw.dress(disp, cast(mean), cast(std), idx, cast(minimal)), tw.tensor(pose), None, tw.tensor(transl))
        wt = tw.tensor(w)
        per_sample = (wt[None, :, None] * (v - tw.tensor(target)) ** 2).sum((1, 2)) / wt.sum()
        per_sample.sum().backward()
        return disp.grad.double().numpy(), per_sample.detach().double().numpy()

    g64, l64 = by_twin(torch.float64)
    g32, l32 = by_twin(torch.float32)
    disp = torch.tensor(d, device="cuda", requires_grad=True)
    posed, _ = model.forward_diff(smpl.dress_diff(disp, mean, std, idx, minimal), torch.tensor(pose, device="cuda"), None,
                                  torch.tensor(transl, device="cuda"))
    loss, grad = _weighted_l2(posed.detach(), torch.tensor(target, device="cuda"), torch.tensor(w, device="cuda"))
    torch.autograd.backward([posed], [grad])
    torch.cuda.synchronize()
    parity_bar.check("smpl_chain", "loss", _nerr(loss.cpu().numpy(), l64), _nerr(l32, l64))
    parity_bar.check("smpl_chain", "d_disp", _nerr(disp.grad.cpu().numpy(), g64), _nerr(g32, g64))


# ---- CAPE.fit_posed ------------------------------------------------------------------------------------------------------
SIZE = 5


@pytest.fixture(scope="module")
def fit_setup(mesh_ops):
    from cape_amd import smpl
    from test_gpu_smpl import _cape_model
    model = _cape_model(mesh_ops, batch_size=4)                 # size 5: the last batch is padded
    m = synth.smpl_like(seed=6)
    body = smpl.SMPL(m)
    rng = np.random.default_rng(21)
    cond, cond2 = rng.standard_normal((SIZE, model.nz_cond)), rng.standard_normal((SIZE, model.nz_cond2))
    z_true = rng.standard_normal((SIZE, model.nz))
    pose = np.load(os.path.join(GOLD, "demo_pose_params.npz"))["pose"][rng.integers(0, 6, SIZE)]
    st = np.load(os.path.join(GOLD, "trainset_stats.npz"))
    idx = np.load(os.path.join(GOLD, "clothing_verts_idx.npy"))
    dress_args = (st["mean"], st["std"], idx)
    target, _ = model.decode_posed(np.concatenate([z_true, cond, cond2], 1), cond, cond2, pose, body, *dress_args)
    return dict(model=model, m=m, body=body, cond=cond, cond2=cond2, z_true=z_true, pose=pose, dress=dress_args, target=target)


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


def _data_term(posed, target, dtype, w=None):
    w = np.ones(posed.shape[1], dtype) if w is None else w.astype(dtype)
    d = posed.astype(dtype) - target.astype(dtype)
    return (w[None, :, None] * (d * d)).sum((1, 2), dtype=dtype) / w.sum(dtype=dtype)


def test_fit_posed_without_steps_is_decode_posed_and_its_data_term(fit_setup):
    s = fit_setup
    model, m, (mean, std, idx) = s["model"], s["m"], s["dress"]
    z0 = 0.3 * np.random.default_rng(1).standard_normal((SIZE, model.nz))
    res = model.fit_posed(s["target"], s["pose"], s["cond"], s["cond2"], s["body"], *s["dress"], z0=z0, steps=0)
    assert res["z"].shape == (SIZE, model.nz) and res["loss"].shape == (1, SIZE) and res["transl"] is None
    assert np.array_equal(res["z"], z0.astype(np.float32)) and np.array_equal(res["pose"], s["pose"].astype(np.float32))
    # test_decode_posed_equals_decode_then_dress_and_pose's comparison, on fit_posed's outputs
    zt = np.concatenate([z0, s["cond"], s["cond2"]], 1)
    pred = model.decode(zt, cond=s["cond"], cond2=s["cond2"])
    minimal = model.verts_ref
    t64 = ref.dress(pred, mean, std, idx, minimal)
    t32 = ref.dress(pred.astype(np.float32), mean.astype(np.float32), std.astype(np.float32), idx, minimal.astype(np.float32),
                    np.float32)
    parity_bar.check("fit_posed_steps0", "clothed", _err(res["clothed"], t64), _err(t32, t64))
    v64, _ = ref.forward(m, t64, s["pose"])
    v32, _ = ref.forward(m, t32, s["pose"].astype(np.float32), dtype=np.float32)
    extent = float(np.ptp(v64.reshape(-1, 3), 0).max())
    parity_bar.check("fit_posed_steps0", "posed", _err(res["posed"], v64), _err(v32, v64), also_below=1e-5 * extent)
    # loss[0]: the data term of decode_posed(z0), in float64 numpy
    posed0, _ = model.decode_posed(zt, s["cond"], s["cond2"], s["pose"], s["body"], *s["dress"])
    l64, l32 = _data_term(posed0, s["target"], np.float64), _data_term(posed0, s["target"], np.float32)
    parity_bar.check("fit_posed_steps0", "loss0", _nerr(res["loss"][0], l64), _nerr(l32, l64))
    # the same with per-vertex weights (a fifth of them zero): sum_v w_v |d_v|^2 / sum_v w_v
    w = np.random.default_rng(3).uniform(0.0, 2.0, 6890).astype(np.float32)
    w[::5] = 0.0
    res_w = model.fit_posed(s["target"], s["pose"], s["cond"], s["cond2"], s["body"], *s["dress"], z0=z0, steps=0, weights=w)
    l64, l32 = _data_term(posed0, s["target"], np.float64, w), _data_term(posed0, s["target"], np.float32, w)
    parity_bar.check("fit_posed_steps0", "loss0_weighted", _nerr(res_w["loss"][0], l64), _nerr(l32, l64))


def _snapshot(model):
    return {k: (v.detach().clone(), v.requires_grad) for k, v in model._vars.items()}


def _assert_model_untouched(model, before, decode_in, decode_out):
    for k, v in model._vars.items():
        assert torch.equal(v.detach(), before[k][0]) and v.grad is None and v.requires_grad == before[k][1], k
    again = model.decode(decode_in[0], cond=decode_in[1], cond2=decode_in[2])
    assert again.tobytes() == decode_out.tobytes()


def _assert_fit_consistent(s, res, steps, pose=None):
    model = s["model"]
    assert res["z"].shape == (SIZE, model.nz) and res["loss"].shape == (steps + 1, SIZE)      # no z for the padded rows
    assert np.isfinite(res["loss"]).all() and np.all(res["loss"][-1] < res["loss"][0]), res["loss"][[0, -1]]
    zt = np.concatenate([res["z"], s["cond"], s["cond2"]], 1)
    posed, clothed = model.decode_posed(zt, s["cond"], s["cond2"], res["pose"] if pose is None else pose, s["body"], *s["dress"])
    # fit_posed evaluates the returned leaves exactly as decode_posed does: the same bits
    assert np.array_equal(res["posed"], posed) and np.array_equal(res["clothed"], clothed)


def test_fit_posed_lowers_the_data_term_and_leaves_the_model_alone(fit_setup):
    s = fit_setup
    model = s["model"]
    before = _snapshot(model)
    din = (np.concatenate([s["z_true"], s["cond"], s["cond2"]], 1), s["cond"], s["cond2"])
    dout = model.decode(din[0], cond=din[1], cond2=din[2])
    steps = 30
    res = model.fit_posed(s["target"], s["pose"], s["cond"], s["cond2"], s["body"], *s["dress"], steps=steps)
    _assert_fit_consistent(s, res, steps)
    assert np.array_equal(res["pose"], s["pose"].astype(np.float32))
    _assert_model_untouched(model, before, din, dout)
    # the edge term on request: another objective, same bookkeeping
    res_e = model.fit_posed(s["target"], s["pose"], s["cond"], s["cond2"], s["body"], *s["dress"], steps=3, lambda_edge=1.0)
    assert np.isfinite(res_e["z"]).all() and not np.array_equal(res_e["z"], model.fit_posed(
        s["target"], s["pose"], s["cond"], s["cond2"], s["body"], *s["dress"], steps=3)["z"])
    _assert_model_untouched(model, before, din, dout)


def test_fit_posed_with_pose_and_translation_as_leaves(fit_setup):
    s = fit_setup
    model = s["model"]
    before = _snapshot(model)
    din = (np.concatenate([s["z_true"], s["cond"], s["cond2"]], 1), s["cond"], s["cond2"])
    dout = model.decode(din[0], cond=din[1], cond2=din[2])
    pose0 = (s["pose"] + 0.05 * np.random.default_rng(2).standard_normal(s["pose"].shape)).astype(np.float32)
    steps = 30
    res = model.fit_posed(s["target"], pose0, s["cond"], s["cond2"], s["body"], *s["dress"], steps=steps, optimize_pose=True,
                          optimize_transl=True)
    assert res["pose"].shape == pose0.shape and res["transl"].shape == (SIZE, 3)
    assert np.all(np.abs(res["pose"] - pose0).max(1) > 0) and np.all(np.abs(res["transl"]).max(1) > 0)
    assert res["z"].shape == (SIZE, model.nz) and np.all(res["loss"][-1] < res["loss"][0]), res["loss"][[0, -1]]
    zt = np.concatenate([res["z"], s["cond"], s["cond2"]], 1)
    posed, _ = model.decode_posed(zt, s["cond"], s["cond2"], res["pose"], s["body"], *s["dress"], transl=res["transl"])
    assert np.array_equal(res["posed"], posed)
    _assert_model_untouched(model, before, din, dout)


def test_fit_posed_prior_term_has_the_documented_weight(fit_setup):
    """lambda_z * mean(z^2) adds 2 lambda_z z / nz to the gradient.  With the target made from z0 itself the data gradient at
    z0 is a rounding residual r, so the first Adam step (m = g, v = g^2) is  -lr g / (|g| + 1e-8)  with  g = k z0 + r,
    k = 2 lambda_z / nz.  k = 4e-7 puts |g| next to Adam's epsilon for |z0| <= 0.1, where the step depends on k: half or twice
    the weight moves it by up to 0.17 lr.  Bound on r: the differentiated forward's posed mesh is within 2.4e-7 m of the target
    (DESIGN 7f), so the gradient on a coordinate is at most 2 * 2.4e-7 / 6890 = 7e-11; a unit of one z component moves a
    coordinate by about 1.6e-4 m (1.3e-3 m rms for all 64); all 20670 coordinates pulling the same way give
    |r| <= 20670 * 1.6e-4 * 7e-11 = 2.3e-10, which moves the step by at most lr * |r| / 1e-8 = 0.023 lr: the tolerance."""
    s = fit_setup
    model, lr, k = s["model"], 0.1, 4e-7
    z0 = np.random.default_rng(4).uniform(-0.1, 0.1, (SIZE, model.nz)).astype(np.float32)
    zt = np.concatenate([z0, s["cond"], s["cond2"]], 1)
    target, _ = model.decode_posed(zt, s["cond"], s["cond2"], s["pose"], s["body"], *s["dress"])
    res = model.fit_posed(target, s["pose"], s["cond"], s["cond2"], s["body"], *s["dress"], z0=z0, steps=1, lr=lr,
                          lambda_z=k * model.nz / 2)
    g = k * z0.astype(np.float64)
    want = z0 - lr * g / (np.abs(g) + 1e-8)
    err = float(np.abs(res["z"] - want).max())
    print("prior step: max |z1 - expected| = %.3e (tolerance %.3e)" % (err, 0.023 * lr))
    assert err <= 0.023 * lr
    # without the prior the same step is the residual's alone: nowhere near the prior's
    res0 = model.fit_posed(target, s["pose"], s["cond"], s["cond2"], s["body"], *s["dress"], z0=z0, steps=1, lr=lr, lambda_z=0.0)
    assert float(np.abs(res0["z"] - z0).max()) <= 0.023 * lr


def test_fit_posed_edge_term_is_per_sample(fit_setup):
    """The edge term is normalised per sample: a sample fitted alone (a batch with one live row) and the same sample in a full
    batch of four take the same steps.  Adam's step lr g / (|g| + eps) moves by at most lr |dg| eps / (|g| + eps)^2 <= lr / 4
    times the relative error of g; kernels that sum a batch in another order give g to about 1e-6, so three steps agree to a
    few 1e-7 lr: held to 1e-4 lr.  A batch mean left in the term would scale it by four and move the steps by a share of lr."""
    s = fit_setup
    model, lr = s["model"], 0.1
    args = lambda sl: (s["target"][sl], s["pose"][sl], s["cond"][sl], s["cond2"][sl], s["body"]) + tuple(s["dress"])
    kw = dict(steps=3, lr=lr, lambda_edge=1.0)
    full = model.fit_posed(*args(slice(0, SIZE)), **kw)
    alone = model.fit_posed(*args(slice(0, 1)), **kw)
    plain = model.fit_posed(*args(slice(0, 1)), steps=3, lr=lr)
    d_same, d_edge = float(np.abs(alone["z"][0] - full["z"][0]).max()), float(np.abs(alone["z"][0] - plain["z"][0]).max())
    print("edge term: alone vs in a batch %.3e, with vs without the term %.3e" % (d_same, d_edge))
    assert d_same <= 1e-4 * lr
    assert d_edge > 1e-2 * lr, "the edge term does not move the fit: the comparison above shows nothing"
