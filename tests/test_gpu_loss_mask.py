"""loss_mask on the device: the weighted reconstruction + edge loss (the weighted entry of cape_amd/csrc/loss.hip) against fp64
torch autograd of its definition, recon = sum w * l(pred - gt) / sum w (TF's Reduction.MEAN of the weighted loss, reference
lib/models.py:47-52, 357-369), and the model, the captured step and the drivers with a mask set."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_FILE = os.path.join(ROOT, "tests", "golden", "loss_mask_binary.npy")
V = 6890
TOL = 2e-5                   # tests/test_gpu_ops.py: per-vertex gradient error
KINDS = ["l1", "huber", "l2"]


def vertex_err(a, ref):
    a = np.asarray(a, dtype=np.float64).reshape(-1, ref.shape[-1])
    r = np.asarray(ref, dtype=np.float64).reshape(-1, ref.shape[-1])
    return np.sqrt(((a - r) ** 2).sum(-1)).max() / max(np.sqrt((r * r).sum(-1)).max(), 1e-30)


def _binary_mask():
    return np.repeat(np.load(MASK_FILE)[:, None], 3, 1)


def _random_mask(seed=5):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 2.0, (V, 3))
    w[rng.random((V, 3)) < 0.3] = 0.0                      # exact zeros
    return w


def _pointwise(d, kind):
    if kind == "l1":
        return d.abs()
    if kind == "huber":
        a = d.abs()
        return torch.where(a <= 0.1, 0.5 * a * a, 0.1 * a - 0.005)
    return d * d


def _weighted_recon(pred, gt, w, kind):
    W = torch.as_tensor(np.broadcast_to(w, pred.shape), dtype=pred.dtype)
    return (W * _pointwise(pred - gt, kind)).sum() / W.sum()


def _inputs(N, seed):
    """fp32-representable pred / gt with exact zeros and exact |d| = 0.1f among the differences."""
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((N, V, 3)).astype(np.float32)
    gt = (pred + 0.2 * rng.standard_normal((N, V, 3))).astype(np.float32)
    # one coordinate per vertex, so that no edge vector vanishes (the fp64 reference's sqrt has no gradient at 0)
    gt[:, :300, 0] = pred[:, :300, 0]                               # d = 0
    tenth = np.float32(0.1)
    pred[:, 300:600, 1], gt[:, 300:600, 1] = tenth, 0.0             # d = +0.1f
    pred[:, 600:900, 2], gt[:, 600:900, 2] = 0.0, tenth             # d = -0.1f
    return pred.astype(np.float64), gt.astype(np.float64)


def _tables(mesh_ops, dev):
    from cape_amd.graph import vertex_edge_table
    pack = mesh_ops["pack"]
    edges, vr = pack["edges_smpl"], pack["template_verts"]
    vptr, vidx = vertex_edge_table(edges, V)
    d = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    return edges, vr, (d(vr, torch.float32), d(edges, torch.int32), d(vptr, torch.int32), d(vidx, torch.int32))


def _masked(pred_dev, gt, w, kind, tabs, w_recon=0.7, w_edge=1.3, terms=()):
    from cape_amd import ops
    dev = pred_dev.device
    wt = torch.tensor(w, dtype=torch.float32, device=dev)
    wsum = float(wt.double().sum())
    term_a, w_a, term_b = terms if terms else (None, 0.0, None)
    return ops.ReconEdgeLossFn.apply(pred_dev, torch.tensor(gt, dtype=torch.float32, device=dev), *tabs, w_recon, w_edge,
                                     term_a, w_a, term_b, wt, wsum, kind)


@pytest.mark.parametrize("N", [1, 16])
@pytest.mark.parametrize("rows", ["dense", "rows4"])
@pytest.mark.parametrize("mask", ["binary", "random"])
@pytest.mark.parametrize("kind", KINDS)
def test_masked_recon_edge_loss(kind, mask, rows, N, mesh_ops):
    from oracle import torch_twin as tt
    dev = torch.device("cuda:0")
    edges, vr, tabs = _tables(mesh_ops, dev)
    pred, gt = _inputs(N, seed=11 + N)
    w = _binary_mask() if mask == "binary" else _random_mask()
    # fp64 autograd of the definition; the weights as the device holds them (fp32)
    w = w.astype(np.float32).astype(np.float64)
    tp = torch.tensor(pred, requires_grad=True)
    tg, tvr = torch.tensor(gt), torch.tensor(vr)
    recon = _weighted_recon(tp, tg, w, kind)
    edge = tt.edge_loss_calc(tp + tvr, tg + tvr, edges)
    (0.7 * recon + 1.3 * edge).backward()

    if rows == "dense":
        hp = torch.tensor(pred, dtype=torch.float32, device=dev, requires_grad=True)
        view = hp
    else:                                                    # the decoder's 16-byte rows, padding never read
        hp = torch.full((N, V, 4), 1e9, dtype=torch.float32, device=dev)
        hp[:, :, :3] = torch.tensor(pred, dtype=torch.float32, device=dev)
        hp.requires_grad_(True)
        view = hp[:, :, :3]
    ha = torch.tensor(3.5, dtype=torch.float32, device=dev, requires_grad=True)
    hb = torch.tensor(-0.75, dtype=torch.float32, device=dev)
    total, parts = _masked(view, gt, w, kind, tabs, terms=(ha, 0.25, hb))
    total.backward()
    r, e, tot = float(parts[0]), float(parts[1]), float(total)
    assert abs(r - recon.item()) < 1e-5 * abs(recon.item()), (r, recon.item())
    assert abs(e - edge.item()) < 1e-5 * abs(edge.item()), (e, edge.item())
    want = 0.7 * recon.item() + 1.3 * edge.item() + 0.25 * 3.5 - 0.75
    assert abs(tot - want) < 1e-5 * abs(want), (tot, want)
    assert abs(ha.grad.item() - 0.25) < 1e-7
    g = hp.grad if rows == "dense" else hp.grad[:, :, :3]
    assert vertex_err(g.cpu().numpy(), tp.grad.numpy()) < TOL
    if rows == "rows4":
        assert float(hp.grad[:, :, 3].abs().max()) == 0.0


def test_masked_loss_zero_weights_edge_bits_and_determinism(mesh_ops):
    """Zero-weight coordinates carry the edge gradient alone and do not see gt; the edge term is the unmasked kernel's, bit
    for bit; an all-ones l1 mask is the unmasked loss; two calls agree bit for bit."""
    from cape_amd import ops
    dev = torch.device("cuda:0")
    edges, vr, tabs = _tables(mesh_ops, dev)
    N = 4
    pred, gt = _inputs(N, seed=3)
    w = _random_mask(seed=8)
    zero = torch.tensor(w == 0.0, device=dev).expand(N, V, 3)
    hp = torch.tensor(pred, dtype=torch.float32, device=dev)
    hgt = torch.tensor(gt, dtype=torch.float32, device=dev)
    for kind in KINDS:
        p1 = hp.clone().requires_grad_(True)
        t1, parts1 = _masked(p1, gt, w, kind, tabs)
        t1.backward()
        # the edge alone through the unmasked kernel (w_recon = 0)
        p0 = hp.clone().requires_grad_(True)
        t0, parts0 = ops.ReconEdgeLossFn.apply(p0, hgt, *tabs, 0.0, 1.3)
        t0.backward()
        assert torch.equal(parts1[1], parts0[1]), kind                          # edge value: same bits
        assert torch.equal(p1.grad[zero], p0.grad[zero]), kind                  # zero weight: the edge gradient only
        # gt moved where the weight is zero: recon unchanged to the bit
        gt2 = gt + np.where(w == 0.0, 0.5, 0.0)[None]
        _, parts2 = _masked(hp.clone().requires_grad_(True), gt2, w, kind, tabs)
        assert torch.equal(parts2[0], parts1[0]), kind
        # determinism
        p3 = hp.clone().requires_grad_(True)
        t3, parts3 = _masked(p3, gt, w, kind, tabs)
        t3.backward()
        assert torch.equal(parts3, parts1) and torch.equal(t3, t1) and torch.equal(p3.grad, p1.grad), kind
    # all-ones l1 mask = the unmasked l1 loss
    pm = hp.clone().requires_grad_(True)
    tm, pa = _masked(pm, gt, np.ones((V, 3)), "l1", tabs)
    tm.backward()
    pu = hp.clone().requires_grad_(True)
    tu, pb = ops.ReconEdgeLossFn.apply(pu, hgt, *tabs, 0.7, 1.3)
    tu.backward()
    assert torch.equal(pa[1], pb[1])
    assert abs(float(pa[0]) - float(pb[0])) <= 4 * 2.0 ** -24 * abs(float(pb[0]))
    assert abs(float(tm) - float(tu)) <= 4 * 2.0 ** -24 * abs(float(tu))
    assert vertex_err(pm.grad.cpu().numpy(), pu.grad.cpu().numpy().astype(np.float64)) < 1e-6


# ---- model level ---------------------------------------------------------------------------------------------------------

def _project(tmp_path):
    d = tmp_path / "data"
    d.mkdir(parents=True, exist_ok=True)
    shutil.copyfile(MASK_FILE, str(d / "loss_mask_binary.npy"))
    return str(tmp_path)


def _build_masked(cfg, mesh_ops, N, tmp_path, overrides=None):
    """test_gpu_model._build with loss_mask='binary' on the model; the twin gets no loss_mask (it is reweighted instead)."""
    import test_gpu_model as T
    from cape_amd.models import CAPE
    P, twin = T._twin(cfg, mesh_ops, N, overrides)
    m = mesh_ops
    model = CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], p=m["p"], loss_mask='binary',
                 project_dir=_project(tmp_path), **P)
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='train')
    return P, twin, model


def _reweight(twin, ls, xh, gt, l1_sign=None):
    """The twin's losses with its recon replaced by the weighted one: loss_g - lambda recon + lambda recon_w."""
    w = _binary_mask().astype(np.float32).astype(np.float64)
    g = torch.as_tensor(gt, dtype=xh.dtype)
    if twin.which_loss == "l1" and l1_sign is not None:
        d = xh - g
        W = torch.as_tensor(np.broadcast_to(w, d.shape), dtype=d.dtype)
        rw = (W * torch.as_tensor(np.asarray(l1_sign), dtype=d.dtype) * d).sum() / W.sum()
    else:
        rw = _weighted_recon(xh, g, w, twin.which_loss if twin.which_loss in ("l1", "huber") else "l2")
    out = dict(ls)
    out['recon'] = rw
    out['loss_g'] = ls['loss_g'] - twin.lambda_l1 * ls['recon'] + twin.lambda_l1 * rw
    return out


@pytest.mark.parametrize("cfg,overrides", [("affine_nz64", None), ("cmr_nz18", dict(loss='huber'))],
                         ids=["affine_nz64_l1", "cmr_nz18_huber"])
def test_model_with_binary_mask(cfg, overrides, mesh_ops, tmp_path):
    """Forward losses and every variable's gradient of the masked model against the reweighted fp64 twin on the device's
    activation pattern (tests/test_gpu_model.py::_full_model_parity with the recon term weighted)."""
    import test_gpu_model as T
    from cape_amd import ops
    from parity_bar import check
    N = 2
    P, twin, model = _build_masked(cfg, mesh_ops, N, tmp_path, overrides)
    x, gt, xd, cond, cond_d, clo, clo_d, eps = T._inputs(N, P["nz"])
    xh, zm, zl, d_real, d_fake, ls = T._run_twin(twin, x, gt, xd, cond, cond_d, clo, clo_d, eps)
    ls = _reweight(twin, ls, xh, gt)
    model.load_variables(twin.vs.vars)
    dev = model.device
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    ops.ACT_TRACE, ops.L1_SIGN_TRACE = [], []
    try:
        out = model.forward_losses(t(x), t(cond), t(clo), t(gt), t(xd), t(cond_d), t(clo_d), eps=t(eps))
        signs, l1 = list(ops.ACT_TRACE), list(ops.L1_SIGN_TRACE)
    finally:
        ops.ACT_TRACE = ops.L1_SIGN_TRACE = None
    assert (len(l1) == 1) == (twin.which_loss == "l1")
    l1_sign = l1[0].numpy() if l1 else None
    tag = "masked_model[%s%s,N=%d]" % (cfg, "" if not overrides else "+" + ",".join(sorted(overrides)), N)
    for k in ('recon', 'latent', 'edge', 'gan_g', 'gan_d', 'loss_g', 'loss_d'):
        assert abs(float(out[k]) - float(ls[k])) < 1e-4 * max(abs(float(ls[k])), 1e-3), (k, float(out[k]), float(ls[k]))
    # the weighted recon differs from the plain mean (the mask is in effect)
    plain = float((torch.tensor(xh.detach().numpy()) - torch.tensor(gt)).abs().mean()) if twin.which_loss == "l1" else None
    if plain is not None:
        assert abs(float(out['recon']) - plain) > 1e-3 * plain

    P32, twin32 = T._twin(cfg, mesh_ops, N, overrides, tdtype=torch.float32)
    xh32, _, _, _, _, ls32 = T._run_twin(twin32, x, gt, xd, cond, cond_d, clo, clo_d, eps, signs=signs, l1_sign=l1_sign)
    ls32 = _reweight(twin32, ls32, xh32, gt, l1_sign)
    xhm, _, _, _, _, lsm = T._run_twin(twin, x, gt, xd, cond, cond_d, clo, clo_d, eps, signs=signs, l1_sign=l1_sign)
    lsm = _reweight(twin, lsm, xhm, gt, l1_sign)
    for k in ('loss_g', 'loss_d'):
        assert abs(float(lsm[k]) - float(ls[k])) < 1e-6 * max(abs(float(ls[k])), 1e-3), k
    g_names, d_names = model._g_names, model._d_names
    tg = torch.autograd.grad(lsm['loss_g'], [twin.params[n] for n in g_names], retain_graph=True, allow_unused=True)
    td = torch.autograd.grad(lsm['loss_d'], [twin.params[n] for n in d_names], allow_unused=True)
    hg = torch.autograd.grad(out['loss_g'], [model._vars[n] for n in g_names], retain_graph=True, allow_unused=True)
    hd = torch.autograd.grad(out['loss_d'], [model._vars[n] for n in d_names], allow_unused=True)
    fg = torch.autograd.grad(ls32['loss_g'], [twin32.params[n] for n in g_names], retain_graph=True, allow_unused=True)
    fd = torch.autograd.grad(ls32['loss_d'], [twin32.params[n] for n in d_names], allow_unused=True)
    rows, num, den, num32 = [], 0.0, 0.0, 0.0
    for names, tgr, hgr, fgr in ((g_names, tg, hg, fg), (d_names, td, hd, fd)):
        for n, a, b, c in zip(names, tgr, hgr, fgr):
            if a is None:
                assert b is None or float(b.abs().max()) == 0.0, n
                continue
            a64, b64, c64 = a.numpy(), b.cpu().numpy().astype(np.float64), c.numpy().astype(np.float64)
            e2, r2, f2 = ((b64 - a64) ** 2).sum(), (a64 ** 2).sum(), ((c64 - a64) ** 2).sum()
            rows.append((n, np.sqrt(e2 / max(r2, 1e-300)), r2, np.sqrt(f2 / max(r2, 1e-300))))
            num += e2
            den += r2
            num32 += f2
    gl = np.sqrt(num / den)
    judged = [r for r in rows if r[2] > 1e-16 * den]
    check(tag, "gradient, whole bucket (rel L2)", gl, np.sqrt(num32 / den), T.GRAD_TOL)
    check(tag, "gradient, worst variable (rel L2)", max(r[1] for r in judged), max(r[3] for r in judged), T.GRAD_TOL)
    print("masked model gradients: worst variable %.3g relative L2, global %.3g" % (max(r[1] for r in judged), gl))
    for n, e, r2, e32 in judged:
        assert e < T.GRAD_TOL, (n, e)
    assert gl < T.GRAD_TOL, gl


def test_graphed_step_with_mask(mesh_ops, tmp_path):
    """The captured adversarial step with the mask: bit-identical replays run after run, the replayed recon is the eager
    one, and the step calls the weighted loss entry once and the unmasked one never."""
    import test_gpu_model as T
    from cape_amd import ops
    from cape_amd.runtime import GraphedTrainStep
    N = 2
    P, twin, model = _build_masked("affine_nz64", mesh_ops, N, tmp_path, dict(regularization=0.5, lr_warmup=False,
                                                                                decay_steps=1000))
    x, gt, xd, cond, cond_d, clo, clo_d, eps = T._inputs(N, P["nz"])
    dev = model.device
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    runner = GraphedTrainStep(model, with_gan=True)
    runner.load_batch(data_g=x, cond_g=cond, cond2_g=clo, gt=gt, data_d=xd, cond_d=cond_d, cond2_d=clo_d, eps=eps)
    runner.capture(preserve_state=True)
    groups = ('g', 'd')
    start = {g: {k: model._opt_state[g][k].detach().clone() for k in ('flat', 'm')} for g in groups}
    step0 = model.global_step
    runs, first_recon = [], []
    for rep in range(2):
        with torch.no_grad():
            for g in groups:
                for k in ('flat', 'm'):
                    model._opt_state[g][k].copy_(start[g][k])
        model.global_step = step0
        for i in range(3):
            runner.step()
            if i == 0:
                torch.cuda.synchronize()
                first_recon.append(float(runner.losses['recon']))
        torch.cuda.synchronize()
        runs.append({(g, k): model._opt_state[g][k].detach().clone() for g in groups for k in ('flat', 'm')})
    moved = False
    for key in runs[0]:
        assert torch.equal(runs[0][key], runs[1][key]), key
        moved = moved or not torch.equal(runs[0][key], start[key[0]][key[1]])
    assert moved
    assert first_recon[0] == first_recon[1]
    # the eager evaluation from the same state (no autograd graph: a graph recorded outside the capture stream and kept
    # alive would tie later captures to the default stream)
    with torch.no_grad():
        for g in groups:
            for k in ('flat', 'm'):
                model._opt_state[g][k].copy_(start[g][k])
        eager = float(model.forward_losses(t(x), t(cond), t(clo), t(gt), t(xd), t(cond_d), t(clo_d), eps=t(eps),
                                           reg_via_bucket=True)['recon'])
    assert abs(first_recon[0] - eager) <= 1e-6 * abs(eager), (first_recon[0], eager)

    eager_runner = GraphedTrainStep(model, with_gan=True, use_graph=False)
    eager_runner.load_batch(data_g=x, cond_g=cond, cond2_g=clo, gt=gt, data_d=xd, cond_d=cond_d, cond2_d=clo_d, eps=eps)
    ops.LAUNCH_LOG = []
    try:
        eager_runner._fwd_bwd()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert names.count("masked_recon_edge_loss") == 1 and "recon_edge_loss" not in names, names


def test_predict_and_evaluate_report_the_weighted_recon(mesh_ops, tmp_path):
    """predict / evaluate average loss_terms' recon over the batches like the reference (:1083-1086, quirk C8: the padded
    last batch gets weight 0): with the mask that is sum w * |d| / sum w of every full batch, recomputed here in fp64."""
    import test_gpu_model as T
    N = 2
    P, twin, model = _build_masked("affine_nz64", mesh_ops, N, tmp_path)
    x, gt, xd, cond, cond_d, clo, clo_d, eps = T._inputs(5, P["nz"], seed=4)      # 5 = 2 + 2 + 1 (padded last batch)
    torch.manual_seed(7)
    preds, lr_, ll_, le_ = model.predict(x, cond, clo, labels=gt, sess=model)
    assert preds.shape == (5, V, 3) and np.isfinite([lr_, ll_, le_]).all()
    w = _binary_mask().astype(np.float32).astype(np.float64)
    p32 = lambda a: a.astype(np.float32).astype(np.float64)
    per_batch = [(w * np.abs(preds[b:b + N].astype(np.float64) - p32(gt[b:b + N]))).sum() / (N * w.sum()) for b in (0, 2)]
    want = sum(per_batch) * N / 5
    assert abs(lr_ - want) < 1e-5 * want, (lr_, want)
    plain = sum(np.abs(preds[b:b + N].astype(np.float64) - p32(gt[b:b + N])).mean() for b in (0, 2)) * N / 5
    assert abs(lr_ - plain) > 1e-3 * plain                  # the weighted mean, not the plain one
    torch.manual_seed(7)                                    # the same latent samples: evaluate reports predict's numbers
    string, er, el, ee = model.evaluate(x, cond, clo, gt, model)
    assert string.startswith('recon loss:')
    assert abs(er - lr_) <= 1e-6 * lr_ and abs(ee - le_) <= 1e-6 * le_


def test_fit_with_mask(mesh_ops, tmp_path):
    import types
    from test_gpu_dropin_api import _args_dict, _params
    from cape_amd import models
    m = mesh_ops
    ad = _args_dict()
    ad['loss_mask'] = 'binary'
    rng = np.random.default_rng(0)
    n_train, n_val = 8, 4
    data = types.SimpleNamespace(
        vertices_train=rng.standard_normal((n_train, V, 3)).astype(np.float32),
        cond1_train=rng.standard_normal((n_train, 126)).astype(np.float32),
        cond2_train=np.eye(4, dtype=np.float32)[rng.integers(0, 4, n_train)],
        vertices_val=rng.standard_normal((n_val, V, 3)).astype(np.float32),
        cond1_val=rng.standard_normal((n_val, 126)).astype(np.float32),
        cond2_val=np.eye(4, dtype=np.float32)[rng.integers(0, 4, n_val)])
    params = _params(ad, m["p"], decay_steps=ad['decay_every'] * n_train / ad['batch_size'])
    assert params['loss_mask'] == 'binary'
    model = models.CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], project_dir=_project(tmp_path), **params)
    assert model.loss_mask.shape == (model.batch_size, V, 3)
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='train')
    loss, t_step = model.fit(data)
    assert len(loss) >= 1 and np.isfinite(loss).all() and t_step > 0
    assert os.path.exists(os.path.join(str(tmp_path), 'checkpoints', params['name']))


def test_bf16_storage_with_mask(mesh_ops, tmp_path):
    """act_dtype='bf16' (BASELINE configs[4]) with the mask: the losses see fp32 and take the same kernel; forward within
    test_gpu_bf16's 2e-2 bar of the reweighted fp64 twin, gradients within its global bar."""
    import test_gpu_model as T
    from cape_amd import ops
    N = 2
    P, twin, model = _build_masked("affine_nz64", mesh_ops, N, tmp_path, dict(act_dtype='bf16'))
    x, gt, xd, cond, cond_d, clo, clo_d, eps = T._inputs(N, P["nz"])
    xh, zm, zl, d_real, d_fake, ls = T._run_twin(twin, x, gt, xd, cond, cond_d, clo, clo_d, eps)
    ls = _reweight(twin, ls, xh, gt)
    model.load_variables(twin.vs.vars)
    dev = model.device
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    ops.LAUNCH_LOG = []
    try:
        out = model.forward_losses(t(x), t(cond), t(clo), t(gt), t(xd), t(cond_d), t(clo_d), eps=t(eps))
        torch.cuda.synchronize()
        names = [r[0] for r in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert names.count("masked_recon_edge_loss") == 1 and "recon_edge_loss" not in names
    for k in ('recon', 'latent', 'edge', 'gan_g', 'gan_d', 'loss_g', 'loss_d'):
        assert abs(float(out[k]) - float(ls[k])) < 2e-2 * max(abs(float(ls[k])), 1e-3), (k, float(out[k]), float(ls[k]))
    g_names = model._g_names
    tg = torch.autograd.grad(ls['loss_g'], [twin.params[n] for n in g_names], allow_unused=True)
    hg = torch.autograd.grad(out['loss_g'], [model._vars[n] for n in g_names], allow_unused=True)
    num = den = 0.0
    for a, b in zip(tg, hg):
        if a is None:
            continue
        a64, b64 = a.numpy(), b.cpu().numpy().astype(np.float64)
        num += ((b64 - a64) ** 2).sum()
        den += (a64 ** 2).sum()
    gl = float(np.sqrt(num / den))
    print("bf16 storage with mask: generator gradients, global relative L2 error %.2e" % gl)
    assert gl < 3e-2, gl
