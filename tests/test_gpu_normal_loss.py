"""lambda_normal on the device: the face-normal loss (cape_amd/csrc/normal_loss/face_normal_loss.hip) against fp64 torch
autograd of its definition (tests/normal_loss_reference.py; reference lib/losses.py:27-52), and the model, the captured step
and the drivers with the option on.

Bars: SURVEY 8(c) through tests/parity_bar.check -- the device's error against fp64 may be at most 4 x the error of the fp32
restatement on the same inputs and measure (floor 4 * 2^-24): (a) the value as an ABSOLUTE error (every term lies in [0, 1]),
(b) the gradient's vertex_err (max per-vertex error norm / max per-vertex gradient norm), (c) its whole-tensor relative L2.
sign(c) is discontinuous, so every parity case first asserts, on the CPU references alone, that fp64 min |c| >= 1e-5 and that
the fp32 and fp64 restatements agree on every sign(c); no face is ever left out of a comparison."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACES_FILE = os.path.join(ROOT, "tests", "golden", "template_faces.npy")
V = 6890
MIN_C_OP, MIN_C_MODEL = 1e-5, 1e-3


def vertex_err(a, ref):
    a = np.asarray(a, dtype=np.float64).reshape(-1, ref.shape[-1])
    r = np.asarray(ref, dtype=np.float64).reshape(-1, ref.shape[-1])
    return np.sqrt(((a - r) ** 2).sum(-1)).max() / max(np.sqrt((r * r).sum(-1)).max(), 1e-30)


def rel_l2(a, ref):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.sqrt(((a - r) ** 2).sum() / max((r * r).sum(), 1e-300))


def _faces():
    return np.load(FACES_FILE)


def _recipe(seed, N, s, t, nv=V):
    """The issue's input recipe: float32-rounded pred / gt, returned as float64 arrays holding those values."""
    rng = np.random.default_rng(seed)
    pred = (s * rng.standard_normal((N, nv, 3))).astype(np.float32)
    gt = (pred + t * rng.standard_normal((N, nv, 3))).astype(np.float32)
    return pred.astype(np.float64), gt.astype(np.float64)


RECIPES = {"rng13": (13, 2, 1.0, 0.2), "rng27_n16": (27, 16, 1.0, 0.2), "rng5_c_near_1": (5, 2, 1.0, 1e-3),
           "rng7_template_scale": (7, 2, 0.02, 0.005)}


def _tables(faces, nv, dev):
    from cape_amd.graph import vertex_face_table
    fptr, fidx = vertex_face_table(faces, nv)
    d = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.int32, device=dev)
    return d(faces), d(fptr), d(fidx)


def _device(pred, gt, vr, faces, w=1.0, rows="dense", term=None):
    """(normal, total, d total / d pred [N, nv, 3], pad gradient or None, d total / d term or None) from the device op."""
    from cape_amd import ops
    dev = torch.device("cuda:0")
    N, nv, _ = pred.shape
    tabs = _tables(faces, nv, dev)
    if rows == "dense":
        hp = torch.tensor(pred, dtype=torch.float32, device=dev, requires_grad=True)
        view = hp
    else:                                                    # the decoder's 16-byte rows, padding never read
        hp = torch.full((N, nv, 4), 1e9, dtype=torch.float32, device=dev)
        hp[:, :, :3] = torch.tensor(pred, dtype=torch.float32, device=dev)
        hp.requires_grad_(True)
        view = hp[:, :, :3]
    ht = None if term is None else torch.tensor(term, dtype=torch.float32, device=dev, requires_grad=True)
    total, parts = ops.FaceNormalLossFn.apply(view, torch.tensor(gt, dtype=torch.float32, device=dev),
                                              torch.tensor(vr, dtype=torch.float32, device=dev), *tabs, w, ht)
    assert parts.shape == (1,) and not parts.requires_grad
    total.backward()
    torch.cuda.synchronize()
    g = hp.grad.cpu().numpy().astype(np.float64)
    return (float(parts[0]), float(total), g[:, :, :3], g[:, :, 3] if rows != "dense" else None,
            None if ht is None else float(ht.grad))


def _references(pred, gt, vr, faces, min_c):
    """fp64 and fp32 restatements, after the condition on the inputs (CPU references only)."""
    import normal_loss_reference as R
    vr32 = np.asarray(vr, dtype=np.float32)
    v64, g64, c64 = R.evaluate(pred, gt, vr32.astype(np.float64), faces, torch.float64)
    v32, g32, c32 = R.evaluate(pred, gt, vr32, faces, torch.float32)
    assert np.abs(c64).min() >= min_c, ("input condition: fp64 min |c| = %.3g" % np.abs(c64).min())
    assert np.array_equal(np.sign(c64), np.sign(c32)), "input condition: fp32 and fp64 disagree on a sign(c)"
    return (v64, g64), (v32, g32), c64


def _judge(tag, dev_val, dev_grad, ref64, ref32, w=1.0):
    from parity_bar import check
    (v64, g64), (v32, g32) = ref64, ref32
    errs = (abs(dev_val - v64), vertex_err(dev_grad, w * g64), rel_l2(dev_grad, w * g64))
    errs32 = (abs(v32 - v64), vertex_err(w * g32, w * g64), rel_l2(w * g32, w * g64))
    print("%s: value %.8g (fp64 %.8g) abs err %.2e [fp32 %.2e]; gradient vertex_err %.2e [fp32 %.2e], rel L2 %.2e [fp32 %.2e]"
          % (tag, dev_val, v64, errs[0], errs32[0], errs[1], errs32[1], errs[2], errs32[2]))
    check(tag, "normal value (abs)", errs[0], errs32[0])
    check(tag, "normal gradient (vertex_err)", errs[1], errs32[1])
    check(tag, "normal gradient (rel L2)", errs[2], errs32[2])


# ---- 1. op parity on the real template -----------------------------------------------------------------------------------

@pytest.mark.parametrize("with_term", [False, True], ids=["alone", "term_in"])
@pytest.mark.parametrize("rows", ["dense", "rows4"])
@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_face_normal_loss_op(recipe, rows, with_term, mesh_ops):
    vr, faces = mesh_ops["pack"]["template_verts"], _faces()
    pred, gt = _recipe(*RECIPES[recipe])
    ref64, ref32, _ = _references(pred, gt, vr, faces, MIN_C_OP)
    w, term = 0.6, (3.5 if with_term else None)
    val, total, g, pad, gterm = _device(pred, gt, vr, faces, w, rows, term)
    assert np.isfinite(g).all()
    _judge("normal_op[%s,%s,%s]" % (recipe, rows, "term" if with_term else "alone"), val, g, ref64, ref32, w)
    want = (term or 0.0) + w * val                                   # the device's own value: the sum is one fp32 fma
    assert abs(total - want) <= 2.0 ** -23 * abs(want), (total, want)
    if with_term:
        assert gterm == 1.0
    if rows == "rows4":
        assert float(np.abs(pad).max()) == 0.0


# ---- 2. synthetic small meshes -------------------------------------------------------------------------------------------

def _fan_mesh():
    """52 vertices: a fan of 40 faces around vertex 0 (rim 1..41), three separate triangles 42-44 / 45-47 / 48-50 that the
    tests make degenerate, and vertex 51 in no face.  Exact (dyadic) coordinates, verts_ref = 0."""
    rng = np.random.default_rng(0)
    nv = 52
    x = np.round(rng.standard_normal((1, nv, 3)) * 64) / 64
    ang = 2 * np.pi * np.arange(41) / 41
    x[0, 1:42, 0], x[0, 1:42, 1] = np.round(np.cos(ang) * 256) / 256, np.round(np.sin(ang) * 256) / 256
    x[0, 1:42, 2] = np.round(0.3 * rng.standard_normal(41) * 64) / 64
    x[0, 0] = (0.0, 0.0, 0.5)
    faces = np.array([[0, i, i + 1] for i in range(1, 41)] + [[42, 43, 44], [45, 46, 47], [48, 49, 50]])
    y = x + np.round(0.05 * rng.standard_normal(x.shape) * 1024) / 1024
    return x, y, faces


def test_degenerate_faces_fan_and_unused_vertex():
    import normal_loss_reference as R
    zero = np.zeros((3, 3))
    tri = np.array([[0, 1, 2]])
    good = np.array([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0.25]]])
    coincident = np.array([[[0.5, 1, 2], [0.5, 1, 2], [3, 1, 0]]])
    sliver = np.array([[[0.0, 0, 0], [1, 1, 1], [2, 2, 2]]])
    for name, p, g in (("coincident in pred", coincident, good), ("sliver in pred", sliver, good),
                       ("coincident in gt", good, coincident), ("sliver in gt", good, sliver), ("both", sliver, coincident)):
        val, total, grad, _, _ = _device(p, g, zero, tri, w=2.0)
        assert val == 1.0 and total == 2.0, (name, val, total)       # F = 1: the degenerate face's term is exactly 1
        assert not grad.any(), (name, grad)
    # the fan mesh with the three separate triangles degenerate: coincident + sliver in pred, coincident in gt
    x, y, faces = _fan_mesh()
    nv, F = x.shape[1], len(faces)
    x[0, 43] = x[0, 42]
    x[0, 45], x[0, 46], x[0, 47] = (0, 0, 0), (0.5, 0.25, 1), (1, 0.5, 2)
    y[0, 49] = y[0, 50]
    ref = np.zeros((nv, 3))
    v64, g64, c64 = R.evaluate(x, y, ref, faces, torch.float64)
    v32, g32, c32 = R.evaluate(x, y, ref, faces, torch.float32)
    assert (c64[0, 40:] == 0).all() and np.abs(c64[0, :40]).min() >= MIN_C_OP and np.array_equal(np.sign(c64), np.sign(c32))
    val, total, grad, _, _ = _device(x, y, ref, faces)
    assert np.isfinite([val, total]).all() and np.isfinite(grad).all()
    assert not grad[0, 42:].any()                                    # degenerate faces and the unused vertex: exactly 0
    assert np.abs(grad[0, 0]).max() > 0                              # the fan vertex, 40 incident faces
    _judge("normal_op[fan+degenerate]", val, grad, (v64, g64), (v32, g32))
    assert val >= 3.0 / F                                            # the three terms of exactly 1 show in the mean


def test_pred_equal_gt(mesh_ops):
    """pred == gt: fp64 gives 0; in fp32 n.n is 1 only to a few roundings, so a term may be slightly negative -- no clamp."""
    from parity_bar import check
    import normal_loss_reference as R
    vr, faces = mesh_ops["pack"]["template_verts"], _faces()
    pred, _ = _recipe(13, 2, 1.0, 0.2)
    vr32 = np.asarray(vr, dtype=np.float32)
    v64, _, _ = R.evaluate(pred, pred, vr32.astype(np.float64), faces, torch.float64)
    v32, _, _ = R.evaluate(pred, pred, vr32, faces, torch.float32)
    assert abs(v64) < 1e-15
    val, total, grad, _, _ = _device(pred, pred, vr, faces)
    print("pred == gt: device value %.3e, fp32 restatement %.3e" % (val, v32))
    check("normal_op[pred==gt]", "normal value (abs)", abs(val - v64), abs(v32 - v64))
    assert np.isfinite(grad).all()


# ---- 3. orientation ------------------------------------------------------------------------------------------------------

def test_winding_does_not_matter(mesh_ops):
    vr, faces = mesh_ops["pack"]["template_verts"], _faces()
    pred, gt = _recipe(13, 2, 1.0, 0.2)
    ref64, _, _ = _references(pred, gt, vr, faces, MIN_C_OP)
    flipped = np.ascontiguousarray(faces[:, [0, 2, 1]])
    ref64f, ref32f, _ = _references(pred, gt, vr, flipped, MIN_C_OP)
    assert abs(ref64f[0] - ref64[0]) < 1e-14 and rel_l2(ref64f[1], ref64[1]) < 1e-12      # |c| does not see the winding
    val, _, g, _, _ = _device(pred, gt, vr, flipped)
    _judge("normal_op[flipped winding]", val, g, ref64, ref32f)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------

def test_two_calls_same_bits(mesh_ops):
    from cape_amd import ops
    dev = torch.device("cuda:0")
    vr, faces = mesh_ops["pack"]["template_verts"], _faces()
    pred, gt = _recipe(27, 16, 1.0, 0.2)
    tabs = _tables(faces, V, dev)
    hv = torch.tensor(vr, dtype=torch.float32, device=dev)
    hg = torch.tensor(gt, dtype=torch.float32, device=dev)
    term = torch.tensor(0.37, dtype=torch.float32, device=dev)
    runs = []
    for _ in range(2):
        hp = torch.tensor(pred, dtype=torch.float32, device=dev, requires_grad=True)
        total, parts = ops.FaceNormalLossFn.apply(hp, hg, hv, *tabs, 0.8, term)
        total.backward()
        torch.cuda.synchronize()
        runs.append((parts.clone(), total.detach().clone(), hp.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with torch.no_grad():                                            # value only (dpred == NULL): the same value bits
        total, parts = ops.FaceNormalLossFn.apply(torch.tensor(pred, dtype=torch.float32, device=dev), hg, hv, *tabs, 0.8, term)
    assert torch.equal(parts, runs[0][0]) and torch.equal(total, runs[0][1])


# ---- 5. model level ------------------------------------------------------------------------------------------------------

LAMBDA = 0.5


def _build_normal(cfg, mesh_ops, N, overrides=None, lam=LAMBDA, **model_kw):
    """test_gpu_model._build with lambda_normal on the model; the twin knows nothing of the term (it is added on top)."""
    import test_gpu_model as T
    from cape_amd.models import CAPE
    P, twin = T._twin(cfg, mesh_ops, N, overrides)
    m = mesh_ops
    model = CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], p=m["p"], lambda_normal=lam, faces=_faces(),
                 **dict(P, **model_kw))
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='train')
    return P, twin, model


def _gt_near_prediction(twin, inputs, rel_noise, seed=21):
    """Ground truth = the twin's float32-rounded prediction plus noise of ``rel_noise`` x the prediction's spread (the
    generator's forward does not read gt), so that the cosines stay away from 0."""
    import test_gpu_model as T
    x, gt, xd, cond, cond_d, clo, clo_d, eps = inputs
    xh = T._run_twin(twin, x, gt, xd, cond, cond_d, clo, clo_d, eps)[0].detach().numpy()
    rng = np.random.default_rng(seed)
    gt2 = xh.astype(np.float32).astype(np.float64) + rel_noise * xh.std() * rng.standard_normal(xh.shape)
    return (x, gt2.astype(np.float32).astype(np.float64), xd, cond, cond_d, clo, clo_d, eps)


def _add_normal(twin, ls, xh, gt, vr, lam=LAMBDA):
    """The twin's losses with the normal term on top: loss_g + lambda_normal * normal(x_hat, gt), in the twin's dtype."""
    import normal_loss_reference as R
    dt = xh.dtype
    vr_t = torch.as_tensor(np.asarray(vr, dtype=np.float32), dtype=dt)
    c = R.face_cosines(xh, torch.as_tensor(gt, dtype=dt), vr_t, _faces())
    out = dict(ls)
    out['normal'] = (1 - c.abs()).mean()
    out['loss_g'] = ls['loss_g'] + lam * out['normal']
    return out, c.detach().double().numpy()


def _model_parity(cfg, overrides, mesh_ops, tmp_path, mask):
    import test_gpu_model as T
    import test_gpu_loss_mask as LM
    from cape_amd import ops
    from parity_bar import check
    N = 2
    kw = dict(loss_mask='binary', project_dir=LM._project(tmp_path)) if mask else {}
    P, twin, model = _build_normal(cfg, mesh_ops, N, overrides, **kw)
    vr = mesh_ops["pack"]["template_verts"]
    inputs = _gt_near_prediction(twin, T._inputs(N, P["nz"]), 0.005)
    x, gt, xd, cond, cond_d, clo, clo_d, eps = inputs
    both = (lambda tw, ls, xh, sg=None: _add_normal(tw, LM._reweight(tw, ls, xh, gt, sg) if mask else ls, xh, gt, vr))
    xh, zm, zl, d_real, d_fake, ls = T._run_twin(twin, *inputs)
    ls, c64 = both(twin, ls, xh)
    assert np.abs(c64).min() >= MIN_C_MODEL, "input condition: fp64 min |c| = %.3g" % np.abs(c64).min()
    model.load_variables(twin.vs.vars)
    dev = model.device
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    ops.ACT_TRACE, ops.L1_SIGN_TRACE, ops.LAUNCH_LOG = [], [], []
    try:
        out = model.forward_losses(t(x), t(cond), t(clo), t(gt), t(xd), t(cond_d), t(clo_d), eps=t(eps))
        signs, l1, names = list(ops.ACT_TRACE), list(ops.L1_SIGN_TRACE), [r[0] for r in ops.LAUNCH_LOG]
    finally:
        ops.ACT_TRACE = ops.L1_SIGN_TRACE = ops.LAUNCH_LOG = None
    assert names.count("face_normal_loss") == 1
    l1_sign = l1[0].numpy() if l1 else None
    tag = "normal_model[%s%s%s,N=%d]" % (cfg, "" if not overrides else "+" + ",".join(sorted(overrides)), "+mask" if mask else "", N)
    assert float(ls['normal']) > 1e-4                        # the term is in effect
    for k in ('recon', 'latent', 'edge', 'normal', 'gan_g', 'gan_d', 'loss_g', 'loss_d'):
        print("%s %s: device %.8g, fp64 twin %.8g" % (tag, k, float(out[k]), float(ls[k])))
        assert abs(float(out[k]) - float(ls[k])) < 1e-4 * max(abs(float(ls[k])), 1e-3), (k, float(out[k]), float(ls[k]))

    P32, twin32 = T._twin(cfg, mesh_ops, N, overrides, tdtype=torch.float32)
    xh32, _, _, _, _, ls32 = T._run_twin(twin32, *inputs, signs=signs, l1_sign=l1_sign)
    ls32, c32 = both(twin32, ls32, xh32, l1_sign)
    xhm, _, _, _, _, lsm = T._run_twin(twin, *inputs, signs=signs, l1_sign=l1_sign)
    lsm, cm = both(twin, lsm, xhm, l1_sign)
    assert np.abs(cm).min() >= MIN_C_MODEL and np.array_equal(np.sign(cm), np.sign(c32)), "input condition on the twins"
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
    for names_, tgr, hgr, fgr in ((g_names, tg, hg, fg), (d_names, td, hd, fd)):
        for n, a, b, c in zip(names_, tgr, hgr, fgr):
            if a is None:
                assert b is None or float(b.abs().max()) == 0.0, n
                continue
            a64, b64, c64_ = a.numpy(), b.cpu().numpy().astype(np.float64), c.numpy().astype(np.float64)
            e2, r2, f2 = ((b64 - a64) ** 2).sum(), (a64 ** 2).sum(), ((c64_ - a64) ** 2).sum()
            rows.append((n, np.sqrt(e2 / max(r2, 1e-300)), r2, np.sqrt(f2 / max(r2, 1e-300))))
            num += e2
            den += r2
            num32 += f2
    gl, gl32 = np.sqrt(num / den), np.sqrt(num32 / den)
    judged = [r for r in rows if r[2] > 1e-16 * den]
    print("%s gradients: whole bucket rel L2 %.3g [fp32 twin %.3g]; worst variable %.3g [fp32 twin's worst %.3g]"
          % (tag, gl, gl32, max(r[1] for r in judged), max(r[3] for r in judged)))
    # the absolute bar in addition only where the float32 twin's own error leaves room for it
    check(tag, "gradient, whole bucket (rel L2)", gl, gl32, T.GRAD_TOL if gl32 < T.GRAD_TOL / 4 else None)
    for n, e, r2, e32 in judged:
        check(tag, "gradient of %s (rel L2)" % n, e, e32, T.GRAD_TOL if e32 < T.GRAD_TOL / 4 else None)


@pytest.mark.parametrize("cfg,overrides,mask", [("affine_nz64", None, False), ("cmr_nz18", dict(loss='huber'), False),
                                                ("affine_nz64", None, True)],
                         ids=["affine_nz64_l1", "cmr_nz18_huber", "affine_nz64_l1_mask"])
def test_model_with_normal_loss(cfg, overrides, mask, mesh_ops, tmp_path):
    """Forward losses incl. 'normal' against the fp64 twin + lambda_normal * normal64(x_hat, gt) at the 1e-4 relative bar;
    every variable's gradient and the whole bucket against the float32 twin + float32 restatement (factor 4)."""
    _model_parity(cfg, overrides, mesh_ops, tmp_path, mask)


# ---- 6. captured step ----------------------------------------------------------------------------------------------------

def _fwd_bwd_names(model, batch):
    from cape_amd import ops
    from cape_amd.runtime import GraphedTrainStep
    r = GraphedTrainStep(model, with_gan=True, use_graph=False)
    r.load_batch(**batch)
    ops.LAUNCH_LOG = []
    try:
        r._fwd_bwd()
        torch.cuda.synchronize()
        return [e[0] for e in ops.LAUNCH_LOG], r
    finally:
        ops.LAUNCH_LOG = None


def test_graphed_step_with_normal_loss(mesh_ops):
    """The captured adversarial step with the option on: bit-identical optimiser state over repeated replays from the same
    start, the replayed 'normal' is the eager one, face_normal_loss once per step; with lambda_normal = 0 none at all."""
    import test_gpu_model as T
    from cape_amd.runtime import GraphedTrainStep
    N = 2
    P, twin, model = _build_normal("affine_nz64", mesh_ops, N, dict(regularization=0.5, lr_warmup=False, decay_steps=1000))
    x, gt, xd, cond, cond_d, clo, clo_d, eps = T._inputs(N, P["nz"])
    batch = dict(data_g=x, cond_g=cond, cond2_g=clo, gt=gt, data_d=xd, cond_d=cond_d, cond2_d=clo_d, eps=eps)
    dev = model.device
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    runner = GraphedTrainStep(model, with_gan=True)
    runner.load_batch(**batch)
    runner.capture(preserve_state=True)
    tables = [a.data_ptr() for a in model._face_dev]
    groups = ('g', 'd')
    start = {g: {k: model._opt_state[g][k].detach().clone() for k in ('flat', 'm')} for g in groups}
    step0 = model.global_step
    runs, first = [], []
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
                first.append(float(runner.losses['normal']))
        torch.cuda.synchronize()
        runs.append({(g, k): model._opt_state[g][k].detach().clone() for g in groups for k in ('flat', 'm')})
    moved = False
    for key in runs[0]:
        assert torch.equal(runs[0][key], runs[1][key]), key
        moved = moved or not torch.equal(runs[0][key], start[key[0]][key[1]])
    assert moved and first[0] == first[1] and 0.0 < first[0] <= 1.0
    assert tables == [a.data_ptr() for a in model._face_dev]         # the tables the capture points at are still the model's
    with torch.no_grad():
        for g in groups:
            for k in ('flat', 'm'):
                model._opt_state[g][k].copy_(start[g][k])
        eager = float(model.forward_losses(t(x), t(cond), t(clo), t(gt), t(xd), t(cond_d), t(clo_d), eps=t(eps),
                                           reg_via_bucket=True)['normal'])
    assert abs(first[0] - eager) <= 1e-6 * abs(eager), (first[0], eager)
    names, _ = _fwd_bwd_names(model, batch)
    assert names.count("face_normal_loss") == 1 and names.count("recon_edge_loss") == 1, names

    P0, _, model0 = T._build("affine_nz64", mesh_ops, N, dict(regularization=0.5, lr_warmup=False, decay_steps=1000))
    names0, r0 = _fwd_bwd_names(model0, batch)
    assert "face_normal_loss" not in names0 and len(names0) == len(names) - 1
    assert model0.lambda_normal == 0.0 and model0._faces is None and not hasattr(model0, '_face_dev')
    with torch.no_grad():
        assert 'normal' not in r0.losses and 'normal' not in model0.loss_terms(t(x), t(gt), t(eps), t(eps))


# ---- 7. drivers ----------------------------------------------------------------------------------------------------------

def test_predict_and_evaluate_keep_their_tuples(mesh_ops):
    import test_gpu_model as T
    N = 2
    P, twin, model = _build_normal("affine_nz64", mesh_ops, N)
    x, gt, xd, cond, cond_d, clo, clo_d, eps = T._inputs(5, P["nz"], seed=4)      # 5 = 2 + 2 + 1 (padded last batch)
    torch.manual_seed(7)
    res = model.predict(x, cond, clo, labels=gt, sess=model)
    assert len(res) == 4
    preds, lr_, ll_, le_ = res
    assert preds.shape == (5, V, 3) and np.isfinite(preds).all() and np.isfinite([lr_, ll_, le_]).all()
    assert model.predict(x, cond, clo, sess=model).shape == (5, V, 3)
    torch.manual_seed(7)
    res = model.evaluate(x, cond, clo, gt, model)
    assert len(res) == 4 and res[0].startswith('recon loss:')
    assert abs(res[1] - lr_) <= 1e-6 * lr_ and abs(res[3] - le_) <= 1e-6 * le_


def test_fit_with_normal_loss(mesh_ops, tmp_path):
    import types
    from test_gpu_dropin_api import _args_dict, _params
    from cape_amd import models
    m = mesh_ops
    ad = _args_dict()
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
    model = models.CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], project_dir=str(tmp_path),
                        lambda_normal=1.0, faces=_faces(), **params)
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='train')
    res = model.fit(data)
    assert len(res) == 2
    loss, t_step = res
    assert len(loss) >= 1 and np.isfinite(loss).all() and t_step > 0
    assert os.path.exists(os.path.join(str(tmp_path), 'checkpoints', params['name']))


def test_bf16_storage_with_normal_loss(mesh_ops):
    """act_dtype='bf16' with the option on: the losses see fp32 and take the same kernel; forward within test_gpu_bf16's 2e-2
    bar of the fp64 twin + normal term, generator gradients within its global 3e-2 bar."""
    import test_gpu_model as T
    from cape_amd import ops
    N = 2
    P, twin, model = _build_normal("affine_nz64", mesh_ops, N, dict(act_dtype='bf16'))
    vr = mesh_ops["pack"]["template_verts"]
    inputs = _gt_near_prediction(twin, T._inputs(N, P["nz"]), 0.3)
    x, gt, xd, cond, cond_d, clo, clo_d, eps = inputs
    xh, zm, zl, d_real, d_fake, ls = T._run_twin(twin, *inputs)
    ls, _ = _add_normal(twin, ls, xh, gt, vr)
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
    assert names.count("face_normal_loss") == 1
    for k in ('recon', 'latent', 'edge', 'normal', 'gan_g', 'gan_d', 'loss_g', 'loss_d'):
        print("bf16 %s: device %.6g, fp64 twin %.6g" % (k, float(out[k]), float(ls[k])))
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
    print("bf16 storage with lambda_normal: generator gradients, global relative L2 error %.2e" % gl)
    assert gl < 3e-2, gl
