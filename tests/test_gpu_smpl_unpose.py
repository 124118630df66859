"""Unposing on the device (cape_amd.smpl.SMPL.unpose / undress, CAPE.encode_posed; cape_smpl_unpose_joints /
cape_smpl_unpose_skin / cape_smpl_undress) against the float64 numpy oracle of tests/smpl_unpose_reference.py, under
tests/parity_bar.py's bar (at most 4x the error of the float32 restatement on the same float32 inputs) and, where the
conditioning is capped, below 1e-5 of the body's extent; seeded synthetic SMPL-format models (tests/smpl_synth.py)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity_bar                       # noqa: E402
import smpl_reference as ref            # noqa: E402
import smpl_synth as synth              # noqa: E402
import smpl_unpose_reference as uref    # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
POSE_SCALE = {"small": 0.3, "smpl_like": 0.3, "j52": 0.2}       # j52 at 0.3 reaches cond(I + QL) = 191
_MODELS, _CASES = {}, {}

f32 = lambda a: None if a is None else np.asarray(a, np.float32)
dev = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


def _model(which):
    if which not in _MODELS:
        from cape_amd import smpl
        m = getattr(synth, which)()
        _MODELS[which] = (m, smpl.SMPL(m))
    return _MODELS[which]


def _case(which, N, shape):
    """Inputs and both numpy results, computed once per (model, N, with / without betas and transl) and left unchanged."""
    key = (which, N, shape)
    if key not in _CASES:
        m, _ = _model(which)
        V, J = m["v_template"].shape[0], len(ref.parents_of(m))
        rng = np.random.default_rng(100 + N)
        pose = POSE_SCALE[which] * rng.standard_normal((N, 3 * J))
        pose[0] = 0
        T = m["v_template"][None] + 0.01 * rng.standard_normal((N, V, 3))
        betas, transl = 0.8 * rng.standard_normal((N, 10)), 0.3 * rng.standard_normal((N, 3))
        pose, betas, transl = f32(pose), f32(betas) if shape else None, f32(transl) if shape else None
        P = f32(ref.forward(m, T, pose, betas, transl)[0])
        o64 = uref.unpose(m, P, pose, betas, transl, full=True)
        r32 = uref.unpose(m, P, pose, betas, transl, dtype=np.float32)
        _CASES[key] = dict(T=T, P=P, pose=pose, betas=betas, transl=transl, o64=o64, r32=r32,
                           extent=float(np.ptp(o64["rest"].reshape(-1, 3), 0).max()))
    return _CASES[key]


@pytest.mark.parametrize("N", [1, 3, 17])
@pytest.mark.parametrize("which", ["small", "smpl_like", "j52"])
def test_unpose_matches_the_oracle(which, N):
    _, model = _model(which)
    for shape in (True, False):
        c = _case(which, N, shape)
        o64 = c["o64"]
        # a badly conditioned draw must not hide behind the relative bar
        assert o64["cond_system"].max() <= 100 and o64["cond_mrot"].max() <= 20, (o64["cond_system"].max(), o64["cond_mrot"].max())
        assert _err(o64["rest"], c["T"]) < 1e-5 * c["extent"]                    # the inputs are the rounded forward of T
        rest, joints = model.unpose(dev(c["P"]), dev(c["pose"]), dev(c["betas"]), dev(c["transl"]))
        torch.cuda.synchronize()
        name = "unpose_%s_N%d_%s" % (which, N, "shape_transl" if shape else "plain")
        e_v, e_j = _err(rest.cpu().numpy(), o64["rest"]), _err(joints.cpu().numpy(), o64["rest_joints"])
        r_v, r_j = _err(c["r32"][0], o64["rest"]), _err(c["r32"][1], o64["rest_joints"])
        print("%s: rest %.3e (fp32 %.3e), rest joints %.3e (fp32 %.3e), cond %.1f / %.1f" %
              (name, e_v, r_v, e_j, r_j, o64["cond_system"].max(), o64["cond_mrot"].max()))
        parity_bar.check(name, "rest", e_v, r_v, also_below=1e-5 * c["extent"])
        parity_bar.check(name, "rest_joints", e_j, r_j, also_below=1e-5 * c["extent"])


def test_unpose_demo_poses():
    """Joint angles up to 2.4 rad on the synthetic weights: cond(Mrot) about 2e3, the float32 restatement itself at 1e-4.  The
    parity bar only; the margin is recorded."""
    m, model = _model("smpl_like")
    pose = f32(np.load(os.path.join(GOLD, "demo_pose_params.npz"))["pose"])
    rng = np.random.default_rng(8)
    T = m["v_template"][None] + 0.01 * rng.standard_normal((len(pose), 6890, 3))
    P = f32(ref.forward(m, T, pose)[0])
    o64 = uref.unpose(m, P, pose, full=True)
    r32 = uref.unpose(m, P, pose, dtype=np.float32)
    rest, joints = model.unpose(dev(P), dev(pose))
    torch.cuda.synchronize()
    e_v, e_j = _err(rest.cpu().numpy(), o64["rest"]), _err(joints.cpu().numpy(), o64["rest_joints"])
    r_v, r_j = _err(r32[0], o64["rest"]), _err(r32[1], o64["rest_joints"])
    print("unpose demo poses: rest %.3e (fp32 %.3e, ratio %.2f), rest joints %.3e (fp32 %.3e, ratio %.2f), cond %.1f / %.1f" %
          (e_v, r_v, e_v / r_v, e_j, r_j, e_j / r_j, o64["cond_system"].max(), o64["cond_mrot"].max()))
    parity_bar.check("unpose_demo_poses", "rest", e_v, r_v)
    parity_bar.check("unpose_demo_poses", "rest_joints", e_j, r_j)


@pytest.mark.parametrize("per_sample", [False, True])
def test_explicit_joints_forward_and_its_inverse(per_sample):
    m, model = _model("smpl_like")
    c = _case("smpl_like", 3, True)
    rng = np.random.default_rng(21)
    JF = f32(m["v_template"][None] + (0.005 * rng.standard_normal((3, 6890, 3)) if per_sample else 0))
    T32 = f32(c["T"])
    args = (c["pose"], c["betas"], c["transl"])
    v64, j64 = uref.forward(m, T32, *args, joints_from=JF)
    v32, j32 = uref.forward(m, T32, *args, joints_from=JF, dtype=np.float32)
    dargs = tuple(dev(a) for a in args)
    vo, jo = model.forward(dev(T32), *dargs, joints_from=dev(JF))
    extent = c["extent"]
    tag = "explicit_joints_%s" % ("per_sample" if per_sample else "one_body")
    parity_bar.check(tag, "vertices", _err(vo.cpu().numpy(), v64), _err(v32, v64), also_below=1e-5 * extent)
    parity_bar.check(tag, "joints", _err(jo.cpu().numpy(), j64), _err(j32, j64), also_below=1e-5 * extent)
    # the inverse with the same joints, on the rounded posed vertices
    P = f32(v64)
    t64, n64 = uref.unpose(m, P, *args, joints_from=JF)
    t32, n32 = uref.unpose(m, P, *args, joints_from=JF, dtype=np.float32)
    assert _err(t64, T32) < 1e-5 * extent
    rest, rj = model.unpose(dev(P), *dargs, joints_from=dev(JF))
    parity_bar.check(tag, "rest", _err(rest.cpu().numpy(), t64), _err(t32, t64), also_below=1e-5 * extent)
    parity_bar.check(tag, "rest_joints", _err(rj.cpu().numpy(), n64), _err(n32, n64), also_below=1e-5 * extent)
    # joints_from=None is the forward as it was: the same bits as a plain call
    a = model.forward(dev(T32), *dargs, joints_from=None)
    b = model.forward(dev(T32), *dargs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], vo)
    with pytest.raises(NotImplementedError):
        model.forward_diff(dev(T32), *dargs, joints_from=dev(JF))


@pytest.mark.parametrize("which,N", [("small", 3), ("smpl_like", 17), ("j52", 17)])
def test_det_min_matches_the_oracle(which, N):
    _, model = _model(which)
    c = _case(which, N, True)
    args = [dev(c[k]) for k in ("P", "pose", "betas", "transl")]
    d64 = c["o64"]["det_min"]
    d32 = uref.unpose(_model(which)[0], c["P"], c["pose"], c["betas"], c["transl"], dtype=np.float32, full=True)["det_min"]
    det = torch.full((N,), -1.0, device="cuda")
    model.unpose(*args, det_min=det)
    parity_bar.check("unpose_det_min_%s_N%d" % (which, N), "det_min", _err(det.cpu().numpy(), d64), _err(d32, d64))
    assert det[0].item() == pytest.approx(1.0, abs=1e-6)             # row 0: zero pose
    # explicit joints: the same rotations, the same minimum
    det2 = torch.full((N,), -1.0, device="cuda")
    model.unpose(*args, joints_from=dev(_model(which)[0]["v_template"][None]), det_min=det2)
    parity_bar.check("unpose_det_min_%s_N%d_explicit" % (which, N), "det_min", _err(det2.cpu().numpy(), d64), _err(d32, d64))


def test_unpose_is_deterministic_and_graph_capturable():
    _, model = _model("smpl_like")
    c = _case("smpl_like", 17, True)
    N = 17
    P, pose, betas, transl = (dev(c[k]) for k in ("P", "pose", "betas", "transl"))
    da, db = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    a = [x.clone() for x in model.unpose(P, pose, betas, transl, det_min=da)]
    b = [x.clone() for x in model.unpose(P, pose, betas, transl, det_min=db)]
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(da, db)
    out = (torch.zeros(N, 6890, 3, device="cuda"), torch.zeros(N, 24, 3, device="cuda"))
    ws, det = model.unpose_workspace(N), torch.zeros(N, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.unpose(P, pose, betas, transl, out=out, det_min=det, workspace=ws)            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    out[0].zero_()
    out[1].zero_()
    det.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        model.unpose(P, pose, betas, transl, out=out, det_min=det, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], a[0]) and torch.equal(out[1], a[1]) and torch.equal(det, da)
    with pytest.raises(RuntimeError):
        model.unpose(P.clone().requires_grad_(True), pose)
    with pytest.raises(ValueError):
        model.unpose(P[:1], pose)                                    # no broadcast of the posed input


def test_unpose_np_round_trips_pose():
    m, model = _model("small")
    c = _case("small", 3, True)
    posed, _ = model.pose(f32(c["T"]), c["pose"], c["betas"], c["transl"])
    rest, joints = model.unpose_np(posed, c["pose"], c["betas"], c["transl"])
    assert rest.dtype == joints.dtype == np.float32 and rest.shape == (3, 37, 3) and joints.shape == (3, 5, 3)
    assert _err(rest, f32(c["T"])) < 1e-5 * c["extent"]


def _stats():
    st = np.load(os.path.join(GOLD, "trainset_stats.npz"))
    return st["mean"], st["std"], np.load(os.path.join(GOLD, "clothing_verts_idx.npy"))


def test_undress_matches_numpy_and_is_the_right_inverse_of_dress():
    from cape_amd import smpl
    mean, std, idx = _stats()
    minimal = synth.template()
    T = f32(minimal[None] + 0.02 * np.random.default_rng(5).standard_normal((5, 6890, 3)))
    mean32, std32, min32 = f32(mean), f32(std), f32(minimal)
    for ci, tag in ((idx, "clothing"), (None, "every_vertex")):
        d = smpl.undress(dev(T), mean, std, ci, minimal)
        d64 = uref.undress(T, mean, std, ci, minimal)
        d32 = uref.undress(T, mean32, std32, ci, min32, np.float32)
        parity_bar.check("smpl_undress_%s" % tag, "disp", _err(d.cpu().numpy(), d64), _err(d32, d64))
    # dress(undress(T)) = minimal + mask (T - minimal) to one rounding of the result, u |result| with u = 2^-24, plus what the
    # six roundings before the last addition carry in: at most 5 u (|T - minimal| + |mean|)
    d = smpl.undress(dev(T), mean, std, idx, minimal)
    again = smpl.dress(d, mean, std, idx, minimal).cpu().numpy().astype(np.float64)
    mask = np.zeros((6890, 1))
    mask[idx] = 1
    a = T.astype(np.float64) - min32
    want = min32 + mask * a
    tol = 2.0 ** -24 * (np.abs(want) + 5 * (np.abs(a) + np.abs(mean32)))
    assert (np.abs(again - want) <= tol).all(), float((np.abs(again - want) / tol).max())


# ---- CAPE.encode_posed ------------------------------------------------------------------------------------------------
SIZE = 5            # batch 4: one full batch and a padded batch of one row


@pytest.fixture(scope="module")
def setup(mesh_ops):
    from cape_amd import smpl
    from test_gpu_smpl import _cape_model
    model = _cape_model(mesh_ops, batch_size=4)
    mean, std, idx = _stats()
    m = synth.smpl_like(seed=6)
    rng = np.random.default_rng(60)
    pose = f32(0.3 * rng.standard_normal((SIZE, 72)))
    pose[0] = 0
    return dict(model=model, m=m, body=smpl.SMPL(m), mean=mean, std=std, idx=idx, pose=pose, rng=rng,
                cond=0.5 * rng.standard_normal((SIZE, 126)), clo=np.eye(4)[np.arange(SIZE) % 4])


def test_encode_posed_is_encode_on_the_unposed_displacements(setup):
    s = setup
    model, m = s["model"], s["m"]
    rng = np.random.default_rng(61)
    minimal = np.asarray(model.verts_ref, np.float64)
    T = minimal[None] + 0.01 * rng.standard_normal((SIZE, 6890, 3))
    betas, transl = f32(0.8 * rng.standard_normal((SIZE, 10))), f32(0.3 * rng.standard_normal((SIZE, 3)))
    P = f32(ref.forward(m, T, s["pose"], betas, transl)[0])
    zm, zv, y, y2, disp = model.encode_posed(P, s["pose"], s["cond"], s["clo"], s["body"], s["mean"], s["std"], s["idx"],
                                             transl=transl, betas=betas, return_disp=True)
    assert disp.shape == (SIZE, 6890, 3) and disp.dtype == np.float32 and zm.shape == (SIZE, model.nz)
    # same encoder, same input, same padding: the same bits
    em, ev, ey, ey2 = model.encode(disp, s["cond"], s["clo"])
    assert np.array_equal(zm, em) and np.array_equal(zv, ev) and np.array_equal(y, ey) and np.array_equal(y2, ey2)
    four = model.encode_posed(P, s["pose"], s["cond"], s["clo"], s["body"], s["mean"], s["std"], s["idx"], transl=transl, betas=betas)
    assert len(four) == 4 and np.array_equal(four[0], zm) and np.array_equal(four[1], zv)
    # the displacements against float64 unpose + undress on the same float32 inputs
    mean32, std32, min32 = f32(s["mean"]), f32(s["std"]), f32(minimal)
    d64 = uref.undress(uref.unpose(m, P, s["pose"], betas, transl)[0], s["mean"], s["std"], s["idx"], minimal)
    d32 = uref.undress(uref.unpose(m, P, s["pose"], betas, transl, dtype=np.float32)[0], mean32, std32, s["idx"], min32, np.float32)
    print("encode_posed disp: hip %.3e, fp32 %.3e" % (_err(disp, d64), _err(d32, d64)))
    parity_bar.check("encode_posed", "disp", _err(disp, d64), _err(d32, d64))
    # explicit joints and one pose row for every sample run through the same loop
    one = model.encode_posed(P, s["pose"][:1], s["cond"], s["clo"], s["body"], s["mean"], s["std"], s["idx"],
                             joints_from=minimal[None], return_disp=True)
    assert one[4].shape == (SIZE, 6890, 3) and np.isfinite(one[0]).all()
    with pytest.raises(ValueError):
        model.encode_posed(P, s["pose"][:2], s["cond"], s["clo"], s["body"], s["mean"], s["std"], s["idx"])


def test_decode_posed_then_encode_posed_returns_the_decoders_displacements(setup):
    s = setup
    model, m, idx = s["model"], s["m"], s["idx"]
    rng = np.random.default_rng(62)
    z = rng.standard_normal((SIZE, model.nz + model.nz_cond + model.nz_cond2))
    ce, ce2 = rng.standard_normal((SIZE, model.nz_cond)), rng.standard_normal((SIZE, model.nz_cond2))
    posed, _ = model.decode_posed(z, ce, ce2, s["pose"], s["body"], s["mean"], s["std"], idx)
    x = model.decode(z, ce, ce2)
    disp = model.encode_posed(posed, s["pose"], s["cond"], s["clo"], s["body"], s["mean"], s["std"], idx, return_disp=True)[4]
    # the float32 oracle's own round trip from the same decoder output sets the bar
    mean32, std32, min32 = f32(s["mean"]), f32(s["std"]), f32(model.verts_ref)
    T32 = ref.dress(x, mean32, std32, idx, min32, np.float32)
    P32 = ref.forward(m, T32, s["pose"], dtype=np.float32)[0]
    back32 = uref.undress(uref.unpose(m, P32, s["pose"], dtype=np.float32)[0], mean32, std32, idx, min32, np.float32)
    e_hip, e_f32 = _err(disp[:, idx], x[:, idx].astype(np.float64)), _err(back32[:, idx], x[:, idx].astype(np.float64))
    print("decode_posed -> encode_posed: hip %.3e, fp32 oracle round trip %.3e (normalised units)" % (e_hip, e_f32))
    parity_bar.check("encode_posed_round_trip", "disp", e_hip, e_f32)
