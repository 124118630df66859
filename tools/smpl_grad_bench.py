"""Differentiable SMPL posing throughput: forward + backward of cape_amd.smpl.SMPL.forward_diff for N in {1, 16, 256} meshes on
the 6890-vertex template with a seeded synthetic SMPL-format model (tests/smpl_synth.py), one JSON line per N with two
implementations timed in the same run, device events, median of --calls after warm-up:
  fused   forward_diff (cape_smpl_joints + cape_smpl_skin) and its backward (cape_smpl_joints again for coef / G,
          cape_smpl_skin_bwd, cape_smpl_joints_bwd, cape_smpl_jreg_bwd), gradients to rest body, pose, betas and translation;
          the backward's kernels are also timed one by one
  torch   torch autograd on the op-by-op float32 twin of the forward (tests/smpl_torch_twin.py) on the same GPU
Algorithmic bytes of the backward: the blend basis read once per sample tile, the skinning weights (ELL) twice, the rest
vertices and gV in, dT out, q out and in again, and the workgroup partials out and in.
A last line times one step of CAPE.fit_posed (decoder forward + data gradient, dress, posing, loss, Adam) at batch 16 on the
affine nz64 model.  Usage: python tools/smpl_grad_bench.py [--calls 50] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time_events(fn, calls, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def _phases(model, T, pose, betas, transl, gV, gJ, calls):
    """The backward's kernels one by one, on the arguments SMPL._backward hands them (per-sample rest bodies)."""
    from cape_amd import _lib
    from cape_amd.smpl import _p, _stream
    lib, d = _lib.lib, model._dev
    N, J, V, B = pose.shape[0], model.J, model.V, betas.shape[1]
    K = B + 9 * (J - 1)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=T.device)
    coef, G = model._joints(T, pose, betas, transl, None)
    plan = (C.c_int32 * 3)()
    _lib.check(lib.cape_smpl_skin_bwd_plan(K, J, V, N, plan), "plan")
    ws, q, dJn, dT = new(N * plan[1] * plan[2]), new(N, V, 3), new(N, J, 3), new(N, V, 3)
    dpose, dbetas, dtransl = new(N, 3 * J), new(N, B), new(N, 3)
    skin = lambda: lib.cape_smpl_skin_bwd(_p(T), 3 * V, model._basis(B), K, _p(coef), _p(G), _p(d.ell_j), _p(d.ell_w), model.ell_width,
                                          _p(gV), 3 * V, J, V, N, 1, _p(q), 3 * V, _p(ws), 4 * ws.numel(), _stream())
    joints = lambda: lib.cape_smpl_joints_bwd(_p(T), 3 * V, _p(d.rowptr), _p(d.colidx), _p(d.vals), _p(pose), _p(betas), B,
                                              _p(d.jshapedirs), model._parents_c, J, V, N, _p(gJ), _p(ws), int(plan[1]), 1, _p(dpose),
                                              _p(dbetas), _p(dtransl), _p(dJn), _stream())
    jreg = lambda: lib.cape_smpl_jreg_bwd(_p(q), 3 * V, _p(d.jt_colptr), _p(d.jt_rowidx), _p(d.jt_vals), _p(dJn), J, V, N, 0, _p(dT),
                                          3 * V, _stream())
    out = {}
    for name, fn in (("skin_bwd", skin), ("joints_bwd", joints), ("jreg_bwd", jreg)):
        assert fn() == 0, name
        out[name + "_us"] = round(_time_events(fn, calls), 2)
    out["recompute_joints_us"] = round(_time_events(lambda: model._joints(T, pose, betas, transl, None), calls), 2)
    return out, list(plan)


def _fit_step(calls):
    """One fit_posed step at batch 16: the wall time of a (steps = calls) run minus a (steps = 0) run, per step."""
    import smpl_synth as synth
    from cape_amd import smpl
    from cape_amd.configs import cape_params
    from cape_amd.load_data import load_graph_mtx
    from cape_amd.models import CAPE
    L, D, U, p, L_d, D_d, _ = load_graph_mtx(None, load_for_demo=True)
    model = CAPE(L=L, D=D, U=U, L_d=L_d, D_d=D_d, **cape_params('CAPE-affineconv_nz64_pose32_clotype32_male', p=p, batch_size=16))
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='demo')
    model.load_variables({k: v.detach().cpu().numpy() for k, v in model._vars.items()})
    m = synth.smpl_like()
    body = smpl.SMPL(m)
    gold = os.path.join(ROOT, "tests", "golden")
    st, idx = np.load(os.path.join(gold, "trainset_stats.npz")), np.load(os.path.join(gold, "clothing_verts_idx.npy"))
    rng = np.random.default_rng(0)
    n = 16
    cond, cond2 = rng.standard_normal((n, model.nz_cond)), rng.standard_normal((n, model.nz_cond2))
    pose = 0.3 * rng.standard_normal((n, 72))
    zt = np.concatenate([rng.standard_normal((n, model.nz)), cond, cond2], 1)
    target, _ = model.decode_posed(zt, cond, cond2, pose, body, st["mean"], st["std"], idx)

    def run(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.fit_posed(target, pose, cond, cond2, body, st["mean"], st["std"], idx, steps=steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    run(2)
    base = min(run(0) for _ in range(3))
    full = min(run(calls) for _ in range(3))
    return dict(tool="smpl_grad_bench", what="fit_posed step", batch=n, steps=calls, ms_per_step=round((full - base) / calls * 1e3, 3),
                ms_steps0=round(base * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import smpl_synth as synth
    import smpl_torch_twin as twin
    from cape_amd import smpl, _lib
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    m = synth.smpl_like()
    model = smpl.SMPL(m, device=dev)
    tw = twin.Twin(m, torch.float32, dev)
    J, V = model.J, model.V
    K = model.num_betas + 9 * (J - 1)
    rng = np.random.default_rng(0)
    lines = []
    for N in [int(x) for x in a.sizes.split(",")]:
        t = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
        ins = [t(m["v_template"][None] + 0.01 * rng.standard_normal((N, V, 3))), t(0.5 * rng.standard_normal((N, 3 * J))),
               t(rng.standard_normal((N, model.num_betas))), t(0.3 * rng.standard_normal((N, 3)))]
        gV, gJ = t(rng.standard_normal((N, V, 3))), t(rng.standard_normal((N, J, 3)))

        def run(forward):
            leaves = [x.detach().requires_grad_(True) for x in ins]
            v, j = forward(*leaves)
            torch.autograd.backward([v, j], [gV, gJ])
            return leaves
        us_fused = _time_events(lambda: run(model.forward_diff), a.calls)
        us_torch = _time_events(lambda: run(tw.forward), a.calls)
        with torch.no_grad():
            us_fwd = _time_events(lambda: model.forward(*ins), a.calls)
        gf, gt = run(model.forward_diff), run(tw.forward)
        diff = {k: float((x.grad - y.grad).abs().max() / y.grad.abs().max()) for k, x, y in zip(("dT", "dpose", "dbetas", "dtransl"), gf, gt)}
        phases, plan = _phases(model, *ins, gV, gJ, a.calls)
        tile, blocks, rec_len = plan
        tiles = -(-N // tile)
        ws = 4 * N * blocks * rec_len
        nbytes = tiles * 4 * 3 * K * V + 2 * model.ell_width * V * 8 + 5 * N * V * 3 * 4 + 2 * ws
        rec = dict(tool="smpl_grad_bench", N=N, V=V, J=J, K=K, tile=tile, blocks=blocks, workspace_bytes=int(ws), bwd_bytes=int(nbytes),
                   fused_fwd_bwd_us=round(us_fused, 2), fused_fwd_only_us=round(us_fwd, 2), torch_gpu_fwd_bwd_us=round(us_torch, 2),
                   speedup_vs_torch_gpu=round(us_torch / us_fused, 2), phases=phases,
                   skin_bwd_GBps=round(nbytes / phases["skin_bwd_us"] / 1e3, 1), max_norm_diff_vs_torch=diff)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if not a.no_fit:
        rec = _fit_step(a.calls)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
