"""SMPL posing throughput: N in {1, 16, 256} meshes on the 6890-vertex template with a seeded synthetic SMPL-format model
(tests/smpl_synth.py), one JSON line per N with three implementations timed in the same run:
  fused   cape_amd.smpl.SMPL.forward (cape_smpl_joints + cape_smpl_skin), device events, median of --calls after warm-up:
          eager calls (host launch cost included) and replays of one captured graph of the call (device time)
  torch   an op-by-op torch-GPU restatement of the same forward pass (below), same timing
  cpu     the reference's posture: one fp32 torch-CPU forward per mesh (demos.py:267-283 calls smplx once per mesh)
Algorithmic bytes: the blend basis read once per sample tile (cape_smpl_skin_tile samples), the skinning weights (ELL), the rest
vertices in and the posed vertices out.  Usage: python tools/smpl_bench.py [--calls 50] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_forward(t, T, pose, betas):
    """Op-by-op restatement (smplx's order) on tensors from ``_torch_arrays``."""
    N, J = pose.shape[0], t["parents"].shape[0]
    v_shaped = T + torch.einsum("vck,nk->nvc", t["shapedirs"], betas)
    Jn = torch.einsum("jv,nvc->njc", t["jreg"], v_shaped)
    r = pose.reshape(N, J, 3)
    th2 = (r * r).sum(-1, keepdim=True)
    th = th2.clamp_min(1e-12).sqrt()
    s = torch.where(th2 < 1e-6, 1 - th2 / 6, torch.sin(th) / th)
    h = torch.sin(0.5 * th) / th
    c = torch.where(th2 < 1e-6, 0.5 - th2 / 24, 2 * h * h)
    x, y, z = r.unbind(-1)
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(N, J, 3, 3)
    eye = torch.eye(3, device=T.device)
    R = eye + s[..., None] * K + c[..., None] * (r[..., :, None] * r[..., None, :] - th2[..., None] * eye)
    pf = (R[:, 1:] - eye).reshape(N, -1)
    v_posed = v_shaped + torch.einsum("vck,nk->nvc", t["posedirs"], pf)
    rel = Jn.clone()
    rel[:, 1:] = Jn[:, 1:] - Jn[:, t["parents"][1:]]
    Tm = torch.zeros(N, J, 4, 4, device=T.device)
    Tm[..., :3, :3], Tm[..., :3, 3], Tm[..., 3, 3] = R, rel, 1
    chain = [Tm[:, 0]]
    for j in range(1, J):
        chain.append(chain[int(t["parents"][j])] @ Tm[:, j])
    A = torch.stack(chain, 1)
    G = A.clone()
    G[..., :3, 3] = A[..., :3, 3] - (A[..., :3, :3] @ Jn[..., None])[..., 0]
    M = torch.einsum("vj,njab->nvab", t["weights"], G[..., :3, :])
    return (M[..., :3] @ v_posed[..., None])[..., 0] + M[..., 3], A[..., :3, 3]


def _torch_arrays(m, dev):
    import scipy.sparse as sp
    f = lambda a: torch.tensor(a.toarray() if sp.issparse(a) else np.asarray(a), dtype=torch.float32, device=dev)
    par = np.asarray(m["kintree_table"])[0].astype(np.int64)
    par[par == 4294967295] = -1
    return dict(shapedirs=f(m["shapedirs"]), posedirs=f(m["posedirs"]), jreg=f(m["J_regressor"]), weights=f(m["weights"]),
                parents=torch.tensor(par))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--cpu-meshes", type=int, default=16, help="meshes timed on the CPU path (per-mesh time x N reported)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import smpl_synth as synth
    from cape_amd import smpl, _lib
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    m = synth.smpl_like()
    model = smpl.SMPL(m, device=dev)
    tt = _torch_arrays(m, dev)
    tc = _torch_arrays(m, "cpu")
    J, V = model.J, model.V
    K = model.num_betas + 9 * (J - 1)
    tile = _lib.lib.cape_smpl_skin_tile(K, J)
    rng = np.random.default_rng(0)
    lines = []
    for N in [int(x) for x in a.sizes.split(",")]:
        T = torch.tensor(m["v_template"][None] + 0.01 * rng.standard_normal((N, V, 3)), dtype=torch.float32, device=dev)
        pose = torch.tensor(0.5 * rng.standard_normal((N, 3 * J)), dtype=torch.float32, device=dev)
        betas = torch.tensor(rng.standard_normal((N, model.num_betas)), dtype=torch.float32, device=dev)
        out = (torch.empty(N, V, 3, device=dev), torch.empty(N, J, 3, device=dev))
        with torch.no_grad():
            us_fused = _time_events(lambda: model.forward(T, pose, betas, None, out=out), a.calls)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                model.forward(T, pose, betas, None, out=out)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                model.forward(T, pose, betas, None, out=out)
            us_graph = _time_events(g.replay, a.calls)
            us_torch = _time_events(lambda: torch_forward(tt, T, pose, betas), a.calls)
            ref_v, _ = torch_forward(tt, T, pose, betas)
            dmax = float((ref_v - out[0]).abs().max())
            Tc, pc, bc = T.cpu(), pose.cpu(), betas.cpu()
            nc = min(N, a.cpu_meshes)
            t0 = time.perf_counter()
            for i in range(nc):
                torch_forward(tc, Tc[i:i + 1], pc[i:i + 1], bc[i:i + 1])
            us_cpu = (time.perf_counter() - t0) / nc * N * 1e6
        tiles = -(-N // tile)
        nbytes = tiles * 4 * 3 * K * V + model.ell_width * V * 8 + 2 * N * V * 3 * 4
        rec = dict(tool="smpl_bench", N=N, V=V, J=J, K=K, tile=tile, bytes=int(nbytes), max_abs_diff_vs_torch=dmax,
                   fused=dict(us=round(us_fused, 2), meshes_per_s=round(N / us_fused * 1e6), GBps=round(nbytes / us_fused / 1e3, 1)),
                   fused_graph=dict(us=round(us_graph, 2), meshes_per_s=round(N / us_graph * 1e6),
                                    GBps=round(nbytes / us_graph / 1e3, 1)),
                   torch_gpu=dict(us=round(us_torch, 2), meshes_per_s=round(N / us_torch * 1e6),
                                  GBps=round(nbytes / us_torch / 1e3, 1)),
                   cpu_per_mesh=dict(us=round(us_cpu, 1), meshes_per_s=round(N / us_cpu * 1e6), meshes_timed=nc),
                   speedup_vs_torch_gpu=round(us_torch / us_fused, 2))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
