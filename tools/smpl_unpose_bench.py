"""SMPL unposing throughput: N in {16, 256} posed meshes on the 6890-vertex template with a seeded synthetic SMPL-format
model (tests/smpl_synth.py), one JSON line per N, everything timed in the same run on the same device:
  unpose        cape_amd.smpl.SMPL.unpose, the exact inverse (cape_smpl_unpose_joints + cape_smpl_unpose_skin): eager calls
                (host launch cost included) and replays of one captured graph of the call (device time)
  solve / skin  its two launches alone (eager, device events)
  explicit      SMPL.unpose(joints_from=template): cape_smpl_joints twice + cape_smpl_unpose_skin, graph replay
  forward       SMPL.forward at the same N, graph replay: the skin half of unposing streams the same blend basis
  torch         an op-by-op torch-GPU restatement of the exact inverse (torch.linalg.inv per vertex, torch.linalg.solve per
                sample), eager
Device events, median of --calls after warm-up.  Algorithmic bytes of the skin half: the blend basis read once per sample tile,
the skinning weights (ELL), the posed vertices in and the rest vertices out.
Usage: python tools/smpl_unpose_bench.py [--calls 50] [--sizes 16,256] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_unpose(t, P, pose, betas):
    """Op-by-op restatement of the exact inverse on tensors from ``smpl_bench._torch_arrays`` (plus ``jreg_cols``, the vertices the regressor touches)."""
    N, J = pose.shape[0], t["parents"].shape[0]
    r = pose.reshape(N, J, 3)
    th2 = (r * r).sum(-1, keepdim=True)
    th = th2.clamp_min(1e-12).sqrt()
    s = torch.where(th2 < 1e-6, 1 - th2 / 6, torch.sin(th) / th)
    h = torch.sin(0.5 * th) / th
    c = torch.where(th2 < 1e-6, 0.5 - th2 / 24, 2 * h * h)
    x, y, z = r.unbind(-1)
    zero = torch.zeros_like(x)
    Kx = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(N, J, 3, 3)
    eye = torch.eye(3, device=P.device)
    R = eye + s[..., None] * Kx + c[..., None] * (r[..., :, None] * r[..., None, :] - th2[..., None] * eye)
    pf = (R[:, 1:] - eye).reshape(N, -1)
    chain = [R[:, 0]]
    for j in range(1, J):
        chain.append(chain[int(t["parents"][j])] @ R[:, j])
    Wr = torch.stack(chain, 1)                                                   # [N, J, 3, 3]
    acc = torch.einsum("vck,nk->nvc", t["posedirs"], pf)
    shape = torch.einsum("vck,nk->nvc", t["shapedirs"], betas)
    Minv = torch.linalg.inv(torch.einsum("vj,njab->nvab", t["weights"], Wr))
    # G_j.t = (L Jn)_j: the chain on selector matrices
    E = torch.eye(3 * J, device=P.device).reshape(J, 3, 3 * J)
    At = [E[0].expand(N, 3, 3 * J)]
    for j in range(1, J):
        p = int(t["parents"][j])
        At.append(At[p] + Wr[:, p] @ (E[j] - E[p]))
    L = (torch.stack(At, 1) - Wr @ E).reshape(N, 3 * J, 3 * J)
    cols = t["jreg_cols"]
    jr, w = t["jreg"][:, cols], t["weights"][cols]
    y0 = (Minv[:, cols] @ P[:, cols, :, None])[..., 0]
    rhs = torch.einsum("jv,nvc->njc", jr, y0 - acc[:, cols])
    wm = (w[None, :, :, None, None] * Minv[:, cols][:, :, None]).reshape(N, len(cols), 9 * J)
    Q = (jr @ wm).reshape(N, J, J, 3, 3).permute(0, 1, 3, 2, 4).reshape(N, 3 * J, 3 * J)
    Jn = torch.linalg.solve(torch.eye(3 * J, device=P.device) + Q @ L, rhs.reshape(N, 3 * J, 1)).reshape(N, J, 3)
    Gt = (L @ Jn.reshape(N, 3 * J, 1)).reshape(N, J, 3)
    Mt = torch.einsum("vj,njc->nvc", t["weights"], Gt)
    return (Minv @ (P - Mt)[..., None])[..., 0] - acc - shape, Jn


def _graph(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--sizes", default="16,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import smpl_synth as synth
    from smpl_bench import _time_events, _torch_arrays
    from cape_amd import smpl, _lib
    from cape_amd.smpl import _p, _stream
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    m = synth.smpl_like()
    model = smpl.SMPL(m, device=dev)
    tt = _torch_arrays(m, dev)
    tt["jreg_cols"] = torch.tensor(np.flatnonzero((m["J_regressor"].toarray() != 0).any(0)), device=dev)
    J, V, B = model.J, model.V, model.num_betas
    K = B + 9 * (J - 1)
    tile = _lib.lib.cape_smpl_skin_tile(K, J)
    d = model._upload()
    rng = np.random.default_rng(0)
    lines = []
    for N in [int(x) for x in a.sizes.split(",")]:
        T = torch.tensor(m["v_template"][None] + 0.01 * rng.standard_normal((N, V, 3)), dtype=torch.float32, device=dev)
        pose = torch.tensor(0.3 * rng.standard_normal((N, 3 * J)), dtype=torch.float32, device=dev)
        betas = torch.tensor(rng.standard_normal((N, B)), dtype=torch.float32, device=dev)
        JF = torch.tensor(m["v_template"][None], dtype=torch.float32, device=dev)
        with torch.no_grad():
            P, _ = model.forward(T, pose, betas)
            out = (torch.empty(N, V, 3, device=dev), torch.empty(N, J, 3, device=dev))
            fout = (torch.empty(N, V, 3, device=dev), torch.empty(N, J, 3, device=dev))
            ws = model.unpose_workspace(N)
            coef, G = torch.empty(N, K, device=dev), torch.empty(N, J, 12, device=dev)
            exact = lambda: model.unpose(P, pose, betas, out=out, workspace=ws)
            us_eager = _time_events(exact, a.calls)
            us_graph = _time_events(_graph(exact).replay, a.calls)
            us_explicit = _time_events(_graph(lambda: model.unpose(P, pose, betas, joints_from=JF, out=out)).replay, a.calls)
            us_forward = _time_events(_graph(lambda: model.forward(T, pose, betas, out=fout)).replay, a.calls)
            solve = lambda: _lib.check(_lib.lib.cape_smpl_unpose_joints(
                _p(P), 3 * V, _p(d.rowptr), _p(d.colidx), _p(d.vals), _p(d.ell_j), _p(d.ell_w), model.ell_width, _p(pose), _p(betas),
                B, _p(d.jposedirs), None, model._parents_c, J, V, N, _p(ws), ws.numel() * 8, _p(coef), _p(G), _p(out[1]), None, None,
                _stream()), "cape_smpl_unpose_joints")
            skin = lambda: _lib.check(_lib.lib.cape_smpl_unpose_skin(
                _p(P), 3 * V, model._basis(B), K, _p(coef), _p(G), _p(d.ell_j), _p(d.ell_w), model.ell_width, None, J, V, N,
                _p(out[0]), 3 * V, None, _stream()), "cape_smpl_unpose_skin")
            us_solve = _time_events(solve, a.calls)
            us_skin = _time_events(skin, a.calls)
            exact()
            err = float((out[0] - T).abs().max())
            us_torch = _time_events(lambda: torch_unpose(tt, P, pose, betas), max(5, a.calls // 5), warmup=3)
            dmax = float((torch_unpose(tt, P, pose, betas)[0] - out[0]).abs().max())
        tiles = -(-N // tile)
        nbytes = tiles * 4 * 3 * K * V + model.ell_width * V * 8 + 2 * N * V * 3 * 4
        rec = dict(tool="smpl_unpose_bench", N=N, V=V, J=J, K=K, tile=tile, skin_bytes=int(nbytes),
                   workspace_bytes=int(ws.numel() * 8), max_abs_round_trip=err, max_abs_diff_vs_torch=dmax,
                   unpose_eager_us=round(us_eager, 2), unpose_graph_us=round(us_graph, 2), solve_us=round(us_solve, 2),
                   skin_us=round(us_skin, 2), skin_GBps=round(nbytes / us_skin / 1e3, 1), explicit_graph_us=round(us_explicit, 2),
                   forward_graph_us=round(us_forward, 2), torch_gpu_us=round(us_torch, 2),
                   meshes_per_s=round(N / us_graph * 1e6), speedup_vs_torch_gpu=round(us_torch / us_eager, 2),
                   unpose_over_forward=round(us_graph / us_forward, 2))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
