"""Vertex-normal throughput: N in {1, 16, 256} meshes on the 6890-vertex / 13776-face template, one JSON line per N with, timed
in the same run (device events, median of --calls after warm-up, eager calls: host launch cost included):
  fwd       cape_amd.vertex_normals.VertexNormals.forward (cape_vertex_normals_fwd, one launch)
  fwd_bwd   VertexNormals.diff and its backward (cape_vertex_normals_fwd + cape_vertex_normals_bwd, three launches + autograd)
  torch     an op-by-op torch-GPU restatement (gather, cross, index_add_, normalise) without and with autograd
  pose      cape_amd.smpl.SMPL.forward at the same N on a seeded synthetic SMPL-format model: a vertex pass of this size
``fwd_graph``: replays of one captured graph of the forward call (device time without the host's launch cost).
Algorithmic bytes of the forward: vertices in, normals out, the three tables once (the gathers of a sample's 83 KB of
positions are cache traffic).  Usage: python tools/vertex_normals_bench.py [--calls 50] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_normals(x, f):
    """Op-by-op restatement on device tensors: x [N, V, 3] float32, f [F, 3] int64."""
    x0, x1, x2 = x[:, f[:, 0]], x[:, f[:, 1]], x[:, f[:, 2]]
    m = torch.cross(x1 - x0, x2 - x0, dim=-1)
    ss = (m * m).sum(-1, keepdim=True)
    u = m / torch.sqrt(ss + (ss == 0).to(m.dtype))
    s = torch.zeros_like(x)
    for k in range(3):
        s = s.index_add(1, f[:, k], u)
    ss = (s * s).sum(-1, keepdim=True)
    return s / torch.sqrt(ss + (ss == 0).to(s.dtype))


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import smpl_synth as synth
    from cape_amd import smpl, _lib
    from cape_amd.vertex_normals import VertexNormals
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    faces = np.load(os.path.join(ROOT, "tests", "golden", "template_faces.npy"))
    m = synth.smpl_like()
    body = smpl.SMPL(m, device=dev)
    V, F = body.V, int(faces.shape[0])
    vn = VertexNormals(faces, V, device=dev)
    ft = torch.tensor(faces, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(0)
    lines = []
    for N in [int(x) for x in a.sizes.split(",")]:
        x = torch.tensor(m["v_template"][None] + 0.005 * rng.standard_normal((N, V, 3)), dtype=torch.float32, device=dev)
        g = torch.tensor(rng.standard_normal((N, V, 3)), dtype=torch.float32, device=dev)
        pose = torch.tensor(0.5 * rng.standard_normal((N, 3 * body.J)), dtype=torch.float32, device=dev)
        out = torch.empty_like(x)
        pout = (torch.empty(N, V, 3, device=dev), torch.empty(N, body.J, 3, device=dev))
        xg = x.clone().requires_grad_(True)

        def fwd_bwd():
            xg.grad = None
            vn.diff(xg).backward(g)

        def torch_fwd_bwd():
            xg.grad = None
            torch_normals(xg, ft).backward(g)

        with torch.no_grad():
            us_fwd = _time_events(lambda: vn.forward(x, out=out), a.calls)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                vn.forward(x, out=out)
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                vn.forward(x, out=out)
            us_graph = _time_events(graph.replay, a.calls)
            us_torch = _time_events(lambda: torch_normals(x, ft), a.calls)
            us_pose = _time_events(lambda: body.forward(x, pose, None, None, out=pout), a.calls)
            dmax = float((torch_normals(x, ft) - out).abs().max())
        us_fb = _time_events(fwd_bwd, a.calls)
        g_hip = xg.grad.clone()
        us_torch_fb = _time_events(torch_fwd_bwd, a.calls)
        gdiff = float((xg.grad - g_hip).abs().max() / g_hip.abs().max())
        nbytes = 2 * N * V * 3 * 4 + (3 * F + V + 1 + 3 * F) * 4
        rate = lambda us: dict(us=round(us, 2), meshes_per_s=round(N / us * 1e6))
        rec = dict(tool="vertex_normals_bench", N=N, V=V, F=F, fwd_bytes=int(nbytes), max_abs_diff_vs_torch=dmax,
                   grad_max_rel_diff_vs_torch=gdiff,
                   fwd=dict(rate(us_fwd), GBps=round(nbytes / us_fwd / 1e3, 1)),
                   fwd_graph=dict(rate(us_graph), GBps=round(nbytes / us_graph / 1e3, 1)),
                   fwd_bwd=rate(us_fb), torch_fwd=rate(us_torch), torch_fwd_bwd=rate(us_torch_fb), pose=rate(us_pose),
                   speedup_fwd_vs_torch=round(us_torch / us_fwd, 2), speedup_fwd_bwd_vs_torch=round(us_torch_fb / us_fb, 2))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
