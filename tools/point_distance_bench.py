"""Mesh-to-scan distance throughput: the 6890 template vertices of N in {1, 16} meshes against M = 20000 scan points each, one
JSON line per (N, M) with, timed in the same run (device events, median of --calls after warm-up, eager calls: host launch cost
included):
  fwd          cape_amd.point_distance.PointDistance.forward (cape_point_nearest_fwd: search, merge + fp64 evaluation)
  fwd_bwd      PointDistance.diff and its backward to the vertices only (+ cape_point_nearest_bwd without dp; + autograd)
  fwd_bwd_dp   the same with a gradient to the points too (+ the per-point gather)
  torch        an op-by-op torch-GPU restatement of the brute force (every vertex against every point in the difference form
               |q - p|^2 -- no cdist, no expanded form -- and the min over the points), chunked over --chunk vertices, without
               and with autograd to the vertices (--torch-calls calls)
``tests_per_s``: vertex-point tests (N Q M) per second of the call; ``valu_fraction``: tests x 9 VALU instructions per test
against --valu-peak instructions x lanes per second (default: the part's fp32 vector rate of 157.3 TFLOPS counted in
fused multiply-adds, 7.865e13; plain fp32 VALU instructions issue faster than 16 lanes per SIMD and clock here).
With --fit: one ``CAPE.fit_scan`` step at batch 16 on a seeded model, M = 20000 points per scan, with ``lambda_mesh`` 0 and 1
in alternating sets (--fit-rounds of them), each from calls of --fit-steps and 0 steps.
With --cos-min C: also the normal-compatible forward (``query_normals`` = the meshes' vertex normals, ``point_normals`` = the
sampled faces' normals, ``cos_min`` = C; cape_point_nearest_compat_fwd) next to the plain one, in alternating sets of the same
run: ``fwd_plain_alt``, ``fwd_compat`` and their ratio ``compat_over_plain``.  --torch-calls 0 leaves the torch restatement out.
Usage: python tools/point_distance_bench.py [--calls 50] [--torch-calls 20] [--cos-min C] [--fit] [--out FILE]"""
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

OPS_PER_TEST = 9          # 3 sub, mul, 2 fma, cmp, 2 cndmask


def torch_d2(q, p):
    """Op-by-op restatement on device tensors: q [C, 3], p [M, 3] -> min over the points of |q - p|^2 [C]."""
    d = q[:, None, :] - p[None]
    dist = (d * d).sum(-1)
    dist = torch.where(torch.isfinite(dist), dist, torch.full_like(dist, float("inf")))
    return dist.min(1).values


def torch_points(x, p, chunk):
    """d2 [N, Q] of queries x [N, Q, 3] and points p [N, M, 3], one sample and ``chunk`` queries at a time."""
    return torch.stack([torch.cat([torch_d2(x[n, j:j + chunk], p[n]) for j in range(0, x.shape[1], chunk)])
                        for n in range(x.shape[0])])


def _time_events(fn, calls, warmup):
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


def _time_alternating(fns, calls, warmup, sets=5):
    """Median us per call of each of ``fns``, timed in ``sets`` alternating sets of calls / sets calls each: what drifts during the
    run (clocks, temperature) reaches all of them alike."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(sets):
        for k, fn in enumerate(fns):
            for _ in range(max(1, calls // sets)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts[k].append(a.elapsed_time(b) * 1e3)
    return [float(np.median(t)) for t in ts]


def fit_steps(steps, M, rounds, seed=0):
    """us per fit_scan step at batch 16 for lambda_mesh 0 and 1, ``rounds`` alternating sets: each figure is the difference of
    a call with ``steps`` steps and one with none, after a warm-up call of either kind.  Returns two lists."""
    import smpl_synth as synth
    import scan_distance_reference as R
    from cape_amd import smpl
    from cape_amd.load_data import load_graph_mtx
    from cape_amd.models import CAPE
    from oracle.configs import cape_params
    L, D, U, p, L_d, D_d, _ = load_graph_mtx(None, load_for_demo=True)
    bs = 16
    model = CAPE(L=L, D=D, U=U, L_d=L_d, D_d=D_d, p=p, **cape_params('affine_nz64', bs))
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='demo')
    model.load_variables({k: v.detach().cpu().numpy() for k, v in model._vars.items()})
    m = synth.smpl_like(seed=6)
    body = smpl.SMPL(m)
    gold = os.path.join(ROOT, "tests", "golden")
    rng = np.random.default_rng(seed)
    cond, cond2 = rng.standard_normal((bs, model.nz_cond)), rng.standard_normal((bs, model.nz_cond2))
    z = rng.standard_normal((bs, model.nz))
    pose = np.load(os.path.join(gold, "demo_pose_params.npz"))["pose"][rng.integers(0, 6, bs)]
    st = np.load(os.path.join(gold, "trainset_stats.npz"))
    dress = (st["mean"], st["std"], np.load(os.path.join(gold, "clothing_verts_idx.npy")))
    posed, _ = model.decode_posed(np.concatenate([z, cond, cond2], 1), cond, cond2, pose, body, *dress)
    faces = np.asarray(m["f"], dtype=np.int64)
    scan = np.stack([R.surface_samples(rng, posed[n].astype(np.float64), faces, M)[0] for n in range(bs)]).astype(np.float32)

    def per_step(lam):
        fn = lambda k: model.fit_scan(scan, pose, cond, cond2, body, *dress, steps=k, lambda_mesh=lam)
        t = []
        for k in (0, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return (t[1] - t[0]) / steps * 1e6

    for lam in (0.0, 1.0):
        model.fit_scan(scan, pose, cond, cond2, body, *dress, steps=2, lambda_mesh=lam)
    one, two = [], []
    for _ in range(rounds):
        one.append(per_step(0.0))
        two.append(per_step(1.0))
    return one, two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--torch-calls", type=int, default=20)
    ap.add_argument("--sizes", default="1,16")
    ap.add_argument("--points", default="20000")
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--valu-peak", type=float, default=157.3e12 / 2)
    ap.add_argument("--cos-min", type=float, default=None)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--fit-steps", type=int, default=20)
    ap.add_argument("--fit-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import scan_distance_reference as R
    from cape_amd import _lib
    from cape_amd.point_distance import PointDistance
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    verts, faces = R.template()
    Q = verts.shape[0]
    pd = PointDistance(device=dev)
    rng = np.random.default_rng(0)
    lines = []
    for N in [int(x) for x in a.sizes.split(",")]:
        for M in [int(x) for x in a.points.split(",")]:
            xs = (verts[None] + 0.005 * rng.standard_normal((N, Q, 3))).astype(np.float32)
            samples = [R.surface_samples(rng, xs[n].astype(np.float64), faces, M) for n in range(N)]
            ps = np.stack([s[0] + rng.uniform(-0.01, 0.03, M)[:, None] * s[1] for s in samples]).astype(np.float32)
            x, p = torch.tensor(xs, device=dev), torch.tensor(ps, device=dev)
            g = torch.tensor(rng.standard_normal((N, Q)), dtype=torch.float32, device=dev)
            xg, pg = x.clone().requires_grad_(True), p.clone().requires_grad_(True)

            def fwd_bwd():
                xg.grad = None
                pd.diff(xg, p).backward(g)

            def fwd_bwd_dp():
                xg.grad = pg.grad = None
                pd.diff(xg, pg).backward(g)

            def torch_fwd_bwd():                      # chunk by chunk: the graph of all chunks at once would not fit
                xg.grad = None
                for n in range(N):
                    for j in range(0, Q, a.chunk):
                        torch_d2(xg[n, j:j + a.chunk], p[n]).backward(g[n, j:j + a.chunk])

            with torch.no_grad():
                us_fwd = _time_events(lambda: pd.forward(x, p), a.calls, 10)
            us_fb = _time_events(fwd_bwd, a.calls, 10)
            g_hip = xg.grad.clone()
            us_fb_dp = _time_events(fwd_bwd_dp, a.calls, 10)
            tests = float(N) * Q * M
            rate = lambda us: dict(us=round(us, 1), tests_per_s=float("%.4g" % (tests / us * 1e6)),
                                   valu_fraction=float("%.3g" % (tests * OPS_PER_TEST / (us * 1e-6) / a.valu_peak)))
            rec = dict(tool="point_distance_bench", N=N, Q=Q, M=M, split=pd.plan(N, Q, M)[0], fwd=rate(us_fwd), fwd_bwd=rate(us_fb),
                       fwd_bwd_dp=rate(us_fb_dp), calls=a.calls, torch_calls=a.torch_calls)
            if a.torch_calls > 0:
                with torch.no_grad():
                    us_torch = _time_events(lambda: torch_points(x, p, a.chunk), a.torch_calls, 2)
                    d_hip, d_torch = pd.forward(x, p)[0], torch_points(x, p, a.chunk)
                    dmax = float((d_hip.sqrt() - d_torch.sqrt()).abs().max())
                xg.grad = None
                fwd_bwd()
                g_hip = xg.grad.clone()
                us_torch_fb = _time_events(torch_fwd_bwd, a.torch_calls, 2)
                gdiff = float((xg.grad - g_hip).abs().max() / g_hip.abs().max())
                rec.update(max_abs_dist_diff_vs_torch=dmax, grad_max_rel_diff_vs_torch=gdiff, torch_fwd=rate(us_torch),
                           torch_fwd_bwd=rate(us_torch_fb), speedup_fwd_vs_torch=round(us_torch / us_fwd, 1),
                           speedup_fwd_bwd_vs_torch=round(us_torch_fb / us_fb, 1))
            if a.cos_min is not None:
                from cape_amd.vertex_normals import VertexNormals
                pn = torch.tensor(np.stack([s[1] for s in samples]).astype(np.float32), device=dev)
                with torch.no_grad():
                    qn = VertexNormals(faces, Q, device=dev).forward(x)
                    kw = dict(query_normals=qn, point_normals=pn, cos_min=a.cos_min)
                    us_plain, us_compat = _time_alternating([lambda: pd.forward(x, p), lambda: pd.forward(x, p, **kw)], a.calls, 10)
                    kept = int((pd.forward(x, p, **kw)[1] >= 0).sum())
                rec.update(cos_min=a.cos_min, fwd_plain_alt=rate(us_plain), fwd_compat=rate(us_compat),
                           compat_over_plain=round(us_compat / us_plain, 3), queries_with_a_point=kept)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.fit:
        one, two = fit_steps(a.fit_steps, 20000, a.fit_rounds)
        rec = dict(tool="point_distance_bench", fit_batch=16, fit_points=20000, steps=a.fit_steps, rounds=a.fit_rounds,
                   fit_scan_step_us=dict(lambda_mesh_0=[round(t, 1) for t in one], lambda_mesh_1=[round(t, 1) for t in two]),
                   median_us=dict(lambda_mesh_0=round(float(np.median(one)), 1), lambda_mesh_1=round(float(np.median(two)), 1)))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
