"""Scan-to-mesh distance throughput on the 6890-vertex / 13776-face template: N in {1, 16} meshes against M in {2000, 20000} scan
points each, one JSON line per (N, M) with, timed in the same run (device events, median of --calls after warm-up, eager calls:
host launch cost included):
  fwd        cape_amd.scan_distance.ScanDistance.forward (cape_scan_nearest_fwd: records, search, merge + fp64 evaluation)
  fwd_bwd    ScanDistance.diff and its backward to the vertices (+ cape_scan_nearest_bwd: point records, gather; + autograd)
  torch      an op-by-op torch-GPU restatement of the brute force (every point against every face, the seven-region rule with
             torch.where, min over the faces), chunked over --chunk points, without and with autograd (--torch-calls calls)
``tests_per_s``: point-triangle tests (N M F) per second of the call.  With --fit: one ``CAPE.fit_posed`` step and one
``CAPE.fit_scan`` step at batch 16 on a seeded model, M = 20000 points per scan, from calls of --fit-steps and 0 steps.
With --cos-min C: also the normal-compatible forward (``normals`` = the sampled faces' normals, ``cos_min`` = C;
cape_scan_nearest_compat_fwd) next to the plain one, in alternating sets of the same run: ``fwd_plain_alt``, ``fwd_compat`` and
their ratio ``compat_over_plain``.  --torch-calls 0 leaves the torch restatement out.
Usage: python tools/scan_distance_bench.py [--calls 50] [--torch-calls 50] [--cos-min C] [--fit] [--out FILE]"""
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


def torch_d2(x, f, p):
    """Op-by-op restatement on device tensors: x [V, 3] float32, f [F, 3] int64, p [P, 3] -> min over the faces of d2 [P]."""
    a, b, c = x[f[:, 0]][None], x[f[:, 1]][None], x[f[:, 2]][None]
    q = p[:, None, :]
    ab, ac, ap, bp, cp = b - a, c - a, q - a, q - b, q - c
    dot = lambda u, v: (u * v).sum(-1)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    denom = va + vb + vc
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    v, w = vb / denom, vc / denom
    t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    for cond, vv, ww in (((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), 1 - t, t),
                         ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),
                         ((d6 >= 0) & (d5 <= d6), zero, one),
                         ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),
                         ((d3 >= 0) & (d4 <= d3), one, zero),
                         ((d1 <= 0) & (d2 <= 0), zero, zero)):                      # the rule's order reversed: the first wins
        v, w = torch.where(cond, vv, v), torch.where(cond, ww, w)
    r = ap - v[..., None] * ab - w[..., None] * ac
    dist = (r * r).sum(-1)
    dist = torch.where(torch.isfinite(dist), dist, torch.full_like(dist, float("inf")))
    return dist.min(1).values


def torch_scan(x, f, p, chunk):
    """d2 [N, M] of meshes x [N, V, 3] and points p [N, M, 3], one mesh and ``chunk`` points at a time."""
    return torch.stack([torch.cat([torch_d2(x[n], f, p[n, i:i + chunk]) for i in range(0, p.shape[1], chunk)])
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


def fit_steps(steps, M, seed=0):
    """(us per fit_posed step, us per fit_scan step) at batch 16: the difference of a call with ``steps`` steps and one with
    none, both after a warm-up call."""
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

    def per_step(fn):
        fn(2)
        t = []
        for k in (0, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return (t[1] - t[0]) / steps * 1e6

    us_posed = per_step(lambda k: model.fit_posed(posed, pose, cond, cond2, body, *dress, steps=k))
    us_scan = per_step(lambda k: model.fit_scan(scan, pose, cond, cond2, body, *dress, steps=k))
    return us_posed, us_scan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--torch-calls", type=int, default=50)
    ap.add_argument("--sizes", default="1,16")
    ap.add_argument("--points", default="2000,20000")
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--cos-min", type=float, default=None)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--fit-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import scan_distance_reference as R
    from cape_amd import _lib
    from cape_amd.scan_distance import ScanDistance
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    verts, faces = R.template()
    V, F = verts.shape[0], int(faces.shape[0])
    sd = ScanDistance(faces, V, device=dev)
    ft = torch.tensor(faces, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(0)
    lines = []
    for N in [int(x) for x in a.sizes.split(",")]:
        for M in [int(x) for x in a.points.split(",")]:
            xs = (verts[None] + 0.005 * rng.standard_normal((N, V, 3))).astype(np.float32)
            samples = [R.surface_samples(rng, xs[n].astype(np.float64), faces, M) for n in range(N)]
            ps = np.stack([s[0] + rng.uniform(-0.01, 0.03, M)[:, None] * s[1] for s in samples]).astype(np.float32)
            x, p = torch.tensor(xs, device=dev), torch.tensor(ps, device=dev)
            nrm = torch.tensor(np.stack([s[1] for s in samples]).astype(np.float32), device=dev)
            g = torch.tensor(rng.standard_normal((N, M)), dtype=torch.float32, device=dev)
            xg = x.clone().requires_grad_(True)

            def fwd_bwd():
                xg.grad = None
                sd.diff(xg, p).backward(g)

            def torch_fwd_bwd():                      # chunk by chunk: the graph of all chunks at once would not fit
                xg.grad = None
                for n in range(N):
                    for i in range(0, M, a.chunk):
                        torch_d2(xg[n], ft, p[n, i:i + a.chunk]).backward(g[n, i:i + a.chunk])

            with torch.no_grad():
                us_fwd = _time_events(lambda: sd.forward(x, p), a.calls, 10)
            us_fb = _time_events(fwd_bwd, a.calls, 10)
            g_hip = xg.grad.clone()
            tests = float(N) * M * F
            rate = lambda us: dict(us=round(us, 1), tests_per_s=float("%.4g" % (tests / us * 1e6)))
            rec = dict(tool="scan_distance_bench", N=N, M=M, V=V, F=F, split=sd.plan(N, M)[0], fwd=rate(us_fwd), fwd_bwd=rate(us_fb),
                       calls=a.calls, torch_calls=a.torch_calls)
            if a.torch_calls > 0:
                with torch.no_grad():
                    us_torch = _time_events(lambda: torch_scan(x, ft, p, a.chunk), a.torch_calls, 2)
                    d_hip, d_torch = sd.forward(x, p)[0], torch_scan(x, ft, p, a.chunk)
                    dmax = float((d_hip.sqrt() - d_torch.sqrt()).abs().max())
                us_torch_fb = _time_events(torch_fwd_bwd, a.torch_calls, 2)
                # 0 * inf: autograd through torch.where gives NaN where an unselected branch divides by a rounded-to-zero denominator
                fin = torch.isfinite(xg.grad)
                gdiff = float((xg.grad - g_hip)[fin].abs().max() / g_hip.abs().max())
                rec.update(max_abs_dist_diff_vs_torch=dmax, grad_max_rel_diff_vs_torch=gdiff,
                           torch_grad_nonfinite=int((~fin).sum()), torch_fwd=rate(us_torch), torch_fwd_bwd=rate(us_torch_fb),
                           speedup_fwd_vs_torch=round(us_torch / us_fwd, 1), speedup_fwd_bwd_vs_torch=round(us_torch_fb / us_fb, 1))
            if a.cos_min is not None:
                with torch.no_grad():
                    us_plain, us_compat = _time_alternating(
                        [lambda: sd.forward(x, p), lambda: sd.forward(x, p, normals=nrm, cos_min=a.cos_min)], a.calls, 10)
                    kept = int((sd.forward(x, p, normals=nrm, cos_min=a.cos_min)[1] >= 0).sum())
                rec.update(cos_min=a.cos_min, fwd_plain_alt=rate(us_plain), fwd_compat=rate(us_compat),
                           compat_over_plain=round(us_compat / us_plain, 3), points_with_a_face=kept)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.fit:
        us_posed, us_scan = fit_steps(a.fit_steps, 20000)
        rec = dict(tool="scan_distance_bench", fit_batch=16, fit_points=20000, fit_posed_step_us=round(us_posed, 1),
                   fit_scan_step_us=round(us_scan, 1), steps=a.fit_steps)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
