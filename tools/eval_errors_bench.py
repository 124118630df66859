"""The test-set error of the headline configuration (CAPE-affineconv_nz64 at batch 16, --samples synthetic samples, the shipped
std and clothing vertices) made two ways, end to end on the host clock:
  device   CAPE.test_errors: generator + losses + distance launch per batch, one statistics call, small copies
  host     predict(labels=...) -- every prediction copied to the host -- followed by the numpy formula of demos.py:68-78
           (de-normalise both sides, subtract, clothing vertices, norms, np.mean / np.std / np.median)
in alternating windows (one evaluation per window), median of --rounds each.  Then the statistics call alone on the
[--samples, 3627] buffer: device events around its 12 launches (no copy), median of --rounds windows of --stat-calls calls,
with the passes it makes over the buffer and the resulting GB/s; --stats-only runs just that (for a kernel trace).
One JSON line.  Usage: python tools/eval_errors_bench.py [--samples 2048] [--rounds 5] [--stats-only]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
STAT_PASSES = 6          # row sums, variance, per-vertex means, three digit passes (cape_amd.ops.error_stats_launch)


def build(batch, config):
    from cape_amd.configs import cape_params
    from cape_amd.load_data import load_graph_mtx
    from cape_amd.models import CAPE
    L, D, U, p, L_d, D_d, _ = load_graph_mtx(None, load_for_demo=True)
    decay_steps = 2 * (31036 - 100) / 16                     # as bench.build_model
    params = cape_params(config, p=p, batch_size=batch, name='eval_errors_bench', decay_steps=decay_steps)
    model = CAPE(L=L, D=D, U=U, L_d=L_d, D_d=D_d, device='cuda:0', **params)
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='train')
    model.load_variables({}, strict=False)                   # the initial weights count as loaded
    return model


def host_way(model, data, cond, clo, mean, std, idx):
    preds, lr_, ll_, le_ = model.predict(data, cond, clo, labels=data, sess=model)
    p = preds * std + mean
    g = data * std + mean
    d = np.sqrt((((p - g)[:, idx]) ** 2).sum(-1))
    return dict(recon=lr_, latent=ll_, edge=le_, euclidean_mean=float(d.mean()), euclidean_std=float(d.std()),
                euclidean_median=float(np.median(d)))


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def end_to_end(args, std, mean, idx):
    model = build(args.batch, args.config)
    rng = np.random.default_rng(1234)
    S = args.samples
    data = rng.standard_normal((S, 6890, 3)).astype(np.float32)
    cond = (0.5 * rng.standard_normal((S, 126))).astype(np.float32)
    clo = np.eye(4, dtype=np.float32)[rng.integers(0, 4, S)]
    ways = [lambda: model.test_errors(data, cond, clo, std=std, clothing_idx=idx),
            lambda: host_way(model, data, cond, clo, mean, std, idx)]
    results = [None, None]
    for i, fn in enumerate(ways):                             # warm-up, and the two results on the same seed
        torch.manual_seed(5)
        results[i] = fn()
    sec = [[], []]
    for _ in range(args.rounds):
        for i, fn in enumerate(ways):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            sec[i].append(time.perf_counter() - t0)
    keys = ('recon', 'latent', 'edge', 'euclidean_mean', 'euclidean_std', 'euclidean_median')
    out = dict(samples=S, batch=args.batch, device_s=summary(sec[0]), host_s=summary(sec[1]),
               host_over_device=round(statistics.median(sec[1]) / statistics.median(sec[0]), 3),
               device_result={k: results[0][k] for k in keys}, host_result={k: results[1][k] for k in keys})
    return out


def stats_alone(args):
    from cape_amd import ops
    S, Vc = args.samples, 3627
    rng = np.random.default_rng(7)
    dist = torch.tensor(np.exp(rng.uniform(-9, -3, (S, Vc))).astype(np.float32), device='cuda:0')
    n = S * Vc
    lo, hi, _ = ops.quantile_ranks(n, 0.5)
    ranks = sorted({lo, hi})
    for _ in range(3):
        ops.error_stats_launch(dist, ranks)
    torch.cuda.synchronize()
    us = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.stat_calls):
            ops.error_stats_launch(dist, ranks)
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / args.stat_calls)
    med = statistics.median(us)
    t0 = time.perf_counter()
    res = ops.error_statistics(dist, (0.5,))
    wall_ms = 1e3 * (time.perf_counter() - t0)
    return dict(shape=[S, Vc], buffer_mb=round(n * 4 / 1e6, 2), ranks=len(ranks), launches=12, passes=STAT_PASSES,
                us_per_call=summary(us), gb_per_s_over_all_passes=round(STAT_PASSES * n * 4 / (med * 1e-6) / 1e9, 1),
                with_copy_and_sync_ms=round(wall_ms, 3), median=res['euclidean_median'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=5, help='timed windows per way (alternating)')
    ap.add_argument('--stat-calls', type=int, default=20, help='statistics calls per timed window')
    ap.add_argument('--config', default='CAPE-affineconv_nz64_pose32_clotype32_male')
    ap.add_argument('--stats-only', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stats = np.load(os.path.join(GOLDEN, 'trainset_stats.npz'))
    std, mean = stats['std'].astype(np.float32), stats['mean'].astype(np.float32)
    idx = np.load(os.path.join(GOLDEN, 'clothing_verts_idx.npy'))
    out = dict(config=args.config)
    out['statistics_call'] = stats_alone(args)
    if not args.stats_only:
        out['end_to_end'] = end_to_end(args, std, mean, idx)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
