"""A/B of the weighted reconstruction loss (loss_mask) on the headline step: CAPE-affineconv_nz64 at batch 16, the captured
generator step bench.py times, built twice in one process -- without a mask (cape_recon_edge_loss_fwd_bwd) and with the
binary mask (cape_masked_recon_edge_loss_fwd_bwd) -- on the same seeded batch.  The two captured steps are timed in
alternating windows (--rounds x --steps replays each, host clock around a device synchronise); the result is the median of
the windows' ms/step per variant.  The C-ABI dispatches of one step are counted afterwards in an eager pass of each step
body (cape_amd.ops.LAUNCH_LOG).  One JSON line.  Usage: python tools/loss_mask_ab.py [--steps 50] [--rounds 7] [--gan]"""
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


def build(batch, config, mask):
    from bench import synthetic_batch
    from cape_amd.configs import cape_params
    from cape_amd.load_data import load_graph_mtx
    from cape_amd.models import CAPE
    L, D, U, p, L_d, D_d, _ = load_graph_mtx(None, load_for_demo=True)
    decay_steps = 2 * (31036 - 100) / 16                     # as bench.build_model
    params = cape_params(config, p=p, batch_size=batch, name='loss_mask_ab', decay_steps=decay_steps)
    params['loss_mask'] = mask
    model = CAPE(L=L, D=D, U=U, L_d=L_d, D_d=D_d, device='cuda:0', **params)
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='train')
    return model, synthetic_batch(model, seed=1234)


def dispatches(model, batch, gan):
    """(C-ABI calls of one step body, loss-kernel entries among them) from an eager pass."""
    from cape_amd import ops
    from cape_amd.runtime import GraphedTrainStep
    r = GraphedTrainStep(model, with_gan=gan, use_graph=False)
    r.load_batch(**batch)
    ops.LAUNCH_LOG = []
    try:
        r._fwd_bwd()
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    return len(names), sorted(n for n in set(names) if "recon_edge_loss" in n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50, help='replays per timed window')
    ap.add_argument('--rounds', type=int, default=7, help='timed windows per variant (alternating)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--config', default='CAPE-affineconv_nz64_pose32_clotype32_male')
    ap.add_argument('--gan', action='store_true', help='the adversarial step instead of the generator step')
    ap.add_argument('--mask', default=os.path.join(ROOT, 'tests', 'golden', 'loss_mask_binary.npy'))
    args = ap.parse_args()
    from cape_amd.runtime import GraphedTrainStep
    torch.cuda.set_device(0)
    variants = {}
    for name, mask in (("unmasked", None), ("masked", np.load(args.mask))):
        model, batch = build(args.batch, args.config, mask)
        runner = GraphedTrainStep(model, with_gan=args.gan)
        runner.load_batch(**batch)
        torch.cuda.synchronize()
        runner.capture()
        for _ in range(args.warmup):
            runner.step()
        torch.cuda.synchronize()
        variants[name] = dict(model=model, batch=batch, runner=runner, ms=[])
    for _ in range(args.rounds):
        for v in variants.values():
            r = v["runner"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                r.step()
            torch.cuda.synchronize()
            v["ms"].append(1e3 * (time.perf_counter() - t0) / args.steps)
    # counted after every capture: an eager pass records an autograd graph on the default stream that a later capture of the
    # same model must not meet
    for v in variants.values():
        v["dispatches"], v["loss_entries"] = dispatches(v["model"], v["batch"], args.gan)
    out = dict(config=args.config, batch=args.batch, gan=args.gan, steps=args.steps, rounds=args.rounds)
    for name, v in variants.items():
        out[name] = dict(ms_per_step_median=round(statistics.median(v["ms"]), 4), ms_per_step_min=round(min(v["ms"]), 4),
                         ms_per_step_max=round(max(v["ms"]), 4), dispatches_per_step=v["dispatches"],
                         loss_entries=v["loss_entries"], recon=float(v["runner"].losses["recon"]))
    a, b = out["unmasked"]["ms_per_step_median"], out["masked"]["ms_per_step_median"]
    out["masked_over_unmasked"] = round(b / a, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
