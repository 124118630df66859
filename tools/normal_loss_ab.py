"""A/B of the face-normal loss (lambda_normal) on the headline step: CAPE-affineconv_nz64 at batch 16, the captured step
bench.py times, built twice in one process -- lambda_normal = 0 and lambda_normal = 1 (faces from tests/golden) -- on the same
seeded batch, for the generator-only and the adversarial step.  The two captured steps are timed in alternating windows
(--rounds x --steps replays each, host clock around a device synchronise); the result is the median of the windows' ms/step
per variant.  The C-ABI dispatches of one step are counted afterwards in an eager pass of each step body
(cape_amd.ops.LAUNCH_LOG), the torch launches the option adds with the profiler.  Last, the op alone (value + gradient,
N = --batch, --op-calls calls per captured graph) against an op-by-op torch-GPU restatement of the same definition
(tests/normal_loss_reference.py), both graph-replayed, alternating windows, medians.  One JSON line.
Usage: python tools/normal_loss_ab.py [--steps 50] [--rounds 9] [--skip-step] [--skip-op]"""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def build(batch, config, lam, faces):
    from bench import synthetic_batch
    from cape_amd.configs import cape_params
    from cape_amd.load_data import load_graph_mtx
    from cape_amd.models import CAPE
    L, D, U, p, L_d, D_d, _ = load_graph_mtx(None, load_for_demo=True)
    decay_steps = 2 * (31036 - 100) / 16                     # as bench.build_model
    params = cape_params(config, p=p, batch_size=batch, name='normal_loss_ab', decay_steps=decay_steps)
    model = CAPE(L=L, D=D, U=U, L_d=L_d, D_d=D_d, device='cuda:0', lambda_normal=lam, faces=faces, **params)
    model.build_graph(model.input_num_verts, model.nn_input_channel, phase='train')
    return model, synthetic_batch(model, seed=1234)


def dispatches(model, batch, gan):
    """(C-ABI calls of one step body, device kernels of one step body seen by the profiler) from eager passes."""
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
    kernels = None
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            r._fwd_bwd()
            torch.cuda.synchronize()
        kernels = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower()
                      and 'memset' not in e.name.lower())
    except Exception as exc:                                  # the count is informative; the timing does not depend on it
        kernels = 'unavailable: %s' % type(exc).__name__
    return len(names), names.count("face_normal_loss"), kernels


def windows(runners, steps, rounds):
    ms = [[] for _ in runners]
    for _ in range(rounds):
        for i, fn in enumerate(runners):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[i].append(1e3 * (time.perf_counter() - t0) / steps)
    return ms


def summary(ms):
    return dict(median=round(statistics.median(ms), 5), min=round(min(ms), 5), max=round(max(ms), 5))


def step_ab(args, faces, gan):
    from cape_amd.runtime import GraphedTrainStep
    variants = {}
    for name, lam in (("off", 0.0), ("on", 1.0)):
        model, batch = build(args.batch, args.config, lam, faces)
        runner = GraphedTrainStep(model, with_gan=gan)
        runner.load_batch(**batch)
        torch.cuda.synchronize()
        runner.capture()
        for _ in range(args.warmup):
            runner.step()
        torch.cuda.synchronize()
        variants[name] = dict(model=model, batch=batch, runner=runner)
    ms = windows([v["runner"].step for v in variants.values()], args.steps, args.rounds)
    out = {}
    for (name, v), m in zip(variants.items(), ms):
        # counted after every capture: an eager pass records an autograd graph on the default stream that a later capture
        # of the same model must not meet
        calls, normal_calls, kernels = dispatches(v["model"], v["batch"], gan)
        out[name] = dict(ms_per_step=summary(m), c_abi_calls_per_step=calls, face_normal_loss_calls=normal_calls,
                         device_kernels_fwd_bwd=kernels,
                         normal=float(v["runner"].losses["normal"]) if "normal" in v["runner"].losses else None)
    out["on_over_off"] = round(out["on"]["ms_per_step"]["median"] / out["off"]["ms_per_step"]["median"], 5)
    return out


def op_ab(args, faces):
    """us per call of the device op and of the torch restatement (forward + autograd backward), both inside replayed graphs."""
    import normal_loss_reference as R
    from cape_amd import ops
    from cape_amd.graph import vertex_face_table
    from cape_amd.load_data import load_pack
    dev = torch.device('cuda:0')
    vr_np = load_pack()['template_verts']
    V = vr_np.shape[0]
    rng = np.random.default_rng(27)
    pred = torch.tensor(rng.standard_normal((args.batch, V, 3)), dtype=torch.float32, device=dev, requires_grad=True)
    gt = (pred.detach() + 0.2 * torch.tensor(rng.standard_normal((args.batch, V, 3)), dtype=torch.float32, device=dev))
    vr = torch.tensor(vr_np, dtype=torch.float32, device=dev)
    fptr, fidx = vertex_face_table(faces, V)
    tabs = [torch.tensor(np.ascontiguousarray(a), dtype=torch.int32, device=dev) for a in (faces, fptr, fidx)]
    faces_t = tabs[0].long()                                  # the restatement's index tensor, on the device before capture
    keep = {}

    def hip_call():
        total, parts = ops.FaceNormalLossFn.apply(pred, gt, vr, *tabs, 1.0)       # the gradient is computed in forward
        keep['hip'] = (total, parts)

    def torch_call():
        loss = R.normal_loss(pred, gt, vr, faces_t)
        keep['torch'] = (loss, torch.autograd.grad(loss, pred)[0])

    graphs = []
    for fn in (hip_call, torch_call):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.op_calls):
                fn()
        for _ in range(args.warmup):
            g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    ms = windows([g.replay for g in graphs], args.steps, args.rounds)
    us = [dict((k, round(1e3 * v / args.op_calls, 3)) for k, v in summary(m).items()) for m in ms]
    return dict(batch=args.batch, calls_per_graph=args.op_calls, hip_us_per_call=us[0], torch_us_per_call=us[1],
                torch_over_hip=round(us[1]["median"] / us[0]["median"], 2),
                value_hip=float(keep['hip'][1][0]), value_torch=float(keep['torch'][0].detach()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50, help='replays per timed window')
    ap.add_argument('--rounds', type=int, default=9, help='timed windows per variant (alternating)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--op-calls', type=int, default=20, help='calls of the op inside one captured graph')
    ap.add_argument('--config', default='CAPE-affineconv_nz64_pose32_clotype32_male')
    ap.add_argument('--faces', default=os.path.join(ROOT, 'tests', 'golden', 'template_faces.npy'))
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--skip-op', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    faces = np.load(args.faces)
    out = dict(config=args.config, batch=args.batch, steps=args.steps, rounds=args.rounds)
    if not args.skip_op:
        out["op"] = op_ab(args, faces)
    if not args.skip_step:
        out["generator_step"] = step_ab(args, faces, gan=False)
        out["adversarial_step"] = step_ab(args, faces, gan=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
