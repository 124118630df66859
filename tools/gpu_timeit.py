"""Event timing shared by the micro-benchmarks of this directory."""
import torch


def timeit(fn, iters=20):
    """Seconds per call of ``fn``: three warm-up calls, then ``iters`` calls between two events on the current stream."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3
