"""What the wrappers around the C ABI share on the way from a tensor to a pointer: the stream, pointers, the device a wrapper's
tables live on, and the checks between a tensor and the kernels that read through its pointer.  (``ops.py`` keeps its own:
its globals are driven from outside the package.)
"""
import ctypes as C

import torch

from . import _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def resolve_device(device):
    """``device`` (None: the current GPU) as tensors report it: "cuda" -> "cuda:<current>"."""
    dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def rows(name, t, dev, N=None, R=None):
    """(N, R, leading dimension) of a float32 tensor [N, R, 3] on the device ``dev`` whose rows are ld >= 3 floats apart and whose
    samples are R rows apart: a contiguous tensor, or the [:, :, :3] view of one with wider rows.  ``N`` / ``R``: what the
    caller's other arguments fix (None: any size >= 1).  Anything else -- a host tensor, one on another device than the
    tables -- is a ValueError: the kernels would read through its pointer."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev:
        raise ValueError("%s: must be a float32 tensor on %s" % (name, dev))
    shape = tuple(t.shape)                                                           # once: this runs before every launch
    if (len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1 or (N is not None and shape[0] != N)
            or (R is not None and shape[1] != R)):
        raise ValueError("%s: [%s, %s, 3]%s expected, got %s" % (name, "N" if N is None else "%d" % N, "M" if R is None else "%d" % R,
                                                                "" if R is not None else " with M >= 1", shape))
    n, r = shape[:2]
    s0, ld, s2 = t.stride()
    if s2 != 1 or ld < 3 or (n > 1 and s0 != r * ld):                                # one sample: its stride is never used
        raise ValueError("%s: rows of at least 3 floats, unit stride inside a row, samples %d rows apart expected" % (name, r))
    return n, r, ld


def check_tensor(name, t, dtype, shape, dev):
    """ValueError unless ``t`` is a contiguous tensor of ``dtype`` and ``shape`` on ``dev``."""
    if not torch.is_tensor(t) or t.dtype != dtype or t.device != dev or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s: a contiguous %s tensor %s on %s expected" % (name, dtype, tuple(shape), dev))


def workspace(nbytes_or_error, dev, entry_name):
    """(16-byte aligned workspace, its size in bytes) for what a ``*_workspace_bytes`` entry returned; negative: its error."""
    need = int(nbytes_or_error)
    if need < 0:
        _lib.check(need, entry_name)
    return torch.empty((need + 15) // 16 * 2, dtype=torch.float64, device=dev), need
