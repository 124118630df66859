"""Mesh-to-scan distance on the device: for every query (a mesh vertex) the nearest point of a point cloud (a raw scan), for a
batch of query sets and clouds, and its gradient (cape_amd/csrc/scan/point_distance.hip).  The opposite direction of
``cape_amd.scan_distance``; the two together are the symmetric (chamfer) objective.

  PointDistance()                            no topology, nothing to upload
    .forward(queries, points, count=None)    (d2 [N, Q], index [N, Q] int32) of device queries [N, Q, 3] and device points
                                             [N, M, 3], no gradient (cape_point_nearest_fwd: exact search over all points)
    .diff(queries, points, count=None)       d2 as an autograd function: gradients to ``queries`` and ``points``
                                             (cape_point_nearest_bwd: no atomics); the index is saved, not recomputed
    .np(queries, points)                     numpy in, numpy out; ``points`` [N, M, 3] or a list of N arrays [m_n, 3]

``d2`` is the squared distance to ``points[index]``; ``count`` [N] says how many of a sample's M rows are points (the rest is
padding and is never read).  A point with a non-finite coordinate never wins; a query with a non-finite coordinate, a sample
with ``count`` 0 and a sample without a finite point get index -1, d2 NaN and no gradient.  The gradient is that of d2 with the
index held constant (exact wherever d2 is differentiable).  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .scan_distance import _count, _points, pad_points
from .vertex_normals import _p, _stream


def _queries(name, t, dev):
    """(N, Q, leading dimension) of a float32 tensor [N, Q, 3] on ``dev``, by the rules of ``scan_distance._points``."""
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[0] < 1:
        raise ValueError("%s: a float32 tensor [N, Q, 3] on %s expected" % (name, dev))
    N = int(t.shape[0])
    Q, ld = _points(name, t, N, dev)
    return N, Q, ld


class PointDistance(object):
    """Nearest points of point clouds for batches of queries."""

    def __init__(self, device=None):
        self._device = device
        self._dev = None

    def _upload(self):
        """The device, decided on first use (there are no tables to upload)."""
        if self._dev is None:
            _lib.require_gpu()
            self._dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if self._dev.index is None:
                self._dev = torch.device(self._dev.type, torch.cuda.current_device())
        return self._dev

    @property
    def device(self):
        return self._upload()

    def plan(self, N, Q, M):
        """(split, points per LDS tile, queries per workgroup) the library chooses for N samples of Q queries and M points: a
        function of the sizes."""
        out = (C.c_int32 * 3)()
        _lib.check(_lib.lib.cape_point_distance_plan(N, Q, M, out), "cape_point_distance_plan")
        return tuple(out)

    def counts(self, count, N, M):
        """``count`` checked and uploaded once, for calls in a loop: pass the result as their ``count``."""
        return _count(count, N, M, self._upload())

    def _workspace(self, N, Q, M, dev):
        need = int(_lib.lib.cape_point_distance_workspace_bytes(N, Q, M))
        if need < 0:
            _lib.check(need, "cape_point_distance_workspace_bytes")
        return torch.empty((need + 15) // 16 * 2, dtype=torch.float64, device=dev), need

    def forward(self, queries, points, count=None, out=None):
        """(d2 [N, Q], index [N, Q] int32) for ``queries`` [N, Q, 3] and ``points`` [N, M, 3] (float32 on the device; rows may
        be wider than 3 floats, the padding is never read).  ``count`` [N] integers in [0, M] (host or device; checked on the
        host), None: every row is a point.  ``out``: (d2, index) contiguous tensors to write into.  No gradient: inputs that
        require one are refused with a RuntimeError (use ``diff``)."""
        self._upload()
        for t in (queries, points):
            if torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled():
                raise RuntimeError("cape_amd.point_distance: forward only, an input requires grad (use diff)")
        return self._forward(queries, points, count, out)

    def _forward(self, queries, points, count, out):
        dev = self._upload()
        N, Q, ldq = _queries("queries", queries, dev)
        M, ldp = _points("points", points, N, dev)
        _, cnt = _count(count, N, M, dev)
        if out is None:
            out = (torch.empty((N, Q), dtype=torch.float32, device=dev), torch.empty((N, Q), dtype=torch.int32, device=dev))
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("out: (d2, index) expected")
        d2, index = out
        for name, t, dt in (("d2", d2, torch.float32), ("index", index, torch.int32)):
            if not torch.is_tensor(t) or t.dtype != dt or t.device != dev or tuple(t.shape) != (N, Q) or not t.is_contiguous():
                raise ValueError("out %s: a contiguous %s tensor %s on %s expected" % (name, dt, (N, Q), dev))
        ws, need = self._workspace(N, Q, M, dev)
        _lib.check(_lib.lib.cape_point_nearest_fwd(_p(queries), ldq, _p(points), ldp, None if cnt is None else _p(cnt), N, Q, M,
                                                   _p(index), _p(d2), _p(ws), need, _stream()), "cape_point_nearest_fwd")
        return d2, index

    def backward(self, queries, points, index, g, count=None, want_dp=True, dq=None, dp=None):
        """(dq [N, Q, 3], dp [N, M, 3] or None) for the seed ``g`` [N, Q] = dL/dd2 and a forward's ``index``.  ``dq`` is
        overwritten; ``dp`` is a fixed-order sum per point (rows at and beyond ``count`` come back zero) and is skipped, with its
        launch, when not wanted.  ``dq`` / ``dp``: where to write (rows may be wider than 3 floats, the padding is never
        written)."""
        dev = self._upload()
        N, Q, ldq = _queries("queries", queries, dev)
        M, ldp = _points("points", points, N, dev)
        _, cnt = _count(count, N, M, dev)
        if not torch.is_tensor(g) or not torch.is_tensor(index):
            raise ValueError("index, gradient: tensors expected")
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        for name, t, dt in (("index", index, torch.int32), ("gradient", g, torch.float32)):
            if t.dtype != dt or t.device != dev or tuple(t.shape) != (N, Q) or not t.is_contiguous():
                raise ValueError("%s: a contiguous %s tensor %s on %s expected" % (name, dt, (N, Q), dev))
        if dq is None:
            dq = torch.empty((N, Q, 3), dtype=torch.float32, device=dev)
        q2, lddq = _points("dq", dq, N, dev)
        if q2 != Q:
            raise ValueError("dq: %d queries for %d" % (q2, Q))
        lddp = 3
        if want_dp or dp is not None:
            if dp is None:
                dp = torch.empty((N, M, 3), dtype=torch.float32, device=dev)
            m2, lddp = _points("dp", dp, N, dev)
            if m2 != M:
                raise ValueError("dp: %d points for %d" % (m2, M))
        ws, need = self._workspace(N, Q, M, dev)
        _lib.check(_lib.lib.cape_point_nearest_bwd(_p(queries), ldq, _p(points), ldp, None if cnt is None else _p(cnt), _p(index),
                                                   _p(g), N, Q, M, _p(dq), lddq, None if dp is None else _p(dp), lddp, _p(ws),
                                                   need, _stream()), "cape_point_nearest_bwd")
        return dq, dp

    def diff(self, queries, points, count=None, return_selection=False):
        """``forward``'s d2 (bitwise the same values) as an autograd function: a gradient on it flows to ``queries`` and to
        ``points`` where they require one (a cloud that requires none costs no launch).  The chosen indices are saved, not
        recomputed, and are constants of the backward (``return_selection``: (d2, index) instead of d2); fixed-order sums, the
        same inputs give the same bits."""
        dev = self._upload()
        N, _, _ = _queries("queries", queries, dev)
        _points("points", points, N, dev)
        res = _PointDistanceFn.apply(self, queries, points, count)
        return res if return_selection else res[0]

    def np(self, queries, points):
        """``forward``, numpy in, numpy out: ``queries`` [N, Q, 3] or [Q, 3]; ``points`` [N, M, 3], [M, 3] for one query set, or
        a list of N arrays [m_n, 3] (padded to the longest; the padding is never read).  Returns (d2 [N, Q] float32,
        index [N, Q] int32)."""
        x = np.asarray(queries, dtype=np.float32)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[2] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("queries: [N, Q, 3] or [Q, 3] expected, got %s" % (x.shape,))
        x = np.ascontiguousarray(x)
        if not isinstance(points, (list, tuple)) and np.asarray(points).ndim == 2:
            points = np.asarray(points)[None]
        pts, count = pad_points(points)
        if pts.shape[0] != x.shape[0]:
            raise ValueError("points: %d samples for %d query sets" % (pts.shape[0], x.shape[0]))
        dev = self.device
        with torch.no_grad():
            out = self.forward(torch.as_tensor(x).to(dev), torch.as_tensor(pts).to(dev), count)
        return tuple(t.cpu().numpy() for t in out)

    __call__ = forward


class _PointDistanceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pd, queries, points, count):
        ctx.pd = pd
        dev = pd._upload()
        N, _, _ = _queries("queries", queries, dev)
        count = _count(count, N, points.shape[1], dev)         # checked once: the backward passes the pair on
        ctx.count = None if count[0] is None else count
        d2, index = pd._forward(queries.detach(), points.detach(), ctx.count, None)
        ctx.save_for_backward(queries, points, index)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(index)
        return d2, index

    @staticmethod
    def backward(ctx, g, _gindex=None):
        if g is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None, None
        queries, points, index = ctx.saved_tensors
        with torch.no_grad():
            dq, dp = ctx.pd.backward(queries.detach(), points.detach(), index, g, ctx.count, want_dp=ctx.needs_input_grad[2])
        return None, dq if ctx.needs_input_grad[1] else None, dp, None
