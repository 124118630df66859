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

``forward``, ``diff`` and ``np`` also take ``query_normals`` [N, Q, 3], ``point_normals`` [N, M, 3] and ``cos_min``, all or none: a
point then takes part in a query's minimum only if the dot product of the two normals (as given, not normalised) is at least
``cos_min`` (decided in fp32 inside the search, cape_point_nearest_compat_fwd).  A query without a compatible point,
and a normal with a non-finite component on either side, give index -1, d2 NaN and no gradient; normals take no gradient.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._device import check_tensor, ptr as _p, rows, stream as _stream
from .scan_distance import NearestDistance, check_count, pad_points, point_rows

_points, _count = point_rows, check_count                      # the names the host tests import (with pad_points)


def _queries(name, t, dev):
    """(N, Q, leading dimension) of a float32 tensor [N, Q, 3] on ``dev``, by the rules of ``_device.rows``."""
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[0] < 1:
        raise ValueError("%s: a float32 tensor [N, Q, 3] on %s expected" % (name, dev))
    return rows(name, t, dev, N=int(t.shape[0]))


class PointDistance(NearestDistance):
    """Nearest points of point clouds for batches of queries: no topology, nothing to upload.  ``forward(queries, points)``:
    (d2 [N, Q], index [N, Q] int32) for ``queries`` [N, Q, 3]; ``np`` takes ``queries`` [N, Q, 3] or [Q, 3]."""

    _module, _samples, _workspace_bytes = "point_distance", "query sets", _lib.lib.cape_point_distance_workspace_bytes

    def plan(self, N, Q, M):
        """(split, points per LDS tile, queries per workgroup) the library chooses for N samples of Q queries and M points: a
        function of the sizes."""
        out = (C.c_int32 * 3)()
        _lib.check(_lib.lib.cape_point_distance_plan(N, Q, M, out), "cape_point_distance_plan")
        return tuple(out)

    def _sizes(self, queries, points, dev):
        """(N, Q, M, leading dimensions of ``queries`` and ``points``), checked."""
        N, Q, ldq = _queries("queries", queries, dev)
        _, M, ldp = rows("points", points, dev, N=N)
        return N, Q, M, ldq, ldp

    _first_normals = "query_normals"

    def forward(self, queries, points, count=None, out=None, query_normals=None, point_normals=None, cos_min=None):
        """``NearestDistance.forward``; ``query_normals`` [N, Q, 3], ``point_normals`` [N, M, 3] (float32 on the device, by the
        row rules of ``points``; the padding rows are never read) and ``cos_min``, all or none: only the points whose normal
        has a dot product of at least ``cos_min`` with the query's take part (cape_point_nearest_compat_fwd)."""
        return NearestDistance.forward(self, queries, points, count, out,
                                       self._compat(cos_min, query_normals=query_normals, point_normals=point_normals))

    __call__ = forward

    def diff(self, queries, points, count=None, return_selection=False, query_normals=None, point_normals=None, cos_min=None):
        """``NearestDistance.diff``; the normals and ``cos_min`` as in ``forward``.  Normals take no gradient."""
        return NearestDistance.diff(self, queries, points, count, return_selection,
                                    self._compat(cos_min, query_normals=query_normals, point_normals=point_normals))

    def np(self, queries, points, query_normals=None, point_normals=None, cos_min=None):
        """``NearestDistance.np``; ``query_normals`` in the shape of ``queries``, ``point_normals`` in the form of ``points``."""
        return NearestDistance.np(self, queries, points, cos_min, query_normals=query_normals, point_normals=point_normals)

    def _forward(self, queries, points, count, out, compat=None):
        dev = self._upload()[0]
        N, Q, M, ldq, ldp = self._sizes(queries, points, dev)
        if compat is not None:
            ldqn = self._normal_rows("query_normals", compat[1], N, Q, dev)
            ldpn = self._normal_rows("point_normals", compat[2], N, M, dev)
        _, cnt = check_count(count, N, M, dev)
        if out is None:
            out = (torch.empty((N, Q), dtype=torch.float32, device=dev), torch.empty((N, Q), dtype=torch.int32, device=dev))
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("out: (d2, index) expected")
        d2, index = out
        check_tensor("out d2", d2, torch.float32, (N, Q), dev)
        check_tensor("out index", index, torch.int32, (N, Q), dev)
        ws, need = self._workspace(dev, N, Q, M)
        if compat is not None:
            _lib.check(_lib.lib.cape_point_nearest_compat_fwd(_p(queries), ldq, _p(points), ldp, _p(compat[1]), ldqn, _p(compat[2]),
                                                              ldpn, compat[0], _p(cnt), N, Q, M, _p(index), _p(d2), _p(ws), need,
                                                              _stream()), "cape_point_nearest_compat_fwd")
            return d2, index
        _lib.check(_lib.lib.cape_point_nearest_fwd(_p(queries), ldq, _p(points), ldp, _p(cnt), N, Q, M, _p(index), _p(d2), _p(ws),
                                                   need, _stream()), "cape_point_nearest_fwd")
        return d2, index

    def backward(self, queries, points, index, g, count=None, want_dp=True, dq=None, dp=None):
        """(dq [N, Q, 3], dp [N, M, 3] or None) for the seed ``g`` [N, Q] = dL/dd2 and a forward's ``index``.  ``dq`` is
        overwritten; ``dp`` is a fixed-order sum per point (rows at and beyond ``count`` come back zero) and is skipped, with its
        launch, when not wanted.  ``dq`` / ``dp``: where to write (rows may be wider than 3 floats, the padding is never
        written)."""
        dev = self._upload()[0]
        N, Q, M, ldq, ldp = self._sizes(queries, points, dev)
        _, cnt = check_count(count, N, M, dev)
        if not torch.is_tensor(g) or not torch.is_tensor(index):
            raise ValueError("index, gradient: tensors expected")
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        check_tensor("index", index, torch.int32, (N, Q), dev)
        check_tensor("gradient", g, torch.float32, (N, Q), dev)
        if dq is None:
            dq = torch.empty((N, Q, 3), dtype=torch.float32, device=dev)
        q2, lddq = point_rows("dq", dq, N, dev)
        if q2 != Q:
            raise ValueError("dq: %d queries for %d" % (q2, Q))
        dp, lddp = self._points_grad(dp, want_dp, N, M, dev)
        ws, need = self._workspace(dev, N, Q, M)
        _lib.check(_lib.lib.cape_point_nearest_bwd(_p(queries), ldq, _p(points), ldp, _p(cnt), _p(index), _p(g), N, Q, M, _p(dq),
                                                   lddq, _p(dp), lddp, _p(ws), need, _stream()), "cape_point_nearest_bwd")
        return dq, dp

    def _grads(self, queries, points, selection, g, count, want_dp):
        return self.backward(queries, points, selection[0], g, count, want_dp=want_dp)

    def _first_np(self, queries):
        x = np.asarray(queries, dtype=np.float32)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[2] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("queries: [N, Q, 3] or [Q, 3] expected, got %s" % (x.shape,))
        return np.ascontiguousarray(x)
