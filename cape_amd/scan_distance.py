"""Scan-to-mesh distance on the device: for every point of a raw scan the closest point of a triangle mesh's surface, for a
batch of meshes that share one topology, and its gradient (cape_amd/csrc/scan/scan_distance.hip).

  ScanDistance(faces, num_verts)         validates the triangles and uploads them once
    .forward(verts, points, count=None)  (d2 [N, M], face [N, M] int32, bary [N, M, 3]) of device vertices [N, V, 3] and device
                                         points [N, M, 3], no gradient (cape_scan_nearest_fwd: exact search over all faces)
    .diff(verts, points, count=None)     d2 as an autograd function: gradients to ``verts`` and ``points`` (cape_scan_nearest_bwd:
                                         two launches, no atomics); face and bary are saved, not recomputed
    .np(verts, points)                   numpy in, numpy out; ``points`` [N, M, 3] or a list of N arrays [m_n, 3]

``d2`` is the squared distance to the closest point ``sum_k bary_k x[face_k]``; ``count`` [N] says how many of a sample's M rows
are points (the rest is padding: face -1, d2 0, bary 0, no gradient).  A face whose evaluation is not finite never wins; a point
without a finite face, or with a non-finite coordinate, gets face -1, d2 NaN, bary 0 and no gradient.  The gradient is that of
d2 with the face and the region held constant (the envelope theorem: exact wherever d2 is differentiable).  There is no CPU
fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .vertex_normals import _p, _rows, _stream, validate_faces


def _points(name, t, N, dev):
    """(M, leading dimension) of a float32 tensor [N, M, 3] on ``dev``: contiguous, or the [:, :, :3] view of wider rows."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev:
        raise ValueError("%s: must be a float32 tensor on %s" % (name, dev))
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] != N or t.shape[1] < 1:
        raise ValueError("%s: [%d, M, 3] with M >= 1 expected, got %s" % (name, N, tuple(t.shape)))
    M, ld = int(t.shape[1]), t.stride(1)
    if t.stride(2) != 1 or ld < 3 or (N > 1 and t.stride(0) != M * ld):            # one sample: its stride is never used
        raise ValueError("%s: rows of at least 3 floats, unit stride inside a row, samples %d rows apart expected" % (name, M))
    return M, ld


def _count(count, N, M, dev):
    """(host int32 [N], device int32 [N]) of ``count``, or (None, None): integers in [0, M], one per sample.  Checked on the
    host copy; a device tensor comes to the host for that (a loop checks once: ``ScanDistance.counts``)."""
    if count is None:
        return None, None
    if isinstance(count, tuple):                               # ScanDistance.counts: checked and uploaded before
        return count
    host = count.detach().cpu().numpy() if torch.is_tensor(count) else np.asarray(count)
    if host.shape != (N,) or not np.issubdtype(host.dtype, np.integer):
        raise ValueError("count: %d integers expected, got shape %s dtype %s" % (N, host.shape, host.dtype))
    if host.min() < 0 or host.max() > M:
        raise ValueError("count: values outside [0, %d]" % M)
    host = np.ascontiguousarray(host, dtype=np.int32)
    if torch.is_tensor(count) and count.device == dev and count.dtype == torch.int32 and count.is_contiguous():
        return host, count
    return host, torch.as_tensor(host).to(dev)


def pad_points(points):
    """(float32 [N, M, 3], int32 count [N] or None) of ``points``: an array [N, M, 3] (every row a point), or a list of N arrays
    [m_n, 3] with m_n >= 1, padded with zeros to the longest."""
    if isinstance(points, (list, tuple)):
        if len(points) < 1:
            raise ValueError("points: an empty list")
        rows = []
        for n, a in enumerate(points):
            a = np.asarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
                raise ValueError("points[%d]: [m, 3] with m >= 1 expected, got %s" % (n, a.shape))
            rows.append(a)
        count = np.array([a.shape[0] for a in rows], dtype=np.int32)
        out = np.zeros((len(rows), int(count.max()), 3), np.float32)
        for n, a in enumerate(rows):
            out[n, :a.shape[0]] = a
        return out, count
    a = np.asarray(points, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("points: [N, M, 3] with M >= 1 (or a list of [m, 3] arrays) expected, got %s" % (a.shape,))
    return np.ascontiguousarray(a), None


class ScanDistance(object):
    """Closest points on meshes with the triangles ``faces`` [F, 3] over ``num_verts`` vertices."""

    def __init__(self, faces, num_verts, device=None):
        self.V = int(num_verts)
        if self.V < 1:
            raise ValueError("num_verts: %r" % (num_verts,))
        self.faces = validate_faces(faces, self.V)
        self.F = int(self.faces.shape[0])
        self._device = device
        self._dev = None

    def _upload(self):
        """(device, faces) with the triangles on the device, uploaded on first use."""
        if self._dev is None:
            _lib.require_gpu()
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            faces = torch.as_tensor(self.faces).to(dev)
            self._dev = (faces.device, faces)
        return self._dev

    @property
    def device(self):
        return self._upload()[0]

    def plan(self, N, M):
        """(split, face tile, points per workgroup) the library chooses for N samples of M points: a function of the sizes."""
        out = (C.c_int32 * 3)()
        _lib.check(_lib.lib.cape_scan_distance_plan(N, self.F, M, out), "cape_scan_distance_plan")
        return tuple(out)

    def counts(self, count, N, M):
        """``count`` checked and uploaded once, for calls in a loop: pass the result as their ``count``."""
        return _count(count, N, M, self._upload()[0])

    def _workspace(self, N, M, dev):
        need = int(_lib.lib.cape_scan_distance_workspace_bytes(N, self.V, self.F, M))
        if need < 0:
            _lib.check(need, "cape_scan_distance_workspace_bytes")
        return torch.empty((need + 15) // 16 * 2, dtype=torch.float64, device=dev), need

    def forward(self, verts, points, count=None, out=None):
        """(d2 [N, M], face [N, M] int32, bary [N, M, 3]) for ``verts`` [N, V, 3] and ``points`` [N, M, 3] (float32 on the
        tables' device; rows may be wider than 3 floats, the padding is never read).  ``count`` [N] integers in [0, M] (host or
        device; checked on the host), None: every row is a point.  ``out``: (d2, face, bary) contiguous tensors to write into.
        No gradient: inputs that require one are refused with a RuntimeError (use ``diff``)."""
        self._upload()
        for t in (verts, points):
            if torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled():
                raise RuntimeError("cape_amd.scan_distance: forward only, an input requires grad (use diff)")
        return self._forward(verts, points, count, out)

    def _forward(self, verts, points, count, out):
        dev, faces = self._upload()
        ldx = _rows("verts", verts, self.V, dev)
        N = verts.shape[0]
        M, ldp = _points("points", points, N, dev)
        _, cnt = _count(count, N, M, dev)
        if out is None:
            out = (torch.empty((N, M), dtype=torch.float32, device=dev), torch.empty((N, M), dtype=torch.int32, device=dev),
                   torch.empty((N, M, 3), dtype=torch.float32, device=dev))
        d2, face, bary = out
        for name, t, shape, dt in (("d2", d2, (N, M), torch.float32), ("face", face, (N, M), torch.int32),
                                   ("bary", bary, (N, M, 3), torch.float32)):
            if not torch.is_tensor(t) or t.dtype != dt or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("out %s: a contiguous %s tensor %s on %s expected" % (name, dt, shape, dev))
        ws, need = self._workspace(N, M, dev)
        _lib.check(_lib.lib.cape_scan_nearest_fwd(_p(verts), ldx, _p(faces), _p(points), ldp, None if cnt is None else _p(cnt), N,
                                                  self.V, self.F, M, _p(face), _p(bary), _p(d2), _p(ws), need, _stream()),
                   "cape_scan_nearest_fwd")
        return d2, face, bary

    def backward(self, verts, points, face, bary, g, want_dp=True, dx=None, dp=None):
        """(dx [N, V, 3], dp [N, M, 3] or None) for the seed ``g`` [N, M] = dL/dd2 and a forward's ``face`` / ``bary``.  ``dx``
        is overwritten.  ``dx`` / ``dp``: where to write (rows may be wider than 3 floats, the padding is never written)."""
        dev, faces = self._upload()
        ldx = _rows("verts", verts, self.V, dev)
        N = verts.shape[0]
        M, ldp = _points("points", points, N, dev)
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        for name, t, shape, dt in (("face", face, (N, M), torch.int32), ("bary", bary, (N, M, 3), torch.float32),
                                   ("gradient", g, (N, M), torch.float32)):
            if t.dtype != dt or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s: a contiguous %s tensor %s on %s expected" % (name, dt, shape, dev))
        if dx is None:
            dx = torch.empty((N, self.V, 3), dtype=torch.float32, device=dev)
        ldd = _rows("dx", dx, self.V, dev)
        if dx.shape[0] != N:
            raise ValueError("dx: %d samples for %d" % (dx.shape[0], N))
        lddp = 3
        if want_dp or dp is not None:
            if dp is None:
                dp = torch.empty((N, M, 3), dtype=torch.float32, device=dev)
            m2, lddp = _points("dp", dp, N, dev)
            if m2 != M:
                raise ValueError("dp: %d points for %d" % (m2, M))
        ws, need = self._workspace(N, M, dev)
        _lib.check(_lib.lib.cape_scan_nearest_bwd(_p(verts), ldx, _p(faces), _p(points), ldp, _p(face), _p(bary), _p(g), N, self.V,
                                                  self.F, M, _p(dx), ldd, None if dp is None else _p(dp), lddp, _p(ws), need,
                                                  _stream()), "cape_scan_nearest_bwd")
        return dx, dp

    def diff(self, verts, points, count=None, return_selection=False):
        """``forward``'s d2 (bitwise the same values) as an autograd function: a gradient on it flows to ``verts`` and to
        ``points`` where they require one.  The chosen faces and barycentrics are saved, not recomputed, and are constants of
        the backward (``return_selection``: (d2, face, bary) instead of d2); fixed-order sums, the same inputs give the same
        bits."""
        dev = self._upload()[0]
        _rows("verts", verts, self.V, dev)
        _points("points", points, verts.shape[0], dev)
        res = _ScanDistanceFn.apply(self, verts, points, count)
        return res if return_selection else res[0]

    def np(self, verts, points):
        """``forward``, numpy in, numpy out: ``verts`` [N, V, 3] or [V, 3]; ``points`` [N, M, 3], [M, 3] for one mesh, or a
        list of N arrays [m_n, 3] (padded to the longest; the padding comes back as face -1, d2 0, bary 0).  Returns
        (d2 [N, M] float32, face [N, M] int32, bary [N, M, 3] float32)."""
        v = np.asarray(verts, dtype=np.float32)
        x = np.ascontiguousarray(v.reshape(-1, self.V, 3))
        if not isinstance(points, (list, tuple)) and np.asarray(points).ndim == 2:
            points = np.asarray(points)[None]
        pts, count = pad_points(points)
        if pts.shape[0] != x.shape[0]:
            raise ValueError("points: %d samples for %d meshes" % (pts.shape[0], x.shape[0]))
        dev = self.device
        with torch.no_grad():
            out = self.forward(torch.as_tensor(x).to(dev), torch.as_tensor(pts).to(dev), count)
        return tuple(t.cpu().numpy() for t in out)

    __call__ = forward


class _ScanDistanceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sd, verts, points, count):
        ctx.sd = sd
        d2, face, bary = sd._forward(verts.detach(), points.detach(), count, None)
        ctx.save_for_backward(verts, points, face, bary)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(face, bary)
        return d2, face, bary

    @staticmethod
    def backward(ctx, g, _gface=None, _gbary=None):
        if g is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None, None
        verts, points, face, bary = ctx.saved_tensors
        with torch.no_grad():
            dx, dp = ctx.sd.backward(verts.detach(), points.detach(), face, bary, g, want_dp=ctx.needs_input_grad[2])
        return None, dx if ctx.needs_input_grad[1] else None, dp, None
