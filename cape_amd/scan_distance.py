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

``forward``, ``diff`` and ``np`` also take ``normals`` [N, M, 3] (one per point) and ``cos_min``, both or neither: a face then takes
part in a point's minimum only if the dot product of the point's normal (as given, not normalised) and the face's unit normal is
at least ``cos_min`` (decided in fp32 inside the search, cape_scan_nearest_compat_fwd).  A point without a compatible
face, or with a non-finite normal, gets face -1, d2 NaN, bary 0 and no gradient; normals take no gradient.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._device import check_tensor, ptr as _p, resolve_device, rows, stream as _stream, workspace
from .vertex_normals import validate_faces


def point_rows(name, t, N, dev):
    """(M, leading dimension) of a float32 tensor [N, M, 3] on ``dev``, by the rules of ``_device.rows``."""
    return rows(name, t, dev, N=N)[1:]


def check_count(count, N, M, dev):
    """(host int32 [N], device int32 [N]) of ``count``, or (None, None): integers in [0, M], one per sample.  Checked on the
    host copy; a device tensor comes to the host for that (a loop checks once: ``NearestDistance.counts``)."""
    if count is None:
        return None, None
    if isinstance(count, tuple):                               # NearestDistance.counts: checked and uploaded before
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


_points, _count = point_rows, check_count                      # the names the host tests import


def pad_points(points, name="points"):
    """(float32 [N, M, 3], int32 count [N] or None) of ``points``: an array [N, M, 3] (every row a point), or a list of N arrays
    [m_n, 3] with m_n >= 1, padded with zeros to the longest."""
    if isinstance(points, (list, tuple)):
        if len(points) < 1:
            raise ValueError("%s: an empty list" % name)
        rows = []
        for n, a in enumerate(points):
            a = np.asarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
                raise ValueError("%s[%d]: [m, 3] with m >= 1 expected, got %s" % (name, n, a.shape))
            rows.append(a)
        count = np.array([a.shape[0] for a in rows], dtype=np.int32)
        out = np.zeros((len(rows), int(count.max()), 3), np.float32)
        for n, a in enumerate(rows):
            out[n, :a.shape[0]] = a
        return out, count
    a = np.asarray(points, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("%s: [N, M, 3] with M >= 1 (or a list of [m, 3] arrays) expected, got %s" % (name, a.shape))
    return np.ascontiguousarray(a), None


def pad_normals(name, normals, pts, count):
    """float32 [N, M, 3]: ``normals``, one per point of what ``pad_points`` returned as (``pts``, ``count``) -- an array of
    ``pts``' shape ([M, 3] for one sample), or a list of N arrays [m_n, 3] padded with zeros exactly as the points were."""
    if not isinstance(normals, (list, tuple)) and np.asarray(normals).ndim == 2:
        normals = np.asarray(normals)[None]
    out, cnt = pad_points(normals, name)
    full = lambda c: np.full(pts.shape[0], pts.shape[1], np.int32) if c is None else c
    if out.shape != pts.shape or not np.array_equal(full(cnt), full(count)):
        raise ValueError("%s: one normal per point expected (%s, rows %s), got %s, rows %s"
                         % (name, pts.shape, full(count).tolist(), out.shape, full(cnt).tolist()))
    return out


class NearestDistance(object):
    """What the two directions of the nearest search share: the device and the tables on it, decided and
    uploaded on first use; ``count``; the workspace; ``forward``'s refusal of gradients; ``diff``; the point half of ``np``;
    the normal-compatibility arguments (``compat``: None, or what ``_compat`` returned).
    A direction is a subclass: its names (``_module``, ``_samples``), its ``_workspace_bytes`` entry, its host ``_tables``, and
    ``_sizes``, ``_forward``, ``backward``, ``_grads`` and ``_first_np`` -- what it checks, launches and returns -- and the public
    ``forward`` / ``diff`` / ``np`` with its own names for the normals."""

    _module = _samples = _workspace_bytes = None
    _tables = ()
    _first_normals = None                                      # the name of the normals that belong to ``first``, if any

    def __init__(self, device=None):
        self._device = device
        self._dev = None

    def _upload(self):
        """(device, tables...) with the host ``_tables`` on the device, decided and uploaded on first use."""
        if self._dev is None:
            _lib.require_gpu()
            dev = resolve_device(self._device)
            self._dev = (dev,) + tuple(torch.as_tensor(a).to(dev) for a in self._tables)
        return self._dev

    @property
    def device(self):
        return self._upload()[0]

    def counts(self, count, N, M):
        """``count`` checked and uploaded once, for calls in a loop: pass the result as their ``count``."""
        return check_count(count, N, M, self.device)

    def _workspace(self, dev, *sizes):
        return workspace(self._workspace_bytes(*sizes), dev, self._workspace_bytes.__name__)

    def _points_grad(self, dp, want_dp, N, M, dev):
        """(dp, its leading dimension) for the gradient to the points: allocated when wanted and not given; (None, 3) when not
        wanted."""
        if dp is None and not want_dp:
            return None, 3
        if dp is None:
            dp = torch.empty((N, M, 3), dtype=torch.float32, device=dev)
        m2, lddp = point_rows("dp", dp, N, dev)
        if m2 != M:
            raise ValueError("dp: %d points for %d" % (m2, M))
        return dp, lddp

    @staticmethod
    def _compat(cos_min, **normals):
        """None when neither ``cos_min`` nor a normals tensor is given (the plain search); (cos_min, normals...) when all are.
        Some but not all, a NaN ``cos_min``: ValueError; normals that require a gradient: RuntimeError (they take none)."""
        given = [v is not None for v in normals.values()] + [cos_min is not None]
        if not any(given):
            return None
        if not all(given):
            raise ValueError("%s and cos_min: all of them or none" % ", ".join(normals))
        cos_min = float(cos_min)
        if cos_min != cos_min:
            raise ValueError("cos_min: NaN")
        for name, t in normals.items():
            if torch.is_tensor(t) and t.requires_grad:
                raise RuntimeError("%s: normals take no gradient, this tensor requires one" % name)
        return (cos_min,) + tuple(normals.values())

    @staticmethod
    def _normal_rows(name, t, N, R, dev):
        """The leading dimension of the normals [N, R, 3], checked by the row rules of the points."""
        return rows(name, t, dev, N=N, R=R)[2]

    def forward(self, first, points, count=None, out=None, compat=None):
        """The distances and the selection of ``first`` (the subclass's vertices or queries) against ``points`` [N, M, 3]:
        float32 on the device; rows may be wider than 3 floats, the padding is never read.  ``count`` [N] integers in [0, M]
        (host or device; checked on the host), None: every row is a point.  ``out``: contiguous tensors to write into.  No
        gradient: inputs that require one are refused with a RuntimeError (use ``diff``)."""
        self._upload()
        for t in (first, points):
            if torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled():
                raise RuntimeError("cape_amd.%s: forward only, an input requires grad (use diff)" % self._module)
        return self._forward(first, points, count, out, compat)

    def diff(self, first, points, count=None, return_selection=False, compat=None):
        """``forward``'s d2 (bitwise the same values) as an autograd function: a gradient on it flows to ``first`` and to
        ``points`` where they require one (points that require none cost nothing).  The selection is saved, not recomputed,
        and is a constant of the backward (``return_selection``: all of ``forward``'s tensors instead of d2); fixed-order
        sums, the same inputs give the same bits."""
        self._sizes(first, points, self.device)
        res = _NearestFn.apply(self, first, points, count, compat)
        return res if return_selection else res[0]

    def np(self, first, points, cos_min=None, **normals):
        """``forward``, numpy in, numpy out: ``points`` [N, M, 3], [M, 3] for one sample, or a list of N arrays [m_n, 3]
        (padded to the longest); normals of the points in the same form, padded as the points are."""
        x = self._first_np(first)
        if not isinstance(points, (list, tuple)) and np.asarray(points).ndim == 2:
            points = np.asarray(points)[None]
        pts, count = pad_points(points)
        if pts.shape[0] != x.shape[0]:
            raise ValueError("points: %d samples for %d %s" % (pts.shape[0], x.shape[0], self._samples))
        if self._compat(cos_min, **normals) is not None:
            for name, a in normals.items():
                if name == self._first_normals:
                    a = np.asarray(a, dtype=np.float32)
                    if a.size != x.size:
                        raise ValueError("%s: one normal per row of the %s expected, got %s" % (name, self._samples, a.shape))
                    normals[name] = np.ascontiguousarray(a.reshape(x.shape))
                else:
                    normals[name] = pad_normals(name, a, pts, count)
        dev = self.device
        kw = {name: None if a is None else torch.as_tensor(a).to(dev) for name, a in normals.items()}
        with torch.no_grad():
            out = self.forward(torch.as_tensor(x).to(dev), torch.as_tensor(pts).to(dev), count, cos_min=cos_min, **kw)
        return tuple(t.cpu().numpy() for t in out)


class _NearestFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, first, points, count, compat):
        ctx.owner = owner
        # checked once: the backward passes the pair on (``diff`` has checked the shapes)
        count = check_count(count, first.shape[0], points.shape[1], owner.device)
        ctx.count = None if count[0] is None else count
        res = owner._forward(first.detach(), points.detach(), ctx.count, None, compat)
        ctx.save_for_backward(first, points, *res[1:])
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*res[1:])
        return res

    @staticmethod
    def backward(ctx, g, *_):
        if g is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None, None, None
        first, points, *selection = ctx.saved_tensors
        with torch.no_grad():
            d_first, d_points = ctx.owner._grads(first.detach(), points.detach(), selection, g, ctx.count, ctx.needs_input_grad[2])
        return None, d_first if ctx.needs_input_grad[1] else None, d_points, None, None


class ScanDistance(NearestDistance):
    """Closest points on meshes with the triangles ``faces`` [F, 3] over ``num_verts`` vertices.  ``forward(verts, points)``:
    (d2 [N, M], face [N, M] int32, bary [N, M, 3]) for ``verts`` [N, V, 3]; ``np`` takes ``verts`` [N, V, 3] or [V, 3] and
    returns the padding as face -1, d2 0, bary 0."""

    _module, _samples, _workspace_bytes = "scan_distance", "meshes", _lib.lib.cape_scan_distance_workspace_bytes

    def __init__(self, faces, num_verts, device=None):
        NearestDistance.__init__(self, device)
        self.V = int(num_verts)
        if self.V < 1:
            raise ValueError("num_verts: %r" % (num_verts,))
        self.faces = validate_faces(faces, self.V)
        self.F = int(self.faces.shape[0])
        self._tables = (self.faces,)

    def plan(self, N, M):
        """(split, face tile, points per workgroup) the library chooses for N samples of M points: a function of the sizes."""
        out = (C.c_int32 * 3)()
        _lib.check(_lib.lib.cape_scan_distance_plan(N, self.F, M, out), "cape_scan_distance_plan")
        return tuple(out)

    def _sizes(self, verts, points, dev):
        """(N, V, M, leading dimensions of ``verts`` and ``points``), checked."""
        N, V, ldx = rows("verts", verts, dev, R=self.V)
        _, M, ldp = rows("points", points, dev, N=N)
        return N, V, M, ldx, ldp

    def forward(self, verts, points, count=None, out=None, normals=None, cos_min=None):
        """``NearestDistance.forward``; ``normals`` [N, M, 3] (float32 on the device, by the row rules of ``points``; the
        padding rows are never read) and ``cos_min``, both or neither: only the faces whose unit normal has a dot product of at
        least ``cos_min`` with the point's normal take part (cape_scan_nearest_compat_fwd)."""
        return NearestDistance.forward(self, verts, points, count, out, self._compat(cos_min, normals=normals))

    __call__ = forward

    def diff(self, verts, points, count=None, return_selection=False, normals=None, cos_min=None):
        """``NearestDistance.diff``; ``normals`` and ``cos_min`` as in ``forward``.  Normals take no gradient."""
        return NearestDistance.diff(self, verts, points, count, return_selection, self._compat(cos_min, normals=normals))

    def np(self, verts, points, normals=None, cos_min=None):
        """``NearestDistance.np``; ``normals`` in the form of ``points`` (an array, or a list of [m_n, 3] arrays)."""
        return NearestDistance.np(self, verts, points, cos_min, normals=normals)

    def _forward(self, verts, points, count, out, compat=None):
        dev, faces = self._upload()
        N, V, M, ldx, ldp = self._sizes(verts, points, dev)
        if compat is not None:
            ldn = self._normal_rows("normals", compat[1], N, M, dev)
        _, cnt = check_count(count, N, M, dev)
        if out is None:
            out = (torch.empty((N, M), dtype=torch.float32, device=dev), torch.empty((N, M), dtype=torch.int32, device=dev),
                   torch.empty((N, M, 3), dtype=torch.float32, device=dev))
        d2, face, bary = out
        check_tensor("out d2", d2, torch.float32, (N, M), dev)
        check_tensor("out face", face, torch.int32, (N, M), dev)
        check_tensor("out bary", bary, torch.float32, (N, M, 3), dev)
        if compat is not None:
            entry = _lib.lib.cape_scan_distance_compat_workspace_bytes
            ws, need = workspace(entry(N, V, self.F, M), dev, entry.__name__)
            _lib.check(_lib.lib.cape_scan_nearest_compat_fwd(_p(verts), ldx, _p(faces), _p(points), ldp, _p(compat[1]), ldn,
                                                             compat[0], _p(cnt), N, V, self.F, M, _p(face), _p(bary), _p(d2),
                                                             _p(ws), need, _stream()), "cape_scan_nearest_compat_fwd")
            return d2, face, bary
        ws, need = self._workspace(dev, N, V, self.F, M)
        _lib.check(_lib.lib.cape_scan_nearest_fwd(_p(verts), ldx, _p(faces), _p(points), ldp, _p(cnt), N, V, self.F, M, _p(face),
                                                  _p(bary), _p(d2), _p(ws), need, _stream()), "cape_scan_nearest_fwd")
        return d2, face, bary

    def backward(self, verts, points, face, bary, g, want_dp=True, dx=None, dp=None):
        """(dx [N, V, 3], dp [N, M, 3] or None) for the seed ``g`` [N, M] = dL/dd2 and a forward's ``face`` / ``bary``.  ``dx``
        is overwritten.  ``dx`` / ``dp``: where to write (rows may be wider than 3 floats, the padding is never written)."""
        dev, faces = self._upload()
        N, V, M, ldx, ldp = self._sizes(verts, points, dev)
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        check_tensor("face", face, torch.int32, (N, M), dev)
        check_tensor("bary", bary, torch.float32, (N, M, 3), dev)
        check_tensor("gradient", g, torch.float32, (N, M), dev)
        if dx is None:
            dx = torch.empty((N, V, 3), dtype=torch.float32, device=dev)
        n2, _, ldd = rows("dx", dx, dev, R=V)
        if n2 != N:
            raise ValueError("dx: %d samples for %d" % (n2, N))
        dp, lddp = self._points_grad(dp, want_dp, N, M, dev)
        ws, need = self._workspace(dev, N, V, self.F, M)
        _lib.check(_lib.lib.cape_scan_nearest_bwd(_p(verts), ldx, _p(faces), _p(points), ldp, _p(face), _p(bary), _p(g), N, V,
                                                  self.F, M, _p(dx), ldd, _p(dp), lddp, _p(ws), need, _stream()),
                   "cape_scan_nearest_bwd")
        return dx, dp

    def _grads(self, verts, points, selection, g, count, want_dp):
        return self.backward(verts, points, selection[0], selection[1], g, want_dp=want_dp)

    def _first_np(self, verts):
        return np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, self.V, 3))
