"""Per-vertex normals on the device for any triangle mesh: the reference's ``estimate_vertex_normals`` (lib/losses.py:54-80,
its restatement of psbody.mesh's routine; nothing in the reference calls it) for a batch of meshes that share one topology.

  VertexNormals(faces, num_verts)   validates the triangles, builds the vertex -> incident-corner table and uploads both once
    .forward(verts, out=None)       normals [N, V, 3] of device vertices [N, V, 3], no gradient (cape_vertex_normals_fwd)
    .diff(verts)                    the same as an autograd function (cape_vertex_normals_bwd: two launches, no atomics)
    .np(verts)                      numpy in, numpy out

The normal of a vertex is the normalised sum of the UNIT normals of its faces -- uniform weights, as psbody.mesh and the
reference have it.  Area weighting is the one-line variant that sums the unnormalised cross products instead; it is not
implemented.  A degenerate face adds nothing, a vertex without faces gets a zero normal.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from ._device import ptr as _p, resolve_device, rows, stream as _stream
from .graph import vertex_face_table


def validate_faces(faces, num_verts):
    """``faces`` as a contiguous int32 [F, 3] array, or ValueError: (F, 3) integers in [0, num_verts), no vertex twice in a
    face (what ``lambda_normal`` asks of its faces)."""
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError("faces: shape %s, expected (F, 3)" % (f.shape,))
    if not np.issubdtype(f.dtype, np.integer):
        raise ValueError("faces: dtype %s, expected integers" % f.dtype)
    if f.min() < 0 or f.max() >= num_verts:
        raise ValueError("faces: vertex indices outside [0, %d)" % num_verts)
    if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any():
        raise ValueError("faces: a face names the same vertex twice")
    return np.ascontiguousarray(f, dtype=np.int32)


def _rows(name, t, V, dev):
    """The leading dimension of a float32 tensor [N, V, 3] on ``dev``, by the rules of ``_device.rows``."""
    return rows(name, t, dev, R=V)[2]


class VertexNormals(object):
    """Vertex normals of meshes with the triangles ``faces`` [F, 3] over ``num_verts`` vertices."""

    def __init__(self, faces, num_verts, device=None):
        self.V = int(num_verts)
        if self.V < 1:
            raise ValueError("num_verts: %r" % (num_verts,))
        self.faces = validate_faces(faces, self.V)
        self.F = int(self.faces.shape[0])
        self.vptr, self.vidx = vertex_face_table(self.faces, self.V)
        self._device = device
        self._dev = None

    def _upload(self):
        """(device, faces, vptr, vidx) with the tables on the device, uploaded on first use."""
        if self._dev is None:
            _lib.require_gpu()
            dev = resolve_device(self._device)
            self._dev = (dev,) + tuple(torch.as_tensor(a).to(dev) for a in (self.faces, self.vptr, self.vidx))
        return self._dev

    @property
    def device(self):
        return self._upload()[0]

    def forward(self, verts, out=None):
        """Normals [N, V, 3] of ``verts`` [N, V, 3] (float32 on the device; rows may be wider than 3 floats, the padding is never
        read).  ``out``: where to write them (likewise; padding never written).  Both must live on the tables' device
        (ValueError otherwise, nothing is launched).  No gradient: ``verts`` that require one are refused with a RuntimeError,
        as ``SMPL.forward`` refuses them (use ``diff``)."""
        self._upload()
        if torch.is_tensor(verts) and verts.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("cape_amd.vertex_normals: forward only, verts requires grad (use diff)")
        return self._forward(verts, out)

    def _forward(self, verts, out):
        dev, faces, vptr, vidx = self._upload()
        ldx = _rows("verts", verts, self.V, dev)
        N = verts.shape[0]
        if out is None:
            out = torch.empty((N, self.V, 3), dtype=torch.float32, device=dev)
        ldn = _rows("out", out, self.V, dev)
        if out.shape[0] != N:
            raise ValueError("out: %d samples for %d" % (out.shape[0], N))
        _lib.check(_lib.lib.cape_vertex_normals_fwd(_p(verts), ldx, _p(faces), _p(vptr), _p(vidx), N, self.V, self.F, _p(out), ldn,
                                                    _stream()), "cape_vertex_normals_fwd")
        return out

    def _backward(self, verts, g):
        dev, faces, vptr, vidx = self._upload()
        N = verts.shape[0]
        ldx = _rows("verts", verts, self.V, dev)
        g = g.to(device=dev, dtype=torch.float32)            # autograd hands over what the consumer produced: bring it here
        if tuple(g.shape) != (N, self.V, 3):
            raise ValueError("gradient: [%d, %d, 3] expected, got %s" % (N, self.V, tuple(g.shape)))
        if g.stride(2) != 1 or g.stride(1) < 3 or g.stride(0) != self.V * g.stride(1):
            g = g.contiguous()
        dx = torch.empty((N, self.V, 3), dtype=torch.float32, device=dev)
        need = int(_lib.lib.cape_vertex_normals_workspace_bytes(N, self.V))
        if need < 0:
            _lib.check(need, "cape_vertex_normals_workspace_bytes")
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib.cape_vertex_normals_bwd(_p(verts), ldx, _p(g), g.stride(1), _p(faces), _p(vptr), _p(vidx), N,
                                                    self.V, self.F, _p(dx), 3, _p(ws), need, _stream()), "cape_vertex_normals_bwd")
        return dx

    def diff(self, verts):
        """``forward`` (bitwise the same values) as an autograd function: a gradient on the normals flows to ``verts`` when it
        requires one.  ``verts`` is all that is saved; backward recomputes the sums (two launches, fixed-order sums: the same
        inputs give the same bits)."""
        _rows("verts", verts, self.V, self._upload()[0])
        return _VertexNormalsFn.apply(self, verts)

    def np(self, verts):
        """``forward``, numpy in ([N, V, 3] or [V, 3]), numpy out (float32, the input's shape)."""
        a = np.asarray(verts, dtype=np.float32)
        x = torch.as_tensor(np.ascontiguousarray(a.reshape(-1, self.V, 3))).to(self.device)
        with torch.no_grad():
            return self.forward(x).cpu().numpy().reshape(a.shape)

    __call__ = forward


class _VertexNormalsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vn, verts):
        ctx.vn = vn
        ctx.save_for_backward(verts)
        ctx.set_materialize_grads(False)
        return vn._forward(verts.detach(), None)

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[1]:
            return None, None
        verts, = ctx.saved_tensors
        with torch.no_grad():
            dx = ctx.vn._backward(verts.detach(), g)
        return None, dx
