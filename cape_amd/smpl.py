"""SMPL posing on the device: the step after ``decode`` that turns CAPE's rest-pose clothing displacements into posed clothed
bodies (reference demos.py:155-161, 207-213 and :249-331, which go through ``smplx`` one mesh at a time on the CPU).

  load_smpl_model(path)      an SMPL model file (.npz, or a chumpy-free .pkl) -> ``SMPL`` with its arrays on the device
  SMPL.forward(...)          batched forward pass on torch device tensors (libcape_hip.so cape_smpl_joints / cape_smpl_skin)
  SMPL.forward_diff(...)     the same as an autograd function: gradients to the rest body, pose, betas and translation
                             (cape_smpl_skin_bwd / cape_smpl_joints_bwd / cape_smpl_jreg_bwd)
  SMPL.pose(...)             the same on numpy arrays
  SMPL.unpose(...)           the inverse of ``forward``: posed vertices + pose -> the rest body and its joints
                             (cape_smpl_unpose_joints / cape_smpl_unpose_skin); ``unpose_np`` on numpy arrays
  SMPL.vertex_normals(...)   per-vertex normals of meshes in the model's topology (``cape_amd.vertex_normals`` on the model's
                             ``faces``); ``vertex_normals_diff`` with a gradient, ``vertex_normals_np`` on numpy arrays
  SMPL.scan_distance(...)    squared distance and closest point of raw scan points to meshes in the model's topology
                             (``cape_amd.scan_distance``); ``scan_distance_diff`` with a gradient, ``scan_distance_np`` on numpy
  SMPL.point_distance(...)   the opposite direction: squared distance of every vertex to the nearest raw scan point
                             (``cape_amd.point_distance``); ``point_distance_diff`` with a gradient, ``point_distance_np`` on numpy
  dress(...)                 de-normalise + clothing mask + minimal body (cape_smpl_dress)
  undress(...)               its right-inverse: rest body -> normalised displacements (cape_smpl_undress)
  dress_diff(...)            the same with a gradient to the displacements (cape_smpl_dress_bwd)
  weighted_l2(...)           per-sample weighted squared distance to target meshes and its gradient (cape_smpl_weighted_l2)
  create(...), body_models   an ``smplx``-compatible factory: with a one-line ``smplx.py`` in the reference checkout
                             (``from cape_amd.smpl import body_models``) demos.py poses through the device unchanged

The joints are regressed from the rest body the caller passes -- in demos.py the CLOTHED body, because it overwrites the
model's ``v_template`` with it.  There is no CPU fallback.  ``forward`` and ``dress`` carry no gradient (``forward`` refuses
inputs that require one); ``forward_diff`` and ``dress_diff`` are the differentiable forms, hand-derived backward kernels
behind ``torch.autograd.Function``s that save their inputs only.
"""
import ctypes as C
import os
import pickle
import types

import numpy as np
import torch

from . import _lib
from ._device import ptr as _p, resolve_device, stream as _stream

MAX_JOINTS = 64


# ---- model files ----------------------------------------------------------------------------------------------------------
def _dense(a):
    return a.toarray() if hasattr(a, "toarray") else np.asarray(a)


def read_model_file(path):
    """The arrays of an SMPL model file as a dict of numpy arrays / scipy sparse matrices (SMPL key names)."""
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
        if "J_regressor_data" in d:            # a sparse J_regressor saved as its CSR parts
            import scipy.sparse as sp
            d["J_regressor"] = sp.csr_matrix((d.pop("J_regressor_data"), d.pop("J_regressor_indices"),
                                              d.pop("J_regressor_indptr")), shape=tuple(d.pop("J_regressor_shape")))
        return d
    with open(path, "rb") as fh:
        try:
            d = pickle.load(fh, encoding="latin1")
        except ModuleNotFoundError as e:
            if "chumpy" in str(e):
                raise ValueError(
                    "%s stores its arrays as chumpy objects, which cape_amd does not read. Convert it once where chumpy is "
                    "installed: load it with pickle (encoding='latin1'), replace every chumpy array x by np.array(x), and "
                    "pickle the dict again (or np.savez it with the same keys)." % path) from None
            raise
    return dict(d)


def _model_arrays(d, num_betas):
    for k in ("v_template", "J_regressor", "weights", "posedirs", "shapedirs", "kintree_table", "f"):
        if k not in d:
            raise KeyError("SMPL model: missing array %r" % k)
    vt = np.asarray(d["v_template"], dtype=np.float64)
    V = vt.shape[0]
    parents = np.asarray(d["kintree_table"])[0].astype(np.int64)
    parents[parents == 4294967295] = -1                  # the files store parents[0] = -1 as uint32
    J = len(parents)
    if not 1 <= J <= MAX_JOINTS:
        raise ValueError("SMPL model: %d joints (1..%d supported)" % (J, MAX_JOINTS))
    if parents[0] != -1 or any(not 0 <= parents[j] < j for j in range(1, J)):
        raise ValueError("SMPL model: the kinematic tree is not parent-ordered (parents[j] < j); reordering a file's joints "
                         "is not supported")
    import scipy.sparse as sp
    jreg = sp.csr_matrix(d["J_regressor"], dtype=np.float64)
    jreg.sum_duplicates()
    jreg.sort_indices()
    W = _dense(d["weights"]).astype(np.float64)
    posedirs = np.asarray(d["posedirs"], dtype=np.float64)
    shapedirs = np.asarray(_dense(d["shapedirs"]), dtype=np.float64)
    if (jreg.shape != (J, V) or W.shape != (V, J) or vt.shape != (V, 3) or posedirs.shape != (V, 3, 9 * (J - 1))
            or shapedirs.ndim != 3 or shapedirs.shape[:2] != (V, 3)):
        raise ValueError("SMPL model: inconsistent array shapes")
    B = min(int(num_betas), shapedirs.shape[2])
    return dict(v_template=vt, J_regressor=jreg, weights=W, posedirs=posedirs, shapedirs=shapedirs[:, :, :B],
                parents=parents, faces=np.asarray(d["f"]).astype(np.int64), J=J, V=V, B=B)


def load_smpl_model(path, num_betas=10, device=None):
    """Read an SMPL model file (.npz with the SMPL key names, or a chumpy-free .pkl) and upload it: ``SMPL``."""
    return SMPL(read_model_file(path), num_betas=num_betas, device=device)


class SMPL(object):
    """An SMPL body model with its arrays in the device layouts of include/cape_hip.h ("SMPL posing")."""

    def __init__(self, arrays, num_betas=10, device=None):
        m = _model_arrays(arrays, num_betas)
        self._device = device
        self.J, self.V, self.num_betas = m["J"], m["V"], m["B"]
        self.parents = m["parents"]
        self.faces = m["faces"]
        self.v_template_np = m["v_template"]
        self.host = m                                     # float64 host arrays (tests, the compat object)
        J, V = self.J, self.V
        jreg = m["J_regressor"]
        rp, ci = jreg.indptr.astype(np.int32), jreg.indices.astype(np.int32)
        _lib.check(_lib.lib.cape_csr_validate(J, V, int(jreg.nnz), rp.ctypes.data_as(C.c_void_p),
                                              ci.ctypes.data_as(C.c_void_p)), "SMPL J_regressor")
        # skinning weights: ELL of the nonzeros in increasing joint order, padded with (joint 0, 0.0); planar [W][V]
        nz = m["weights"] != 0
        width = max(1, int(nz.sum(1).max()))
        ell_j = np.zeros((width, V), np.int32)
        ell_w = np.zeros((width, V), np.float32)
        for v in range(V):
            js = np.flatnonzero(nz[v])
            ell_j[:len(js), v] = js
            ell_w[:len(js), v] = m["weights"][v, js]
        self.ell_width = width
        # [shapedirs | posedirs] planar [K][3][V]: lanes of a wave load consecutive words of one coefficient's plane
        basis = np.concatenate([m["shapedirs"].transpose(2, 1, 0), m["posedirs"].transpose(2, 1, 0)], 0)
        jsd = np.einsum("jv,vcb->bjc", jreg.toarray(), m["shapedirs"])          # J_regressor . shapedirs, [B][J][3]
        # J_regressor . posedirs, [9(J-1)][J][3]: the pose blend's share of the regressed joints, which unposing takes out
        jpd = np.asarray(jreg @ m["posedirs"].reshape(V, -1)).reshape(J, 3, 9 * (J - 1)).transpose(2, 0, 1)
        # the regressor's transpose for the backward's gather per vertex: CSC of [J, V] = CSR of [V, J]
        jt = jreg.T.tocsr()
        jt.sort_indices()
        tp, ti = jt.indptr.astype(np.int32), jt.indices.astype(np.int32)
        _lib.check(_lib.lib.cape_csr_validate(V, J, int(jt.nnz), tp.ctypes.data_as(C.c_void_p),
                                              ti.ctypes.data_as(C.c_void_p)), "SMPL J_regressor (transposed)")
        self.layouts = dict(rowptr=(rp, np.int32), colidx=(ci, np.int32), vals=(jreg.data, np.float32),
                            ell_j=(ell_j, np.int32), ell_w=(ell_w, np.float32), basis=(basis, np.float32),
                            jshapedirs=(jsd, np.float32), jposedirs=(jpd, np.float32), v_template=(m["v_template"], np.float32),
                            jt_colptr=(tp, np.int32), jt_rowidx=(ti, np.int32), jt_vals=(jt.data, np.float32))
        self._dev = None
        self._normals = None
        self._scan = None
        self._point = None
        self._parents_c = (C.c_int32 * J)(*[int(x) for x in self.parents])

    @property
    def device(self):
        return self._upload().device

    def _upload(self):
        """The device arrays, uploaded on first use (a model can be read and inspected without a GPU)."""
        if self._dev is None:
            _lib.require_gpu()
            dev = resolve_device(self._device)
            self._dev = types.SimpleNamespace(device=dev, **{k: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
                                                             for k, (a, dt) in self.layouts.items()})
        return self._dev

    @property
    def basis_bytes(self):
        return self.layouts["basis"][0].size * 4

    def _arguments(self, verts, pose, betas, transl, grad):
        """forward's argument checks; ``betas`` comes back padded to the model's shape rows (or None)."""
        J, V, d = self.J, self.V, self._upload()
        if verts is None:
            verts = d.v_template[None]
        pose = pose.reshape(pose.shape[0], -1)
        N = pose.shape[0]
        for name, t in (("verts", verts), ("pose", pose), ("betas", betas), ("transl", transl)):
            if t is None:
                continue
            if t.requires_grad and not grad:
                raise RuntimeError("cape_amd.smpl: forward only, %s requires grad" % name)
            if t.dtype != torch.float32 or t.device != d.device or not t.is_contiguous():
                raise ValueError("cape_amd.smpl: %s must be a contiguous float32 tensor on %s" % (name, d.device))
        if pose.shape[1] != 3 * J:
            raise ValueError("pose: %d values per sample, the model has %d joints" % (pose.shape[1], J))
        if verts.dim() != 3 or verts.shape[1:] != (V, 3) or verts.shape[0] not in (1, N):
            raise ValueError("verts: [%d or 1, %d, 3] expected, got %s" % (N, V, tuple(verts.shape)))
        if betas is not None:
            betas = betas.reshape(N, -1)
            B = betas.shape[1]
            if B > self.num_betas:
                raise ValueError("betas: %d given, the model keeps %d" % (B, self.num_betas))
            if B == 0:
                betas = None
            elif B < self.num_betas:      # the basis keeps the model's shape rows in front of the pose rows: pad with zeros
                betas = torch.cat([betas, betas.new_zeros((N, self.num_betas - B))], 1)
        if transl is not None and tuple(transl.shape) not in ((N, 3),):
            raise ValueError("transl: [%d, 3] expected" % N)
        return verts, pose, betas, transl

    def _basis(self, B):
        """The blend basis for B shape rows: with no betas it starts past the model's shape rows."""
        return C.c_void_p(self._dev.basis.data_ptr() + 4 * 3 * self.V * (self.num_betas - B))

    def _joints(self, verts, pose, betas, transl, jo):
        """cape_smpl_joints on checked arguments: (coef, G), the posed joints into ``jo`` (None: not wanted)."""
        J, V, d, N = self.J, self.V, self._dev, pose.shape[0]
        B = 0 if betas is None else betas.shape[1]
        coef = torch.empty((N, B + 9 * (J - 1)), dtype=torch.float32, device=d.device)
        G = torch.empty((N, J, 12), dtype=torch.float32, device=d.device)
        _lib.check(_lib.lib.cape_smpl_joints(_p(verts), 0 if verts.shape[0] == 1 else 3 * V, _p(d.rowptr), _p(d.colidx),
                                             _p(d.vals), _p(pose), _p(betas), B, _p(d.jshapedirs), _p(transl),
                                             self._parents_c, J, V, N, _p(coef), _p(G), _p(jo), _stream()), "cape_smpl_joints")
        return coef, G

    def _body_argument(self, name, t, N):
        """The checks ``_arguments`` makes on ``verts``, for another body of the call (``joints_from``)."""
        d = self._upload()
        if t.requires_grad:
            raise RuntimeError("cape_amd.smpl: forward only, %s requires grad" % name)
        if t.dtype != torch.float32 or t.device != d.device or not t.is_contiguous():
            raise ValueError("cape_amd.smpl: %s must be a contiguous float32 tensor on %s" % (name, d.device))
        if t.dim() != 3 or t.shape[1:] != (self.V, 3) or t.shape[0] not in (1, N):
            raise ValueError("%s: [%d or 1, %d, 3] expected, got %s" % (name, N, self.V, tuple(t.shape)))
        return t

    def _launch(self, verts, pose, betas, transl, out, joints_from=None):
        J, V, d, N = self.J, self.V, self._dev, pose.shape[0]
        if out is None:
            out = (torch.empty((N, V, 3), dtype=torch.float32, device=d.device),
                   torch.empty((N, J, 3), dtype=torch.float32, device=d.device))
        vo, jo = out
        if tuple(vo.shape) != (N, V, 3) or tuple(jo.shape) != (N, J, 3) or not (vo.is_contiguous() and jo.is_contiguous()):
            raise ValueError("out: contiguous [N,V,3] and [N,J,3] float32 tensors expected")
        coef, G = self._joints(verts if joints_from is None else joints_from, pose, betas, transl, jo)
        _lib.check(_lib.lib.cape_smpl_skin(_p(verts), 0 if verts.shape[0] == 1 else 3 * V, self._basis(coef.shape[1] - 9 * (J - 1)),
                                           coef.shape[1], _p(coef), _p(G), _p(d.ell_j), _p(d.ell_w), self.ell_width, _p(transl),
                                           J, V, N, _p(vo), 3 * V, _stream()), "cape_smpl_skin")
        return vo, jo

    def forward(self, verts, pose, betas=None, transl=None, out=None, joints_from=None):
        """Pose N meshes.  ``verts`` [N,V,3] or [1,V,3] (one rest body for every pose; None: the template), ``pose`` [N,J*3]
        axis-angle (joint 0 = global orientation), ``betas`` [N,<=B], ``transl`` [N,3]: float32 tensors on this model's device.
        Returns (vertices [N,V,3], joints [N,J,3]); with ``out`` = that pair preallocated, nothing synchronises the host, so
        the call can be captured in a graph.  No gradient: see ``forward_diff``.  ``joints_from`` [N or 1, V, 3]: regress the
        joints from that body (plus the shape term) instead of from ``verts``; None is the forward as it always was."""
        verts, pose, betas, transl = self._arguments(verts, pose, betas, transl, grad=False)
        if joints_from is not None:
            joints_from = self._body_argument("joints_from", joints_from, pose.shape[0])
        return self._launch(verts, pose, betas, transl, out=out, joints_from=joints_from)

    def unpose_workspace(self, N):
        """A workspace for ``unpose`` of N samples with ``joints_from=None`` (cape_smpl_unpose_workspace_bytes)."""
        nbytes = _lib.lib.cape_smpl_unpose_workspace_bytes(self.J, N)
        _lib.check(min(nbytes, 0), "cape_smpl_unpose_workspace_bytes")
        return torch.empty((nbytes // 8,), dtype=torch.float64, device=self.device)

    def unpose(self, posed, pose, betas=None, transl=None, joints_from=None, out=None, det_min=None, workspace=None):
        """The inverse of ``forward``: ``posed`` [N,V,3] vertices in this model's topology and the ``pose`` / ``betas`` /
        ``transl`` they were posed with (as in ``forward``) -> (rest [N,V,3], rest_joints [N,J,3]), the rest body with
        ``forward(rest, pose, betas, transl) = posed`` and the joints ``forward`` regresses from it.
        ``joints_from=None`` is the exact inverse: the joints depend on the unknown rest body, one 3J x 3J solve per sample
        finds them (cape_smpl_unpose_joints, fp64).  ``joints_from`` [N or 1, V, 3] takes them from that body instead
        (cape_smpl_joints), which inverts ``forward(..., joints_from=that body)``; against the plain forward it is off by
        as far as the two bodies' joints differ (centimetres for a template body under clothing).
        ``det_min`` [N] float32 (optional) receives min_v |det| of the blended skinning rotations: near zero the pose has
        collapsed some vertex's transform and the rest body is ill-determined there.  With ``out`` = the returned pair and
        ``workspace`` (``unpose_workspace(N)``) preallocated, nothing synchronises the host.  No gradient."""
        posed, pose, betas, transl = self._arguments(posed, pose, betas, transl, grad=False)
        J, V, d, N = self.J, self.V, self._dev, pose.shape[0]
        if posed.shape[0] != N:
            raise ValueError("posed: [%d, %d, 3] expected, got %s" % (N, V, tuple(posed.shape)))
        if out is None:
            out = (torch.empty((N, V, 3), dtype=torch.float32, device=d.device),
                   torch.empty((N, J, 3), dtype=torch.float32, device=d.device))
        to, jo = out
        if tuple(to.shape) != (N, V, 3) or tuple(jo.shape) != (N, J, 3) or not (to.is_contiguous() and jo.is_contiguous()):
            raise ValueError("out: contiguous [N,V,3] and [N,J,3] float32 tensors expected")
        if det_min is not None and (det_min.dtype != torch.float32 or tuple(det_min.shape) != (N,) or det_min.device != d.device
                                    or not det_min.is_contiguous()):
            raise ValueError("det_min: a contiguous float32 [%d] tensor on %s expected" % (N, d.device))
        B = 0 if betas is None else betas.shape[1]
        if joints_from is None:
            ws = self.unpose_workspace(N) if workspace is None else workspace
            coef = torch.empty((N, B + 9 * (J - 1)), dtype=torch.float32, device=d.device)
            G = torch.empty((N, J, 12), dtype=torch.float32, device=d.device)
            _lib.check(_lib.lib.cape_smpl_unpose_joints(_p(posed), 3 * V, _p(d.rowptr), _p(d.colidx), _p(d.vals), _p(d.ell_j),
                                                        _p(d.ell_w), self.ell_width, _p(pose), _p(betas), B, _p(d.jposedirs),
                                                        _p(transl), self._parents_c, J, V, N, _p(ws),
                                                        ws.numel() * ws.element_size(), _p(coef), _p(G), _p(jo), None,
                                                        _p(det_min), _stream()), "cape_smpl_unpose_joints")
        else:
            joints_from = self._body_argument("joints_from", joints_from, N)
            coef, G = self._joints(joints_from, pose, betas, transl, None)
            self._joints(joints_from, torch.zeros_like(pose), betas, None, jo)       # zero pose: the posed joints are the rest joints
            if det_min is not None:
                det_min.fill_(float("inf"))
        _lib.check(_lib.lib.cape_smpl_unpose_skin(_p(posed), 3 * V, self._basis(B), coef.shape[1], _p(coef), _p(G), _p(d.ell_j),
                                                  _p(d.ell_w), self.ell_width, _p(transl), J, V, N, _p(to), 3 * V, _p(det_min),
                                                  _stream()), "cape_smpl_unpose_skin")
        return to, jo

    def unpose_np(self, posed, pose, betas=None, transl=None, joints_from=None):
        """``unpose``, numpy in, numpy out: (rest [N,V,3], rest_joints [N,J,3]) float32."""
        t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(self.device)
        with torch.no_grad():
            pose = np.asarray(pose).reshape(-1, 3 * self.J)
            posed = np.asarray(posed).reshape(-1, self.V, 3)
            jf = None if joints_from is None else np.asarray(joints_from).reshape(-1, self.V, 3)
            to, jo = self.unpose(t(posed), t(pose), t(betas), t(transl), joints_from=t(jf))
            return to.cpu().numpy(), jo.cpu().numpy()

    def forward_diff(self, verts, pose, betas=None, transl=None, joints_from=None):
        """``forward`` (same arguments, same checks, bitwise the same values) as an autograd function: gradients on the returned
        vertices and / or joints flow to whichever of ``verts`` ([1,V,3]: summed over the samples), ``pose``, ``betas`` and
        ``transl`` require them.  The inputs are all that is saved; backward recomputes the joint transforms.  The backward
        kernels assume the joints come from ``verts``: ``joints_from`` is refused."""
        if joints_from is not None:
            raise NotImplementedError("cape_amd.smpl: forward_diff has no joints_from (use forward, which carries no gradient)")
        verts, pose, betas, transl = self._arguments(verts, pose, betas, transl, grad=True)
        return _PoseFn.apply(self, verts, pose, betas, transl)

    def _backward(self, verts, pose, betas, transl, gV, gJ, need):
        """(dT, dpose, dbetas, dtransl) for the wanted ones of ``need`` (four flags), None for the others."""
        J, V, d, N = self.J, self.V, self._dev, pose.shape[0]
        lib, s = _lib.lib, _stream()
        need_T, need_pose, need_betas, need_transl = need
        need_betas = need_betas and betas is not None
        need_transl = need_transl and transl is not None
        if (gV is None and gJ is None) or not (need_T or need_pose or need_betas or need_transl):
            return None, None, None, None
        B = 0 if betas is None else betas.shape[1]
        K = B + 9 * (J - 1)
        tss = 0 if verts.shape[0] == 1 else 3 * V
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=d.device)
        ws, blocks, q, need_coef = None, 0, None, bool(need_pose or need_betas)
        if gV is not None:
            gV = gV.contiguous()
            coef, G = self._joints(verts, pose, betas, transl, None)
            plan = (C.c_int32 * 3)()
            _lib.check(lib.cape_smpl_skin_bwd_plan(K, J, V, N, plan), "cape_smpl_skin_bwd_plan")
            blocks = int(plan[1])
            ws = new(N * blocks * int(plan[2]))
            q = new(N, V, 3) if need_T else None
            _lib.check(lib.cape_smpl_skin_bwd(_p(verts), tss, self._basis(B), K, _p(coef), _p(G), _p(d.ell_j), _p(d.ell_w),
                                              self.ell_width, _p(gV), 3 * V, J, V, N, int(need_coef), _p(q), 3 * V, _p(ws),
                                              4 * ws.numel(), s), "cape_smpl_skin_bwd")
        if gJ is not None:
            gJ = gJ.contiguous()
        dpose = new(N, 3 * J) if need_pose else None
        dbetas = new(N, B) if need_betas else None
        dtransl = new(N, 3) if need_transl else None
        dJn = new(N, J, 3) if need_T else None
        _lib.check(lib.cape_smpl_joints_bwd(_p(verts), tss, _p(d.rowptr), _p(d.colidx), _p(d.vals), _p(pose), _p(betas), B,
                                            _p(d.jshapedirs), self._parents_c, J, V, N, _p(gJ), _p(ws), blocks, int(need_coef),
                                            _p(dpose), _p(dbetas), _p(dtransl), _p(dJn), s), "cape_smpl_joints_bwd")
        dT = None
        if need_T:
            dT = new(verts.shape[0], V, 3)
            _lib.check(lib.cape_smpl_jreg_bwd(_p(q), 3 * V, _p(d.jt_colptr), _p(d.jt_rowidx), _p(d.jt_vals), _p(dJn), J, V, N,
                                              int(verts.shape[0] == 1), _p(dT), 3 * V, s), "cape_smpl_jreg_bwd")
        return dT, dpose, dbetas, dtransl

    __call__ = forward

    def _vertex_normals(self):
        """``VertexNormals`` on the model's own ``faces``, validated and uploaded on first use (a model whose faces are not a
        valid triangle list still poses)."""
        if self._normals is None:
            from .vertex_normals import VertexNormals
            self._normals = VertexNormals(self.faces, self.V, device=self._device)
        return self._normals

    def vertex_normals(self, verts, out=None):
        """Per-vertex normals [N, V, 3] of device meshes ``verts`` [N, V, 3] in the model's topology -- posed or not -- as
        ``cape_amd.vertex_normals.VertexNormals.forward`` computes them (uniform weights; no gradient)."""
        return self._vertex_normals().forward(verts, out)

    def vertex_normals_diff(self, verts):
        """``vertex_normals`` as an autograd function: gradients on the normals flow to ``verts``."""
        return self._vertex_normals().diff(verts)

    def vertex_normals_np(self, verts):
        """``vertex_normals``, numpy in, numpy out."""
        return self._vertex_normals().np(verts)

    def _scan_distance(self):
        """``ScanDistance`` on the model's own ``faces``, validated and uploaded on first use."""
        if self._scan is None:
            from .scan_distance import ScanDistance
            self._scan = ScanDistance(self.faces, self.V, device=self._device)
        return self._scan

    def scan_distance(self, verts, points, count=None, out=None, normals=None, cos_min=None):
        """(d2 [N, M], face [N, M], bary [N, M, 3]): for every device scan point ``points`` [N, M, 3] the squared distance to,
        and the closest point on, the device meshes ``verts`` [N, V, 3] in the model's topology, as
        ``cape_amd.scan_distance.ScanDistance.forward`` computes them (no gradient).  ``normals`` [N, M, 3] and ``cos_min``,
        both or neither: only the faces whose normal agrees with the point's that far are searched."""
        return self._scan_distance().forward(verts, points, count, out, normals, cos_min)

    def scan_distance_diff(self, verts, points, count=None, normals=None, cos_min=None):
        """``scan_distance``'s d2 as an autograd function: gradients on it flow to ``verts`` and ``points``."""
        return self._scan_distance().diff(verts, points, count, normals=normals, cos_min=cos_min)

    def scan_distance_np(self, verts, points, normals=None, cos_min=None):
        """``scan_distance``, numpy in (``points`` and ``normals`` an array or a list of [m_n, 3] arrays), numpy out."""
        return self._scan_distance().np(verts, points, normals, cos_min)

    def _point_distance(self):
        """``PointDistance`` on the model's device, constructed on first use."""
        if self._point is None:
            from .point_distance import PointDistance
            self._point = PointDistance(device=self._device)
        return self._point

    def _query_normals(self, verts, point_normals):
        """The vertex normals of ``verts`` for the normal-compatible search (no gradient); None without ``point_normals``."""
        if point_normals is None:
            return None
        with torch.no_grad():
            return self.vertex_normals(verts.detach())

    def point_distance(self, verts, points, count=None, out=None, point_normals=None, cos_min=None):
        """(d2 [N, V], index [N, V] int32): for every vertex of ``verts`` [N, V, 3] the squared distance to the nearest of
        ``points`` [N, M, 3] (``count`` [N]: how many rows of a sample are points) and that point's index, as
        ``cape_amd.point_distance.PointDistance.forward`` computes them (no gradient).  ``point_normals`` [N, M, 3] and
        ``cos_min``, both or neither: only the points whose normal agrees that far with the vertex's
        (``vertex_normals(verts)``) are searched."""
        return self._point_distance().forward(verts, points, count, out, self._query_normals(verts, point_normals),
                                              point_normals, cos_min)

    def point_distance_diff(self, verts, points, count=None, point_normals=None, cos_min=None):
        """``point_distance``'s d2 as an autograd function: gradients on it flow to ``verts`` and ``points``; the vertex
        normals of the filter are constants."""
        return self._point_distance().diff(verts, points, count, query_normals=self._query_normals(verts, point_normals),
                                           point_normals=point_normals, cos_min=cos_min)

    def point_distance_np(self, verts, points, point_normals=None, cos_min=None):
        """``point_distance``, numpy in (``points`` and ``point_normals`` an array or a list of [m_n, 3] arrays), numpy out."""
        qn = None if point_normals is None else self.vertex_normals_np(np.asarray(verts, dtype=np.float32).reshape(-1, self.V, 3))
        return self._point_distance().np(verts, points, qn, point_normals, cos_min)

    def pose(self, verts, pose, betas=None, transl=None):
        """numpy in, numpy out: (vertices [N,V,3], joints [N,J,3]) float32."""
        t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(self.device)
        with torch.no_grad():
            pose = np.asarray(pose).reshape(-1, 3 * self.J)
            verts = None if verts is None else np.asarray(verts).reshape(-1, self.V, 3)
            vo, jo = self.forward(t(verts), t(pose), t(betas), t(transl))
            return vo.cpu().numpy(), jo.cpu().numpy()


class _PoseFn(torch.autograd.Function):
    """SMPL.forward_diff: the forward entries, and in backward the kernels of csrc/smpl/smpl_bwd.hip on the saved inputs."""

    @staticmethod
    def forward(ctx, model, verts, pose, betas, transl):
        vo, jo = model._launch(verts.detach(), pose.detach(), None if betas is None else betas.detach(),
                               None if transl is None else transl.detach(), None)
        ctx.model = model
        ctx.has = (betas is not None, transl is not None)
        ctx.save_for_backward(*[t for t in (verts, pose, betas, transl) if t is not None])
        ctx.set_materialize_grads(False)
        return vo, jo

    @staticmethod
    def backward(ctx, gV, gJ):
        saved = list(ctx.saved_tensors)
        verts, pose = saved[0], saved[1]
        betas = saved[2] if ctx.has[0] else None
        transl = saved[-1] if ctx.has[1] else None
        with torch.no_grad():
            return (None,) + ctx.model._backward(verts, pose, betas, transl, gV, gJ, ctx.needs_input_grad[1:5])


class _DressFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, arrays, disp):
        ctx.arrays = arrays
        ctx.set_materialize_grads(False)
        return arrays(disp.detach())

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[1]:
            return None, None
        a, g = ctx.arrays, g.contiguous()
        out = torch.empty_like(g)
        _lib.check(_lib.lib.cape_smpl_dress_bwd(_p(g), 3 * a.V, _p(a.std), _p(a.mask), _p(out), 3 * a.V, g.shape[0], a.V,
                                                _stream()), "cape_smpl_dress_bwd")
        return None, out


# ---- dress ---------------------------------------------------------------------------------------------------------------
class _DressArrays(object):
    """mean / std / minimal [V,3] and the clothing mask [V] on the device, uploaded once."""

    def __init__(self, mean, std, clothing_idx, minimal_shape, V, device):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        self.every_vertex = clothing_idx is None
        mask = np.ones(V, np.float32) if self.every_vertex else np.zeros(V, np.float32)
        if not self.every_vertex:
            mask[np.asarray(clothing_idx, dtype=np.int64)] = 1.0
        self.mean, self.std = dev(np.reshape(mean, (V, 3))), dev(np.reshape(std, (V, 3)))
        self.minimal, self.mask = dev(np.reshape(minimal_shape, (V, 3))), dev(mask)
        self.V = V

    def __call__(self, disp, out=None):
        N, V = disp.shape[0], self.V
        if disp.dtype != torch.float32 or not disp.is_contiguous() or tuple(disp.shape[1:]) != (V, 3):
            raise ValueError("disp: contiguous float32 [N, %d, 3] expected" % V)
        if out is None:
            out = torch.empty((N, V, 3), dtype=torch.float32, device=disp.device)
        _lib.check(_lib.lib.cape_smpl_dress(_p(disp), 3 * V, _p(self.mean), _p(self.std), _p(self.mask), _p(self.minimal),
                                            _p(out), 3 * V, N, V, _stream()), "cape_smpl_dress")
        return out

    def undress(self, T, out=None):
        """The right-inverse of the call: (mask * (T - minimal) - mean) / std (cape_smpl_undress)."""
        N, V = T.shape[0], self.V
        if T.dtype != torch.float32 or not T.is_contiguous() or tuple(T.shape[1:]) != (V, 3):
            raise ValueError("T: contiguous float32 [N, %d, 3] expected" % V)
        if out is None:
            out = torch.empty((N, V, 3), dtype=torch.float32, device=T.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (N, V, 3) or not out.is_contiguous():
            raise ValueError("out: contiguous float32 [%d, %d, 3] expected" % (N, V))
        _lib.check(_lib.lib.cape_smpl_undress(_p(T), 3 * V, _p(self.mean), _p(self.std), None if self.every_vertex else _p(self.mask),
                                              _p(self.minimal), _p(out), 3 * V, N, V, _stream()), "cape_smpl_undress")
        return out

    def diff(self, disp):
        """The same with a gradient to ``disp``: mask * std * the incoming gradient (cape_smpl_dress_bwd)."""
        if disp.dtype != torch.float32 or not disp.is_contiguous() or tuple(disp.shape[1:]) != (self.V, 3):
            raise ValueError("disp: contiguous float32 [N, %d, 3] expected" % self.V)
        return _DressFn.apply(self, disp)


def dress(disp, mean, std, clothing_idx, minimal_shape):
    """demos.py:155-161: ``minimal_shape + mask(clothing_idx) * (disp * std + mean)`` for a device tensor ``disp`` [N,V,3];
    the other arguments are host arrays.  Returns the clothed rest bodies [N,V,3] on the device."""
    return _DressArrays(mean, std, clothing_idx, minimal_shape, disp.shape[1], disp.device)(disp)


def undress(T, mean, std, clothing_idx, minimal_shape):
    """The way back from ``dress`` (reference lib/prep_data.py:74 packs ``v_cano - minimal`` for training):
    ``(mask(clothing_idx) * (T - minimal_shape) - mean) / std`` for a device tensor ``T`` [N,V,3] of rest bodies; the other
    arguments are host arrays, ``clothing_idx=None`` means every vertex.  ``dress(undress(T))`` is ``T`` on the clothing
    vertices and ``minimal_shape`` elsewhere.  Returns the normalised displacements [N,V,3] on the device."""
    return _DressArrays(mean, std, clothing_idx, minimal_shape, T.shape[1], T.device).undress(T)


def dress_diff(disp, mean, std, clothing_idx, minimal_shape):
    """``dress`` with a gradient to ``disp``."""
    return _DressArrays(mean, std, clothing_idx, minimal_shape, disp.shape[1], disp.device).diff(disp)


def weighted_l2(posed, target, w, inv_wsum, n, loss_out, grad_out=None):
    """The data term of ``CAPE.fit_posed`` for the first ``n`` samples of ``posed`` / ``target`` (contiguous float32 [N,V,3] on
    the device, ``w`` [V]): loss_out[i] = inv_wsum * sum_v w_v |posed_iv - target_iv|^2, and into ``grad_out`` [N,V,3] (None:
    not wanted) its gradient to ``posed``, 2 inv_wsum w_v (posed - target).  Rows from ``n`` on are left as they are."""
    V = posed.shape[1]
    _lib.check(_lib.lib.cape_smpl_weighted_l2(_p(posed), 3 * V, _p(target), 3 * V, _p(w), inv_wsum, n, V, _p(loss_out),
                                              _p(grad_out), 3 * V, _stream()), "cape_smpl_weighted_l2")


# ---- smplx-compatible factory (demos.py:22-24, 267-283, 312-326) -------------------------------------------------------------
class _Output(object):
    def __init__(self, vertices, joints):
        self.vertices = vertices
        self.joints = joints


class SMPLLayer(object):
    """What demos.py touches of an ``smplx.SMPL``: writable CPU float32 ``v_template`` [V,3], ``body_pose`` [1,3(J-1)],
    ``global_orient`` [1,3], ``transl`` [1,3], ``betas`` [1,B] and ``faces``; calling it poses on the device and returns
    ``.vertices`` [1,V,3] and ``.joints`` [1,J,3].  ``.joints`` holds the J skeleton joints only, not the extra vertex
    joints smplx appends."""

    def __init__(self, model):
        self.model = model
        self.faces = model.faces
        self.v_template = torch.tensor(model.v_template_np, dtype=torch.float32)
        self.body_pose = torch.zeros((1, 3 * (model.J - 1)), dtype=torch.float32)
        self.global_orient = torch.zeros((1, 3), dtype=torch.float32)
        self.transl = torch.zeros((1, 3), dtype=torch.float32)
        self.betas = torch.zeros((1, model.num_betas), dtype=torch.float32)

    def __call__(self, betas=None, body_pose=None, global_orient=None, transl=None, **kw):
        m = self.model
        d = lambda t, default: (default if t is None else t).detach().to(device=m.device, dtype=torch.float32).contiguous()
        with torch.no_grad():
            pose = torch.cat([d(global_orient, self.global_orient).reshape(1, 3),
                              d(body_pose, self.body_pose).reshape(1, -1)], 1).contiguous()
            vo, jo = m.forward(d(None, self.v_template)[None], pose, d(betas, self.betas).reshape(1, -1),
                               d(transl, self.transl).reshape(1, 3))
        return _Output(vo, jo)

    forward = __call__


def create(model_path, model_type="smpl", gender="neutral", ext="pkl", num_betas=10, device=None, **kw):
    """``smplx.create`` for SMPL: ``model_path`` is a model file, or a folder holding ``smpl/SMPL_<GENDER>.<ext>``."""
    if model_type.lower() != "smpl":
        raise ValueError("cape_amd.smpl.create: only model_type='smpl' is supported, not %r" % model_type)
    path = model_path
    if os.path.isdir(path):
        sub = os.path.join(path, model_type.lower())
        path = os.path.join(sub if os.path.isdir(sub) else path, "SMPL_%s.%s" % (gender.upper(), ext))
    if not os.path.exists(path):
        raise FileNotFoundError("SMPL model file not found: %s" % path)
    return SMPLLayer(load_smpl_model(path, num_betas=num_betas, device=device))


class body_models(object):
    """``smplx.body_models`` namespace: ``body_models.create(...)`` as demos.py:22 calls it."""
    create = staticmethod(create)
