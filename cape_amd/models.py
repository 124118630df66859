"""``CAPE`` -- Mesh-CVAE + mesh-patch discriminator on MI355X, API-compatible with the
reference's ``lib.models.CAPE`` (reference lib/models.py:13-64, 230-351, 837-1174).

Drop-in contract: same constructor keywords, ``build_graph(input_num_verts,
nn_input_channel, phase)``, ``fit``, ``encode``, ``encode_only_condition``, ``predict``,
``evaluate``, ``decode`` with numpy in / numpy out, static ``batch_size`` with zero padding,
operators selected by NAME (``filter='chebyshev5'``, ``activation='b1leakyrelu'|...``,
``pool/unpool='poolwT'``; :58-62).  Variables carry the TF variable names of the reference's
scopes and the reference's layouts (conv weight ``[Fin*K, Fout]`` with
row ``fin*K+k``; dense kernels ``[in, out]``), so a converted TF checkpoint can be loaded by
name.  All mesh-tensor arithmetic runs in the HIP kernels (cape_amd.ops); PyTorch is the
autograd / optimizer shell.  There is no CPU fallback.
"""
import collections
import contextlib
import weakref
import glob
import os
import shutil
import time

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from . import _lib
from . import tf_checkpoint
from .graph import ConvOperators, HostCSR, is_identity, vertex_edge_table, vertex_face_table
from .load_data import load_pack

_ACTIVATIONS = ("b1leakyrelu", "b1relu", "b1tanh", "b2relu")


def _trunc_normal(rng, shape, std=0.1):
    out = rng.standard_normal(int(np.prod(shape)))
    bad = np.abs(out) > 2.0
    while bad.any():
        out[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(out) > 2.0
    return (std * out).reshape(shape).astype(np.float32)


class _Series(object):
    """The per-sample series of a fit's batch: one zeroed [steps + 1, batch_size] device tensor per name (``name=dtype``); a
    step writes its row (``series[name][step]``), ``numpy(nb)`` returns the valid columns [:, :nb] by name."""

    def __init__(self, steps, batch_size, device, **dtypes):
        self._rows = {k: torch.zeros((steps + 1, batch_size), dtype=dt, device=device) for k, dt in dtypes.items()}

    def __getitem__(self, name):
        return self._rows[name]

    def numpy(self, nb):
        return {k: t[:, :nb].cpu().numpy() for k, t in self._rows.items()}


class base_model(object):
    """Reference lib/models.py:13-227: hyper-parameters, operator name binding, variables."""

    def __init__(self, L, D, U, F=None, K=None, p=None, nz=18, loss='l1', nn_input_channel=3,
                 filter='chebyshev5', activation='b1leakyrelu', pool='poolwT',
                 unpool='poolwT', num_epochs=60, lr=0.008, decay_rate=0.99,
                 optimizer='sgd', decay_steps=None, momentum=0.9, cond_dim=0, nz_cond=0,
                 regularization=0, batch_size=32, seed=123,
                 lambda_recon=1.0, lambda_edge=0.0, lambda_latent=1e-3,
                 restart=False, name='', loss_mask=None, project_dir=None, device=None, lambda_normal=0.0, faces=None,
                 **ignored):
        self.seed = seed
        self.input_num_verts = L[0].shape[0]
        self.nn_input_channel = nn_input_channel
        self.name = name
        self.restart = restart
        self.Laplacian, self.Downsample_mtx, self.Upsample_mtx, self.p = L, D, U, p
        self.out_channels = F
        self.poly_order = K
        self.which_loss = loss
        self.num_epochs, self.learning_rate = num_epochs, lr
        self.decay_rate, self.decay_steps, self.momentum = decay_rate, decay_steps, momentum
        self.regularization = regularization
        self.batch_size = batch_size
        self.optimizer = optimizer
        self.plot_latent = False
        self.project_dir = project_dir or os.getcwd()
        self.device = torch.device(device) if device is not None else torch.device("cuda:0")

        # template vertices + SMPL edge list (reference :44-45 reads data/template_mesh.obj and
        # data/edges_smpl.npy next to lib/); a CAPE checkout at project_dir wins, else the pack.
        self.verts_ref, self.vpe = self._load_template()

        # loss_mask (reference :47-52): 'binary' reads the shipped per-vertex weights; any other string or None is the
        # reference's else branch.  _loss_mask_w: the [V, 3] float32 weights, None without a mask.
        self._loss_mask_w = self._resolve_loss_mask(loss_mask)
        if self._loss_mask_w is None:
            self.loss_mask = 1.0
        else:
            # what the reference meant to build (:49-50): the weights repeated over the batch
            self.loss_mask = np.repeat(self._loss_mask_w[np.newaxis], batch_size, 0)
            self._loss_mask_sum = float(self._loss_mask_w.astype(np.float64).sum())      # one sample's sum of weights

        # lambda_normal: weight of the face-normal loss (lib/losses.py:27-52, unwired in the reference).  0 = off:
        # no file is read and no table is built.  _faces: the [F, 3] int32 triangles, None when off.
        self.lambda_normal, self._faces = self._resolve_normal(lambda_normal, faces)

        self.nz = nz
        self.cond_dim = cond_dim
        self.nz_cond = nz_cond

        # operator plug-points resolved by name, like getattr(self, name) at reference :58-62
        for opname in (filter, activation, pool, unpool):
            if not hasattr(self, opname):
                raise AttributeError("'%s' object has no attribute '%s'" % (type(self).__name__, opname))
        self.filter = getattr(self, filter)
        self.brelu = getattr(self, activation)
        self.pool = getattr(self, pool)
        self.unpool = getattr(self, unpool)
        self._activation_name = activation

        self.lambda_l1, self.lambda_edge, self.lambda_latent = lambda_recon, lambda_edge, lambda_latent

        self._vars = collections.OrderedDict()     # TF variable name -> torch Parameter
        self._kinds = {}
        self._scope = []
        self._ops_cache = {}
        self._csr_cache = {}
        self._init_rng = np.random.default_rng(seed)
        self._grad_views = {}      # TF variable name -> view of the flat gradient bucket (train phase)
        self._grad_views_d = {}    # the same for the discriminator variables, used while D runs as a single merged pass
        self._conv_meta = {}       # conv weight name -> (feature channels, K, Fout), recorded while tracing
        self._conv_fpairs = {}     # graph_linear_2 <-> graph_linear_input of a GraphCMR block (they share a forward accumulator)
        self._conv_pairs = {}      # graph_conv weight <-> affine weight of a res_block_affine (they share a data-gradient accumulator)
        self._piece_plan = None    # ops.PiecePlan over every conv weight that qualifies (fp16 two-piece contractions)
        self._pieces_dirty = True  # the planes do not reflect the current weights
        self._cond_plan = None     # consumers of the decoder's condition vector, recorded on the first pass
        self._cond_rec = None      # ... while recording
        self._cond_bank = None     # iterator over the precomputed coefficient tensors of the current pass
        self._cond_vec = None      # the condition tensor those consumers share

    # ---- data assets ---------------------------------------------------------------------------
    def _load_template(self):
        obj = os.path.join(self.project_dir, 'data', 'template_mesh.obj')
        edg = os.path.join(self.project_dir, 'data', 'edges_smpl.npy')
        if os.path.exists(obj) and os.path.exists(edg):
            verts = []
            with open(obj) as fh:
                for line in fh:
                    if line.startswith('v '):
                        verts.append([float(t) for t in line.split()[1:4]])
            return np.asarray(verts, dtype=np.float64), np.load(edg)
        pack = load_pack()
        return pack['template_verts'], pack['edges_smpl']

    def _resolve_loss_mask(self, loss_mask):
        """[V, 3] float32 weights of the reconstruction loss, or None.  'binary': <project_dir>/data/loss_mask_binary.npy (where
        the reference ships it), else <project_dir>/lib/data/loss_mask_binary.npy (the path its code names, quirk C5).  An
        array of shape (V,), (V, 1) or (V, 3): custom weights, non-negative and finite, not all zero."""
        if loss_mask is None or isinstance(loss_mask, str):
            if loss_mask != 'binary':
                return None
            paths = [os.path.join(self.project_dir, 'data', 'loss_mask_binary.npy'),
                     os.path.join(self.project_dir, 'lib', 'data', 'loss_mask_binary.npy')]
            found = [q for q in paths if os.path.exists(q)]
            if not found:
                raise FileNotFoundError("loss_mask='binary': neither %s nor %s exists" % tuple(paths))
            loss_mask = np.load(found[0])
        V = self.input_num_verts
        w = np.asarray(loss_mask, dtype=np.float64)
        if w.shape == (V,):
            w = w[:, np.newaxis]
        if w.shape not in ((V, 1), (V, 3)):
            raise ValueError("loss_mask: shape %s, expected (%d,), (%d, 1) or (%d, 3)" % (w.shape, V, V, V))
        if not np.isfinite(w).all():
            raise ValueError("loss_mask: non-finite weights")
        if (w < 0).any():
            raise ValueError("loss_mask: negative weights")
        if not (w > 0).any():
            raise ValueError("loss_mask: all weights are zero")
        return np.ascontiguousarray(np.broadcast_to(w, (V, 3)), dtype=np.float32)

    def _resolve_normal(self, lambda_normal, faces):
        """(lambda_normal, faces [F, 3] int32 or None).  Faces are resolved only for lambda_normal > 0: an explicit array wins,
        else the 'f' lines of <project_dir>/data/template_mesh.obj."""
        try:
            lam = float(lambda_normal)
        except (TypeError, ValueError):
            raise ValueError("lambda_normal: %r is not a number" % (lambda_normal,))
        if not np.isfinite(lam) or lam < 0:
            raise ValueError("lambda_normal must be finite and >= 0, got %r" % (lambda_normal,))
        if lam == 0.0:
            return 0.0, None
        if self.nn_input_channel != 3:
            raise ValueError("lambda_normal > 0 needs 3 input channels (vertex coordinates), got %d" % self.nn_input_channel)
        if faces is None:
            obj = os.path.join(self.project_dir, 'data', 'template_mesh.obj')
            if not os.path.exists(obj):
                raise FileNotFoundError("lambda_normal > 0 needs the template's triangles: pass faces=<(F, 3) integer array> "
                                        "or provide %s with its 'f' lines" % obj)
            faces = self._obj_faces(obj)
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError("faces: shape %s, expected (F, 3)" % (f.shape,))
        if not np.issubdtype(f.dtype, np.integer):
            raise ValueError("faces: dtype %s, expected integers" % f.dtype)
        V = self.input_num_verts
        if f.min() < 0 or f.max() >= V:
            raise ValueError("faces: vertex indices outside [0, %d)" % V)
        if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any():
            raise ValueError("faces: a face names the same vertex twice")
        return lam, np.ascontiguousarray(f, dtype=np.int32)

    @staticmethod
    def _obj_faces(path):
        """Triangles of a Wavefront .obj: 'f a b c' lines, 1-based, 'a/b/c' tokens tolerated (the vertex index comes first)."""
        faces = []
        with open(path) as fh:
            for line in fh:
                if line.startswith('f '):
                    tok = line.split()[1:]
                    if len(tok) != 3:
                        raise ValueError("%s: face line with %d vertices, triangles expected: %r" % (path, len(tok), line.strip()))
                    faces.append([int(t.split('/')[0]) - 1 for t in tok])
        if not faces:
            raise ValueError("%s has no 'f' lines" % path)
        return np.asarray(faces, dtype=np.int64)

    # ---- variable store (TF-style scoped names) ------------------------------------------------
    class _ScopeCtx(object):
        def __init__(self, model, name):
            self.model, self.name = model, name

        def __enter__(self):
            self.model._scope.append(self.name)

        def __exit__(self, *a):
            self.model._scope.pop()

    def variable_scope(self, name):
        return base_model._ScopeCtx(self, name)

    def _get_variable(self, name, shape, kind):
        full = '/'.join(self._scope + [name])
        if full in self._vars:
            v = self._vars[full]
            assert tuple(v.shape) == tuple(int(s) for s in shape), (full, tuple(v.shape), shape)
            return v
        shape = tuple(int(s) for s in shape)
        if kind == 'conv':            # tf.truncated_normal_initializer(0, 0.1), reference :217-221
            arr = _trunc_normal(self._init_rng, shape, 0.1)
        elif kind == 'bias':          # tf.constant_initializer(0.1), :223-227
            arr = np.full(shape, 0.1, dtype=np.float32)
        elif kind == 'fc_kernel':     # tf.layers.dense default: glorot uniform
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            arr = self._init_rng.uniform(-lim, lim, size=shape).astype(np.float32)
        elif kind in ('fc_bias', 'gn_beta'):
            arr = np.zeros(shape, dtype=np.float32)
        elif kind == 'gn_gamma':
            arr = np.ones(shape, dtype=np.float32)
        else:
            raise ValueError(kind)
        v = torch.nn.Parameter(torch.from_numpy(arr).to(self.device))
        self._vars[full] = v
        self._kinds[full] = kind
        return v

    def _weight_variable(self, shape):
        return self._get_variable('weights', shape, 'conv')

    def _bias_variable(self, shape):
        return self._get_variable('bias', shape, 'bias')

    def _dense_vars(self, in_dim, units):
        """kernel, bias of a tf.layers.dense in the current scope and the gradient-bucket views of both."""
        with self.variable_scope('dense'):
            k = self._get_variable('kernel', (in_dim, units), 'fc_kernel')
            b = self._get_variable('bias', (units,), 'fc_bias')
            base = '/'.join(self._scope)
        return k, b, (self._grad_views.get(base + '/kernel'), self._grad_views.get(base + '/bias'))

    def _dense(self, x, units, activation=None):
        """tf.layers.dense (act(x @ kernel + bias)): the two 7M-parameter layers run on the weight-streaming
        kernels of csrc/fc.hip, the small condition-MLP layers on rocBLAS via torch."""
        k, b, gv = self._dense_vars(int(x.shape[-1]), units)
        return ops.dense(x, k, b, activation=activation, grad_bufs=gv)

    # ---- operator caches -----------------------------------------------------------------------
    def _conv_ops(self, L, K, unpool=None, pool=None):
        key = (id(L), int(K), id(unpool) if unpool is not None else None, id(pool) if pool is not None else None)
        if key not in self._ops_cache:
            host = ConvOperators(L, K, unpool=unpool, pool=pool)
            self._ops_cache[key] = (ops.DeviceConvOps(host, self.device), L, unpool, pool)
        return self._ops_cache[key][0]

    def _csr_pair(self, P):
        key = id(P)
        if key not in self._csr_cache:
            P64 = sp.csr_matrix(P, dtype=np.float64)
            self._csr_cache[key] = (ops.DeviceCSR(HostCSR(P64), self.device),
                                    ops.DeviceCSR(HostCSR(P64.T), self.device), P)
        return self._csr_cache[key][:2]

    # ---- fp16 two-piece contractions: piece planes of the conv weights ----------------------------------
    def _build_piece_plan(self):
        specs = []
        for name, (Ch, K, Fout) in sorted(self._conv_meta.items()):
            W = self._vars.get(name)
            if W is None or W.dtype != torch.float32 or not W.is_cuda or Ch % 8 or Fout % 8 or W.shape[0] < Ch * K:
                continue
            if not ((Ch % 32 == 0 and Fout >= 64) or (Fout % 32 == 0 and Ch >= 64)):
                continue
            pair = None
            pn = self._conv_pairs.get(name)
            if pn is not None and pn in self._conv_meta and pn in self._vars:
                pair = (self._vars[pn].detach(), self._conv_meta[pn][1])
            fpair = None
            fn = self._conv_fpairs.get(name)
            if fn is not None and fn in self._conv_meta and fn in self._vars:
                fpair = (self._vars[fn].detach(), self._conv_meta[fn][0] * self._conv_meta[fn][1])
            specs.append(dict(W=W.detach(), Ch=Ch, K=K, pair=pair, fpair=fpair))
        self._piece_plan_key = tuple(sorted(self._conv_meta.items()))
        old = getattr(self, '_piece_finalizer', None)
        if old is not None:
            old()                                       # the registry entries of the plan this one replaces
        self._piece_plan = ops.PiecePlan(specs, self.device) if specs else None
        # the registry (ops.PIECES, keyed by the weights' addresses) keeps weights and planes alive: drop this model's entries
        # when the model goes (a process that builds many models -- the test suite -- would otherwise accumulate them)
        self._piece_finalizer = weakref.finalize(self, ops.drop_pieces, [sp_["W"].data_ptr() for sp_ in specs]) if specs else None

    def _weights_version(self):
        """Version counters of everything the piece planes are computed from: the flat buckets (training: the variables are
        views of them) and the conv weights themselves (a model without optimiser state holds them as separate tensors).
        In-place edits through torch bump them; kernels that write through raw pointers and graph replays do not -- those
        paths set ``_pieces_dirty``."""
        v = tuple(int(st['flat']._version) for st in self._opt_state.values()) if getattr(self, '_opt_state', None) else ()
        names = getattr(self, '_conv_names_sorted', None)
        if names is None or len(names) != len(self._conv_meta):             # (the layer list only grows, during the first trace)
            names = self._conv_names_sorted = [n for n in sorted(self._conv_meta) if n in self._vars]
        return v + tuple(int(self._vars[n]._version) for n in names)

    def prepare_pieces(self):
        """(Re)write the piece planes of all conv weights from their CURRENT values: two launches.  Runs at the start of
        every forward_losses (so a captured training step always contains it) and lazily before the first contraction of
        any other pass once the weights may have changed (``_pieces_dirty``: optimiser step, restore, in-place edits)."""
        if not ops.H2 or self.act_dtype != torch.float32 or not self._conv_meta:
            return
        if getattr(self, '_piece_plan_key', None) != tuple(sorted(self._conv_meta.items())):
            self._build_piece_plan()                    # (also when no layer qualified last time: the key says so)
        if self._piece_plan is None:
            return
        for wp in self._piece_plan.run():
            ops.PIECES[wp.W.data_ptr()] = wp
        self._pieces_dirty = False
        self._pieces_versions = self._weights_version()

    def _begin_pass(self):
        """Entry of every top-level pass (forward_losses, encode, encode_only_condition, predict / evaluate, decode): the piece
        planes are rewritten from the current weights UNCONDITIONALLY -- two small launches -- instead of trusting that every
        writer of the variables (optimiser kernels, graph replays, collectives, raw-pointer writers) was seen."""
        self.prepare_pieces()

    def sync_variables(self, src=0):
        """Data parallel: every rank starts from rank ``src``'s variables (cape_amd.dist.broadcast_flat on the flat buckets)."""
        from . import dist as cdist
        for st in self._opt_state.values():
            cdist.broadcast_flat(st['flat'], src=src)
        self._pieces_dirty = True               # (a collective writes the bucket without a version bump)

    def _ensure_pieces(self):
        if self._piece_plan is None and not getattr(self, '_traced', False):
            return                      # first trace (build_graph): the layers prepare their planes on demand
        if self._piece_plan is None or self._pieces_dirty or self._weights_version() != getattr(self, '_pieces_versions', None):
            self.prepare_pieces()       # (a traced model without a plan yet -- inference only -- gets one here: two launches per
                                        # pass instead of two per layer)

    # ---- the reference's named operators (plug-points) --------------------------------------------
    def chebyshev5(self, x, L, Fout, K, activation=None, bias=None, pool=None, unpool=None, cond=None,
                   W_affine=None, cond_in=None):
        """Graph conv (reference :69-103); optional fusions are keyword-only extensions.  ``cond_in``
        = vertex-constant input channels appended after x's channels (never materialised)."""
        Cin = x.shape[-1] + (0 if cond_in is None else cond_in.shape[1])
        W = self._weight_variable([Cin * K, Fout])
        dops = self._conv_ops(L, K, unpool=unpool, pool=pool)
        if cond_in is not None and not dops.fused:
            # polynomial orders above 3 take the explicit recurrence (no precomposed operators): the condition channels
            # are materialised for it, as the reference does (tf.concat before the filter, lib/models.py:586-613)
            x, cond_in = ops.ConcatCondFn.apply(x, cond_in), None
        wname = '/'.join(self._scope + ['weights'])
        waname = '/'.join(self._scope[:-1] + ['affine', 'weights'])
        bname = '/'.join(self._scope + ['bias'])
        Ch = int(x.shape[-1])
        self._conv_meta[wname] = (Ch, int(K), int(Fout))
        if W_affine is not None:
            self._conv_pairs[wname], self._conv_pairs[waname] = waname, wname
        self._ensure_pieces()
        gW = self._grad_views.get(wname)
        gB = self._grad_views.get(bname) if bias is not None else None      # channel bias [1,1,F] or vertex bias [1,M,F]
        gWa = None
        if W_affine is not None:
            self._conv_meta[waname] = (Ch, 1, int(Fout))
            gWa = self._grad_views.get(waname)
        coef = None
        if cond_in is not None and cond_in is self._cond_vec:
            # one of the consumers of the decoder's condition vector: its rank-1 coefficients come from the
            # all-layers launch (CondCoefFn) once the list of consumers is known, i.e. from the second pass on
            if self._cond_bank is not None:
                coef, cond_in = next(self._cond_bank), None
            elif self._cond_rec is not None:
                self._cond_rec.append(dict(wname=wname, waname=waname if W_affine is not None else None, Ch=Ch, K=int(K)))
        return ops.chebyshev5(x, W, dops, bias=bias,
                              activation=activation, cond=cond, W_affine=W_affine, cond_in=cond_in,
                              grad_bufs=(gW, gWa), bias_grad_buf=gB, coef=coef)

    # ---- condition-coefficient bank (decoder) -------------------------------------------------------
    def _cond_bank_begin(self, cond):
        """Called with the decoder's condition vector before its first consumer runs."""
        self._cond_vec, self._cond_bank, self._cond_rec = cond, None, None
        plan = self._cond_plan
        if plan is None:
            self._cond_rec = []
            return
        need_grad = torch.is_grad_enabled()
        layers = []
        for e in plan:
            gW = self._grad_views.get(e['wname'])
            gWa = self._grad_views.get(e['waname']) if e['waname'] else None
            if need_grad and (gW is None or (e['waname'] and gWa is None)):
                return            # no gradient bucket to write into (e.g. a bare autograd.grad call): per-layer path
            layers.append(dict(W=self._vars[e['wname']], Wa=self._vars[e['waname']] if e['waname'] else None,
                               Ch=e['Ch'], K=e['K'], gW=gW, gWa=gWa))
        if layers:
            self._cond_bank = iter(ops.CondCoefFn.apply(cond, layers))

    def _cond_bank_end(self):
        if self._cond_rec is not None:
            self._cond_plan, self._cond_rec = self._cond_rec, None
        elif self._cond_bank is not None:
            assert next(self._cond_bank, None) is None, "condition-consumer list changed between passes"
        self._cond_vec = self._cond_bank = None

    def _brelu_named(self, x, kind):
        shape = [1, x.shape[1], x.shape[2]] if kind == 'b2relu' else [1, 1, x.shape[2]]
        return ops.brelu(x, self._bias_variable(shape), kind)

    def b1leakyrelu(self, x):
        return self._brelu_named(x, 'b1leakyrelu')

    def b1relu(self, x):
        return self._brelu_named(x, 'b1relu')

    def b1tanh(self, x):
        return self._brelu_named(x, 'b1tanh')

    def b2relu(self, x):
        return self._brelu_named(x, 'b2relu')

    def poolwT(self, x, P):
        """Pool / unpool with a precomputed sparse matrix (reference :129-152)."""
        if is_identity(P):
            return x
        fwd, bwd = self._csr_pair(P)
        return ops.poolwT(x, fwd, bwd)

    def _fusable(self):
        return (self.filter.__func__ is base_model.chebyshev5 and self.pool.__func__ is base_model.poolwT
                and self.unpool.__func__ is base_model.poolwT and self._activation_name in _ACTIVATIONS)

    def _conv_act_pool(self, x, L, Fout, K, D, cond_in=None):
        """conv -> bias+act -> pool (cnp / cnp_d bodies, reference :154-171, :796-810)."""
        kind = self._activation_name
        if self._fusable():
            host = self._conv_ops(L, K, pool=D).host
            if host.pool_fused and host.fused and kind != 'b2relu':
                b = self._bias_variable([1, 1, Fout])
                return self.chebyshev5(x, L, Fout, K, activation=kind, bias=b, pool=D, cond_in=cond_in)
        if cond_in is not None:
            x = ops.ConcatCondFn.apply(x, cond_in)
        x = self.filter(x, L, Fout, K)
        x = self.brelu(x)
        return self.pool(x, D)

    def cnp(self, x, i, name, cond_in=None):
        with self.variable_scope(name):
            return self._conv_act_pool(x, self.Laplacian[i], self.out_channels[i], self.poly_order[i],
                                       self.Downsample_mtx[i], cond_in=cond_in)

    def udn(self, x, out_channels, i, name, cond_in=None):
        """unpool -> conv -> bias+act (reference :173-191), unpool folded into the conv operators."""
        with self.variable_scope(name):
            L, Fout, K = self.Laplacian[-i - 2], out_channels[-i - 1], self.poly_order[-i - 1]
            U = self.Upsample_mtx[-i - 1]
            kind = self._activation_name
            if self._fusable() and K <= 3 and kind != 'b2relu':
                b = self._bias_variable([1, 1, Fout])
                return self.chebyshev5(x, L, Fout, K, activation=kind, bias=b, unpool=U, cond_in=cond_in)
            if cond_in is not None:
                x = ops.ConcatCondFn.apply(x, cond_in)
            x = self.unpool(x, U)
            return self.brelu(self.filter(x, L, Fout, K))

    def vae_sampling(self, z_mean, z_logvar, eps=None):
        if eps is None:
            eps = torch.randn((z_mean.shape[0], int(self.nz)), device=z_mean.device, dtype=torch.float32)
        # reference :195 writes sqrt(exp(logvar)); exp(0.5*logvar) is the same number (to rounding) but
        # its gradient stays finite when exp(logvar) under/overflows in fp32 (|logvar| > ~88..103), where
        # the sqrt/exp chain yields inf*0 = NaN -- reached within 10 steps from the reference initialisers
        # on N(0,1) data.
        return z_mean + torch.exp(0.5 * z_logvar) * eps

    def _get_path(self, folder):
        return os.path.join(self.project_dir, folder, self.name)

    # ---- variables in / out -----------------------------------------------------------------------
    def get_var(self, name):
        self._get_session()
        return self._vars[name].detach().cpu().numpy()

    def variables(self):
        return collections.OrderedDict((k, v.detach().cpu().numpy()) for k, v in self._vars.items())

    def load_variables(self, arrays, strict=True):
        """Assign variables by TF name (conv ``[Fin*K,Fout]``, dense ``[in,out]`` layouts)."""
        missing = [k for k in self._vars if k not in arrays]
        if strict and missing:
            raise KeyError("missing variables: %s" % missing[:5])
        with torch.no_grad():
            for k, v in self._vars.items():
                if k in arrays:
                    a = np.asarray(arrays[k], dtype=np.float32)
                    if tuple(a.shape) != tuple(v.shape):
                        raise ValueError("shape mismatch for %s: %s vs %s" % (k, a.shape, tuple(v.shape)))
                    v.copy_(torch.from_numpy(a).to(v.device))
        self._weights_loaded = True
        self._pieces_dirty = True


class CAPE(base_model):
    """Mesh CVAE + discriminator with two conditions (pose, clothing type) -- reference :230-832."""

    def __init__(self, L, D, U, L_d, D_d, lr_scaler, lambda_gan, use_res_block, use_res_block_dec, nz_cond2,
                 cond2_dim, Kd, n_layer_cond=1, cond_encoder=True, reduce_dim=True, affine=False,
                 lr_warmup=False, optim_condnet=True, bug_compat=False, act_dtype='fp32', **kwargs):
        super(CAPE, self).__init__(L, D, U, **kwargs)
        # Storage type of the mesh activations [N, M, C] (an extension over the reference, whose placeholders are fp32,
        # :272-282): 'fp32' = the parity path; 'bf16' = BASELINE configs[4] -- activations and their gradients live in HBM
        # as bf16, the contractions compute with bf16 operands and fp32 accumulation, variables / optimiser state / the
        # dense layers / losses stay fp32 (master weights).
        if act_dtype not in ('fp32', 'bf16', torch.float32, torch.bfloat16):
            raise ValueError("act_dtype must be 'fp32' or 'bf16'")
        self.act_dtype = torch.bfloat16 if act_dtype in ('bf16', torch.bfloat16) else torch.float32
        if self.act_dtype == torch.bfloat16 and (use_res_block or (use_res_block_dec and not affine)):
            raise NotImplementedError("bf16 activation storage covers the cnp encoder with the affine / udn decoders "
                                      "(the res_block and group-norm kernels read fp32)")
        self.Laplacian_d, self.Downsample_mtx_d = L_d, D_d
        self.Laplacian, self.Downsample_mtx, self.Upsample_mtx = L, D, U
        self.poly_order_d = [Kd] * len(self.out_channels)
        self.use_res_block = use_res_block
        self.use_res_block_dec = use_res_block_dec
        self.nz_cond2 = nz_cond2
        self.cond2_dim = cond2_dim
        self.n_layer_cond = n_layer_cond
        self.cond_encoder = cond_encoder
        self.optim_condnet = optim_condnet
        self.reduce_dim = reduce_dim
        self.affine = affine
        if self.reduce_dim > 0:
            self.reduce_rate = self.out_channels[-1] // self.reduce_dim
        elif self.reduce_dim == 0:
            self.reduce_rate = 1
        else:
            raise ValueError('reduce dim must be greater than 0!')
        self.lr_g = self.learning_rate
        self.lr_d = self.learning_rate * lr_scaler
        self.lambda_gan = lambda_gan
        self.lr_warmup = lr_warmup
        # Reference quirks C1/C2: with bug_compat the discriminator "gradient" is
        # its clipped weights and every fit iteration applies both optimizers twice.
        self.bug_compat = bug_compat
        self.phase = None
        self.global_step = 0
        self._weights_loaded = False
        self._opt_state = None
        self._ema = {'g': 0.0, 'd': 0.0}

    # ======================= network components (reference :479-832) ==============================
    def condition(self, y, name, nz_cond, nlayers=1):
        y_dim = int(y.shape[-1])
        with self.variable_scope('condition_{}'.format(name)):
            if nlayers == 1:
                with self.variable_scope('fc1'):
                    y = self._dense(y, nz_cond)
            else:
                if nz_cond < y_dim // 2:
                    n_out_fc1 = y_dim // 2
                elif nz_cond < y_dim * 2:
                    n_out_fc1 = y_dim
                else:
                    n_out_fc1 = nz_cond // 2
                with self.variable_scope('fc1'):
                    y = self._dense(y, n_out_fc1, activation='leaky_relu')
                with self.variable_scope('fc2'):
                    y = self._dense(y, nz_cond)
        return y

    def _conditions(self, cond, cond2):
        """Pose and clothing-type embeddings (:284-290).  With the default layer counts (pose MLP 2 layers, clothing type 1)
        both networks run as ONE launch per direction (ops.CondNetsFn) and the embeddings are the two halves of the
        concatenated condition every consumer needs (``_cat_cond``); variables are created under the reference's names."""
        self._ycat = None
        y_dim = int(cond.shape[-1])
        nzc = int(self.nz_cond)
        hid = y_dim // 2 if nzc < y_dim // 2 else (y_dim if nzc < y_dim * 2 else nzc // 2)       # rule of :498-503
        # shape limits of the fused kernels (csrc/condnet.hip condnet_check); anything else takes the per-layer path below
        fits = (y_dim <= 512 and hid <= 256 and
                4 * int(cond.shape[0]) * (hid + nzc + int(self.nz_cond2)) <= 60 * 1024)
        if (self.n_layer_cond == 1 and cond.is_cuda and cond.dim() == 2 and cond.shape[0] <= 64 and fits
                and cond.dtype == torch.float32 and cond2.dtype == torch.float32):
            with self.variable_scope('condition_pose'):
                with self.variable_scope('fc1'):
                    W1, b1, g1 = self._dense_vars(y_dim, hid)
                with self.variable_scope('fc2'):
                    W2, b2, g2 = self._dense_vars(hid, nzc)
            with self.variable_scope('condition_clo_label'):
                with self.variable_scope('fc1'):
                    Wc, bc, gc = self._dense_vars(int(cond2.shape[-1]), int(self.nz_cond2))
            gb = g1 + g2 + gc
            # under differentiation the kernel writes the embedding twice: the second buffer belongs to the decoder input
            # [z | y | y2] alone, so that its gradient reaches the backward kernel by itself (no element-wise sum of the two)
            two = torch.is_grad_enabled() and any(v.requires_grad for v in (W1, W2, Wc))
            res = ops.CondNetsFn.apply(cond, cond2, W1, b1, W2, b2, Wc, bc, gb if all(v is not None for v in gb) else None,
                                       2 if two else 1)
            ycat, ycat_b = res if two else (res, None)
            y, y2 = ycat[:, :nzc], ycat[:, nzc:]
            self._ycat = (y, y2, ycat, ycat_b)
            return y, y2
        y = self.condition(cond, 'pose', self.nz_cond, nlayers=2)
        y2 = self.condition(cond2, 'clo_label', self.nz_cond2, nlayers=self.n_layer_cond)
        return y, y2

    def _cat_cond(self, y, y2, own=False):
        """tf.concat([y, y2], 1): the tensor the fused condition kernel already produced when y / y2 are its halves
        (``own``: the second copy, reserved for ONE consumer -- see _conditions)."""
        t = getattr(self, '_ycat', None)
        if t is not None and y is t[0] and y2 is t[1]:
            return t[3] if own and t[3] is not None else t[2]
        return torch.cat([y, y2], 1)

    def res_block(self, x_in, i, name):
        with self.variable_scope(name):
            L, F_, K = self.Laplacian[i], self.out_channels[i], self.poly_order[i]
            with self.variable_scope('filter_1'):
                x1 = self.filter(x_in, L, F_, K)
            with self.variable_scope('bias_relu_1'):
                x1 = self.brelu(x1)
            with self.variable_scope('filter_2'):
                x2 = self.filter(x1, L, F_, K)
            if x_in.shape[-1] != x2.shape[-1]:
                with self.variable_scope('1x1-conv'):
                    x_in = self.filter(x_in, L, x2.shape[-1], 1)
            with self.variable_scope('addition'):
                x2 = x2 + x_in
            with self.variable_scope('bias_relu_2'):
                x2 = self.brelu(x2)
            return self.pool(x2, self.Downsample_mtx[i])

    def gn(self, x, name, relu=False, G=32, eps=1e-5, passthrough=False):
        with self.variable_scope(name):
            Cn = int(x.shape[-1])
            gamma = self._get_variable('gamma', (Cn,), 'gn_gamma')
            beta = self._get_variable('beta', (Cn,), 'gn_beta')
            base = '/'.join(self._scope)
        Ge = ops.group_count(x.shape[0], Cn, G)      # the reference's free-dimension reshape, lib/models.py:698
        return ops.GroupNormFn.apply(x, gamma, beta, Ge, eps, 1 if relu else 0, passthrough,
                                     self._grad_views.get(base + '/gamma'), self._grad_views.get(base + '/beta'))

    def _plain_weight(self, scope, shape):
        """A 1x1 filter's weight in ``scope`` with its gradient-bucket view (what chebyshev5 does for K = 1)."""
        with self.variable_scope(scope):
            W = self._weight_variable(shape)
            wname = '/'.join(self._scope + ['weights'])
        self._conv_meta[wname] = (int(shape[0]), 1, int(shape[1]))
        return W, self._grad_views.get(wname)

    def res_block_decoder(self, x_in, i, name, cond=None):
        Fi, Lm = self.out_channels[-i - 1], self.Laplacian[-i - 2]
        with self.variable_scope(name):
            xu = self.unpool(x_in, self.Upsample_mtx[-i - 1])
            # the fused tail: graph_linear_2 + graph_linear_input + addition + concat as one contraction (same variables,
            # same creation order as the reference's :763-774); needs the 1x1 input filter, i.e. differing channel counts
            fuse_tail = bool(ops.CMR_FUSED_TAIL and self._fusable() and xu.shape[-1] != Fi and xu.is_cuda
                             and xu.dtype == torch.float32)
            if fuse_tail:
                x, xu = self.gn(xu, 'group_norm', relu=True, passthrough=True)
            else:
                x = self.gn(xu, 'group_norm', relu=True)
            with self.variable_scope('graph_linear_1'):
                x = self.filter(x, Lm, Fi // 2, 1)
            x = self.gn(x, 'group_norm_1', relu=True)
            with self.variable_scope('graph_conv'):
                x = self.filter(x, Lm, Fi // 2, self.poly_order[-i - 1])
            x = self.gn(x, 'group_norm_2', relu=True)
            if fuse_tail:
                W2, gW2 = self._plain_weight('graph_linear_2', [int(x.shape[-1]), Fi])
                Wi, gWi = self._plain_weight('graph_linear_input', [int(xu.shape[-1]), Fi])
                n2, ni = '/'.join(self._scope + ['graph_linear_2', 'weights']), '/'.join(self._scope + ['graph_linear_input', 'weights'])
                self._conv_fpairs[n2], self._conv_fpairs[ni] = ni, n2      # their products share one accumulator
                return ops.ResidualLinearFn.apply(x, xu, W2, Wi, cond, gW2, gWi)
            with self.variable_scope('graph_linear_2'):
                x = self.filter(x, Lm, Fi, 1)
            if xu.shape[-1] != x.shape[-1]:
                with self.variable_scope('graph_linear_input'):
                    xu = self.filter(xu, Lm, x.shape[-1], 1)
            x = x + xu
            if cond is not None:
                x = ops.ConcatCondFn.apply(x, cond)
            return x

    def res_block_affine(self, x, i, name, cond_in=None):
        """unpool -> relu(K-conv) + 1x1 affine conv (reference :776-793): ONE fused launch; the
        condition channels of the input enter as rank-1 terms."""
        Lm, Fh, K = self.Laplacian[-i - 2], self.out_channels[-i - 1] // 2, self.poly_order[-i - 1]
        U = self.Upsample_mtx[-i - 1]
        with self.variable_scope(name):
            if self._fusable() and K <= 3:
                Cin = x.shape[-1] + (0 if cond_in is None else cond_in.shape[1])
                with self.variable_scope('affine'):
                    Wa = self._weight_variable([Cin, Fh])
                with self.variable_scope('graph_conv'):
                    return self.chebyshev5(x, Lm, Fh, K, unpool=U, W_affine=Wa, cond_in=cond_in)
            if cond_in is not None:
                x = ops.ConcatCondFn.apply(x, cond_in)
            x = self.unpool(x, U)
            with self.variable_scope('graph_conv'):
                x_gc = torch.relu(self.filter(x, Lm, Fh, K))
                ops._trace_sign(x_gc, "relu")
            with self.variable_scope('affine'):
                x_aff = self.filter(x, Lm, Fh, 1)
            return x_aff + x_gc

    def cnp_d(self, x, i, name, cond_in=None):
        with self.variable_scope(name):
            return self._conv_act_pool(x, self.Laplacian_d[i], self.out_channels[i], self.poly_order_d[i],
                                       self.Downsample_mtx_d[i], cond_in=cond_in)

    def fit_cond_dim(self, x, y):
        return y.reshape(x.shape[0], 1, y.shape[-1]).expand(x.shape[0], x.shape[1], y.shape[-1])

    def encoder(self, x, y, y2, use_res_block=False, use_cond=True):
        cond_in = self._cat_cond(y, y2) if use_cond else None
        if cond_in is not None and use_res_block:
            x, cond_in = ops.ConcatCondFn.apply(x, cond_in), None      # res_block reads its input twice
        if x.dtype != self.act_dtype:
            x = x.to(self.act_dtype)                                   # bf16 storage: the mesh tensors from here on
        with self.variable_scope('encoder'):
            # the plain stack hands each layer's output to exactly one consumer (the next layer): its backward pass may fuse
            # the activation gradient of the layer below into the kernel that produces that layer's incoming gradient
            with ops.sole_consumer_chain(not use_res_block):
                for i in range(len(self.out_channels)):
                    if use_res_block:
                        x = self.res_block(x, i, 'encoder_resblock{}'.format(i + 1))
                    else:
                        x = self.cnp(x, i, 'encoder_conv{}'.format(i + 1), cond_in=cond_in if i == 0 else None)
                if self.reduce_dim > 0:
                    with self.variable_scope('1x1-conv'):
                        x = self.filter(x, self.Laplacian[-1], self.out_channels[-1] // self.reduce_rate, K=1)
            if getattr(self, 'split_backward', False) and torch.is_grad_enabled() and x.requires_grad:
                # two-phase backward (data-parallel overlap, see backward_phase1/2): the graph is cut here, below the
                # dense layers -- everything downstream of the cut is differentiated first
                self._enc_feat = x
                x = x.detach().requires_grad_(True)
                self._enc_feat_cut = x
            x = x.reshape(x.shape[0], -1)
            if x.dtype != torch.float32:
                x = x.float()                                          # the dense layers (fp32 master weights) read fp32
            with self.variable_scope('fc_mean'):
                km, bm, gm = self._dense_vars(int(x.shape[-1]), int(self.nz))
            with self.variable_scope('fc_var'):
                kv, bv, gv = self._dense_vars(int(x.shape[-1]), int(self.nz))
            z_mean, z_var = ops.dense_pair(x, km, bm, kv, bv, (gm, gv))      # both layers in one pass over x
        return z_mean, z_var

    def decoder_cond_vert(self, x, y, y2, use_res_block=False):
        N = x.shape[0]
        cond = self._cat_cond(y, y2)
        # the GraphCMR block group-normalises over the concatenated [features | condition] channels, so it
        # needs the condition materialised; every other consumer takes it as rank-1 ``cond_in`` terms.
        materialise = bool(use_res_block and not self.affine) or not self._fusable()
        if not materialise:
            self._cond_bank_begin(cond)
        with self.variable_scope('decoder'):
            with self.variable_scope('fc1'):
                out_nodes = int(self.p[-1] * self.out_channels[-1]) // self.reduce_rate
                x = self._dense(x, out_nodes, activation='leaky_relu')
            x = x.reshape(N, int(self.p[-1]), -1)
            if x.dtype != self.act_dtype:
                x = x.to(self.act_dtype)
            if self.reduce_dim > 0:
                with self.variable_scope('1x1-conv'):
                    if self._fusable():
                        x = self.chebyshev5(x, self.Laplacian[-1], self.out_channels[-1], 1,
                                            cond=cond if materialise else None)
                    else:
                        x = ops.ConcatCondFn.apply(self.filter(x, self.Laplacian[-1], self.out_channels[-1], K=1), cond)
            elif materialise:
                x = ops.ConcatCondFn.apply(x, cond)
            for i in range(len(self.out_channels)):
                if use_res_block:
                    if not self.affine:
                        x = self.res_block_decoder(x, i, 'decoder_resblock_cmr{}'.format(i + 1), cond=cond)
                    else:
                        x = self.res_block_affine(x, i, 'decoder_resblock_affine{}'.format(i + 1),
                                                  cond_in=None if materialise else cond)
                        if materialise:
                            x = ops.ConcatCondFn.apply(x, cond)
                else:
                    x = self.udn(x, self.out_channels, i, 'decoder_conv{}'.format(i + 1),
                                 cond_in=None if materialise else cond)
                    if materialise:
                        x = ops.ConcatCondFn.apply(x, cond)
            with self.variable_scope('outputs'):
                M = self.Laplacian[0].shape[0]
                Fo = int(self.nn_input_channel)
                b = self._bias_variable([1, M, Fo])      # one bias per vertex per channel (:615)
                if self._fusable():
                    x = self.chebyshev5(x, self.Laplacian[0], Fo, self.poly_order[0], bias=b,
                                        cond_in=None if materialise else cond)
                else:
                    x = self.filter(x, self.Laplacian[0], Fo, self.poly_order[0]) + b
        if not materialise:
            self._cond_bank_end()
        return x.float() if x.dtype != torch.float32 else x           # losses and callers see fp32

    def generator(self, x, y, y2, eps=None):
        with self.variable_scope('generator'):
            z_mean, z_logvar = self.encoder(x, y, y2, use_res_block=self.use_res_block, use_cond=self.cond_encoder)
            if eps is None:
                eps = torch.randn((z_mean.shape[0], int(self.nz)), device=z_mean.device, dtype=torch.float32)
            # sampling (:193-196) and the KL term (:371-372) share one hand-differentiated op
            # (the op also appends the condition: [z | y | y2], the decoder's input of :296, without a concat launch)
            z_total, self._kl_of_last_sample = ops.VaeSampleKLFn.apply(z_mean, z_logvar, eps, self._cat_cond(y, y2, own=True))
            self._kl_inputs = (z_mean, z_logvar)
            x_hat = self.decoder_cond_vert(z_total, y, y2, use_res_block=self.use_res_block_dec)
        return x_hat, z_mean, z_logvar

    def discriminator(self, x, y, y2, cond=None):
        """``cond``: the concatenated condition [y | y2] when the caller already holds it (then y / y2 are not read)."""
        if cond is None:
            cond = self._cat_cond(y, y2)
        if x.dtype != self.act_dtype:
            x = x.to(self.act_dtype)
        with self.variable_scope('discriminator'):
            with self.variable_scope('shared'):
                for i in range(len(self.Downsample_mtx_d)):
                    x = self.cnp_d(x, i, 'conv{}'.format(i + 1), cond_in=cond if i == 0 else None)
            with self.variable_scope('prediction_map'):
                # poly_order[-1] (=2), not poly_order_d: reference quirk C3 (:676), kept for
                # checkpoint-shape compatibility
                pred_map = self.filter(x, self.Laplacian_d[-1], 1, self.poly_order[-1])
        return pred_map.float() if pred_map.dtype != torch.float32 else pred_map

    # ======================= losses (reference :354-416) ==========================================
    def _edge_tables(self):
        if not hasattr(self, '_edge_dev'):
            vptr, vidx = vertex_edge_table(self.vpe, self.input_num_verts)
            d = self.device
            self._edge_dev = (torch.tensor(np.asarray(self.verts_ref), dtype=torch.float32, device=d),
                              torch.tensor(np.asarray(self.vpe), dtype=torch.int32, device=d),
                              torch.tensor(vptr, dtype=torch.int32, device=d),
                              torch.tensor(vidx, dtype=torch.int32, device=d))
        return self._edge_dev

    def _loss_mask_dev(self):
        """The mask's [V, 3] weights on the device, made once: a captured step keeps pointing at this tensor."""
        if not hasattr(self, '_loss_mask_t'):
            self._loss_mask_t = torch.tensor(self._loss_mask_w, dtype=torch.float32, device=self.device)
        return self._loss_mask_t

    def _face_tables(self):
        """Faces and the vertex -> incident-corner table on the device, made once: a captured step keeps pointing at them."""
        if not hasattr(self, '_face_dev'):
            fptr, fidx = vertex_face_table(self._faces, self.input_num_verts)
            d = self.device
            self._face_dev = (torch.tensor(self._faces, dtype=torch.int32, device=d),
                              torch.tensor(fptr, dtype=torch.int32, device=d),
                              torch.tensor(fidx, dtype=torch.int32, device=d))
        return self._face_dev

    def _add_normal(self, out, g_outputs, g_gt):
        """lambda_normal > 0: out['normal'], and lambda_normal * normal added to out['total_no_gan'] by the loss's own
        finishing kernel."""
        faces, fptr, fidx = self._face_tables()
        total, parts = ops.FaceNormalLossFn.apply(g_outputs, g_gt, self._edge_tables()[0], faces, fptr, fidx,
                                                  float(self.lambda_normal), out['total_no_gan'])
        out['normal'], out['total_no_gan'] = parts[0], total
        return out

    def loss_terms(self, g_outputs, g_gt, z_mean, z_logvar):
        """recon / latent / edge / fc-regularisation terms and their weighted sum (no GAN term)."""
        out = self._loss_terms(g_outputs, g_gt, z_mean, z_logvar)
        return self._add_normal(out, g_outputs, g_gt) if self.lambda_normal > 0 else out

    def _loss_terms(self, g_outputs, g_gt, z_mean, z_logvar):
        """loss_terms without the face-normal term: the reference's wired losses."""
        out = {}
        lat = self._latent_term(z_mean, z_logvar)
        reg = self._fc_regulariser()
        out['latent'], out['fc_reg_g'] = lat, reg
        masked = self._loss_mask_w is not None
        if (masked or self.which_loss == 'l1') and g_outputs.shape[-1] == 3:
            # one device kernel: l1, or with loss_mask (reference :357-369) every loss kind as sum w * l / sum w
            vr, ed, vptr, vidx = self._edge_tables()
            weighted = ()
            if masked:
                kind = self.which_loss if self.which_loss in ('l1', 'huber') else 'l2'   # :367 else: mean_squared_error
                weighted = (self._loss_mask_dev(), self._loss_mask_sum, kind)
            # the latent term and the regulariser value join the weighted sum INSIDE the loss kernel when they are device
            # scalars already (the fused sampling / KL op; the bucket path's detached regulariser): no element-wise launches
            # for  total_re + lambda_latent * latent + reg  and none for their gradients
            scalar = lambda t: torch.is_tensor(t) and t.dim() == 0 and t.is_cuda and t.dtype == torch.float32
            reg_ok = (scalar(reg) and not reg.requires_grad) if torch.is_tensor(reg) else float(reg) == 0.0
            fold = g_outputs.is_cuda and scalar(lat) and reg_ok
            terms = (lat, float(self.lambda_latent), reg if torch.is_tensor(reg) else None) if fold else (None, 0.0, None)
            total_re, parts = ops.ReconEdgeLossFn.apply(g_outputs, g_gt, vr, ed, vptr, vidx, float(self.lambda_l1),
                                                        float(self.lambda_edge), *terms, *weighted)
            out['recon'], out['edge'] = parts[0], parts[1]
            if fold:
                out['total_no_gan'] = total_re
                return out
        else:
            diff = g_outputs - g_gt
            if self.which_loss == 'l1':
                out['recon'] = diff.abs().mean()
                if ops.L1_SIGN_TRACE is not None:
                    ops.L1_SIGN_TRACE.append(torch.sign(diff.detach()).cpu())
            elif self.which_loss == 'huber':
                a = diff.abs()
                out['recon'] = torch.where(a <= 0.1, 0.5 * a * a, 0.1 * a - 0.005).mean()
            else:
                out['recon'] = (diff * diff).mean()
            vr, ed, vptr, vidx = self._edge_tables()
            e_total, parts = ops.ReconEdgeLossFn.apply(g_outputs, g_gt, vr, ed, vptr, vidx, 0.0,
                                                       float(self.lambda_edge))
            out['edge'] = parts[1]
            total_re = out['recon'] * self.lambda_l1 + e_total
        out['total_no_gan'] = torch.add(total_re, lat, alpha=float(self.lambda_latent)) + reg      # two launches, not three
        return out

    def _latent_term(self, z_mean, z_logvar):
        if getattr(self, '_kl_inputs', None) is not None and self._kl_inputs[0] is z_mean and self._kl_inputs[1] is z_logvar:
            return self._kl_of_last_sample            # computed together with the sampling
        lat = -0.5 * torch.sum(1 + z_logvar - z_mean * z_mean - torch.exp(z_logvar), dim=1)
        return lat.mean()

    def _fc_regulariser(self):
        """l2_regularizer(scale)(w) = scale*sum(w^2)/2 on dense kernels under 'generator', multiplied by
        `regularization` once more (reference :40, :378-379; quirk C6).  Its VALUE is reported here from
        detached kernels; its GRADIENT (regularization^2 * w) is folded into the optimiser's norm and update
        kernels on the flat bucket (apply_updates, Momentum and Adam alike) -- identical numbers, without recording 7M-element tape nodes for three kernels."""
        reg = 0.0
        self._reg_names = []
        if self.regularization:
            self._reg_names = [n for n in self._vars if self._kinds[n] == 'fc_kernel' and n.startswith('generator')]
            if self._reg_names:
                coef = self.regularization * self.regularization
                if self._opt_state is not None and torch.is_grad_enabled() and getattr(self, '_reg_via_bucket', False):
                    st = self._opt_state['g']
                    with torch.no_grad():
                        reg = ops.sumsq_ranges(st['flat'], self._reg_ranges(), 0.5 * coef, st['ws'])
                    self._reg_in_bucket = True
                else:
                    reg = sum(0.5 * (self._vars[n] * self._vars[n]).sum() for n in self._reg_names) * coef
                    self._reg_in_bucket = False
        return reg

    @staticmethod
    def _bce(logits, label):
        return torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.full_like(logits, label))

    # ======================= graph building =========================================================
    def build_graph(self, input_num_verts, nn_input_channel, phase='train'):
        """Materialise variables and per-layer operators (static shapes, like the reference's
        tf.Graph; :267-351) by tracing one zero batch through every network on the device."""
        _lib.require_gpu()
        assert phase in ('train', 'demo', 'test')
        self.phase = phase
        B, d = self.batch_size, self.device
        with torch.no_grad():
            x = torch.zeros((B, input_num_verts, nn_input_channel), device=d)
            c = torch.zeros((B, self.cond_dim), device=d)
            c2 = torch.zeros((B, self.cond2_dim), device=d)
            y, y2 = self._conditions(c, c2)
            x_hat, _, _ = self.generator(x, y, y2, eps=torch.zeros((B, int(self.nz)), device=d))
            self.discriminator(x_hat, y, y2)
        g_names = [n for n in self._vars if n.startswith('generator') or (self.optim_condnet and 'condition' in n)]
        # "late" variables: their gradient is only complete once the backward pass has run through the encoder
        # convolutions (the encoder conv stack and the condition nets, which also feed a conditioned encoder); all other
        # gradients (decoder, dense layers: 96 % of the bucket) are final earlier and can be exchanged while the
        # encoder backward still runs.  Late variables sit at the end of the flat bucket.
        is_late = lambda n: ('condition' in n) or (n.startswith('generator/encoder/') and '/fc_' not in n)
        self._g_names = [n for n in g_names if not is_late(n)] + [n for n in g_names if is_late(n)]
        self._g_early = sum(1 for n in g_names if not is_late(n))
        self._d_names = [n for n in self._vars if n.startswith('discriminator')]
        if phase == 'train':
            self._init_optimizer()
        self._traced = True
        return self

    # ======================= optimiser shell (reference :419-474) ===================================
    def _init_optimizer(self):
        """Flatten each variable group (G: generator + condition nets, D: discriminator) into ONE
        contiguous fp32 buffer (variables become views of it) with matching flat gradient and
        momentum buffers: the optimiser is a handful of launches over the flat buffers and the
        data-parallel exchange is a single all-reduce of ``flat_grad`` (cape_amd.dist)."""
        self._opt_state = {}
        for grp, names in (('g', self._g_names), ('d', self._d_names)):
            params = [self._vars[n] for n in names]
            # every variable starts on a 256-byte boundary of the bucket: the kernels' float4 weight
            # staging needs 16-byte aligned blocks (an unaligned base silently takes the scalar path, 2x
            # slower); the padding stays zero in parameters, gradients and momentum.
            al = lambda n: (n + 63) // 64 * 64
            total = sum(al(p.numel()) for p in params)
            flat = torch.zeros(total, device=self.device, dtype=torch.float32)
            flat_grad = torch.zeros(total, device=self.device, dtype=torch.float32)
            views, off, offsets = [], 0, {}
            with torch.no_grad():
                for nm_, p in zip(names, params):
                    n = p.numel()
                    offsets[nm_] = (off, al(n))
                    flat[off:off + n].copy_(p.detach().reshape(-1))
                    p.data = flat[off:off + n].view(p.shape)
                    views.append(flat_grad[off:off + n].view(p.shape))
                    off += al(n)
            if grp == 'g':
                # generator/condition variables are used exactly once per step, so their gradient kernels
                # may write the bucket directly; discriminator variables are shared by the real and the
                # fake pass (two contributions that autograd must add) and keep private gradient tensors.
                for nm, view in zip(names, views):
                    self._grad_views[nm] = view
            else:
                # ... unless the step evaluates D(generated) and D(real) as ONE pass (forward_losses, ops.merged_d_pass):
                # _grad_views hands these out only while that pass is traced (self._d_single_use)
                self._grad_views_d = dict(zip(names, views))
            n_early = self._g_early if grp == 'g' else len(names)
            split_off = offsets[names[n_early]][0] if n_early < len(names) else total
            st = {'params': params, 'flat': flat, 'flat_grad': flat_grad, 'grad_views': views, 'offsets': offsets,
                  'n_early': n_early, 'split_off': split_off,
                  'm': torch.zeros_like(flat), 'sumsq': torch.zeros((), device=self.device, dtype=torch.float32),
                  'ws': ops.flat_workspace(self.device),
                  'neg_lr': torch.zeros((), device=self.device, dtype=torch.float32)}
            if self.optimizer == 'adam':
                st['v'] = torch.zeros_like(flat)
                # device-resident step count of cape_flat_adam_update ([count, workgroup ticket]): graph replays advance it
                st['t'] = torch.zeros(2, device=self.device, dtype=torch.int32)
            self._opt_state[grp] = st
        self.global_step = 0

    def _lr_at(self, base_lr, step, warmup_duration=8):
        ds = int(self.decay_steps)
        if self.lr_warmup:
            warm = int(self.decay_steps * warmup_duration)
            if step < warm:
                return base_lr * float(step) / float(warm)
            return base_lr * self.decay_rate ** ((step - warm) // max(ds, 1))
        return base_lr * self.decay_rate ** (step // max(ds, 1))

    def set_learning_rates(self, groups=('g', 'd')):
        """Host side of the lr schedule (:426-442): write -lr into the device scalars read by
        ``apply_updates`` (kept outside any captured graph).  ``groups``: the variable groups the coming step updates
        (a CVAE-only step skips the discriminator's scalar: one tiny launch less per step)."""
        lr_g = self._lr_at(self.lr_g, self.global_step)
        lr_d = self._lr_at(self.lr_d, self.global_step)
        for grp, lr in (('g', lr_g), ('d', lr_d)):
            st = self._opt_state[grp]
            # the staircase schedule holds a value for decay_steps steps: the scalar is rewritten only when it changes
            # (a fill launch in front of every graph replay otherwise); checkpoint restores reset the cache
            if grp in groups and st.get('neg_lr_host') != -lr:
                st['neg_lr'].fill_(-lr)
                st['neg_lr_host'] = -lr
        return lr_g, lr_d

    def adam_steps(self, grp):
        """Number of Adam updates applied to a group so far (TF keeps it as beta1_power / beta2_power, :447-449)."""
        return int(self._opt_state[grp]['t'][0].item())

    def _set_adam_steps(self, grp, t):
        with torch.no_grad():
            self._opt_state[grp]['t'].copy_(torch.tensor([int(t), 0], dtype=torch.int32))

    def _reg_ranges(self):
        """Element ranges (padded to the 256-byte variable alignment; the padding holds zeros) of the generator's
        regularised dense kernels inside the G bucket."""
        off = self._opt_state['g']['offsets']
        return [(off[n][0], off[n][0] + off[n][1]) for n in getattr(self, '_reg_names', [])]

    def store_grads(self, grp, grads, lo=0, hi=None):
        """Put the gradients of variables [lo, hi) of a group into its flat gradient bucket."""
        st = self._opt_state[grp]
        with torch.no_grad():
            dst, src = [], []
            for view, g in zip(st['grad_views'][lo:hi], grads):
                if g is None:
                    view.zero_()
                elif g.data_ptr() != view.data_ptr():      # kernels may already have written the bucket
                    dst.append(view)
                    src.append(g.reshape(view.shape))
            if dst:
                torch._foreach_copy_(dst, src)             # one multi-tensor launch for the small variables

    def apply_updates(self, grp, clip=5.0, grad_scale=None):
        """clip_by_global_norm(5.0) (:461) + Momentum (non-Nesterov, TF semantics: accum = m*accum + g;
        var -= lr*accum) or Adam (:447-449), on the flat buffers.  Capturable: no host reads, no host-side counters."""
        st = self._opt_state[grp]
        g, flat, m = st['flat_grad'], st['flat'], st['m']
        with torch.no_grad():
            # 3 launches on the flat buckets (csrc/optim.hip), Momentum and Adam alike; the dense kernels' regulariser
            # gradient regularization^2 * w is part of the effective gradient (norm AND update) on its ranges
            ranges, coef = [], 0.0
            if grp == 'g' and getattr(self, '_reg_in_bucket', False):
                ranges, coef = self._reg_ranges(), self.regularization * self.regularization
            # data parallel: the bucket holds the SUM over the ranks (cape_amd.dist.GradAverager, defer_mean) and the kernels
            # apply 1 / world themselves; bug-compat D "gradients" are the (replicated) weights and are never exchanged
            # (``grad_scale`` is the CALLER's: the step runner that arranged the deferred mean passes its own value, so that a
            # second runner or a bare train_step on the same model cannot inherit it -- ADVICE r05)
            gs = 1.0 if (grp == 'd' and self.bug_compat) else float(1.0 if grad_scale is None else grad_scale)
            ops.flat_gradnorm(g, flat, ranges, coef, st['sumsq'], st['ws'], grad_scale=gs)
            if self.optimizer == 'adam':
                # tf.train.AdamOptimizer(learning_rate) with TensorFlow's defaults (:447-449); the step count is on the device
                ops.flat_adam_update(flat, g, m, st['v'], 0.9, 0.999, 1e-8, clip, st['sumsq'], st['neg_lr'], st['t'], ranges, coef,
                                     grad_scale=gs)
            else:
                ops.flat_momentum_update(flat, g, m, self.momentum, clip, st['sumsq'], st['neg_lr'], ranges, coef, grad_scale=gs)
            self._pieces_dirty = True           # (the kernel writes through raw pointers: no version bump to detect)
        return st['sumsq']

    # ======================= training step ========================================================
    def forward_losses(self, data_g, cond_g, cond2_g, gt, data_d=None, cond_d=None, cond2_d=None, eps=None,
                       with_gan=True, reg_via_bucket=False):
        """One evaluation of the training graph: returns dict with loss_g, loss_d and parts.
        ``reg_via_bucket``: the caller will use backward_to_flat(), which adds the dense-kernel
        regularisation gradient to the flat bucket itself (the loss then carries only its value)."""
        self._reg_via_bucket = reg_via_bucket
        self._reg_in_bucket = False
        self._begin_pass()                      # unconditionally: a captured step must contain the refresh of the piece planes
        y_g, y2_g = self._conditions(cond_g, cond2_g)
        # heads of the two-phase backward: the tensors the decoder / discriminator actually consume
        self._y_pair = tuple(t for t in self._ycat[2:] if t is not None) if self._ycat is not None else (y_g, y2_g)
        x_hat, z_mean, z_logvar = self.generator(data_g, y_g, y2_g, eps=eps)
        out = self.loss_terms(x_hat, gt, z_mean, z_logvar)
        out['prediction'] = x_hat
        out['z_mean'], out['z_logvar'] = z_mean, z_logvar
        loss_g = out['total_no_gan']
        if with_gan:
            smooth = 0.1
            # ONE discriminator pass over the generated batch serves both losses (the reference builds D(fake) once,
            # lib/models.py:299-302): loss_g is differentiated w.r.t. the generator/condition variables only and
            # loss_d w.r.t. the discriminator variables only (backward_to_flat), so neither gradient leaks.
            d_all = None
            if self.bug_compat or not ops.merged_d_pass(x_hat.shape[0]):
                d_fake = self.discriminator(x_hat, y_g, y2_g)
                y_d, y2_d = self._conditions(cond_d, cond2_d)
                if self.bug_compat:
                    with torch.no_grad():
                        d_real = self.discriminator(data_d, y_d, y2_d)
                else:
                    d_real = self.discriminator(data_d, y_d.detach(), y2_d.detach())
            else:
                # D(fake) and D(real) share weights and every operator on the path is per sample (:648-678; group norm
                # included): the two evaluations run as ONE pass over the concatenated batch [generated ; real] -- half
                # the launches of the discriminator's forward and of its weight-gradient sweep, and one weight-gradient
                # contraction per layer instead of two whose results autograd then adds.
                ycat_g = self._ycat[2] if self._ycat is not None else None       # (the generator's, from _conditions above)
                y_d, y2_d = self._conditions(cond_d, cond2_d)
                ycat_d = self._ycat[2] if self._ycat is not None else None
                # every discriminator variable is then used exactly once per step: its gradient kernels may write the
                # bucket directly and queue their reductions like the generator's (backward_to_flat flushes them)
                single = bool(reg_via_bucket and self._grad_views_d)
                if single:
                    self._grad_views.update(self._grad_views_d)
                try:
                    x_all = torch.cat([x_hat, data_d.to(x_hat.dtype)], 0)
                    if ycat_g is not None and ycat_d is not None:
                        # the fused condition networks already produced [y | y2]: one concat over the batch, and the
                        # gradient comes back to that tensor whole instead of through two slices
                        d_all = self.discriminator(x_all, None, None, cond=torch.cat([ycat_g, ycat_d.detach()], 0))
                    else:
                        d_all = self.discriminator(x_all, torch.cat([y_g, y_d.detach()], 0), torch.cat([y2_g, y2_d.detach()], 0))
                finally:
                    if single:
                        for nm in self._grad_views_d:
                            self._grad_views.pop(nm, None)
                nb = x_hat.shape[0]
                d_fake, d_real = d_all[:nb], d_all[nb:]
            if self.bug_compat or not d_fake.is_cuda or d_fake.dtype != torch.float32:
                out['gan_g'] = self._bce(d_fake, 1 - smooth)
                loss_g = loss_g + out['gan_g'] * self.lambda_gan
                if self.bug_compat:
                    d_fake = d_fake.detach()
                out['gan_d'] = self._bce(d_real, 1 - smooth) + self._bce(d_fake, smooth)
                out['loss_d'] = out['gan_d'] * self.lambda_gan
            else:
                # both adversarial terms (:381-390), scaled by lambda_gan (:393,397), and their gradients: one launch
                if d_all is not None:
                    lg, ld_, parts = ops.GanLossFn.apply(d_all, None, int(x_hat.shape[0]), smooth, float(self.lambda_gan))
                else:
                    lg, ld_, parts = ops.GanLossFn.apply(d_fake, d_real, int(d_fake.shape[0]), smooth, float(self.lambda_gan))
                out['gan_g'], out['gan_d'] = parts[0], parts[1]
                loss_g = loss_g + lg
                out['loss_d'] = ld_
        out['loss_g'] = loss_g
        return out

    def _one_scalar(self):
        if getattr(self, '_one', None) is None:
            self._one = torch.ones((), device=self.device, dtype=torch.float32)      # d(loss)/d(loss), allocated once
        ops.UNIT_GRAD = self._one                   # lets the loss op skip the multiplication by this constant
        return self._one

    @contextlib.contextmanager
    def _deferred_sweep(self):
        """Queue the reductions of one backward sweep and finish them when the sweep is over.  When the sweep ITSELF raised,
        the queues hold items whose buffers belong to an abandoned tape: they are dropped, not flushed, so that nothing
        stale reaches the bucket of a later call.  The failure is tracked explicitly -- an ambient exception
        of the caller (a step retried from inside an `except:` block) must not make a successful sweep drop its queued
        weight / group-norm / bias reductions."""
        ops.DEFERRED = []
        failed = False
        try:
            yield
        except BaseException:
            failed = True
            raise
        finally:
            try:
                if not failed:
                    ops.flush_deferred()
            finally:
                ops.DEFERRED = None
                ops.DEFERRED_DW[:] = []
                ops.DEFERRED_GN[:] = []

    @contextlib.contextmanager
    def _data_grad_only_through_d(self, active):
        """The generator sweep passes through D(fake) only for its data gradient: name the discriminator variables so
        that their layers skip the weight/bias-gradient kernels in this sweep (the discriminator sweep computes them)."""
        if not active:
            yield
            return
        ops.NO_WEIGHT_GRAD = {p.data_ptr() for p in self._opt_state['d']['params']}
        try:
            yield
        finally:
            ops.NO_WEIGHT_GRAD = None

    def backward_phase1(self, out):
        """First half of the two-phase backward (``split_backward``): everything downstream of the encoder's
        convolution stack -- decoder, dense layers, discriminator.  Afterwards the EARLY part of the G bucket
        ([0, split_off)) and the whole D bucket are final and may be exchanged while phase 2 runs."""
        st = self._opt_state['g']
        ne = st['n_early']
        one = self._one_scalar()
        with self._deferred_sweep():
            heads = [t for t in (self._enc_feat_cut,) + tuple(self._y_pair) if t.requires_grad]
            with self._data_grad_only_through_d('loss_d' in out):
                res = torch.autograd.grad(out['loss_g'], st['params'][:ne] + heads, grad_outputs=one, retain_graph=True, allow_unused=True)
            self.store_grads('g', res[:ne], 0, ne)
            self._phase_heads = (heads, list(res[ne:]))
            if 'loss_d' in out:
                grads_d = torch.autograd.grad(out['loss_d'], self._opt_state['d']['params'], grad_outputs=one, retain_graph=True,
                                              allow_unused=True)
                self.store_grads('d', grads_d)

    def backward_phase2(self):
        """Second half: from the cut (and the condition embeddings) through the encoder convolutions and the
        condition nets -> the LATE part of the G bucket."""
        st = self._opt_state['g']
        ne = st['n_early']
        heads, gouts = self._phase_heads
        roots, seeds = [], []
        for h, g in zip(heads, gouts):
            if g is not None:
                roots.append(self._enc_feat if h is self._enc_feat_cut else h)
                seeds.append(g)
        late = st['params'][ne:]
        try:
            with self._deferred_sweep():
                if late:
                    res = torch.autograd.grad(roots, late, grad_outputs=seeds, allow_unused=True) if roots else [None] * len(late)
                    self.store_grads('g', res, ne, None)
        finally:
            self._phase_heads = self._enc_feat = self._enc_feat_cut = None

    def backward_to_flat(self, out):
        """Gradients of loss_g w.r.t. the G group and loss_d w.r.t. the D group -> flat gradient buffers."""
        if getattr(self, 'split_backward', False) and not self.bug_compat and getattr(self, '_enc_feat_cut', None) is not None:
            self.backward_phase1(out)
            self.backward_phase2()
            return
        g_params = self._opt_state['g']['params']
        d_params = self._opt_state['d']['params']
        one = self._one_scalar()
        with self._deferred_sweep():
            self._backward_to_flat_single(out, g_params, d_params, one)

    def _backward_to_flat_single(self, out, g_params, d_params, one):
        if 'loss_d' not in out:
            grads_g = torch.autograd.grad(out['loss_g'], g_params, grad_outputs=one, allow_unused=True)
            self.store_grads('g', grads_g)
            return
        if self.bug_compat:
            grads_g = torch.autograd.grad(out['loss_g'], g_params, allow_unused=True)
            grads_d = [p.detach() for p in d_params]          # quirk C2: the WEIGHTS are clipped and applied
        else:
            # two sweeps over the shared D(fake) graph: the first needs only data gradients inside D, the second only
            # reaches the discriminator variables
            with self._data_grad_only_through_d(True):
                grads_g = torch.autograd.grad(out['loss_g'], g_params, grad_outputs=one, retain_graph=True, allow_unused=True)
            grads_d = torch.autograd.grad(out['loss_d'], d_params, grad_outputs=one, allow_unused=True)
        self.store_grads('g', grads_g)
        self.store_grads('d', grads_d)

    def train_step(self, data_g, cond_g, cond2_g, gt, data_d, cond_d, cond2_d, eps=None, grad_hook=None):
        """forward + backward + both optimiser updates on one (G batch, D batch) pair.
        ``grad_hook(flat_grad)`` runs between backward and the update (data-parallel all-reduce)."""
        out = self.forward_losses(data_g, cond_g, cond2_g, gt, data_d, cond_d, cond2_d, eps=eps, reg_via_bucket=True)
        self.backward_to_flat(out)
        out['lr_g'], out['lr_d'] = self.set_learning_rates()
        for grp in ('g', 'd'):
            if grad_hook is not None and not (grp == 'd' and self.bug_compat):
                grad_hook(self._opt_state[grp]['flat_grad'])
            self.apply_updates(grp)
            self.global_step += 1
        return out

    # ======================= checkpoints ============================================================
    def save_checkpoint(self, step):
        path = self._get_path('checkpoints')
        os.makedirs(path, exist_ok=True)
        arrays = self.variables()
        arrays['training/global_step'] = np.asarray(self.global_step, dtype=np.int64)
        if self._opt_state is not None:
            for grp in ('g', 'd'):
                st = self._opt_state[grp]
                arrays['training/momentum_' + grp] = st['m'].detach().cpu().numpy()
                if 'v' in st:                        # Adam: second moment and step count (bias correction)
                    arrays['training/adam_v_' + grp] = st['v'].detach().cpu().numpy()
                    arrays['training/adam_t_' + grp] = np.asarray(self.adam_steps(grp), dtype=np.int64)
        fn = os.path.join(path, 'model-%d.npz' % step)
        np.savez(fn, **arrays)
        keep = sorted(glob.glob(os.path.join(path, 'model-*.npz')), key=os.path.getmtime)
        for old in keep[:-5]:                     # tf.train.Saver(max_to_keep=5), reference :351
            os.remove(old)
        return fn

    def latest_checkpoint(self):
        """Newest checkpoint of this experiment: an ``.npz`` written by ``save_checkpoint`` or a TensorFlow
        bundle named by the directory's ``checkpoint`` state file (the reference's
        ``tf.train.latest_checkpoint``, :213) -- e.g. a pretrained model dropped into ``checkpoints/<name>/``."""
        path = self._get_path('checkpoints')
        files = glob.glob(os.path.join(path, 'model-*.npz'))
        newest = max(files, key=os.path.getmtime) if files else None
        tf_prefix = tf_checkpoint.latest_checkpoint(path)
        if tf_prefix is not None and (newest is None or
                                      os.path.getmtime(tf_prefix + '.index') > os.path.getmtime(newest)):
            return tf_prefix
        return newest

    # TF slot-variable names (tf.train.MomentumOptimizer / AdamOptimizer, reference :447-452)
    _SLOTS = {'m': {'momentum': '/Momentum', 'adam': '/Adam'}, 'v': {'adam': '/Adam_1'}}

    def _slot_suffix(self, buf):
        return self._SLOTS[buf].get('adam' if self.optimizer == 'adam' else 'momentum')

    def restore(self, filename):
        """Load variables (and optimiser state when present) from an ``.npz`` of ``save_checkpoint`` or from a
        TensorFlow checkpoint prefix (``.../model-1234``, files ``.index`` + ``.data-*``) with the variable
        names of the reference graph."""
        if os.path.isfile(filename + '.index'):
            arrays = tf_checkpoint.BundleReader(filename).read_all()
        elif filename.endswith('.index') and os.path.isfile(filename):
            arrays = tf_checkpoint.BundleReader(filename[:-len('.index')]).read_all()
        else:
            with np.load(filename) as ck:
                arrays = {k: ck[k] for k in ck.files}
        self.load_variables(arrays, strict=True)
        self.global_step = int(arrays.get('training/global_step', 0))
        if self._opt_state is None:
            return
        with torch.no_grad():
            for grp in ('g', 'd'):
                st = self._opt_state[grp]
                key = 'training/momentum_' + grp
                if key in arrays and arrays[key].shape == tuple(st['m'].shape):
                    st['m'].copy_(torch.from_numpy(arrays[key]).to(self.device))
                    if 'v' in st:
                        kv, kt = 'training/adam_v_' + grp, 'training/adam_t_' + grp
                        if kv in arrays and kt in arrays and arrays[kv].shape == tuple(st['v'].shape):
                            st['v'].copy_(torch.from_numpy(arrays[kv]).to(self.device))
                            self._set_adam_steps(grp, int(arrays[kt]))
                        else:
                            # first moment without second moment / step count: restart Adam's statistics instead of
                            # applying the t = 1 bias correction to a warm m (a 10x first step)
                            st['m'].zero_()
                            st['v'].zero_()
                            self._set_adam_steps(grp, 0)
                    continue
                for buf in ('m', 'v'):                     # per-variable TF slots -> flat bucket
                    suffix = self._slot_suffix(buf)
                    if suffix is None or buf not in st:
                        continue
                    for name, (off, _) in st['offsets'].items():
                        a = arrays.get(name + suffix)
                        if a is not None and a.size == self._vars[name].numel():
                            st[buf][off:off + a.size].copy_(
                                torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(self.device))
                if 't' in st:
                    b1p = arrays.get('training/beta1_power' if grp == 'g' else 'training/beta1_power_1')
                    self._set_adam_steps(grp, int(round(np.log(float(b1p)) / np.log(0.9))) if b1p is not None and 0 < float(b1p) < 1
                                         else self.global_step // 2)

    def export_tf_checkpoint(self, prefix=None, with_slots=True):
        """Write the variables as a TensorFlow V2 checkpoint the reference's ``tf.train.Saver`` can restore
        (names and layouts of its graph; optimiser slots as ``<var>/Momentum`` or ``<var>/Adam[_1]``) and
        record it in the directory's ``checkpoint`` state file."""
        if prefix is None:
            prefix = os.path.join(self._get_path('checkpoints'), 'model-%d' % self.global_step)
        arrays = dict(self.variables())
        arrays['training/global_step'] = np.asarray(self.global_step, dtype=np.int32)
        if with_slots and self._opt_state is not None:
            for grp in ('g', 'd'):
                st = self._opt_state[grp]
                for buf in ('m', 'v'):
                    suffix = self._slot_suffix(buf)
                    if suffix is None or buf not in st:
                        continue
                    flat = st[buf].detach().cpu().numpy()
                    for name, (off, _) in st['offsets'].items():
                        v = self._vars[name]
                        arrays[name + suffix] = flat[off:off + v.numel()].reshape(tuple(v.shape)).copy()
                if 't' in st:
                    tag = '' if grp == 'g' else '_1'
                    arrays['training/beta1_power' + tag] = np.asarray(0.9 ** self.adam_steps(grp), dtype=np.float32)
                    arrays['training/beta2_power' + tag] = np.asarray(0.999 ** self.adam_steps(grp), dtype=np.float32)
        tf_checkpoint.write_bundle(prefix, arrays)
        tf_checkpoint.update_checkpoint_state(os.path.dirname(os.path.abspath(prefix)), os.path.abspath(prefix))
        return prefix

    def _get_session(self, sess=None):
        """The reference restores the latest checkpoint on every inference call (:209-215, quirk C9);
        here weights are loaded once and cached.  Raises like the reference if nothing can be restored."""
        if sess is not None or self._weights_loaded:
            return self
        fn = self.latest_checkpoint()
        if fn is None:
            raise ValueError("no checkpoint found under %s (train with fit(), call restore() or "
                             "load_variables() first)" % self._get_path('checkpoints'))
        self.restore(fn)
        self._weights_loaded = True
        return self

    # ======================= training / inference drivers (reference :837-1174) ====================
    def _dev(self, a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(self.device)

    @staticmethod
    def _dense_np(a):
        return a if isinstance(a, np.ndarray) else a.toarray()

    def fit(self, data_wrapper):
        train_data, train_cond, train_cond2, train_labels = \
            data_wrapper.vertices_train, data_wrapper.cond1_train, data_wrapper.cond2_train, data_wrapper.vertices_train
        val_data, val_cond, val_cond2, val_labels = \
            data_wrapper.vertices_val, data_wrapper.cond1_val, data_wrapper.cond2_val, data_wrapper.vertices_val
        num_steps_epoch = int(train_data.shape[0] / self.batch_size)
        num_steps = self.num_epochs * num_steps_epoch
        t_start = time.time()
        if self.restart is not True:
            print('\n==========Loading from checkpoint {}...'.format(self.name))
            self._weights_loaded = False
            self._get_session()
            start_step = self.global_step
            end_step = start_step + num_steps
        else:
            ck = self._get_path('checkpoints')
            if 'rmtree_protection' in ck or ck.endswith('checkpoints/') or self.name == '':
                raise ValueError('Please provide an expriment name by setting the --name flag.')
            print('\n==========Start training from scratch...')
            shutil.rmtree(self._get_path('summaries'), ignore_errors=True)
            shutil.rmtree(ck, ignore_errors=True)
            os.makedirs(ck)
            self._init_optimizer()
            start_step = 1
            end_step = start_step + num_steps
        self._weights_loaded = True
        losses = []
        indices_g, indices_d = collections.deque(), collections.deque()
        # The step itself runs through the HIP-graph runner (cape_amd.runtime.GraphedTrainStep: the whole adversarial
        # step captured once and replayed -- the counterpart of the reference's static graph + sess.run, :905-906);
        # per step the host only stages the batch into the runner's static input buffers and draws eps.  The loss
        # averages (reference: ExponentialMovingAverage(0.9), :407-411) stay on the device and are read at epoch ends.
        from .runtime import GraphedTrainStep
        runner = GraphedTrainStep(self, with_gan=True, grad_hook=getattr(self, 'grad_hook', None))
        ema = torch.tensor([self._ema['g'], self._ema['d']], device=self.device, dtype=torch.float32)
        cur = torch.zeros(2, device=self.device, dtype=torch.float32)
        captured = False
        for step in range(start_step, end_step):
            if len(indices_g) < self.batch_size:
                indices_g.extend(np.random.permutation(train_data.shape[0]))
            if len(indices_d) < self.batch_size:
                indices_d.extend(np.random.permutation(train_data.shape[0]))
            idx_g = [indices_g.popleft() for _ in range(self.batch_size)]
            idx_d = [indices_d.popleft() for _ in range(self.batch_size)]
            runner.load_batch(data_g=self._dense_np(train_data[idx_g]), cond_g=train_cond[idx_g], cond2_g=train_cond2[idx_g],
                              gt=self._dense_np(train_labels[idx_g]), data_d=self._dense_np(train_data[idx_d]),
                              cond_d=train_cond[idx_d], cond2_d=train_cond2[idx_d])
            for _ in range(2 if self.bug_compat else 1):   # quirk C1: two sess.run, each applies both updates
                runner.buf['eps'].normal_()                # tf.random_normal inside the graph (:194): fresh per run
                if not captured:
                    runner.capture(preserve_state=True)
                    captured = True
                runner.step()
                torch.stack([runner.losses['loss_g'], runner.losses['loss_d']], out=cur)
                ema.mul_(0.9).add_(cur, alpha=0.1)
            if step % num_steps_epoch == 0 or step == num_steps:
                self._ema['g'], self._ema['d'] = (float(v) for v in ema.tolist())
                learning_rate_g = self._lr_at(self.lr_g, max(self.global_step - 2, 0))
                learning_rate_d = self._lr_at(self.lr_d, max(self.global_step - 2, 0))
                epoch = int(step * self.batch_size / train_data.shape[0])
                print('step {} / {} (epoch {} / {}):'.format(step, num_steps, epoch, self.num_epochs))
                print('  learning_rate_g = {:.2e}, loss_average_g = {:.2e}'.format(learning_rate_g, self._ema['g']))
                print('  learning_rate_d = {:.2e}, loss_average_d = {:.2e}'.format(learning_rate_d, self._ema['d']))
                string, recon_loss, latent_loss, edge_loss = self.evaluate(val_data, val_cond, val_cond2, val_labels, self)
                losses.append(recon_loss)
                print('  validation {}'.format(string))
                print('  time: {:.0f}s'.format(time.time() - t_start))
                self.save_checkpoint(step)
        self._ema['g'], self._ema['d'] = (float(v) for v in ema.tolist())
        t_step = (time.time() - t_start) / max(num_steps, 1)
        return losses, t_step

    def _batches(self, size):
        """(begin, end) of the batches of ``batch_size`` rows that cover ``range(size)`` in order; the last may be short."""
        for begin in range(0, size, self.batch_size):
            yield begin, min(begin + self.batch_size, size)

    def _padded_np(self, arr, begin, end):
        """The padded batch every driver feeds the network, on the host: a float32 block of ``batch_size`` rows with rows
        begin:end of ``arr`` (numpy or scipy.sparse) in front and zeros behind (reference :1035-1046).  An array of ONE row
        stands for all samples -- one condition, many z samples (reference :1155-1158) -- and is repeated into the valid rows."""
        out = np.zeros((self.batch_size,) + tuple(arr.shape[1:]), np.float32)
        out[:end - begin] = self._dense_np(arr[0:1] if arr.shape[0] == 1 else arr[begin:end])
        return out

    def _padded(self, arr, begin, end):
        return torch.from_numpy(self._padded_np(arr, begin, end)).to(self.device)

    def _open_pass(self, sess=None):
        """What every inference and fitting driver does once, before its loop and before it touches the device."""
        self._get_session(sess)
        self._begin_pass()

    def _embedded(self, size, cond, cond2):
        """(begin, end, y, y2) per padded batch: the condition embeddings on the device."""
        for begin, end in self._batches(size):
            yield (begin, end) + self._conditions(self._padded(cond, begin, end), self._padded(cond2, begin, end))

    def encode(self, data=None, cond=None, cond2=None):
        self._open_pass()
        zs = []
        with torch.no_grad():
            for begin, end, y, y2 in self._embedded(data.shape[0], cond, cond2):
                with self.variable_scope('generator'):
                    zm, zv = self.encoder(self._padded(data, begin, end), y, y2, use_res_block=self.use_res_block,
                                          use_cond=self.cond_encoder)
                zs.append([t[:end - begin].cpu().numpy() for t in (zm, zv, y, y2)])
        return tuple(np.concatenate(l, 0) for l in zip(*zs))

    def encode_only_condition(self, cond=None, cond2=None):
        self._open_pass()
        zs = []
        with torch.no_grad():
            for begin, end, y, y2 in self._embedded(cond.shape[0], cond, cond2):
                zs.append([t[:end - begin].cpu().numpy() for t in (y, y2)])
        return tuple(np.concatenate(l, 0) for l in zip(*zs))

    def _generated(self, data, cond, cond2, labels):
        """predict's and test_errors' loop: (begin, end, x_hat, labels_batch, loss_terms) per padded batch, all on the device;
        the last two are None without ``labels``.  The generator draws its eps here, once per batch."""
        for begin, end, y, y2 in self._embedded(data.shape[0], cond, cond2):
            x_hat, zm, zv = self.generator(self._padded(data, begin, end), y, y2)
            bl = lt = None
            if labels is not None:
                bl = self._padded(labels, begin, end)
                lt = self.loss_terms(x_hat, bl, zm, zv)
            yield begin, end, x_hat, bl, lt

    def _loss_averages(self, terms, size):
        """(recon, latent, edge) averaged over ``size`` samples from the per-batch loss_terms the way the reference does it
        (:1083-1086, quirk C8): the last batch is taken as zero-padded and weighs ``batch_size - num_zero_phs``, and with the
        float division of :1039 ``num_zero_phs`` is ``batch_size``: that weight is 0 up to rounding.  The scalars stayed on the
        device until here (nothing synchronises for them inside the loop) and come back in one copy."""
        # float64 holds an fp32 scalar, an fp64 one and a Python float alike exactly
        scal = lambda t: (t if torch.is_tensor(t) else torch.tensor(float(t), dtype=torch.float64)).reshape(()).double().to(self.device)
        per_batch = torch.stack([torch.stack([scal(lt[k]) for lt in terms]) for k in ('recon', 'latent', 'edge')]).cpu().numpy()
        num_zero_phs = self.batch_size * (size / self.batch_size + 1) - size
        return tuple((np.sum(c[:-1]) * self.batch_size + float(c[-1]) * (self.batch_size - num_zero_phs)) / size
                     for c in per_batch)

    def predict(self, data, cond=None, cond2=None, labels=None, sess=None, phase='train'):
        self._open_pass(sess)
        preds, terms = [], []
        with torch.no_grad():
            for begin, end, x_hat, _, lt in self._generated(data, cond, cond2, labels):
                terms.append(lt)
                preds.append(x_hat[:end - begin].cpu().numpy())
            predictions = np.concatenate(preds, 0)
            if labels is None:
                return predictions
            return (predictions,) + self._loss_averages(terms, data.shape[0])

    def evaluate(self, data, cond=None, cond2=None, labels=None, sess=None):
        t_start = time.time()
        predictions, loss_recon, loss_latent, loss_edge = self.predict(data, cond, cond2, labels, sess)
        string = 'recon loss: {:.2e}, latent loss: {:.2e}, edge_loss: {:.2e}' \
                 '(weighted)'.format(loss_recon * self.lambda_l1, loss_latent * self.lambda_latent,
                                     loss_edge * self.lambda_edge)
        if sess is None:
            string += '\ntime: {:.0f}s'.format(time.time() - t_start)
        return string, loss_recon, loss_latent, loss_edge

    def test_errors(self, data, cond=None, cond2=None, labels=None, std=None, clothing_idx=None, quantiles=(0.5,),
                    return_distances=False):
        """The reference's test-set number (demos.py:63-85): the per-vertex Euclidean distance between reconstruction and
        ``labels`` (default: ``data``), de-normalised by the training set's ``std`` ((V, 3), (3,), a scalar; default ones) and
        restricted to ``clothing_idx`` (default every vertex, used in the order given), with its statistics -- all on the
        device.  Batching, padding and seeding are predict's; per batch the generator, the losses and one distance
        launch on the valid rows; at the end one statistics call, whose results come back in one small copy (the per-batch loss
        scalars in another).  No prediction goes to the host and nothing synchronises inside the loop.
        Returns a dict: recon / latent / edge (predict's averages, quirk C8), euclidean_mean, euclidean_std (population),
        euclidean_median (when 0.5 is among ``quantiles``), quantiles {q: value} (numpy's linear rule, at most 4),
        per_vertex_mean [Vc], per_sample_mean [size], count, nonfinite (> 0: mean, std and quantiles are NaN), and
        distances [size, Vc] float32 when ``return_distances``."""
        size = data.shape[0]
        sd, idx, qs = ops.error_arguments(self.input_num_verts, self.nn_input_channel, size, std, clothing_idx, quantiles)
        if labels is None:
            labels = data
        self._open_pass()
        sd_dev = torch.tensor(sd, dtype=torch.float32, device=self.device)
        idx_dev = torch.tensor(idx, dtype=torch.int32, device=self.device)
        dist = torch.empty((size, idx.size), dtype=torch.float32, device=self.device)
        terms = []
        with torch.no_grad():
            for begin, end, x_hat, bl, lt in self._generated(data, cond, cond2, labels):
                terms.append(lt)
                xv = x_hat[:end - begin]
                ops.vertex_error(xv if xv.dtype == torch.float32 else xv.float(), bl[:end - begin], sd_dev, idx_dev, dist,
                                 row0=begin)
            res = ops.error_statistics(dist, qs)
            res['recon'], res['latent'], res['edge'] = self._loss_averages(terms, size)
        del res['order_ranks'], res['order_values'], res['euclidean_var']
        if return_distances:
            res['distances'] = dist.cpu().numpy()
        return res

    def _decoded(self, data, cond, cond2):
        """decode's loop: (begin, end, x) per padded batch, ``x`` the decoder's output for all ``batch_size`` rows on the
        device.  One condition row stands for every z sample (``_padded_np``)."""
        for begin, end in self._batches(data.shape[0]):
            bz, bc, bc2 = (self._padded(a, begin, end) for a in (data, cond, cond2))
            with self.variable_scope('generator'):
                x = self.decoder_cond_vert(bz, bc, bc2, use_res_block=self.use_res_block_dec)
            yield begin, end, x

    def decode(self, data, cond=None, cond2=None):
        self._open_pass()
        with torch.no_grad():
            return np.concatenate([x[:end - begin].cpu().numpy() for begin, end, x in self._decoded(data, cond, cond2)], 0)

    def _posed_arguments(self, size, body_model, pose, transl, dress, cond=None, cond2=None):
        """What decode_posed and fit_posed share of their arguments: the body model, ``pose`` [1 or size, 3J] and ``transl``
        [1 or size, 3] (or None) as float32, ``cond`` / ``cond2`` (when given: one row or one per sample, the same for both)
        as float32, and the dressing arrays of ``dress`` = (mean, std, clothing_idx, minimal_shape) on the device."""
        from . import smpl as smpl_mod
        body = getattr(body_model, 'model', body_model)
        pose = np.asarray(pose, dtype=np.float32).reshape(-1, 3 * body.J)
        if pose.shape[0] not in (1, size):
            raise ValueError("pose: %d rows for %d samples" % (pose.shape[0], size))
        if transl is not None:
            transl = np.asarray(transl, dtype=np.float32).reshape(-1, 3)
            if transl.shape[0] not in (1, size):
                raise ValueError("transl: %d rows for %d samples" % (transl.shape[0], size))
        if cond is not None:
            cond, cond2 = np.asarray(cond, dtype=np.float32), np.asarray(cond2, dtype=np.float32)
            if cond.shape[0] not in (1, size) or cond2.shape[0] != cond.shape[0]:
                raise ValueError("cond / cond2: one row, or one per sample")
        mean, std, clothing_idx, minimal_shape = dress
        dressing = smpl_mod._DressArrays(mean, std, clothing_idx, self.verts_ref if minimal_shape is None else minimal_shape,
                                         body.V, self.device)
        return body, pose, transl, dressing, cond, cond2

    def _fit_arguments(self, size, body, pose, transl, dress, cond, cond2, z0, steps, optimize_transl):
        """What fit_posed and fit_scan share of their arguments: ``_posed_arguments`` (``transl`` zeros when it is a leaf and
        None), the starting codes ``z0`` [size, nz] (zeros) and ``steps``."""
        nz = int(self.nz)
        if transl is None and optimize_transl:
            transl = np.zeros((size, 3), np.float32)
        _, pose, transl, dressing, cond, cond2 = self._posed_arguments(size, body, pose, transl, dress, cond, cond2)
        z0 = np.zeros((size, nz), np.float32) if z0 is None else np.asarray(z0, dtype=np.float32)
        if z0.shape != (size, nz):
            raise ValueError("z0: [%d, %d] expected" % (size, nz))
        return pose, transl, dressing, cond, cond2, z0, int(steps)

    def decode_posed(self, data, cond, cond2, pose, body_model, mean, std, clothing_idx, minimal_shape=None, transl=None,
                     return_normals=False):
        """``decode`` followed by demos.py's posing step (:155-161 / :207-213 dress, :267-283 / :312-326 SMPL forward), on
        the device per padded batch: decoder -> cape_smpl_dress -> cape_smpl_joints -> cape_smpl_skin.  ``pose`` [size, 72]
        or [1, 72] (one pose for every sample), ``transl`` likewise or None; ``body_model`` a ``cape_amd.smpl.SMPL`` (or the
        object ``cape_amd.smpl.create`` returns); ``minimal_shape`` defaults to the template mesh.  Batching, padding and the
        one-condition-many-samples rule are decode's.  Returns (posed, clothed_unposed) [size, V, 3] float32; with
        ``return_normals`` a third array, the per-vertex normals of the posed meshes [size, V, 3] (``SMPL.vertex_normals`` on
        the model's faces: uniform weights, unit length, zero where a vertex has no non-degenerate face), computed on the
        device per batch before the copy to the host."""
        body, pose, transl, dressing, _, _ = self._posed_arguments(data.shape[0], body_model, pose, transl,
                                                                   (mean, std, clothing_idx, minimal_shape))
        self._open_pass()
        posed, clothed, normals = [], [], []
        with torch.no_grad():
            for begin, end, x in self._decoded(data, cond, cond2):
                nb = end - begin
                T = dressing(x[:nb].float().contiguous())
                vo, _ = body.forward(T, self._padded(pose, begin, end)[:nb], None,
                                     None if transl is None else self._padded(transl, begin, end)[:nb])
                if return_normals:
                    normals.append(body.vertex_normals(vo).cpu().numpy())
                posed.append(vo.cpu().numpy())
                clothed.append(T.cpu().numpy())
        if return_normals:
            return np.concatenate(posed, 0), np.concatenate(clothed, 0), np.concatenate(normals, 0)
        return np.concatenate(posed, 0), np.concatenate(clothed, 0)

    def encode_posed(self, posed, pose, cond, cond2, body_model, mean, std, clothing_idx=None, minimal_shape=None, transl=None,
                     betas=None, joints_from=None, return_disp=False):
        """``decode_posed`` the other way: posed registrations in SMPL topology -> what ``encode`` returns.  Per padded batch on
        the device: ``SMPL.unpose`` (demos.py's posing step inverted) -> ``undress`` (``v_cano - minimal`` of the reference's
        lib/prep_data.py:74, masked and normalised) -> encoder.  ``posed`` [size, V, 3]; ``pose`` / ``transl`` / ``body_model``
        / ``mean`` / ``std`` / ``minimal_shape`` as in ``decode_posed``, ``clothing_idx=None``: every vertex; ``betas``
        [1 or size, <=B] or None; ``joints_from`` [1 or size, V, 3] as in ``SMPL.unpose`` (None: the exact inverse);
        ``cond`` / ``cond2`` as ``encode`` takes them.  Batching and padding are encode's.  Returns (z_mean, z_logvar, y, y2),
        and with ``return_disp`` the normalised displacements [size, V, 3] the encoder saw as a fifth."""
        posed = np.asarray(posed, dtype=np.float32)
        size = posed.shape[0]
        body, pose, transl, dressing, _, _ = self._posed_arguments(size, body_model, pose, transl,
                                                                   (mean, std, clothing_idx, minimal_shape))
        if posed.shape != (size, body.V, 3):
            raise ValueError("posed: [size, %d, 3] expected, got %s" % (body.V, posed.shape))

        def rows(name, a, tail):
            a = np.asarray(a, dtype=np.float32).reshape((-1,) + tail)
            if a.shape[0] not in (1, size):
                raise ValueError("%s: %d rows for %d samples" % (name, a.shape[0], size))
            return a

        betas = None if betas is None else rows("betas", betas, (np.asarray(betas).shape[-1],))
        jf = None if joints_from is None else rows("joints_from", joints_from, (body.V, 3))
        jf_all = self._dev(jf) if jf is not None and jf.shape[0] == 1 else None          # one body for every sample: uploaded once
        self._open_pass()
        zs, disps = [], []
        with torch.no_grad():
            for begin, end, y, y2 in self._embedded(size, cond, cond2):
                nb = end - begin
                part = lambda a: None if a is None else self._padded(a, begin, end)[:nb]
                T, _ = body.unpose(part(posed), part(pose), part(betas), part(transl),
                                   joints_from=jf_all if jf_all is not None else part(jf))
                x = torch.zeros((self.batch_size, body.V, 3), dtype=torch.float32, device=self.device)   # encode's zero padding
                dressing.undress(T, out=x[:nb])
                with self.variable_scope('generator'):
                    zm, zv = self.encoder(x, y, y2, use_res_block=self.use_res_block, use_cond=self.cond_encoder)
                zs.append([t[:nb].cpu().numpy() for t in (zm, zv, y, y2)])
                if return_disp:
                    disps.append(x[:nb].cpu().numpy())
        res = tuple(np.concatenate(l, 0) for l in zip(*zs))
        return res + (np.concatenate(disps, 0),) if return_disp else res

    def fit_posed(self, target, pose, cond, cond2, body_model, mean, std, clothing_idx, minimal_shape=None, transl=None, z0=None,
                  weights=None, steps=200, lr=0.1, lambda_z=0.0, lambda_edge=0.0, optimize_pose=False, optimize_transl=False,
                  lambda_vnormal=0.0):
        """The latent codes that explain posed meshes: gradient descent (Adam) on ``z`` through
        decoder -> cape_smpl_dress -> SMPL posing, all on the device (``smpl.dress_diff`` / ``SMPL.forward_diff``).

        ``target`` [size, V, 3] posed meshes in SMPL topology; ``pose`` / ``transl`` / ``body_model`` / ``mean`` / ``std`` /
        ``clothing_idx`` / ``minimal_shape`` as in ``decode_posed``; ``cond`` / ``cond2`` condition EMBEDDINGS, one row for all
        samples or one per sample (decode_posed's rule); ``z0`` [size, nz] the starting codes (zeros); ``weights`` [V]
        per-vertex weights of the data term (ones).  Per sample the objective is

            sum_v w_v |posed_v - target_v|^2 / sum_v w_v  +  lambda_z mean(z^2)  [+ lambda_edge edge(posed, target)]
                [+ lambda_vnormal sum_v w_v (1 - n_v(posed) . n_v(target)) / sum_v w_v]

        (edge: the training loss's edge term between the posed mesh and the target, per sample; asking for it costs one
        element-wise product and one sum on [N, V, 3] per step in torch, where the two gradients meet.  vnormal: VERTEX normals
        on the body model's faces, ``SMPL.vertex_normals_diff`` -- not the training option ``lambda_normal``, which is face
        normals; the target's normals are computed once per batch, the term's gradient -lambda_vnormal w_v n_v(target) / sum w
        is a constant of the batch and enters the one backward call next to the data gradient; the term's value costs one
        product and one sum on [N, V, 3] per step in torch.)  The leaves are ``z``, and
        ``pose`` / ``transl`` with ``optimize_pose`` / ``optimize_transl`` (``transl`` then starts at zero when None); the
        samples are independent.  The model's variables take no gradient and no weight-gradient kernel runs; optimiser state
        and gradient buckets stay as a ``decode`` call leaves them.  The defaults (200 steps, lr 0.1, lambda_z 0) come from
        the synthetic recovery run of DESIGN 7f; the data term is in squared metres (about 1e-6 for a code one standard
        deviation off), so a useful ``lambda_z`` is of that order or below.  The rows of ``loss`` before the last come from
        the differentiated forward, whose decoder kernels differ from ``decode``'s in the last bit; the last row, ``posed``
        and ``clothed`` are evaluated exactly as ``decode_posed`` evaluates the returned leaves.

        Returns a dict: ``z`` [size, nz], ``pose`` [size, 3J], ``transl`` [size, 3] or None, ``posed`` / ``clothed``
        [size, V, 3] for the returned leaves, ``loss`` [steps + 1, size] the data term per sample (row 0: before the first
        update), and with ``lambda_vnormal > 0`` ``normal`` [steps + 1, size], the vertex-normal term per sample before the
        multiplication by ``lambda_vnormal``."""
        from . import smpl as smpl_mod
        body = getattr(body_model, 'model', body_model)
        target = np.asarray(target, dtype=np.float32)
        size, V, bs = target.shape[0], body.V, self.batch_size
        if target.shape != (size, V, 3):
            raise ValueError("target: [size, %d, 3] expected, got %s" % (V, target.shape))
        pose, transl, dressing, cond, cond2, z0, steps = self._fit_arguments(
            size, body, pose, transl, (mean, std, clothing_idx, minimal_shape), cond, cond2, z0, steps, optimize_transl)
        w = np.ones(V, np.float32) if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
        if w.shape != (V,) or not float(w.sum()) > 0.0:
            raise ValueError("weights: [%d] with a positive sum expected" % V)
        lambda_vnormal = float(lambda_vnormal)
        if not np.isfinite(lambda_vnormal) or lambda_vnormal < 0:
            raise ValueError("lambda_vnormal must be finite and >= 0, got %r" % (lambda_vnormal,))
        inv_wsum = 1.0 / float(w.astype(np.float64).sum())
        w_dev = self._dev(w)
        self._open_pass()
        if lambda_edge:
            _, ed, vptr, vidx = self._edge_tables()
            no_ref = torch.zeros((V, 3), dtype=torch.float32, device=self.device)

        def data_term(begin, end):
            nb = end - begin
            tgt = self._padded(target, begin, end)
            series = _Series(steps, bs, self.device, loss=torch.float32, **(dict(normal=torch.float32) if lambda_vnormal else {}))
            grad = torch.zeros((bs, V, 3), dtype=torch.float32, device=self.device)       # padded rows stay zero
            if lambda_vnormal:
                # w_v n_v(target) / sum w in fp64 (the term's value is summed in fp64), padded rows zero; the term's
                # gradient to the posed normals is -lambda_vnormal times that, the same at every step
                with torch.no_grad():
                    tnw = body.vertex_normals(tgt).double() * (w_dev.double() * inv_wsum)[None, :, None]
                    tnw[nb:] = 0.0
                    g_normal = (-lambda_vnormal * tnw).float()

            def term(step, posed, want_grad):
                smpl_mod.weighted_l2(posed, tgt, w_dev, inv_wsum, nb, series['loss'][step], grad if want_grad else None)
                roots, seeds = [posed], [grad]
                if lambda_vnormal:
                    nrm = body.vertex_normals_diff(posed) if want_grad else body.vertex_normals(posed)
                    # sum_v w_v / sum w = 1: the term is 1 - sum_v w_v n_v . n_v(target) / sum w
                    series['normal'][step, :nb] = (1.0 - (nrm.detach().double() * tnw).sum((1, 2)))[:nb].float()
                if lambda_edge and want_grad:
                    # the batch mean of the training loss's edge term, scaled back to a sum over the samples
                    e_total, _ = ops.ReconEdgeLossFn.apply(posed[:nb], tgt[:nb], no_ref, ed, vptr, vidx, 0.0,
                                                           float(lambda_edge) * nb)
                    roots.append(e_total)
                    seeds.append(None)
                if lambda_vnormal:
                    roots.append(nrm)
                    seeds.append(g_normal)
                return roots, seeds

            return term, series

        return self._fit_leaves(size, body, dressing, z0, cond, cond2, pose, transl, steps, lr, lambda_z, optimize_pose,
                                optimize_transl, data_term)

    def _fit_leaves(self, size, body, dressing, z0, cond, cond2, pose, transl, steps, lr, lambda_z, optimize_pose, optimize_transl,
                    data_term):
        """fit_posed's and fit_scan's batch loop: Adam on the leaves ``z`` (and ``pose`` / ``transl``) of
        decoder -> ``dressing.diff`` -> ``body.forward_diff`` per padded batch, with the model's variables frozen and its
        gradient buckets out of reach, and a last evaluation of the returned leaves as ``decode_posed`` evaluates them.
        ``data_term(begin, end)`` returns per batch (term, series): ``term(step, posed, want_grad)`` records the step's values
        in ``series`` (a ``_Series``: the batch's per-sample arrays [steps + 1, nb] by name) and returns the (roots, seeds) of
        the one backward call.  Arguments as ``_posed_arguments`` returns them; the device pass is open."""
        bs, nz = self.batch_size, int(self.nz)
        res = dict(z=[], pose=[], transl=[], posed=[], clothed=[])
        # the model's variables are constants here: no gradient bucket to write into and, while the steps run, nothing that
        # requires a gradient (the ops then skip their weight-gradient kernels)
        grad_views, self._grad_views = self._grad_views, {}
        trainable = [v for v in self._vars.values() if v.requires_grad]

        def freeze(on):
            for v in trainable:
                v.requires_grad_(not on)

        try:
            for begin, end in self._batches(size):
                nb = end - begin
                # one condition row stands for every sample, in the valid rows only: the batches decode_posed feeds the decoder
                z, bc, bc2, bp = (self._padded(a, begin, end) for a in (z0, cond, cond2, pose))
                z.requires_grad_(True)
                bp.requires_grad_(bool(optimize_pose))
                bt = None if transl is None else self._padded(transl, begin, end).requires_grad_(bool(optimize_transl))
                leaves = [z] + ([bp] if optimize_pose else []) + ([bt] if optimize_transl else [])
                opt = torch.optim.Adam(leaves, lr=float(lr))
                term, series = data_term(begin, end)

                def evaluate(step, want_grad):
                    with self.variable_scope('generator'):
                        x = self.decoder_cond_vert(torch.cat([z, bc, bc2], 1), bc, bc2, use_res_block=self.use_res_block_dec)
                    T = dressing.diff(x.float().contiguous())
                    posed, _ = body.forward_diff(T, bp, None, bt)
                    return (T, posed) + tuple(term(step, posed, want_grad))

                freeze(True)
                try:
                    for step in range(steps):
                        T, posed, roots, seeds = evaluate(step, True)
                        opt.zero_grad(set_to_none=True)
                        torch.autograd.backward(roots, seeds)
                        if lambda_z:
                            z.grad.add_(z.detach(), alpha=2.0 * float(lambda_z) / nz)
                        opt.step()
                finally:
                    freeze(False)
                with torch.no_grad():            # the returned leaves as decode_posed evaluates them, kernel for kernel
                    T, posed, _, _ = evaluate(steps, False)
                res['z'].append(z.detach()[:nb].cpu().numpy())
                res['pose'].append(bp.detach()[:nb].cpu().numpy())
                res['transl'].append(None if bt is None else bt.detach()[:nb].cpu().numpy())
                res['posed'].append(posed[:nb].cpu().numpy())
                res['clothed'].append(T[:nb].cpu().numpy())
                for k, a in series.numpy(nb).items():
                    res.setdefault(k, []).append(a)
        finally:
            self._grad_views = grad_views
        cat = lambda k, ax=0: np.concatenate(res[k], ax)
        out = dict(z=cat('z'), pose=cat('pose'), transl=None if transl is None else cat('transl'), posed=cat('posed'),
                   clothed=cat('clothed'))
        for k in res:
            if k not in out:
                out[k] = cat(k, 1)
        return out

    def fit_scan(self, scan, pose, cond, cond2, body_model, mean, std, clothing_idx, minimal_shape=None, transl=None, z0=None,
                 steps=200, lr=0.1, lambda_z=0.0, optimize_pose=False, optimize_transl=False, max_dist=None, lambda_mesh=0.0,
                 mesh_weights=None, mesh_max_dist=None, scan_normals=None, normal_angle=None):
        """``fit_posed`` for raw scans -- points without correspondence: gradient descent (Adam) on ``z`` through
        decoder -> cape_smpl_dress -> SMPL posing -> scan-to-mesh distance (``SMPL.scan_distance_diff``: for every scan point
        the closest point of the posed surface, searched over all faces on the device at every step).

        ``scan`` a [size, M, 3] array, or a list of ``size`` arrays [m_n, 3] with m_n >= 1; everything else as in
        ``fit_posed``, which this shares its loop with.  Per sample the objective is

            (1 / m_n) sum_i [d2_i <= max_dist^2] d2_i  +  lambda_z mean(z^2)

        with d2_i the squared distance of scan point i to the posed mesh.  ``max_dist`` (metres; None: no truncation) drops the
        points farther than that from the current mesh: the mask comes from each step's forward and is a constant of that
        step's gradient.  Points without a finite distance (a non-finite coordinate) are dropped likewise.

        That term alone pulls every scan point's closest surface point and nothing else: it cannot see a part of the surface
        that no scan point chose.  ``lambda_mesh > 0`` adds the opposite, mesh-to-scan term (``SMPL.point_distance_diff``;
        DESIGN 7j), which makes the objective two-sided (chamfer):

            +  lambda_mesh  sum_v w_v [e2_v <= mesh_max_dist^2] e2_v / sum_v w_v

        with e2_v the squared distance of posed vertex v to the nearest of the sample's scan points, searched over all points
        on the device at every step, and w ``mesh_weights`` [V] (None: ones; a positive sum is required).  The term samples
        the mesh AT ITS VERTICES (about 1 cm apart on SMPL), not on the face interiors.  ``mesh_max_dist`` (metres; None: no
        truncation) drops the vertices farther than that from the scan -- what a partial scan needs; the mask comes from each
        step's forward and is a constant of that step's gradient, and a distance that is NaN is dropped.  The scan is a
        constant: no gradient to its points is computed.  With ``lambda_mesh = 0`` nothing of this runs.

        ``scan_normals`` and ``normal_angle``, both or neither, accept a correspondence only where the two normals agree
        within ``normal_angle`` degrees (0 < normal_angle < 180) -- what keeps the two sides of a sleeve, or an arm
        and the torso, from being pulled onto each other.  ``scan_normals`` has the form of ``scan`` (an array or a list) and
        holds unit normals pointing out of the scanned surface; for a scan that is a mesh they are
        ``VertexNormals(scan_faces, n).np(scan_verts)``.  A scan point searches only the faces whose normal has a cosine of at
        least cos(normal_angle) with its own; with ``lambda_mesh > 0`` a vertex likewise searches only the scan points that
        agree with its vertex normal (the posed mesh's, computed once per step, a constant of the gradient).  A point or
        vertex without a compatible partner has a NaN distance and is dropped by the masks above, so ``inliers`` and
        ``mesh_inliers`` keep their meaning.  Without ``scan_normals`` nothing of this is constructed or launched.

        Returns a dict: ``z``, ``pose``, ``transl``, ``posed``, ``clothed`` as ``fit_posed`` returns them, ``loss``
        [steps + 1, size] the scan-to-mesh term per sample (row 0: before the first update; the last row for the returned
        leaves) and ``inliers`` [steps + 1, size], the number of points under the mask; with ``lambda_mesh > 0`` also
        ``mesh_loss`` [steps + 1, size], the mesh-to-scan term before the multiplication by ``lambda_mesh``, and
        ``mesh_inliers`` [steps + 1, size], the number of vertices with a positive weight under its mask."""
        from .scan_distance import pad_normals, pad_points
        lambda_mesh = float(lambda_mesh)
        if not np.isfinite(lambda_mesh) or lambda_mesh < 0:
            raise ValueError("lambda_mesh must be finite and >= 0, got %r" % (lambda_mesh,))
        if mesh_max_dist is not None:
            mesh_max_dist = float(mesh_max_dist)
            if not mesh_max_dist >= 0.0:
                raise ValueError("mesh_max_dist must be >= 0 or None, got %r" % (mesh_max_dist,))
        body = getattr(body_model, 'model', body_model)
        pts, count = pad_points(scan)
        size, M, V, bs = pts.shape[0], pts.shape[1], body.V, self.batch_size
        if (scan_normals is None) != (normal_angle is None):
            raise ValueError("scan_normals and normal_angle: both or neither")
        nrm = None
        if scan_normals is not None:
            normal_angle = float(normal_angle)
            if not 0.0 < normal_angle < 180.0:
                raise ValueError("normal_angle must lie in (0, 180) degrees, got %r" % (normal_angle,))
            nrm = pad_normals("scan_normals", scan_normals, pts, count)
            cos_min = float(np.cos(np.deg2rad(normal_angle)))
        if count is None:
            count = np.full(size, M, np.int32)
        mw = np.ones(V, np.float32) if mesh_weights is None else np.asarray(mesh_weights, dtype=np.float32)
        if mw.shape != (V,) or not float(mw.astype(np.float64).sum()) > 0.0:
            raise ValueError("mesh_weights: [%d] with a positive sum expected" % V)
        if max_dist is not None:
            max_dist = float(max_dist)
            if not max_dist >= 0.0:
                raise ValueError("max_dist must be >= 0 or None, got %r" % (max_dist,))
        pose, transl, dressing, cond, cond2, z0, steps = self._fit_arguments(
            size, body, pose, transl, (mean, std, clothing_idx, minimal_shape), cond, cond2, z0, steps, optimize_transl)
        limit = float('inf') if max_dist is None else max_dist * max_dist
        mesh_limit = float('inf') if mesh_max_dist is None else mesh_max_dist * mesh_max_dist
        self._open_pass()
        if lambda_mesh:
            mw_dev = self._dev(mw).double()[None]
            mw_pos = self._dev(mw)[None] > 0
            inv_mwsum = 1.0 / float(mw.astype(np.float64).sum())

        def data_term(begin, end):
            nb = end - begin
            p = self._padded(pts, begin, end)
            near_kw, mesh_kw = {}, {}
            if nrm is not None:
                pn = self._padded(nrm, begin, end)
                near_kw, mesh_kw = dict(normals=pn, cos_min=cos_min), dict(point_normals=pn, cos_min=cos_min)
            cnt = np.zeros(bs, np.int32)                                                  # padded rows: no points
            cnt[:nb] = count[begin:end]
            counts = body._scan_distance().counts(cnt, bs, M)                             # checked and uploaded once
            cnt_dev = counts[1]
            inv_m = (1.0 / torch.as_tensor(np.maximum(cnt, 1)).to(self.device).double())[:, None]
            valid = torch.arange(M, device=self.device)[None, :] < cnt_dev[:, None]
            series = _Series(steps, bs, self.device, loss=torch.float32, inliers=torch.int32,
                             **(dict(mesh_loss=torch.float32, mesh_inliers=torch.int32) if lambda_mesh else {}))

            def term(step, posed, want_grad):
                d2 = (body.scan_distance_diff(posed, p, counts, **near_kw) if want_grad
                      else body.scan_distance(posed, p, counts, **near_kw)[0])
                d = d2.detach()
                mask = valid & (d <= limit)                                               # a NaN distance is no inlier
                md = mask.double()
                series['loss'][step] = ((d.double() * md).nan_to_num_(nan=0.0).sum(1, keepdim=True) * inv_m)[:, 0].float()
                series['inliers'][step] = mask.sum(1).int()
                roots, seeds = [d2], [(md * inv_m).float()]
                if lambda_mesh:
                    # the same checked counts: a padded row has none, its vertices come back NaN and are dropped
                    e2 = (body.point_distance_diff(posed, p, counts, **mesh_kw) if want_grad
                          else body.point_distance(posed, p, counts, **mesh_kw)[0])
                    e = e2.detach()
                    near = e <= mesh_limit                                                # a NaN distance is no inlier
                    wm = near.double() * mw_dev
                    series['mesh_loss'][step] = ((e.double() * wm).nan_to_num_(nan=0.0).sum(1) * inv_mwsum).float()
                    series['mesh_inliers'][step] = (near & mw_pos).sum(1).int()
                    roots.append(e2)
                    seeds.append((wm * (lambda_mesh * inv_mwsum)).float())
                return roots, seeds

            return term, series

        return self._fit_leaves(size, body, dressing, z0, cond, cond2, pose, transl, steps, lr, lambda_z, optimize_pose,
                                optimize_transl, data_term)
