"""Small synthetic graphs for the on-chip Chebyshev recurrence (csrc/cheb_fused.hip, cape_amd.graph.ChebPatchPlan): their
normalised Laplacians, the float64 reference of the layer and its gradients, and the numpy restatement of the patch-local
algorithm the kernels run.  TEST INFRASTRUCTURE ONLY (tests/test_cheb_synth_host.py, tests/test_gpu_cheb_fused.py,
tests/test_cheb_patch_plan.py).

Every Laplacian L = I - D^-1/2 A D^-1/2 (an isolated vertex keeps its diagonal 1, so its row of L~ = L - I is EMPTY) is rounded
to float32 before anything uses it: the plan uploads float32 values, and a reference built from the unrounded operator would put
the operator's rounding (1e-7) into every comparison.

FAMILIES names the graphs, EXPECT the plan each must get per (K, Cin) -- P, the range of the patch sizes, the range of
patch + halo -- or REFUSED where ChebPatchPlan must decline.  tests/test_cheb_synth_host.py asserts those facts on the CPU, so
that a change of the partitioner cannot silently move a case off the edge it is there for."""
import numpy as np
import scipy.sparse as sp

FOUT = 32


# ---- graphs (symmetric 0/1 adjacency, no self loops) ----------------------------------------------------------------------------
def _adj(M, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    A = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(M, M)).tocsr()
    A = ((A + A.T) > 0).astype(np.float64).tocsr()
    A.sort_indices()
    return A


def ring(M, hops=(1,)):
    """Vertex i next to i +- h for every h in ``hops`` (M = 1: one isolated vertex; M = 2: one edge)."""
    i = np.arange(M)
    return _adj(M, np.concatenate([np.stack([i, (i + h) % M], 1) for h in hops]))


def path(M):
    i = np.arange(M - 1)
    return _adj(M, np.stack([i, i + 1], 1))


def tri_grid(w, h):
    """w x h vertices (vertex = row * w + column), every cell split by the diagonal (r, c) - (r + 1, c + 1): interior rows of 6
    entries, edges 4, two corners 3 and two corners 2."""
    v = np.arange(w * h).reshape(h, w)
    return _adj(w * h, np.concatenate([np.stack([v[:, :-1].ravel(), v[:, 1:].ravel()], 1),
                                       np.stack([v[:-1].ravel(), v[1:].ravel()], 1),
                                       np.stack([v[:-1, :-1].ravel(), v[1:, 1:].ravel()], 1)]))


def isolate(A, v):
    A = A.tolil()
    A[v, :] = 0
    A[:, v] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    return A


def hub_grid():
    """tri_grid(20, 20) with five extra edges at the corner vertex 0 (3 + 5 = 8 entries) to vertices on the far borders, whose rows
    grow from 4 to 5 (and the 2-entry corner 19 to 3): every other row keeps 2 .. 6."""
    A = tri_grid(20, 20).tolil()
    for t in (19, 399 - 7, 20 * 9 + 19, 20 * 19 + 4, 20 * 14 + 19):
        A[0, t] = A[t, 0] = 1.0
    return A.tocsr()


def disjoint(A, B):
    return sp.block_diag([A, B], format="csr")


def matchings(M, count, seed):
    """Union of ``count`` random permutation matchings i - perm(i): degree <= 2 * count, an expander (the halo of any patch is the
    whole graph after a few rings)."""
    rng = np.random.default_rng(seed)
    i = np.arange(M)
    return _adj(M, np.concatenate([np.stack([i, rng.permutation(M)], 1) for _ in range(count)]))


def laplacian(A):
    """I - D^-1/2 A D^-1/2 with float32-exact values (float64 storage)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    d = np.asarray(A.sum(axis=1)).ravel()
    s = np.where(d > 0, 1.0 / np.sqrt(np.maximum(d, 1.0)), 0.0)
    L = sp.identity(A.shape[0], format="csr") - sp.diags(s) @ A @ sp.diags(s)
    L = sp.csr_matrix(L)
    L.data = L.data.astype(np.float32).astype(np.float64)
    L.eliminate_zeros()
    L.sort_indices()
    return L


def row_normalised_laplacian(A):
    """I - D^-1 A: NOT symmetric unless the graph is regular (the backward kernels need a symmetric operator)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    d = np.asarray(A.sum(axis=1)).ravel()
    L = sp.csr_matrix(sp.identity(A.shape[0], format="csr") - sp.diags(np.where(d > 0, 1.0 / np.maximum(d, 1.0), 0.0)) @ A)
    L.data = L.data.astype(np.float32).astype(np.float64)
    L.eliminate_zeros()
    return L


FAMILIES = {
    "ring7": lambda: ring(7),
    "ring40": lambda: ring(40),
    "grid17x15": lambda: tri_grid(17, 15),
    "grid17x15_isolated5": lambda: isolate(tri_grid(17, 15), 5),
    "grid33x31": lambda: tri_grid(33, 31),
    "grid33x32": lambda: tri_grid(33, 32),
    "ring300_hops6": lambda: ring(300, range(1, 7)),          # every row exactly 12 entries
    "ring300_hops7": lambda: ring(300, range(1, 8)),          # rows of 14: refused
    "hub_grid": hub_grid,
    "grid10x10+ring37": lambda: disjoint(tri_grid(10, 10), ring(37)),
    "matchings2_1024": lambda: matchings(1024, 2, 3),
    "matchings3_1000": lambda: matchings(1000, 3, 3),         # (seeds 2, 4 and 5 give 64 patches of 15 .. 16 instead of 96)
    "path1": lambda: path(1), "path2": lambda: path(2), "path3": lambda: path(3),
    "ring1": lambda: ring(1), "ring2": lambda: ring(2), "ring3": lambda: ring(3),
}
TINY = ("path1", "path2", "path3", "ring1", "ring2", "ring3")      # fewer vertices than the smallest candidate plan has patches

REFUSED = "refused"
# family -> M, row lengths of L~ (min, max), and per (K, Cin) -- None = any -- the plan: P, (smallest, largest) patch and, where
# the edge depends on it, (smallest, largest) patch + halo.  Computed on the CPU; tests/test_cheb_synth_host.py asserts them.
EXPECT = {
    "ring7": dict(M=7, deg=(2, 2), plans={(None, None): dict(P=4, own=(1, 2)), (6, None): dict(P=4, own=(1, 2), rtot=(7, 7))}),
    "ring40": dict(M=40, deg=(2, 2), plans={(None, None): dict(P=4, own=(10, 10)), (6, None): dict(P=4, own=(10, 10), rtot=(20, 20))}),
    "grid17x15": dict(M=255, deg=(2, 6), plans={(None, None): dict(P=4, own=(63, 64)), (6, None): dict(P=4, own=(63, 64), rtot=(151, 190))}),
    "grid17x15_isolated5": dict(M=255, deg=(0, 6), plans={(None, None): dict(P=4, own=(63, 64))}),
    "grid33x31": dict(M=1023, deg=(2, 6), plans={(None, None): dict(P=4, own=(255, 256)), (8, None): dict(P=4, own=(255, 256), rtot=(500, 620))}),
    "grid33x32": dict(M=1056, deg=(2, 6), plans={(None, None): dict(P=6, own=(176, 176))}),
    "ring300_hops6": dict(M=300, deg=(12, 12), plans={(None, None): dict(P=4, own=(75, 75)), (6, None): dict(P=4, own=(75, 75), rtot=(135, 135))}),
    "ring300_hops7": dict(M=300, deg=(14, 14), plans={(None, None): REFUSED}),
    "hub_grid": dict(M=400, deg=(2, 8), plans={(None, None): dict(P=4, own=(100, 100))}),
    "grid10x10+ring37": dict(M=137, deg=(2, 6), plans={(None, None): dict(P=4, own=(34, 35)), (8, None): dict(P=4, own=(34, 35), rtot=(37, 116))}),
    "matchings2_1024": dict(M=1024, deg=(3, 4), plans={(6, 8): dict(P=4, own=(256, 256), rtot=(1024, 1024), rmax=1024), (6, 16): REFUSED}),
    "matchings3_1000": dict(M=1000, deg=(4, 6), plans={(4, 16): dict(P=96, own=(10, 11), rtot=(688, 840))}),
}
for _f, _m in (("path1", 1), ("path2", 2), ("path3", 3), ("ring1", 1), ("ring2", 2), ("ring3", 3)):
    EXPECT[_f] = dict(M=_m, deg=None, plans={(None, None): REFUSED})


def expected_plan(family, K, Cin):
    plans = EXPECT[family]["plans"]
    for key in ((K, Cin), (K, None), (None, None)):
        if key in plans:
            return plans[key]
    return None                                    # nothing stated for this combination


_GRAPHS = {}


def graph(family):
    """(adjacency, Laplacian) of a family, built once."""
    if family not in _GRAPHS:
        A = FAMILIES[family]()
        _GRAPHS[family] = (A, laplacian(A))
    return _GRAPHS[family]


def rescaled(L):
    from cape_amd.mesh_sampling import rescale_L
    Lt = sp.csr_matrix(rescale_L(sp.csr_matrix(L), lmax=2), dtype=np.float64)
    Lt.eliminate_zeros()
    Lt.sort_indices()
    return Lt


_PLANS = {}


def plan(family, K, Cin):
    """ChebPatchPlan of (family, K, Cin) exactly as ops.DeviceConvOps.patch_plan asks for it, or None when the planner refuses
    (ValueError).  Built once per process: the 96-patch plan and the refusal of the 1024-vertex expander take seconds."""
    key = (family, int(K), int(Cin))
    if key not in _PLANS:
        from cape_amd.graph import ChebPatchPlan
        try:
            _PLANS[key] = ChebPatchPlan(rescaled(graph(family)[1]), K, Cin, reserve_bytes=8 * 4 * int(Cin) * FOUT)
        except ValueError:
            _PLANS[key] = None
    return _PLANS[key]


def plan_facts(p, K):
    own = p.pinfo[:, 3]
    tot = p.pinfo[:, 3 + K - 1]
    return dict(P=int(p.P), own=(int(own.min()), int(own.max())), rtot=(int(tot.min()), int(tot.max())), rmax=int(p.rmax))


# ---- float64 reference ----------------------------------------------------------------------------------------------------------
def reference(L, K, x, W, dy):
    """Dense evaluation through graph.cheb_polys.  x [N, M, Cin], W [Cin*K, Fout] (row c*K + k), dy [N, M, Fout]:
    y = sum_k T_k x W[k::K];  dx = sum_k T_k^T (dy W[k::K]^T);  dW[k::K] = sum_n (T_k x[n])^T dy[n];
    dW_abs = sum of |(T_k x)[n, r, c] dy[n, r, f]| over the terms (n, r) of every dW element (kernel_bars.sum_bar)."""
    from cape_amd.graph import cheb_polys
    x, W, dy = (np.asarray(a, np.float64) for a in (x, W, dy))
    T = [np.asarray(t.todense()) for t in cheb_polys(L, K)]
    y, dx = np.zeros(dy.shape), np.zeros(x.shape)
    dW, dW_abs = np.zeros(W.shape), np.zeros(W.shape)
    for k in range(K):
        Tx = np.einsum("rs,nsc->nrc", T[k], x)
        y += Tx @ W[k::K]
        dx += np.einsum("sr,nsc->nrc", T[k], dy @ W[k::K].T)
        dW[k::K] = np.einsum("nrc,nrf->cf", Tx, dy)
        dW_abs[k::K] = np.einsum("nrc,nrf->cf", np.abs(Tx), np.abs(dy))
    return y, dx, dW, dW_abs


def twin32(L, K, x, W, dy):
    """The float32 restatement the element bar is measured against: oracle.torch_twin.chebyshev5 and its autograd on the CPU."""
    import torch
    from oracle import torch_twin as tt
    tx = torch.tensor(np.asarray(x), dtype=torch.float32, requires_grad=True)
    tW = torch.tensor(np.asarray(W), dtype=torch.float32, requires_grad=True)
    ty = tt.chebyshev5(tx, L, tW, K)
    ty.backward(torch.tensor(np.asarray(dy), dtype=torch.float32))
    return ty.detach().numpy(), tx.grad.numpy(), tW.grad.numpy()


def inputs(seed, N, M, K, Cin, Fout=FOUT, only_order=None):
    """Gaussian x, W, dy with float32-exact values; ``only_order``: every weight of the other orders is zero."""
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    x, W, dy = f(rng.standard_normal((N, M, Cin))), f(0.5 * rng.standard_normal((Cin * K, Fout))), f(rng.standard_normal((N, M, Fout)))
    if only_order is not None:
        keep = np.zeros(Cin * K, bool)
        keep[only_order::K] = True
        W[~keep] = 0.0
    return x, W, dy


# ---- the patch-local algorithm, restated ------------------------------------------------------------------------------------------
def ell_rows_equal_csr(plan_, K):
    """Every ELL row of the plan = its CSR row, real entries first in CSR order, padded with (own local index, 0)."""
    W_ = plan_.ell_col.shape[1]
    for p in range(plan_.P):
        e0, r0, er = int(plan_.pinfo[p, 2]), int(plan_.csr_rowptr_off[p]), int(plan_.pinfo[p, 1])
        nrow = int(plan_.pinfo[p, 3 + max(K - 2, 0)])
        rp = plan_.rowptr[r0:r0 + nrow + 1]
        for i in range(nrow):
            d = int(rp[i + 1] - rp[i])
            if d > W_:
                return False
            c, v = plan_.ell_col[er + i], plan_.ell_val[er + i]
            if not (np.array_equal(c[:d], plan_.lcol[e0 + rp[i]:e0 + rp[i + 1]]) and np.array_equal(v[:d], plan_.val[e0 + rp[i]:e0 + rp[i + 1]])
                    and np.all(c[d:] == i) and np.all(v[d:] == 0.0)):
                return False
    return True


def emulate(plan, x, W, dy, K, Cin, Fout):
    """Per-patch evaluation exactly as the kernel organises it (float64)."""
    M = plan.M
    y = np.zeros((M, Fout))
    dx = np.zeros((M, Cin))
    dW = np.zeros((Cin * K, Fout))
    Wk = [W[k::K] for k in range(K)]                      # W_k [Cin, Fout]: rows c*K + k
    for p in range(plan.P):
        v0, e0 = int(plan.pinfo[p, 0]), int(plan.pinfo[p, 2])
        r0 = int(plan.csr_rowptr_off[p])
        R = [int(v) for v in plan.pinfo[p, 3:3 + K]]
        vid = plan.vid[v0:v0 + R[-1]]
        nrow = R[max(K - 2, 0)]
        rp = plan.rowptr[r0:r0 + nrow + 1]
        A = sp.csr_matrix((plan.val[e0:e0 + rp[-1]].astype(np.float64), plan.lcol[e0:e0 + rp[-1]], rp), shape=(nrow, R[-1]))
        # the ELL rows the kernel reads describe the same matrix (padding = (own row, 0))
        er = int(plan.pinfo[p, 1])
        ec, ev = plan.ell_col[er:er + nrow], plan.ell_val[er:er + nrow]
        E = sp.csr_matrix((ev.ravel().astype(np.float64), (np.repeat(np.arange(nrow), ec.shape[1]), ec.ravel())), shape=(nrow, R[-1]))
        assert abs(E - A).max() == 0.0 and plan.ell_col.shape[1] == 12
        own = R[0]
        # forward (and the recomputation of the backward's part 1)
        prev, other = x[vid].copy(), np.full((R[-1], Cin), np.nan)
        acc = prev[:own] @ Wk[0]
        dW[0::K] += prev[:own].T @ dy[vid[:own]]
        for k in range(1, K):
            Rk = R[K - 1 - k]
            new = (A[:Rk] @ prev) * (1.0 if k == 1 else 2.0) - (other[:Rk] if k > 1 else 0.0)
            other[:Rk] = new                                 # in place over T_{k-2}; rows beyond keep stale data
            prev, other = other, prev
            assert not np.isnan(prev[:Rk]).any()
            acc += prev[:own] @ Wk[k]
            dW[k::K] += prev[:own].T @ dy[vid[:own]]
        y[vid[:own]] = acc
        # adjoint by Clenshaw: b_k = G_k + 2 L b_{k+1} - b_{k+2} on the k-ring
        G = lambda k, Rk: dy[vid[:Rk]] @ Wk[k].T
        if K == 1:
            dx[vid[:own]] = G(0, own)
            continue
        bA, bB = np.full((R[-1], Cin), np.nan), np.full((R[-1], Cin), np.nan)
        bA[:R[K - 1]] = G(K - 1, R[K - 1])
        for k in range(K - 2, 0, -1):
            Rk = R[k]
            bB[:Rk] = G(k, Rk) - (bB[:Rk] if k < K - 2 else 0.0)
            bB[:Rk] += 2.0 * (A[:Rk] @ np.nan_to_num(bA))     # (columns outside the (k+1)-ring are never referenced)
            assert not np.isnan(A[:Rk] @ np.where(np.isnan(bA), np.inf, bA)).any()
            bA, bB = bB, bA
        t = G(0, own) - (bB[:own] if K > 2 else 0.0)
        dx[vid[:own]] = A[:own] @ np.nan_to_num(bA) + t
    return y, dx, dW
