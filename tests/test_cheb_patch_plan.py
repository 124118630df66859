"""Host logic of the on-chip Chebyshev recurrence (cape_amd.graph.ChebPatchPlan, consumed by csrc/cheb_fused.hip): the
patches partition the vertices, the halo rings are what the K-step recurrence needs, and the patch-local algorithm the
kernel runs -- forward recurrence on shrinking rings, contraction on the patch; Clenshaw for the adjoint, weight gradient
from the recomputed recurrence -- restated here in numpy per patch, equals the dense evaluation of reference
lib/models.py:69-103 and its gradients."""
import numpy as np
import scipy.sparse as sp

from cheb_synth import emulate as _emulate      # shared with tests/test_cheb_synth_host.py


def test_patch_plan_and_patch_local_algorithm(mesh_ops):
    from cape_amd.graph import ChebPatchPlan, cheb_polys
    from cape_amd.mesh_sampling import rescale_L
    rng = np.random.default_rng(0)
    for level, K, Cin, Fout in ((6, 6, 16, 32), (4, 4, 8, 32), (6, 2, 16, 32), (6, 3, 24, 64)):
        L = mesh_ops["L"][level]
        M = L.shape[0]
        Lt = sp.csr_matrix(rescale_L(sp.csr_matrix(L), lmax=2), dtype=np.float64)
        plan = ChebPatchPlan(Lt, K, Cin, reserve_bytes=8 * 4 * Cin * Fout)
        own = np.concatenate([plan.vid[plan.pinfo[p, 0]:plan.pinfo[p, 0] + plan.pinfo[p, 3]] for p in range(plan.P)])
        assert np.array_equal(np.sort(own), np.arange(M)) and plan.own_max <= 256
        assert 2 * plan.rmax * (Cin + 4) * 4 + 8 * 4 * Cin * Fout <= 160 * 1024
        x = rng.standard_normal((M, Cin))
        W = rng.standard_normal((Cin * K, Fout))
        dy = rng.standard_normal((M, Fout))
        T = cheb_polys(L, K)
        ref_y = sum((T[k] @ x) @ W[k::K] for k in range(K))
        ref_dx = sum(T[k].T @ (dy @ W[k::K].T) for k in range(K))
        ref_dW = np.zeros_like(W)
        for k in range(K):
            ref_dW[k::K] = (T[k] @ x).T @ dy
        y, dx, dW = _emulate(plan, x, W, dy, K, Cin, Fout)
        for a, b in ((y, ref_y), (dx, ref_dx), (dW, ref_dW)):
            assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (level, K, np.abs(a - b).max())
    # the plan is a pure function of its inputs (the solver's start vector and the Fiedler sign are fixed)
    a, b = ChebPatchPlan(Lt, 3, 24), ChebPatchPlan(Lt, 3, 24)
    assert np.array_equal(a.vid, b.vid) and np.array_equal(a.pinfo, b.pinfo)
