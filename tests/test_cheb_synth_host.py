"""Host side of the synthetic-graph tests of the on-chip Chebyshev recurrence (tests/cheb_synth.py; the device side is
tests/test_gpu_cheb_fused.py): every family gets the plan its edge case needs -- asserted, so that a change of the partitioner
cannot silently move a case off its edge -- the plan is well formed (patches partition the vertices, none is empty, it fits the
kernel's limits, ELL rows = CSR rows), and the patch-local algorithm restated in numpy equals the dense float64 reference."""
import numpy as np
import pytest

import cheb_synth as S

KS = (2, 3, 6, 8)
CASES = [(f, K, 8 if K in (3, 8) else 16) for f in S.FAMILIES if not f.startswith("matchings") and f not in S.TINY for K in KS]
CASES += [("matchings2_1024", K, 8) for K in KS] + [("matchings2_1024", 6, 16)]
CASES += [("matchings3_1000", K, 16) for K in (2, 3, 4)]
CASES += [(f, K, Cin) for f in S.TINY for K, Cin in ((6, 16), (2, 8))]


def test_families_are_what_their_names_say():
    for f, e in S.EXPECT.items():
        A, L = S.graph(f)
        assert A.shape == (e["M"], e["M"]) and abs(A - A.T).max() == 0 and A.diagonal().sum() == 0, f
        Lt = S.rescaled(L)
        deg = np.diff(Lt.indptr)
        assert np.array_equal(deg, np.asarray(A.sum(axis=1)).ravel().astype(int)), f          # zero diagonal, no stored zeros
        assert e["deg"] is None or (int(deg.min()), int(deg.max())) == e["deg"], (f, deg.min(), deg.max())
        assert np.array_equal(Lt.data.astype(np.float32).astype(np.float64), Lt.data) and abs(Lt - Lt.T).max() == 0, f
    from scipy.sparse.csgraph import connected_components
    assert connected_components(S.graph("grid10x10+ring37")[0], directed=False)[0] == 2
    deg = np.diff(S.rescaled(S.graph("hub_grid")[1]).indptr)
    assert deg[0] == 8 and np.sort(deg)[-2] == 6                       # the hub row among rows of 2 .. 6
    assert np.diff(S.rescaled(S.graph("grid17x15_isolated5")[1]).indptr)[5] == 0
    assert abs(S.rescaled(S.graph("ring40")[1]).data + 0.5).max() == 0  # exact -0.5 entries
    Lr = S.row_normalised_laplacian(S.graph("hub_grid")[0])
    assert abs(Lr - Lr.T).max() > 0.01


@pytest.mark.parametrize("family,K,Cin", CASES, ids=lambda v: str(v))
def test_plan_and_patch_local_algorithm(family, K, Cin):
    exp = S.expected_plan(family, K, Cin)
    p = S.plan(family, K, Cin)                       # None = ChebPatchPlan raised its ValueError
    if exp == S.REFUSED:
        assert p is None, (family, K, Cin, S.plan_facts(p, K))
        if S.EXPECT[family]["M"] <= 300:             # (cheap enough to see the exception itself)
            from cape_amd.graph import ChebPatchPlan
            with pytest.raises(ValueError):
                ChebPatchPlan(S.rescaled(S.graph(family)[1]), K, Cin, reserve_bytes=8 * 4 * Cin * S.FOUT)
        return
    assert p is not None, (family, K, Cin)
    facts = S.plan_facts(p, K)
    for key, want in (exp or {}).items():
        assert facts[key] == want, (family, K, Cin, key, facts)
    M = S.EXPECT[family]["M"]
    own = np.concatenate([p.vid[p.pinfo[q, 0]:p.pinfo[q, 0] + p.pinfo[q, 3]] for q in range(p.P)])
    assert np.array_equal(np.sort(own), np.arange(M))                                   # the patches partition the vertices
    assert (p.pinfo[:, 3] >= 1).all() and (np.diff(p.pinfo[:, 3:3 + K], axis=1) >= 0).all()      # none is empty; rings grow
    assert p.own_max <= 256 and p.rmax <= 1024 and p.rmax % 4 == 0 and p.rmax >= facts["rtot"][1]
    assert 2 * p.rmax * (Cin + 4) * 4 + 8 * 4 * Cin * S.FOUT <= 160 * 1024
    assert p.ell_col.shape[1] == 12 and S.ell_rows_equal_csr(p, K)
    assert (p.ell_col >= 0).all() and all((p.ell_col[p.pinfo[q, 1]:p.pinfo[q, 1] + p.pinfo[q, 3 + K - 2]] < p.pinfo[q, 3 + K - 1]).all()
                                          for q in range(p.P))                          # local columns inside patch + halo
    L = S.graph(family)[1]
    x, W, dy = S.inputs(K + Cin, 1, M, K, Cin)
    ref = S.reference(L, K, x, W, dy)
    got = S.emulate(p, x[0], W, dy[0], K, Cin, S.FOUT)
    for name, a, b in zip(("y", "dx", "dW"), got, (ref[0][0], ref[1][0], ref[2])):
        assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (family, K, Cin, name, np.abs(a - b).max())


def test_no_candidate_with_more_patches_than_vertices():
    """ChebPatchPlan used to hand out a 4-patch plan for graphs of 1 .. 3 vertices: patches with R_0 = R_{K-1} = 0, for which the
    data-gradient kernel computes vid[min(.., Rtot - 1)] = vid[-1].  From 4 vertices on every patch of the bisection is non-empty."""
    from cape_amd.graph import ChebPatchPlan, spectral_patches, _adjacency
    for M in (4, 5, 6, 9):
        Lt = S.rescaled(S.laplacian(S.ring(M)))
        p = ChebPatchPlan(Lt, 6, 16, reserve_bytes=8 * 4 * 16 * S.FOUT)
        assert p.P == 4 and (p.pinfo[:, 3] >= 1).all() and p.pinfo[:, 3].sum() == M
    for M, nparts in ((4, 4), (6, 6), (13, 12), (128, 128), (200, 128)):
        owner = spectral_patches(_adjacency(S.rescaled(S.laplacian(S.ring(M)))), nparts)
        assert np.bincount(owner, minlength=nparts).min() >= 1, (M, nparts)
