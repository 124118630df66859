"""CPU checks of tests/sparse_reference.py: the synthetic operators have the degrees and the ELL width their family names, the
float64 restatements are the formulas of include/cape_hip.h (scipy / einsum), and the float32 restatements alone pass the bars
tests/test_gpu_sparse.py holds the device to."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparse_reference as R
from kernel_bars import element_bar, mat_err

SHAPES = [(37, 190), (300, 53), (37, 53), (300, 190)]


def _max_degree(family):
    return {"ell4": 4, "ell8": 8}.get(family, 12)


def _host(S):
    from cape_amd.graph import HostCSR
    return HostCSR(S)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_generator_yields_the_degrees_and_ell_width_of_its_family(family, shape):
    from cape_amd import ops
    rows, cols = shape
    S = R.synth_operator(np.random.default_rng(rows + cols), rows, cols, family)
    deg = R.degrees(S)
    h = _host(S)
    assert h.nnz == S.nnz and np.array_equal(h.colidx, S.indices)            # stored zeros and the entry order survive
    assert S.indices.min() == 0 and S.indices.max() == cols - 1
    for r in range(rows):
        c = S.indices[S.indptr[r]:S.indptr[r + 1]]
        assert np.all(np.diff(c) > 0)
    v = S.data / np.exp2(np.floor(np.log2(np.abs(np.where(S.data == 0, 1.0, S.data)))))
    assert np.array_equal(S.data, R.f32(S.data)) and np.all(np.abs(v) < 2)
    ell = ops.ell_arrays(h)
    assert (0 if ell is None else ell[0].shape[1]) == R.expected_ell_w(family)
    if family == "ell4":
        assert deg[0] == 0 and deg[-1] == 0 and set(deg) == {0, 1, 2, 3, 4} and h.max_row <= 4
    elif family == "ell8":
        assert deg.max() == 8 and {0, 4, 5, 8} <= set(deg)
    else:
        assert {0, 8, 9, 12} <= set(deg) and (deg == 0).sum() >= 3
        assert deg.max() == (40 if family == "csr" else 12)
        if family == "csr":
            assert 13 in set(deg)
    S37 = R.synth_operator(np.random.default_rng(3), 37, 37, family)                  # square and narrower than the long row
    assert R.degrees(S37).max() == (37 if family == "csr" else _max_degree(family))
    if family == "zeros_inside":
        assert (S.data == 0).any() and ell is not None
        groups = ell[1].reshape(rows, -1, 4)
        assert ((groups == 0).any(axis=2) & (groups != 0).any(axis=2)).any()
    if family == "zero_group":
        r = next(r for r in range(rows) if deg[r] >= 9 and np.all(S.data[S.indptr[r] + 4:S.indptr[r] + 8] == 0))
        assert S.data[S.indptr[r] + 8] != 0 and ell is None


@pytest.mark.parametrize("family", ["ell4", "ell8", "ell12", "zeros_inside"])
def test_ell_arrays_pad_with_the_first_column_and_weight_zero(family):
    from cape_amd import ops
    S = R.synth_operator(np.random.default_rng(4), 37, 53, family)
    ec, ev = ops.ell_arrays(_host(S))
    deg = R.degrees(S)
    assert ec.dtype == np.int32 and ev.dtype == np.float32
    for r in range(37):
        a, b = S.indptr[r], S.indptr[r + 1]
        assert np.array_equal(ec[r, :deg[r]], S.indices[a:b]) and np.array_equal(ev[r, :deg[r]], S.data[a:b].astype(np.float32))
        assert np.all(ev[r, deg[r]:] == 0) and np.all(ec[r, deg[r]:] == (S.indices[a] if deg[r] else 0))
    assert (deg == 0).any()


def _inputs(rng, *shape):
    return R.f32(rng.standard_normal(shape) * np.exp2(rng.integers(-3, 3, size=shape[:-1] + (1,))))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_restatements_are_the_header_formulas_and_float32_meets_the_bar(family):
    rng = np.random.default_rng(11)
    N, Mo, Mi, C = 3, 37, 53, 12
    S, S2 = (R.synth_operator(rng, Mo, Mi, f) for f in (family, "ell8"))
    x, x2, xi, z = _inputs(rng, N, Mi, C), _inputs(rng, N, Mi, C), _inputs(rng, N, Mo, C), _inputs(rng, N, Mo, C)
    app = lambda m, v: np.stack([m @ v[n] for n in range(N)])
    close = lambda a, b: mat_err(a, b) < 1e-13
    tag = "host[%s]" % family
    # cape_spmm
    want = 1.3 * app(S, x) - 0.7 * z
    assert close(R.spmm(S, x, np.float64(1.3), z, np.float64(-0.7)), np.float64(np.float32(1.3)) * app(S, x) + np.float64(np.float32(-0.7)) * z)
    element_bar(tag, "spmm", R.spmm(S, x, 1.3, z, -0.7, np.float32), R.spmm(S, x, 1.3, z, -0.7, np.float32), R.spmm(S, x, 1.3, z, -0.7))
    assert mat_err(R.spmm(S, x, 1.3, z, -0.7), want) < 1e-7
    assert np.all(R.spmm(S, x)[:, R.degrees(S) == 0] == 0)
    # cape_spmm_multi
    terms = [(None, xi, 1.0), (S, x, 0.5), (S2, x2, 3.0), (None, z, 1.0)]
    outs = R.spmm_multi(terms, False)
    assert close(outs[1], 0.5 * app(S, x)) and close(outs[2], 3.0 * app(S2, x2)) and np.array_equal(outs[0], xi)
    tot = R.spmm_multi(terms, True)
    assert close(tot, xi + 0.5 * app(S, x) + 3.0 * app(S2, x2) + z)
    element_bar(tag, "spmm_multi sum", R.spmm_multi(terms, True, np.float32), R.spmm_multi(terms, True, np.float32), tot)
    # cape_spmm_multi_actgrad
    ax = _inputs(rng, N, Mo, C)
    ax[:, ::5], ax[:, 1::7] = 0.0, -0.0
    for act, slope in (("leaky", np.float64(np.float32(0.2))), ("relu", 0.0)):
        y, db = R.actgrad(terms, ax, act)
        assert close(y, tot * np.where(ax > 0, 1.0, slope)) and close(db, np.einsum("nrc->c", y))
        assert close(R.block_partials(y, 4).sum(axis=1), y.sum(axis=1))
    # cape_bwd_prep_spmm / cape_spmm_multi_prep
    F = 32
    Sq = R.synth_operator(rng, Mo, Mo, family if family != "csr" else "ell12")
    g = _inputs(rng, N, Mo, F)
    bits = rng.random((N, Mo, F)) < 0.55
    assert np.array_equal(R.unpack_words(R.sign_words(bits), F), bits)
    rs = R.f32(rng.standard_normal((3, Mo)))
    o = R.bwd_prep_spmm(Sq, g, bits, rs, 2, 2)
    dz = np.where(bits, g, 0.0)
    assert np.array_equal(o["dz"], dz) and close(o["t1"], app(Sq, dz))
    assert close(o["dcoef"], np.einsum("jr,nrf->njf", rs[:2], dz)) and close(o["dcoef_g"], np.einsum("r,nrf->nf", rs[2], g))
    element_bar(tag, "t1", R.bwd_prep_spmm(Sq, g, bits, rs, 0, None, np.float32)["t1"], R.bwd_prep_spmm(Sq, g, bits, rs, 0, None, np.float32)["t1"], o["t1"])
    Sc = [R.synth_operator(rng, 17, Mo, "ell4"), R.synth_operator(rng, 17, Mo, "ell12")]
    Ts, sums, _ = R.multi_prep([Sc[0], Sc[1], Sc[0]], g, bits, [1, 1, 0])
    assert close(Ts[0], app(Sc[0], dz)) and close(Ts[1], app(Sc[1], dz)) and close(Ts[2], app(Sc[0], g))
    # the identity the fused form rests on: column sums of S^T-applied rows = row sums weighted by S 1
    assert close(sums[1], np.einsum("r,nrf->nf", np.asarray(Sc[1].sum(axis=0)).ravel(), dz))


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("F", [6, 36, 64, 96])
@pytest.mark.parametrize("shape", [(37, 53), (300, 190)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", ["ell8", "ell12"])
def test_combine_restatement_and_the_share_of_uncertain_signs(family, shape, F, dual):
    c = R.combine_case(family, F, dual, Mo=shape[0], Mi=shape[1])
    N = c["N"]
    app = lambda m, v: np.stack([m @ v[n] for n in range(N)])
    r1 = lambda j: c["rowscale"][j][None, :, None] * c["coef"][:, j][:, None, :]
    y, a1 = R.combine(**c["args"])
    S, Z = c["S"], c["Z"]
    if dual:
        want1 = app(S[0], Z[0]) + app(S[1], Z[1])
        want = np.maximum(want1, 0) + app(S[2], Z[2]) + r1(0) + r1(1)
    else:
        want1 = sum(app(S[k], Z[k]) for k in range(3)) + r1(0) + r1(1)
        v = want1 + c["bias"]
        want = np.where(v > 0, v, np.float64(np.float32(0.2)) * v)
    assert mat_err(a1, want1) < 1e-13 and mat_err(y, want) < 1e-13
    y32, _ = R.combine(prec=np.float32, **c["args"])
    element_bar("host combine[%s,%d,%d]" % (family, F, dual), "y", y32, y32, y)
    if dual:
        unsure = R.uncertain_signs(a1)
        assert unsure.mean() <= 0.005
        assert (a1 == 0).any()                               # empty rows, no rank term on acc1: the sign of an exact zero is asserted
