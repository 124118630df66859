"""No GPU needed: the cases of tests/test_gpu_loss.py (tests/loss_cases.py) are what they are named for, the references
(tests/loss_reference.py) are what they claim, the bars are reachable by float32 arithmetic and the judges reject corrupted results.

* ``definition64`` equals fp64 torch autograd of the definition (oracle.torch_twin.edge_loss_calc plus the point-wise losses of
  test_gpu_loss_mask._pointwise) on cases without vanishing edges, and oracle.cape_oracle.sigmoid_xent for the GAN values.
* ``restate32`` stays inside every judge on every case x regime; its figures are printed.
* Each corruption is applied to ``restate32`` on the case built for it and rejected: a flipped sign in the vertex -> edge table,
  the hub's last edge dropped, ce over E - 1, the l1 slope at 0 set to 1, the unit vector of a zero-length edge set to NaN and to
  (1, 0, 0), a reversed repeat taken to cancel its original, the rows past the first grid-stride trip left out, the edge vector
  formed without ref in the working regime (exact -- and not the reference's op order), and for the GAN kernel the wrong sigmoid
  branch, a gradient on the real rows of ga, swapped divisors and log1p(e) taken as e.
* graph.vertex_edge_table on ``odd_small``; the argument checks of both C entries, none of which launches."""
import ctypes

import numpy as np
import pytest
import torch

import kernel_bars
import loss_cases as LC
import loss_reference as LR

F32, F64 = np.float32, np.float64


# ---- the tables ------------------------------------------------------------------------------------------------------------

def test_the_cases_are_what_they_are_named_for():
    names = [c["name"] for c in LC.RECON_EDGE_CASES]
    assert names == ["one_edge", "odd_small", "block_tail", "multi_block", "second_trip", "smpl_n2"] and all(c["why"] for c in LC.RECON_EDGE_CASES)
    for c in LC.RECON_EDGE_CASES:
        edges, _ = LC.graph_of(c["name"])
        assert edges.dtype == np.int32 and edges.shape == (c["E"], 2) and edges.min() >= 0 and edges.max() < c["V"]
        assert set(c["regimes"]) <= set(LC.REGIMES)
    c = LC.by_name("block_tail")
    assert c["N"] * c["V"] == LR.LB + 1 and c["N"] * c["E"] == 2 * LR.LB + 1
    c = LC.by_name("multi_block")
    assert c["V"] % LR.LB and c["E"] % LR.LB and c["N"] * c["V"] > 4 * LR.LB
    c = LC.by_name("second_trip")
    assert LC.STRIDE == 262144 and c["N"] * c["V"] == 262150 and c["N"] * c["E"] == 262200 and c["regimes"] == ("generic", "zeros")
    assert LC.inputs("second_trip", "generic")["pred"].nbytes < 3.1 * 2 ** 20
    assert LC.by_name("smpl_n2")["regimes"] == ("working", "converged")
    # odd_small: the hub, the isolated vertices, the self-loops, the repeats and the reversed one
    edges, _ = LC.graph_of("odd_small")
    deg = np.bincount(edges.reshape(-1), minlength=37)
    assert deg[0] >= 33 and not deg[34:].any() and (deg[:34] > 0).all()
    assert (edges[:, 0] == edges[:, 1]).sum() == 2
    proper = [tuple(e) for e in edges.tolist() if e[0] != e[1]]
    assert len(proper) - len(set(proper)) >= 2 and any((b, a) in set(proper) for a, b in proper)
    for name in ("one_edge", "block_tail", "multi_block", "second_trip"):
        e, _ = LC.graph_of(name)
        assert (e[:, 0] != e[:, 1]).all(), name


def test_the_regimes_are_what_they_claim():
    for name, regime in LC.CASE_REGIMES:
        d = LC.inputs(name, regime)
        c = LC.by_name(name)
        assert all(d[k].dtype == F32 for k in ("pred", "gt", "ref")) and d["pred"].shape == (c["N"], c["V"], 3), (name, regime)
        res = np.abs(d["pred"].astype(F64) - d["gt"]).max()
        if regime == "working":
            assert 1e-4 < res < 1e-2 and np.abs(d["pred"]).max() < 0.1 and np.abs(d["ref"]).max() > 0.3
        elif regime == "converged":
            assert 1e-6 < res < 1e-4 and np.abs(d["ref"]).max() > 0.3
        elif regime == "fit":
            assert not d["ref"].any() and res < 1e-3 and (c["V"] < 10 or np.abs(d["pred"]).max() > 0.3)
    for name in ("odd_small", "multi_block", "second_trip"):
        d = LC.inputs(name, "zeros")
        c = LC.by_name(name)
        diff = d["pred"] - d["gt"]
        _, dv = LR._differences(d["pred"], d["gt"], d["ref"], d["edges"], F64, True)
        vanishing = (np.sqrt((dv * dv).sum(-1)) == 0)
        loops = (d["edges"][:, 0] == d["edges"][:, 1])
        assert (vanishing[0] & ~loops).sum() >= 3                                   # zero-length edges that are no self-loops
        assert vanishing[LC.zero_sample(c["N"])].all() and not diff[LC.zero_sample(c["N"])].any()
        assert (diff[0] == F32(0.1)).sum() >= 3 and (diff[0] == -F32(0.1)).sum() >= 3 and (diff[0] == 0).sum() >= 6
    w = LC.weights_of("odd_small", "random")
    assert w.dtype == F32 and (w == 0).sum() > 10 and (w > 0).sum() > 50 and LC.weights_of("odd_small", "ones").all()
    for smooth in LC.GAN_SMOOTH:
        for case in LC.GAN_CASES:
            fake, real = LC.gan_inputs(case, smooth, "extremes")
            if fake.size >= 10:
                both = np.concatenate([fake.reshape(-1), real.reshape(-1)])
                for v in (88.0, -88.0, 104.0, -104.0, 1e4, -1e4):
                    assert (both == F32(v)).any(), (case, v)
                assert ((both == 0) & np.signbit(both)).any() and ((both == 0) & ~np.signbit(both)).any()
    x = LC.gan_extremes(0.1)[-2:]
    sig = 1.0 / (1.0 + np.exp(-x.astype(F64)))
    assert abs(sig[0] - float(F32(1) - F32(0.1))) < 1e-7 and abs(sig[1] - float(F32(0.1))) < 1e-7
    assert [LC.GAN_CASES[i] for i in range(5)] == [(1, 1, 1), (2, 5, 37), (3, 3, 431), (1, 2, 1025), (4, 4, 300)]
    assert np.exp(F32(-88.0)) < np.finfo(F32).tiny and np.exp(F32(-104.0)) == 0            # below the normal range; underflow


# ---- the references --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["block_tail", "multi_block"])
def test_definition64_is_autograd_of_the_definition(name):
    from oracle import torch_twin as tt
    import test_gpu_loss_mask as M
    d = LC.inputs(name, "generic")
    for which, kind in ((None, "l1"), ("random", "l1"), ("random", "huber"), ("random", "l2"), ("ones", "huber")):
        w = None if which is None else LC.weights_of(name, which)
        tp = torch.tensor(d["pred"].astype(F64), requires_grad=True)
        tg, tr = torch.tensor(d["gt"].astype(F64)), torch.tensor(d["ref"].astype(F64))
        w64 = np.ones((LC.by_name(name)["V"], 3)) if w is None else w.astype(F64)
        recon = M._weighted_recon(tp, tg, w64, kind)
        edge = tt.edge_loss_calc(tp + tr, tg + tr, d["edges"])
        wr, we = float(F32(LC.W_RECON)), float(F32(LC.W_EDGE))
        (wr * recon + we * edge).backward()
        got = LR.definition64(d["pred"], d["gt"], d["ref"], d["edges"], LC.W_RECON, LC.W_EDGE, w, kind, delta=0.1)
        assert abs(got.recon - recon.item()) <= 1e-13 * abs(recon.item()) and abs(got.edge - edge.item()) <= 1e-13 * abs(edge.item())
        assert LC.vertex_err(got.dpred, tp.grad.numpy()) < 1e-12, (name, which, kind)
        assert abs(got.recon_terms.sum() - got.recon) < 1e-12 and abs(got.edge_terms.sum() - got.edge) < 1e-12
        assert got.recon_abs >= got.recon - 1e-15 and got.edge_abs >= got.edge - 1e-15
    # the device's huber threshold is float32(0.1): a slope that differs from the definition's by 1.5e-9
    a = LR.definition64(d["pred"], d["gt"], d["ref"], d["edges"], LC.W_RECON, LC.W_EDGE, w, "huber")
    b = LR.definition64(d["pred"], d["gt"], d["ref"], d["edges"], LC.W_RECON, LC.W_EDGE, w, "huber", delta=0.1)
    assert 0 < LC.vertex_err(a.dpred, b.dpred) < 1e-7


def test_the_two_float64_references_part_as_the_residual_shrinks():
    """generic: one reference; working / converged: definition64 is no reference of a float32 evaluation any more"""
    errs = {}
    for regime in ("generic", "working", "converged"):
        d = LC.inputs("multi_block", regime)
        args = (d["pred"], d["gt"], d["ref"], d["edges"], LC.W_RECON, LC.W_EDGE)
        r, f, dd = LR.rounded64(*args), LR.restate32(*args), LR.definition64(*args)
        errs[regime] = (LC.vertex_err(dd.dpred, r.dpred), LC.vertex_err(f.dpred, r.dpred))
        print("multi_block / %s: definition64 against rounded64 %.2e, restate32 against rounded64 %.2e" % ((regime,) + errs[regime]))
    assert errs["generic"][0] < 2e-6 and errs["working"][0] > 2e-5 and errs["converged"][0] > 1e-3
    assert all(v[1] < 1e-6 for v in errs.values())


def test_gan_reference_is_sigmoid_cross_entropy():
    from oracle import cape_oracle as co
    for case in LC.GAN_CASES:
        for smooth in LC.GAN_SMOOTH:
            fake, real = LC.gan_inputs(case, smooth, "generic")
            r = LR.gan_bce(fake, real, smooth, LC.GAN_SCALE)
            tr, tf = LR.gan_targets(smooth, F64)
            g = co.sigmoid_xent(fake.astype(F64), tr).mean()
            d = co.sigmoid_xent(real.astype(F64), tr).mean() + co.sigmoid_xent(fake.astype(F64), tf).mean()
            assert abs(r.gan_g - g) <= 1e-13 * abs(g) and abs(r.gan_d - d) <= 1e-13 * abs(d)
            assert abs(r.scaled_g - float(F32(LC.GAN_SCALE)) * g) <= 1e-13 * abs(g)
            tx = torch.tensor(fake.astype(F64), requires_grad=True)
            ty = torch.tensor(real.astype(F64), requires_grad=True)
            bce = torch.nn.functional.binary_cross_entropy_with_logits
            lg = bce(tx, torch.full_like(tx, tr))
            ld = bce(ty, torch.full_like(ty, tr)) + bce(tx, torch.full_like(tx, tf))
            sc = float(F32(LC.GAN_SCALE))
            gg = torch.autograd.grad(sc * lg, [tx], retain_graph=True)[0].numpy()
            gd = torch.autograd.grad(sc * ld, [tx, ty])
            Nf = case[0]
            assert np.abs(r.ga[:Nf] - gg).max() < 1e-15 and not r.ga[Nf:].any()
            assert np.abs(r.gb[:Nf] - gd[0].numpy()).max() < 1e-15 and np.abs(r.gb[Nf:] - gd[1].numpy()).max() < 1e-15
    assert LR.gan_targets(0.1, F64) == (float(F32(1) - F32(0.1)), float(F32(0.1)))


# ---- restate32 inside every judge ------------------------------------------------------------------------------------------

VARIANTS = [(None, "l1"), ("random", "l1"), ("random", "huber"), ("random", "l2"), ("ones", "l1"), ("ones", "huber"), ("ones", "l2")]


def _got(f32, terms=False):
    got = dict(recon=f32.recon, edge=f32.edge, dpred=f32.dpred)
    wr, we = F32(LC.W_RECON), F32(LC.W_EDGE)
    tot = wr * (got["recon"]) + we * (got["edge"])
    if terms:
        tot = (tot + F32(LC.W_A) * F32(LC.TERM_A)) + F32(LC.TERM_B)
    got["total"] = F32(tot)
    return got


@pytest.mark.parametrize("name,regime", LC.CASE_REGIMES, ids=["%s-%s" % cr for cr in LC.CASE_REGIMES])
def test_restate32_stays_inside_every_judge(name, regime):
    d = LC.inputs(name, regime)
    for which, kind in VARIANTS:
        tag = "restate32[%s,%s,%s,%s]" % (name, regime, which, kind)
        r64, f32, d64 = LC.references(name, regime, kind, which)
        got = _got(f32, terms=True)
        LC.judge_sums(tag, got, r64, f32)
        LC.judge_total(tag, got, term_a=F32(LC.TERM_A), w_a=LC.W_A, term_b=F32(LC.TERM_B))
        LC.judge_dpred(tag, regime, got["dpred"], r64, f32, d64)
        w = None if which is None else LC.weights_of(name, which)
        LC.judge_exact(tag, name, regime, got["dpred"], LR.recon_slope32(d["pred"], d["gt"], LC.W_RECON, w, kind))
        print("%s: dpred against rounded64 %.2e per element, %.2e per vertex" % (tag, kernel_bars.mat_err(f32.dpred, r64.dpred),
                                                                                  LC.vertex_err(f32.dpred, r64.dpred)))
        # w_edge = 0: the whole gradient is the float32 slope expression
        f0 = LR.restate32(d["pred"], d["gt"], d["ref"], d["edges"], LC.W_RECON, 0.0, w, kind)
        assert np.array_equal(f0.dpred, LR.recon_slope32(d["pred"], d["gt"], LC.W_RECON, w, kind)), tag


@pytest.mark.parametrize("case", LC.GAN_CASES, ids=LC.gan_id)
def test_gan_restatement_stays_inside_the_judge(case):
    for smooth in LC.GAN_SMOOTH:
        for data in LC.GAN_DATA:
            fake, real = LC.gan_inputs(case, smooth, data)
            r64, f32 = LR.gan_bce(fake, real, smooth, LC.GAN_SCALE), LR.gan_bce(fake, real, smooth, LC.GAN_SCALE, F32)
            LC.judge_gan("restate32[%s,%g,%s]" % (LC.gan_id(case), smooth, data), _gan_got(f32, case[0]), r64, f32)
            assert np.isfinite(f32.ga).all() and np.isfinite(f32.gb).all()


def _gan_got(f32, nf):
    return dict(gan_g=f32.gan_g, gan_d=f32.gan_d, scaled_g=f32.scaled_g, scaled_d=f32.scaled_d, ga=f32.ga, gb=f32.gb, nf=nf)


def test_all_ones_weights_are_the_unweighted_entry_where_the_scales_agree():
    """with w_recon a power of two, w_recon / (3 N V) and w_recon * (1 / (N sum w)) are one float32 value, and so is every
    operation after it: the fact tests/test_gpu_loss.py holds the device to, bit for bit"""
    for name in ("odd_small", "second_trip"):
        c = LC.by_name(name)
        ones = LC.weights_of(name, "ones")
        a, b = LR.recon_scale32(c["N"], c["V"], 2.0), LR.recon_scale32(c["N"], c["V"], 2.0, ones)
        assert a == b and a[0].dtype == F32
    d = LC.inputs("odd_small", "generic")
    args = (d["pred"], d["gt"], d["ref"], d["edges"], 2.0, LC.W_EDGE)
    u, m = LR.restate32(*args), LR.restate32(*args, LC.weights_of("odd_small", "ones"), "l1")
    assert kernel_bars.same_bits(u.dpred, m.dpred) and u.recon == m.recon and u.edge == m.edge


# ---- the judges reject -----------------------------------------------------------------------------------------------------

def _judge_all(tag, name, regime, f32bad, kind="l1", which=None, sums=True):
    r64, f32, d64 = LC.references(name, regime, kind, which)
    got = _got(f32bad)
    if sums:
        LC.judge_sums(tag, got, r64)
    LC.judge_dpred(tag, regime, got["dpred"], r64, f32, d64)
    d = LC.inputs(name, regime)
    w = None if which is None else LC.weights_of(name, which)
    LC.judge_exact(tag, name, regime, got["dpred"], LR.recon_slope32(d["pred"], d["gt"], LC.W_RECON, w, kind))


def _mutant(name, regime, mut, kind="l1", which=None):
    d = LC.inputs(name, regime)
    w = None if which is None else LC.weights_of(name, which)
    return LR.restate32(d["pred"], d["gt"], d["ref"], d["edges"], LC.W_RECON, LC.W_EDGE, w, kind, mut=mut)


def _rejected(*a, **kw):
    with pytest.raises(AssertionError):
        _judge_all(*a, **kw)


def test_the_judges_reject_each_corruption_of_the_recon_edge_kernels():
    from cape_amd.graph import vertex_edge_table
    _judge_all("clean", "odd_small", "generic", _mutant("odd_small", "generic", {}))            # nothing is rejected that is right
    edges, _ = LC.graph_of("odd_small")
    vptr, vidx = vertex_edge_table(edges, 37)
    # one entry of the vertex -> edge table with its sign bit flipped (a vertex of degree 1 or 2 would do as well as the hub)
    proper = np.nonzero((edges[vidx >> 1, 0] != edges[vidx >> 1, 1]) & (np.arange(len(vidx)) >= vptr[1]))[0]
    for at in (int(proper[0]), int(proper[-1]), int(vptr[1]) - 1):              # (under two other vertices, and under the hub)
        bad = vidx.copy()
        bad[at] ^= 1
        _rejected("sign", "odd_small", "generic", _mutant("odd_small", "generic", dict(table=(vptr, bad))), sums=False)
    # the last incident edge of the hub dropped
    ptr2 = vptr.copy()
    ptr2[1:] -= 1
    _rejected("hub", "odd_small", "generic", _mutant("odd_small", "generic", dict(table=(ptr2, np.delete(vidx, int(vptr[1]) - 1)))), sums=False)
    # ce = w_edge / (N (E - 1))
    for name in ("odd_small", "multi_block"):
        _rejected("ce", name, "generic", _mutant(name, "generic", dict(ce_edges=LC.by_name(name)["E"] - 1)), sums=False)
    # the l1 slope at d == 0 set to 1
    for which in (None, "ones"):
        _rejected("sign0", "odd_small", "zeros", _mutant("odd_small", "zeros", dict(sign0=1.0), which=which), which=which, sums=False)
    # the unit vector of a zero-length edge: NaN, (1, 0, 0)
    for unit in ((np.nan,) * 3, (1.0, 0.0, 0.0)):
        for name in ("odd_small", "multi_block"):
            _rejected("unit0", name, "zeros", _mutant(name, "zeros", dict(zero_unit=unit)), sums=False)
    # ... on a self-loop alone (generic data: the only vanishing edges are the two self-loops, whose two entries cancel under
    # (1, 0, 0) -- NaN does not)
    _rejected("unit0", "odd_small", "generic", _mutant("odd_small", "generic", dict(zero_unit=(np.nan,) * 3)), sums=False)
    # a reversed repeat taken to cancel its original: both entries of the pair dropped from both vertices.  (It does not cancel:
    # (b, a) after (a, b) has the negated vector AND the swapped signs, so the pair counts twice, as the definition has it.)
    pairs = {}
    for e, (a, b) in enumerate(edges.tolist()):
        pairs.setdefault((min(a, b), max(a, b)), []).append((e, a, b))
    rev = next(v for v in pairs.values() if len(v) == 2 and v[0][1] != v[0][2] and v[0][1] == v[1][2])
    drop = np.isin(vidx >> 1, [rev[0][0], rev[1][0]])
    owner = np.repeat(np.arange(37), np.diff(vptr))[~drop]
    ptr3 = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=37))]).astype(np.int32)
    _rejected("reversed", "odd_small", "generic", _mutant("odd_small", "generic", dict(table=(ptr3, vidx[~drop]))), sums=False)
    # the rows past the first trip of either grid-stride loop left at zero: each sum and the gradient, one judge at a time
    r64, f32, d64 = LC.references("second_trip", "generic")
    bad = _got(_mutant("second_trip", "generic", dict(rows_limit=LC.STRIDE)))
    for k in ("recon", "edge"):
        with pytest.raises(AssertionError, match="/ %s:" % k):
            LC.judge_sums("trip", dict(_got(f32), **{k: bad[k]}), r64)
    with pytest.raises(AssertionError):
        LC.judge_dpred("trip", "generic", bad["dpred"], r64, f32, d64)
    LC.judge_sums("trip", _got(f32), r64)
    # total: one term left out, the weights swapped
    got = _got(f32, terms=True)
    LC.judge_total("total", got, term_a=F32(LC.TERM_A), w_a=LC.W_A, term_b=F32(LC.TERM_B))
    for wrong in (F32(LC.W_RECON) * got["recon"] + F32(LC.W_EDGE) * got["edge"] + F32(LC.W_A) * F32(LC.TERM_A),
                  F32(LC.W_EDGE) * got["recon"] + F32(LC.W_RECON) * got["edge"] + F32(LC.W_A) * F32(LC.TERM_A) + F32(LC.TERM_B),
                  got["total"] + F32(2.0 ** -20) * F32(LR.total64(got["recon"], got["edge"], LC.W_RECON, LC.W_EDGE, LC.TERM_A, LC.W_A, LC.TERM_B)[1])):
        with pytest.raises(AssertionError):
            LC.judge_total("total", dict(got, total=F32(wrong)), term_a=F32(LC.TERM_A), w_a=LC.W_A, term_b=F32(LC.TERM_B))


@pytest.mark.parametrize("name", ["multi_block", "smpl_n2"])
def test_the_working_regime_has_power(name):
    """the edge vector formed without ref is exact -- and is not what the reference's op order gives in float32; it must fail
    against rounded64 on the element bar, or the regime could not tell a fused kernel that reorders the differences"""
    r64, f32, _ = LC.references(name, "working")
    bad = _mutant(name, "working", dict(no_ref=True))
    with pytest.raises(AssertionError):
        kernel_bars.element_bar("no_ref", "dpred (element)", bad.dpred, f32.dpred, r64.dpred)
    d = LC.inputs(name, "working")
    dd = LR.definition64(d["pred"], d["gt"], d["ref"], d["edges"], LC.W_RECON, LC.W_EDGE)
    assert LC.vertex_err(bad.dpred, dd.dpred) < LC.vertex_err(f32.dpred, dd.dpred)             # (closer to the definition, all the same)


def test_the_judge_rejects_each_corruption_of_the_gan_kernel():
    def run(case, smooth, data, mut):
        fake, real = LC.gan_inputs(case, smooth, data)
        r64, f32 = LR.gan_bce(fake, real, smooth, LC.GAN_SCALE), LR.gan_bce(fake, real, smooth, LC.GAN_SCALE, F32)
        LC.judge_gan("gan", _gan_got(LR.gan_bce(fake, real, smooth, LC.GAN_SCALE, F32, mut=mut), case[0]), r64, f32)

    run((2, 5, 37), 0.1, "extremes", {})
    for case, smooth, data, mut in (((3, 3, 431), 0.1, "generic", dict(neg_branch_pos=True)),
                                    ((2, 5, 37), 0.0, "extremes", dict(neg_branch_pos=True)),
                                    ((2, 5, 37), 0.1, "generic", dict(ga_real_nonzero=True)),
                                    ((2, 5, 37), 0.1, "generic", dict(swap_div=True)),
                                    # (at +-88 itself log1p(e) IS e in float32: the corruption is the whole tensor's, on the data
                                    # that holds those logits)
                                    ((2, 5, 37), 0.1, "extremes", dict(log1p_as_e=True)),
                                    ((1, 2, 1025), 0.0, "extremes", dict(log1p_as_e=True))):
        with pytest.raises(AssertionError):
            run(case, smooth, data, mut)


# ---- the vertex -> edge table ----------------------------------------------------------------------------------------------

def test_vertex_edge_table_on_the_odd_graph():
    from cape_amd.graph import vertex_edge_table
    edges, _ = LC.graph_of("odd_small")
    V, E = 37, 90
    vptr, vidx = vertex_edge_table(edges, V)
    assert vptr.dtype == vidx.dtype == np.int32 and vptr.shape == (V + 1,) and vidx.shape == (2 * E,) and vptr[0] == 0 and vptr[-1] == 2 * E
    assert sorted(vidx.tolist()) == list(range(2 * E))                           # every edge once as 2e and once as 2e + 1
    for v in range(V):
        codes = vidx[vptr[v]:vptr[v + 1]]
        for code in codes:
            assert edges[code >> 1, code & 1] == v
        # the stable sort's order: the first endpoints by edge, then the second endpoints by edge
        first, second = codes[(codes & 1) == 0], codes[(codes & 1) == 1]
        assert list(codes) == sorted(first) + sorted(second), v
    for e in np.nonzero(edges[:, 0] == edges[:, 1])[0]:                           # a self-loop: both codes under the one vertex
        v = edges[e, 0]
        assert {2 * e, 2 * e + 1} <= set(vidx[vptr[v]:vptr[v + 1]].tolist())
    assert (np.diff(vptr)[34:] == 0).all() and vptr[1] - vptr[0] >= 33


# ---- argument checks: nothing here launches ----------------------------------------------------------------------------------

def test_recon_edge_entry_rejects_bad_arguments_before_launching():
    from cape_amd._lib import lib
    P = ctypes.c_void_p
    N, M, E = 3, 37, 90
    need = int(lib.cape_recon_edge_workspace_bytes(N, M, E))
    assert need == (N * E * 3 + 2048) * 4
    assert lib.cape_recon_edge_workspace_bytes(0, M, E) == -1 and lib.cape_recon_edge_workspace_bytes(N, 0, E) == -1
    assert lib.cape_recon_edge_workspace_bytes(N, M, 0) == -1

    def call(**kw):
        a = dict(pred=P(0x100000), ldp=4, gt=P(0x200000), ref=P(0x300000), edges=P(0x400000), vptr=P(0x500000), vidx=P(0x600000),
                 N=N, M=M, E=E, out=P(0x800000), total=P(0x810000), dpred=P(0x900000), ldd=4, ws=P(0xa00000), need=need)
        a.update(kw)
        return lib.cape_recon_edge_loss_fwd_bwd(a["pred"], a["ldp"], a["gt"], a["ref"], a["edges"], a["vptr"], a["vidx"], a["N"], a["M"],
                                                a["E"], 1.0, 1.0, a["out"], a["total"], None, 0.0, None, a["dpred"], a["ldd"], a["ws"],
                                                a["need"], None)

    for k in ("pred", "gt", "ref", "edges", "out", "ws"):
        assert call(**{k: None}) == -1, k
    for k in ("N", "M", "E"):
        assert call(**{k: 0}) == -1 and call(**{k: -1}) == -1, k
    assert call(ldp=2) == -1
    assert call(ldd=2) == -1 and call(vptr=None) == -1 and call(vidx=None) == -1         # a gradient needs ldd >= 3 and the table
    assert call(need=need - 4) == -4 and call(need=0) == -4                               # CAPE_EWORKSPACE
    assert call(need=need - 4, dpred=None, vptr=None, vidx=None) == -4                    # (checked without a gradient too)


def test_gan_entry_rejects_bad_arguments_before_launching():
    from cape_amd._lib import lib
    P = ctypes.c_void_p
    names = ("fake", "real", "out", "sg", "sd", "ga", "gb")

    def call(**kw):
        a = dict(fake=P(0x100000), fss=431, ldf=1, real=P(0x200000), rss=431, ldr=1, Nf=3, Nr=3, M=431, out=P(0x300000),
                 sg=P(0x400000), sd=P(0x500000), ga=P(0x600000), gb=P(0x700000))
        a.update(kw)
        return lib.cape_gan_bce_fwd_bwd(a["fake"], a["fss"], a["ldf"], a["real"], a["rss"], a["ldr"], a["Nf"], a["Nr"], a["M"], 0.1, 1.0,
                                        a["out"], a["sg"], a["sd"], a["ga"], a["gb"], None)

    for k in names:
        assert call(**{k: None}) == -1, k
    for k in ("Nf", "Nr", "M", "ldf", "ldr"):
        assert call(**{k: 0}) == -1 and call(**{k: -3}) == -1, k
    assert call(Nf=2 ** 15, Nr=2 ** 15, M=2 ** 15) == -1                                  # (Nf + Nr) M = 2^31
    assert call(Nf=1, Nr=1, M=2 ** 30) == -1
