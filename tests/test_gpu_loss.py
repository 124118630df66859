"""The loss kernels (cape_amd/csrc/loss.hip: edge_fwd_kernel, vert_kernel, masked_vert_kernel<0|1|2>, loss_final_kernel,
gan_bce_kernel) against float64 on small graphs and at their edges: the cases, regimes and judges of tests/loss_cases.py, the
references of tests/loss_reference.py (pinned on the host by tests/test_loss_cases_host.py).

The device is judged against ``rounded64`` -- the kernel's two float32 differences, everything after them in float64 -- in every
regime, the sums by kernel_bars.sum_bar, the gradient by kernel_bars.element_bar against the float32 restatement on the element and
the vertex measure; in the ``generic`` regime also against the definition at 2e-5 per vertex.  Then the facts that hold as values or
bits: vertices without edges, w_edge = 0, a sample at gt = pred, a self-loop, the real rows of the generator's GAN gradient,
all-ones weights, two calls."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import kernel_bars
import loss_cases as LC
import loss_reference as LR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
P = ctypes.c_void_p
# (name, weights, kind, layout of the prediction, gradient through 2 * total)
VARIANTS = [("plain", None, "l1", "dense", False), ("plain_rows4_x2", None, "l1", "rows4", True),
            ("l1_random_rows4", "random", "l1", "rows4", False), ("huber_random_x2", "random", "huber", "dense", True),
            ("l2_random_rows4", "random", "l2", "rows4", False), ("l1_ones", "ones", "l1", "dense", False),
            ("huber_ones_rows4_x2", "ones", "huber", "rows4", True), ("l2_ones", "ones", "l2", "dense", False)]
RUNS = [(n, r, v) for n, r in LC.CASE_REGIMES for v in VARIANTS]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, dev, dt=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dt, device=dev)


@functools.lru_cache(maxsize=2)
def _tables(name, regime, dev):
    """(gt, ref, edges, vptr, vidx) on the device"""
    from cape_amd.graph import vertex_edge_table
    d = LC.inputs(name, regime)
    vptr, vidx = vertex_edge_table(d["edges"], LC.by_name(name)["V"])
    return (_t(d["gt"], dev), _t(d["ref"], dev), _t(d["edges"], dev, torch.int32), _t(vptr, dev, torch.int32), _t(vidx, dev, torch.int32))


def _pred(pred, rows, dev):
    """(leaf, view handed to the loss): dense, or a [:, :, :3] view of 16-byte rows whose fourth lane holds 1e9"""
    if rows == "dense":
        hp = _t(pred, dev).requires_grad_(True)
        return hp, hp
    N, V, _ = pred.shape
    hp = torch.full((N, V, 4), 1e9, dtype=torch.float32, device=dev)
    hp[:, :, :3] = _t(pred, dev)
    hp.requires_grad_(True)
    return hp, hp[:, :, :3]


def _apply(name, regime, dev, which=None, kind="l1", rows="dense", doubled=False, terms=True, w_recon=LC.W_RECON, w_edge=LC.W_EDGE,
           tabs=None):
    """one forward + backward through ops.ReconEdgeLossFn; dict(recon, edge, total, dpred [N, V, 3] fp32, ...)"""
    from cape_amd import ops
    d = LC.inputs(name, regime)
    gt, ref, edges, vptr, vidx = tabs or _tables(name, regime, dev)
    hp, view = _pred(d["pred"], rows, dev)
    ha = torch.tensor(LC.TERM_A, dtype=torch.float32, device=dev, requires_grad=True) if terms else None
    hb = torch.tensor(LC.TERM_B, dtype=torch.float32, device=dev) if terms else None
    extra = ()
    if which is not None:
        w = LC.weights_of(name, which)
        extra = (_t(w, dev), LR.weight_sum(w), kind)
    total, parts = ops.ReconEdgeLossFn.apply(view, gt, ref, edges, vptr, vidx, w_recon, w_edge, ha, LC.W_A if terms else 0.0, hb, *extra)
    ((2.0 * total) if doubled else total).backward()
    g = hp.grad.cpu().numpy()
    mult = 2.0 if doubled else 1.0
    if terms:
        assert abs(ha.grad.item() - mult * LC.W_A) < 1e-7
    if rows == "rows4":
        assert not g[:, :, 3].any()                                 # the padding lane takes no gradient
        g = g[:, :, :3]
    return dict(recon=F32(parts[0].item()), edge=F32(parts[1].item()), total=F32(total.item()),
                dpred=np.ascontiguousarray(g * F32(1.0 / mult)), parts=parts.detach().cpu().numpy(), raw=g)


@pytest.mark.parametrize("name,regime,variant", RUNS, ids=["%s-%s-%s" % (n, r, v[0]) for n, r, v in RUNS])
def test_recon_edge_loss_cases(name, regime, variant, dev):
    _, which, kind, rows, doubled = variant
    tag = "loss[%s,%s,%s]" % (name, regime, variant[0])
    got = _apply(name, regime, dev, which, kind, rows, doubled)
    r64, f32, d64 = LC.references(name, regime, kind, which)
    LC.judge_sums(tag, got, r64, f32)
    LC.judge_total(tag, got, term_a=F32(LC.TERM_A), w_a=LC.W_A, term_b=F32(LC.TERM_B))
    LC.judge_dpred(tag, regime, got["dpred"], r64, f32, d64)
    d = LC.inputs(name, regime)
    w = None if which is None else LC.weights_of(name, which)
    LC.judge_exact(tag, name, regime, got["dpred"], LR.recon_slope32(d["pred"], d["gt"], LC.W_RECON, w, kind))


@pytest.mark.parametrize("name,regime", LC.CASE_REGIMES, ids=["%s-%s" % cr for cr in LC.CASE_REGIMES])
def test_without_the_edge_term_the_gradient_is_the_slope_expression(name, regime, dev):
    """w_edge = 0: every value of the gradient is cr * dl, cr * (w * dl) in float32, for the unweighted entry and all three kinds
    (values, not bits: zeros may differ in sign) -- whatever the unit vectors are, zero-length edges included"""
    d = LC.inputs(name, regime)
    for which, kind in ((None, "l1"), ("random", "l1"), ("random", "huber"), ("random", "l2")):
        got = _apply(name, regime, dev, which, kind, terms=False, w_edge=0.0)
        w = None if which is None else LC.weights_of(name, which)
        assert np.array_equal(got["dpred"], LR.recon_slope32(d["pred"], d["gt"], LC.W_RECON, w, kind)), (name, regime, which, kind)
        assert np.isfinite(got["parts"]).all() and np.isfinite(got["total"])


@pytest.mark.parametrize("name,regime", [("odd_small", "generic"), ("odd_small", "zeros"), ("second_trip", "generic"), ("second_trip", "zeros")])
def test_all_ones_weights_are_the_unweighted_entry_and_two_calls_agree(name, regime, dev):
    """w_recon = 2: w_recon / (3 N V) and w_recon * (1 / (N sum w)) are one float32 value (test_loss_cases_host.py), so an
    all-ones l1 mask gives the unweighted entry's bits in every output; and every entry repeats its own bits"""
    runs = {}
    for which, kind in ((None, "l1"), ("ones", "l1"), ("random", "huber"), ("random", "l2")):
        a = _apply(name, regime, dev, which, kind, w_recon=2.0)
        b = _apply(name, regime, dev, which, kind, w_recon=2.0)
        for k in ("raw", "parts", "total"):
            assert kernel_bars.same_bits(np.asarray(a[k]), np.asarray(b[k])), (name, which, kind, k)
        runs[which, kind] = a
    u, m = runs[None, "l1"], runs["ones", "l1"]
    for k in ("raw", "parts", "total"):
        assert kernel_bars.same_bits(np.asarray(u[k]), np.asarray(m[k])), (name, k)
    # the edge value is the same bits whatever the vertex pass
    assert len({runs[k]["parts"][1].tobytes() for k in runs}) == 1


def test_a_self_loop_contributes_nothing_to_its_vertex(dev):
    """odd_small with one self-loop moved from its vertex to an isolated one, at the same place of the edge list: its two table
    entries add +-ce * 0, so no value of any output moves -- and the vertex that was isolated still carries the slope alone"""
    from cape_amd.graph import vertex_edge_table
    name = "odd_small"
    for regime in ("generic", "zeros"):
        d = LC.inputs(name, regime)
        edges = d["edges"].copy()
        at = int(np.nonzero(edges[:, 0] == edges[:, 1])[0][0])
        edges[at] = 36
        vptr, vidx = vertex_edge_table(edges, 37)
        assert vptr[37] - vptr[36] == 2
        gt, ref = _tables(name, regime, dev)[:2]
        tabs = (gt, ref, _t(edges, dev, torch.int32), _t(vptr, dev, torch.int32), _t(vidx, dev, torch.int32))
        for which, kind in ((None, "l1"), ("random", "huber")):
            a, b = _apply(name, regime, dev, which, kind), _apply(name, regime, dev, which, kind, tabs=tabs)
            assert np.array_equal(a["dpred"], b["dpred"]) and kernel_bars.same_bits(a["parts"], b["parts"]) and a["total"] == b["total"]


# ---- the C entry points ------------------------------------------------------------------------------------------------------

def _c_call(name, regime, dev, pred=None, ldp=3, total=True, term_a=None, term_b=None, dpred="new", ldd=3, which=None, kind="l1"):
    """cape_[masked_]recon_edge_loss_fwd_bwd on raw pointers; (rc, loss_out [2], total or None, dpred buffer or None)"""
    from cape_amd import ops
    from cape_amd._lib import lib
    c = LC.by_name(name)
    N, V, E = c["N"], c["V"], c["E"]
    d = LC.inputs(name, regime)
    gt, ref, edges, vptr, vidx = _tables(name, regime, dev)
    hp = _t(d["pred"], dev) if pred is None else pred
    need = int(lib.cape_recon_edge_workspace_bytes(N, V, E))
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=dev)
    tot = torch.full((), float("nan"), dtype=torch.float32, device=dev) if total else None
    if isinstance(dpred, str):
        dpred = torch.full((N, V, ldd), -7.0, dtype=torch.float32, device=dev)
    ptr = lambda t: None if t is None else P(t.data_ptr())
    head = (pred_ptr(hp), ldp, ptr(gt), ptr(ref), ptr(edges), ptr(vptr) if dpred is not None else None,
            ptr(vidx) if dpred is not None else None, N, V, E)
    tail = (LC.W_RECON, LC.W_EDGE, ptr(out), ptr(tot), ptr(term_a), LC.W_A, ptr(term_b), ptr(dpred), ldd, ptr(ws), need, ops._stream())
    if which is None:
        rc = lib.cape_recon_edge_loss_fwd_bwd(*head, *tail)
    else:
        w = LC.weights_of(name, which)
        wt = _t(w, dev)
        rc = lib.cape_masked_recon_edge_loss_fwd_bwd(*head, ptr(wt), LR.KINDS.index(kind), 1.0 / (N * LR.weight_sum(w)), *tail)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), None if tot is None else tot.cpu().numpy(), None if dpred is None else dpred.cpu().numpy()


def pred_ptr(t):
    """a tensor's first element, or (tensor, element offset)"""
    return P(t[0].data_ptr() + 4 * t[1]) if isinstance(t, tuple) else P(t.data_ptr())


@pytest.mark.parametrize("regime", ["generic", "zeros"])
@pytest.mark.parametrize("name", ["odd_small", "block_tail"])
def test_c_entries_optional_outputs_and_leading_dimensions(name, regime, dev):
    c = LC.by_name(name)
    N, V = c["N"], c["V"]
    d = LC.inputs(name, regime)
    for which, kind in ((None, "l1"), ("random", "huber")):
        kw = dict(which=which, kind=kind)
        r64, f32, d64 = LC.references(name, regime, kind, which)
        ta, tb = torch.tensor(LC.TERM_A, device=dev), torch.tensor(LC.TERM_B, device=dev)
        rc, out, tot, g = _c_call(name, regime, dev, term_a=ta, term_b=tb, **kw)
        assert rc == 0
        tag = "c_entry[%s,%s,%s]" % (name, regime, kind if which else "plain")
        got = dict(recon=out[0], edge=out[1], total=tot, dpred=g)
        LC.judge_sums(tag, got, r64, f32)
        LC.judge_dpred(tag, regime, g, r64, f32, d64)
        # dpred == NULL (and no table): the same loss_out and total bits
        rc, out0, tot0, g0 = _c_call(name, regime, dev, term_a=ta, term_b=tb, dpred=None, **kw)
        assert rc == 0 and g0 is None and kernel_bars.same_bits(out0, out) and kernel_bars.same_bits(tot0, tot)
        # total_out == NULL: the terms are not consulted (NaN in them reaches nothing) and keep their bits
        na, nb = torch.tensor(float("nan"), device=dev), torch.tensor(float("nan"), device=dev)
        rc, out1, tot1, g1 = _c_call(name, regime, dev, total=False, term_a=na, term_b=nb, **kw)
        assert rc == 0 and tot1 is None and kernel_bars.same_bits(out1, out) and kernel_bars.same_bits(g1, g)
        assert torch.isnan(na).item() and torch.isnan(nb).item()
        # the four combinations of term_a / term_b
        for a, b in ((None, None), (ta, None), (None, tb), (ta, tb)):
            rc, out2, tot2, _ = _c_call(name, regime, dev, term_a=a, term_b=b, dpred=None, **kw)
            assert rc == 0 and kernel_bars.same_bits(out2, out)
            LC.judge_total(tag, dict(recon=out2[0], edge=out2[1], total=tot2), term_a=None if a is None else F32(LC.TERM_A), w_a=LC.W_A,
                           term_b=None if b is None else F32(LC.TERM_B))
        # ldp = 4, and 7 as a channel slice starting at channel 1 of a wider poisoned buffer: the bits of ldp = 3
        for ldp, off in ((4, 0), (7, 1)):
            buf = torch.full((N, V, ldp), float("nan"), dtype=torch.float32, device=dev)
            buf[:, :, off:off + 3] = _t(d["pred"], dev)
            rc, out3, tot3, g3 = _c_call(name, regime, dev, pred=(buf, off), ldp=ldp, term_a=ta, term_b=tb, **kw)
            assert rc == 0 and kernel_bars.same_bits(out3, out) and kernel_bars.same_bits(tot3, tot) and kernel_bars.same_bits(g3, g), ldp
        # ldd = 5: lanes 3 and 4 keep their marker, lanes 0..2 are the bits of ldd = 3
        rc, out4, _, g4 = _c_call(name, regime, dev, ldd=5, **kw)
        assert rc == 0 and kernel_bars.same_bits(out4, out) and (g4[:, :, 3:] == -7.0).all()
        assert kernel_bars.same_bits(np.ascontiguousarray(g4[:, :, :3]), g)
        # ldd = 3 inside a longer buffer: nothing behind row N V - 1 is written
        flat = torch.full((N * V * 3 + 64,), -7.0, dtype=torch.float32, device=dev)
        rc, _, _, g5 = _c_call(name, regime, dev, dpred=flat, **kw)
        assert rc == 0 and (g5[N * V * 3:] == -7.0).all() and kernel_bars.same_bits(g5[:N * V * 3].reshape(N, V, 3), g)


# ---- adversarial losses ----------------------------------------------------------------------------------------------------

GAN_RUNS = [(c, s, dt) for c in LC.GAN_CASES for s in LC.GAN_SMOOTH for dt in LC.GAN_DATA]


def _gan_refs(case, smooth, data):
    fake, real = LC.gan_inputs(case, smooth, data)
    return fake, real, LR.gan_bce(fake, real, smooth, LC.GAN_SCALE), LR.gan_bce(fake, real, smooth, LC.GAN_SCALE, F32)


@pytest.mark.parametrize("merged", [True, False], ids=["merged", "split"])
@pytest.mark.parametrize("case,smooth,data", GAN_RUNS, ids=["%s-s%g-%s" % (LC.gan_id(c), s, dt) for c, s, dt in GAN_RUNS])
def test_gan_loss_cases(case, smooth, data, merged, dev):
    from cape_amd import ops
    Nf, Nr, M = case
    fake, real, r64, f32 = _gan_refs(case, smooth, data)
    if merged:
        buf = ops.alloc_act(Nf + Nr, M, 1, dev)                     # ld = 4: the layout the discriminator's last layer writes
        buf.copy_(_t(np.concatenate([fake, real])[:, :, None], dev))
        leaves = [buf.detach().requires_grad_(True)]
        lg, ld, parts = ops.GanLossFn.apply(leaves[0], None, Nf, smooth, LC.GAN_SCALE)
    else:
        leaves = []
        for a in (fake, real):
            buf = ops.alloc_act(a.shape[0], M, 1, dev)
            buf.copy_(_t(a[:, :, None], dev))
            leaves.append(buf.detach().requires_grad_(True))
        lg, ld, parts = ops.GanLossFn.apply(leaves[0], leaves[1], Nf, smooth, LC.GAN_SCALE)
    ga = torch.cat(torch.autograd.grad(lg, leaves, retain_graph=True)).cpu().numpy()[:, :, 0]
    gb = torch.cat(torch.autograd.grad(ld, leaves)).cpu().numpy()[:, :, 0]
    got = dict(gan_g=F32(parts[0].item()), gan_d=F32(parts[1].item()), scaled_g=F32(lg.item()), scaled_d=F32(ld.item()), ga=ga, gb=gb, nf=Nf)
    LC.judge_gan("gan[%s,%g,%s,%s]" % (LC.gan_id(case), smooth, data, "merged" if merged else "split"), got, r64, f32)


def _gan_c_call(fake_t, fss, ldf, real_t, rss, ldr, case, smooth, dev):
    from cape_amd import ops
    from cape_amd._lib import lib
    Nf, Nr, M = case
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=dev)
    sg, sd = (torch.full((), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
    ga, gb = (torch.full(((Nf + Nr) * M + 32,), -7.0, dtype=torch.float32, device=dev) for _ in range(2))
    rc = lib.cape_gan_bce_fwd_bwd(P(fake_t.data_ptr()), fss, ldf, P(real_t.data_ptr()), rss, ldr, Nf, Nr, M, smooth, LC.GAN_SCALE,
                                  P(out.data_ptr()), P(sg.data_ptr()), P(sd.data_ptr()), P(ga.data_ptr()), P(gb.data_ptr()), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    ga, gb, out = ga.cpu().numpy(), gb.cpu().numpy(), out.cpu().numpy()
    assert (ga[(Nf + Nr) * M:] == -7.0).all() and (gb[(Nf + Nr) * M:] == -7.0).all()          # nothing behind the last row
    return dict(gan_g=out[0], gan_d=out[1], scaled_g=F32(sg.item()), scaled_d=F32(sd.item()), ga=ga[:(Nf + Nr) * M].reshape(Nf + Nr, M),
                gb=gb[:(Nf + Nr) * M].reshape(Nf + Nr, M), nf=Nf)


@pytest.mark.parametrize("case", LC.GAN_CASES, ids=LC.gan_id)
def test_gan_c_entry_strides(case, dev):
    """ldf / ldr = 1 and 3 with NaN between the logits, and a real tensor whose sample stride exceeds M * ld (NaN behind every
    sample): the bits of the dense call, under the judge"""
    Nf, Nr, M = case
    smooth = 0.1
    fake, real, r64, f32 = _gan_refs(case, smooth, "extremes")
    base = _gan_c_call(_t(fake, dev), M, 1, _t(real, dev), M, 1, case, smooth, dev)
    LC.judge_gan("gan_c[%s,ld1]" % LC.gan_id(case), base, r64, f32)
    fb = torch.full((Nf, M, 3), float("nan"), dtype=torch.float32, device=dev)
    fb[:, :, 0] = _t(fake, dev)
    rb = torch.full((Nr, M * 3 + 5), float("nan"), dtype=torch.float32, device=dev)            # sample stride 3 M + 5
    rb[:, :M * 3:3] = _t(real, dev)
    wide = _gan_c_call(fb, 3 * M, 3, rb, 3 * M + 5, 3, case, smooth, dev)
    for k in ("ga", "gb"):
        assert kernel_bars.same_bits(np.ascontiguousarray(wide[k]), np.ascontiguousarray(base[k])), k
    for k in ("gan_g", "gan_d", "scaled_g", "scaled_d"):
        assert np.asarray(wide[k], F32).tobytes() == np.asarray(base[k], F32).tobytes(), k
    again = _gan_c_call(_t(fake, dev), M, 1, _t(real, dev), M, 1, case, smooth, dev)            # two calls agree bit for bit
    assert kernel_bars.same_bits(again["ga"], base["ga"]) and kernel_bars.same_bits(again["gb"], base["gb"]) and again["gan_d"] == base["gan_d"]
