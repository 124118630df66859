"""The cases of tests/test_gpu_loss.py: graphs, data regimes, case tables and judges of the loss kernels (cape_amd/csrc/loss.hip:
edge_fwd_kernel, vert_kernel, masked_vert_kernel<0|1|2>, loss_final_kernel, gan_bce_kernel).  TEST INFRASTRUCTURE ONLY; pinned on
the host by tests/test_loss_cases_host.py, which also feeds the judges corrupted results.

A new loss kind, a fused edge / vertex pass or a last-block final needs its row here: ``second_trip`` (both grid-stride loops take
a second trip, 1024 partials per sum) and the ``zeros`` regime (zero-length edges, a whole sample at gt = pred) are the ones a
fusion must keep passing.

The bars are the project's own (kernel_bars.sum_bar, kernel_bars.element_bar = parity_bar.check at factor 4 with the 2e-5
backstop); nothing here introduces a tolerance.  The one derived figure is the scalar identity's 2^-22: ``total`` and the scaled
GAN values are at most four float32 roundings of partial sums no larger than sum |terms|, each at most 2^-24 of it."""
import functools
import zlib

import numpy as np

import kernel_bars
import loss_reference as LR
import parity_bar

F32, F64 = np.float32, np.float64
TOL = kernel_bars.TOL
W_RECON, W_EDGE = 0.7, 1.3
TERM_A, W_A, TERM_B = 3.5, 0.25, -0.75
IDENTITY_REL = 2.0 ** -22
STRIDE = LR.LB * LR.GRID_CAP                     # 262144: rows one trip of either pass covers


def vertex_err(a, ref):
    """tests/test_gpu_ops.py's measure: the largest per-vertex error over the largest per-vertex norm"""
    a = np.asarray(a, dtype=F64).reshape(-1, ref.shape[-1])
    r = np.asarray(ref, dtype=F64).reshape(-1, ref.shape[-1])
    return np.sqrt(((a - r) ** 2).sum(-1)).max() / max(np.sqrt((r * r).sum(-1)).max(), 1e-30)


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


# ---- graphs ----------------------------------------------------------------------------------------------------------------

def edge_graph(V, E, seed, hub=False, isolated=0, self_loops=0, repeats=0):
    """int32 [E, 2]: random pairs a != b; ``hub``: vertex 0 joined to every other non-isolated vertex; ``isolated``: the last k
    vertices appear in no edge; ``self_loops``: k edges (v, v); ``repeats``: k edges listed again, the first of them reversed.
    The list is shuffled, so that no kind of edge sits in a range of its own."""
    rng = np.random.default_rng(seed)
    live = V - isolated
    assert live >= 2
    rows = [(0, v) for v in range(1, live)] if hub else []
    n_rand = E - len(rows) - self_loops - repeats
    assert n_rand >= (1 if repeats else 0) and (repeats == 0 or n_rand + len(rows) >= repeats)
    a = rng.integers(0, live, n_rand)
    b = (a + rng.integers(1, live, n_rand)) % live
    rows += list(zip(a.tolist(), b.tolist()))
    again = [rows[i] for i in rng.choice(len(rows), repeats, replace=False)] if repeats else []
    if again:
        again[0] = again[0][::-1]
    loops = [(int(v), int(v)) for v in rng.integers(1, live, self_loops)]
    edges = np.asarray(rows + again + loops, np.int32).reshape(-1, 2)
    edges = edges[rng.permutation(len(edges))]
    assert edges.shape == (E, 2)
    return np.ascontiguousarray(edges)


SMALL = ("generic", "working", "converged", "fit", "zeros")
RECON_EDGE_CASES = [
    dict(name="one_edge", N=1, V=2, E=1, graph={}, regimes=SMALL, why="one live thread per pass"),
    dict(name="odd_small", N=3, V=37, E=90, graph=dict(hub=True, isolated=3, self_loops=2, repeats=3), regimes=SMALL,
         why="hub of degree >= 33, 3 isolated vertices, 2 self-loops, 3 repeats"),
    dict(name="block_tail", N=1, V=257, E=513, graph={}, regimes=SMALL, why="N V = 256 + 1, N E = 2 * 256 + 1"),
    dict(name="multi_block", N=7, V=431, E=1290, graph={}, regimes=SMALL, why="sample boundaries inside workgroups"),
    dict(name="second_trip", N=5, V=52430, E=52440, graph={}, regimes=("generic", "zeros"),
         why="N V = 262150 and N E = 262200: both loops' second trip, 1024 partials per sum"),
    dict(name="smpl_n2", N=2, V=6890, E=20664, graph="smpl", regimes=("working", "converged"),
         why="the real template and edge list, for the working regime on the real ref"),
]
REGIMES = dict(generic="pred, gt ~ N(0, 1), ref of extent 1", working="pred = 1e-2 N, gt = pred + 1e-3 N, ref of extent 1",
               converged="pred = 1e-2 N, gt = pred + 1e-5 N, ref of extent 1", fit="ref = 0, pred of extent 1, gt = pred + 1e-4 N",
               zeros="generic with zero-length edges, a whole sample at gt = pred, |d| = 0.1f and d = 0 on blocks of coordinates")
CASE_REGIMES = [(c["name"], r) for c in RECON_EDGE_CASES for r in c["regimes"]]


def by_name(name):
    return next(c for c in RECON_EDGE_CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def graph_of(name):
    c = by_name(name)
    if c["graph"] == "smpl":
        from cape_amd.load_data import load_pack
        pack = load_pack()
        edges, ref = np.ascontiguousarray(pack["edges_smpl"], np.int32), np.ascontiguousarray(pack["template_verts"], F32)
        assert edges.shape == (c["E"], 2) and ref.shape == (c["V"], 3)
        return edges, ref
    return edge_graph(c["V"], c["E"], _seed(name, "graph"), **c["graph"]), None


def zero_blocks(V):
    """three vertex ranges at the end of the list (the isolated vertices are among them): d = +0.1f on coordinate 1 of the first,
    -0.1f on coordinate 2 of the second, 0 on coordinate 0 of the third"""
    t = max(1, V // 5)
    return [(max(0, V - 3 * t), max(0, V - 2 * t)), (max(0, V - 2 * t), V - t), (V - t, V)]


def zero_vertices(edges, count=4):
    """both ends of the first ``count`` edges that are no self-loops"""
    proper = edges[edges[:, 0] != edges[:, 1]][:count]
    return np.unique(proper.reshape(-1))


def zero_sample(N):
    """the sample held at gt = pred in the ``zeros`` regime (none when there is only one: the rest of the case keeps its power)"""
    return N - 1 if N > 1 else None


@functools.lru_cache(maxsize=4)
def inputs(name, regime):
    """dict(pred, gt [N, V, 3], ref [V, 3], edges [E, 2]), fp32 / int32, seeded by the case and the regime"""
    c = by_name(name)
    N, V = c["N"], c["V"]
    edges, ref = graph_of(name)
    rng = np.random.default_rng(_seed(name, regime))
    normal = lambda s=1.0: s * rng.standard_normal((N, V, 3))
    if ref is None:
        ref = rng.uniform(-0.5, 0.5, (V, 3)).astype(F32)
    if regime in ("generic", "zeros"):
        pred, gt = normal().astype(F32), normal().astype(F32)
    elif regime in ("working", "converged"):
        pred = normal(1e-2).astype(F32)
        gt = (pred + normal(1e-3 if regime == "working" else 1e-5)).astype(F32)
    else:
        assert regime == "fit", regime
        ref = np.zeros((V, 3), F32)
        pred = rng.uniform(-0.5, 0.5, (N, V, 3)).astype(F32)
        gt = (pred + normal(1e-4)).astype(F32)
    if regime == "zeros":
        tenth = F32(0.1)
        (a0, a1), (b0, b1), (c0, c1) = zero_blocks(V)
        pred[:, a0:a1, 1], gt[:, a0:a1, 1] = tenth, 0.0              # d = +0.1f
        pred[:, b0:b1, 2], gt[:, b0:b1, 2] = 0.0, tenth              # d = -0.1f
        gt[:, c0:c1, 0] = pred[:, c0:c1, 0]                          # d = 0
        z = zero_vertices(edges)
        gt[:, z] = pred[:, z]                                        # zero-length edges
        if zero_sample(N) is not None:
            gt[zero_sample(N)] = pred[zero_sample(N)]
    out = dict(pred=pred, gt=gt, ref=ref, edges=edges)
    for v in out.values():
        v.setflags(write=False)
    return out


def weights_of(name, which):
    """[V, 3] fp32: ``random`` in [0, 2) with exact zeros on three coordinates in ten, or ``ones``"""
    V = by_name(name)["V"]
    if which == "ones":
        return np.ones((V, 3), F32)
    rng = np.random.default_rng(_seed(name, "weights"))
    w = rng.uniform(0.0, 2.0, (V, 3))
    w[rng.random((V, 3)) < 0.3] = 0.0
    if not w.any():
        w[0, 0] = 1.0
    return w.astype(F32)


@functools.lru_cache(maxsize=16)
def references(name, regime, kind="l1", which=None, w_recon=W_RECON, w_edge=W_EDGE):
    """(rounded64, restate32, definition64 or None) of one case; computed once, shared by the tests, never written to"""
    d = inputs(name, regime)
    w = None if which is None else weights_of(name, which)
    args = (d["pred"], d["gt"], d["ref"], d["edges"], w_recon, w_edge, w, kind)
    r64, f32 = LR.rounded64(*args), LR.restate32(*args)
    d64 = LR.definition64(*args) if regime == "generic" else None
    return r64, f32, d64


# ---- judges ----------------------------------------------------------------------------------------------------------------

def judge_sums(tag, got, r64, f32=None):
    """recon and edge through kernel_bars.sum_bar against rounded64, sum |terms| as the scale"""
    kernel_bars.sum_bar(tag, "recon", np.asarray([got["recon"]]), np.asarray([r64.recon]), np.asarray([r64.recon_abs]),
                        f32=None if f32 is None else np.asarray([f32.recon]))
    kernel_bars.sum_bar(tag, "edge", np.asarray([got["edge"]]), np.asarray([r64.edge]), np.asarray([r64.edge_abs]),
                        f32=None if f32 is None else np.asarray([f32.edge]))


def judge_identity(tag, quantity, got, want, scale):
    """a device scalar against the same expression in float64 from the device's own operands"""
    line = "%s / %s: |dev - float64 of its own operands| = %.2e of sum |terms|" % (tag, quantity, abs(float(got) - want) / max(scale, 1e-300))
    print(line)
    assert np.isfinite(got) and abs(float(got) - want) <= IDENTITY_REL * scale, line


def judge_total(tag, got, w_recon=W_RECON, w_edge=W_EDGE, term_a=None, w_a=0.0, term_b=None):
    want, scale = LR.total64(got["recon"], got["edge"], w_recon, w_edge, term_a, w_a, term_b)
    judge_identity(tag, "total", got["total"], want, scale)


def judge_dpred(tag, regime, dpred, r64, f32, d64=None):
    """element_bar against rounded64 on the element and the vertex measure; in ``generic`` also 2e-5 per vertex against the
    definition, which ties the rounded-difference reference back to it"""
    dpred = np.asarray(dpred)
    assert dpred.dtype == F32 and dpred.shape == r64.dpred.shape, (tag, dpred.dtype, dpred.shape)
    kernel_bars.element_bar(tag, "dpred (element)", dpred, f32.dpred, r64.dpred)
    parity_bar.check(tag, "dpred (vertex)", vertex_err(dpred, r64.dpred), vertex_err(f32.dpred, r64.dpred), TOL, factor=4.0)
    if regime == "generic":
        err = vertex_err(dpred, d64.dpred)
        print("%s / dpred against the definition: %.2e per vertex" % (tag, err))
        assert err < TOL, (tag, err)


def judge_exact(tag, name, regime, dpred, slope32):
    """the facts that hold as values: a vertex without edges carries the recon slope times its scale and nothing else; a sample
    at gt = pred has no gradient at all; everything is finite.  ``slope32``: loss_reference.recon_slope32"""
    c = by_name(name)
    dpred = np.asarray(dpred)
    assert np.isfinite(dpred).all(), tag
    iso = c["graph"].get("isolated", 0) if isinstance(c["graph"], dict) else 0
    if iso:
        assert np.array_equal(dpred[:, c["V"] - iso:], slope32[:, c["V"] - iso:]), tag
    if regime == "zeros" and zero_sample(c["N"]) is not None:
        assert not dpred[zero_sample(c["N"])].any(), tag


# ---- adversarial losses ----------------------------------------------------------------------------------------------------

GAN_CASES = [(1, 1, 1), (2, 5, 37), (3, 3, 431), (1, 2, 1025), (4, 4, 300)]
GAN_SMOOTH = (0.0, 0.1)
GAN_DATA = ("generic", "extremes")
GAN_SCALE = 0.7
EXTREMES = (0.0, -0.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)


def gan_id(case):
    return "f%d_r%d_m%d" % case


def gan_extremes(smooth):
    """0, -0.0, where expf leaves the normal range (88) and underflows (104), where it is zero (1e4), and for smooth > 0 the
    logits where sigmoid - target cancels: logit(1 - smooth) against the real target, its negative against the fake one"""
    v = list(EXTREMES)
    if smooth > 0:
        t = float(F32(1.0) - F32(smooth))
        v += [np.log(t / (1.0 - t)), -np.log(t / (1.0 - t))]
    return np.asarray(v, F32)


@functools.lru_cache(maxsize=None)
def gan_inputs(case, smooth, data):
    """(fake [Nf, M], real [Nr, M]) fp32: 4 N(0, 1); ``extremes``: the special values on top, in both tensors, as far as they fit"""
    Nf, Nr, M = case
    rng = np.random.default_rng(_seed(gan_id(case), smooth, data))
    fake, real = ((4 * rng.standard_normal((n, M))).astype(F32) for n in (Nf, Nr))
    if data == "extremes":
        v = gan_extremes(smooth)
        for t, shift in ((fake, 0), (real, 3)):
            flat = t.reshape(-1)
            k = min(len(v), len(flat))
            at = rng.choice(len(flat), k, replace=False)
            flat[at] = np.roll(v, shift)[:k]
    fake.setflags(write=False)
    real.setflags(write=False)
    return fake, real


def judge_gan(tag, got, r64, f32):
    """got: dict(gan_g, gan_d, scaled_g, scaled_d, ga, gb [Nf + Nr, M]); ``nf``: rows of the generated samples"""
    kernel_bars.sum_bar(tag, "gan_g", np.asarray([got["gan_g"]]), np.asarray([r64.gan_g]), np.asarray([r64.g_abs]), f32=np.asarray([f32.gan_g]))
    kernel_bars.sum_bar(tag, "gan_d", np.asarray([got["gan_d"]]), np.asarray([r64.gan_d]), np.asarray([r64.d_abs]), f32=np.asarray([f32.gan_d]))
    sc = float(F32(GAN_SCALE))
    for k, v in (("scaled_g", "gan_g"), ("scaled_d", "gan_d")):
        judge_identity(tag, k, got[k], sc * float(got[v]), abs(sc * float(got[v])))
    for k in ("ga", "gb"):
        kernel_bars.element_bar(tag, k, np.asarray(got[k]), getattr(f32, k), getattr(r64, k))
    nf = got["nf"]
    assert not np.asarray(got["ga"])[nf:].any(), tag                # the real rows take no gradient from gan_g
