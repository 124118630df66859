"""The stand-alone element-wise and reduction operators of csrc/elementwise.hip (``bias_act_kernel``, ``act_bwd_kernel<VEC>``,
``mask_mul_kernel``, ``colsum_partial[_vec]_kernel`` + ``colsum_final_kernel``, ``sum_over_samples_kernel``, ``fill_cond_kernel``,
``reduce_cond[_vec]_kernel``, ``rowscale_partial / final_kernel``) against numpy, operator by operator.

Each of them chooses between a float4 and a scalar form on pointer / stride / channel alignment (``aligned4``; for the column
sums also ``256 % (C / 4) == 0``).  Every case therefore runs THE SAME DATA IN TWO LAYOUTS: ``padded``, the row-padded
16-byte-aligned view of ``ops.alloc_act``, and ``sliced``, a channel slice that starts at channel 1 of a wider buffer, which
no float4 access can address.  Row padding and the channels outside a slice hold 1e9 in inputs (a kernel that reads them
shows it) and a marker in outputs (a kernel that writes them shows it).

Results that are one rounding of an exact float32 expression must equal the float32 numpy evaluation bit for bit; tanh and
its gradient meet the element bar; the fixed-order sums meet the sum bar per output element (tests/kernel_bars.py)."""
import numpy as np
import pytest
import torch

from kernel_bars import element_bar, sum_bar, same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = 1.0e9           # around inputs
MARK = -7.0e8            # around outputs
LAYOUTS = ("padded", "sliced")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class Lay(object):
    """[N, M, C] device view ``v`` of a buffer ``base`` [N, M, ld] filled with ``fill``; the view is channels [c0, c0 + C)."""

    def __init__(self, host, layout, dev, fill, c0=None, ld=None):
        from cape_amd import ops
        N, M, Cn = host.shape
        if layout == "padded":
            self.v = ops.alloc_act(N, M, Cn, dev)
            self.base = self.v if self.v._base is None else self.v._base
            self.c0 = 0
            assert self.v.data_ptr() % 16 == 0 and self.base.shape[2] % 4 == 0
        elif layout == "sliced":
            self.base = torch.empty((N, M, Cn + 6), device=dev)
            self.c0 = 1
            self.v = self.base[:, :, 1:1 + Cn]
            assert self.v.data_ptr() % 16 == 4
        else:                                   # channels [c0, c0 + C) of a row-padded buffer of ld channels
            self.base = torch.empty((N, M, ld), device=dev)
            self.c0 = c0
            self.v = self.base[:, :, c0:c0 + Cn]
        self.fill, self.C = fill, Cn
        self.base.fill_(fill)
        self.v.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(dev))

    def host(self):
        return self.v.cpu().numpy()

    def outside_untouched(self):
        h = self.base.cpu().numpy().copy()
        h[:, :, self.c0:self.c0 + self.C] = F32(self.fill)
        return bool((h == F32(self.fill)).all())


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _act32(v, act):
    """cape_act in float32, operation for operation."""
    if act == "leaky":
        return np.where(v > 0, v, F32(0.2) * v).astype(F32)
    if act == "relu":
        return np.where(v > 0, v, F32(0)).astype(F32)
    if act == "tanh":
        return np.tanh(v).astype(F32)
    return v


def _act_grad(y, act, T):
    """cape_act_grad_from_out: the derivative expressed through the OUTPUT (y > 0 ? 1 : 0.2 / 0, so 0.2 / 0 at both zeros)."""
    if act == "leaky":
        return np.where(y > 0, T(1), T(0.2))
    if act == "relu":
        return np.where(y > 0, T(1), T(0))
    if act == "tanh":
        return T(1) - y.astype(T) * y.astype(T)
    return np.ones(y.shape, T)


# ---------------------------------------------------------------------------------------------- bias + activation
BA_SHAPES = [(3, 431, 64), (2, 862, 35), (1, 6890, 3), (16, 27, 262)]


def _bias_act_data(N, M, Cn, mode, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, M, Cn)).astype(F32)
    bias = None
    if mode == "channel":
        bias = (0.5 * rng.standard_normal((1, 1, Cn))).astype(F32)
    elif mode == "vertex":
        bias = (0.5 * rng.standard_normal((1, M, Cn))).astype(F32)
    b = F32(0) if bias is None else bias
    # exact zeros of x + b (x = -b) and negative zeros (x = -0 where b = -0)
    flat = x.reshape(-1)
    xb = np.broadcast_to(b, x.shape).reshape(-1) if bias is not None else None
    idx = np.arange(0, flat.size, 11)
    flat[idx] = F32(0) if bias is None else -xb[idx]
    if bias is not None:
        bias[..., 0] = F32(-0.0)
    x[:, ::5, 0] = F32(-0.0)
    s = x.copy() if bias is None else (x + b).astype(F32)          # (no bias: nothing is added, -0 stays -0)
    assert (s == 0).sum() > 0 and np.signbit(s[s == 0]).any() and (~np.signbit(s[s == 0])).any()
    dy = rng.standard_normal((N, M, Cn)).astype(F32)
    return x, bias, s, dy


@pytest.mark.parametrize("mode", ["none", "channel", "vertex"])
@pytest.mark.parametrize("act", ["none", "leaky", "relu", "tanh"])
@pytest.mark.parametrize("shape", BA_SHAPES, ids=["x".join(map(str, s)) for s in BA_SHAPES])
def test_bias_act_and_its_gradient(shape, act, mode, dev):
    from cape_amd import ops, _lib
    N, M, Cn = shape
    tag = "bias_act[%s,%s,%s]" % ("x".join(map(str, shape)), act, mode)
    x, bias, s, dy = _bias_act_data(N, M, Cn, mode, 7)
    bmode = {"none": _lib.BIAS_NONE, "channel": _lib.BIAS_CHANNEL, "vertex": _lib.BIAS_VERTEX}[mode]
    bt = None if bias is None else _t(bias, dev)
    y32 = _act32(s, act)
    y64 = np.tanh(s.astype(np.float64)) if act == "tanh" else y32.astype(np.float64)
    dz32 = (dy * _act_grad(y32, act, F32)).astype(F32)
    dz64 = dy.astype(np.float64) * _act_grad(y32.astype(np.float64), act, np.float64)

    def fwd_ok(got, what):
        if act == "tanh":
            element_bar(tag, what, got, y32, y64)
        else:
            assert same_bits(got, y32), what

    def bwd_ok(got, what):
        if act == "tanh":
            element_bar(tag, what, got, dz32, dz64)
        else:
            assert same_bits(got, dz32), what

    for layout in LAYOUTS:
        xin, yout = Lay(x, layout, dev, POISON), Lay(np.zeros_like(x), layout, dev, MARK)
        ops.bias_act_fwd(xin.v, bt, bmode, act, y=yout.v)
        fwd_ok(yout.host(), "y[%s]" % layout)
        assert yout.outside_untouched() and xin.outside_untouched() and same_bits(xin.host(), x)
        xio = Lay(x, layout, dev, MARK)                              # in place: y aliases x
        ops.bias_act_fwd(xio.v, bt, bmode, act, y=xio.v)
        fwd_ok(xio.host(), "y_inplace[%s]" % layout)
        assert xio.outside_untouched()

        yin, gin, zout = Lay(y32, layout, dev, POISON), Lay(dy, layout, dev, POISON), Lay(np.zeros_like(x), layout, dev, MARK)
        ops.act_bwd(gin.v, yin.v, act, dz=zout.v)
        bwd_ok(zout.host(), "dz[%s]" % layout)
        assert zout.outside_untouched()
        gio = Lay(dy, layout, dev, MARK)                             # in place: dz aliases dy
        ops.act_bwd(gio.v, yin.v, act, dz=gio.v)
        bwd_ok(gio.host(), "dz_inplace[%s]" % layout)
        assert gio.outside_untouched()
        # mixed alignment: an aligned gradient with a sliced output must take the scalar form
        other = Lay(np.zeros_like(x), LAYOUTS[1 - LAYOUTS.index(layout)], dev, MARK)
        ops.act_bwd(gin.v, yin.v, act, dz=other.v)
        bwd_ok(other.host(), "dz_mixed[%s]" % layout)
        assert other.outside_untouched()

        # the autograd operator: forward, data gradient, bias gradient (column sums over samples and vertices, or samples)
        xa = Lay(x, layout, dev, POISON).v.detach().requires_grad_(True)
        ba = None if bt is None else bt.clone().requires_grad_(True)
        ya = ops.BiasActFn.apply(xa, ba, act, bmode)
        fwd_ok(ya.detach().cpu().numpy(), "BiasActFn.y[%s]" % layout)
        g = Lay(dy, layout, dev, POISON).v
        grads = torch.autograd.grad(ya, (xa,) if ba is None else (xa, ba), g)
        yh = ya.detach().cpu().numpy()
        d32 = (dy * _act_grad(yh, act, F32)).astype(F32)             # (from the operator's own output, as the kernel takes it)
        d64 = dy.astype(np.float64) * _act_grad(yh.astype(np.float64), act, np.float64)
        got = grads[0].cpu().numpy()
        if act == "tanh":
            element_bar(tag, "BiasActFn.dx[%s]" % layout, got, d32, d64)
        else:
            assert same_bits(got, d32)
        if ba is not None:
            dz_dev = got.astype(np.float64)                          # the sums are taken over the device's dz
            axes = (0, 1) if mode == "channel" else (0,)
            sum_bar(tag, "BiasActFn.dbias[%s]" % layout, grads[1].cpu().numpy().reshape(dz_dev.sum(axes).shape), dz_dev.sum(axes),
                    np.abs(dz_dev).sum(axes), f32=got.sum(axes, dtype=F32))


# ---------------------------------------------------------------------------------------------- column sums
COLSUM_VEC_C = [4, 32, 64, 128, 256, 512]            # float4 form in the padded layout
COLSUM_SCALAR_C = [3, 36, 96, 70, 262, 260]          # C % 4 != 0, or 256 % (C / 4) != 0, or C > 256 not a multiple of 256
COLSUM_ROWS = {1: (1, 1), 127: (1, 127), 128: (2, 64), 129: (3, 43), 2 * 6890: (2, 6890)}


@pytest.mark.parametrize("rows", list(COLSUM_ROWS))
@pytest.mark.parametrize("Cn", COLSUM_VEC_C + COLSUM_SCALAR_C)
def test_colsum_over_samples_and_vertices(Cn, rows, dev):
    from cape_amd import ops
    N, M = COLSUM_ROWS[rows]
    rng = np.random.default_rng(1000 + Cn + rows)
    x = (rng.standard_normal((N, M, Cn)) * np.exp2(rng.integers(-3, 4, (1, 1, Cn)))).astype(F32)
    out0 = rng.standard_normal(Cn).astype(F32)
    x64 = x.astype(np.float64)
    for layout in LAYOUTS:
        for acc in (False, True):
            xin = Lay(x, layout, dev, POISON)
            out = torch.full((Cn + 8,), MARK, device=dev)
            out[:Cn] = _t(out0, dev)
            ops.colsum(xin.v, out[:Cn], per_vertex=False, accumulate=acc)
            got = out.cpu().numpy()
            ref = x64.sum((0, 1)) + (out0 if acc else 0.0)
            scale = np.abs(x64).sum((0, 1)) + (np.abs(out0) if acc else 0.0)
            f32 = x.reshape(-1, Cn).sum(0, dtype=F32) + (out0 if acc else F32(0))
            sum_bar("colsum[C%d,%dx%d,%s,acc%d]" % (Cn, N, M, layout, acc), "out", got[:Cn], ref, scale, f32=f32)
            assert (got[Cn:] == F32(MARK)).all() and xin.outside_untouched()


PV_SHAPES = [(3, 43, 36), (2, 6890, 64), (16, 27, 262), (1, 127, 4), (64, 431, 3)]


@pytest.mark.parametrize("shape", PV_SHAPES, ids=["x".join(map(str, s)) for s in PV_SHAPES])
def test_colsum_per_vertex(shape, dev):
    from cape_amd import ops
    N, M, Cn = shape
    rng = np.random.default_rng(31)
    x = rng.standard_normal(shape).astype(F32)
    out0 = rng.standard_normal((M, Cn)).astype(F32)
    x64 = x.astype(np.float64)
    for layout in LAYOUTS:
        for acc in (False, True):
            xin = Lay(x, layout, dev, POISON)
            out = torch.full((M * Cn + 8,), MARK, device=dev)
            out[:M * Cn] = _t(out0.reshape(-1), dev)
            ops.colsum(xin.v, out[:M * Cn], per_vertex=True, accumulate=acc)
            got = out.cpu().numpy()
            ref = x64.sum(0) + (out0 if acc else 0.0)
            scale = np.abs(x64).sum(0) + (np.abs(out0) if acc else 0.0)
            sum_bar("colsum_vertex[%s,%s,acc%d]" % ("x".join(map(str, shape)), layout, acc), "out", got[:M * Cn].reshape(M, Cn), ref, scale,
                    f32=x.sum(0, dtype=F32) + (out0 if acc else F32(0)))
            assert (got[M * Cn:] == F32(MARK)).all() and xin.outside_untouched()


# ---------------------------------------------------------------------------------------------- condition channels
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("M", [1, 3, 255, 256, 431, 6890])
@pytest.mark.parametrize("Cx", [64, 67])
@pytest.mark.parametrize("Cc", [4, 35, 64, 68, 6, 130])
def test_fill_and_reduce_cond(Cc, Cx, M, N, dev):
    """The condition channels [Cx, Cx + Cc) of a row-padded [N, M, Cx + Cc] activation: filled from cond [N, Cc] (x scale[m]) and
    reduced back over the vertices.  Cx = 64 with Cc % 4 == 0 is the float4 form of the reduction (two rows per trip and a
    one-row tail: M = 255 / 256 / 431 / 6890 end differently), everything else the scalar one."""
    from cape_amd import ops
    tag = "cond[Cc%d,Cx%d,M%d,N%d]" % (Cc, Cx, M, N)
    rng = np.random.default_rng(Cc * 7 + Cx + M + N)
    ld = (Cx + Cc + 3) // 4 * 4
    cond = rng.standard_normal((N, Cc)).astype(F32)
    scale = rng.uniform(0.25, 2.0, M).astype(F32)
    dy = rng.standard_normal((N, M, Cc)).astype(F32)
    out0 = rng.standard_normal((N, Cc)).astype(F32)
    condw = torch.full((N, Cc + 5), POISON, device=dev)                    # cond itself as a row-strided view
    condw[:, 2:2 + Cc] = _t(cond, dev)
    for sc in (None, scale):
        sct = None if sc is None else _t(sc, dev)
        y = Lay(np.zeros((N, M, Cc), F32), "channels", dev, MARK, c0=Cx, ld=ld)
        ops.fill_cond(condw[:, 2:2 + Cc], y.v, scale=sct)
        want = np.broadcast_to(cond[:, None, :], (N, M, Cc))
        if sc is not None:
            want = (want * sc[None, :, None]).astype(F32)
        assert same_bits(y.host(), np.ascontiguousarray(want)), "fill_cond"
        assert y.outside_untouched()

        g = Lay(dy, "channels", dev, POISON, c0=Cx, ld=ld)
        terms = dy.astype(np.float64) * (1.0 if sc is None else sc.astype(np.float64)[None, :, None])
        t32 = (dy * (F32(1) if sc is None else sc[None, :, None])).astype(F32)
        for acc in (False, True):
            outw = torch.full((N, Cc + 3), MARK, device=dev)              # the result as a row-strided view too
            outw[:, :Cc] = _t(out0, dev)
            ops.reduce_cond(g.v, scale=sct, out=outw[:, :Cc], accumulate=acc)
            got = outw.cpu().numpy()
            sum_bar(tag, "reduce_cond[scale%d,acc%d]" % (sc is not None, acc), got[:, :Cc], terms.sum(1) + (out0 if acc else 0.0),
                    np.abs(terms).sum(1) + (np.abs(out0) if acc else 0.0), f32=t32.sum(1, dtype=F32) + (out0 if acc else F32(0)))
            assert (got[:, Cc:] == F32(MARK)).all()
        assert g.outside_untouched()
    assert float(condw[:, :2].min().cpu()) == POISON and float(condw[:, 2 + Cc:].min().cpu()) == POISON


@pytest.mark.parametrize("shape", [(2, 431, 64, 32), (1, 255, 67, 35), (3, 6890, 64, 68), (16, 27, 3, 130), (1, 1, 67, 6)],
                         ids=lambda s: "x".join(map(str, s)))
def test_concat_cond_operator(shape, dev):
    """ops.ConcatCondFn: [x | cond tiled over the vertices] and its two gradients."""
    from cape_amd import ops
    N, M, Cx, Cc = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((N, M, Cx)).astype(F32)
    cond = rng.standard_normal((N, Cc)).astype(F32)
    g = rng.standard_normal((N, M, Cx + Cc)).astype(F32)
    xt, ct = _t(x, dev).requires_grad_(True), _t(cond, dev).requires_grad_(True)
    out = ops.ConcatCondFn.apply(xt, ct)
    want = np.concatenate([x, np.broadcast_to(cond[:, None, :], (N, M, Cc))], 2)
    assert same_bits(out.detach().cpu().numpy(), want)
    for layout in LAYOUTS:
        gl = Lay(g, layout, dev, POISON)
        dx, dc = torch.autograd.grad(out, (xt, ct), gl.v, retain_graph=True)
        assert same_bits(dx.cpu().numpy(), np.ascontiguousarray(g[:, :, :Cx]))
        gc = g[:, :, Cx:].astype(np.float64)
        sum_bar("concat_cond[%s,%s]" % ("x".join(map(str, shape)), layout), "dcond", dc.cpu().numpy(), gc.sum(1), np.abs(gc).sum(1),
                f32=g[:, :, Cx:].sum(1, dtype=F32))


# ---------------------------------------------------------------------------------------------- dropout-style bit masks
@pytest.mark.parametrize("Fc", [1, 31, 32, 33, 96, 262])
def test_mask_mul(Fc, dev):
    from cape_amd import ops
    N, M = 3, 431
    rng = np.random.default_rng(Fc)
    words = (Fc + 31) // 32
    mask = rng.integers(0, 1 << 32, (N * M, words), dtype=np.uint64).astype(np.uint32)
    if Fc % 32:
        mask[:, -1] |= np.uint32((0xFFFFFFFF << (Fc % 32)) & 0xFFFFFFFF)       # the unused high bits are SET: they must be ignored
    dy = rng.standard_normal((N, M, Fc)).astype(F32)
    f = np.arange(Fc)
    keep = ((mask[:, f >> 5] >> (f & 31).astype(np.uint32)) & np.uint32(1)).astype(bool).reshape(N, M, Fc)
    assert keep.any() and (~keep).any() if Fc > 1 else True
    want = np.where(keep, dy, F32(0)).astype(F32)
    mt = torch.from_numpy(mask.view(np.int32)).to(dev)
    for layout in LAYOUTS:
        gin, zout = Lay(dy, layout, dev, POISON), Lay(np.zeros_like(dy), layout, dev, MARK)
        ops.mask_mul(gin.v, mt, dz=zout.v)
        assert same_bits(zout.host(), want) and zout.outside_untouched() and gin.outside_untouched()
        gio = Lay(dy, layout, dev, MARK)
        ops.mask_mul(gio.v, mt, dz=gio.v)                                       # in place
        assert same_bits(gio.host(), want) and gio.outside_untouched()


# ---------------------------------------------------------------------------------------------- rank-1 condition terms
@pytest.mark.parametrize("Fc", [3, 64, 70, 256])
@pytest.mark.parametrize("Mo", [1, 31, 32, 33, 431, 6890])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_rowscale_reduce(R, Mo, Fc, dev):
    """out[n, j, f] = sum_r rowscale[j, r] dz[n, r, f]."""
    from cape_amd import ops
    N = 2
    rng = np.random.default_rng(R * 1000 + Mo + Fc)
    dz = rng.standard_normal((N, Mo, Fc)).astype(F32)
    rs = rng.standard_normal((R, Mo)).astype(F32)
    terms = rs.astype(np.float64)[None, :, :, None] * dz.astype(np.float64)[:, None, :, :]          # [N, R, Mo, F]
    t32 = (rs[None, :, :, None] * dz[:, None, :, :]).astype(F32)
    rst = torch.full((R * Mo + 16,), POISON, device=dev)
    rst[:R * Mo] = _t(rs.reshape(-1), dev)
    for layout in LAYOUTS:
        zin = Lay(dz, layout, dev, POISON)
        out = ops.rowscale_reduce(zin.v, rst[:R * Mo], R)
        assert tuple(out.shape) == (N, R, Fc)
        sum_bar("rowscale_reduce[R%d,Mo%d,F%d,%s]" % (R, Mo, Fc, layout), "out", out.cpu().numpy(), terms.sum(2), np.abs(terms).sum(2),
                f32=t32.sum(2, dtype=F32))
        assert zin.outside_untouched()


def test_rowscale_reduce_refuses_more_than_four_terms(dev):
    from cape_amd import ops
    dz = torch.zeros((2, 33, 64), device=dev)
    rs = torch.zeros((5, 33), device=dev)
    with pytest.raises(RuntimeError):
        ops.rowscale_reduce(dz, rs, 5)
    with pytest.raises(RuntimeError):
        ops.rowscale_reduce(dz, rs, 0)
