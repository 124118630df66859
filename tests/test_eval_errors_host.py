"""test_errors on the host: the three C entries in the header and the binding, their argument checks (decided before any
launch), numpy's linear quantile rule restated as ranks, and every ValueError of the operand helper.  None of this needs a
device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 6890
ENTRIES = ("cape_vertex_error", "cape_error_stats_workspace_bytes", "cape_error_stats")


def test_header_names_the_entries_and_abi_is_18():
    from cape_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    assert int(re.search(r"#define CAPE_ABI_VERSION (\d+)", hdr).group(1)) == 18
    assert _lib.lib.cape_abi_version() == 18
    for name in ENTRIES:
        assert re.search(r"^\s*(?:int|int64_t)\s+%s\s*\(" % name, hdr, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.SIGNATURES["cape_error_stats_workspace_bytes"][0] is ctypes.c_int64
    assert "demos.py:68-78" in hdr[:hdr.index("#ifndef CAPE_HIP_H")]


def test_vertex_error_rejects_bad_arguments_before_launching():
    from cape_amd._lib import lib
    P = ctypes.c_void_p

    def call(**kw):
        a = dict(pred=P(0x100000), ldp=4, gt=P(0x200000), std=P(0x300000), idx=P(0x400000), N=2, V=V, Vc=3627,
                 dist=P(0x500000), row0=4, S=6)
        a.update(kw)
        return lib.cape_vertex_error(a["pred"], a["ldp"], a["gt"], a["std"], a["idx"], a["N"], a["V"], a["Vc"], a["dist"],
                                     a["row0"], a["S"], None)

    for name in ("pred", "gt", "std", "idx", "dist"):
        assert call(**{name: None}) == -1, name
    for name in ("N", "V", "Vc", "S"):
        assert call(**{name: 0}) == -1 and call(**{name: -2}) == -1, name
    assert call(Vc=V + 1) == -1
    assert call(ldp=2) == -1
    assert call(row0=5) == -1                                   # row0 + N > S
    assert call(row0=-1) == -1
    assert call(N=1, S=1 << 20, Vc=2048, row0=0) == -1          # S * Vc = 2^31


def test_error_stats_rejects_bad_arguments_before_launching():
    from cape_amd._lib import lib
    P = ctypes.c_void_p
    S, Vc = 64, 3627
    need = int(lib.cape_error_stats_workspace_bytes(S, Vc, 8))
    assert need >= 8 * 2048 * 4 + S * 8                         # a histogram per rank and a partial per sample at least
    assert lib.cape_error_stats_workspace_bytes(S, Vc, 1) <= need
    for bad in ((0, Vc, 2), (S, 0, 2), (-1, Vc, 2), (S, Vc, 0), (S, Vc, 9), (1 << 20, 2048, 2)):
        assert lib.cape_error_stats_workspace_bytes(*bad) == -1, bad

    def call(**kw):
        a = dict(dist=P(0x100000), S=S, Vc=Vc, ranks=[0, S * Vc // 2, S * Vc - 1], moments=P(0x200000), order=P(0x300000),
                 pv=P(0x400000), ps=P(0x500000), ws=P(0x600000), need=need)
        a.update(kw)
        r = a["ranks"]
        arr = None if r is None else (ctypes.c_int64 * max(len(r), 1))(*r)
        return lib.cape_error_stats(a["dist"], a["S"], a["Vc"], arr, a.get("R", 0 if r is None else len(r)), a["moments"],
                                    a["order"], a["pv"], a["ps"], a["ws"], a["need"], None)

    for name in ("dist", "moments", "order", "pv", "ps", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(ranks=None, R=2) == -1
    assert call(S=0) == -1 and call(Vc=0) == -1 and call(S=-3) == -1
    assert call(S=1 << 20, Vc=2048) == -1                       # S * Vc = 2^31
    assert call(ranks=[]) == -1 and call(ranks=list(range(9))) == -1
    assert call(ranks=[S * Vc]) == -1 and call(ranks=[-1]) == -1 and call(ranks=[0, 1 << 40]) == -1
    for ranks in ([0], [0, S * Vc // 2, S * Vc - 1], list(range(8))):
        exact = int(lib.cape_error_stats_workspace_bytes(S, Vc, len(ranks)))
        assert call(ranks=ranks, need=exact - 8) == -4          # workspace too small


@pytest.mark.parametrize("n", [1, 2, 185, 148])
@pytest.mark.parametrize("q", [0, 0.25, 0.5, 0.9, 1])
def test_quantile_ranks_agree_with_numpy(n, q):
    from cape_amd.ops import quantile_ranks
    lo, hi, frac = quantile_ranks(n, q)
    assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= frac < 1.0
    assert (lo, hi, frac) == (int(np.floor(q * (n - 1))), int(np.ceil(q * (n - 1))), q * (n - 1) - np.floor(q * (n - 1)))
    rng = np.random.default_rng(n)
    a = np.sort(np.exp(rng.uniform(-20, 5, n)).astype(np.float32)).astype(np.float64)
    got = a[lo] + (a[hi] - a[lo]) * frac
    want = float(np.quantile(a, q))                             # method 'linear' is numpy's default
    assert abs(got - want) <= 4 * 2.0 ** -53 * abs(want), (got, want)
    if q == 0.5:
        assert abs(got - float(np.median(a))) <= 4 * 2.0 ** -53 * abs(want)


def test_quantile_ranks_rejects_bad_input():
    from cape_amd.ops import quantile_ranks
    for n, q in ((0, 0.5), (5, -0.1), (5, 1.5), (5, float("nan"))):
        with pytest.raises(ValueError):
            quantile_ranks(n, q)


def test_error_arguments_defaults_and_broadcasts():
    from cape_amd.ops import error_arguments
    sd, idx, qs = error_arguments(V, 3, 5)
    assert sd.shape == (V, 3) and sd.dtype == np.float32 and (sd == 1).all()
    assert idx.dtype == np.int32 and np.array_equal(idx, np.arange(V)) and qs == (0.5,)
    sd, _, _ = error_arguments(V, 3, 5, std=0.25)
    assert (sd == 0.25).all()
    sd, _, _ = error_arguments(V, 3, 5, std=[1.0, 2.0, 3.0])
    assert (sd == np.array([1, 2, 3], dtype=np.float32)).all() and sd.shape == (V, 3)
    full = np.random.default_rng(0).uniform(0, 1, (V, 3))
    sd, idx, qs = error_arguments(V, 3, 5, std=full, clothing_idx=[7, 3, 6889, 0], quantiles=[0, 0.25, 0.5, 1])
    assert np.array_equal(sd, full.astype(np.float32))
    assert idx.tolist() == [7, 3, 6889, 0]                      # the order given
    assert qs == (0.0, 0.25, 0.5, 1.0)


@pytest.mark.parametrize("bad", ["idx_float", "idx_bool", "idx_negative", "idx_too_large", "idx_repeated", "idx_2d", "idx_empty",
                                 "std_nan", "std_inf", "std_negative", "std_shape", "five_quantiles", "no_quantiles",
                                 "quantile_above", "quantile_below", "quantile_nan", "six_channels", "too_many_values"])
def test_error_arguments_value_errors(bad):
    from cape_amd.ops import error_arguments
    kw = dict(num_verts=V, channels=3, size=5, std=None, clothing_idx=np.array([4, 2, 9]), quantiles=(0.5,))
    std = np.ones((V, 3))
    if bad == "idx_float":
        kw["clothing_idx"] = np.array([4.0, 2.0])
    elif bad == "idx_bool":
        kw["clothing_idx"] = np.ones(V, dtype=bool)
    elif bad == "idx_negative":
        kw["clothing_idx"] = np.array([4, -1])
    elif bad == "idx_too_large":
        kw["clothing_idx"] = np.array([4, V])
    elif bad == "idx_repeated":
        kw["clothing_idx"] = np.array([4, 2, 4])
    elif bad == "idx_2d":
        kw["clothing_idx"] = np.array([[4, 2]])
    elif bad == "idx_empty":
        kw["clothing_idx"] = np.array([], dtype=np.int64)
    elif bad == "std_nan":
        std[5, 1] = np.nan
        kw["std"] = std
    elif bad == "std_inf":
        kw["std"] = np.inf
    elif bad == "std_negative":
        std[0, 0] = -1e-3
        kw["std"] = std
    elif bad == "std_shape":
        kw["std"] = np.ones((V, 1))
    elif bad == "five_quantiles":
        kw["quantiles"] = (0.1, 0.2, 0.3, 0.4, 0.5)
    elif bad == "no_quantiles":
        kw["quantiles"] = ()
    elif bad == "quantile_above":
        kw["quantiles"] = (0.5, 1.01)
    elif bad == "quantile_below":
        kw["quantiles"] = (-0.01,)
    elif bad == "quantile_nan":
        kw["quantiles"] = (float("nan"),)
    elif bad == "six_channels":
        kw["channels"] = 6
    else:
        kw["size"], kw["clothing_idx"] = 1 << 20, np.arange(2048)          # size * Vc = 2^31
    with pytest.raises(ValueError):
        error_arguments(**kw)
    if bad == "too_many_values":
        kw["size"] -= 1
        error_arguments(**kw)                                              # 2^31 - 2048: allowed


def test_test_errors_checks_its_arguments_without_a_device(mesh_ops):
    """CAPE.test_errors raises from the helper before it touches weights or the device."""
    from cape_amd.configs import cape_params
    from cape_amd.models import CAPE
    m = mesh_ops
    model = CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], **cape_params(p=m["p"], batch_size=2))
    data = np.zeros((3, V, 3))
    cond, clo = np.zeros((3, 126)), np.zeros((3, 4))
    for kw in (dict(clothing_idx=[1, 1]), dict(std=-1.0), dict(quantiles=(0.1, 0.2, 0.3, 0.4, 0.5)), dict(quantiles=(2.0,)),
               dict(clothing_idx=[0.5])):
        with pytest.raises(ValueError):
            model.test_errors(data, cond, clo, **kw)
    model6 = CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], **cape_params(p=m["p"], batch_size=2, nn_input_channel=6))
    with pytest.raises(ValueError):
        model6.test_errors(np.zeros((3, V, 6)), cond, clo)
