"""The batch iterator, the padded host block and the posed drivers' argument checks that CAPE's inference and fitting drivers
share (cape_amd/models.py: _batches, _padded_np, _posed_arguments), without a device.  The padded block is held, bit for bit,
to the rule every driver used to spell out: a float64 block of zeros, the rows copied in front, cast to float32 on upload."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

BS = 4


@pytest.fixture(scope="module")
def model(mesh_ops):
    from cape_amd.configs import cape_params
    from cape_amd.models import CAPE
    m = mesh_ops
    return CAPE(L=m["L"], D=m["D"], U=m["U"], L_d=m["L_d"], D_d=m["D_d"], **cape_params(p=m["p"], batch_size=BS))


@pytest.mark.parametrize("size", [1, 3, 4, 5, 9])
def test_batches_cover_the_range_once_in_order(model, size):
    got = list(model._batches(size))
    assert [i for b, e in got for i in range(b, e)] == list(range(size))
    assert all(e - b == BS for b, e in got[:-1]) and 0 < got[-1][1] - got[-1][0] <= BS
    assert len(got) == -(-size // BS) and got[-1][1] - got[-1][0] == (size % BS or BS)


def _old_pad(arr, b, e):
    out = np.zeros((BS,) + tuple(arr.shape[1:]))
    out[:e - b] = arr[b:e] if isinstance(arr, np.ndarray) else arr[b:e].toarray()
    return out.astype(np.float32)


def _arrays():
    rng = np.random.default_rng(12)
    f64 = rng.standard_normal((9, 7)) * np.exp2(rng.integers(-30, 30, (9, 7)))      # values that float32 has to round
    csr = sp.random(9, 11, density=0.3, format="csr", random_state=3, dtype=np.float64)
    return dict(float64=f64, float32=f64.astype(np.float32), csr=sp.csr_matrix(csr), three_d=rng.standard_normal((9, 5, 3)))


@pytest.mark.parametrize("name", ["float64", "float32", "csr", "three_d"])
@pytest.mark.parametrize("size", [5, 9])
def test_padded_block_is_the_old_rule(model, name, size):
    arr = _arrays()[name][:size]
    for b, e in model._batches(size):
        got = model._padded_np(arr, b, e)
        assert got.dtype == np.float32 and got.shape == (BS,) + tuple(arr.shape[1:]) and got.flags.c_contiguous
        assert np.array_equal(got, _old_pad(arr, b, e))
        assert not got[e - b:].any()


@pytest.mark.parametrize("size", [5, 9])
def test_one_row_is_repeated_into_the_valid_rows_only(model, size):
    """decode's rule for one condition and many z samples: ``bc[:n] = cond[0:batch_size]`` on a block of zeros."""
    cond = _arrays()["float64"][2:3]
    for b, e in model._batches(size):
        want = np.zeros((BS, cond.shape[1]))
        want[:e - b] = cond[0:BS]
        got = model._padded_np(cond, b, e)
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
        assert (got[:e - b] == cond.astype(np.float32)).all() and not got[e - b:].any()


def test_posed_arguments_raise_the_drivers_messages(model):
    body = types.SimpleNamespace(J=24, V=6890)
    dress = (None, None, None, None)                    # never reached: the checks come first
    pose, cond, cond2 = np.zeros((5, 72)), np.zeros((5, 3)), np.zeros((5, 2))
    with pytest.raises(ValueError, match=r"^pose: 2 rows for 5 samples$"):
        model._posed_arguments(5, body, pose[:2], None, dress)
    with pytest.raises(ValueError, match=r"^transl: 2 rows for 5 samples$"):
        model._posed_arguments(5, body, pose, np.zeros((2, 3)), dress)
    with pytest.raises(ValueError, match=r"^cond / cond2: one row, or one per sample$"):
        model._posed_arguments(5, body, pose[:1], np.zeros((1, 3)), dress, cond, cond2[:1])
    with pytest.raises(ValueError, match=r"^cond / cond2: one row, or one per sample$"):
        model._posed_arguments(5, body, pose, None, dress, cond[:3], cond2[:3])
