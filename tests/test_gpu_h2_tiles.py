"""Every tile form of the fp16 two-piece contractions against float64 numpy (cases, references and judges: tests/h2_cases.py):
gemm_h2_kernel as 128 x 128, 128 x 64, 64 x 128, 64 x 64 and DUAL 128 x 64, gemm_h2x_kernel (128 x 256), dw_h2_kernel as
64 x 64, 64 x 128, 128 x 64 and 128 x 128.  Each case asserts the exact plan tuple the library reports before it judges.

What the shapes are for: pipeline lengths of 4 / 5 / 6 / 7 chunks (the four ways through the steady loop and its tail) and odd
lengths on the wide tile; a source change on every chunk, inside the grouped schedule, and with all eight source slots used; a
last row tile of one row, a column tile of 8 columns, F in 192..255; the general epilogue (rank-1 terms, vertex bias, tanh) on
the wide and the 64 x 64 tile; the DUAL form's second weight set ending at a source change and its sign mask; sources and
outputs that are channel-offset views with NaN next to them; row bounds of width 8 / 12 / 16 as a producing epilogue writes
them (width 20 must be declined, not mis-run), on a producer of every family; weight gradients with dz2, accumulate, a row range
shorter than one chunk per group, and NaN in the columns an edge tile overhangs.

The tiles the default process never chooses run in one fresh child process per knob leg (the library latches its knobs at
first use)."""
import os
import subprocess
import sys

import pytest

from tests import h2_cases as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_name = lambda c: c["name"]


@pytest.mark.parametrize("case", H.FWD_CASES, ids=_name)
def test_forward_tile(case):
    H.run_fwd(case)


@pytest.mark.parametrize("case", H.BWD_CASES, ids=_name)
def test_data_gradient_wide_tile(case):
    H.run_bwd(case)


@pytest.mark.parametrize("case", H.VIEW_CASES, ids=_name)
def test_channel_offset_views_next_to_nan(case):
    """Sources = columns 4 .. 4 + C of buffers C + 12 wide whose other columns hold NaN, output = columns 4 .. 4 + F of a
    sentinel-filled buffer: still family 3, finite, within the bar, nothing written outside the view."""
    H.run_fwd(case)


@pytest.mark.parametrize("case", H.CHAIN_CASES, ids=_name)
def test_row_bound_chain(case):
    """A producing epilogue (families 3, 0, 1, 2) writes the bounds of F_A columns; a two-piece consumer reads all of them: the
    producer's last 32-column block is 2^6 larger than the rest, so a consumer that read only the first four entries would
    overflow fp16.  Width 20 exceeds what the kernel reads: the launch must be declined and still be right."""
    H.run_chain(case)


@pytest.mark.parametrize("case", H.DW_CASES, ids=_name)
def test_weight_gradient_tile(case):
    H.run_dw(case)


@pytest.mark.parametrize("leg", sorted(H.LEG_CASES))
def test_knob_leg(leg):
    env = {k: v for k, v in os.environ.items() if k not in H.PLAN_KNOBS}
    env.update(H.LEG_ENV[leg])
    r = subprocess.run([sys.executable, "-m", "tests.h2_cases", leg], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, "(returncode %d) %s" % (r.returncode, out[-3000:])
    lines = out.splitlines()
    for case in H.LEG_CASES[leg]:
        want = "%dx%d" % case["tile"]
        hits = [l.split() for l in lines if l.split()[:1] == [case["name"]]]
        assert len(hits) == 1 and hits[0][1] == want, (case["name"], want, out[-3000:])
