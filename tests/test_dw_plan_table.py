"""What the weight-gradient host path decides, pinned without a GPU: tools/record_dw_plans.py recomputed against the committed
tests/dw_plan_table.json -- the kernel id, tile, slab count and workspace size of every case of its grid (a readable subset row
by row, the whole grid by digest), the same digest under each kernel-selection switch (one child process per switch: the
library latches them at first use), the batched-contraction plans of the lists of tests/test_dw_batch_plan.py, and the return
codes of the argument errors.  The table is a record of the library's decisions, not a specification: re-record it (and say
why) when a tile, slot or split rule is meant to change."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_dw_plans as R                # noqa: E402

TABLE = json.load(open(R.TABLE))


@pytest.fixture(scope="module")
def rows():
    assert not any(k in os.environ for k in R.PLAN_KNOBS), "the table holds the plans of the library's defaults"
    return R.grid_rows()


def test_whole_grid_by_digest(rows):
    assert len(rows) == TABLE["grid_cases"]
    assert R.digest(rows) == TABLE["grid_sha256"]


def test_readable_subset_row_by_row(rows):
    sub = R.subset_of(rows)                                   # (also asserts that every kernel id and tile is reached)
    assert len(sub) == len(TABLE["subset"])
    for got, want in zip(sub, TABLE["subset"]):
        assert got == want, (dict(zip(TABLE["columns"], got)), dict(zip(TABLE["columns"], want)))


@pytest.mark.parametrize("switch", R.SWITCHES)
def test_grid_digest_with_one_switch_off(switch):
    assert R.switch_digest(switch) == TABLE["switch_sha256"][switch]
    assert TABLE["switch_sha256"][switch] != TABLE["grid_sha256"]          # (the switch moves a plan of the grid)


def test_batched_contraction_plans():
    assert R.batch_plans() == TABLE["batch_plans"]


def test_argument_errors():
    got = R.error_cases()
    assert got == TABLE["errors"]
    # what the interface promises, independent of the record: -1 = CAPE_EINVAL, -3 = CAPE_EWORKSPACE
    assert got["stage_3"][1] == -1 and got["null_srcs"] == [-1, -1] and got["nsrc_0"] == [-1, -1] and got["nsrc_9"] == [-1, -1]
    assert got["lddz_below_F"] == [-1, -1] and got["dz2_mask_without_dz2"][1] == -1
