"""The decoder's delivery planner without a GPU: csrc/dec_delivery.h -- which kernels a picture leaves through, in which order, reading and
writing what -- compiled for the host and swept under AddressSanitizer + UndefinedBehaviorSanitizer by tools/dec_delivery_check.cpp (a
stand-alone program: nothing sanitized is loaded into Python) over chroma format x size x target kind x scale x out420p x postsharp x
draw_info x pointer offset x pitch, on synthetic addresses.  The program checks coverage, launch order, kernel forms, job counts and
sources of every case by its own interval arithmetic and states how many cases hit each row of the planner's table."""
import re

import pytest

from sanitized_tool import build_and_run

# 5 formats x 6 sizes x (a pinned frame: 2 out420p; planar / semiplanar: (2 out420p + 3 shifts) x 9 placements; RGB: 4 shifts x 9) x 4 sharp / draw
CASES = 5 * 6 * (2 + 2 * 5 * 9 + 4 * 9) * 4
TABLE_ROWS = 12


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/dec_delivery_check.cpp with the sanitizers, runs its whole sweep and returns what it printed"""
    return build_and_run("tools/dec_delivery_check.cpp", tmp_path_factory.mktemp("dec_delivery"))[0]


def test_every_case_of_the_sweep_holds(sweep):
    m = re.search(r"dec_delivery_check: (\d+) cases: coverage, order, form, counts and sources hold", sweep)
    assert m, sweep[-1000:]
    assert int(m.group(1)) == CASES


def test_every_row_of_the_planners_table_is_hit(sweep):
    rows = re.findall(r"^\s+(\d+) cases  (\S.*)$", sweep, flags=re.M)
    assert len(rows) == TABLE_ROWS
    print(sweep)
    for hits, name in rows:
        assert 0 < int(hits) < CASES, name
