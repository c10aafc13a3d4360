"""The decoder's delivery planner for SIZED targets without a GPU: csrc/dec_delivery.h compiled for the host and swept under
AddressSanitizer + UndefinedBehaviorSanitizer by tools/dec_delivery_sized_check.cpp (a stand-alone program: nothing sanitized is loaded
into Python) over chroma format x size x delivered size x target kind x postsharp x draw_info x pointer offset x pitch, on synthetic
addresses.  The program checks that every job's destination lies inside the target or the staging it was given, that staging is asked
for exactly when the predicates say so, and that a target which is not sized gets no resampling job, no full-size staging and the
predicates' answers of before (what its plan does hold is the business of tests/test_dec_delivery_cpu.py, which is unchanged)."""
import re

import pytest

from sanitized_tool import build_and_run

# 5 formats x 7 sizes x 8 delivered sizes x 3 kinds x 4 sharp / draw x 9 placements; the plain comparison: one delivered size, 4 shifts
CASES = 5 * 7 * 8 * 3 * 4 * 9
PLAIN = 5 * 7 * 3 * 4 * 9 * 4


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/dec_delivery_sized_check.cpp with the sanitizers, runs its whole sweep and returns what it printed"""
    return build_and_run("tools/dec_delivery_sized_check.cpp", tmp_path_factory.mktemp("dec_delivery_sized"))[0]


def test_every_sized_case_of_the_sweep_holds(sweep):
    m = re.search(r"dec_delivery_sized_check: (\d+) sized cases \((\d+) in the wide form\): staging, jobs, ranges and form hold", sweep)
    assert m, sweep[-1000:]
    assert int(m.group(1)) == CASES
    assert 0 < int(m.group(2)) < CASES  # both forms of the resampling are planned


def test_targets_that_are_not_sized_get_nothing_of_the_resampling(sweep):
    m = re.search(r"(\d+) plans of targets that are not sized hold nothing of the resampling", sweep)
    assert m, sweep[-1000:]
    assert int(m.group(1)) == PLAIN
