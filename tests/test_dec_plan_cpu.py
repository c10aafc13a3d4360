"""The decoder's delivery planner for tensor targets, planar [3, h, w] and interleaved [h, w, 3], without a GPU: csrc/dec_delivery.h
compiled for the host and swept under AddressSanitizer + UndefinedBehaviorSanitizer by tools/dec_plan_check.cpp (a stand-alone program:
nothing sanitized is loaded into Python) over chroma format x size x element type x order x sized or not x postsharp x draw_info x
pointer offset x pitch, on synthetic addresses.  The program checks the jobs' addresses and contents; this file restates the rules for
the job counts, the wide flag and the staging predicates and compares them line by line.  The plans of earlier planners are pinned by
digests in tests/golden/: every FRAME / PLANAR / SEMI / RGB target of the older sweeps (dec_plans_parent.json), every planar tensor
target (dec_tensor_plans_parent.json) and every interleaved one with its job's members (dec_hwc_plans_parent.json) -- each recorded from
the planner of the commit its "what" names -- so one record for the three layouts plans what three records planned."""
import hashlib
import json
import os
import re

import pytest

import dsvabi as A
from sanitized_tool import build_and_run

ELEM = {0: 1, 1: 2, 2: 2, 3: 4}
# 5 formats x 5 sizes x 4 element types x 4 delivered sizes x 4 sharp / draw x 4 offsets x 3 pitches, x 2 orders for HWC
TENSOR_CASES = 5 * 5 * 4 * 4 * 4 * 4 * 3
HWC_CASES = 2 * TENSOR_CASES
# per format and size: FRAME 2 (out420p) + three device kinds x (plain 2, or 1 for RGB; 3 shifts; 3 sizes), x 4 sharp / draw x 9 placements
PARENT = 5 * 5 * (2 + (2 + 3 + 3) + (2 + 3 + 3) + (1 + 3 + 3)) * 4 * 9


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/dec_plan_check.cpp with the sanitizers, runs its whole sweep and returns what it printed"""
    return build_and_run("tools/dec_plan_check.cpp", tmp_path_factory.mktemp("dec_plan"))[0]


def test_every_tensor_case_of_the_sweep_holds(sweep):
    m = re.search(r"dec_plan_check: (\d+) planar tensor cases \((\d+) in the wide form\) and (\d+) interleaved \((\d+)\): target, staging, jobs and form hold",
                  sweep)
    assert m, sweep[-1000:]
    assert int(m.group(1)) == TENSOR_CASES
    assert 0 < int(m.group(2)) < TENSOR_CASES  # both forms of the planar conversion are planned
    assert int(m.group(3)) == HWC_CASES
    assert 0 < int(m.group(4)) < HWC_CASES  # ... and of the interleaved one


@pytest.mark.parametrize("prefix", ["R", "H"], ids=["planar", "interleaved"])
def test_job_counts_wide_flags_and_staging_follow_the_rules(sweep, prefix):
    """per case: one conversion job; the luma's egress job exactly under postsharp / draw_info; three resampling jobs exactly for a sized
    tensor; the overlay exactly under draw_info, sharpened in place behind it exactly with postsharp on top; wide exactly where the
    pointers (256 bytes + offset elements behind a 16-byte boundary) and the pitch are multiples of four elements and the delivered width
    of 4; the staged luma, the staged scaled picture and its full size exactly where the predicates' rules say"""
    hwc = prefix == "H"
    lines = [ln.split() for ln in sweep.splitlines() if ln.startswith(prefix + " ")]
    assert len(lines) == (HWC_CASES if hwc else TENSOR_CASES)
    seen = set()
    for f in lines:
        head = 12 if hwc else 11
        assert f[head] == ":"
        if hwc:
            fmt, w, h, dtype, bgr, ow, oh, sharp, draw, offset, pitch_kind = (int(v) for v in f[1:12])
            assert f[head + 10] == "hwc" and len(f) == head + 10 + 1 + 19 + 6
        else:
            fmt, w, h, dtype, ow, oh, sharp, draw, offset, pitch_kind = (int(v) for v in f[1:11])
            bgr = 0
            assert len(f) == head + 10
        got = tuple(int(v) for v in f[head + 1:head + 10])
        elem, dw = ELEM[dtype], ow or w
        rb = (3 if hwc else 1) * dw * elem
        pitch = rb if pitch_kind == 0 else rb + elem if pitch_kind == 1 else (rb + 255) // 256 * 256
        sized, staged = int(ow != 0), int(bool(sharp or draw))
        wide = int((256 + offset * elem) % (4 * elem) == 0 and pitch % (4 * elem) == 0 and dw % 4 == 0)
        want = (staged, 3 * sized, 1, int(draw != 0), int(bool(draw and sharp)), wide, staged, sized, sized)
        assert got == want, f
        seen.add((dtype, bgr, sized, staged, wide))
    assert len(seen) == 4 * (2 if hwc else 1) * 2 * 2 * 2  # every element type (and order), sized and not, staged and not, in both forms


def digests(sweep, prefix):
    groups, count = {}, 0
    for ln in sweep.splitlines():
        if ln.startswith(prefix + " "):
            f = ln.split()
            groups.setdefault("%s %sx%s" % (f[1], f[2], f[3]), hashlib.sha256()).update((ln + "\n").encode())
            count += 1
    return {k: v.hexdigest() for k, v in groups.items()}, count


def test_plans_of_the_surface_targets_equal_the_parent_planners(sweep):
    golden = json.load(open(os.path.join(A.ROOT, "tests", "golden", "dec_plans_parent.json")))
    m = re.search(r"(\d+) plans of the other targets and (\d+) of tensor targets printed$", sweep, flags=re.M)
    assert m and int(m.group(1)) == PARENT, sweep[-1000:]
    groups, count = digests(sweep, "P")
    assert count == PARENT and len(groups) == 25 and PARENT == 25 * golden["cases_per_group"]
    assert groups == golden["groups"]


def test_plans_of_the_tensor_targets_equal_the_parent_planners(sweep):
    golden = json.load(open(os.path.join(A.ROOT, "tests", "golden", "dec_tensor_plans_parent.json")))
    m = re.search(r"(\d+) of tensor targets printed$", sweep, flags=re.M)
    assert m and int(m.group(1)) == TENSOR_CASES, sweep[-1000:]
    groups, count = digests(sweep, "T")
    assert count == TENSOR_CASES and len(groups) == 25 and TENSOR_CASES == 25 * golden["cases_per_group"]
    assert groups == golden["groups"]


def test_plans_of_the_interleaved_targets_equal_the_parent_planners(sweep):
    golden = json.load(open(os.path.join(A.ROOT, "tests", "golden", "dec_hwc_plans_parent.json")))
    groups, count = digests(sweep, "H")
    assert count == HWC_CASES and len(groups) == 25 and HWC_CASES == 25 * golden["cases_per_group"]
    assert groups == golden["groups"]
