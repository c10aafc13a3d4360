"""The encoder's acceptance rule and ingest planner for HWC sources (dsv2hip_enc_batch_hwc) without a GPU: csrc/enc_ingest.h compiled
for the host and swept under AddressSanitizer + UndefinedBehaviorSanitizer by tools/enc_hwc_plan_check.cpp (a stand-alone program:
nothing sanitized is loaded into Python) over chroma format x size x element type x order x pointer offset x pitch, on synthetic
addresses.  The program checks acceptance, every refusal, the job's addresses, quads, constants and form, and that a uint8 tensor is
the three-byte surface member for member; this file restates the rules for the record counts and the wide fact and compares them line
by line.  For every surface kind, call and route of the older sweep the program prints every member an IngestPlan had before tensors;
their digests equal tests/golden/enc_plans_parent.json.  For every planar tensor case of tools/enc_tensor_plan_check.cpp's sweep it
prints the whole plan, tensor job and constants included; their digests equal tests/golden/enc_tensor_plans_parent.json, recorded from
the PARENT commit's enc_ingest.h compiled into the same program under another namespace (the tool's -DPARENT_HEADER build, which also
compares the two planners' lines): the plans of every source that existed are what they were."""
import hashlib
import json
import os
import re

import pytest

import dsvabi as A
from sanitized_tool import build_and_run

ELEM = {0: 1, 1: 2, 2: 2, 3: 4}
CASES = 5 * 5 * 4 * 2 * 4 * 3    # formats x sizes x element types x orders x offsets x pitches
TENSORS = 5 * 5 * 4 * 4 * 3      # formats x sizes x element types x offsets x pitches
PARENT = 5 * 5 * 5 * 12 * 4 * 3  # formats x sizes x surface kinds x (call, route) x offsets x pitches


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/enc_hwc_plan_check.cpp with the sanitizers, runs its whole sweep and returns what it printed"""
    return build_and_run("tools/enc_hwc_plan_check.cpp", tmp_path_factory.mktemp("enc_hwc_plan"))[0]


def test_every_hwc_case_of_the_sweep_holds(sweep):
    m = re.search(r"enc_hwc_plan_check: (\d+) hwc cases \((\d+) in the wide form\): acceptance, refusals, job and form hold", sweep)
    assert m, sweep[-1000:]
    assert int(m.group(1)) == CASES
    assert 0 < int(m.group(2)) < CASES  # both forms are planned


def test_record_counts_and_the_wide_fact_follow_the_rules(sweep):
    """per case: a float tensor brings one HwcInJob and no Rgb3Job, a uint8 tensor one packed Rgb3Job and no HwcInJob; wide exactly where
    the pointer (256 bytes + offset elements behind a 256-byte boundary) and the pitch (tight; + 1 element; rounded up to 256 bytes) are
    multiples of four elements -- a uint8 tensor: of four bytes, the three-byte surface's rule -- and w of 4"""
    lines = [ln.split() for ln in sweep.splitlines() if ln.startswith("H ")]
    assert len(lines) == CASES
    seen = set()
    for f in lines:
        assert f[8] == ":"
        fmt, w, h, dtype, order, offset, pitch_kind = (int(v) for v in f[1:8])
        got = tuple(int(v) for v in f[9:])
        elem = ELEM[dtype]
        rb = 3 * w * elem
        pitch = rb if pitch_kind == 0 else rb + elem if pitch_kind == 1 else (rb + 255) // 256 * 256
        wide = int(offset % 4 == 0 and pitch % (4 * elem) == 0 and w % 4 == 0)
        assert got == (int(dtype != 0), int(dtype == 0), wide), f
        assert order in (0x20, 0x21)
        seen.add((dtype, order, wide))
    assert len(seen) == 4 * 2 * 2  # every element type in both orders and both forms


def digests(sweep, tag):
    groups, count = {}, 0
    for ln in sweep.splitlines():
        if ln.startswith(tag + " "):
            f = ln.split()
            groups.setdefault("%s %sx%s" % (f[1], f[2], f[3]), hashlib.sha256()).update((ln + "\n").encode())
            count += 1
    return {k: v.hexdigest() for k, v in groups.items()}, count


def test_plans_of_the_surfaces_equal_the_parent_planners(sweep):
    golden = json.load(open(os.path.join(A.ROOT, "tests", "golden", "enc_plans_parent.json")))
    m = re.search(r"(\d+) planar tensor cases and (\d+) cases of the other sources \((\d+) taken\) printed$", sweep, flags=re.M)
    assert m and int(m.group(1)) == TENSORS and int(m.group(2)) == PARENT and 0 < int(m.group(3)) < PARENT, sweep[-1000:]  # (this tree's planner printed them)
    groups, count = digests(sweep, "P")
    assert count == PARENT and len(groups) == 25 and PARENT == 25 * golden["cases_per_group"]
    assert groups == golden["groups"]


def test_plans_of_the_planar_tensors_equal_the_parent_planners(sweep):
    golden = json.load(open(os.path.join(A.ROOT, "tests", "golden", "enc_tensor_plans_parent.json")))
    groups, count = digests(sweep, "T")
    assert count == TENSORS and len(groups) == 25 and TENSORS == 25 * golden["cases_per_group"]
    assert groups == golden["groups"]
