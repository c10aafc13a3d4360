"""The encoder's acceptance rule and ingest planner for TENSOR sources without a GPU: csrc/enc_ingest.h compiled for the host and swept
under AddressSanitizer + UndefinedBehaviorSanitizer by tools/enc_tensor_plan_check.cpp (a stand-alone program: nothing sanitized is
loaded into Python) over chroma format x size x element type x pointer offset x pitch, on synthetic addresses.  The program checks
acceptance, every refusal, and the job's addresses and contents; this file restates the rules for the record counts and the wide fact
and compares them line by line.  For every surface kind, call and route of the older sweep the program prints every member an
IngestPlan had before; their digests equal tests/golden/enc_plans_parent.json, recorded from the PARENT commit's enc_ingest.h compiled
into the same program under another namespace (the tool's -DPARENT_HEADER build, which also compares the two planners' lines): the
plans of the existing sources are what they were."""
import hashlib
import json
import os
import re

import pytest

import dsvabi as A
from sanitized_tool import build_and_run

ELEM = {0: 1, 1: 2, 2: 2, 3: 4}
CASES = 5 * 5 * 4 * 4 * 3        # formats x sizes x element types x offsets x pitches
PARENT = 5 * 5 * 5 * 12 * 4 * 3  # formats x sizes x surface kinds x (call, route) x offsets x pitches


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/enc_tensor_plan_check.cpp with the sanitizers, runs its whole sweep and returns what it printed"""
    return build_and_run("tools/enc_tensor_plan_check.cpp", tmp_path_factory.mktemp("enc_tensor_plan"))[0]


def test_every_tensor_case_of_the_sweep_holds(sweep):
    m = re.search(r"enc_tensor_plan_check: (\d+) tensor cases \((\d+) in the wide form\): acceptance, refusals, job and form hold", sweep)
    assert m, sweep[-1000:]
    assert int(m.group(1)) == CASES
    assert 0 < int(m.group(2)) < CASES  # both forms are planned


def test_record_counts_and_the_wide_fact_follow_the_rules(sweep):
    """per case: a float tensor brings one TensorInJob and no Rgb3Job, a uint8 tensor one planar Rgb3Job and no TensorInJob; wide exactly
    where the plane pointers (256 bytes + offset elements behind a 16-byte boundary), the three pitches (tight; + 1 element; rounded up
    to 256 bytes and 16 more per plane) are multiples of four elements and w of 4"""
    lines = [ln.split() for ln in sweep.splitlines() if ln.startswith("T ")]
    assert len(lines) == CASES
    seen = set()
    for f in lines:
        assert f[7] == ":"
        fmt, w, h, dtype, offset, pitch_kind = (int(v) for v in f[1:7])
        got = tuple(int(v) for v in f[8:])
        elem = ELEM[dtype]
        rb = w * elem
        pitch = rb if pitch_kind == 0 else rb + elem if pitch_kind == 1 else (rb + 255) // 256 * 256
        pitches = [pitch + (16 * k if pitch_kind == 2 else 0) for k in range(3)]
        wide = int(offset % 4 == 0 and all(p % (4 * elem) == 0 for p in pitches) and w % 4 == 0)
        assert got == (int(dtype != 0), int(dtype == 0), wide), f
        seen.add((dtype, wide))
    assert len(seen) == 4 * 2  # every element type in both forms


def test_plans_of_the_existing_sources_equal_the_parent_planners(sweep):
    golden = json.load(open(os.path.join(A.ROOT, "tests", "golden", "enc_plans_parent.json")))
    m = re.search(r"(\d+) cases of the other sources \((\d+) taken\) printed$", sweep, flags=re.M)
    assert m and int(m.group(1)) == PARENT and 0 < int(m.group(2)) < PARENT, sweep[-1000:]  # (this tree's planner printed them)
    groups, count = {}, 0
    for ln in sweep.splitlines():
        if ln.startswith("P "):
            f = ln.split()
            groups.setdefault("%s %sx%s" % (f[1], f[2], f[3]), hashlib.sha256()).update((ln + "\n").encode())
            count += 1
    assert count == PARENT and len(groups) == 25 and PARENT == 25 * golden["cases_per_group"]
    assert {k: v.hexdigest() for k, v in groups.items()} == golden["groups"]
