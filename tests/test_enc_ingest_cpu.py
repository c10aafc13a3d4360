"""The encoder's ingest planner without a GPU: csrc/enc_ingest.h -- which surfaces the three surface calls take, and which kernels a taken
picture enters through, reading and writing what -- compiled for the host and swept under AddressSanitizer + UndefinedBehaviorSanitizer
by tools/enc_ingest_check.cpp (a stand-alone program: nothing sanitized is loaded into Python) over chroma format x encoder size x source
kind x (call, route) x pointer offset x pitch, on synthetic addresses.  The program checks acceptance, record counts, coverage, reads and
kernel forms of every case by its own interval arithmetic and states how many cases hit each row of its two tables."""
import os
import re
import subprocess

import pytest

import dsvabi as A

HIPCC = "/opt/rocm/bin/hipcc"
# 12 ways in: the plain call; the scaled call without a scale and at a half, a quarter, an eighth; the sized call at the encoder's own size, from
# one column more, 3 : 2 and 8 : 1, and with the three scale values
WAYS = 1 + 4 + 7
KINDS = 5  # planar, semiplanar, four-byte RGB, three-byte RGB, planar RGB
# (the two YUV kinds in 6 formats -- the five and UYVY --, the three RGB kinds in the five) x ways x 5 sizes x 4 offsets x 3 pitches
CASES = (2 * 6 + 3 * 5) * WAYS * 5 * 4 * 3
COUNT_ROWS = 11  # kind x route -> records: 5 plain, 3 reduced, 3 sized
TABLE_ROWS = COUNT_ROWS + WAYS * KINDS


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/enc_ingest_check.cpp with the sanitizers, runs its whole sweep and returns what it printed"""
    exe = str(tmp_path_factory.mktemp("enc_ingest") / "enc_ingest_check")
    # (host code only, and the sanitizers named for the host side alone: nothing sanitized is ever built for the GPU)
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-I", os.path.join(A.ROOT, "digital-subband-video-2_amd", "csrc"), os.path.join(A.ROOT, "tools", "enc_ingest_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    return r.stdout


def test_every_case_of_the_sweep_holds(sweep):
    m = re.search(r"enc_ingest_check: (\d+) cases, (\d+) of them taken: acceptance, counts, coverage, reads and form hold", sweep)
    assert m, sweep[-1000:]
    assert int(m.group(1)) == CASES
    assert 0 < int(m.group(2)) < CASES


def test_every_row_of_both_tables_is_hit(sweep):
    rows = re.findall(r"^\s+(\d+) cases  (\S.*)$", sweep, flags=re.M)
    assert len(rows) == TABLE_ROWS
    print(sweep)
    for hits, name in rows:
        assert 0 < int(hits) < CASES, name
