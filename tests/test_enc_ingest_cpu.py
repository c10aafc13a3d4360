"""The encoder's ingest planner without a GPU: csrc/enc_ingest.h -- which surfaces the three surface calls take, and which kernels a taken
picture enters through, reading and writing what -- compiled for the host and swept under AddressSanitizer + UndefinedBehaviorSanitizer
by tools/enc_ingest_check.cpp (a stand-alone program: nothing sanitized is loaded into Python) over chroma format x encoder size x source
kind x (call, route) x pointer offset x pitch, on synthetic addresses.  The program checks acceptance, record counts, coverage, reads and
kernel forms of every case by its own interval arithmetic and states how many cases hit each row of its two tables."""
import re

import pytest

from sanitized_tool import build_and_run

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
    return build_and_run("tools/enc_ingest_check.cpp", tmp_path_factory.mktemp("enc_ingest"))[0]


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
