"""Every reference stream tests/test_gpu_enc_resize.py compares with, built here without a GPU (tests/enc_resize_cases.py): the
reference encoder runs on the oracle's planes, and each stream must meet the two conditions of a case -- its packets stay inside
the bound within which the reference is defined (edge_cases.packet_bound_holds), and I and P pictures both occur.  A broken case
shows on this machine and not on the GPU."""
import os

import pytest

import dsvabi as A
import enc_resize_cases as K

pytestmark = pytest.mark.skipif(not os.path.exists(A.REF_SO), reason="the reference library is not built")

REFS = K.every_reference()


@pytest.mark.parametrize("what,make", REFS, ids=[r[0].replace(" ", "_") for r in REFS])
def test_reference_stream_meets_both_conditions(what, make):
    packets = make()  # (ref_packets asserts both conditions)
    assert len(packets) >= K.NFR


def test_the_cases_cover_what_the_gpu_test_promises():
    assert {(c[2], c[3]) for c in K.SOURCES_420} >= {(16, 16), (18, 16), (34, 18), (48, 16)} and any(c[2] > 256 for c in K.SOURCES_420)
    assert {c[0] for c in K.FORMAT_SOURCES} == {"444", "422", "420", "411", "410"}
    assert [m[3] for m in K.MIXED] == ["plain", "half", "sized", "sized", "sized"] and K.MIXED[4][1:3] == (34, 18)
