"""The library against the reference on the crafted motion fields of tests/field_cases.py: k_side_info (csrc/sideinfo.hip), the
sums of k_block_stats_b (csrc/hme.hip) and everything they feed, on fields a test chose -- handed to the library behind its
search by dsv2hip_seam_set_field, to the reference through the hook library.  tests/test_field_cases_ref.py shows on the
reference alone that every case is what it claims."""
import json
import os
import subprocess
import sys

import pytest

import dsvabi as A
import field_cases as F
import long_motion as L
from hipabi import bind, parse_mode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def assert_same(name, want, got):
    (wp, ws), (gp, gs) = want, got
    assert len(wp) == len(gp), "%s: %d packets, the reference has %d" % (name, len(gp), len(wp))
    for i, (a, b) in enumerate(zip(wp, gp)):
        assert len(a) == len(b), "%s packet %d (%s): %d bytes, the reference has %d" % (name, i, "P" if a[5] & 1 else "I", len(b), len(a))
        if a != b:
            d = next(k for k in range(len(a)) if a[k] != b[k])
            raise AssertionError("%s packet %d (%s) differs at byte %d of %d" % (name, i, "P" if a[5] & 1 else "I", d, len(a)))
    assert ws == gs, "%s: stats %r, the reference has %r" % (name, gs, ws)


def run_case(c):
    """packets and stats equal the reference's; the side-flag counter moves by exactly the labelled amount"""
    hip = bind(A.load_hip())
    before = hip.dsv2hip_enc_side_flag_count()
    got = F.encode_case(hip, F.hip_setter(hip), c)
    moved = hip.dsv2hip_enc_side_flag_count() - before
    assert_same(c.name, F.reference_case(c.name), got)
    assert moved == F.expected_flags(c), "%s: k_side_info handed %d pictures to the host, labelled %d" % (c.name, moved, F.expected_flags(c))


def test_seam_entry_refuses_what_it_cannot_take():
    hip = bind(A.load_hip())
    f = F.blank(4)
    assert hip.dsv2hip_seam_set_field(None, f.ctypes.data, 4, 0, 0, 4, 0) == -1
    enc = A.ENCODER()
    hip.dsv_enc_init(enc)
    assert hip.dsv2hip_seam_set_field(enc, f.ctypes.data, 0, 0, 0, 4, 0) == -1
    assert hip.dsv2hip_seam_set_field(enc, f.ctypes.data, 4, 0, 0, 4, 0) == 0
    assert hip.dsv2hip_seam_set_field(enc, None, 0, 0, 0, 0, 0) == 0  # dropped again
    hip.dsv_enc_free(enc)


def test_a_field_of_the_wrong_size_is_dropped_aloud(capfd):
    """queued on an encoder that has not coded a picture yet, so the entry cannot refuse it: the picture is coded from the search's
    own field, as the plain reference codes it, and stderr says so"""
    from codec_run import configure_encoder
    import ctypes as C
    import numpy as np
    c = F.BY_NAME["random-176x144"]
    w, h = F.GEOMS[c.geom][:2]
    ref = A.load_ref()
    want = F.encode_case(ref, lambda enc, f, ints: 0, c)  # (no field: the reference's own search)
    hip = bind(A.load_hip())
    wrong = F.blank(F.nblocks(c.geom) + 1)
    queued = []

    def setter(enc, f, ints):
        queued.append(hip.dsv2hip_seam_set_field(C.byref(enc), wrong.ctypes.data, len(wrong), *ints))
        return 0

    enc = A.ENCODER()
    configure_encoder(hip, enc, A.mk_meta(w, h, A.SUBSAMP_420), **F.case_cfg(c))
    assert hip.dsv2hip_seam_set_field(C.byref(enc), wrong.ctypes.data, len(wrong), 0, 0, 1, 0) == 0  # fresh: taken as it is
    bufs, got = (A.BUF * 4)(), []
    for fb in F.pictures(w, h, 2):
        arr = np.frombuffer(fb, dtype=np.uint8).copy()
        for i in range(hip.dsv_enc(C.byref(enc), hip.dsv_load_planar_frame(A.SUBSAMP_420, arr.ctypes.data, w, h), bufs)):
            got.append(bytes(C.string_at(bufs[i].data, bufs[i].len)))
            hip.dsv_buf_free(C.byref(bufs[i]))
    assert hip.dsv2hip_seam_set_field(C.byref(enc), wrong.ctypes.data, len(wrong), 0, 0, 1, 0) == -1  # ready: refused
    hip.dsv_enc_free(C.byref(enc))
    assert tuple(got) == tuple(want[0])
    assert "dsv2hip_seam_set_field: a field of 100 blocks was queued, the encoder has 99" in capfd.readouterr().err


@pytest.mark.parametrize("fg", F.FAMILIES, ids=F.family_id)
def test_small_cases(fg):
    for c in F.family_cases(fg):
        run_case(c)


@pytest.mark.parametrize("c", F.CAP_CASES, ids=lambda c: c.name)
def test_cap_cases(c):
    """each cap decided by the kernel on both sides: raised for -above and -far (and above the block-count gate), not for -below"""
    assert F.expected_flags(c) == (0 if c.name.endswith("-below") else 1)
    run_case(c)


# ---- the host coders on the same fields: DSV2_SIDE_FORCE_FALLBACK=1 in a child process -------------------------------------------
def chunks(names, n):
    return [names[i:i + n] for i in range(0, len(names), n)]


FALLBACK_CHUNKS = chunks([c.name for c in F.SMALL_CASES], 80) + chunks([c.name for c in F.CAP_CASES], 4)


@pytest.mark.parametrize("names", FALLBACK_CHUNKS, ids=lambda names: "%s..%s" % (names[0], names[-1]))
def test_forced_fallback_gives_the_same_packets(names):
    env = dict(os.environ, DSV2_SIDE_FORCE_FALLBACK="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "field_worker.py"), "hip"] + names, stdout=subprocess.PIPE, env=env, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    # (the forced fall-back does not move the counter: only the kernel's own verdicts do)
    assert got.pop("side_flag_count") == sum(F.expected_flags(F.BY_NAME[n]) for n in names)
    want = {n: F.digest(*F.reference_case(n)) for n in names}
    assert got == want, [n for n in names if got.get(n) != want[n]]


# ---- the decoder on the reference's packets: partial sub-masks, DC predictions and EPRM blocks by choice ----------------------------
def decode_check(names, mode):
    ref = A.load_ref()
    with parse_mode(mode) as hip:
        for n in names:
            pk = F.reference_case(n)[0]
            L.assert_decodes_equal(L.decode_packets(ref, pk), L.decode_packets(hip, pk), n)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("fg", F.FAMILIES, ids=F.family_id)
def test_decoder_on_the_references_packets(fg, mode):
    decode_check([c.name for c in F.family_cases(fg)], mode)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("c", F.CAP_CASES, ids=lambda c: c.name)
def test_decoder_on_the_references_cap_packets(c, mode):
    decode_check([c.name], mode)


# ---- lockstep steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_six_fields_in_one_step(order):
    """six encoders at 352 x 288 in one dsv2hip_enc_batch_host step, each with another field and other votes"""
    names = F.STEP_SIX if order == "listed" else F.STEP_SIX[::-1]
    hip = bind(A.load_hip())
    before = hip.dsv2hip_enc_side_flag_count()
    got = F.encode_step(hip, names)
    for n, g in zip(names, got):
        assert_same("%s in slot %d" % (n, names.index(n)), F.reference_case(n), g)
    assert hip.dsv2hip_enc_side_flag_count() == before
    assert len({F.labels(F.fields_of(F.BY_NAME[n])[0], "352x288").inv for n in names}) > 1, "the votes of the six do not differ"


def test_three_at_1080p_of_which_the_middle_one_overflows():
    hip = bind(A.load_hip())
    before = hip.dsv2hip_enc_side_flag_count()
    got = F.encode_step(hip, F.STEP_1080)
    for n, g in zip(F.STEP_1080, got):
        assert_same(n, F.reference_case(n), g)
    assert [F.expected_flags(F.BY_NAME[n]) for n in F.STEP_1080] == [0, 1, 0]
    assert hip.dsv2hip_enc_side_flag_count() - before == 1
