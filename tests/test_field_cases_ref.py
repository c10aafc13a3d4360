"""The crafted motion fields of tests/field_cases.py are what they claim, shown on the reference alone (CPU): the hook library is
the reference when nothing is queued; every picture has the labelled type, the labelled inversion bits and sub-streams of the
labelled lengths; packets stay clear of the reference's bound; two runs are equal (for the cases outside the domain of dsv_hme's
records: over two fresh processes); the reference's decoder takes every packet."""
import json
import os
import subprocess
import sys

import pytest

import dsvabi as A
import field_cases as F
import long_motion as L
from codec_run import encode_stream, frames

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hook_library_is_the_reference_when_nothing_is_queued():
    """a plain stream (six pictures, the search's own fields, scene-change detection on) through libdsv2ref_field.so, byte for byte"""
    fr = frames(176, 144, 1, 1, 6, 5)
    cfg = dict(qp=55, effort=10, gop=4)
    want = encode_stream(A.load_ref(), fr, 176, 144, A.SUBSAMP_420, **cfg)
    lib = F.load_field_ref()
    assert lib.dsv2ref_set_field(None, 0, 0, 0, 0, 0) == 0  # (dropping a field that is not there)
    got = encode_stream(lib, fr, 176, 144, A.SUBSAMP_420, **cfg)
    assert got == want
    assert any(p[5] & 1 for p in want[0] if p[5] & 4), "no P picture: the search was never called"


def test_every_field_is_legal_or_listed():
    for c in F.CASES:
        for f in F.fields_of(c):
            assert F.legal(f) == (c.family not in F.OUTSIDE), c.name
    assert {c.family for c in F.CASES if c.family in F.OUTSIDE} == set(F.OUTSIDE)


def check_case(c):
    w, h = F.GEOMS[c.geom][:2]
    pk, stats = F.reference_case(c.name)
    pics = [p for p in pk if p[5] & 4]
    types = "".join("P" if p[5] & 1 else "I" for p in pics)
    assert types == F.expected_types(c), c.name
    for p, f in zip(pics[1:], F.fields_of(c)):
        if not p[5] & 1:
            continue
        lab = F.labels(f, c.geom)
        bw, bh, inv, lengths = L.side_substream_lengths(p)
        assert (bw, bh) == F.grid(c.geom)[2:4], c.name
        assert inv == lab.inv, "%s: inversion bits %r, labelled %r" % (c.name, inv, lab.inv)
        assert lengths == [(b + 7) // 8 for b in lab.bits], "%s: sub-stream bytes %r, labelled bits %r" % (c.name, lengths, lab.bits)
    for p in pk:
        assert 4 * len(p) <= 3 * 2 * w * h, "%s: a packet of %d bytes" % (c.name, len(p))


@pytest.mark.parametrize("fg", F.FAMILIES, ids=F.family_id)
def test_small_cases_are_what_they_claim(fg):
    for c in F.family_cases(fg):
        check_case(c)
        lib = F.load_field_ref()
        again = F.encode_case(lib, F.ref_setter(lib), c)
        assert (tuple(again[0]), again[1]) == F.reference_case(c.name), c.name
        got = L.decode_packets(A.load_ref(), F.reference_case(c.name)[0])
        assert all(code in (A.DEC_OK, A.DEC_GOT_META) for code, _, _ in got), c.name
        assert sum(planes is not None for _, _, planes in got) == len(F.fields_of(c)) + 1, c.name


@pytest.mark.parametrize("c", F.CAP_CASES, ids=lambda c: c.name)
def test_cap_cases_are_what_they_claim(c):
    check_case(c)
    got = L.decode_packets(A.load_ref(), F.reference_case(c.name)[0])
    assert [code for code, _, _ in got] == [A.DEC_GOT_META, A.DEC_OK, A.DEC_OK], c.name


def test_scene_change_pairs_lie_on_both_sides():
    """do_scd = 1: of two fields a single block apart, and of one field under two ndiff one apart, the reference flips one to
    intra and keeps the other P (check_case asserts each case's types against its label)"""
    t = {c.name: "".join("P" if p[5] & 1 else "I" for p in F.reference_case(c.name)[0] if p[5] & 4) for c in F.CASES if c.family == "scene"}
    assert (t["scene-k21-ndiff80"], t["scene-k22-ndiff80"]) == ("IP", "II")
    assert (t["scene-k48-ndiff80"], t["scene-k49-ndiff80"]) == ("II", "IP")
    assert (t["scene-k20-ndiff82"], t["scene-k20-ndiff83"]) == ("IP", "II")
    for a, b in ((21, 22), (48, 49)):
        fa, fb = F.scene_field("176x144", a), F.scene_field("176x144", b)
        assert int((fa != fb).sum()) == 1, "the fields of a pair differ in one block"
    assert all(dict(c.cfg)["do_scd"] == 1 for c in F.CASES if c.family == "scene")
    assert all(F.case_cfg(c)["do_scd"] == 0 for c in F.CASES if c.family != "scene")


def test_caps_lie_on_both_sides_of_the_kernels_rule():
    """the distance of each pair from the rule, in bits: as near as the code lengths allow (vector differences come in steps of
    two bits, intra records of two, run-length codes of one: an even count cannot be -1)"""
    want = {"mv": (-2, 0), "sbim": (-2, 0), "rle": (-1, 0)}
    for which in F.CAP_MAKERS:
        below, above, far = (F.cap_margin(which, s) for s in ("below", "above", "far"))
        assert (below, above) == want[which] and far > 1000, which
        verdicts = [F.labels(F.cap_field(which, s), F.CAP_MAKERS[which][0]).verdict for s in ("below", "above", "far")]
        assert verdicts == [0, 1, 1], which
    gate = F.BY_NAME["gate-2320x1808"]
    assert F.nblocks(gate.geom) == 16385 > F.GATE_BLOCKS and F.expected_flags(gate) == 1
    f = F.fields_of(gate)[0]
    assert all((b + 40) // 8 + 8 <= F.CAP_MV for b in F.labels(f, gate.geom).bits[2:4]), "the gate case must trip on the gate alone"


def test_two_runs_of_the_cap_cases_are_equal():
    lib = F.load_field_ref()
    for c in F.CAP_CASES:
        again = F.encode_case(lib, F.ref_setter(lib), c)
        assert (tuple(again[0]), again[1]) == F.reference_case(c.name), c.name


def test_reference_is_deterministic_outside_the_domain():
    """the families whose records dsv_hme cannot store: two fresh processes and this one agree"""
    names = [c.name for c in F.CASES if c.family in F.OUTSIDE]
    assert len(names) >= 6
    runs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.join(HERE, "field_worker.py"), "ref"] + names, stdout=subprocess.PIPE, check=True, text=True)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    here = {n: F.digest(*F.reference_case(n)) for n in names}
    assert runs[0] == runs[1] == here
