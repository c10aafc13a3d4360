"""The cases of tests/test_gpu_enc_mixed_steps.py are what they claim -- shown on the reference encoder alone, on the CPU.  These
are conditions of the cases, not tolerances: a case that does not hold them tests less than its name says, or compares with
packets that the reference does not define (tests/edge_cases.py: the packet bound)."""
import os

import pytest

import dsvabi as A
import mixed_steps as M
from edge_cases import packet_bound_holds, stream_inverse_is_undefined

pytestmark = [pytest.mark.skipif(not os.path.exists(A.REF_SO), reason="oracle/_ref is not built (python __graft_entry__.py builds it from the reference tree)")]

CASES = M.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_stream_is_defined_and_no_two_are_alike(name):
    streams, _ = CASES[name]
    packets = []
    for s, sp in enumerate(streams):
        pk, stats = M._reference(sp)
        packet_bound_holds(pk, sp.w, sp.h, M.FMT[sp.fmt][0])
        assert not stream_inverse_is_undefined(sp.w, sp.h, M.FMT[sp.fmt][0], dict(sp.cfg)), "stream %d: the reference cannot invert a plane of it" % s
        assert len(M.picture_types(pk)) == sp.nframes
        packets.append(pk)
    for a in range(len(streams)):
        for b in range(a):  # (a slot mix-up between two streams with the same packets would be invisible)
            assert not set(p for p in packets[a] if p[5] & 4) & set(p for p in packets[b] if p[5] & 4), "streams %d and %d share a picture packet" % (b, a)


def test_the_table_has_every_value_and_no_row_twice():
    rows = [M.row(s) for s in range(M.NROWS)]
    assert len(set(tuple(sorted(c.items())) + tuple(sorted(m.items())) for c, m in rows)) == M.NROWS
    for key, vals in (("qp", M.QP), ("effort", M.EFFORT), ("rc_mode", M.RC), ("gop", M.GOP), ("skip_block_thresh", M.SKIP), ("do_inter_filter", M.INTER_FILTER),
                      ("do_intra_filter", (0, 1)), ("do_temporal_aq", (0, 1)), ("do_dark_intra_boost", (0, 1)), ("do_scd", (0, 1)),
                      ("variable_i_interval", (0, 1)), ("scene_change_pct", M.SCENE_PCT), ("intra_pct_thresh", M.INTRA_PCT)):
        assert set(c[key] for c, _ in rows) == set(vals), key
    assert set(m["fps"] for _, m in rows) == set(M.FPS) and set(m["inter_sharpen"] for _, m in rows) == {0, 1}
    assert sum(c["qp"] == 100 for c, _ in rows) >= 2 and len(M.CUTS) >= 2
    for name in ("small", "alternating") + tuple("key_" + k for k in M.KEY_CASES):  # the small cases still mix the classes of options
        cfgs = [dict(sp.cfg) for sp in CASES[name][0]]
        for key in ("qp", "effort", "gop", "rc_mode", "do_inter_filter", "do_intra_filter", "skip_block_thresh"):
            assert len(set(c[key] for c in cfgs)) >= 2, (name, key)


def steps_of(name):
    """the lockstep steps of a case, in order: [(stream, type, lossless)] each"""
    streams, sched = CASES[name]
    flat = [ids for groups in sched for ids in groups]
    per = M.types_per_step(streams, flat)
    return [st for st in per if st]


@pytest.mark.parametrize("name", ["staggered", "everything"])
def test_every_step_from_the_third_on_mixes_intra_and_inter(name):
    for t, st in enumerate(steps_of(name)):
        if t >= 2:
            assert {"I", "P"} <= set(ty for _, ty, _ in st), "step %d: %r" % (t, st)


@pytest.mark.parametrize("name", ["everything", "key_444"])
def test_a_step_holds_all_four_slice_classes(name):
    assert any(len(set((ty, ll) for _, ty, ll in st)) == 4 for st in steps_of(name))


def test_the_key_cases_mix_slice_classes():
    for k in M.KEY_CASES:
        assert any(len(set((ty, ll) for _, ty, ll in st)) >= 3 for st in steps_of("key_" + k)), k


def test_the_cut_frames_arrive_as_P_and_leave_as_intra():
    """the late intra analysis: without its cut the stream's picture at that index is P (so the search ran on it), with the cut it
    is coded intra"""
    cuts = list(dict.fromkeys(sp for streams, _ in CASES.values() for sp in streams if sp.cut is not None))
    for sp in cuts:
        assert M.picture_types(M._reference(sp._replace(cut=None))[0])[sp.cut] == "P", "%r: frame %d is no P picture" % (sp, sp.cut)
        assert M.picture_types(M._reference(sp)[0])[sp.cut] == "I", "%r: the cut at frame %d did not flip the picture" % (sp, sp.cut)
    assert set(dict(sp.cfg)["qp"] == 100 for sp in cuts) == {False, True}
    for name in ("everything", "alternating", "regrouping", "threads"):
        assert any(sp.cut is not None for sp in CASES[name][0])
    assert sum(sp.cut is not None for sp in CASES["everything"][0]) >= 2


def test_the_abr_quantiser_moves():
    """the search of a P picture is given the quantiser of the picture before it (prev_quant): in the ABR row that differs between
    two P pictures, and from what the same stream gets under CRF"""
    abr = M.table_stream(M.ABR_ROW)
    cfg = dict(abr.cfg)
    assert cfg["rc_mode"] == 1
    twin = abr._replace(cfg=tuple(sorted(dict(cfg, rc_mode=0).items())))
    types = M.picture_types(M._reference(abr)[0])
    q, qt = M.reference_quants(abr), M.reference_quants(twin)
    searched = [q[t - 1] for t in range(1, len(types)) if types[t] == "P"]
    assert len(set(searched)) >= 2, "every P picture of the ABR row is searched with the same quantiser: %r" % (q,)
    assert q != qt
    sizes = lambda sp: [len(p) for p in M._reference(sp)[0] if p[5] & 1]
    assert sizes(abr) != sizes(twin) and M._reference(abr)[1] != M._reference(twin)[1]


def test_the_staggered_schedule():
    streams, sched = M.staggered()
    first = [min(t for t, ids in enumerate(sched) if s in ids) for s in range(8)]
    assert first == list(range(8))
    assert [streams[s].nframes for s in (1, 4)] == [4, 4]
    assert all(2 not in sched[t] for t in (5, 6)) and 2 in sched[4] and 2 in sched[7]
    assert all(dict(sp.cfg)["gop"] == 3 for sp in streams) and streams[8].lie
    # frame-number parity (temporal_mc) differs within the steps
    pos, mixed = [0] * 9, 0
    for ids in sched:
        mixed += len(set(pos[s] % 2 for s in ids)) == 2
        for s in ids:
            pos[s] += 1
    assert mixed >= 8


def test_regrouping_moves_encoders_between_groups():
    _, sched = M.regrouping()
    assert all(sorted(a + b) == list(range(12)) for a, b in sched)
    assert all(set(sched[t][0]) != set(sched[t + 2][0]) and set(sched[t][0]) & set(sched[t + 2][0]) for t in range(0, len(sched) - 2, 2))
