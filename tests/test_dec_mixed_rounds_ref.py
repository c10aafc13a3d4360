"""The cases of tests/test_gpu_dec_mixed_rounds.py are what they claim -- shown on the reference alone, on the CPU, so that a green GPU
run means something.  These are conditions of the cases, not tolerances: a case that does not hold them tests less than its name says,
or compares with pictures that the reference does not define (tests/edge_cases.py: the packet bound)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dec_mixed_rounds as D
import dsvabi as A
import mixed_steps as M
from edge_cases import packet_bound_holds, stream_inverse_is_undefined

pytestmark = [pytest.mark.skipif(not os.path.exists(A.REF_SO), reason="oracle/_ref is not built (python __graft_entry__.py builds it from the reference tree)")]

BATCH_NAMES = [n for n in D.NAMES if n not in ("threads", "orphan")]


def specs_of(name):
    return list(dict.fromkeys(sp for fd in D.case(name).feeds for sp in fd.parts))


@pytest.mark.parametrize("name", D.NAMES)
def test_every_reference_packet_is_within_its_bound(name):
    for sp in specs_of(name):
        pk = M._reference(sp)[0]
        packet_bound_holds(pk, sp.w, sp.h, M.FMT[sp.fmt][0])
        assert not stream_inverse_is_undefined(sp.w, sp.h, M.FMT[sp.fmt][0], dict(sp.cfg)), "%r: the reference cannot invert a plane of it" % (sp,)
        assert len(M.picture_types(pk)) == sp.nframes and D.kind(pk[0]) == "M" and D.kind(pk[1]) == "I"  # (a closed GOP in front)


@pytest.mark.parametrize("name", ["everything", "change", "two_rounds", "key_352x288_bsx1"])
def test_the_header_reader_reads_what_the_decoder_returns(name):
    """tests/dec_mixed_rounds.py: picture_header against the frame numbers the reference decoder returns and the streams' settings"""
    for fd in D.case(name).feeds:
        at = 0
        for sp in fd.parts:
            cfg = dict(sp.cfg)
            for pk in M._reference(sp)[0]:
                if pk[5] & 4:
                    hd, res = D.picture_header(pk), D.reference(fd)[at]
                    assert res[0] == A.DEC_OK and res[1] == hd["fno"]
                    assert hd["lossless"] == int(cfg["qp"] == 100)
                    assert (hd["blk_w"], hd["blk_h"]) == tuple(2 * b if cfg.get(k) else b for b, k in
                                                              zip(A.block_geometry(sp.w, sp.h)[:2], ("block_size_override_x", "block_size_override_y")))
                at += 1


def differs_from_first(group, key):
    return any(e[key] != group[0][key] for e in group[1:])


@pytest.mark.parametrize("name,order", [("everything", o) for o in D.ORDERS] + [("small", "rotated"), ("staggered", "order"), ("damaged", "order")])
def test_steps_mix_what_a_round_need_not_share(name, order):
    """"everything" and "staggered": every step from the third on in which every decoder of the case takes part (the intra-only rows
    have twice the packets, so the last steps are theirs alone) holds I and P pictures; the other cases have three such steps at
    least.  Some step of "everything" holds all four (P, lossless) slice classes, some step of the others three ("small": two).  In some
    step the FIRST picture of the lossy P slice differs from a later one of that slice in the quantiser, in do_filter and in
    inter_sharpen, and the first of the lossy I slice in the quantiser and in do_filter -- what a kernel that reads the slice's first
    record would get wrong; both frame-number parities occur among the P pictures of one step."""
    cs = D.case(name, order)
    table = D.step_table(cs)
    if name == "staggered":  # (decoders come and go: the steps with four pictures at least)
        full = [t for t, row in enumerate(table) if sum(e["kind"] in "IP" for e in row) >= 4]
    else:
        full = [t for t, row in enumerate(table) if len(row) == len(cs.feeds)]
    assert len(full) >= 6
    both = [t for t in full if {"I", "P"} <= set(e["kind"] for e in table[t])]
    if name in ("everything", "staggered"):
        assert both == [t for t in full if t >= 2], "steps with I and P pictures: %r of %r" % (both, full)
    assert len(both) >= 3
    classes = [dict(D.slices(row)) for row in table]
    assert any(len(c) == dict(everything=4, small=2).get(name, 3) for c in classes)  # (the other cases have one lossless row, "small" none)
    assert any(2 in c and all(differs_from_first(c[2], key) for key in ("quant", "do_filter", "inter_sharpen")) for c in classes)
    assert any(0 in c and all(differs_from_first(c[0], key) for key in ("quant", "do_filter")) for c in classes)
    assert any(len(set(e["fno"] % 2 for e in row if e["kind"] == "P")) == 2 for row in table)
    assert any(len(set(e["kind"] for e in row)) >= 3 for row in table)  # (metadata beside pictures)


def test_the_staggered_schedule():
    cs = D.case("staggered")
    first = [min(t for t, step in enumerate(cs.schedule) if any(k == s for k, _ in step)) for s in range(9)]
    assert first == [0, 1, 2, 3, 4, 5, 6, 7, 1]
    last = [max(t for t, step in enumerate(cs.schedule) if any(k == s for k, _ in step)) for s in range(9)]
    assert last[1] < last[0] and last[4] < last[0]  # (1 and 4 leave early)
    ids = [[k for k, _ in step] for step in cs.schedule]
    assert all(2 not in ids[t] for t in (5, 6)) and 2 in ids[4] and 2 in ids[7]
    table = D.step_table(cs)
    before, after = next(e for e in table[4] if e["k"] == 2), next(e for e in table[7] if e["k"] == 2)
    assert after["kind"] == "P" and before["kind"] in "IP"  # (the picture behind the gap predicts from the one in front of it)
    assert all(ids[t] == sorted(ids[t], reverse=bool(t % 2)) for t in range(len(ids)))
    assert all(sorted(p for step in cs.schedule for k, p in step if k == s) == list(range(len(D.packets(fd)))) for s, fd in enumerate(cs.feeds))


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_no_two_decoders_deliver_the_same_picture_in_a_step(name):
    """(if two did, the judge would miss a swap)"""
    cs = D.case(name)
    digests = [D.digest(D.reference(fd)) for fd in cs.feeds]
    for t, step in enumerate(cs.schedule):
        seen = [digests[k][p][2] for k, p in step if p < len(digests[k]) and digests[k][p][2] is not None]
        assert len(seen) == len(set(seen)), "step %d" % t
    assert sum(d[2] is not None for dg in digests for d in dg) == sum(sp.nframes for fd in cs.feeds for sp in fd.parts)


# ---- damaged neighbours -----------------------------------------------------------------------------------------------------------
def child(k):
    code = ("import sys; sys.path.insert(0, %r)\nimport dec_mixed_rounds as D\nD.child_report(D.case('damaged').feeds[%d])\n" % (os.path.dirname(os.path.abspath(__file__)), k))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    result = [line for line in r.stdout.splitlines() if line.startswith("result ")]
    assert len(result) == 1
    return json.loads(result[0][7:]), D.refused_planes(r.stdout)


def test_the_damaged_decoders_sit_between_clean_ones():
    cs = D.case("damaged")
    hurt = sorted(k for k, fd in enumerate(cs.feeds) if fd.damage)
    assert hurt == sorted(D.DAMAGE) and len(hurt) == 2 and 0 not in hurt and hurt[1] - hurt[0] > 1 and len(cs.feeds) == 8


def test_the_reference_judges_the_damaged_packets():
    """the reference's result is a function of the damaged packets (two fresh child processes and this one agree); every damaged
    picture differs from its clean decode; the plane decoder REFUSES -- not merely misreads -- a luma and a chroma plane, in an I and
    in a P picture; pictures behind a damaged one are decoded on top of it and differ too"""
    cs = D.case("damaged")
    refused_in = set()
    for k in sorted(D.DAMAGE):
        fd = cs.feeds[k]
        (a, log_a), (b, log_b) = child(k), child(k)
        here = D.digest(D.reference(fd))
        assert a == b == here and log_a == log_b
        clean = D.digest(D.reference(fd._replace(damage=None)))
        assert [r[:2] for r in here] == [r[:2] for r in clean]  # (the reference goes on: same codes, same frame numbers)
        pk, was = D.packets(fd), D.clean_packets(fd)
        hit = [i for i in range(len(pk)) if pk[i] != was[i]]
        pics = [i for i, p in enumerate(pk) if p[5] & 4]
        assert hit == [pics[n] for n in fd.damage[1]] and {"I", "P"} <= set(D.kind(pk[i]) for i in hit)
        assert all(len(pk[i]) == len(was[i]) and pk[i][:len(pk[i]) // 2] == was[i][:len(was[i]) // 2] for i in hit)  # (the second half only)
        for i in hit:
            assert here[i][2] != clean[i][2], "decoder %d packet %d: the damage does not show" % (k, i)
        assert any(here[i][2] != clean[i][2] and D.kind(pk[i]) == "P" for i in pics if i not in hit)  # (on top of a damaged reference picture)
        assert set(log_a) <= set(hit), "planes refused in packets that are not damaged: %r" % (log_a,)
        refused_in |= {(D.kind(pk[i]), "luma" if c == 0 else "chroma") for i, planes in log_a.items() for c in planes}
    assert {("I", "luma"), ("P", "luma"), ("I", "chroma"), ("P", "chroma")} <= refused_in or \
        ({t for t, _ in refused_in} == {"I", "P"} and {c for _, c in refused_in} == {"luma", "chroma"}), refused_in


# ---- parameters change under a decoder ----------------------------------------------------------------------------------------------
def test_a_concatenation_decodes_as_its_parts():
    cs = D.case("change")
    changed = [fd for fd in cs.feeds if len(fd.parts) > 1]
    assert len(changed) == 4 and len(cs.feeds) == 6
    points = []
    for fd in changed:
        whole = D.digest(D.reference(fd))
        parts = [r for sp in fd.parts for r in D.digest(D.reference(D.feed(sp, eos=False)))]
        assert whole[:len(parts)] == parts and len(whole) == len(parts) + 1 and whole[-1][0] == A.DEC_EOS
        at, pts = 0, []
        for sp in fd.parts:
            pk = M._reference(sp)[0]
            assert [D.kind(p) for p in pk[:2]] == ["M", "I"]  # the first picture after every change is intra
            pts.append(at)
            at += len(pk)
        points.append(tuple(pts[1:]))
    assert len(set(p for pts in points for p in pts)) == sum(len(pts) for pts in points), "change points coincide: %r" % (points,)
    size, block, fmt, meta = changed
    assert [(sp.w, sp.h) for sp in size.parts] == [(176, 144), (178, 146), (176, 144)]
    hd = [D.picture_header(M._reference(sp)[0][1]) for sp in block.parts]
    assert [(h["blk_w"], h["blk_h"]) for h in hd] == [(16, 16), (32, 32), (16, 16)] and len(set((sp.w, sp.h) for sp in block.parts)) == 1
    assert [sp.fmt for sp in fmt.parts] == ["420", "422"]
    assert [dict(sp.meta)["inter_sharpen"] for sp in meta.parts] == [0, 1] and len(set(dict(sp.meta)["fps"] for sp in meta.parts)) == 2
    # the decoders are mid-GOP when a neighbour changes: a P picture shares the step of every first picture after a change
    table = D.step_table(cs)
    for fd, pts in zip(changed, points):
        k = cs.feeds.index(fd)
        for p in pts:
            row = next(r for r in table if any(e["k"] == k and e["packet"] == p + 1 for e in r))
            assert any(e["kind"] == "P" for e in row if e["k"] != k), "decoder %d packet %d" % (k, p + 1)


def test_two_rounds_of_one_size():
    cs = D.case("two_rounds")
    blocks = []
    for fd in cs.feeds:
        assert D.geometry(fd) == (M.W, M.H, "420")
        hds = [D.picture_header(p) for p in D.packets(fd) if p[5] & 4]
        assert len(set((h["blk_w"], h["blk_h"]) for h in hds)) == 1
        blocks.append((hds[0]["blk_w"], hds[0]["blk_h"]))
    assert blocks == [(16, 16), (32, 32)] * 3  # interleaved slot by slot
    assert any({"I", "P"} <= set(e["kind"] for e in row if blocks[e["k"]] == b) for row in D.step_table(cs) for b in set(blocks))


def test_the_orphan_fails_alone():
    """the reference: metadata, DSV_DEC_ERROR for the P picture without its reference picture, then the stream's pictures as ever"""
    cs = D.case("orphan")
    fd = cs.feeds[2]
    got, whole = D.digest(D.reference(fd)), D.digest(D.reference(fd._replace(pick=None)))
    assert [D.kind(p) for p in D.packets(fd)[:4]] == ["M", "P", "I", "P"]
    assert got[:2] == [[A.DEC_GOT_META, None, None], [A.DEC_ERROR, None, None]] and got[2:] == whole[1:12]
    assert [D.kind(D.packets(f)[1]) for f in cs.feeds] == ["I", "I", "P", "I", "I", "I"]  # (step 1: the refused picture between five others)


def test_each_way_out_has_a_stream_of_its_own():
    cs = D.case("ways")
    assert len(cs.feeds) == len(set(cs.feeds)) == len(set(cs.opts)) == 10
    assert sorted(o.way[0] for o in cs.opts) == ["frame"] * 3 + ["packed"] + ["surface"] * 6
    kinds = ["".join(D.kind(p) for p in D.packets(fd)) for fd in cs.feeds]
    assert all("I" in k for k in kinds) and sum("P" in k for k in kinds) >= 5  # (rows 3, 4, 8, 9 are intra only, row 5 is I I)
    for k, o in enumerate(cs.opts):
        if o.draw:
            assert "P" in kinds[k] and not np.array_equal(D.reference(cs.feeds[k], o.draw)[2][2][0], D.reference(cs.feeds[k])[2][2][0])
