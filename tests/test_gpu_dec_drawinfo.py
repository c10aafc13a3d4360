"""DSV_DECODER.draw_info: the overlay the decoder draws on the luma of the pictures it hands out (block grid, skip / stable /
maintain dashes, motion vectors, intra sub-block marks; dsv_decoder.c:240-350, :555-561) must equal the reference's, picture for
picture -- in single calls, in lockstep batches that mix drawn and undrawn decoders, with either parser, with -out420p and on
damaged input -- and must never reach the picture the next P picture predicts from.

The one documented difference: the reference stores the intra marks without a bounds check, which in a clipped last block row /
column lands outside the luma plane; the product drops such a mark.  Mode bit 4 is therefore compared with the reference on
block-aligned geometries only and checked on the product alone on clipped ones."""
import numpy as np
import pytest

import dsvabi as A
from dec_out import batch_decode, check, decode, pictures, stream
from hipabi import bind

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def same(want, got, planes=(0, 1, 2)):
    assert len(want) == len(got)
    for (fa, *pa), (fb, *pb) in zip(want, got):
        assert fa == fb
        for c in planes:
            assert np.array_equal(pa[c], pb[c]), "frame %d plane %d differs in %d samples" % (fa, c, int(np.sum(pa[c] != pb[c])))


def differs(a, b):
    return any(not np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def every_mode_equals_reference(ref, hip, w, h, packets, npics):
    bw, bh, _, _ = A.block_geometry(w, h)
    assert w % bw == 0 and h % bh == 0  # block-aligned: the reference's unchecked intra marks stay inside the luma plane
    want = {m: pictures(decode(ref, packets, m)) for m in range(9)}
    assert len(want[0]) == npics
    # the material shows dashes, vectors and intra marks (else equality under those modes would say nothing about them)
    assert differs(want[8], want[0])
    for m in (1, 2, 4):
        assert differs(want[m], want[8]), "mode %d draws nothing beyond the grid on this stream" % m
    for m in range(1, 9):
        same(want[m], pictures(decode(hip, packets, m)))


@pytest.mark.parametrize("w,h,nfr,gop", [(352, 288, 9, 4), (1280, 720, 3, 48)])
def test_every_mode_block_aligned(w, h, nfr, gop):
    every_mode_equals_reference(A.load_ref(), A.load_hip(), w, h, stream(w, h, "420", nfr, gop), nfr)


def test_vectors_and_dashes_keep_the_serial_order():
    """Mode 3: a vector drawn by an earlier block loses to a later block's dash zero pixel; the block's own vector (it starts on
    the dash's centre) and every later block's vector win."""
    ref, hip = A.load_ref(), A.load_hip()
    w, h = 352, 288
    packets = stream(w, h, "420", 9, 4)
    bw, bh, nbh, nbv = A.block_geometry(w, h)
    plain, m1, m2, m3 = (pictures(decode(ref, packets, m)) for m in (0, 1, 2, 3))
    lost = won = 0
    cy, cx = np.meshgrid(np.arange(nbv) * bh + bh // 2, np.arange(nbh) * bw + bw // 2, indexing="ij")
    for p0, p1, p2, p3 in zip(plain, m1, m2, m3):
        # a dash zero pixel that survived where a vector passes (the undrawn picture is not 255 there: the vector made it so)
        lost += int(np.sum((p3[1] == 0) & (p2[1] == 255) & (p0[1] != 255)))
        # a dash centre (0 under mode 1, not 0 undrawn) that a vector overwrote
        won += int(np.sum((p1[1][cy, cx] == 0) & (p0[1][cy, cx] != 0) & (p3[1][cy, cx] == 255)))
    assert lost > 0, "no vector crosses a later block's dash in this stream"
    assert won > 0, "no dash centre is overwritten by a vector in this stream"
    same(m3, pictures(decode(hip, packets, 3)))


def test_prediction_is_not_drawn_on():
    """The overlay lands in the picture handed out only: P pictures predicted from drawn-on pictures equal the reference's, with
    draw_info constant and toggled from packet to packet on one decoder."""
    ref, hip = A.load_ref(), A.load_hip()
    packets = stream(1280, 720, "420", 3, 48)
    want = pictures(decode(ref, packets, 7))
    assert len(want) == 3
    same(want, pictures(decode(hip, packets, 7)))
    for toggle in (lambda k: 7 * (k & 1), lambda k: 7 * (~k & 1)):
        want = pictures(decode(ref, packets, toggle))
        same(want, pictures(decode(hip, packets, toggle)))
    # and the toggle is seen: exactly the pictures of the odd packets are drawn on
    plain = [r for r in decode(ref, packets, 0) if r[2] is not None]
    got = [(k, r) for k, r in enumerate(decode(hip, packets, lambda k: 7 * (k & 1))) if r[2] is not None]
    assert len(got) == 3
    for (k, g), p in zip(got, plain):
        assert np.array_equal(g[2][0], p[2][0]) == (k % 2 == 0)


@pytest.mark.parametrize("w,h,fmt,nfr", [(354, 290, "420", 3), (354, 290, "444", 3), (1920, 1080, "420", 2)])
def test_clipped_geometry(w, h, fmt, nfr):
    ref, hip = A.load_ref(), A.load_hip()
    packets = stream(w, h, fmt, nfr, 48)
    bw, bh, nbh, nbv = A.block_geometry(w, h)
    assert w % bw or h % bh
    for m in (1, 2, 3, 8):  # every store of these modes is bounds-checked in the reference
        same(pictures(decode(ref, packets, m)), pictures(decode(hip, packets, m)))
    # mode 7 on the product alone: mode 3 plus intra marks at in-plane positions only, chroma untouched
    plain, m3, m7 = (pictures(decode(hip, packets, m)) for m in (0, 3, 7))
    marks = np.zeros((h, w), dtype=bool)
    ys = [j * bh + q * bh // 4 for j in range(nbv) for q in (1, 3)]
    xs = [i * bw + q * bw // 4 for i in range(nbh) for q in (1, 3)]
    marks[np.ix_([y for y in ys if y < h], [x for x in xs if x < w])] = True
    assert len(m7) == nfr
    for p0, p3, p7 in zip(plain, m3, m7):
        assert p0[0] == p3[0] == p7[0]
        assert np.array_equal(p7[1][~marks], p3[1][~marks])
        assert np.all((p7[1][marks] == 255) | (p7[1][marks] == p3[1][marks]))
        assert np.array_equal(p7[2], p0[2]) and np.array_equal(p7[3], p0[3])


def test_batch_mixes_drawn_and_undrawn_decoders():
    """One lockstep step sequence over four decoders: CIF mode 7, CIF undrawn, CIF mode 2 and (a second geometry) 720p mode 5."""
    ref, hip = A.load_ref(), A.load_hip()
    bind(hip)
    cif, hd = stream(352, 288, "420", 9, 4), stream(1280, 720, "420", 3, 48)
    streams, modes = [cif, cif, cif, hd], [7, 0, 2, 5]
    got = batch_decode(hip, streams, modes)
    for pk, m, g in zip(streams, modes, got):
        check(pictures(decode(ref, pk, m)), g)
    check(pictures(decode(ref, cif, 0)), got[1])
    assert differs(got[0], got[1]) and differs(got[2], got[1])


def test_every_mode_with_the_device_parser():
    ref, hip = A.load_ref(), bind(A.load_hip())
    try:
        assert hip.dsv2hip_dec_set_parse_mode(2) == 2
        every_mode_equals_reference(ref, hip, 352, 288, stream(352, 288, "420", 9, 4), 9)
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)


def test_out420p_draws_on_the_delivered_luma_only():
    ref, hip = A.load_ref(), A.load_hip()
    packets = stream(354, 290, "444", 3, 48)
    want = pictures(decode(ref, packets, 3))
    got = pictures(decode(hip, packets, 3, out420p=True))
    undrawn = pictures(decode(hip, packets, 0, out420p=True))
    same(want, got, planes=(0,))
    same(undrawn, got, planes=(1, 2))
    assert got[0][2].shape == (145, 177) and differs(got, undrawn)


def test_damaged_input_with_the_overlay_on():
    """Picture packets cut short at fixed fractions of their length, decoded with draw_info = 7: the reference's return codes,
    and its pictures wherever both return one (block-aligned geometry: the reference's own stores stay in bounds).  The reference
    reads a cut plane section to the length its header names, past the buffer's stated length: each buffer owns that many zeroed
    bytes behind the cut, or what the reference decodes is whatever the heap holds there -- often the tail of the uncut packet that
    an earlier test freed at the same address, and then a whole picture where the library, which stops at the stated length, has
    a damaged one."""
    ref, hip = A.load_ref(), A.load_hip()
    ref.dsv_set_log_level(0)  # the reference reports every damaged plane on stderr
    packets = stream(352, 288, "420", 9, 4)
    compared = 0
    for num in (4, 5, 6, 7):  # eighths of the packet kept: the cut lands in the plane sections
        cut = [pk[:len(pk) * num // 8] if len(pk) > 400 else pk for pk in packets]
        room = [len(pk) - len(c) for pk, c in zip(packets, cut)]
        want, got = decode(ref, cut, 7, room=room), decode(hip, cut, 7, room=room)
        assert [r[0] for r in want] == [r[0] for r in got]
        for (_, fw, pw), (_, fg, pg) in zip(want, got):
            if pw is not None and pg is not None:
                assert fw == fg
                for c in range(3):
                    assert np.array_equal(pw[c], pg[c])
                compared += 1
    assert compared > 0
