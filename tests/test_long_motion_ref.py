"""Long motion on the CPU (tests/long_motion.py): oracle/orc_hme.c equals the reference's dsv_hme on every case, and the cases
are what they claim -- shown on the reference alone.  Those are conditions of the inputs, not tolerances: a case that misses one
tests less than its name says, and is mended by changing the scene."""
import os

import numpy as np
import pytest

import dsvabi as A
import long_motion as L
import mixed_steps as M
from edge_cases import packet_bound_holds
from hme_common import assert_fields_equal

pytestmark = pytest.mark.skipif(not os.path.exists(A.REF_SO), reason="oracle/_ref not built")

stage_cases = pytest.mark.parametrize("case", L.STAGE_CASES, ids=[L.case_id(c) for c in L.STAGE_CASES])


@stage_cases
def test_oracle_matches_reference(case):
    ref, orc = A.load_ref(), A.load_oracle()
    want, sums_r = L.reference_result(case)
    sc = L.scene(ref, case)
    got, ipct_o, scb_o, err_o = sc.run_oracle(orc, case.quant, case.effort, case.skip)
    for l in range(sc.levels, -1, -1):
        assert_fields_equal(want[l], got[l], "level %d" % l)
    assert sums_r == (ipct_o, scb_o, err_o)


def stats_of(case):
    w, h, subsamp, blk = L.geometry(case.geom)
    meta = A.mk_meta(w, h, subsamp)
    return L.field_stats(L.reference_result(case)[0][0], A.mk_params(meta, w, h, 1, blk=blk), w, h, case.pan)


@stage_cases
def test_the_case_has_long_and_off_picture_vectors(case):
    st = stats_of(case)
    assert overflows(case) == 0, "find_inliers overflows: the reference is undefined on this case"
    assert st.ge16 >= 0.10, "%.0f %% of the inter blocks have a component of 16 px or more" % (100 * st.ge16)
    assert st.off_picture >= 1, "no block is predicted from more than 16 px outside the picture"
    if case.prev == "long" and case.pan in L.FAST_PANS:
        assert st.ge32 >= 0.50, "%.0f %% of the inter blocks have a component of 32 px or more" % (100 * st.ge32)
    if case.skip == 8:
        assert st.band_skips >= 1, "no block of the static band is skipped"


def test_the_cases_cover_what_they_name():
    cases = L.STAGE_CASES
    for name in L.GEOMETRIES:
        mine = [c for c in cases if c.geom == name]
        assert set(c.pan for c in mine) == set(L.PANS) and set(c.prev for c in mine) == set(L.PREV_KINDS)
        assert set((c.effort, c.quant, c.skip) for c in mine) == set(L.CONFIGS), name
    assert set(c.geom for c in cases) == set(L.GEOMETRIES) | set(L.FULL_SIZES)
    assert all(any(c.pan == p and c.prev == "long" for c in cases) for p in L.FAST_PANS)
    assert set(c.geom for c in L.ALT_FORM_CASES) == {"352x288", "352x288-b32x32"} and set(L.BMC_CASES) <= set(cases)
    # the forced block sizes arrive in the parameters
    for name, bw, bh in (("352x288-b32x16", 32, 16), ("352x288-b32x32", 32, 32), ("352x288-b16x32", 16, 32), ("336x280-b32x16", 32, 16)):
        sc = L.scene(A.load_ref(), next(c for c in cases if c.geom == name))
        assert (sc.params.blk_w, sc.params.blk_h) == (bw, bh) and sc.nb == len(L.reference_result(next(c for c in cases if c.geom == name))[0][0])
    assert L.scene(A.load_ref(), next(c for c in cases if c.geom == "178x146")).levels == 3


def test_the_limit_field_is_invalid_for_neighbours():
    """a "limit" vector keeps its own block inside the padded picture and takes the neighbours nearer to the border out of it"""
    for name in ("352x288", "352x288-b32x32", "336x280-b32x16", "178x146"):
        w, h, subsamp, blk = L.geometry(name)
        params = A.mk_params(A.mk_meta(w, h, subsamp), w, h, 1, blk=blk)
        bx, by = L.block_origins(params)
        bw, bh = L.block_dims(params, w, h)
        nbv, nbh = params.nblocks_v, params.nblocks_h

        def inside(vx, vy):  # every block moved by (vx, vy): the whole quarter-pel footprint within the 32-pixel border
            px, py = 4 * bx + vx, 4 * by + vy
            return (px >= -4 * A.BORDER) & (py >= -4 * A.BORDER) & (px + 4 * bw <= 4 * (w + A.BORDER)) & (py + 4 * bh <= 4 * (h + A.BORDER))

        def invalid_share(m):  # of the (block, neighbour) pairs: the neighbour's vector on the block itself
            x, y = m["x"].astype(np.int32), m["y"].astype(np.int32)
            assert np.all(inside(x, y))
            shares = []
            for dy, dx in ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)):
                nx, ny = np.roll(x.reshape(nbv, nbh), (dy, dx), (0, 1)).ravel(), np.roll(y.reshape(nbv, nbh), (dy, dx), (0, 1)).ravel()
                shares.append(np.mean(~inside(nx, ny)))
            return float(np.mean(shares))
        limit = L.prev_field("limit", params, w, h, (24, 0), 5)
        # a border zone covers over half of either axis at these sizes, and three of a block's eight neighbours lie nearer to the border
        assert invalid_share(limit) > 0.25, name
        assert invalid_share(L.prev_field("long", params, w, h, (24, 0), 5)) < 0.05, name
        assert max(np.abs(limit["x"]).max(), np.abs(limit["y"]).max()) <= 4 * L.LIMIT_REACH


def overflows(case, keep=True):
    w, h, subsamp, blk = L.geometry(case.geom)
    p = A.mk_params(A.mk_meta(w, h, subsamp), w, h, 1, blk=blk)
    fields = (L.reference_result if keep else L.reference_result.__wrapped__)(case)[0]
    return L.inlier_sum_overflows(fields, p.nblocks_h, p.nblocks_v)


def test_the_full_range_limit_field_leaves_the_reference_undefined():
    """why "limit" stops at LIMIT_REACH: with either extreme for every block the parent vectors lie up to 400 pixels apart and
    find_inliers' sum of squares overflows `int` -- not a parity case (tests/long_motion.py: inlier_sum_overflows)"""
    full = [c._replace(prev="limit-full") for c in L.STAGE_CASES if c.prev == "limit" and c.geom in ("352x288", "178x146")]
    assert sum(overflows(c, keep=False) > 0 for c in full) >= len(full) // 2


def test_the_reference_is_deterministic():
    for case in L.STAGE_CASES:
        first, sums = L.reference_result(case)
        ref = A.load_ref()
        again, ipct, scb, aerr = L.scene(ref, case).run_reference(ref, case.quant, case.effort, case.skip)
        for l in range(len(first)):
            assert_fields_equal(first[l], again[l], "%s level %d" % (L.case_id(case), l))
        assert sums == (ipct, scb, aerr)


# ---- whole streams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", L.STREAMS, ids=[L.stream_id(s) for s in L.STREAMS])
def test_stream_is_defined_and_has_its_picture_types(stream):
    pk, stats = L.reference_stream(stream)
    packet_bound_holds(pk, stream.w, stream.h, A.SUBSAMP_420)
    types = "".join(M.picture_types(pk))
    assert types == (L.PICTURE_TYPES[stream.vel] if stream.scd else "IPPPPPPP")
    assert len(L.reference_decode(stream)) == len(pk)
    assert [c for c, _, _ in L.reference_decode(stream)].count(A.DEC_OK) == L.STREAM_FRAMES


def test_no_two_streams_share_a_picture_packet():
    """(a stream and its twin without scene-change detection begin alike, and in the lossless setting come together again)"""
    seen = {}
    for s in L.STREAMS:
        for p in L.reference_stream(s)[0]:
            if p[5] & 4:
                assert seen.setdefault(p, s)._replace(scd=s.scd) == s, "%s and %s" % (L.stream_id(seen[p]), L.stream_id(s))


# ---- the side-information coder's overflow ------------------------------------------------------------------------------------
def test_a_motion_substream_outgrows_the_side_information_image():
    """read from the reference's packets: in a P picture of the jittered 1440p stream the x or y vector sub-stream is longer than
    the image csrc/sideinfo.hip gives it, so the kernel's own overflow decision runs; the packets stay inside 3/4 of their bound"""
    pk, stats = L.reference_jitter_stream()
    packet_bound_holds(pk, L.SIDE_W, L.SIDE_H, A.SUBSAMP_420)
    assert "".join(M.picture_types(pk)) == "I" + "P" * (L.SIDE_FRAMES - 1)
    lengths = [L.motion_substream_lengths(p) for p in pk if p[5] & 4 and p[5] & 1]
    assert all((bw, bh) == (16, 16) for bw, bh, _ in lengths)
    for bw, bh, sub in lengths:
        assert 0 < sum(sub) < len(pk[-1]) and all(n >= 0 for n in sub)
    assert all(max(sub[1], sub[2]) > L.SIDE_MV_CAP for _, _, sub in lengths), lengths
