"""Long motion on the GPU (tests/long_motion.py: the cases; tests/test_long_motion_ref.py: they are what they claim): the library's
motion search against the reference's where the vectors pass +-31 px, candidates point off the padded picture and the refinement
stops at its border -- the search's stage call in its default and its alternative forms, prediction and reconstruction with such
vectors, and whole streams of panning pictures through the plain API, the lockstep encode engine and the decoder's three parse
modes.  Every assertion is equality with the reference."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dsvabi as A
import long_motion as L
import mixed_steps as M
from codec_run import encode_stream
from hme_common import assert_fields_equal
from hipabi import PARSE_IDS, bind, parse_mode
from test_oracle_bmc import clone

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def check_stage(hip, case):
    want, sums_r = L.reference_result(case)
    sc = L.scene(A.load_ref(), case)
    got, ipct_h, scb_h, err_h = sc.run_reference(hip, case.quant, case.effort, case.skip)  # same call, the product library
    for l in range(sc.levels, -1, -1):
        assert_fields_equal(want[l], got[l], "level %d" % l)
    assert sums_r == (ipct_h, scb_h, err_h)


@pytest.mark.parametrize("case", L.STAGE_CASES, ids=[L.case_id(c) for c in L.STAGE_CASES])
def test_hme_matches_reference(case):
    check_stage(A.load_hip(), case)


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import dsvabi as A
import long_motion as L
import test_gpu_long_motion as T
hip = A.load_hip()
bad = []
for c in L.ALT_FORM_CASES:
    try:
        T.check_stage(hip, c)
    except AssertionError as e:
        bad.append("%%s: %%s" %% (L.case_id(c), e))
print("checked %%d" %% len(L.ALT_FORM_CASES))
print("\n".join(bad))
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("env_extra", [{"DSV2_HME_FAST": "0"}, {"DSV2_HME_SPLIT": "0"}, {"DSV2_HME_SPLIT": "1"}],
                         ids=["general-routine", "level0-in-place", "level0-split"])
def test_alternative_forms_match_reference(env_extra):
    """the 352 x 288 cases with 16 x 16 and with 32 x 32 blocks in a process where the search runs its other form (the switches are
    read when the library loads): the general block routine at every level, and each of the two forms of level 0"""
    r = subprocess.run([sys.executable, "-c", _CHILD % os.path.dirname(os.path.abspath(__file__))], env=dict(os.environ, **env_extra),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "checked %d" % len(L.ALT_FORM_CASES) in r.stdout


# ---- prediction and reconstruction with these vectors -----------------------------------------------------------------------
def check_bmc(sc, mvs, q, do_filter, lossless=0):
    """tests/test_gpu_bmc.py's comparison on the scene's own pictures"""
    ref, hip = A.load_ref(), A.load_hip()
    w, h, subsamp = sc.w, sc.h, sc.subsamp
    params = A.mk_params(sc.meta, w, h, 1, lossless, temporal_mc=sc.params.temporal_mc,
                         blk=(sc.params.blk_w, sc.params.blk_h, sc.params.nblocks_h, sc.params.nblocks_v))
    mvp = C.cast(mvs.ctypes.data, C.POINTER(A.MV))
    refframe, src = sc.ref0, sc.src0  # (both extended by the Scene)

    pred_r, resd_r = A.HostFrame(subsamp, w, h), clone(src)
    pred_h, resd_h = A.HostFrame(subsamp, w, h), clone(src)
    ref.dsv_sub_pred(mvp, C.byref(params), pred_r.ptr(), resd_r.ptr(), refframe.ptr())
    hip.dsv_sub_pred(mvp, C.byref(params), pred_h.ptr(), resd_h.ptr(), refframe.ptr())
    for c in range(3):
        assert np.array_equal(pred_r.full[c], pred_h.full[c]), "prediction plane %d" % c
        assert np.array_equal(resd_r.full[c], resd_h.full[c]), "residual plane %d" % c

    fm = A.FMETA()
    fm.params = C.pointer(params)
    fm.isP = 1
    ref.dsv_add_res(mvp, C.byref(fm), q, resd_r.ptr(), pred_r.ptr(), do_filter)
    hip.dsv_add_res(mvp, C.byref(fm), q, resd_h.ptr(), pred_h.ptr(), do_filter)
    for c in range(3):
        assert np.array_equal(resd_r.full[c], resd_h.full[c]), "add_res plane %d" % c

    resd = clone(sc.ogr0)
    out_r, out_h = A.HostFrame(subsamp, w, h), A.HostFrame(subsamp, w, h)
    ref.dsv_add_pred(mvp, C.byref(fm), q, resd.ptr(), out_r.ptr(), refframe.ptr(), do_filter)
    hip.dsv_add_pred(mvp, C.byref(fm), q, resd.ptr(), out_h.ptr(), refframe.ptr(), do_filter)
    for c in range(3):
        assert np.array_equal(out_r.full[c], out_h.full[c]), "add_pred plane %d" % c


@pytest.mark.parametrize("lossless,do_filter", [(0, 1), (1, 0)], ids=["filtered", "lossless"])
@pytest.mark.parametrize("case", L.BMC_CASES, ids=[L.case_id(c) for c in L.BMC_CASES])
def test_prediction_with_the_references_own_field(case, lossless, do_filter):
    sc = L.scene(A.load_ref(), case)
    field = L.reference_result(case)[0][0].copy()
    st = L.field_stats(field, sc.params, sc.w, sc.h, case.pan)
    assert st.ge16 >= 0.10 and st.off_picture >= 1
    check_bmc(sc, field, 1 if lossless else case.quant, do_filter, lossless)


@pytest.mark.parametrize("case", L.BMC_CASES, ids=[L.case_id(c) for c in L.BMC_CASES])
def test_prediction_with_a_random_long_field(case):
    """+-800 quarter-pels a component (200 px: past the border from every block of the picture), with the flag classes of
    tests/test_oracle_bmc.py's rand_motion"""
    from test_oracle_bmc import rand_motion
    sc = L.scene(A.load_ref(), case)
    rng = np.random.RandomState(L.case_seed(case))
    mvs = rand_motion(rng, sc.params, big=True)
    inter = (mvs["flags"] & (L.FLAG_INTRA | L.FLAG_SKIP)) == 0
    mvs["x"][inter] = rng.randint(-800, 801, size=int(inter.sum()))
    mvs["y"][inter] = rng.randint(-800, 801, size=int(inter.sum()))
    assert max(np.abs(mvs["x"]).max(), np.abs(mvs["y"]).max()) > 780
    check_bmc(sc, mvs, case.quant, 1)


# ---- whole streams ------------------------------------------------------------------------------------------------------------
streams = pytest.mark.parametrize("stream", L.STREAMS, ids=[L.stream_id(s) for s in L.STREAMS])


@streams
def test_stream_through_dsv_enc(stream):
    want = L.reference_stream(stream)
    pk, stats = encode_stream(A.load_hip(), list(L.stream_frames(stream.vel)), stream.w, stream.h, A.SUBSAMP_420, eos=False, **L.stream_cfg(stream))
    M.assert_same([want], ([pk], [stats]), L.stream_id(stream))


@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_streams_in_lockstep(setting):
    """every velocity of a setting, and the twins without scene-change detection, in one dsv2hip_enc_batch_host step a picture:
    the pan differs per slot, and from the second step on intra pictures (flipped by the search's sums) sit beside P pictures"""
    mine = [s for s in L.STREAMS if s.setting == setting]
    assert len(set(s.vel for s in mine)) == len(L.VELOCITIES)
    built = [L.built(s) for s in mine]
    got = M.run_schedule(A.load_hip(), built, [list(range(len(mine)))] * L.STREAM_FRAMES, lambda t: "host")
    M.assert_same([L.reference_stream(s) for s in mine], got, setting)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=PARSE_IDS.get)
@streams
def test_decoder_on_the_references_packets(stream, mode):
    """return code, frame number and every delivered byte of every packet, under the three parse modes"""
    with parse_mode(mode) as hip:
        got = L.decode_packets(hip, L.reference_stream(stream)[0])
    L.assert_decodes_equal(L.reference_decode(stream), got, L.stream_id(stream))


# ---- the side-information coder's overflow ------------------------------------------------------------------------------------
def test_side_information_overflows_on_its_own():
    """three pictures of 2560 x 1440 with 16 x 16 blocks whose tiles jitter: the x and y vector sub-streams of the P pictures
    outgrow the kernel's 16 384-byte images (tests/test_long_motion_ref.py reads their lengths from the reference's packets),
    so k_side_info itself raises the flag that hands the picture to the host -- no DSV2_SIDE_FORCE_FALLBACK"""
    assert "DSV2_SIDE_FORCE_FALLBACK" not in os.environ
    want = L.reference_jitter_stream()
    hip = bind(A.load_hip())
    before = hip.dsv2hip_enc_side_flag_count()
    pk, stats = encode_stream(hip, list(L.jitter_frames()), L.SIDE_W, L.SIDE_H, A.SUBSAMP_420, eos=False, **L.SIDE_CFG)
    M.assert_same([want], ([pk], [stats]), "jitter")
    assert hip.dsv2hip_enc_side_flag_count() - before == L.SIDE_FRAMES - 1  # every P picture, by the kernel's own verdict
