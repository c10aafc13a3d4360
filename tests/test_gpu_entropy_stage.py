"""The GPU entropy coder (csrc/entropy_gpu.hip) and the device parser (csrc/dec_parse_dev.hip) behind the stage seam, on the crafted
planes of tests/entropy_cases.py: dsv_encode_plane with the seam switched to the device coder gives the reference's bytes and raises
exactly the flags the model predicts; dsv_decode_plane gives the reference's plane from the reference's bytes with the host parser and
with the device parser, on sound sections and on damaged ones.  tests/test_entropy_cases_ref.py says what each case exercises.

A damaged section: the reference keeps what it had placed before it gave up (hzcc.c:490, :510), and so does the seam's host parser;
the device parser drops a failed section's symbols and has its plane zeroed, which is what the decoder makes of a failed plane
(dsv_decoder.c:516-523).  So on a failed section the three agree on the return value and on bs.pos, the host parser's plane equals
the reference's, and the device parser's plane is zero behind the DC."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dsvabi as A
import entropy_cases as E
import hipabi as H
from entropy_cases import CASES
from test_entropy_cases_ref import reference_section

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

FLAGS = (1, 2, 4, 8)


class device_coder:
    """dsv_encode_plane on the GPU coder inside the block"""

    def __enter__(self):
        self.hip = H.bind(A.load_hip())
        assert self.hip.dsv2hip_seam_set_gpu_entropy(1) == 1
        return self.hip

    def __exit__(self, *a):
        self.hip.dsv2hip_seam_set_gpu_entropy(0)


def flag_counts(hip):
    return [hip.dsv2hip_enc_ent_flag_count(f) for f in FLAGS]


def check_encode(case, plane=0, offset=0):
    want, want_pos = reference_section(case, plane, offset)
    raised = case.model().flags()
    with device_coder() as hip:
        before = flag_counts(hip)
        got, got_pos, coefs = E.encode_plane(hip, case, plane, offset)
        moved = [a - b for a, b in zip(flag_counts(hip), before)]
    print("%s: flags predicted %d, counters moved by %s; %d bytes" % (case.name, raised, moved, want_pos // 8 - offset))
    assert got_pos == want_pos
    assert np.array_equal(got, want), "the buffer: what stands in front, the section, zeros behind"
    assert np.array_equal(coefs, case.plane())
    assert moved == [1 if raised & f else 0 for f in FLAGS]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_encode(case):
    check_encode(case)


@pytest.mark.parametrize("plane", [1, 2])
@pytest.mark.parametrize("name", E.GEOMETRY_CASES)
def test_encode_as_plane(name, plane):
    check_encode(E.BY_NAME[name], plane=plane)


@pytest.mark.parametrize("offset", E.OFFSETS[1:])
@pytest.mark.parametrize("name", E.OFFSET_CASES)
def test_encode_at_offset(name, offset):
    check_encode(E.BY_NAME[name], offset=offset)


def test_host_coder_is_the_default_and_raises_no_flag():
    hip = H.bind(A.load_hip())
    if "DSV2_SEAM_GPU_ENTROPY" not in os.environ:
        assert hip.dsv2hip_seam_set_gpu_entropy(-1) == 0
    hip.dsv2hip_seam_set_gpu_entropy(0)
    case = E.BY_NAME["dense-200-finest"]
    want, want_pos = reference_section(case)
    before = flag_counts(hip)
    got, got_pos, _ = E.encode_plane(hip, case)
    assert got_pos == want_pos and np.array_equal(got, want)
    assert flag_counts(hip) == before
    assert hip.dsv2hip_enc_ent_flag_count(3) == -1


# ---- decode -------------------------------------------------------------------------------------------------------------------------
MODES = pytest.mark.parametrize("mode", [0, 2], ids=[H.PARSE_IDS[0], H.PARSE_IDS[2]])
TAIL = 64  # bytes of 0xff behind a section: a code that runs over the section's end ends there, in every library


def padded(buf, end):
    out = np.array(buf[:end + TAIL])
    out[end:] = 0xFF
    return out


def check_decode(case, mode, plane=0, offset=0):
    want, want_pos = reference_section(case, plane, offset)
    buf = padded(want, want_pos // 8)
    ok_r, pos_r, plane_r = E.decode_plane(A.load_ref(), buf, case, plane, offset)
    with H.parse_mode(mode) as hip:
        ok, pos, got = E.decode_plane(hip, buf, case, plane, offset)
    assert ok_r == 1 and pos_r == want_pos and np.array_equal(plane_r, case.plane())
    assert (ok, pos) == (ok_r, pos_r)
    assert np.array_equal(got, plane_r)


@MODES
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_decode(case, mode):
    check_decode(case, mode)


@MODES
@pytest.mark.parametrize("plane", [1, 2])
@pytest.mark.parametrize("name", E.GEOMETRY_CASES)
def test_decode_as_plane(name, plane, mode):
    check_decode(E.BY_NAME[name], mode, plane=plane)


@MODES
@pytest.mark.parametrize("offset", E.OFFSETS[1:])
@pytest.mark.parametrize("name", E.OFFSET_CASES)
def test_decode_at_offset(name, offset, mode):
    check_decode(E.BY_NAME[name], mode, offset=offset)


def damaged(case):
    """(name, buffer) of the section with its last byte gone, its length one less, its 24-bit symbol count one more and one less"""
    want, want_pos = reference_section(case)
    end, m = want_pos // 8, case.model()
    count_at = 4 + (E.seg_len(m.ll) + 7) // 8
    assert int.from_bytes(bytes(want[count_at:count_at + 3]), "big") == m.n and want[end - 1] == 0x55
    out = []
    cut = padded(want, end - 1)
    out.append(("last byte gone", cut))
    short = padded(want, end)
    short[:4] = list((end - 5).to_bytes(4, "big"))
    out.append(("length one less", short))
    for name, n in (("count one more", m.n + 1), ("count one less", m.n - 1)):
        if n >= 0:  # (an empty section has no count one less)
            b = padded(want, end)
            b[count_at:count_at + 3] = list(n.to_bytes(3, "big"))
            out.append((name, b))
    return out


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_decode_damaged(case):
    ref = A.load_ref()
    for name, buf in damaged(case):
        ok_r, pos_r, plane_r = E.decode_plane(ref, buf, case)
        with H.parse_mode(0) as hip:
            ok_h, pos_h, plane_h = E.decode_plane(hip, buf, case)
        with H.parse_mode(2) as hip:
            ok_d, pos_d, plane_d = E.decode_plane(hip, buf, case, fill=7)
        print("%s, %s: reference %d, host parser %d, device parser %d" % (case.name, name, ok_r, ok_h, ok_d))
        assert (ok_h, pos_h) == (ok_r, pos_r) and (ok_d, pos_d) == (ok_r, pos_r), name
        assert np.array_equal(plane_h, plane_r), name
        if ok_r:
            with H.parse_mode(2) as hip:
                _, _, plane_d = E.decode_plane(hip, buf, case)
            assert np.array_equal(plane_d, plane_r), name
        else:  # the conditional fill ran: nothing of what the plane held, nothing of what was parsed
            assert plane_d[0] == plane_r[0] and not np.any(plane_d[1:]), name


# ---- a whole stream whose I picture reaches flag 1 inside the packet bound (tests/stream_sections.py) ------------------------------------
def run_streams(names, kind):
    """the named streams, all in every step of `kind`: (packets per stream, how far the flag-1 counter moved)"""
    import mixed_steps as M
    import stream_sections as S
    from test_entropy_cases_ref import stream_reference
    streams = [S.flag1_stream() if n == "flag1" else S.neighbour_stream() for n in names]
    hip = H.bind(A.load_hip())
    before = hip.dsv2hip_enc_ent_flag_count(1)
    got, _ = M.run_schedule(hip, streams, M.together([st["spec"] for st in streams]), lambda t: kind)
    moved = hip.dsv2hip_enc_ent_flag_count(1) - before
    for n, g in zip(names, got):
        want = stream_reference(n)[0]
        assert len(g) == len(want) and all(a == b for a, b in zip(want, g)), "packets of the %s stream" % n
    return moved, sum(stream_reference(n)[2] for n in names)


def test_stream_that_falls_back_through_dsv_enc():
    moved, predicted = run_streams(["flag1"], "frame")
    assert predicted == 1 and moved == 1


def test_stream_that_falls_back_beside_one_that_does_not():
    moved, predicted = run_streams(["neighbour", "flag1"], "host")
    assert predicted == 1 and moved == 1, "one picture of the two streams' four hands its planes to the host coder"


# ---- the other paths of the same kernels, chosen when the library loads: processes of their own ----------------------------------------
def rerun(select, env, files=("tests/test_gpu_entropy_stage.py",), timeout=900):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", select] + list(files), cwd=A.ROOT,
                       env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.strip().splitlines()[-1]


# DSV2_ENT_EMIT_WORDS shrinks the emit kernel's LDS image of a chunk: 8 words send every chunk down the path that ORs its code words
# straight into global memory, 40 mix both paths
@pytest.mark.parametrize("words", ["8", "40"])
def test_child_encode_with_a_small_emit_image(words):
    rerun("test_encode and not child", {"DSV2_ENT_EMIT_WORDS": words})


# DSV2_DEC_LANE_ROUNDS=0: the parser's serial step alone
def test_child_decode_with_the_serial_step():
    rerun("test_decode and device-parse", {"DSV2_DEC_LANE_ROUNDS": "0"})


def test_switches_of_this_process():
    """a process started with DSV2_TEST_EXPECT_DEVICE_CODERS=1 (the child below) runs the seam on both device coders"""
    hip = H.bind(A.load_hip())
    if os.environ.get("DSV2_TEST_EXPECT_DEVICE_CODERS") == "1":
        assert hip.dsv2hip_seam_set_gpu_entropy(-1) == 1 and hip.dsv2hip_dec_parse_mode() == 2
    else:
        assert hip.dsv2hip_seam_set_gpu_entropy(-1) == int(os.environ.get("DSV2_SEAM_GPU_ENTROPY", "0") != "0")


# the plane cases of the older modules -- the lossy quantiser's real symbol lists at the edge geometries and contents -- once more with
# the seam's encode side on the GPU coder and its decode side on the device parser; their assertions are theirs
def test_child_plane_tests_on_the_device_coders():
    rerun("test_encode_decode_plane or test_switches_of_this_process",
          {"DSV2_SEAM_GPU_ENTROPY": "1", "DSV2_DEC_DEVICE_PARSE": "2", "DSV2_TEST_EXPECT_DEVICE_CODERS": "1"},
          files=("tests/test_gpu_entropy_stage.py", "tests/test_gpu_quant.py", "tests/test_gpu_edges.py"), timeout=1500)
