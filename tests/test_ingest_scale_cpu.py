"""Half, quarter and eighth-size ingest without a GPU: the thread bodies of k_ingest_surface_scaled and k_ingest_rgb_scaled and the
device-free validity rule (csrc/ingest_scale.h) compiled for the host and swept under AddressSanitizer + UndefinedBehaviorSanitizer
by tools/ingest_scale_check.cpp (a stand-alone program: nothing sanitized is loaded into Python), its dumped planes against the
numpy oracle tests/ingest_scale.py -- which pins the kernels' text, the program's C restatement and the oracle of
tests/test_gpu_enc_scale.py to one another -- the arithmetic claims the header makes about the scaled conversion over all 2^24
colours, the refusal matrix of the validity rule, and dsv2hip_enc_scaled_dims (the library loads without a GPU).
"""
import ctypes as C
import os

import numpy as np
import pytest

import box_reduce as B
import dsvabi as A
import ingest_scale as S
import rgb_csc as R
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
SUBSAMP = {"444": 0x0, "422": 0x4, "420": 0x5, "411": 0x8, "410": 0xA}
UYVY = 0x14


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    """builds tools/ingest_scale_check.cpp with the sanitizers, runs its whole sweep and returns the directory of its dumped cases"""
    out, dump = build_and_run("tools/ingest_scale_check.cpp", tmp_path_factory.mktemp("ingest_scale"), ["--dump", "{dump}"], timeout=900)
    assert "in the wide form" in out and "cases of the validity rule equal its restatement" in out
    return dump


def same_bytes(name, got, want):
    assert got.size == want.size, name
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: byte %d of the packed planes is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want[bad[0]])


def test_kernel_body_sweep_is_clean_and_equals_the_numpy_oracle(dump_dir):
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".src"))
    seen = set()
    for name in names:
        parts = name.split("_")
        w, h = (int(v) for v in parts[-1].split("x"))
        s = int(parts[-2][1:])
        hs, vs = FMT[parts[-3]]
        src = np.fromfile(os.path.join(dump_dir, name + ".src"), dtype=np.uint8)
        got = np.fromfile(os.path.join(dump_dir, name + ".yuv"), dtype=np.uint8)
        if parts[0] in ("planar", "semi"):
            kind = S.SEMI if parts[0] == "semi" else S.PLANAR
            planes, at = [], 0
            for rb, rows in S.source_dims(w, h, hs, vs, kind):
                planes.append(src[at:at + rb * rows].reshape(rows, rb))
                at += rb * rows
            assert at == src.size
            want = S.reduce_yuv(planes, s)
        else:
            layout = {"bgra": R.BGRA, "rgba": R.RGBA}[parts[0]] | int(parts[1], 16)
            want = S.convert_scaled(src.reshape(h, w, 4), layout, hs, vs, s)
        assert [p.shape for p in want] == [(S.up(h, s), S.up(w, s))] + [(S.up(S.up(h, s), vs), S.up(S.up(w, s), hs))] * 2
        same_bytes(name, got, np.frombuffer(S.packed(want), dtype=np.uint8))
        seen.add((parts[0], parts[-3], s))
    assert {k[0] for k in seen} == {"planar", "semi", "bgra", "rgba"} and {k[1] for k in seen} == set(FMT) and {k[2] for k in seen} == {1, 2, 3}
    assert len(names) >= 13


def test_refusal_matrix_of_the_validity_rule(dump_dir):
    """a 34x18 encoder: what the scaled calls take and what they refuse, by the device-free rule they call"""
    got = dict(line.split() for line in open(os.path.join(dump_dir, "validity.txt")))
    want = {"planar_half": 1, "nv12_quarter": 1, "bgra709_half": 1, "rgba_full_eighth": 1, "plain_planar": 1,
            "layout_0x4000": 0, "layout_0x1010": 0, "layout_0x1012": 0, "planar_half_bt709": 0, "semiplanar_half_full": 0,
            "source_69x35": 0, "source_67x37": 0, "src_w_0": 0, "src_h_negative": 0,
            "pitch_short_planar_0": 0, "pitch_short_planar_1": 0, "pitch_short_planar_2": 0, "pitch_short_nv12_1": 0, "pitch_short_rgb_0": 0,
            "null_planar_2": 0, "null_nv12_1": 0, "null_nv12_2_is_ignored": 1, "null_rgb_0": 0,
            "rgb_on_uyvy_format": 0, "nv16_on_uyvy_format": 1}
    assert {k: int(v) for k, v in got.items()} == want


# ---- the oracle itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FMT))
def test_shift_0_is_the_plain_conversion(name):
    hs, vs = FMT[name]
    rng = np.random.default_rng(11)
    for k, (w, h) in enumerate([(1, 1), (17, 16), (22, 19), (37, 23)]):
        px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        layout = (R.BGRA, R.RGBA)[k & 1] | R.CSC[k % 4]
        for a, b in zip(S.convert_scaled(px, layout, hs, vs, 0), R.convert(px, layout, hs, vs)):
            assert np.array_equal(a, b)


def test_yuv_oracle_is_the_reduction_of_each_source_plane():
    """planar and semiplanar sources of one picture give the same planes, and they are box_reduce's of each source plane"""
    rng = np.random.default_rng(12)
    for name, (hs, vs) in FMT.items():
        for w, h in [(1, 1), (31, 31), (67, 35), (121, 125)]:
            dims = S.source_dims(w, h, hs, vs, S.PLANAR)
            planes = [rng.integers(0, 256, (rows, rb), dtype=np.uint8) for rb, rows in dims]
            for s in (1, 2, 3):
                got = S.reduce_yuv(planes, s)
                semi = S.reduce_yuv([planes[0], B.interleave(planes[1], planes[2])], s)
                for c in range(3):
                    assert np.array_equal(got[c], B.reduce(planes[c], s)) and np.array_equal(got[c], semi[c])
                assert got[0].shape == (S.up(h, s), S.up(w, s)) and got[1].shape == (S.up(S.up(h, s), vs), S.up(S.up(w, s), hs))  # (round-ups commute)


@pytest.mark.parametrize("csc", R.CSC, ids=["bt601", "bt709", "bt601_full", "bt709_full"])
def test_arithmetic_claims_over_all_colours(csc):
    """What include/dsv2_hip.h says of the scaled conversion, for s = 1 .. 3 and every chroma footprint (hs + vs + 2s = 2 .. 10): a
    footprint of equal pixels gives what one pixel gives, for every one of the 2^24 colours; limited range stays within Y 16..235 and
    U, V 16..240 without a clamp; every sum is non-negative before its shift; the largest accumulator -- 1024 pixels of the extreme
    colour, positive or negative part -- is at most 1024 * 255 * 128 and, with the bias, below 2^32."""
    full = bool(csc & R.FULL)
    m = R.MATRIX[csc]
    g, b = (a.astype(np.int64) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    for r0 in range(256):
        r = np.full_like(g, r0)
        y1 = R.weighted(m[0], r, g, b)
        one = (y1 + 128 + 256 * R.ybase(csc)) >> 8
        if not full:
            assert one.min() >= 16 and one.max() <= 235
        for s in (1, 2, 3):
            assert np.array_equal(((y1 << (2 * s)) + ((128 + 256 * R.ybase(csc)) << (2 * s))) >> (8 + 2 * s), one)
        for row in m[1:]:
            c1 = R.weighted(row, r, g, b)
            single = R.chroma_sum(c1, 0)
            raw = (c1 + 32896) >> 8
            assert c1.min() + 32896 >= 0
            if not full:
                assert raw.min() >= 16 and raw.max() <= 240
            for lg in range(2, 11):  # (sums of 1 << lg equal pixels: the bias scales alike, so the sum stays non-negative)
                assert np.array_equal(R.chroma_sum(c1 << lg, lg), single)
    for row in m[1:]:  # (the kernel sums the positive coefficients and the magnitudes of the negative ones apart)
        pos, neg = sum(c for c in row if c > 0), -sum(c for c in row if c < 0)
        assert max(pos, neg) <= 128 and 1024 * 255 * max(pos, neg) <= 33423360
        assert 1024 * 255 * pos + (32896 << 10) < 1 << 32
    assert 64 * 255 * sum(m[0]) + ((128 + 256 * 16) << 6) <= 33423360  # (luma: 64 pixels at most)


def test_mixed_footprints_stay_in_range():
    """random and extreme footprints through the oracle: limited range needs no clamp at any scale"""
    rng = np.random.default_rng(13)
    px = rng.integers(0, 256, (64, 96, 4), dtype=np.uint8)
    px[:32, :48, :3] = rng.choice(np.array([0, 255], dtype=np.uint8), (32, 48, 3))
    for s in (1, 2, 3):
        for name, (hs, vs) in FMT.items():
            y, u, v = S.convert_scaled(px, R.RGBA | R.BT709, hs, vs, s)
            assert 16 <= y.min() and y.max() <= 235 and 16 <= min(u.min(), v.min()) and max(u.max(), v.max()) <= 240


# ---- dsv2hip_enc_scaled_dims ------------------------------------------------------------------------------------------------------
def scaled_dims(hip, src_w, src_h, subsamp, layout):
    hip.dsv2hip_enc_scaled_dims.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    hip.dsv2hip_enc_scaled_dims.restype = C.c_int
    ew, eh, rb, rows = C.c_int(-7), C.c_int(-7), (C.c_size_t * 3)(), (C.c_int * 3)()
    r = hip.dsv2hip_enc_scaled_dims(src_w, src_h, subsamp, layout, C.byref(ew), C.byref(eh), rb, rows)
    return r, (ew.value, eh.value), list(rb), list(rows)


def test_scaled_dims_at_odd_sizes_in_every_format():
    hip = A.load_hip()
    for name, (hs, vs) in FMT.items():
        for src_w, src_h in [(1, 1), (31, 31), (67, 35), (133, 69), (269, 141), (297, 169), (1920, 1080)]:
            scw, sch = S.up(src_w, hs), S.up(src_h, vs)
            for s in range(4):
                enc = (S.up(src_w, s), S.up(src_h, s))
                assert scaled_dims(hip, src_w, src_h, SUBSAMP[name], S.SCALE[s] | S.PLANAR) == (0, enc, [src_w, scw, scw], [src_h, sch, sch])
                assert scaled_dims(hip, src_w, src_h, SUBSAMP[name], S.SCALE[s] | S.SEMI) == (0, enc, [src_w, 2 * scw, 0], [src_h, sch, 0])
                assert scaled_dims(hip, src_w, src_h, SUBSAMP[name], S.SCALE[s] | R.RGBA | R.BT709) == (0, enc, [4 * src_w, 0, 0], [src_h, 0, 0])
                # the reduced source planes are the encoder's planes (nested round-ups commute)
                assert (S.up(scw, s), S.up(sch, s)) == (S.up(enc[0], hs), S.up(enc[1], vs))


def test_scaled_dims_refuses_what_is_no_layout_size_or_format():
    hip = A.load_hip()
    for layout in (0x4000, 0x1010, 0x1012, 0x12, 0x410, 0x1100, 0x1201, 0x2, -1):
        assert scaled_dims(hip, 67, 35, 0x5, layout)[0] == -1, hex(layout)
    for layout in (0x0, 0x1, 0x10, 0x311, 0x1000, 0x2001, 0x1110, 0x1210, 0x1310, 0x1011, 0x2010, 0x3010, 0x3311):
        assert scaled_dims(hip, 67, 35, 0x5, layout)[0] == 0, hex(layout)
    for w, h in [(0, 35), (67, 0), (-1, 35), (67, -4)]:
        assert scaled_dims(hip, w, h, 0x5, 0x1000)[0] == -1
    assert scaled_dims(hip, 67, 35, UYVY, 0x1001)[0] == 0 and scaled_dims(hip, 67, 35, UYVY, 0x1011)[0] == -1
    for bad_format in (0x1, 0x6, 0xF, 0x15, -1):
        assert scaled_dims(hip, 67, 35, bad_format, 0x1000)[0] == -1
    hip.dsv2hip_enc_scaled_dims.argtypes = None
    assert hip.dsv2hip_enc_scaled_dims(67, 35, 0x5, 0x1000, None, None, None, None) == -1
