"""Ingest at any larger size without a GPU: the thread bodies of k_ingest_sized and k_ingest_rgb_sized and the device-free validity
rule (csrc/ingest_resize.h) compiled for the host and swept under AddressSanitizer + UndefinedBehaviorSanitizer by
tools/ingest_resize_check.cpp (a stand-alone program: nothing sanitized is loaded into Python), its dumped planes against the numpy
oracle tests/ingest_resize.py -- which pins the kernels' text, the program's C restatement and the oracle of
tests/test_gpu_enc_resize.py to one another -- the arithmetic claims the header makes about the sized RGB conversion, the refusal
matrix of the validity rule, and dsv2hip_enc_sized_dims (the library loads without a GPU).
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import area_resize as AR
import dsvabi as A
import ingest_resize as IR
import ingest_scale as S
import rgb_csc as R
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
SUBSAMP = {"444": 0x0, "422": 0x4, "420": 0x5, "411": 0x8, "410": 0xA}
UYVY = 0x14


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    """builds tools/ingest_resize_check.cpp with the sanitizers, runs its whole sweep and returns the directory of its dumped cases"""
    out, dump = build_and_run("tools/ingest_resize_check.cpp", tmp_path_factory.mktemp("ingest_resize"), ["--dump", "{dump}"], timeout=900)
    assert "in the wide form" in out and "cases of the validity rule equal its restatement" in out
    return dump


def same_bytes(name, got, want):
    assert got.size == want.size, name
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: byte %d of the packed planes is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want[bad[0]])


def test_kernel_body_sweep_is_clean_and_equals_the_numpy_oracle(dump_dir):
    """the dumps: NAME = layout[_csc]_format_SWxSH_WxH"""
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".src"))
    seen = set()
    for name in names:
        parts = name.split("_")
        sw, sh = (int(v) for v in parts[-2].split("x"))
        w, h = (int(v) for v in parts[-1].split("x"))
        hs, vs = FMT[parts[-3]]
        src = np.fromfile(os.path.join(dump_dir, name + ".src"), dtype=np.uint8)
        got = np.fromfile(os.path.join(dump_dir, name + ".yuv"), dtype=np.uint8)
        if parts[0] in ("planar", "semi"):
            kind = S.SEMI if parts[0] == "semi" else S.PLANAR
            planes, at = [], 0
            for rb, rows in S.source_dims(sw, sh, hs, vs, kind):
                planes.append(src[at:at + rb * rows].reshape(rows, rb))
                at += rb * rows
            assert at == src.size
            want = IR.resize_yuv(planes, w, h, hs, vs)
        else:
            layout = {"bgra": R.BGRA, "rgba": R.RGBA}[parts[0]] | int(parts[1], 16)
            want = IR.convert_sized(src.reshape(sh, sw, 4), layout, w, h, hs, vs)
        assert [p.shape for p in want] == [(h, w)] + [(S.up(h, vs), S.up(w, hs))] * 2
        same_bytes(name, got, np.frombuffer(IR.packed(want), dtype=np.uint8))
        seen.add((parts[0], parts[-3]))
    assert {k[0] for k in seen} == {"planar", "semi", "bgra", "rgba"} and {k[1] for k in seen} == set(FMT)
    assert len(names) >= 14


def test_the_sweep_ran_the_promised_cases(dump_dir):
    """cases.txt: the twelve shapes of test_egress_resize_cpu.py in both forms, planar and semiplanar, with noise and the four
    constants, at offsets 0 .. 3 and the three pitches; RGB in both byte orders, the four presets and the five formats, both forms,
    footprints of 2, 9 and 33 taps."""
    yuv, rgb = set(), set()
    for line in open(os.path.join(dump_dir, "cases.txt")):
        f = line.split()
        rec = (f[1], f[2], f[3], tuple(int(v) for v in f[4:8]), int(f[8]), int(f[9]), int(f[10]))
        (yuv if f[0] == "yuv" else rgb).add(rec)
    for shape in AR.SWEEP_SHAPES:
        for layout in ("planar", "semi"):
            # (the documented rule: the wide form needs every source plane's row bytes to be a multiple of 4)
            can_wide = all(rb % 4 == 0 for rb, _ in S.source_dims(shape[0], shape[1], 1, 1, S.SEMI if layout == "semi" else S.PLANAR))
            forms = {r[0] for r in yuv if r[1] == layout and r[3] == shape and r[4] == -1}
            assert forms == ({"wide", "general"} if can_wide else {"general"}), (shape, layout)
            assert {(r[5], r[6]) for r in yuv if r[1] == layout and r[3] == shape and r[4] == -1} == set(itertools.product(range(3), range(4)))
            assert {r[4] for r in yuv if r[1] == layout and r[3] == shape} == {-1, 0, 1, 254, 255}
    assert sum(all(rb % 4 == 0 for rb, _ in S.source_dims(c[0], c[1], 1, 1, S.SEMI)) for c in AR.SWEEP_SHAPES) >= 4
    assert any(r[3][2] > 256 for r in yuv) and any(r[3][2] > 256 for r in rgb)  # a row of more than one workgroup
    assert {r[2] for r in yuv} == set(FMT) and {r[2] for r in rgb} == set(FMT)
    assert {r[1] for r in rgb} == {"%s%03x" % (o, c) for o in ("bgra", "rgba") for c in (0x000, 0x100, 0x200, 0x300)}
    assert {r[0] for r in rgb} == {"wide", "general"}
    assert {(r[5], r[6]) for r in rgb} >= set(itertools.product(range(3), range(4)))
    assert {r[4] for r in rgb} == {-1, 0, 1, 254, 255}
    # footprints of 2 taps (35 -> 34), 9 (127 -> 16) and 33 (the "4:1:0" chroma of 254 x 250 -> 32 x 32: 254 -> 8, 31.75 pixels a sample)
    for name in FMT:
        assert {r[3] for r in rgb if r[2] == name} >= {(35, 19, 34, 18), (127, 121, 16, 16), (254, 250, 32, 32)}
    w = AR.weights(254, 8)
    assert (w > 0).sum(axis=1).max() == 33 and (AR.weights(127, 16) > 0).sum(axis=1).max() == 9 and (AR.weights(35, 34) > 0).sum(axis=1).max() == 2


def test_refusal_matrix_of_the_validity_rule(dump_dir):
    """a 34x18 encoder: what the sized calls take and what they refuse, by the device-free rule they call"""
    got = dict(line.split() for line in open(os.path.join(dump_dir, "validity.txt")))
    want = {"planar_51x27": 1, "nv12_35x19": 1, "bgra709_51x27": 1, "rgba_full_272x144": 1, "own_size_planar": 1, "anamorphic_272x18": 1,
            "nv12_half_67x35": 1, "nv12_half_51x27": 0, "source_273x18": 0, "source_33x18": 0, "source_34x145": 0,
            "src_w_0": 0, "src_h_0": 0, "src_w_negative": 0, "layout_0x4000": 0, "layout_0x1010": 0, "layout_0x2": 0, "planar_bt709": 0,
            "pitch_tight_planar": 1, "pitch_short_planar_0": 0, "pitch_short_planar_1": 0, "pitch_short_planar_2": 0,
            "pitch_tight_nv12": 1, "pitch_short_nv12_1": 0, "pitch_tight_rgb": 1, "pitch_short_rgb_0": 0,
            "null_planar_2": 0, "null_nv12_1": 0, "null_rgb_0": 0, "rgb_on_uyvy_format": 0, "nv16_on_uyvy_format": 1, "format_0x1": 0}
    assert {k: int(v) for k, v in got.items()} == want


# ---- the oracle itself, and the header's arithmetic claims --------------------------------------------------------------------------
def extreme_pictures(sw, sh):
    """pictures of the eight extreme colours, whole and in halves, in RGBA order"""
    out = []
    for r, g, b in itertools.product((0, 255), repeat=3):
        px = np.zeros((sh, sw, 4), dtype=np.uint8)
        px[..., 0], px[..., 1], px[..., 2], px[..., 3] = r, g, b, 200
        out.append(px)
        half = px.copy()
        half[:, sw // 2:, :3] = 255 - half[:, sw // 2:, :3]
        out.append(half)
    return out


@pytest.mark.parametrize("csc", R.CSC, ids=["bt601", "bt709", "bt601_full", "bt709_full"])
def test_arithmetic_claims_over_the_extreme_colours(csc):
    """What include/dsv2_hip.h says of the sized conversion: every numerator is non-negative and, with D <= 65 535, below 2^32 (the
    oracle asserts both for every sample it makes, and the bound is worked out here for the largest D); the divisor 256 * D is below
    2^24; a footprint of equal pixels gives what one pixel gives; limited range stays within Y 16 ... 235 and U, V 16 ... 240."""
    m = R.MATRIX[csc]
    D = IR.RGB_MAX_D
    for c, row in enumerate(m):
        pos, neg = sum(v for v in row if v > 0), -sum(v for v in row if v < 0)
        bias = (128 + 256 * R.ybase(csc)) if c == 0 else 32896
        assert 255 * pos * D + bias * D <= 65536 * D < 1 << 32  # the largest numerator: the positive part saturated, the negative one 0
        assert bias * D - 255 * neg * D >= 0                    # the smallest
    assert 256 * D < 1 << 24 and 65536 * (D + 1) >= 1 << 32  # (and 65 536 is no bound to spare: D = 65 536 would not fit)
    for (sw, sh, w, h), (hs, vs) in [((51, 27, 34, 18), (1, 1)), ((127, 121, 16, 16), (2, 2)), ((255, 257, 254, 256), (0, 0))]:
        assert IR.allowed(sw, sh, w, h, hs, vs, True)
        for px in extreme_pictures(sw, sh):
            y, u, v = IR.convert_sized(px, R.RGBA | csc, w, h, hs, vs)  # (asserts the numerators' range)
            if not csc & R.FULL:
                assert 16 <= y.min() and y.max() <= 235 and 16 <= min(u.min(), v.min()) and max(u.max(), v.max()) <= 240
            if np.all(px[..., :3] == px[0, 0, :3]):
                one = R.convert(px[:1, :1], R.RGBA | csc, 0, 0)
                assert np.all(y == one[0][0, 0]) and np.all(u == one[1][0, 0]) and np.all(v == one[2][0, 0])
    assert IR.D_of(255, 257, 254, 256) == 65535 and not IR.allowed(256, 256, 255, 255, 0, 0, True) and IR.allowed(256, 256, 255, 255, 0, 0, False)


def test_the_headers_examples():
    for w, h in [(1280, 720), (854, 480)]:
        assert IR.allowed(1920, 1080, w, h, 1, 1, True) and IR.allowed(1920, 1080, w, h, 1, 1, False)
    assert (IR.D_of(1920, 1080, 1280, 720), IR.D_of(1920, 1080, 640, 360)) == (9, 9)
    assert (IR.D_of(1920, 1080, 854, 480), IR.D_of(1920, 1080, 427, 240)) == (8640, 17280)
    assert (IR.D_of(1920, 1080, 224, 224), IR.D_of(1920, 1080, 112, 112)) == (8100, 16200)  # inside the bound on D ...
    assert not IR.allowed(1920, 1080, 224, 224, 1, 1, True) and IR.allowed(1792, 1080, 224, 224, 1, 1, True)  # ... but 1920 > 8 * 224
    assert IR.D_of(1920, 1080, 1918, 1078) == 518400
    assert not IR.allowed(1920, 1080, 1918, 1078, 1, 1, True) and IR.allowed(1920, 1080, 1918, 1078, 1, 1, False)


@pytest.mark.parametrize("name", sorted(FMT))
def test_exact_ratios_equal_the_scaled_oracle(name):
    """src = n * enc with W, H multiples of the chroma subsampling: the sized formulas are the scaled call's, YUV and RGB"""
    hs, vs = FMT[name]
    rng = np.random.default_rng(21)
    for s in (1, 2, 3):
        w, h = 16, 12
        sw, sh = w << s, h << s
        px = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)
        for k, csc in enumerate(R.CSC):
            layout = (R.BGRA, R.RGBA)[k & 1] | csc
            for a, b in zip(IR.convert_sized(px, layout, w, h, hs, vs), S.convert_scaled(px, layout, hs, vs, s)):
                assert np.array_equal(a, b)
        dims = S.source_dims(sw, sh, hs, vs, S.PLANAR)
        planes = [rng.integers(0, 256, (rows, rb), dtype=np.uint8) for rb, rows in dims]
        for a, b in zip(IR.resize_yuv(planes, w, h, hs, vs), S.reduce_yuv(planes, s)):
            assert np.array_equal(a, b)
    px = rng.integers(0, 256, (12, 16, 4), dtype=np.uint8)  # the encoder's own size: the plain conversion
    for a, b in zip(IR.convert_sized(px, R.BGRA | R.BT709, 16, 12, hs, vs), R.convert(px, R.BGRA | R.BT709, hs, vs)):
        assert np.array_equal(a, b)


def test_yuv_oracle_is_the_resampling_of_each_source_plane():
    rng = np.random.default_rng(22)
    for name, (hs, vs) in FMT.items():
        for sw, sh, w, h in [(51, 27, 34, 18), (127, 121, 16, 16), (35, 19, 34, 18)]:
            planes = [rng.integers(0, 256, (rows, rb), dtype=np.uint8) for rb, rows in S.source_dims(sw, sh, hs, vs, S.PLANAR)]
            got = IR.resize_yuv(planes, w, h, hs, vs)
            semi = IR.resize_yuv([planes[0], np.stack([planes[1], planes[2]], axis=2).reshape(planes[1].shape[0], -1)], w, h, hs, vs)
            for c, (ow, oh) in enumerate(AR.plane_sizes(w, h, hs, vs)):
                assert np.array_equal(got[c], AR.resize(planes[c], ow, oh)) and np.array_equal(got[c], semi[c])


# ---- dsv2hip_enc_sized_dims through the library ----------------------------------------------------------------------------------------
def sized_dims(hip, sw, sh, w, h, subsamp, layout):
    hip.dsv2hip_enc_sized_dims.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    hip.dsv2hip_enc_sized_dims.restype = C.c_int
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    r = hip.dsv2hip_enc_sized_dims(sw, sh, w, h, subsamp, layout, rb, rows)
    return r, list(rb), list(rows)


def test_sized_dims_in_every_format_and_at_every_bound():
    hip = A.load_hip()
    for name, (hs, vs) in FMT.items():
        for w, h in [(1, 1), (16, 16), (34, 18), (1280, 720)]:
            for sw, sh in [(w, h), (w + 1, h), (w, 8 * h), (8 * w, 8 * h), (8 * w + 1, h), (w, 8 * h + 1), (w - 1, h), (0, h), (w, -2), (3 * w // 2 + 1, 3 * h // 2 + 1)]:
                scw, sch = S.up(sw, hs), S.up(sh, vs)
                for layout, rgb, rb, rows in [(S.PLANAR, False, [sw, scw, scw], [sh, sch, sch]), (S.SEMI, False, [sw, 2 * scw, 0], [sh, sch, 0]),
                                              (R.RGBA | R.BT709, True, [4 * sw, 0, 0], [sh, 0, 0])]:
                    got = sized_dims(hip, sw, sh, w, h, SUBSAMP[name], layout)
                    if IR.allowed(sw, sh, w, h, hs, vs, rgb):
                        assert got == (0, rb, rows), (name, sw, sh, w, h, layout)
                    else:
                        assert got[0] == -1, (name, sw, sh, w, h, layout)
    assert sized_dims(hip, 1920, 1080, 1918, 1078, 0x5, S.SEMI)[0] == 0 and sized_dims(hip, 1920, 1080, 1918, 1078, 0x5, R.BGRA | R.FULL)[0] == -1
    assert sized_dims(hip, 4099, 4099, 4098, 4098, 0x0, S.PLANAR)[0] == -1 and sized_dims(hip, 4093, 4099, 4092, 4098, 0x0, S.PLANAR)[0] == 0
    assert sized_dims(hip, 32769, 64, 16384, 32, 0x0, S.PLANAR)[0] == -1 and sized_dims(hip, 32768, 64, 16384, 32, 0x0, S.PLANAR)[0] == 0


def test_sized_dims_refuses_what_is_no_layout_or_format_and_follows_the_scaled_rule_with_a_scale_value():
    hip = A.load_hip()
    for layout in (0x4000, 0x1010, 0x1012, 0x12, 0x410, 0x1100, 0x1201, 0x2, -1):
        assert sized_dims(hip, 67, 35, 34, 18, 0x5, layout)[0] == -1, hex(layout)
    for layout in (0x0, 0x1, 0x10, 0x311):  # sized from 51x27
        assert sized_dims(hip, 51, 27, 34, 18, 0x5, layout)[0] == 0, hex(layout)
    for layout in (0x1000, 0x1001, 0x1110, 0x1011):  # half size: from 67x35 or 68x36 alone
        assert sized_dims(hip, 67, 35, 34, 18, 0x5, layout)[0] == 0 and sized_dims(hip, 68, 36, 34, 18, 0x5, layout)[0] == 0
        assert sized_dims(hip, 51, 27, 34, 18, 0x5, layout)[0] == -1 and sized_dims(hip, 69, 35, 34, 18, 0x5, layout)[0] == -1
    assert sized_dims(hip, 51, 27, 34, 18, UYVY, 0x1)[0] == 0 and sized_dims(hip, 51, 27, 34, 18, UYVY, 0x11)[0] == -1
    for bad_format in (0x1, 0x6, 0xF, 0x15, -1):
        assert sized_dims(hip, 51, 27, 34, 18, bad_format, 0x0)[0] == -1
    hip.dsv2hip_enc_sized_dims.argtypes = None
    assert hip.dsv2hip_enc_sized_dims(51, 27, 34, 18, 0x5, 0x0, None, None) == -1
