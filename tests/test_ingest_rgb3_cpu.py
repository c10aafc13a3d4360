"""The three-byte and planar RGB ingest without a GPU: the thread body of k_ingest_rgb3 (csrc/ingest_rgb3.h) compiled for the host
and swept under AddressSanitizer + UndefinedBehaviorSanitizer by tools/ingest_rgb3_check.cpp (a stand-alone program: nothing
sanitized is loaded into Python), its dumped planes against the numpy oracle tests/rgb3_csc.py; the oracle's own claim that a
three-byte, a planar and a four-byte picture of the same pixels are one picture; and, through the library (which loads without a
GPU), that the scaled and sized grammars know nothing of the three layouts.
"""
import ctypes as C
import os

import numpy as np
import pytest

import dsvabi as A
import rgb3_csc as R3
import rgb_csc as R
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
SUBSAMP = {name: 4 * hs + vs for name, (hs, vs) in FMT.items()}  # DSV_SUBSAMP_*: the two shifts


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    """builds tools/ingest_rgb3_check.cpp with the sanitizers, runs its whole sweep and returns the directory of its dumped cases"""
    out, dump = build_and_run("tools/ingest_rgb3_check.cpp", tmp_path_factory.mktemp("ingest_rgb3"), ["--dump", "{dump}"], timeout=60)
    assert "in the wide form" in out
    return dump


def test_kernel_body_sweep_is_clean_and_equals_the_numpy_oracle(dump_dir):
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".src"))
    assert len(names) >= 10
    seen = set()
    for name in names:
        order, csc, fmt, size = name.split("_")
        w, h = (int(v) for v in size.split("x"))
        hs, vs = FMT[fmt]
        layout = R3.ORDER[order] | int(csc, 16)
        pixels = np.fromfile(os.path.join(dump_dir, name + ".src"), dtype=np.uint8).reshape((3, h, w) if order == "rgbp" else (h, w, 3))
        got = np.fromfile(os.path.join(dump_dir, name + ".yuv"), dtype=np.uint8)
        want = np.frombuffer(R3.planar_bytes(pixels, layout, hs, vs), dtype=np.uint8)
        assert got.size == want.size, name
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: byte %d of the packed planes is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want[bad[0]])
        seen.add((order, csc, fmt))
    assert {s[0] for s in seen} == set(R3.ORDER) and {s[1] for s in seen} == {"000", "100", "200", "300"} and {s[2] for s in seen} == set(FMT)
    # 18x18 in the quarter-width formats (cw = 5: the last footprint half outside), which no encoder test can cover, in both kinds
    assert {("rgbp", "410"), ("rgb", "410"), ("rgbp", "411"), ("bgr", "411")} <= {(s[0], s[2]) for s in seen if ("%s_%s_%s_18x18" % s) in names}


SAME = [(18, 18, "411"), (18, 18, "410"), (22, 18, "420"), (17, 16, "444"), (37, 21, "422")]


@pytest.mark.parametrize("w,h,name", SAME, ids=["%dx%d-%s" % s for s in SAME])
def test_three_byte_planar_and_rgba_of_the_same_pixels_are_one_picture(w, h, name):
    """B G R, R G B, three planes and R G B A / B G R A with random alpha: identical planes in every preset -- 18x18 in 4:1:1 and
    "4:1:0" included, which the reference encoder cannot encode (tests/test_gpu_enc_rgb.py) and so only this side covers."""
    hs, vs = FMT[name]
    rng = np.random.default_rng(w * 1000 + h)
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    rgba[:4, :8, :3] = np.array([[255 * (k & 1), 255 * ((k >> 1) & 1), 255 * ((k >> 2) & 1)] for k in range(8)], dtype=np.uint8)  # the cube's corners
    bgra = np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])
    for csc in R.CSC:
        want = R.convert(rgba, R.RGBA | csc, hs, vs)
        assert all(np.array_equal(a, b) for a, b in zip(want, R.convert(bgra, R.BGRA | csc, hs, vs)))
        for order in R3.ORDER.values():
            surface = R3.from_rgba(rgba, order)
            assert surface.shape == ((3, h, w) if order == R3.RGBP else (h, w, 3))
            got = R3.convert(surface, order | csc, hs, vs)
            assert [g.shape for g in got] == [p.shape for p in want]
            assert all(np.array_equal(g, p) for g, p in zip(got, want)), (hex(order | csc), name)
            wide, four = R3.widen(surface, order | csc, alpha=rng.integers(0, 256, (h, w), dtype=np.uint8))
            assert all(np.array_equal(g, p) for g, p in zip(R.convert(wide, four, hs, vs), want))


# ---- the scaled and sized grammars know nothing of the three layouts (the library loads without a GPU) -----------------------------
def test_scaled_and_sized_dims_refuse_the_three_layouts():
    hip = A.load_hip()
    P = C.POINTER
    hip.dsv2hip_enc_scaled_dims.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_int), P(C.c_int), P(C.c_size_t), P(C.c_int)]
    hip.dsv2hip_enc_scaled_dims.restype = C.c_int
    hip.dsv2hip_enc_sized_dims.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_size_t), P(C.c_int)]
    hip.dsv2hip_enc_sized_dims.restype = C.c_int
    ew, eh, rb, rows = C.c_int(), C.c_int(), (C.c_size_t * 3)(), (C.c_int * 3)()
    for name in FMT:
        for layout in (R.RGBA, 0x0):  # the grammar as it was: accepted at these very sizes
            assert hip.dsv2hip_enc_scaled_dims(64, 48, SUBSAMP[name], layout | 0x1000 | (0x100 if layout else 0), C.byref(ew), C.byref(eh), rb, rows) == 0
            assert hip.dsv2hip_enc_sized_dims(64, 48, 40, 30, SUBSAMP[name], layout, rb, rows) == 0
        for order in R3.ORDER.values():
            for csc in R.CSC:
                for scale in (0x0000, 0x1000, 0x2000, 0x3000):
                    layout = order | csc | scale
                    assert hip.dsv2hip_enc_scaled_dims(64, 48, SUBSAMP[name], layout, C.byref(ew), C.byref(eh), rb, rows) == -1, hex(layout)
                    assert hip.dsv2hip_enc_sized_dims(64, 48, 64, 48, SUBSAMP[name], layout, rb, rows) == -1, hex(layout)  # at the encoder's own size
                    assert hip.dsv2hip_enc_sized_dims(64, 48, 40, 30, SUBSAMP[name], layout, rb, rows) == -1, hex(layout)
