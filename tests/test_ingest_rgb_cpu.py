"""The RGB ingest without a GPU: the thread body of k_ingest_rgb (csrc/ingest_rgb.h) compiled for the host and swept under
AddressSanitizer + UndefinedBehaviorSanitizer by tools/ingest_rgb_check.cpp (a stand-alone program: nothing sanitized is loaded
into Python), its dumped planes against the numpy oracle tests/rgb_csc.py -- which pins the kernel's text, the program's C
restatement and the oracle of tests/test_gpu_enc_rgb.py to one another -- and the arithmetic claims the header makes about the
conversion, over all 2^24 colours.
"""
import os

import numpy as np
import pytest

import rgb_csc as R
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    """builds tools/ingest_rgb_check.cpp with the sanitizers, runs its whole sweep and returns the directory of its dumped cases"""
    out, dump = build_and_run("tools/ingest_rgb_check.cpp", tmp_path_factory.mktemp("ingest_rgb"), ["--dump", "{dump}"])
    assert "in the wide form" in out
    return dump


def test_kernel_body_sweep_is_clean_and_equals_the_numpy_oracle(dump_dir):
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".src"))
    assert len(names) >= 6
    seen = set()
    for name in names:
        order, csc, fmt, size = name.split("_")
        w, h = (int(v) for v in size.split("x"))
        hs, vs = FMT[fmt]
        layout = {"bgra": R.BGRA, "rgba": R.RGBA}[order] | int(csc, 16)
        pixels = np.fromfile(os.path.join(dump_dir, name + ".src"), dtype=np.uint8).reshape(h, w, 4)
        got = np.fromfile(os.path.join(dump_dir, name + ".yuv"), dtype=np.uint8)
        want = np.frombuffer(R.planar_bytes(pixels, layout, hs, vs), dtype=np.uint8)
        assert got.size == want.size, name
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: byte %d of the packed planes is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want[bad[0]])
        seen.add((order, csc, fmt))
    assert {s[0] for s in seen} == {"bgra", "rgba"} and {s[1] for s in seen} == {"000", "100", "200", "300"} and {s[2] for s in seen} == set(FMT)


@pytest.mark.parametrize("csc", R.CSC, ids=["bt601", "bt709", "bt601_full", "bt709_full"])
def test_arithmetic_claims_over_all_colours(csc):
    """Rows and ranges as include/dsv2_hip.h states them: chroma rows sum to 0 (grey gives 128), luma rows to 220 / 256, every
    magnitude fits a byte, every sum is non-negative before its shift; limited range gives Y 16..235 and U, V 16..240 with no clamp
    at work; full range reaches Y 255 exactly and clamps U, V only at the one sum 128 * 255, whose unclamped value is 256."""
    full = bool(csc & R.FULL)
    m = R.MATRIX[csc]
    assert sum(m[0]) == (256 if full else 220) and sum(m[1]) == 0 and sum(m[2]) == 0
    assert all(0 <= abs(c) <= 255 for row in m for c in row)
    g, b = (a.astype(np.int64) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    ymin, ymax, cmin, cmax = 1 << 30, -1, [1 << 30] * 2, [-1] * 2
    for r0 in range(256):
        r = np.full_like(g, r0)
        y = (R.weighted(m[0], r, g, b) + 128 + 256 * R.ybase(csc)) >> 8
        ymin, ymax = min(ymin, int(y.min())), max(ymax, int(y.max()))
        for i in (0, 1):
            s = R.weighted(m[1 + i], r, g, b)
            assert s.min() + 32896 >= 0
            raw = (s + 32896) >> 8
            cmin[i], cmax[i] = min(cmin[i], int(raw.min())), max(cmax[i], int(raw.max()))
            over = raw > 255
            assert np.all(s[over] == 128 * 255) and np.all(raw[over] == 256)
            assert np.array_equal(R.chroma_sum(s, 0), np.minimum(raw, 255))
        assert int((R.weighted(m[1], r, r, r) + 32896).flat[0]) >> 8 == 128 and int((R.weighted(m[2], r, r, r) + 32896).flat[0]) >> 8 == 128
    if full:
        assert (ymin, ymax) == (0, 255) and cmin == [1, 1] and cmax == [256, 256]
    else:
        assert (ymin, ymax) == (16, 235) and cmin == [16, 16] and cmax == [240, 240]
    # a footprint of N equal pixels gives what one pixel gives: the sums and the bias scale alike
    s = np.array([128 * 255, -128 * 255, 0, 12345], dtype=np.int64)
    for n in range(1, 5):
        assert np.array_equal(R.chroma_sum(s << n, n), R.chroma_sum(s, 0))
