"""The RGB egress without a GPU: the thread body of k_egress_rgb (csrc/egress_rgb.h) compiled for the host and swept under
AddressSanitizer + UndefinedBehaviorSanitizer by tools/egress_rgb_check.cpp (a stand-alone program: nothing sanitized is loaded
into Python), its dumped surfaces against the numpy oracle tests/yuv_rgb.py -- which pins the kernel's text, the program's C
restatement and the oracle of tests/test_gpu_dec_rgb.py to one another -- and the arithmetic claims the header makes about the
conversion, over all 2^24 (Y, U, V) and, for the round trip behind the encoder's conversion, all 2^24 (R, G, B).
"""
import os

import numpy as np
import pytest

import rgb_csc as R
import yuv_rgb as Q
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
CSC_IDS = ["bt601", "bt709", "bt601_full", "bt709_full"]


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    """builds tools/egress_rgb_check.cpp with the sanitizers, runs its whole sweep and returns the directory of its dumped cases"""
    out, dump = build_and_run("tools/egress_rgb_check.cpp", tmp_path_factory.mktemp("egress_rgb"), ["--dump", "{dump}"])
    assert "in the wide form" in out
    return dump


def test_kernel_body_sweep_is_clean_and_equals_the_numpy_oracle(dump_dir):
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".yuv"))
    assert len(names) >= 6
    seen = set()
    for name in names:
        order, csc, fmt, size = name.split("_")
        w, h = (int(v) for v in size.split("x"))
        hs, vs = FMT[fmt]
        cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
        layout = {"bgra": Q.BGRA, "rgba": Q.RGBA}[order] | int(csc, 16)
        yuv = np.fromfile(os.path.join(dump_dir, name + ".yuv"), dtype=np.uint8)
        assert yuv.size == w * h + 2 * cw * ch, name
        y, u, v = yuv[:w * h].reshape(h, w), yuv[w * h:w * h + cw * ch].reshape(ch, cw), yuv[w * h + cw * ch:].reshape(ch, cw)
        got = np.fromfile(os.path.join(dump_dir, name + ".rgb"), dtype=np.uint8)
        want = Q.convert(y, u, v, layout, hs, vs).reshape(-1)
        assert got.size == want.size, name
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: byte %d of the pixels is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want[bad[0]])
        assert want.min() == 0 and want.reshape(h, w, 4)[..., :3].max() == 255  # (both clamps are in every dumped case)
        seen.add((order, csc, fmt))
    assert {s[0] for s in seen} == {"bgra", "rgba"} and {s[1] for s in seen} == {"000", "100", "200", "300"} and {s[2] for s in seen} == set(FMT)


def all_uv():
    return tuple(a.astype(np.int64) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))


# include/dsv2_hip.h: the extremes of C + rv*E, C + gu*D + gv*E and C + bu*D over all presets and all (Y, U, V); with the rounding
# constant on top that is -73 888 ... 140 057 at the shift
SUM_RANGE = (-74016, 139929)


@pytest.mark.parametrize("csc", Q.CSC, ids=CSC_IDS)
def test_arithmetic_claims_over_all_yuv(csc):
    """The sums' range (24-bit signed multiply-adds suffice), greys, and the ends of the luma range, as include/dsv2_hip.h states
    them."""
    full = bool(csc & Q.FULL)
    ky, ybase, rv, gu, gv, bu = Q.COEFS[csc]
    assert all(abs(c) < 1024 for c in (ky, rv, gu, gv, bu))
    u, v = all_uv()
    lo, hi = 1 << 40, -(1 << 40)
    for y0 in range(256):
        s = Q.sums(csc, np.full_like(u, y0), u, v)
        lo, hi = min(lo, min(int(a.min()) for a in s) - 128), max(hi, max(int(a.max()) for a in s) - 128)
    assert SUM_RANGE[0] <= lo and hi <= SUM_RANGE[1]
    assert -(1 << 23) < lo and hi + 128 < (1 << 23)
    test_arithmetic_claims_over_all_yuv.seen[csc] = (lo, hi)
    grey = np.arange(256)
    mid = np.full(256, 128)
    r, g, b = Q.rgb(csc, grey, mid, mid)
    assert np.array_equal(r, g) and np.array_equal(g, b)  # U = V = 128 gives R = G = B
    if full:
        assert np.array_equal(r, grey)  # a grey Y gives Y exactly
    else:
        assert r[16] == 0 and r[235] == 255
        assert np.all(r[:16] == 0) and np.all(r[235:] == 255) and np.all(np.diff(r[16:236].astype(int)) >= 1)


test_arithmetic_claims_over_all_yuv.seen = {}


def test_the_stated_sum_range_is_reached():
    """-74 016 and 139 929 are the extremes over the four presets, not merely bounds"""
    seen = test_arithmetic_claims_over_all_yuv.seen
    if len(seen) < len(Q.CSC):  # (run on its own: measure here)
        u, v = all_uv()
        for csc in Q.CSC:
            ends = [Q.sums(csc, np.full_like(u, y0), u, v) for y0 in (0, 255)]  # (the sums are monotonic in Y: ky > 0)
            seen[csc] = (min(int(a.min()) for s in ends for a in s) - 128, max(int(a.max()) for s in ends for a in s) - 128)
    assert (min(lo for lo, _ in seen.values()), max(hi for _, hi in seen.values())) == SUM_RANGE


ROUND_TRIP = {False: (2, 2, 3), True: (2, 1, 2)}  # include/dsv2_hip.h: max |error| of R, G, B; limited / full range


@pytest.mark.parametrize("csc", Q.CSC, ids=CSC_IDS)
def test_round_trip_behind_the_encoders_conversion(csc):
    """All 2^24 colours through the encoder's forward conversion at 4:4:4 (tests/rgb_csc.py: one pixel per chroma sample) and back:
    two specifications, neither the code under test."""
    g, b = all_uv()
    worst = [0, 0, 0]
    m = R.MATRIX[csc]
    for r0 in range(256):
        r = np.full_like(g, r0)
        y = R.luma(csc, r, g, b)
        u, v = (R.chroma_sum(R.weighted(row, r, g, b), 0) for row in m[1:])
        assert 0 <= y.min() and y.max() <= 255
        back = Q.rgb(csc, y, u, v)
        for k, (want, got) in enumerate(zip((r, g, b), back)):
            worst[k] = max(worst[k], int(np.abs(want - got.astype(np.int64)).max()))
    bound = ROUND_TRIP[bool(csc & Q.FULL)]
    assert tuple(worst) == bound  # (every preset reaches its range's bound in every channel)


def test_convert_replicates_chroma_over_the_encoders_footprint():
    """pixel (x, y) takes chroma sample (x >> hs, y >> vs), at odd sizes too, and the byte orders differ in bytes 0 and 2 only"""
    rng = np.random.default_rng(1)
    for (hs, vs) in FMT.values():
        w, h = 7, 5
        cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
        y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))
        a, b = Q.convert(y, u, v, Q.BGRA | Q.BT709, hs, vs), Q.convert(y, u, v, Q.RGBA | Q.BT709, hs, vs)
        assert np.array_equal(a[..., [2, 1, 0, 3]], b) and np.all(a[..., 3] == 255)
        for yy in range(h):
            for xx in range(w):
                want = Q.rgb(Q.BT709, y[yy, xx:xx + 1], u[yy >> vs, (xx >> hs):(xx >> hs) + 1], v[yy >> vs, (xx >> hs):(xx >> hs) + 1])
                assert tuple(int(c[0]) for c in want) == tuple(int(c) for c in b[yy, xx, :3])
