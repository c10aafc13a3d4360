"""The RGB egress without a GPU: the thread body of k_egress_rgb (csrc/egress_rgb.h) in its three layouts -- packed four-byte surfaces,
planar [3, h, w] and interleaved [h, w, 3] tensors -- compiled for the host and swept under AddressSanitizer + UndefinedBehaviorSanitizer
by tools/egress_rgb_check.cpp (a stand-alone program: nothing sanitized is loaded into Python): both forms x byte / element orders x
element types x five formats x four presets over widths, heights, pitches, pointer offsets and constants, guard bytes around every row,
every interleaved case also against the planar layout transposed.  Its dumped cases are compared with the numpy oracles bit for bit --
tests/yuv_rgb.py (packed), tests/tensor_out.py (planar), tests/hwc_out.py (interleaved) -- which pins the kernel's text, the program's C
restatement and the oracles of tests/test_gpu_dec_rgb.py, test_gpu_dec_tensor.py and test_gpu_dec_hwc.py to one another.  The
arithmetic claims the headers make about the conversion are checked over all 2^24 (Y, U, V) and, for the round trip behind the
encoder's conversion, all 2^24 (R, G, B); those about the float contract on the oracle itself.
"""
import os
import re

import numpy as np
import pytest

import hwc_out as H
import rgb_csc as R
import tensor_out as T
import yuv_rgb as Q
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
CSC_IDS = ["bt601", "bt709", "bt601_full", "bt709_full"]
DTYPE = {name: dt for dt, name in T.NAMES.items()}
ORDER = {"rgb": H.RGB, "bgr": H.BGR}
# the cases the sweep of each layout runs, at least: packed -- what the program printed before the three layouts shared one body;
# planar: 15 widths x 7 heights x 5 formats x 4 presets x 4 element types x 3 pitches x 4 offsets; interleaved: the same x 2 orders
# (and the general form again wherever the wide one ran, and the named cases, on top)
MIN_CASES = {"packed": 242046, "planar": 15 * 7 * 5 * 4 * 4 * 3 * 4 + 1, "interleaved": 15 * 7 * 5 * 4 * 4 * 2 * 3 * 4 + 1}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/egress_rgb_check.cpp with the sanitizers, runs its whole sweep and returns (what it printed, the directory of its
    dumped cases, one subdirectory per layout)"""
    return build_and_run("tools/egress_rgb_check.cpp", tmp_path_factory.mktemp("egress_rgb"), ["--dump", "{dump}"])


def counts(out):
    m = re.search(r"egress_rgb_check: packed (\d+) cases \((\d+) in the wide form\) equal the pixel-by-pixel conversion, every alpha byte is 255; "
                  r"planar (\d+) cases \((\d+) in the wide form\) equal the element-by-element contract; interleaved (\d+) cases \((\d+) in the wide form\) "
                  r"equal the element-by-element contract and the planar tensor transposed \((\d+)\); no byte outside the rows changed", out)
    assert m, out[-1000:]
    v = [int(g) for g in m.groups()]
    return {"packed": v[0:2], "planar": v[2:4], "interleaved": v[4:6]}, v[6]


@pytest.mark.parametrize("layout", ["packed", "planar", "interleaved"])
def test_kernel_body_sweep_is_clean_in_both_forms(sweep, layout):
    (cases, wide), transposed = counts(sweep[0])[0][layout], counts(sweep[0])[1]
    assert cases >= MIN_CASES[layout]
    assert 0 < wide < cases  # both forms
    if layout == "interleaved":
        assert transposed == cases  # every interleaved case equals the planar layout transposed


def names(dump_dir, layout):
    d = os.path.join(dump_dir, layout)
    return d, sorted(f[:-4] for f in os.listdir(d) if f.endswith(".yuv"))


def planes(d, name, w, h, hs, vs):
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    yuv = np.fromfile(os.path.join(d, name + ".yuv"), dtype=np.uint8)
    assert yuv.size == w * h + 2 * cw * ch, name
    return yuv[:w * h].reshape(h, w), yuv[w * h:w * h + cw * ch].reshape(ch, cw), yuv[w * h + cw * ch:].reshape(ch, cw)


def test_packed_cases_equal_the_numpy_oracle(sweep):
    d, found = names(sweep[1], "packed")
    assert len(found) >= 6
    seen = set()
    for name in found:
        order, csc, fmt, size = name.split("_")
        w, h = (int(v) for v in size.split("x"))
        hs, vs = FMT[fmt]
        layout = {"bgra": Q.BGRA, "rgba": Q.RGBA}[order] | int(csc, 16)
        y, u, v = planes(d, name, w, h, hs, vs)
        got = np.fromfile(os.path.join(d, name + ".rgb"), dtype=np.uint8)
        want = Q.convert(y, u, v, layout, hs, vs).reshape(-1)
        assert got.size == want.size, name
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: byte %d of the pixels is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want[bad[0]])
        assert want.min() == 0 and want.reshape(h, w, 4)[..., :3].max() == 255  # (both clamps are in every dumped case)
        seen.add((order, csc, fmt))
    assert {s[0] for s in seen} == {"bgra", "rgba"} and {s[1] for s in seen} == {"000", "100", "200", "300"} and {s[2] for s in seen} == set(FMT)


def load_planar(d, name):
    dt, csc, fmt, size = name.split("_")[:4]
    dtype, (hs, vs) = DTYPE[dt], FMT[fmt]
    w, h = (int(v) for v in size.split("x"))
    y, u, v = planes(d, name, w, h, hs, vs)
    k = np.fromfile(os.path.join(d, name + ".const"), dtype=np.float32)
    assert k.size == 6
    got = np.fromfile(os.path.join(d, name + ".ten"), dtype=T.BITS[dtype])
    assert got.size == 3 * w * h, name
    return dtype, int(csc, 16), (hs, vs), (y, u, v), (k[:3], k[3:]), got.reshape(3, h, w)


def load_interleaved(d, name):
    dt, order, csc, fmt, size = name.split("_")[:5]
    dtype, (hs, vs) = DTYPE[dt], FMT[fmt]
    w, h = (int(v) for v in size.split("x"))
    y, u, v = planes(d, name, w, h, hs, vs)
    k = np.fromfile(os.path.join(d, name + ".const"), dtype=np.float32)
    assert k.size == 6
    got = np.fromfile(os.path.join(d, name + ".hwc"), dtype=T.BITS[dtype])
    assert got.size == 3 * w * h, name
    return dtype, ORDER[order], int(csc, 16), (hs, vs), (y, u, v), (k[:3], k[3:]), got.reshape(h, w, 3)


def test_planar_cases_equal_the_numpy_oracle(sweep):
    d, found = names(sweep[1], "planar")
    assert len(found) >= 15
    seen, consts = set(), set()
    for name in found:
        dtype, csc, (hs, vs), (y, u, v), (scale, bias), got = load_planar(d, name)
        want = np.stack(T.tensor(y, u, v, csc, hs, vs, dtype, scale, bias))
        assert want.dtype == got.dtype and want.shape == got.shape, name
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: element (x=%d, y=%d) of plane %d is %#x, the oracle says %#x (%d differ)" % (
            name, bad[0][2], bad[0][1], bad[0][0], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
        if dtype == T.U8:
            assert all(p.min() == 0 and p.max() == 255 for p in got), name  # (both clamps are in every dumped U8 case, in every channel)
        seen.add((dtype, csc, (hs, vs)))
        consts.add((tuple(float(s) for s in scale), tuple(float(b) for b in bias)))
    assert {s[0] for s in seen} == set(T.DTYPES) and {s[1] for s in seen} == {0x000, 0x100, 0x200, 0x300} and {s[2] for s in seen} == set(FMT.values())
    for scale, bias in (T.UNIT, T.IMAGENET, T.TINY, T.HUGE):
        assert (tuple(float(np.float32(s)) for s in scale), tuple(float(np.float32(b)) for b in bias)) in consts


def test_interleaved_cases_equal_the_numpy_oracle(sweep):
    d, found = names(sweep[1], "interleaved")
    assert len(found) >= 19
    seen, consts = set(), set()
    for name in found:
        dtype, order, csc, (hs, vs), (y, u, v), (scale, bias), got = load_interleaved(d, name)
        want = H.hwc(y, u, v, csc, hs, vs, dtype, order, scale, bias)
        assert want.dtype == got.dtype and want.shape == got.shape, name
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: element %d of pixel (x=%d, y=%d) is %#x, the oracle says %#x (%d differ)" % (
            name, bad[0][2], bad[0][1], bad[0][0], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
        if dtype == T.U8 and not name.endswith("_ramp"):
            assert all(got[..., e].min() == 0 and got[..., e].max() == 255 for e in range(3)), name  # (both clamps, every element)
        seen.add((dtype, order, csc, (hs, vs)))
        consts.add((tuple(float(s) for s in scale), tuple(float(b) for b in bias)))
    assert {s[0] for s in seen} == set(T.DTYPES) and {s[1] for s in seen} == set(H.ORDERS)
    assert {s[2] for s in seen} == {0x000, 0x100, 0x200, 0x300} and {s[3] for s in seen} == set(FMT.values())
    for scale, bias in (T.UNIT, T.IMAGENET, T.TINY, T.HUGE):
        assert (tuple(float(np.float32(s)) for s in scale), tuple(float(np.float32(b)) for b in bias)) in consts


def test_planar_grey_ramp_holds_every_byte_value_in_every_channel(sweep):
    """full range, U = V = 128: R = G = B = Y, a ramp over all 256 values -- every byte goes through the float contract in every
    element type"""
    d = os.path.join(sweep[1], "planar")
    for dt in T.DTYPES:
        dtype, csc, (hs, vs), (y, u, v), (scale, bias), got = load_planar(d, "%s_200_420_32x8_ramp" % T.NAMES[dt])
        assert csc == 0x200 and np.all(u == 128) and np.all(v == 128)
        assert sorted(y.reshape(-1).tolist()) == list(range(256))
        for c in range(3):
            assert np.array_equal(got[c], T.elements(y, dtype, scale[c], bias[c]))


def test_interleaved_grey_ramp_holds_every_byte_value_in_every_element(sweep):
    """the same in every element type, order and element position"""
    d = os.path.join(sweep[1], "interleaved")
    for dt in T.DTYPES:
        for order in H.ORDERS:
            dtype, o, csc, _, (y, u, v), (scale, bias), got = load_interleaved(d, "%s_%s_200_420_32x8_ramp" % (T.NAMES[dt], H.ORDER_NAMES[order]))
            assert o == order and csc == 0x200 and np.all(u == 128) and np.all(v == 128)
            assert sorted(y.reshape(-1).tolist()) == list(range(256))
            for e in range(3):
                assert np.array_equal(got[..., e], T.elements(y, dtype, scale[e], bias[e]))


# ---- the oracles' own claims --------------------------------------------------------------------------------------------------------
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


def test_the_oracle_tells_a_fused_multiply_add_apart():
    """scale = 1 / (255 * 0.229) with a bias: for some bytes the two roundings of the contract and the single one of a fused
    multiply-add differ in binary32, so a kernel that fuses them cannot pass"""
    s, b = np.float32(T.IMAGENET[0][0]), np.float32(T.IMAGENET[1][0])
    v = np.arange(256, dtype=np.uint8)
    two = T.elements(v, T.F32, s, b)
    fused = (v.astype(np.float64) * np.float64(s) + np.float64(b)).astype(np.float32).view(np.uint32)  # (the product is exact in binary64)
    assert np.any(two != fused)


def test_binary16_edges_of_the_oracle():
    v = np.arange(256, dtype=np.uint8)
    tiny = T.elements(v, T.F16, *[np.float32(k[0]) for k in T.TINY])
    assert tiny[0] == 0 and np.any(tiny == 0) and np.any((tiny > 0) & (tiny < 0x0400))  # zeros and subnormals
    huge = T.elements(v, T.F16, *[np.float32(k[0]) for k in T.HUGE])
    assert np.any(huge == 0x7c00) and huge[0] == 0xc500  # +infinity; -5.0
    assert T.elements(np.array([255], dtype=np.uint8), T.BF16, np.float32(1 / 255), np.float32(0))[0] == 0x3f80


def test_the_interleaved_oracle_is_the_planar_one_interleaved():
    """hwc_out.hwc is tensor_out.tensor with element k taken from the channel the order puts there and the constants of element k"""
    rng = np.random.default_rng(5)
    y, u, v = rng.integers(0, 256, (6, 10), dtype=np.uint8), rng.integers(0, 256, (3, 5), dtype=np.uint8), rng.integers(0, 256, (3, 5), dtype=np.uint8)
    for dt in T.DTYPES:
        planes_ = T.tensor(y, u, v, 0x100, 1, 1, dt, *T.IMAGENET)
        assert all(np.array_equal(H.hwc(y, u, v, 0x100, 1, 1, dt, H.RGB, *T.IMAGENET)[..., c], planes_[c]) for c in range(3))
        bgr = H.hwc(y, u, v, 0x100, 1, 1, dt, H.BGR, T.IMAGENET[0][::-1], T.IMAGENET[1][::-1])
        assert all(np.array_equal(bgr[..., 2 - c], planes_[c]) for c in range(3))
