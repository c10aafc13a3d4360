"""The interleaved tensor egress without a GPU: the thread body of k_egress_hwc (csrc/egress_hwc.h) compiled for the host and swept
under AddressSanitizer + UndefinedBehaviorSanitizer by tools/egress_hwc_check.cpp (a stand-alone program: nothing sanitized is loaded
into Python) -- both forms x four element types x two orders x five formats x four presets over widths, heights, pitches, pointer
offsets and constants, guard bytes around every row, every case also against egress_tensor.h's planar body transposed -- and its
dumped tensors against the numpy oracle tests/hwc_out.py, bit for bit: that pins the kernel's text, the program's C restatement and
the oracle of tests/test_gpu_dec_hwc.py to one another.
"""
import os
import re

import numpy as np
import pytest

import hwc_out as H
import tensor_out as T
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
DTYPE = {name: dt for dt, name in T.NAMES.items()}
ORDER = {"rgb": H.RGB, "bgr": H.BGR}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/egress_hwc_check.cpp with the sanitizers, runs its whole sweep and returns (what it printed, the directory of its
    dumped cases)"""
    return build_and_run("tools/egress_hwc_check.cpp", tmp_path_factory.mktemp("egress_hwc"), ["--dump", "{dump}"])


def test_kernel_body_sweep_is_clean_in_both_forms(sweep):
    m = re.search(r"egress_hwc_check: (\d+) cases \((\d+) in the wide form\) equal the element-by-element contract and the planar tensor "
                  r"transposed \((\d+)\)", sweep[0])
    assert m, sweep[0][-1000:]
    # 15 widths x 7 heights x 5 formats x 4 presets x 4 element types x 2 orders x 3 pitches x 4 offsets, the general form again wherever
    # the wide one ran, and the named cases
    assert int(m.group(1)) > 15 * 7 * 5 * 4 * 4 * 2 * 3 * 4
    assert 0 < int(m.group(2)) < int(m.group(1))
    assert int(m.group(3)) == int(m.group(1))


def load(dump_dir, name):
    dt, order, csc, fmt, size = name.split("_")[:5]
    dtype, (hs, vs) = DTYPE[dt], FMT[fmt]
    w, h = (int(v) for v in size.split("x"))
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    yuv = np.fromfile(os.path.join(dump_dir, name + ".yuv"), dtype=np.uint8)
    assert yuv.size == w * h + 2 * cw * ch, name
    y, u, v = yuv[:w * h].reshape(h, w), yuv[w * h:w * h + cw * ch].reshape(ch, cw), yuv[w * h + cw * ch:].reshape(ch, cw)
    k = np.fromfile(os.path.join(dump_dir, name + ".const"), dtype=np.float32)
    assert k.size == 6
    got = np.fromfile(os.path.join(dump_dir, name + ".hwc"), dtype=T.BITS[dtype])
    assert got.size == 3 * w * h, name
    return dtype, ORDER[order], int(csc, 16), (hs, vs), (y, u, v), (k[:3], k[3:]), got.reshape(h, w, 3)


def test_dumped_cases_equal_the_numpy_oracle(sweep):
    dump_dir = sweep[1]
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".yuv"))
    assert len(names) >= 19
    seen, consts = set(), set()
    for name in names:
        dtype, order, csc, (hs, vs), (y, u, v), (scale, bias), got = load(dump_dir, name)
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


def test_grey_ramp_holds_every_byte_value_in_every_element(sweep):
    """full range, U = V = 128: R = G = B = Y, a ramp over all 256 values -- every byte goes through the float contract in every
    element type, order and element position"""
    dump_dir = sweep[1]
    for dt in T.DTYPES:
        for order in H.ORDERS:
            name = "%s_%s_200_420_32x8_ramp" % (T.NAMES[dt], H.ORDER_NAMES[order])
            dtype, o, csc, _, (y, u, v), (scale, bias), got = load(dump_dir, name)
            assert o == order and csc == 0x200 and np.all(u == 128) and np.all(v == 128)
            assert sorted(y.reshape(-1).tolist()) == list(range(256))
            for e in range(3):
                assert np.array_equal(got[..., e], T.elements(y, dtype, scale[e], bias[e]))


def test_the_oracle_is_the_planar_one_interleaved():
    """hwc_out.hwc is tensor_out.tensor with element k taken from the channel the order puts there and the constants of element k"""
    rng = np.random.default_rng(5)
    y, u, v = rng.integers(0, 256, (6, 10), dtype=np.uint8), rng.integers(0, 256, (3, 5), dtype=np.uint8), rng.integers(0, 256, (3, 5), dtype=np.uint8)
    for dt in T.DTYPES:
        planes = T.tensor(y, u, v, 0x100, 1, 1, dt, *T.IMAGENET)
        assert all(np.array_equal(H.hwc(y, u, v, 0x100, 1, 1, dt, H.RGB, *T.IMAGENET)[..., c], planes[c]) for c in range(3))
        bgr = H.hwc(y, u, v, 0x100, 1, 1, dt, H.BGR, T.IMAGENET[0][::-1], T.IMAGENET[1][::-1])
        assert all(np.array_equal(bgr[..., 2 - c], planes[c]) for c in range(3))
