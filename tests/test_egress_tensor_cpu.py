"""The tensor egress without a GPU: the thread body of k_egress_tensor (csrc/egress_tensor.h) compiled for the host and swept under
AddressSanitizer + UndefinedBehaviorSanitizer by tools/egress_tensor_check.cpp (a stand-alone program: nothing sanitized is loaded
into Python) -- both forms x four element types x five formats x four presets over widths, heights, pitches, pointer offsets and
constants, guard bytes around every row -- and its dumped tensors against the numpy oracle tests/tensor_out.py, bit for bit: that pins
the kernel's text, the program's C restatement and the oracle of tests/test_gpu_dec_tensor.py to one another.
"""
import os
import re

import numpy as np
import pytest

import tensor_out as T
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
DTYPE = {name: dt for dt, name in T.NAMES.items()}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/egress_tensor_check.cpp with the sanitizers, runs its whole sweep and returns (what it printed, the directory of
    its dumped cases)"""
    return build_and_run("tools/egress_tensor_check.cpp", tmp_path_factory.mktemp("egress_tensor"), ["--dump", "{dump}"])


def test_kernel_body_sweep_is_clean_in_both_forms(sweep):
    m = re.search(r"egress_tensor_check: (\d+) cases \((\d+) in the wide form\) equal the element-by-element contract", sweep[0])
    assert m, sweep[0][-1000:]
    # 15 widths x 7 heights x 5 formats x 4 presets x 4 element types x 3 pitches x 4 offsets, the general form again wherever the wide
    # one ran, and the named cases
    assert int(m.group(1)) > 15 * 7 * 5 * 4 * 4 * 3 * 4
    assert 0 < int(m.group(2)) < int(m.group(1))


def load(dump_dir, name):
    dt, csc, fmt, size = name.split("_")[:4]
    dtype, (hs, vs) = DTYPE[dt], FMT[fmt]
    w, h = (int(v) for v in size.split("x"))
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    yuv = np.fromfile(os.path.join(dump_dir, name + ".yuv"), dtype=np.uint8)
    assert yuv.size == w * h + 2 * cw * ch, name
    y, u, v = yuv[:w * h].reshape(h, w), yuv[w * h:w * h + cw * ch].reshape(ch, cw), yuv[w * h + cw * ch:].reshape(ch, cw)
    k = np.fromfile(os.path.join(dump_dir, name + ".const"), dtype=np.float32)
    assert k.size == 6
    got = np.fromfile(os.path.join(dump_dir, name + ".ten"), dtype=T.BITS[dtype])
    assert got.size == 3 * w * h, name
    return dtype, int(csc, 16), (hs, vs), (y, u, v), (k[:3], k[3:]), got.reshape(3, h, w)


def test_dumped_cases_equal_the_numpy_oracle(sweep):
    dump_dir = sweep[1]
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".yuv"))
    assert len(names) >= 15
    seen, consts = set(), set()
    for name in names:
        dtype, csc, (hs, vs), (y, u, v), (scale, bias), got = load(dump_dir, name)
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


def test_grey_ramp_holds_every_byte_value_in_every_channel(sweep):
    """full range, U = V = 128: R = G = B = Y, a ramp over all 256 values -- every byte goes through the float contract in every
    element type"""
    dump_dir = sweep[1]
    for dt in T.DTYPES:
        name = "%s_200_420_32x8_ramp" % T.NAMES[dt]
        dtype, csc, (hs, vs), (y, u, v), (scale, bias), got = load(dump_dir, name)
        assert csc == 0x200 and np.all(u == 128) and np.all(v == 128)
        assert sorted(y.reshape(-1).tolist()) == list(range(256))
        for c in range(3):
            assert np.array_equal(got[c], T.elements(y, dtype, scale[c], bias[c]))


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
