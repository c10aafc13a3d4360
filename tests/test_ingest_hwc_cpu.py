"""The interleaved float tensor ingest without a GPU: the thread body of k_ingest_hwc (csrc/ingest_hwc.h) compiled for the host and swept
under AddressSanitizer + UndefinedBehaviorSanitizer by tools/ingest_hwc_check.cpp (a stand-alone program: nothing sanitized is loaded
into Python), its dumped planes against the numpy oracle tests/hwc_in.py; the oracle's own named values by position; and the round-trip
property include/dsv2_hip.h states: an element the decoder delivers through dsv2hip_dec_batch_hwc under the UNIT or the ImageNet
constants (tests/hwc_out.py) comes back as the same byte under the inverse constants, for every byte, position, order and float
element type.
"""
import os
import re

import numpy as np
import pytest

import hwc_in as H
import hwc_out as HO
import rgb_csc as R
import tensor_in as T
import tensor_out as TO
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
DTYPE = {"f16": H.F16, "bf16": H.BF16, "f32": H.F32}
ORDER = {"rgb": H.RGB, "bgr": H.BGR}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/ingest_hwc_check.cpp with the sanitizers, runs its whole sweep and returns (what it printed, the directory of its
    dumps)"""
    return build_and_run("tools/ingest_hwc_check.cpp", tmp_path_factory.mktemp("ingest_hwc"), ["--dump", "{dump}"], timeout=300)


def test_kernel_body_sweep_is_clean(sweep):
    m = re.search(r"ingest_hwc_check: (\d+) cases \((\d+) in the wide form\) equal the contract and the conversion restated and the planar body", sweep[0])
    assert m, sweep[0][-1000:]
    cases, wide = (int(v) for v in m.groups())
    assert cases > 10000 and 0 < wide < cases


def test_dumped_planes_equal_the_numpy_oracle(sweep):
    dump = sweep[1]
    names = sorted(f[:-4] for f in os.listdir(dump) if f.endswith(".yuv"))
    assert len(names) >= 10
    seen = set()
    for name in names:
        dt, order, csc, fmt, size = name.split("_")
        w, h = (int(v) for v in size.split("x"))
        hs, vs = FMT[fmt]
        dtype = DTYPE[dt]
        hwc = np.fromfile(os.path.join(dump, name + ".hwc"), dtype=H.BITS[dtype]).reshape(h, w, 3)
        k = np.fromfile(os.path.join(dump, name + ".const"), dtype=np.float32)
        assert len({float(v) for v in k[:3]} | {float(v) for v in k[3:]}) >= 3  # (constants that differ by position: a swapped index shows)
        px = H.picture(hwc, dtype, ORDER[order], k[:3], k[3:])
        got = np.fromfile(os.path.join(dump, name + ".yuv"), dtype=np.uint8)
        want = np.frombuffer(R.planar_bytes(px, R.RGBA | int(csc, 16), hs, vs), dtype=np.uint8)
        assert got.size == want.size, name
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: byte %d of the packed planes is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want[bad[0]])
        seen.add((dt, order, csc, fmt))
    assert {s[0] for s in seen} == set(DTYPE) and {s[1] for s in seen} == set(ORDER)
    assert {s[2] for s in seen} == {"000", "100", "200", "300"} and {s[3] for s in seen} == set(FMT)


@pytest.mark.parametrize("order", H.ORDERS, ids=H.ORDER_NAMES.values())
def test_the_oracle_says_what_the_contract_names_by_position(order):
    """one row of four pixels under three different constant pairs by position: ties at position 0, the subnormals 2^-127 and
    1.5 * 2^-127 under 2^127, a NaN and +inf at position 1, the fusion-sensitive element, -inf and -0 at position 2; the channel a
    position's byte lands in is the order's"""
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)
    hwc = np.zeros((1, 4, 3), dtype=np.uint32)
    hwc[0, :, 0] = f(0.5, 1.5, 2.5, 254.5)
    hwc[0, :, 1] = [0x00400000, 0x00600000, 0x7fc00000, 0x7f800000]
    hwc[0, :, 2] = [0x438037fd, 0xff800000, f(258.0)[0], 0x80000000]
    px = H.picture(hwc, H.F32, order, (1.0, 2.0 ** 127, 1 + 2.0 ** -12), (0.0, 0.0, -256.0))
    ch = H.channel_of(order)
    assert list(px[0, :, ch[0]]) == [0, 2, 2, 254]
    assert list(px[0, :, ch[1]]) == [1, 2, 0, 255]
    assert list(px[0, :, ch[2]]) == [0, 0, 2, 0]  # (0x438037fd: 0 unfused, 1 fused -- tests/test_ingest_tensor_cpu.py says why)
    assert not px[..., 3].any()


def test_interleave_and_planes_of_are_inverse_and_constants_follow_the_order():
    planes = [np.full((2, 3), c, dtype=np.uint16) for c in range(3)]
    for order in H.ORDERS:
        hwc = H.interleave(planes, order)
        assert list(hwc[0, 0]) == list(H.channel_of(order)) and hwc.shape == (2, 3, 3)
        assert all(np.array_equal(a, b) for a, b in zip(H.planes_of(hwc, order), planes))
    assert H.by_position((10, 20, 30), H.BGR) == (30, 20, 10) and H.by_position((10, 20, 30), H.RGB) == (10, 20, 30)


@pytest.mark.parametrize("order", H.ORDERS, ids=H.ORDER_NAMES.values())
@pytest.mark.parametrize("constants", ["unit", "imagenet"])
@pytest.mark.parametrize("dtype", T.FLOATS, ids=["f16", "bf16", "f32"])
def test_round_trip_of_the_decoders_interleaved_elements(dtype, constants, order):
    """256 bytes x 3 positions: the decoder's interleaved tensor (tests/hwc_out.py's hwc) of a grey ramp -- full-range BT.601 makes R =
    G = B = Y of it, so every position sees every byte -- under (scale, bias) by position gives the bytes again under scale'[k] = 1 /
    scale[k], bias'[k] = -bias[k] / scale[k]; a BGR consumer holds ImageNet's constants in B, G, R order on both sides"""
    dec = H.by_position(TO.UNIT[0], order), H.by_position(TO.UNIT[1], order)
    if constants == "imagenet":
        dec = H.by_position(TO.IMAGENET[0], order), H.by_position(TO.IMAGENET[1], order)
    enc = T.inverse(dec)
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    grey = np.full((16, 16), 128, dtype=np.uint8)
    hwc = HO.hwc(y, grey, grey, R.FULL, 0, 0, dtype, order, dec[0], dec[1])
    assert hwc.shape == (16, 16, 3) and hwc.dtype == H.BITS[dtype]
    px = H.picture(hwc, dtype, order, enc[0], enc[1])
    for c in range(3):
        assert np.array_equal(px[..., c], y), (T.NAMES[dtype], constants, H.ORDER_NAMES[order], c)
    if constants == "imagenet":  # (the inverse by position is tensor_in's folded constants, permuted)
        assert enc == tuple(tuple(float(np.float32(x)) for x in H.by_position(part, order)) for part in T.IMAGENET_INV)
