"""The float tensor ingest without a GPU: the thread body of k_ingest_tensor (csrc/ingest_tensor.h) compiled for the host and swept
under AddressSanitizer + UndefinedBehaviorSanitizer by tools/ingest_tensor_check.cpp (a stand-alone program: nothing sanitized is
loaded into Python), its dumped planes and bytes against the numpy oracle tests/tensor_in.py; the oracle's own named values; and the
round-trip property include/dsv2_hip.h states: a byte the decoder delivers under the UNIT or the ImageNet constants comes back as the
same byte under the inverse constants, for every byte, channel and float element type.
"""
import os
import re

import numpy as np
import pytest

import rgb_csc as R
import tensor_in as T
import tensor_out as TO
from sanitized_tool import build_and_run

FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0), "410": (2, 2)}
DTYPE = {"f16": T.F16, "bf16": T.BF16, "f32": T.F32}
CONSTANT_SETS = 6  # tools/ingest_tensor_check.cpp: kConsts


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """builds tools/ingest_tensor_check.cpp with the sanitizers, runs its whole sweep and returns (what it printed, the directory of
    its dumps)"""
    return build_and_run("tools/ingest_tensor_check.cpp", tmp_path_factory.mktemp("ingest_tensor"), ["--dump", "{dump}"], timeout=300)


def test_kernel_body_sweep_is_clean(sweep):
    m = re.search(r"ingest_tensor_check: (\d+) cases \((\d+) in the wide form\).* (\d+) element patterns", sweep[0])
    assert m, sweep[0][-1000:]
    cases, wide, patterns = (int(v) for v in m.groups())
    assert cases > 5000 and 0 < wide < cases and patterns > 20_000_000


def test_dumped_planes_equal_the_numpy_oracle(sweep):
    dump = sweep[1]
    names = sorted(f[:-4] for f in os.listdir(dump) if f.endswith(".yuv"))
    assert len(names) >= 10
    seen = set()
    for name in names:
        dt, csc, fmt, size = name.split("_")
        w, h = (int(v) for v in size.split("x"))
        hs, vs = FMT[fmt]
        dtype = DTYPE[dt]
        planes = np.fromfile(os.path.join(dump, name + ".ten"), dtype=T.BITS[dtype]).reshape(3, h, w)
        k = np.fromfile(os.path.join(dump, name + ".const"), dtype=np.float32)
        px = T.picture(list(planes), dtype, k[:3], k[3:])
        got = np.fromfile(os.path.join(dump, name + ".yuv"), dtype=np.uint8)
        want = np.frombuffer(R.planar_bytes(px, R.RGBA | int(csc, 16), hs, vs), dtype=np.uint8)
        assert got.size == want.size, name
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: byte %d of the packed planes is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want[bad[0]])
        seen.add((dt, csc, fmt))
    assert {s[0] for s in seen} == set(DTYPE) and {s[1] for s in seen} == {"000", "100", "200", "300"} and {s[2] for s in seen} == set(FMT)


@pytest.mark.parametrize("dt", sorted(DTYPE))
def test_every_dumped_element_pattern_gives_the_oracles_byte(sweep, dt):
    """all 65 536 binary16 / bfloat16 patterns and two million binary32 ones through the kernel's fetch, under the first plane's
    constants of each of the program's constant sets: the bytes are numpy's"""
    dump, dtype = sweep[1], DTYPE[dt]
    e = np.fromfile(os.path.join(dump, "elems_%s.ten" % dt), dtype=T.BITS[dtype])
    k = np.fromfile(os.path.join(dump, "elems_%s.const" % dt), dtype=np.float32).reshape(CONSTANT_SETS, 6)
    got = np.fromfile(os.path.join(dump, "elems_%s.u8" % dt), dtype=np.uint8).reshape(CONSTANT_SETS, e.size)
    assert e.size >= 65536
    for c in range(CONSTANT_SETS):
        want = T.plane_bytes(e, dtype, k[c][0], k[c][3])
        bad = np.flatnonzero(got[c] != want)
        assert bad.size == 0, "%s element %#x under constant set %d is %d, the oracle says %d" % (dt, e[bad[0]], c, got[c][bad[0]], want[bad[0]])


def test_the_oracle_says_what_the_contract_names():
    f32 = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)
    assert list(T.plane_bytes(f32(0.5, 1.5, 2.5, 254.5, 255.5), T.F32, 1.0, 0.0)) == [0, 2, 2, 254, 255]
    assert list(T.plane_bytes(f32(0.0, -0.0, np.inf, -np.inf, np.nan, -7.0, 1e9), T.F32, 1.0, 0.0)) == [0, 0, 255, 0, 0, 0, 255]
    sub = np.array([0x00400000, 0x00600000], dtype=np.uint32)  # 2^-127, 1.5 * 2^-127
    assert list(T.plane_bytes(sub, T.F32, 2.0 ** 127, 0.0)) == [1, 2]
    assert list(T.plane_bytes((sub >> 16).astype(np.uint16), T.BF16, 2.0 ** 127, 0.0)) == [1, 2]
    assert list(T.plane_bytes(np.array([1, 2, 3], dtype=np.uint16), T.F16, 2.0 ** 23, 0.0)) == [0, 1, 2]  # binary16's subnormals: 0.5, 1, 1.5
    # not fused: 0x438037fd times 1 + 2^-12 is 256.5 + 1.5e-5, which is 256.5 as a product rounded on its own -- with bias -256 the tie
    # 0.5, byte 0; one fused operation would keep the excess, land above the tie and give 1
    assert T.plane_bytes(np.array([0x438037fd], dtype=np.uint32), T.F32, 1 + 2.0 ** -12, -256.0)[0] == 0


@pytest.mark.parametrize("constants", ["unit", "imagenet"])
@pytest.mark.parametrize("dtype", T.FLOATS, ids=["f16", "bf16", "f32"])
def test_round_trip_of_the_decoders_elements(dtype, constants):
    """256 bytes x 3 channels: the decoder's element for byte v under (scale, bias) -- tests/tensor_out.py -- gives v again under
    scale' = 1 / scale, bias' = -bias / scale (for ToTensor + Normalize: 255 * std, 255 * mean)"""
    dec, enc = (TO.UNIT, T.UNIT_INV) if constants == "unit" else (TO.IMAGENET, T.IMAGENET_INV)
    v = np.arange(256, dtype=np.uint8)
    for c in range(3):
        e = TO.elements(v, dtype, dec[0][c], dec[1][c])
        assert np.array_equal(T.plane_bytes(e, dtype, enc[0][c], enc[1][c]), v), (T.NAMES[dtype], constants, c)
    if constants == "imagenet":  # the two ways to write the inverse are one set of binary32 constants
        assert T.inverse(TO.IMAGENET) == tuple(tuple(float(np.float32(x)) for x in part) for part in T.IMAGENET_INV)
