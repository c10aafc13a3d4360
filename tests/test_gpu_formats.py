"""Chroma format coverage of the drop-in encoder / decoder: 4:4:4, 4:2:2, 4:2:0, 4:1:1 and the reference's "4:1:0"
(quarter horizontal, quarter vertical, dsv.h:87-95) give bit-identical packets and pictures."""
import os

import numpy as np
import pytest

import dsvabi as A
from codec_run import FMT, decode_stream, encode_stream, frames

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


@pytest.mark.parametrize("name", sorted(FMT))
@pytest.mark.parametrize("w,h", [(352, 288), (176, 144)])
def test_format_bit_exact(name, w, h):
    code, hs, vs = FMT[name]
    ref, hip = A.load_ref(), A.load_hip()
    fr = frames(w, h, hs, vs, 4, 5)
    pr, _ = encode_stream(ref, fr, w, h, code, qp=60, gop=12)
    ph, _ = encode_stream(hip, fr, w, h, code, qp=60, gop=12)
    assert pr == ph
    dr, dh = decode_stream(ref, pr), decode_stream(hip, pr)
    assert len(dr) == len(dh)
    for a, b in zip(dr, dh):
        assert a[0] == b[0]
        for c in (1, 2, 3):
            assert np.array_equal(a[c], b[c])
