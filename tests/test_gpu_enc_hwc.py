"""Interleaved RGB float tensors (dsv2hip_in_hwc: [h, w, 3] of binary16, bfloat16, binary32, R G B or B G R, under constants per
element position) as encoder input, bit for bit: the packets are the reference encoder's on the planar picture that the conversion of
include/dsv2_hip.h makes of the BYTES the contract makes of the elements (tests/hwc_in.py: the numpy oracle; tests/rgb_csc.py under
RGBA | csc) -- both forms of k_ingest_hwc, the three element types, both orders, the four presets, the five chroma formats, the
smallest pictures and footprints half outside them (lossless, so every LSB reaches the packets), ties, infinities, NaNs, out-of-range
values and subnormals by position, the planar tensor call on the de-interleaved picture, the decoder's own interleaved output under the
inverse constants, torch tensors read in place, a step that mixes everything, the uint8 tensor that is the three-byte surface; the
tensor is never written, padding is never an element, a refused call touches nothing.  The shapes are those of
tests/test_gpu_enc_tensor.py; encoders and the reference's driver are tests/enc_in.py's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dsvabi as A
import hwc_in as H
import hwc_out as HO
import rgb_csc as R
import tensor_in as T
import tensor_out as TO
from codec_run import FMT
from dec_out import aligned, planar_oracle, stream
from edge_cases import stream_inverse_is_undefined
from enc_in import CFG, LOSSLESS, Rgb3Surface, encode_steps, encoders, planes_equal_oracle, rgb_content, rgb_ref_packets, same_packets
from hipabi import bind as bind_surfaces, enc_rgb3_forms as rgb3_forms, enc_rgb_forms as rgb_forms, enc_yuv_forms as yuv_forms, mk_buf, reset_enc_forms

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

F16, BF16, F32, U8 = H.F16, H.BF16, H.F32, H.U8
RGB, BGR = H.RGB, H.BGR
DTYPE_IDS = {F16: "f16", BF16: "bf16", F32: "f32"}
ORDER_IDS = [H.ORDER_NAMES[o] for o in H.ORDERS]
# by POSITION, three different pairs in every set but the first: the inverse of UNIT; the inverse of ImageNet's; near identity; mixed, with
# a negative scale
CONSTANTS = (T.UNIT_INV, T.IMAGENET_INV, ((1.0, 0.5, 2.0), (0.0, 1.0, -1.0)), ((-255.0, 127.5, 300.0), (255.0, 10.25, -20.0)))


def lib():
    hip = H.bind(T.bind(bind_surfaces(A.load_hip())))
    reset_enc_forms(hip)
    T.tensor_forms(hip, reset=True)
    H.hwc_forms(hip, reset=True)
    return hip


def four_byte(order):
    """the four-byte layout that names the colours of bytes 0..2 as the order names elements 0..2 (tests/rgb3_csc.py's widen)"""
    return R.BGRA if order == BGR else R.RGBA


def others_did_not_move(hip):
    """the counters of every other ingest"""
    return rgb3_forms(hip) == (0, 0, 0, 0) and rgb_forms(hip) == (0, 0) and yuv_forms(hip) == (0, 0) and T.tensor_forms(hip) == (0, 0)


@functools.lru_cache(maxsize=None)
def tensors(w, h, nfr, seed, dtype, order, k):
    """nfr tensors (h x w x 3 bit patterns of `order`) near rgb_content's pictures under constant set k, and the pictures their bytes ARE"""
    scale, bias = CONSTANTS[k]
    hwcs = tuple(H.tensor_near(px, dtype, order, scale, bias, 100 * seed + t) for t, px in enumerate(rgb_content(w, h, nfr, seed)))
    pictures = tuple(H.picture(t, dtype, order, scale, bias) for t in hwcs)
    for p in pictures:
        assert len(np.unique(p[..., :3])) > 32, "broken test case: the tensor's bytes are nearly constant"
    return hwcs, pictures


@functools.lru_cache(maxsize=None)
def expected(w, h, nfr, seed, dtype, order, k, csc, name, lossless=False):
    """the real reference encoder on the planar pictures the conversion makes of the oracle's bytes"""
    return tuple(rgb_ref_packets(tensors(w, h, nfr, seed, dtype, order, k)[1], R.RGBA | csc, name, LOSSLESS if lossless else CFG))


def encode(hip, hwcs, dtype, order, csc, k, name, cfg=CFG, fill=H.GUARD, **where):
    """one encoder over the tensors `hwcs`, each in an HwcIn(**where); frees the encoder"""
    h, w = hwcs[0].shape[:2]
    encs = encoders(hip, w, h, name, 1, cfg)
    scale, bias = CONSTANTS[k]
    got = H.encode_hwc_steps(hip, encs, lambda s, t: H.HwcIn(hwcs[t], dtype, order, csc, scale, bias, fill=fill, **where), len(hwcs))
    hip.dsv_enc_free(C.byref(encs[0]))
    return got[0]


# ---- 1. wide form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", H.ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("dtype", H.FLOATS, ids=DTYPE_IDS.values())
def test_wide_form_equals_reference(dtype, order):
    """352x288 4:2:0, three frames, the pointer on a 16-byte boundary and the pitch a multiple of 16: three 8 / 16-byte loads a row; the
    hwc counter reads (3, 0), the counters of the surfaces and of the planar tensors do not move."""
    hip = lib()
    k = (H.FLOATS.index(dtype) + H.ORDERS.index(order)) % 2
    hwcs, _ = tensors(352, 288, 3, 5, dtype, order, k)
    got = encode(hip, hwcs, dtype, order, R.BT709, k, "420", **H.wide_pitch(352, dtype))
    same_packets(expected(352, 288, 3, 5, dtype, order, k, R.BT709, "420"), got)
    assert H.hwc_forms(hip) == (3, 0)
    assert others_did_not_move(hip)


# ---- 2. general form, every format -------------------------------------------------------------------------------------------------
GENERAL = [(354, 290, "420")] + [(176, 144, name) for name in sorted(FMT)]


@pytest.mark.parametrize("dtype", H.FLOATS, ids=DTYPE_IDS.values())
@pytest.mark.parametrize("i,w,h,name", [(i,) + g for i, g in enumerate(GENERAL)], ids=["%dx%d-%s" % g for g in GENERAL])
def test_general_form_equals_reference(i, w, h, name, dtype):
    """The pointer 1, 2 or 3 elements behind a 16-byte boundary and the pitch the row plus 1, 2 or 3 elements; a 354-pixel row is more than
    one pass of the workgroup (256 pixels), its last pass partial, and its last thread holds two pixels of four.  Orders, presets and
    constants rotate across the cases."""
    hip = lib()
    turn = i + H.FLOATS.index(dtype)
    order, csc, k = H.ORDERS[turn % 2], R.CSC[turn % 4], turn % len(CONSTANTS)
    hwcs, _ = tensors(w, h, 3, 5, dtype, order, k)
    got = encode(hip, hwcs, dtype, order, csc, k, name, **H.general_pitch(w, dtype, turn))
    same_packets(expected(w, h, 3, 5, dtype, order, k, csc, name), got)
    assert H.hwc_forms(hip) == (0, 3) and others_did_not_move(hip)


# ---- 3. smallest pictures, clamped footprints: lossless -------------------------------------------------------------------------------
SMALL = ([(16, 16, name, form) for name in sorted(FMT) for form in ("wide", "general")] +
         [(22, 22, "411", "general"), (22, 22, "410", "general"), (22, 18, "420", "general")])


@pytest.mark.parametrize("w,h,name,form", SMALL, ids=["%dx%d-%s-%s" % s for s in SMALL])
def test_smallest_pictures_lossless(w, h, name, form):
    """16x16 in both forms; 22x22 in 4:1:1 and "4:1:0" and 22x18 in 4:2:0 (footprints half outside the picture), which only the general
    form takes.  qp 100: the packets carry every bit of the planes, and the reference decoder gives them back to be compared with the
    conversion of the oracle's bytes directly.  The preset of a case is tests/test_gpu_enc_rgb3.py's; element types, orders and
    constants rotate."""
    assert not stream_inverse_is_undefined(w, h, FMT[name][0], LOSSLESS)
    hip = lib()
    i = SMALL.index((w, h, name, form))
    dtype, order, k, csc = H.FLOATS[i % 3], H.ORDERS[(i // 3) % 2], i % len(CONSTANTS), R.CSC[(i >> 1) % 4]
    hwcs, pictures = tensors(w, h, 3, 9, dtype, order, k)
    where = H.wide_pitch(w, dtype) if form == "wide" else H.general_pitch(w, dtype, i)
    got = encode(hip, hwcs, dtype, order, csc, k, name, cfg=LOSSLESS, **where)
    assert H.hwc_forms(hip) == ((3, 0) if form == "wide" else (0, 3))
    planes_equal_oracle(got, pictures, R.RGBA | csc, name)
    same_packets(expected(w, h, 3, 9, dtype, order, k, csc, name, lossless=True), got)


# ---- 4. the contract ---------------------------------------------------------------------------------------------------------------
def contract_tensor():
    """64x64x3 binary32 under scale 1 / bias 0 (position 0), scale 2^127 / bias 0 (position 1), scale 1 + 2^-12 / bias -256 (position
    2): the values the contract names, in front of noise that crosses every boundary.  Position 2 starts with the element 0x438037fd,
    whose product with the scale is 256.5 + 1.5e-5: rounded on its own it is 256.5 and leaves as the tie 0.5 -> 0; a fused multiply-add
    keeps the excess and gives 1.  (tests/test_gpu_enc_tensor.py's picture, its planes as the three POSITIONS.)"""
    rng = np.random.default_rng(64)
    f = lambda *v: np.array(v, dtype=np.float32)
    named = f(0.5, 1.5, 2.5, 254.5, 255.5, 0.0, -0.0, np.inf, -np.inf, np.nan, -3.0, 300.0, 1e30, -1e30, 0.49999997, 254.50002)
    p0 = (rng.integers(-40, 1200, (64, 64)).astype(np.float32) * np.float32(0.25))  # quarters -10 .. 300: ties among them
    p0.flat[:16] = named
    p1 = (rng.integers(0, 1024, (64, 64)).astype(np.uint32) << 20).view(np.float32).copy()  # subnormals (k < 8), tiny normals, the rest beyond 255
    p1.flat[:2] = np.array([0x00400000, 0x00600000], dtype=np.uint32).view(np.float32)      # 2^-127, 1.5 * 2^-127
    p2 = ((p0[::-1].astype(np.float64) + 256.0) / (1 + 2.0 ** -12)).astype(np.float32)
    p2.flat[:1] = np.array([0x438037fd], dtype=np.uint32).view(np.float32)
    hwc = np.ascontiguousarray(np.stack([p.view(np.uint32) for p in (p0, p1, p2)], axis=-1))
    return hwc, ((1.0, float(2.0 ** 127), 1 + 2.0 ** -12), (0.0, 0.0, -256.0))


@pytest.mark.parametrize("order", H.ORDERS, ids=ORDER_IDS)
def test_contract_ties_infinities_nans_and_subnormals(order):
    """every special value goes where the contract says, on the GPU as in numpy, with the constants in MEMORY order under both orders:
    the same tensor is read once as R G B and once as B G R, so the named bytes land in the channel the order gives position k.  A
    flush to zero would make position 1 hold 0 where it holds 1 and 2, a fused multiply-add or another rounding would move the ties,
    constants indexed by channel would move everything under B G R; lossless 4:4:4, so every byte reaches the packets"""
    hip = lib()
    hwc, (scale, bias) = contract_tensor()
    px = H.picture(hwc, F32, order, scale, bias)
    ch = H.channel_of(order)
    assert list(px[..., ch[0]].flat[:16]) == [0, 2, 2, 254, 255, 0, 0, 255, 0, 0, 0, 255, 255, 0, 0, 255]
    assert list(px[..., ch[1]].flat[:2]) == [1, 2]
    assert px[..., ch[2]].flat[0] == 0 and len(np.unique(px[..., ch[2]])) > 200
    encs = encoders(hip, 64, 64, "444", 1, LOSSLESS)
    got = H.encode_hwc_steps(hip, encs, lambda s, t: H.HwcIn(hwc, F32, order, R.FULL, scale, bias, pitch=768), 1)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    assert H.hwc_forms(hip) == (1, 0)
    planes_equal_oracle(got, (px,), R.RGBA | R.FULL, "444")
    same_packets(rgb_ref_packets((px,), R.RGBA | R.FULL, "444", LOSSLESS), got)


@pytest.mark.parametrize("dtype", H.FLOATS, ids=DTYPE_IDS.values())
def test_equals_the_planar_tensor_calls_packets(dtype):
    """the same picture de-interleaved and handed to dsv2hip_enc_batch_tensor with the constants permuted by the order (B G R here): the
    same packets, and the reference's"""
    hip = lib()
    w, h, name, k, csc, order = 176, 144, "420", 3, R.BT709 | R.FULL, BGR
    hwcs, _ = tensors(w, h, 3, 5, dtype, order, k)
    scale, bias = CONSTANTS[k]
    got = encode(hip, hwcs, dtype, order, csc, k, name, **H.wide_pitch(w, dtype))
    assert H.hwc_forms(hip) == (3, 0) and T.tensor_forms(hip) == (0, 0)
    encs = encoders(hip, w, h, name, 1, CFG)
    planar = T.encode_tensor_steps(hip, encs, lambda s, t: T.TensorIn(H.planes_of(hwcs[t], order), dtype, csc, H.by_position(scale, order), H.by_position(bias, order),
                                                                     **T.wide_pitches(w, dtype)), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    assert T.tensor_forms(hip) == (3, 0)
    same_packets(planar, got, "against the planar tensor call")
    same_packets(expected(w, h, 3, 5, dtype, order, k, csc, name), got)


# ---- 5. the decoder's interleaved output, handed straight back --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decoded_stream():
    return stream(176, 144, "420", 3, 3)


@functools.lru_cache(maxsize=None)
def surface_packets(order, csc):
    """the bytes the decoder delivers as a uint8 tensor of `order` (the library's planar delivery through tests/hwc_out.py's oracle), and
    the packets of the three-byte surface of `order` that holds them"""
    hip = lib()
    w, h = 176, 144
    sp = HO.spec(TO.U8, order, csc, aligned, 0)
    pictures = [p for _, _, p in HO.hwc_expected(planar_oracle(decoded_stream()), "420", sp) if p is not None]
    assert len(pictures) == 3 and all(len(np.unique(p)) > 32 for p in pictures), "broken test case"
    px4 = [np.concatenate([p, np.zeros((h, w, 1), dtype=np.uint8)], axis=-1) for p in pictures]  # (bytes 0..2 in memory order)
    encs = encoders(hip, w, h, "420", 1, CFG)
    got = encode_steps(hip, encs, lambda s, t: Rgb3Surface(px4[t], order | csc, pitch=3 * w + 16), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    want = rgb_ref_packets(px4, four_byte(order) | csc, "420", CFG)
    same_packets(want, got, "the three-byte surface against the reference")
    return tuple(pictures), tuple(got)


@pytest.mark.parametrize("order", H.ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("constants", ["unit", "imagenet"])
@pytest.mark.parametrize("dtype", H.FLOATS, ids=DTYPE_IDS.values())
def test_decoder_output_comes_back_as_its_bytes(dtype, constants, order):
    """A 176x144 4:2:0 stream decoded by dsv2hip_dec_hwc_frame into a pitched float tensor under the UNIT or the ImageNet constants (by
    position), whose pointer and pitch go straight to dsv2hip_enc_hwc_frame under the inverse constants: the packets are those of the
    uint8 three-byte surface of the same order that holds the bytes the elements were made from.  The encoder writes nothing into the
    tensor."""
    csc = R.BT709
    pictures, want = surface_packets(order, csc)
    hip = HO.bind(lib())
    w, h = 176, 144
    dec_consts = TO.UNIT if constants == "unit" else TO.IMAGENET
    dec_consts = (H.by_position(dec_consts[0], order), H.by_position(dec_consts[1], order))
    scale, bias = T.inverse(dec_consts)
    sp = HO.spec(dtype, order, csc, aligned, 0, dec_consts)
    tn = HO.OutHwc((3 * w * H.ELEM[dtype], h), **sp)
    tn.arm()
    torch.cuda.synchronize()
    src = H.descriptor(tn.c.data, tn.c.pitch, dtype, order, csc, scale, bias)
    enc, dec = encoders(hip, w, h, "420", 1, CFG)[0], A.DECODER()
    got, seen = [], 0
    for pk in decoded_stream():
        buf, fn = A.BUF(), C.c_uint32(0)
        mk_buf(hip, buf, pk)
        had_meta = dec.got_metadata
        code = hip.dsv2hip_dec_hwc_frame(C.byref(dec), C.byref(buf), C.byref(tn.c), C.byref(fn))
        if code == A.DEC_EOS:
            break
        if code != A.DEC_OK or not had_meta:
            continue
        delivered = tn.planes()
        assert np.array_equal(H.picture(delivered, dtype, order, scale, bias)[..., list(H.channel_of(order))], pictures[seen])  # (the round trip, on the oracle's side)
        obufs = (A.BUF * 4)()
        n = hip.dsv2hip_enc_hwc_frame(C.byref(enc), C.byref(src), obufs)
        assert 1 <= n <= 4
        for q in range(n):
            got.append(bytes(C.string_at(obufs[q].data, obufs[q].len)))
            hip.dsv_buf_free(C.byref(obufs[q]))
        assert np.array_equal(tn.planes(), delivered)  # (and the encoder wrote nothing into the tensor)
        seen += 1
    hip.dsv_enc_free(C.byref(enc))
    hip.dsv_dec_free(C.byref(dec))
    assert seen == 3 and H.hwc_forms(hip) == (3, 0)
    same_packets(want, got, "against the uint8 surface of the same bytes")


# ---- 6. torch tensors read in place ---------------------------------------------------------------------------------------------------
TORCH = {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}


def as_torch(hwc, dtype):
    """h x w x 3 bit patterns as a contiguous torch [h, w, 3] tensor of the element type on the device"""
    bits = np.ascontiguousarray(hwc).view(np.int16 if dtype != F32 else np.int32)
    return torch.from_numpy(bits).cuda().view(TORCH[dtype]).contiguous()


@pytest.mark.parametrize("dtype,order", [(F16, RGB), (BF16, BGR)], ids=["float16-rgb", "bfloat16-bgr"])
def test_torch_hwc_tensors_read_in_place(dtype, order):
    """A contiguous torch [h, w, 3] tensor of float16 / bfloat16: data = data_ptr, pitch = 3 * w * elem, the wide form."""
    hip = lib()
    w, h, name, k = 352, 288, "420", 1
    hwcs, _ = tensors(w, h, 3, 5, dtype, order, k)
    scale, bias = CONSTANTS[k]

    def make(s, t):
        whole = as_torch(hwcs[t], dtype)
        assert whole.dtype == TORCH[dtype] and whole.shape == (h, w, 3) and whole.is_contiguous()
        return H.TorchIn(whole, whole, dtype, order, R.BT601, scale, bias)

    encs = encoders(hip, w, h, name, 1, CFG)
    got = H.encode_hwc_steps(hip, encs, make, 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(expected(w, h, 3, 5, dtype, order, k, R.BT601, name), got)
    assert H.hwc_forms(hip) == (3, 0)


def test_torch_channels_last_tensor_read_in_place():
    """a float32 [1, 3, h, w] tensor in torch's channels_last memory format IS [h, w, 3] in memory: data = data_ptr, pitch = 3 * w * 4"""
    hip = lib()
    w, h, name, k = 352, 288, "420", 0
    hwcs, _ = tensors(w, h, 3, 5, F32, RGB, k)
    scale, bias = CONSTANTS[k]

    class ChannelsLast:
        def __init__(self, hwc):
            nchw = as_torch(hwc, F32).permute(2, 0, 1).unsqueeze(0).contiguous()  # what a model works on: [1, 3, h, w], contiguous
            self.t = nchw.contiguous(memory_format=torch.channels_last)           # ... and what it hands out under channels_last
            assert self.t.shape == (1, 3, h, w) and self.t.stride() == (3 * h * w, 1, 3 * w, 3) and not self.t.is_contiguous()
            self.was = self.t.clone()
            self.c = H.descriptor(self.t.data_ptr(), 3 * w * 4, F32, RGB, R.BT709, scale, bias)

        def check_untouched(self):
            assert torch.equal(self.t.view(torch.int32), self.was.view(torch.int32)), "the encoder wrote into a tensor"

    encs = encoders(hip, w, h, name, 1, CFG)
    got = H.encode_hwc_steps(hip, encs, lambda s, t: ChannelsLast(hwcs[t]), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(expected(w, h, 3, 5, F32, RGB, k, R.BT709, name), got)
    assert H.hwc_forms(hip) == (3, 0)


def test_torch_crop_is_read_in_place():
    """a 354x290 crop at (7, 5) of a float32 [300, 370, 3] tensor: the parent's pitch, an offset pointer, w no multiple of 4"""
    hip = lib()
    w, h, name, k = 354, 290, "420", 0
    hwcs, _ = tensors(w, h, 3, 5, F32, BGR, k)
    scale, bias = CONSTANTS[k]

    def make(s, t):
        whole = torch.rand((300, 370, 3), dtype=torch.float32, device="cuda")
        view = whole[5:5 + h, 7:7 + w, :]
        view.copy_(as_torch(hwcs[t], F32))
        assert not view.is_contiguous()
        return H.TorchIn(view, whole, F32, BGR, R.BT709, scale, bias)

    encs = encoders(hip, w, h, name, 1, CFG)
    got = H.encode_hwc_steps(hip, encs, make, 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(expected(w, h, 3, 5, F32, BGR, k, R.BT709, name), got)
    assert H.hwc_forms(hip) == (0, 3)


# ---- 7. padding is never an element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,form", [(352, 288, "wide"), (354, 290, "general")], ids=["wide", "general"])
def test_padding_is_never_an_element_and_nothing_is_written(w, h, form):
    """The same elements with the pitch padding and the bytes around the rows holding 0x00, then 0xFF (NaNs), then noise: identical
    packets, the reference's; every byte of the allocations is afterwards what the test put there (encode_hwc_steps)."""
    hip = lib()
    hwcs, _ = tensors(w, h, 3, 5, F16, BGR, 0)
    where = H.wide_pitch(w, F16) if form == "wide" else H.general_pitch(w, F16, 2)
    runs = [encode(hip, hwcs, F16, BGR, R.BT601, 0, "420", fill=fill, **where) for fill in (0x00, 0xFF, None)]
    assert runs[0] == runs[1] == runs[2]
    same_packets(expected(w, h, 3, 5, F16, BGR, 0, R.BT601, "420"), runs[0])


# ---- 8. one step: everything mixed ------------------------------------------------------------------------------------------------------
MIXED = [(F16, RGB, R.BT601, 0, "wide", dict(qp=60, gop=12)), (BF16, BGR, R.BT709 | R.FULL, 1, "general", dict(qp=40, gop=3)),
         (F32, BGR, R.FULL, 3, "wide", dict(qp=100, gop=12)), (F32, RGB, R.BT709, 2, "wide", dict(qp=60, gop=12))]


def test_mixed_step():
    """Four encoders in one call per frame (one step key: 176x144 4:2:0) whose tensors differ in element type, order, preset, constants,
    pointer and pitch -- the BF16 one off alignment, so the step's ONE launch is general and counts once in the general column -- and
    whose streams differ in quantiser and GOP: each stream's packets are those of its own single-encoder run, and the reference's."""
    hip = lib()
    w, h, name, nfr = 176, 144, "420", 3

    def where(s):
        dtype, _, _, _, form, _ = MIXED[s]
        return H.wide_pitch(w, dtype) if form == "wide" else H.general_pitch(w, dtype, s)

    def source(s, t):
        dtype, order, csc, k, _, _ = MIXED[s]
        return H.HwcIn(tensors(w, h, nfr, 40 + s, dtype, order, k)[0][t], dtype, order, csc, *CONSTANTS[k], **where(s))

    alone = []
    for s, (*_, cfg) in enumerate(MIXED):
        encs = encoders(hip, w, h, name, 1, cfg)
        alone.append(H.encode_hwc_steps(hip, encs, lambda _, t: source(s, t), nfr)[0])
        hip.dsv_enc_free(C.byref(encs[0]))
    assert H.hwc_forms(hip, reset=True) == (9, 3)
    encs = [encoders(hip, w, h, name, 1, cfg)[0] for *_, cfg in MIXED]
    got = H.encode_hwc_steps(hip, encs, source, nfr)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    assert H.hwc_forms(hip) == (0, 3) and others_did_not_move(hip)
    for s, (dtype, order, csc, k, form, cfg) in enumerate(MIXED):
        same_packets(alone[s], got[s], "stream %d against its own run" % s)
        same_packets(rgb_ref_packets(tensors(w, h, nfr, 40 + s, dtype, order, k)[1], R.RGBA | csc, name, cfg), got[s], "stream %d" % s)


# ---- 9. uint8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,order", [("wide", RGB), ("general", BGR)], ids=["wide-rgb", "general-bgr"])
def test_u8_tensor_is_the_three_byte_surface(form, order):
    """DSV2HIP_TENSOR_U8 with constants that are not finite: the three-byte surface call's packets on the same bytes, and only the packed
    rgb3 counter moves"""
    hip = lib()
    w, h, name, csc = 176, 144, "420", R.BT709
    pictures = rgb_content(w, h, 3, 5)  # (bytes 0..2 of a picture are the tensor's elements 0..2, whatever the order calls them)
    where = H.wide_pitch(w, U8) if form == "wide" else H.general_pitch(w, U8, 1)
    nan = (float("nan"), float("inf"), -float("inf"))
    encs = encoders(hip, w, h, name, 1, CFG)
    got = H.encode_hwc_steps(hip, encs, lambda s, t: H.HwcIn(np.ascontiguousarray(pictures[t][..., :3]), U8, order, csc, nan, nan, **where), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    assert H.hwc_forms(hip) == (0, 0) and T.tensor_forms(hip) == (0, 0) and rgb_forms(hip) == (0, 0) and yuv_forms(hip) == (0, 0)
    assert rgb3_forms(hip) == ((3, 0, 0, 0) if form == "wide" else (0, 3, 0, 0))
    encs = encoders(hip, w, h, name, 1, CFG)
    surface = encode_steps(hip, encs, lambda s, t: Rgb3Surface(pictures[t], order | csc, pitch=where["pitch"], offset=where.get("offset", 0)), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(surface, got)
    same_packets(rgb_ref_packets(pictures, four_byte(order) | csc, name, CFG), got)


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------
def at(name, k, value):
    def f(c, w, elem):
        getattr(c, name)[k] = value
    return f


def scalar(name, value):
    def f(c, w, elem):
        setattr(c, name, value(c, w, elem) if callable(value) else value)
    return f


REFUSALS = [("dtype_4", scalar("dtype", 4)), ("dtype_negative", scalar("dtype", -1)),
            ("order_rgbp", scalar("order", 0x22)), ("order_bgra", scalar("order", 0x10)), ("order_rgba", scalar("order", 0x11)), ("order_zero", scalar("order", 0)),
            ("order_with_csc_bits", scalar("order", 0x121)),
            ("csc_0x400", scalar("csc", 0x400)), ("csc_layout_bits", scalar("csc", 0x121)),
            ("null_data", scalar("data", None)),
            ("pointer_off_the_element_grid", scalar("data", lambda c, w, e: c.data + 1)),
            ("pitch_off_the_element_grid", scalar("pitch", lambda c, w, e: c.pitch + 1)),
            ("pitch_one_element_short", scalar("pitch", lambda c, w, e: (3 * w - 1) * e)),
            ("pitch_of_a_planar_row", scalar("pitch", lambda c, w, e: w * e)),
            ("scale_inf", at("scale", 1, float("inf"))), ("scale_nan", at("scale", 0, float("nan"))),
            ("bias_inf", at("bias", 2, -float("inf"))), ("bias_nan", at("bias", 1, float("nan")))]


def refused(hip, encs, cs):
    """the batch call on descriptors cs returns -1 and leaves nbufs, the buffers and the encoders alone"""
    n = len(encs)
    encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
    bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)(*[77 + k for k in range(n)])
    blank = bytes(C.string_at(C.byref(bufs), C.sizeof(bufs)))
    state = [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs]
    assert hip.dsv2hip_enc_batch_hwc(n, encp, (H.INHWC * n)(*cs), bufs, nbufs) == -1
    assert list(nbufs) == [77 + k for k in range(n)] and bytes(C.string_at(C.byref(bufs), C.sizeof(bufs))) == blank
    assert [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs] == state


@pytest.mark.parametrize("what,spoil", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_tensor_touches_nothing(what, spoil):
    """Two encoders, the second one's descriptor spoiled (a mixed good / bad batch): -1 (0 packets from the one-frame call), nbufs and the
    buffer slots as the test set them, the encoders' bytes unchanged, the tensors' bytes unchanged; the same encoders then give the
    reference's packets from frame 0 on."""
    hip = lib()
    w, h, name, dtype, order, k = 176, 144, "420", F16 if "grid" not in what else F32, RGB, 0
    hwcs, _ = tensors(w, h, 3, 5, dtype, order, k)
    encs = encoders(hip, w, h, name, 2, CFG)
    good = [H.HwcIn(hwcs[0], dtype, order, R.BT709, *CONSTANTS[k], **H.wide_pitch(w, dtype)) for _ in range(2)]
    bad = H.copy_of(good[1].c)
    spoil(bad, w, H.ELEM[dtype])
    torch.cuda.synchronize()
    refused(hip, encs, [good[0].c, bad])
    state = bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1])))
    assert hip.dsv2hip_enc_hwc_frame(C.byref(encs[1]), C.byref(bad), (A.BUF * 4)()) == 0
    assert bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1]))) == state
    for g in good:
        g.check_untouched()
    assert H.hwc_forms(hip) == (0, 0) and others_did_not_move(hip)
    got = H.encode_hwc_steps(hip, encs, lambda s, t: H.HwcIn(hwcs[t], dtype, order, R.BT709, *CONSTANTS[k], **H.wide_pitch(w, dtype)), 3)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    for s in range(2):
        same_packets(expected(w, h, 3, 5, dtype, order, k, R.BT709, name), got[s], "stream %d" % s)


def test_refused_on_a_uyvy_encoder_and_for_missing_arguments():
    """An encoder whose packed input is interleaved UYVY takes no interleaved tensor, float or uint8; NULL arguments and n = 0 are
    refused; with the switch off again the encoder encodes from frame 0."""
    hip = lib()
    w, h, name, k = 176, 144, "422", 0
    hip.dsv2hip_enc_set_uyvy_input.argtypes, hip.dsv2hip_enc_set_uyvy_input.restype = [C.POINTER(A.ENCODER), C.c_int], C.c_int
    hwcs, _ = tensors(w, h, 3, 5, BF16, BGR, k)
    encs = encoders(hip, w, h, name, 1, CFG)
    src = H.HwcIn(hwcs[0], BF16, BGR, 0, *CONSTANTS[k], **H.wide_pitch(w, BF16))
    u8 = H.copy_of(src.c)
    u8.dtype = U8
    torch.cuda.synchronize()
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 1) == 0
    refused(hip, encs, [src.c])
    refused(hip, encs, [u8])
    assert hip.dsv2hip_enc_hwc_frame(C.byref(encs[0]), C.byref(src.c), (A.BUF * 4)()) == 0
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 0) == 0
    encp, bufs, nbufs = (C.POINTER(A.ENCODER) * 1)(C.pointer(encs[0])), (A.BUF * 4)(), (C.c_int * 1)(77)
    assert hip.dsv2hip_enc_batch_hwc(0, encp, (H.INHWC * 1)(src.c), bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_hwc(1, encp, None, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_hwc(1, encp, (H.INHWC * 1)(src.c), None, nbufs) == -1
    assert hip.dsv2hip_enc_hwc_frame(C.byref(encs[0]), None, bufs) == 0 and nbufs[0] == 77
    src.check_untouched()
    got = H.encode_hwc_steps(hip, encs, lambda s, t: H.HwcIn(hwcs[t], BF16, BGR, 0, *CONSTANTS[k], **H.wide_pitch(w, BF16)), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(expected(w, h, 3, 5, BF16, BGR, k, 0, name), got)
