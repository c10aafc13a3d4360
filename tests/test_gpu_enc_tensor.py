"""Planar RGB float tensors (dsv2hip_in_tensor: binary16, bfloat16, binary32 under per-plane constants) as encoder input, bit for bit:
the packets are the reference encoder's on the planar picture that the conversion of include/dsv2_hip.h makes of the BYTES the
contract makes of the elements (tests/tensor_in.py: the numpy oracle; tests/rgb_csc.py under RGBA | csc) -- both forms of
k_ingest_tensor, the three element types, the four presets, the five chroma formats, the smallest pictures and footprints half outside
them (lossless, so every LSB reaches the packets), ties, infinities, NaNs, out-of-range values and subnormals, the decoder's own
elements under the inverse constants, torch tensors read in place, a step that mixes everything, the uint8 tensor that is the planar
RGB surface; the tensor is never written, padding is never an element, a refused call touches nothing.  The shapes are those of
tests/test_gpu_enc_rgb3.py; encoders and the reference's driver are tests/enc_in.py's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dsvabi as A
import rgb_csc as R
import tensor_in as T
import tensor_out as TO
from codec_run import FMT
from edge_cases import stream_inverse_is_undefined
from enc_in import CFG, LOSSLESS, Rgb3Surface, encode_steps, encoders, planes_equal_oracle, rgb_content, rgb_ref_packets, same_packets
from hipabi import RGBP, bind as bind_surfaces, enc_rgb3_forms as rgb3_forms, enc_rgb_forms as rgb_forms, enc_yuv_forms as yuv_forms, reset_enc_forms

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

F16, BF16, F32, U8 = T.F16, T.BF16, T.F32, T.U8
DTYPE_IDS = {F16: "f16", BF16: "bf16", F32: "f32"}
CONSTANTS = (T.UNIT_INV, T.IMAGENET_INV, T.IDENTITY, ((-255.0, 127.5, 300.0), (255.0, 10.25, -20.0)))


def lib():
    hip = T.bind(bind_surfaces(A.load_hip()))
    reset_enc_forms(hip)
    T.tensor_forms(hip, reset=True)
    return hip


@functools.lru_cache(maxsize=None)
def tensors(w, h, nfr, seed, dtype, k):
    """nfr tensors ([R, G, B] bit patterns) near rgb_content's pictures under constant set k, and the pictures their bytes ARE"""
    scale, bias = CONSTANTS[k]
    planes = tuple(tuple(T.tensor_near(px, dtype, scale, bias, 100 * seed + t)) for t, px in enumerate(rgb_content(w, h, nfr, seed)))
    pictures = tuple(T.picture(p, dtype, scale, bias) for p in planes)
    for p in pictures:
        assert len(np.unique(p[..., :3])) > 32, "broken test case: the tensor's bytes are nearly constant"
    return planes, pictures


@functools.lru_cache(maxsize=None)
def expected(w, h, nfr, seed, dtype, k, csc, name, lossless=False):
    """the real reference encoder on the planar pictures the conversion makes of the oracle's bytes"""
    return tuple(rgb_ref_packets(tensors(w, h, nfr, seed, dtype, k)[1], R.RGBA | csc, name, LOSSLESS if lossless else CFG))


def encode(hip, planes, dtype, csc, k, name, cfg=CFG, fill=T.GUARD, **where):
    """one encoder over the tensors `planes`, each in a TensorIn(**where); frees the encoder"""
    h, w = planes[0][0].shape
    encs = encoders(hip, w, h, name, 1, cfg)
    scale, bias = CONSTANTS[k]
    got = T.encode_tensor_steps(hip, encs, lambda s, t: T.TensorIn(planes[t], dtype, csc, scale, bias, fill=fill, **where), len(planes))
    hip.dsv_enc_free(C.byref(encs[0]))
    return got[0]


# ---- 1. wide form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.FLOATS, ids=DTYPE_IDS.values())
def test_wide_form_equals_reference(dtype):
    """352x288 4:2:0, three frames, pointers on 16-byte boundaries and pitches multiples of 16: one 8 / 16-byte load a plane and row;
    the tensor counter reads (3, 0), the counters of the surfaces do not move."""
    hip = lib()
    k = T.FLOATS.index(dtype) % 2
    planes, _ = tensors(352, 288, 3, 5, dtype, k)
    got = encode(hip, planes, dtype, R.BT709, k, "420", **T.wide_pitches(352, dtype))
    same_packets(expected(352, 288, 3, 5, dtype, k, R.BT709, "420"), got)
    assert T.tensor_forms(hip) == (3, 0)
    assert rgb3_forms(hip) == (0, 0, 0, 0) and rgb_forms(hip) == (0, 0) and yuv_forms(hip) == (0, 0)


# ---- 2. general form, every format -------------------------------------------------------------------------------------------------
GENERAL = [(354, 290, "420")] + [(176, 144, name) for name in sorted(FMT)]


@pytest.mark.parametrize("dtype", T.FLOATS, ids=DTYPE_IDS.values())
@pytest.mark.parametrize("i,w,h,name", [(i,) + g for i, g in enumerate(GENERAL)], ids=["%dx%d-%s" % g for g in GENERAL])
def test_general_form_equals_reference(i, w, h, name, dtype):
    """Pointers 1, 2 and 3 elements behind a 16-byte boundary and pitches of the row plus 1, 2, 3 elements, another per plane; a
    354-pixel row is more than one pass of the workgroup (256 pixels), its last pass partial, and its last thread holds two pixels of
    four.  Presets and constants rotate across the cases."""
    hip = lib()
    turn = i + T.FLOATS.index(dtype)
    csc, k = R.CSC[turn % 4], turn % len(CONSTANTS)
    planes, _ = tensors(w, h, 3, 5, dtype, k)
    got = encode(hip, planes, dtype, csc, k, name, **T.general_pitches(w, dtype, turn))
    same_packets(expected(w, h, 3, 5, dtype, k, csc, name), got)
    assert T.tensor_forms(hip) == (0, 3) and rgb3_forms(hip) == (0, 0, 0, 0)


# ---- 3. smallest pictures, clamped footprints: lossless -------------------------------------------------------------------------------
SMALL = ([(16, 16, name, form) for name in sorted(FMT) for form in ("wide", "general")] +
         [(22, 22, "411", "general"), (22, 22, "410", "general"), (22, 18, "420", "general")])


@pytest.mark.parametrize("w,h,name,form", SMALL, ids=["%dx%d-%s-%s" % s for s in SMALL])
def test_smallest_pictures_lossless(w, h, name, form):
    """16x16 in both forms; 22x22 in 4:1:1 and "4:1:0" and 22x18 in 4:2:0 (footprints half outside the picture), which only the general
    form takes.  qp 100: the packets carry every bit of the planes, and the reference decoder gives them back to be compared with the
    conversion of the oracle's bytes directly.  The preset of a case is tests/test_gpu_enc_rgb3.py's (which says why); element types
    and constants rotate."""
    assert not stream_inverse_is_undefined(w, h, FMT[name][0], LOSSLESS)
    hip = lib()
    i = SMALL.index((w, h, name, form))
    dtype, k, csc = T.FLOATS[i % 3], i % len(CONSTANTS), R.CSC[(i >> 1) % 4]
    planes, pictures = tensors(w, h, 3, 9, dtype, k)
    where = T.wide_pitches(w, dtype) if form == "wide" else T.general_pitches(w, dtype, i)
    got = encode(hip, planes, dtype, csc, k, name, cfg=LOSSLESS, **where)
    assert T.tensor_forms(hip) == ((3, 0) if form == "wide" else (0, 3))
    planes_equal_oracle(got, pictures, R.RGBA | csc, name)
    same_packets(expected(w, h, 3, 9, dtype, k, csc, name, lossless=True), got)


# ---- 4. the contract ---------------------------------------------------------------------------------------------------------------
def contract_picture():
    """64x64 binary32 under scale 1 / bias 0 (R), scale 2^127 / bias 0 (G), scale 1 + 2^-12 / bias -256 (B): the values the contract
    names, in front of noise that crosses every boundary.  B starts with the element 0x438037fd, whose product with the scale is
    256.5 + 1.5e-5: rounded on its own it is 256.5 and leaves as the tie 0.5 -> 0; a fused multiply-add keeps the excess and gives 1."""
    rng = np.random.default_rng(64)
    f = lambda *v: np.array(v, dtype=np.float32)
    named = f(0.5, 1.5, 2.5, 254.5, 255.5, 0.0, -0.0, np.inf, -np.inf, np.nan, -3.0, 300.0, 1e30, -1e30, 0.49999997, 254.50002)
    want = [0, 2, 2, 254, 255, 0, 0, 255, 0, 0, 0, 255, 255, 0, 0, 255]
    r = (rng.integers(-40, 1200, (64, 64)).astype(np.float32) * np.float32(0.25))  # quarters -10 .. 300: ties among them
    r.flat[:16] = named
    g = (rng.integers(0, 1024, (64, 64)).astype(np.uint32) << 20).view(np.float32).copy()  # subnormals (k < 8), tiny normals, the rest beyond 255
    g.flat[:2] = np.array([0x00400000, 0x00600000], dtype=np.uint32).view(np.float32)      # 2^-127, 1.5 * 2^-127
    b = ((r[::-1].astype(np.float64) + 256.0) / (1 + 2.0 ** -12)).astype(np.float32)
    b.flat[:1] = np.array([0x438037fd], dtype=np.uint32).view(np.float32)
    planes = [p.view(np.uint32).copy() for p in (r, g, b)]
    constants = ((1.0, float(2.0 ** 127), 1 + 2.0 ** -12), (0.0, 0.0, -256.0))
    px = T.picture(planes, F32, *constants)
    assert list(px[..., 0].flat[:16]) == want and list(px[..., 1].flat[:2]) == [1, 2]
    assert px[..., 2].flat[0] == 0 and len(np.unique(px[..., 2])) > 200
    return planes, constants, px


def test_contract_ties_infinities_nans_and_subnormals():
    """every special value goes where the contract says, on the GPU as in numpy: a flush to zero would make the G plane 0 where it is 1
    and 2, a fused multiply-add or another rounding would move the ties; lossless 4:4:4, so every byte reaches the packets"""
    hip = lib()
    planes, (scale, bias), px = contract_picture()
    encs = encoders(hip, 64, 64, "444", 1, LOSSLESS)
    got = T.encode_tensor_steps(hip, encs, lambda s, t: T.TensorIn(planes, F32, R.FULL, scale, bias, pitches=(256, 256, 256)), 1)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    assert T.tensor_forms(hip) == (1, 0)
    planes_equal_oracle(got, (px,), R.RGBA | R.FULL, "444")
    same_packets(rgb_ref_packets((px,), R.RGBA | R.FULL, "444", LOSSLESS), got)


@pytest.mark.parametrize("dtype", T.FLOATS, ids=DTYPE_IDS.values())
def test_decoder_elements_come_back_as_their_bytes(dtype):
    """the elements the decoder delivers for a picture's bytes under the ImageNet constants (tests/tensor_out.py), encoded under the
    inverse constants: the packets of the planar RGB surface that holds the original bytes, and the reference's"""
    hip = lib()
    w, h, name, csc = 176, 144, "420", R.BT709 | R.FULL
    pictures = rgb_content(w, h, 3, 5)
    planes = [[TO.elements(px[..., c], dtype, TO.IMAGENET[0][c], TO.IMAGENET[1][c]) for c in range(3)] for px in pictures]
    scale, bias = T.IMAGENET_INV
    for p, px in zip(planes, pictures):
        assert np.array_equal(T.picture(p, dtype, scale, bias)[..., :3], px[..., :3])  # (the round trip, on the oracle's side)
    encs = encoders(hip, w, h, name, 1, CFG)
    got = T.encode_tensor_steps(hip, encs, lambda s, t: T.TensorIn(planes[t], dtype, csc, scale, bias, **T.wide_pitches(w, dtype)), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    encs = encoders(hip, w, h, name, 1, CFG)
    surface = encode_steps(hip, encs, lambda s, t: Rgb3Surface(pictures[t], RGBP | csc, pitch=192), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(surface, got, "against the RGBP surface")
    same_packets(rgb_ref_packets(pictures, R.RGBA | csc, name, CFG), got)


# ---- 5. torch tensors read in place ---------------------------------------------------------------------------------------------------
TORCH = {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}


def as_torch(planes, dtype):
    """[R, G, B] bit patterns as a contiguous torch [3, h, w] tensor of the element type on the device"""
    bits = np.stack(planes).view(np.int16 if dtype != F32 else np.int32)
    return torch.from_numpy(bits).cuda().view(TORCH[dtype]).contiguous()


@pytest.mark.parametrize("reverse", [False, True], ids=["rgb", "bgr-by-pointer"])
@pytest.mark.parametrize("dtype", T.FLOATS, ids=DTYPE_IDS.values())
def test_torch_tensors_read_in_place(dtype, reverse):
    """A contiguous torch [3, h, w] tensor of float16 / bfloat16 / float32: plane[c] = data_ptr + c * h * w * elem, pitch = w * elem, the
    wide form.  Reversed: the tensor holds B, G, R, and the planes are handed over in the other order with their constants."""
    hip = lib()
    w, h, name, k = 352, 288, "420", 1
    planes, _ = tensors(w, h, 3, 5, dtype, k)
    scale, bias = CONSTANTS[k]

    def make(s, t):
        whole = as_torch(planes[t][::-1] if reverse else planes[t], dtype)
        assert whole.dtype == TORCH[dtype] and whole.shape == (3, h, w)
        return T.TorchIn(whole, whole, dtype, R.BT601, scale, bias, order=(2, 1, 0) if reverse else (0, 1, 2))

    encs = encoders(hip, w, h, name, 1, CFG)
    got = T.encode_tensor_steps(hip, encs, make, 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(expected(w, h, 3, 5, dtype, k, R.BT601, name), got)
    assert T.tensor_forms(hip) == (3, 0)


def test_torch_crop_is_read_in_place():
    """a 354x290 crop at (7, 5) of a float32 [3, 300, 370] tensor: the parent's pitch, offset pointers, w no multiple of 4"""
    hip = lib()
    w, h, name, k = 354, 290, "420", 0
    planes, _ = tensors(w, h, 3, 5, F32, k)
    scale, bias = CONSTANTS[k]

    def make(s, t):
        whole = torch.rand((3, 300, 370), dtype=torch.float32, device="cuda")
        view = whole[:, 5:5 + h, 7:7 + w]
        view.copy_(as_torch(planes[t], F32))
        assert not view.is_contiguous()
        return T.TorchIn(view, whole, F32, R.BT709, scale, bias)

    encs = encoders(hip, w, h, name, 1, CFG)
    got = T.encode_tensor_steps(hip, encs, make, 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(expected(w, h, 3, 5, F32, k, R.BT709, name), got)
    assert T.tensor_forms(hip) == (0, 3)


# ---- 6. padding is never an element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,form", [(352, 288, "wide"), (354, 290, "general")], ids=["wide", "general"])
def test_padding_is_never_an_element_and_nothing_is_written(w, h, form):
    """The same elements with the pitch padding and the bytes around the planes holding 0x00, then 0xFF (NaNs), then noise: identical
    packets, the reference's; every byte of the allocations is afterwards what the test put there (encode_tensor_steps)."""
    hip = lib()
    planes, _ = tensors(w, h, 3, 5, F16, 0)
    where = T.wide_pitches(w, F16) if form == "wide" else T.general_pitches(w, F16, 2)
    runs = [encode(hip, planes, F16, R.BT601, 0, "420", fill=fill, **where) for fill in (0x00, 0xFF, None)]
    assert runs[0] == runs[1] == runs[2]
    same_packets(expected(w, h, 3, 5, F16, 0, R.BT601, "420"), runs[0])


# ---- 7. one step: everything mixed ------------------------------------------------------------------------------------------------------
MIXED = [(F16, R.BT601, 0, "wide", dict(qp=60, gop=12)), (BF16, R.BT709 | R.FULL, 1, "general", dict(qp=40, gop=3)), (F32, R.FULL, 3, "wide", dict(qp=100, gop=12))]


def test_mixed_step():
    """Three encoders in one call per frame (one step key: 176x144 4:2:0) whose tensors differ in element type, preset, constants,
    pointers and pitches -- the BF16 one element off alignment, so the step's ONE launch is general -- and whose streams differ in
    quantiser and GOP: each stream's packets are those of its own single-encoder run, and the reference's."""
    hip = lib()
    w, h, name, nfr = 176, 144, "420", 3

    def where(s):
        dtype, _, _, form, _ = MIXED[s]
        return T.wide_pitches(w, dtype) if form == "wide" else T.general_pitches(w, dtype, s)

    def source(s, t):
        dtype, csc, k, _, _ = MIXED[s]
        return T.TensorIn(tensors(w, h, nfr, 40 + s, dtype, k)[0][t], dtype, csc, *CONSTANTS[k], **where(s))

    alone = []
    for s, (dtype, csc, k, form, cfg) in enumerate(MIXED):
        encs = encoders(hip, w, h, name, 1, cfg)
        alone.append(T.encode_tensor_steps(hip, encs, lambda _, t: source(s, t), nfr)[0])
        hip.dsv_enc_free(C.byref(encs[0]))
    assert T.tensor_forms(hip, reset=True) == (6, 3)
    encs = [encoders(hip, w, h, name, 1, cfg)[0] for *_, cfg in MIXED]
    got = T.encode_tensor_steps(hip, encs, source, nfr)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    assert T.tensor_forms(hip) == (0, 3)
    for s, (dtype, csc, k, form, cfg) in enumerate(MIXED):
        same_packets(alone[s], got[s], "stream %d against its own run" % s)
        same_packets(rgb_ref_packets(tensors(w, h, nfr, 40 + s, dtype, k)[1], R.RGBA | csc, name, cfg), got[s], "stream %d" % s)


# ---- 8. uint8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["wide", "general"])
def test_u8_tensor_is_the_planar_rgb_surface(form):
    """DSV2HIP_TENSOR_U8 with constants that are not finite: the RGBP surface call's packets on the same bytes, and only the planar
    rgb3 counter moves"""
    hip = lib()
    w, h, name, csc = 176, 144, "420", R.BT709
    pictures = rgb_content(w, h, 3, 5)
    where = T.wide_pitches(w, U8) if form == "wide" else T.general_pitches(w, U8, 1)
    nan = (float("nan"), float("inf"), -float("inf"))
    encs = encoders(hip, w, h, name, 1, CFG)
    got = T.encode_tensor_steps(hip, encs, lambda s, t: T.TensorIn(list(pictures[t][..., :3].transpose(2, 0, 1)), U8, csc, nan, nan, **where), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    assert T.tensor_forms(hip) == (0, 0) and rgb_forms(hip) == (0, 0) and yuv_forms(hip) == (0, 0)
    assert rgb3_forms(hip) == ((0, 0, 3, 0) if form == "wide" else (0, 0, 0, 3))
    encs = encoders(hip, w, h, name, 1, CFG)
    surface = encode_steps(hip, encs, lambda s, t: Rgb3Surface(pictures[t], RGBP | csc, pitch=where["pitches"], offset=where.get("offsets", 0)), 3)[0]
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(surface, got)
    same_packets(rgb_ref_packets(pictures, R.RGBA | csc, name, CFG), got)


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def field(name, plane, value):
    def f(c, w, elem):
        getattr(c, name)[plane] = value(c, w, elem) if callable(value) else value
    return f


def scalar(name, value):
    def f(c, w, elem):
        setattr(c, name, value)
    return f


REFUSALS = [("dtype_4", scalar("dtype", 4)), ("dtype_negative", scalar("dtype", -1)), ("csc_0x400", scalar("csc", 0x400)), ("csc_layout_bits", scalar("csc", 0x122)),
            ("null_plane_0", field("plane", 0, None)), ("null_plane_2", field("plane", 2, None)),
            ("pointer_off_the_element_grid", field("plane", 1, lambda c, w, e: c.plane[1] + 1)),
            ("pitch_off_the_element_grid", field("pitch", 2, lambda c, w, e: c.pitch[2] + 1)),
            ("pitch_short", field("pitch", 0, lambda c, w, e: (w - 1) * e)),
            ("scale_inf", field("scale", 1, float("inf"))), ("scale_nan", field("scale", 0, float("nan"))),
            ("bias_inf", field("bias", 2, -float("inf"))), ("bias_nan", field("bias", 1, float("nan")))]


def refused(hip, encs, cs):
    """the batch call on descriptors cs returns -1 and leaves nbufs, the buffers and the encoders alone"""
    n = len(encs)
    encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
    bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)(*[77 + k for k in range(n)])
    blank = bytes(C.string_at(C.byref(bufs), C.sizeof(bufs)))
    state = [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs]
    assert hip.dsv2hip_enc_batch_tensor(n, encp, (T.INTENSOR * n)(*cs), bufs, nbufs) == -1
    assert list(nbufs) == [77 + k for k in range(n)] and bytes(C.string_at(C.byref(bufs), C.sizeof(bufs))) == blank
    assert [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs] == state


@pytest.mark.parametrize("what,spoil", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_tensor_touches_nothing(what, spoil):
    """Two encoders, the second one's descriptor spoiled (a mixed good / bad batch): -1 (0 packets from the one-frame call), nbufs and the
    buffer slots as the test set them, the encoders' bytes unchanged, the tensors' bytes unchanged; the same encoders then give the
    reference's packets from frame 0 on."""
    hip = lib()
    w, h, name, dtype, k = 176, 144, "420", F16 if "grid" not in what else F32, 0
    planes, _ = tensors(w, h, 3, 5, dtype, k)
    encs = encoders(hip, w, h, name, 2, CFG)
    good = [T.TensorIn(planes[0], dtype, R.BT709, *CONSTANTS[k], **T.wide_pitches(w, dtype)) for _ in range(2)]
    bad = T.copy_of(good[1].c)
    spoil(bad, w, T.ELEM[dtype])
    torch.cuda.synchronize()
    refused(hip, encs, [good[0].c, bad])
    state = bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1])))
    assert hip.dsv2hip_enc_tensor_frame(C.byref(encs[1]), C.byref(bad), (A.BUF * 4)()) == 0
    assert bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1]))) == state
    for g in good:
        g.check_untouched()
    assert T.tensor_forms(hip) == (0, 0)
    got = T.encode_tensor_steps(hip, encs, lambda s, t: T.TensorIn(planes[t], dtype, R.BT709, *CONSTANTS[k], **T.wide_pitches(w, dtype)), 3)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    for s in range(2):
        same_packets(expected(w, h, 3, 5, dtype, k, R.BT709, name), got[s], "stream %d" % s)


def test_refused_on_a_uyvy_encoder_and_for_missing_arguments():
    """An encoder whose packed input is interleaved UYVY takes no tensor, float or uint8; NULL arguments and n = 0 are refused; with
    the switch off again the encoder encodes from frame 0."""
    hip = lib()
    w, h, name, k = 176, 144, "422", 0
    hip.dsv2hip_enc_set_uyvy_input.argtypes, hip.dsv2hip_enc_set_uyvy_input.restype = [C.POINTER(A.ENCODER), C.c_int], C.c_int
    planes, _ = tensors(w, h, 3, 5, BF16, k)
    encs = encoders(hip, w, h, name, 1, CFG)
    src = T.TensorIn(planes[0], BF16, 0, *CONSTANTS[k], **T.wide_pitches(w, BF16))
    u8 = T.copy_of(src.c)
    u8.dtype = U8
    torch.cuda.synchronize()
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 1) == 0
    refused(hip, encs, [src.c])
    refused(hip, encs, [u8])
    assert hip.dsv2hip_enc_tensor_frame(C.byref(encs[0]), C.byref(src.c), (A.BUF * 4)()) == 0
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 0) == 0
    encp, bufs, nbufs = (C.POINTER(A.ENCODER) * 1)(C.pointer(encs[0])), (A.BUF * 4)(), (C.c_int * 1)(77)
    assert hip.dsv2hip_enc_batch_tensor(0, encp, (T.INTENSOR * 1)(src.c), bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_tensor(1, encp, None, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_tensor(1, encp, (T.INTENSOR * 1)(src.c), None, nbufs) == -1
    assert hip.dsv2hip_enc_tensor_frame(C.byref(encs[0]), None, bufs) == 0 and nbufs[0] == 77
    src.check_untouched()
    got = encode_tensor_from(hip, encs, planes, BF16, k, w)
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(expected(w, h, 3, 5, BF16, k, 0, name), got)


def encode_tensor_from(hip, encs, planes, dtype, k, w):
    return T.encode_tensor_steps(hip, encs, lambda s, t: T.TensorIn(planes[t], dtype, 0, *CONSTANTS[k], **T.wide_pitches(w, dtype)), len(planes))[0]
