"""Drive the public codec API (dsv_enc / dsv_dec) of either library on in-memory frames."""
import ctypes as C

import numpy as np

import dsvabi as A

# chroma format name -> (DSV_SUBSAMP_* code, horizontal shift, vertical shift); "410" is the reference's quarter by quarter (dsv.h:87-95)
FMT = {"444": (0x0, 0, 0), "422": (0x4, 1, 0), "420": (0x5, 1, 1), "411": (0x8, 2, 0), "410": (0xA, 2, 2)}


def frames(w, h, hs, vs, n, seed):
    """n packed planar pictures: moving waves with a little noise in luma, moving ramps in chroma"""
    rng = np.random.default_rng(seed)
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:ch, 0:cw]
    out = []
    for t in range(n):
        y = ((np.sin((xx + 3 * t) / 17.0) + np.cos((yy + 2 * t) / 11.0)) * 50 + 128 + rng.integers(-3, 4, (h, w))).clip(0, 255).astype(np.uint8)
        u = ((cx * 2 + t * 3) % 200 + 20).astype(np.uint8)
        v = ((cy * 3 + t * 5) % 180 + 30).astype(np.uint8)
        out.append(y.tobytes() + u.tobytes() + v.tobytes())
    return out


def ueg(v):
    """bit string of the interleaved exp-Golomb code (bs.c:132)"""
    v += 1
    nb = v.bit_length() - 1
    return "".join("0" + str((v >> i) & 1) for i in range(nb - 1, -1, -1)) + "1"


def meta_packet(fields):
    """a metadata packet that carries the given fields"""
    bits = "".join(ueg(f) for f in fields) + "0"
    bits += "0" * (-len(bits) % 8)
    body = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    return b"DSV2" + bytes([8, 0x00]) + bytes(8) + body


def configure_encoder(lib, enc, meta, qp=60, gop=48, effort=10, rc_mode=0, **over):
    """Field set-up as the reference CLI does it (dsv_main.c:548-723) for the given flags."""
    lib.dsv_enc_init(C.byref(enc))
    lib.dsv_enc_set_metadata(C.byref(enc), C.byref(meta))
    fps = (meta.fps_num + meta.fps_den // 2) // meta.fps_den
    enc.gop = fps if gop < 0 else gop
    enc.quality = qp * 4
    enc.effort = effort
    enc.rc_mode = rc_mode
    if rc_mode == 0:
        enc.min_quality = enc.quality - 20
        enc.min_I_frame_quality = enc.quality - 8
    else:
        enc.min_quality = 0
        enc.min_I_frame_quality = 20
    enc.max_quality = 400
    enc.min_quality = min(max(enc.min_quality, 0), 400)
    enc.min_I_frame_quality = min(max(enc.min_I_frame_quality, 0), 400)
    enc.min_q_step, enc.max_q_step = 2, 1
    enc.stable_refresh = min(max(fps, 1), 60)
    enc.bitrate = over.pop("bitrate", 4000000)
    for k, v in over.items():
        setattr(enc, k, v)
    lib.dsv_enc_start(C.byref(enc))


def encode_stream(lib, frames, w, h, subsamp, eos=True, meta=None, **cfg):
    """frames: list of bytes (planar YUV); meta: the stream's metadata where it is not mk_meta's default.  Returns (list of
    packet bytes, dict of the encoder's final stats)."""
    meta = A.mk_meta(w, h, subsamp) if meta is None else meta
    enc = A.ENCODER()
    configure_encoder(lib, enc, meta, **cfg)
    packets = []
    bufs = (A.BUF * 4)()
    keep = []
    for fb in frames:
        arr = np.frombuffer(fb, dtype=np.uint8).copy()
        keep.append(arr)
        fr = lib.dsv_load_planar_frame(subsamp, arr.ctypes.data, w, h)
        n = lib.dsv_enc(C.byref(enc), fr, bufs)
        for i in range(n):
            packets.append(bytes(C.string_at(bufs[i].data, bufs[i].len)))
            lib.dsv_buf_free(C.byref(bufs[i]))
    if eos:
        lib.dsv_enc_end_of_stream(C.byref(enc), bufs)
        packets.append(bytes(C.string_at(bufs[0].data, bufs[0].len)))
        lib.dsv_buf_free(C.byref(bufs[0]))
    stats = {k: getattr(enc.stats, k) for k in ("inum", "pnum", "isize", "psize", "eprm", "skip", "mbI", "mbP", "qpx", "hpx")}
    lib.dsv_enc_free(C.byref(enc))
    return packets, stats


def decode_stream(lib, packets):
    """Returns list of (fnum, Y, U, V) numpy planes."""
    dec = A.DECODER()
    out = []
    for pk in packets:
        buf = A.BUF()
        lib.dsv_mk_buf(C.byref(buf), len(pk) + 64)
        C.memmove(buf.data, pk, len(pk))
        fp = C.POINTER(A.FRAME)()
        fn = C.c_uint32(0)
        code = lib.dsv_dec(C.byref(dec), C.byref(buf), C.byref(fp), C.byref(fn))
        if code == A.DEC_OK and fp:
            f = fp.contents
            planes = []
            for c in range(3):
                p = f.planes[c]
                a = np.ctypeslib.as_array(p.data, shape=(p.h * p.stride,))
                planes.append(a.reshape(-1, p.stride)[:p.h, :p.w].copy() if p.stride * p.h == a.size else None)
            out.append((fn.value, planes[0], planes[1], planes[2]))
            lib.dsv_frame_ref_dec(fp)
        elif code == A.DEC_EOS:
            break
        elif code == A.DEC_ERROR:
            raise RuntimeError("decoder error")
    lib.dsv_dec_free(C.byref(dec))
    return out
