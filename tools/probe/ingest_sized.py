#!/usr/bin/env python3
"""The sized ingest measured next to the plain and the half-size one (experiments), after tools/probe/ingest_scaled.py:
tools/probe/ingest_sized.py [--steps N] [nv12_plain] [bgra_plain] [nv12_s1] [bgra_s1] [nv12_720] [nv12_480] [bgra_720] [bgra_480]   (default: all)
One 1080p 4:2:0 source per stream and step, 64 streams in one lockstep group, N (24) timed steps behind 2 warm-up steps:
  nv12_plain  dsv2hip_enc_batch_surface, NV12, pitch 1920, 1920x1080 encoders (k_ingest_surface<16>: the yardstick)
  bgra_plain  dsv2hip_enc_batch_surface, BGRA | BT709, pitch 7680, 1920x1080 encoders (k_ingest_rgb<16>: the yardstick)
  nv12_s1     dsv2hip_enc_batch_surface_scaled, SCALE_HALF, encoders of 960x540 (k_ingest_surface_scaled<wide>: the second yardstick)
  bgra_s1     the same with the BGRA surfaces (k_ingest_rgb_scaled<wide>)
  nv12_720    dsv2hip_enc_batch_surface_sized, the same NV12 surfaces, encoders of 1280x720 (k_ingest_sized<wide>)
  nv12_480    ... encoders of 854x480
  bgra_720    dsv2hip_enc_batch_surface_sized, the same BGRA surfaces, encoders of 1280x720 (k_ingest_rgb_sized<wide>)
  bgra_480    ... encoders of 854x480
Every stream reads memory of its own (copies of 2 videos), so no stream's reads are served from the cache by another's.  The
frames/s of the legs are not comparable with one another (the encoders behind the ingest differ in size); the ingest kernels'
time per launch is: rocprofv3 --kernel-trace --stats -- python tools/probe/ingest_sized.py <one leg>.  Each leg prints the SHA-1 of
all its packets: DSV2HIP_LIB=<other build> with the plain legs alone runs a build without the sized calls, and must print the same."""
import ctypes as C
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, S, WARM, NVID = 1920, 64, 2, 2
SEMI, BGRA709 = 0x1, 0x110
LEGS = ["nv12_plain", "bgra_plain", "nv12_s1", "bgra_s1", "nv12_720", "nv12_480", "bgra_720", "bgra_480"]
SIZES = {"720": (1280, 720), "480": (854, 480)}


class SURFACE(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("layout", C.c_int)]


def main():
    argv = sys.argv[1:]
    steps = 24
    if argv[:1] == ["--steps"]:
        steps, argv = int(argv[1]), argv[2:]
    legs = argv or LEGS
    assert set(legs) <= set(LEGS), __doc__
    import numpy as np
    import torch
    import dsvabi as A
    from codec_run import configure_encoder
    from conftest import load_pkg
    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0
    P = C.POINTER
    hip.dsv2hip_enc_batch_surface.argtypes = [C.c_int, P(P(A.ENCODER)), P(SURFACE), P(A.BUF), P(C.c_int)]
    if any("_s" in leg for leg in legs):
        hip.dsv2hip_enc_batch_surface_scaled.argtypes = [C.c_int, P(P(A.ENCODER)), P(SURFACE), P(C.c_int), P(C.c_int), P(A.BUF), P(C.c_int)]
        hip.dsv2hip_enc_scale_stats.argtypes = [P(C.c_ulonglong), C.c_int]
    if any(leg.split("_")[1] in SIZES for leg in legs):
        hip.dsv2hip_enc_batch_surface_sized.argtypes = [C.c_int, P(P(A.ENCODER)), P(SURFACE), P(C.c_int), P(C.c_int), P(A.BUF), P(C.c_int)]
        hip.dsv2hip_enc_resize_stats.argtypes = [P(C.c_ulonglong), C.c_int]
    cw = W // 2
    content = {}

    def pictures(H):
        """NVID videos of W x H, WARM + steps packed planar pictures each, on the device"""
        if H not in content:
            vids = [load_pkg().synth.SynthVideo(W, H, "420", seed=401 + v) for v in range(NVID)]
            content[H] = [[torch.from_numpy(np.frombuffer(v.frame_bytes(t), dtype=np.uint8).copy()).cuda() for t in range(WARM + steps)] for v in vids]
        return content[H]

    def surface(p, kind, H):
        """tensors of packed picture p as an aligned NV12 / BGRA surface with tight rows"""
        ch = H // 2
        y, u, v = p[:W * H].view(H, W), p[W * H:W * H + cw * ch].view(ch, cw), p[W * H + cw * ch:].view(ch, cw)
        if kind == "nv12":
            tc = torch.empty((ch, W), dtype=torch.uint8, device="cuda")
            tc[:, 0::2], tc[:, 1::2] = u, v
            return [y.clone(), tc]
        yf = (y.float() - 16.0) * (255.0 / 219.0)  # BT.709 limited range, inverted in floating point
        uf = (u.float() - 128.0).repeat_interleave(2, 0).repeat_interleave(2, 1) * (255.0 / 224.0)
        vf = (v.float() - 128.0).repeat_interleave(2, 0).repeat_interleave(2, 1) * (255.0 / 224.0)
        r, g, b = yf + 1.5748 * vf, yf - 0.1873 * uf - 0.4681 * vf, yf + 1.8556 * uf
        t = torch.empty((H, 4 * W), dtype=torch.uint8, device="cuda")
        px = t.view(H, W, 4)
        for i, c in enumerate((b, g, r)):
            px[..., i] = c.round().clamp(0, 255).to(torch.uint8)
        px[..., 3] = 255
        return [t]

    for leg in legs:
        kind, how = leg.split("_")
        sized = how in SIZES
        s = int(how[1]) if how[0] == "s" else 0
        H = 1080
        ew, eh = SIZES[how] if sized else ((W + (1 << s) - 1) >> s, (H + (1 << s) - 1) >> s)
        meta = A.mk_meta(ew, eh, A.SUBSAMP_420)
        encs = [A.ENCODER() for _ in range(S)]
        for e in encs:
            configure_encoder(hip, e, meta, qp=60, gop=48)
        encp = (P(A.ENCODER) * S)(*[C.pointer(e) for e in encs])
        bufs, nbufs = (A.BUF * (4 * S))(), (C.c_int * S)()
        first = [[surface(p, kind, H) for p in vid] for vid in pictures(H)]
        keep, args = [], []
        for t in range(WARM + steps):
            arr = (SURFACE * S)()
            for k in range(S):
                own = [x.clone() for x in first[k % NVID][t]]
                keep.append(own)
                arr[k].layout = (SEMI if kind == "nv12" else BGRA709) | (s << 12)
                for i, x in enumerate(own):
                    assert x.data_ptr() % 16 == 0 and x.stride(0) % 16 == 0
                    arr[k].plane[i], arr[k].pitch[i] = x.data_ptr(), x.stride(0)
            args.append(arr)
        first = None
        sws, shs = (C.c_int * S)(*[W] * S), (C.c_int * S)(*[H] * S)
        torch.cuda.synchronize()
        if s:
            hip.dsv2hip_enc_scale_stats(None, 1)
        if sized:
            hip.dsv2hip_enc_resize_stats(None, 1)
        nbytes, digest = 0, hashlib.sha1()
        for t in range(WARM + steps):
            if t == WARM:
                t0 = time.perf_counter()
            if sized:
                assert hip.dsv2hip_enc_batch_surface_sized(S, encp, args[t], sws, shs, bufs, nbufs) == 0
            elif s:
                assert hip.dsv2hip_enc_batch_surface_scaled(S, encp, args[t], sws, shs, bufs, nbufs) == 0
            else:
                assert hip.dsv2hip_enc_batch_surface(S, encp, args[t], bufs, nbufs) == 0
            for k in range(S):
                for i in range(nbufs[k]):
                    nbytes += bufs[4 * k + i].len
                    digest.update(C.string_at(bufs[4 * k + i].data, bufs[4 * k + i].len))
                    hip.dsv_buf_free(C.byref(bufs[4 * k + i]))
        el = time.perf_counter() - t0
        form = ""
        if s:
            out = (C.c_ulonglong * 4)()
            hip.dsv2hip_enc_scale_stats(out, 0)
            form = "; scaled steps wide / general: YUV %d / %d, RGB %d / %d" % tuple(out)
        if sized:
            out = (C.c_ulonglong * 4)()
            hip.dsv2hip_enc_resize_stats(out, 0)
            form = "; sized steps wide / general: YUV %d / %d, RGB %d / %d" % tuple(out)
        print("%-10s source %dx%d -> encoders %dx%d, %d streams: %.1f frames/s, %.2f ms per step; %d packet bytes, sha1 %s%s"
              % (leg, W, H, ew, eh, S, S * steps / el, 1e3 * el / steps, nbytes, digest.hexdigest()[:16], form), flush=True)
        for e in encs:
            hip.dsv_enc_free(C.byref(e))
        keep = args = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
