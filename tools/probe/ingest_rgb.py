#!/usr/bin/env python3
"""Frames/s of the batch encoder fed from device-resident pictures three ways (experiments):
tools/probe/ingest_rgb.py [packed] [nv12] [bgra] [rgb24] [rgbp]   (default: the first three)
1080p 4:2:0, 192 streams in one lockstep group, 12 timed steps behind 2 warm-up steps:
  packed  dsv2hip_enc_batch on packed planar pictures (k_ingest16)
  nv12    dsv2hip_enc_batch_surface, NV12, pitch 2048 (k_ingest_surface<16>: 1.5 P bytes in, 1.5 P out)
  bgra    dsv2hip_enc_batch_surface, BGRA (BT.601, limited range), pitch 8192 (k_ingest_rgb<16>: 4 P bytes in, 1.5 P out)
  rgb24   dsv2hip_enc_batch_surface, BGR, three bytes a pixel, pitch 6144 (k_ingest_rgb3<packed, wide>: 3 P bytes in, 1.5 P out)
  rgbp    dsv2hip_enc_batch_surface, RGBP, three planes of pitch 2048 (k_ingest_rgb3<planar, wide>: 3 P bytes in, 1.5 P out)
Every stream reads memory of its own (copies of 4 videos: about 24 GB of BGRA surfaces, 9 GB of NV12), so no stream's reads are
served from the cache by another's.  The three legs encode the same pictures: the BGRA surfaces are made so that their conversion
is close to the packed pictures (not equal: the legs' packet bytes differ), which keeps the encoder's work behind the ingest alike.
Prints frames/s and the kernel launches of the ingest stage per step (dsv2hip_prof_read) for each.  The ingest kernels' time per
launch: rocprofv3 --kernel-trace --stats -- python tools/probe/ingest_rgb.py.  DSV2HIP_LIB=<other build> with `packed` alone runs
a build without the RGB layouts.  bgra, rgb24 and rgbp encode the same colours, so their packet bytes are equal."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, S, WARM, STEPS, NVID = 1920, 1080, 192, 2, 12, 4
PITCH, PITCH_RGB, PITCH_RGB24 = 2048, 8192, 6144
BGRA, BGR, RGBP = 0x10, 0x20, 0x22


class SURFACE(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("layout", C.c_int)]


def main():
    modes = sys.argv[1:] or ["packed", "nv12", "bgra"]
    import numpy as np
    import torch
    import dsvabi as A
    from codec_run import configure_encoder
    from conftest import load_pkg
    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0
    P = C.POINTER
    hip.dsv2hip_enc_batch.argtypes = [C.c_int, P(P(A.ENCODER)), P(C.c_void_p), P(A.BUF), P(C.c_int)]
    hip.dsv2hip_prof_enable.argtypes = [C.c_int]
    hip.dsv2hip_prof_read.argtypes = [P(C.c_double), P(C.c_longlong), P(C.c_longlong)]
    if set(modes) - {"packed"}:
        hip.dsv2hip_enc_batch_surface.argtypes = [C.c_int, P(P(A.ENCODER)), P(SURFACE), P(A.BUF), P(C.c_int)]
    cw, ch = W // 2, H // 2
    vids = [load_pkg().synth.SynthVideo(W, H, "420", seed=401 + v) for v in range(NVID)]
    packed = [[torch.from_numpy(np.frombuffer(v.frame_bytes(t), dtype=np.uint8).copy()).cuda() for t in range(WARM + STEPS)] for v in vids]

    def pitched(p, mode):
        """(tensors, layout) of packed picture p as a surface"""
        y, u, v = p[:W * H].view(H, W), p[W * H:W * H + cw * ch].view(ch, cw), p[W * H + cw * ch:].view(ch, cw)
        if mode == "nv12":
            ty = torch.zeros((H, PITCH), dtype=torch.uint8, device="cuda")
            ty[:, :W] = y
            tc = torch.zeros((ch, PITCH), dtype=torch.uint8, device="cuda")
            tc[:, 0:2 * cw:2], tc[:, 1:2 * cw:2] = u, v
            keep, layout = [ty, tc], 1
        else:  # BT.601 limited range, inverted in floating point: a picture whose conversion is near p
            yf = (y.float() - 16.0) * (255.0 / 219.0)
            uf = (u.float() - 128.0).repeat_interleave(2, 0).repeat_interleave(2, 1) * (255.0 / 224.0)
            vf = (v.float() - 128.0).repeat_interleave(2, 0).repeat_interleave(2, 1) * (255.0 / 224.0)
            r, g, b = yf + 1.402 * vf, yf - 0.344136 * uf - 0.714136 * vf, yf + 1.772 * uf
            b, g, r = (c.round().clamp(0, 255).to(torch.uint8) for c in (b, g, r))
            if mode == "rgbp":  # the same colours as three planes
                keep, layout = [], RGBP
                for c in (r, g, b):
                    t = torch.zeros((H, PITCH), dtype=torch.uint8, device="cuda")
                    t[:, :W] = c
                    keep.append(t)
            elif mode == "rgb24":  # ... and as three bytes a pixel
                t = torch.zeros((H, PITCH_RGB24), dtype=torch.uint8, device="cuda")
                px = t[:, :3 * W].view(H, W, 3)
                px[..., 0], px[..., 1], px[..., 2] = b, g, r
                keep, layout = [t], BGR
            else:
                t = torch.zeros((H, PITCH_RGB), dtype=torch.uint8, device="cuda")
                px = t[:, :4 * W].view(H, W, 4)
                px[..., 0], px[..., 1], px[..., 2] = b, g, r
                px[..., 3] = 255
                keep, layout = [t], BGRA
        return keep, layout

    def own(keep, layout):
        """a stream's own copy of a surface: (tensors kept alive, SURFACE)"""
        keep, sf = [t.clone() for t in keep], SURFACE()
        sf.layout = layout
        for i, t in enumerate(keep):
            sf.plane[i], sf.pitch[i] = t.data_ptr(), t.stride(0)
        return keep, sf

    meta = A.mk_meta(W, H, A.SUBSAMP_420)
    for mode in modes:
        encs = [A.ENCODER() for _ in range(S)]
        for e in encs:
            configure_encoder(hip, e, meta, qp=60, gop=48)
        encp = (P(A.ENCODER) * S)(*[C.pointer(e) for e in encs])
        bufs, nbufs = (A.BUF * (4 * S))(), (C.c_int * S)()
        # every stream reads memory of its own (copies of the NVID videos): no leg's reads are served by what another stream
        # of the step brought into the cache
        if mode == "packed":
            surf = [[packed[s % NVID][t].clone() for t in range(WARM + STEPS)] for s in range(S)]
            args = [(C.c_void_p * S)(*[surf[s][t].data_ptr() for s in range(S)]) for t in range(WARM + STEPS)]
            call = hip.dsv2hip_enc_batch
        else:
            first = [[pitched(p, mode) for p in vid] for vid in packed]
            surf = [[own(*first[s % NVID][t]) for t in range(WARM + STEPS)] for s in range(S)]
            first = None
            args = [(SURFACE * S)(*[surf[s][t][1] for s in range(S)]) for t in range(WARM + STEPS)]
            call = hip.dsv2hip_enc_batch_surface
        torch.cuda.synchronize()
        nbytes = 0
        for t in range(WARM + STEPS):
            if t == WARM:
                hip.dsv2hip_prof_enable(1)
                t0 = time.perf_counter()
            assert call(S, encp, args[t], bufs, nbufs) == 0
            for s in range(S):
                for i in range(nbufs[s]):
                    nbytes += bufs[4 * s + i].len
                    hip.dsv_buf_free(C.byref(bufs[4 * s + i]))
        el = time.perf_counter() - t0
        ms, ln, fr = (C.c_double * 9)(), (C.c_longlong * 9)(), C.c_longlong(0)
        hip.dsv2hip_prof_read(ms, ln, C.byref(fr))
        hip.dsv2hip_prof_enable(0)
        print("%-6s %dx%d %d streams: %.1f frames/s, %.2f ms per step; launches per step: ingest stage %.1f, all stages %.1f; %d packet bytes"
              % (mode, W, H, S, S * STEPS / el, 1e3 * el / STEPS, ln[0] / max(fr.value, 1), sum(ln[:8]) / max(fr.value, 1), nbytes), flush=True)
        for e in encs:
            hip.dsv_enc_free(C.byref(e))
        surf = args = None


if __name__ == "__main__":
    main()
