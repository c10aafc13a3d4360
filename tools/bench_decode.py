#!/usr/bin/env python3
"""Decode throughput of the lockstep batch decoder, same workload family as bench.py:
1080p 4:2:0 -qp=60 -gop=48 streams, S decoder instances per GPU in G lockstep groups.  Prints one JSON line.
The packets are produced on the fly with the GPU encoder (bit-identical to the reference's); every decoded
picture is delivered to host memory as a DSV_FRAME exactly like dsv_dec does (that D2H copy is part of the
timed region) -- or, with --device-out, through dsv2hip_dec_batch_device into one preallocated device buffer
per decoder, or, with --surface-out planar / nv12 / bgra, through dsv2hip_dec_batch_surface into one preallocated pitched surface per
decoder -- with --scale 2 / 4 / 8 at half, quarter or eighth size (DSV2HIP_SCALE_*), with --size WxH at that size
(dsv2hip_dec_batch_surface_sized) --, so that the deliveries can be compared."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
W_, H_, GOP, QP = 1920, 1080, 48, 60


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--draw-info", type=int, default=0, help="DSV_DECODER.draw_info of every decoder (0: no overlay)")
    ap.add_argument("--device-out", action="store_true", help="deliver the pictures to device memory (dsv2hip_dec_batch_device)")
    ap.add_argument("--postsharp", action="store_true", help="dsv2hip_dec_set_postsharp on every decoder")
    ap.add_argument("--surface-out", choices=["planar", "nv12", "bgra"], help="deliver the pictures into pitched device surfaces (dsv2hip_dec_batch_surface)")
    ap.add_argument("--scale", type=int, choices=[1, 2, 4, 8], default=1, help="with --surface-out: deliver at 1 / scale of the size (DSV2HIP_SCALE_HALF / _QUARTER / _EIGHTH)")
    ap.add_argument("--size", metavar="WxH", help="with --surface-out: deliver at this size, w / 8 .. w by h / 8 .. h (dsv2hip_dec_batch_surface_sized); not with --scale")
    ap.add_argument("--pitch-align", type=int, default=256, help="with --surface-out: every row pitch is the row's bytes rounded up to a multiple of this")
    args = ap.parse_args()
    assert not (args.device_out and args.surface_out), "--device-out and --surface-out are two deliveries"
    assert args.pitch_align >= 1
    assert args.scale == 1 or args.surface_out, "--scale belongs to a surface"
    assert not args.size or args.surface_out, "--size belongs to a surface"
    assert not args.size or args.scale == 1, "--size and --scale are two ways to a smaller picture"
    size = tuple(int(v) for v in args.size.lower().split("x")) if args.size else None
    assert size is None or (len(size) == 2 and size[0] > 0 and size[1] > 0), "--size WxH"
    import dsvabi as A
    from codec_run import decode_stream, encode_stream
    from conftest import load_pkg

    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0, "no HIP device: the product has no CPU path"
    hip.dsv2hip_dec_batch.argtypes = [C.c_int, C.POINTER(C.POINTER(A.DECODER)), C.POINTER(A.BUF), C.POINTER(C.POINTER(A.FRAME)),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    hip.dsv2hip_dec_batch.restype = C.c_int
    if args.device_out:
        import torch
        hip.dsv2hip_dec_batch_device.argtypes = [C.c_int, C.POINTER(C.POINTER(A.DECODER)), C.POINTER(A.BUF), C.POINTER(C.c_void_p),
                                                 C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        hip.dsv2hip_dec_batch_device.restype = C.c_int
    if args.surface_out:
        import torch

        class OUTSURF(C.Structure):  # dsv2hip_out_surface
            _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("cap", C.c_size_t * 3), ("layout", C.c_int)]

        hip.dsv2hip_dec_batch_surface.argtypes = [C.c_int, C.POINTER(C.POINTER(A.DECODER)), C.POINTER(A.BUF), C.POINTER(OUTSURF),
                                                  C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        hip.dsv2hip_dec_batch_surface.restype = C.c_int
        if size:
            hip.dsv2hip_dec_batch_surface_sized.argtypes = [C.c_int, C.POINTER(C.POINTER(A.DECODER)), C.POINTER(A.BUF), C.POINTER(OUTSURF), C.POINTER(C.c_int),
                                                            C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
            hip.dsv2hip_dec_batch_surface_sized.restype = C.c_int
    pkg = load_pkg()
    S, G, K, Wm = args.streams, max(1, min(args.groups, args.streams)), args.steps, args.warmup
    nfr = Wm + K
    # a few distinct videos, encoded once; streams reuse them
    vids = []
    for k in range(min(S, 4)):
        v = pkg.synth.SynthVideo(W_, H_, "420", seed=1 + k)
        uniq = [v.frame_bytes(t) for t in range(min(nfr, 24))]
        frames = [uniq[t % len(uniq)] if (t // len(uniq)) % 2 == 0 else uniq[len(uniq) - 1 - t % len(uniq)] for t in range(nfr)]
        pk = encode_stream(hip, frames, W_, H_, A.SUBSAMP_420, eos=False, qp=QP, gop=GOP, effort=10)[0]
        vids.append(pk)  # [meta, pic0, pic1, ...] (one metadata packet per GOP start)
    decs = [A.DECODER() for _ in range(S)]
    for d in decs:
        d.draw_info = args.draw_info
        if args.postsharp:
            hip.dsv2hip_dec_set_postsharp.argtypes = [C.POINTER(A.DECODER), C.c_int]
            assert hip.dsv2hip_dec_set_postsharp(C.byref(d), 1) == 0
    pic_bytes = W_ * H_ * 3 // 2
    dev_out = [torch.empty(pic_bytes, dtype=torch.uint8, device="cuda") for _ in range(S)] if args.device_out else None
    if dev_out:
        torch.cuda.synchronize()
    surf_out = None
    if args.surface_out:
        # one surface per decoder: every plane a tensor of its own, rows `pitch` apart
        # (bgra: DSV2HIP_SURFACE_BGRA | DSV2HIP_CSC_BT709 -- the BT.601 limited-range value at half size, 0x1010, is no layout)
        layout = {"planar": 0, "nv12": 1, "bgra": 0x110}[args.surface_out] | ({1: 0, 2: 1, 4: 2, 8: 3}[args.scale] << 12)
        # the planes' sizes from the library: a probe decoder reads the stream's metadata packet, dsv2hip_dec_surface_dims answers
        hip.dsv2hip_dec_surface_dims.argtypes = [C.POINTER(A.DECODER), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        hip.dsv2hip_dec_surface_dims.restype = C.c_int
        probe, pbuf, pfn = A.DECODER(), A.BUF(), C.c_uint32(0)
        hip.dsv_mk_buf(C.byref(pbuf), len(vids[0][0]) + 64)
        C.memmove(pbuf.data, vids[0][0], len(vids[0][0]))
        assert hip.dsv_dec(C.byref(probe), C.byref(pbuf), C.byref(C.POINTER(A.FRAME)()), C.byref(pfn)) == A.DEC_GOT_META
        rb, nrows = (C.c_size_t * 3)(), (C.c_int * 3)()
        if size:
            hip.dsv2hip_dec_sized_dims.argtypes = [C.POINTER(A.DECODER), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
            hip.dsv2hip_dec_sized_dims.restype = C.c_int
            assert hip.dsv2hip_dec_sized_dims(C.byref(probe), layout, size[0], size[1], rb, nrows) == 0, "--size: not a size the decoder delivers"
        else:
            assert hip.dsv2hip_dec_surface_dims(C.byref(probe), layout, rb, nrows) == 0
        hip.dsv_dec_free(C.byref(probe))
        rows = [(rb[i], nrows[i]) for i in range(3) if nrows[i]]
        assert sum(b * r for b, r in rows) == pic_bytes or args.scale > 1 or size or args.surface_out == "bgra"
        surf_out, keep = [], []
        for _ in range(S):
            c = OUTSURF()
            c.layout = layout
            for i, (rb, nr) in enumerate(rows):
                pitch = (rb + args.pitch_align - 1) // args.pitch_align * args.pitch_align
                t = torch.empty(pitch * nr, dtype=torch.uint8, device="cuda")
                keep.append(t)
                c.plane[i], c.pitch[i], c.cap[i] = t.data_ptr(), pitch, pitch * nr
            surf_out.append(c)
        torch.cuda.synchronize()
    group_of = [list(range(g, S, G)) for g in range(G)]

    def make_bufs(ids, t):
        m = len(ids)
        bufs = (A.BUF * m)()
        for i, s in enumerate(ids):
            pk = vids[s % len(vids)][t]
            hip.dsv_mk_buf(C.byref(bufs[i]), len(pk) + 64)
            C.memmove(bufs[i].data, pk, len(pk))
        return bufs

    npk = len(vids[0])
    assert all(len(v) == npk for v in vids)
    # packets [0, first) = warm-up (metadata + first pictures), then the timed ones
    first = npk - K if npk > K else 0
    plan = {g: [make_bufs(group_of[g], t) for t in range(npk)] for g in range(G)}
    decoded = [0] * G

    def worker(g, t0, t1, bar):
        ids = group_of[g]
        m = len(ids)
        decp = (C.POINTER(A.DECODER) * m)(*[C.pointer(decs[s]) for s in ids])
        outs = (C.POINTER(A.FRAME) * m)()
        fns = (C.c_uint32 * m)()
        rets = (C.c_int * m)()
        if dev_out:
            ptrs = (C.c_void_p * m)(*[dev_out[s].data_ptr() for s in ids])
            caps = (C.c_size_t * m)(*[pic_bytes] * m)
        if surf_out:
            surfs = (OUTSURF * m)(*[surf_out[s] for s in ids])
            ows, ohs = (C.c_int * m)(*[size[0] if size else 0] * m), (C.c_int * m)(*[size[1] if size else 0] * m)
        bar.wait()
        for t in range(t0, t1):
            if surf_out:
                had_meta = [decs[s].got_metadata for s in ids]
                if size:
                    assert hip.dsv2hip_dec_batch_surface_sized(m, decp, plan[g][t], surfs, ows, ohs, fns, rets) == m
                else:
                    assert hip.dsv2hip_dec_batch_surface(m, decp, plan[g][t], surfs, fns, rets) == m
                decoded[g] += sum(1 for i in range(m) if rets[i] == A.DEC_OK and had_meta[i])
                continue
            if dev_out:
                had_meta = [decs[s].got_metadata for s in ids]
                assert hip.dsv2hip_dec_batch_device(m, decp, plan[g][t], ptrs, caps, fns, rets) == m
                decoded[g] += sum(1 for i in range(m) if rets[i] == A.DEC_OK and had_meta[i])
                continue
            hip.dsv2hip_dec_batch(m, decp, plan[g][t], outs, fns, rets)
            for i in range(m):
                if rets[i] == A.DEC_OK and outs[i]:
                    decoded[g] += 1
                    hip.dsv_frame_ref_dec(outs[i])
        bar.wait()

    def run(t0, t1):
        bar = threading.Barrier(G + 1)
        ths = [threading.Thread(target=worker, args=(g, t0, t1, bar)) for g in range(G)]
        for th in ths:
            th.start()
        ts = time.perf_counter()
        bar.wait()
        bar.wait()
        te = time.perf_counter()
        for th in ths:
            th.join()
        return te - ts

    run(0, first)
    before = sum(decoded)
    import resource
    ru0 = resource.getrusage(resource.RUSAGE_SELF)
    elapsed = run(first, npk)
    ru1 = resource.getrusage(resource.RUSAGE_SELF)
    host_cpu_s = (ru1.ru_utime - ru0.ru_utime) + (ru1.ru_stime - ru0.ru_stime)
    nframes = sum(decoded) - before
    for d in decs:
        hip.dsv_dec_free(C.byref(d))
    fps = nframes / elapsed
    delivery = "device" if args.device_out else "host"
    where = delivery + " memory"
    if args.surface_out:
        smaller = "-%dx%d" % size if size else "" if args.scale == 1 else "-1/%d" % args.scale
        delivery = "surface-" + args.surface_out + smaller
        where = "%s device surfaces%s, pitch a multiple of %d" % (args.surface_out, " at %dx%d" % size if size else "" if args.scale == 1 else " at 1/%d of the size" % args.scale,
                                                                   args.pitch_align)
    result = {"metric": "decoded frames/s, 1080p 4:2:0 qp=60 gop=48 (pictures identical to the reference decoder's)", "value": round(fps, 2),
              "unit": "frames/s", "n_gpus": 1, "steps": npk - first, "ms_per_step": round(1e3 * elapsed / max(1, npk - first), 3),
              "higher_is_better": True, "dtype": "u8/int32", "data": "synthetic",
              "config": {"workload": "1920x1080 4:2:0 -qp=60 -gop=48, %d decoder instances in %d lockstep groups, frames delivered to %s" % (S, G, where),
                         "streams_per_gpu": S, "groups": G, "draw_info": args.draw_info, "delivery": delivery, "postsharp": args.postsharp, "host_cpu_cores_busy": round(host_cpu_s / elapsed, 2), "frames": nframes, "mpix_per_s": round(fps * W_ * H_ / 1e6, 1)}}
    if not args.no_cpu_baseline and os.path.exists(A.REF_SO):
        ref = A.load_ref()
        pk = vids[0][:25]
        t0 = time.perf_counter()
        out = decode_stream(ref, pk)
        dt = time.perf_counter() - t0
        result["cpu_baseline"] = {"value": round(len(out) / dt, 3), "unit": "frames/s", "cores": 1, "kind": "reference",
                                  "sample": "first %d pictures of stream 0, reference C decoder -O3, 1 thread" % len(out)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
