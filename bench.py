#!/usr/bin/env python3
"""Benchmark of the DSV2 encode hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run measures the headline and nothing else: it sets up, warms up, times exactly K steps, writes the last step's outputs
when --dump-outputs is given, and prints the JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step = the mean
wall time of one timed step).  Its pictures are made on the GPU (benchparts/synth_gpu.py, the bytes of the package's
generator).  Everything else described below -- the parity checks, the stage-timing pass and its roofline, the CPU
baselines, the decoder, the other configurations and legs -- runs only with --full.

Headline workload (BASELINE.json north star): synthetic 1920x1080 4:2:0, -qp=60 -gop=48, CRF, effort 10
(quarter-pel + EPRM + in-loop filters).  Every rank drives S independent closed-GOP streams on its GPU -- the
reference's own segment-parallel recipe (parallel_encode_yuv.sh:31-52) -- as G lockstep groups: each group is
one host thread calling dsv2hip_enc_batch_host() for its S/G encoder instances, so a kernel launch serves a
whole group and the groups overlap each other's host and device phases.  A "step" is one frame of every
stream: S frames per rank per step.

What the timed region contains: the pictures start in PINNED HOST memory and every frame's
host-to-device upload happens inside the region (the next step's pictures go up on a copy stream under the
current step's kernels), then the whole encode including host controller and entropy coding, up to the
finished packets in host memory.  The streams' GOP phases are staggered (stream s begins s mod 48 steps
before the others, in an untimed pre-roll), so every step -- and any window of steps -- carries the
steady-state share of intra pictures (1/48 of the streams per step) instead of one all-intra step per GOP.

With --full, bit-exactness is checked inside the run: a number of streams (two per lockstep group) are re-encoded by the
real reference (oracle/_ref, CPU) and compared byte for byte, and every stream has a twin with identical
input in ANOTHER lockstep group whose packets must be identical over the whole run.  A mismatch is fatal.

One JSON line is printed by rank 0: frames/s aggregated over all ranks (weak scaling) and, with --full, the roofline object of
the dominant kernel (HIP-event stage spans measured in a short extra pass of the same configuration), the CPU
baselines (the real reference on one thread, and 8 processes on closed-GOP streams as in
parallel_encode_yuv.sh) and -- at N=1 -- the other BASELINE.json configurations and the decoder.

`--gpus N` without a launcher starts the N ranks itself (one process per GPU, torch.distributed over
RCCL); under torchrun it reads RANK / LOCAL_RANK / WORLD_SIZE from the environment.
"""
import argparse
import ctypes as C
import json
import os
import socket
import struct
import subprocess
import sys
import tempfile
import threading
import time

# the lockstep groups each drive their own HIP stream; give them hardware queues of their own
# (ROCm maps streams onto 4 by default).  Must be set before the HIP runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

# The parts (benchparts/): common = constants, host placement, picture generators, EncodeRun (its run() is the timed region);
# roofline = objects built from committed profile passes; reference = the real reference as checker and CPU baseline;
# extras = every leg beside the headline.  This file: arguments, rank start-up, and main() -- headline, roofline, the legs in order.
from benchparts.common import *  # noqa: E402,F401,F403
from benchparts.common import _parse_cpulist  # noqa: E402,F401  (tests/test_bench_host.py)
from benchparts.extras import (api_process_leg, api_thread_legs, batch_curve, class_legs, decode_leg, host_share,  # noqa: E402
                               multi_rank_one_gpu, other_configs)
from benchparts.reference import RefCheck, reference_phase  # noqa: E402
from benchparts.roofline import census_report, issue_roofline  # noqa: E402

def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--streams", type=int, default=int(os.environ.get("DSV2_STREAMS", "768")),
                    help="independent closed-GOP streams (encoder instances) per GPU")
    ap.add_argument("--groups", type=int, default=int(os.environ.get("DSV2_GROUPS", "4")),
                    help="lockstep groups per GPU, one host thread + HIP stream each")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the reference CPU runs (also skips the parity check against them)")
    ap.add_argument("--no-extras", action="store_true", help="skip the other BASELINE.json configurations and the decode leg")
    ap.add_argument("--no-profile", action="store_true", help="skip the extra stage-timing pass that feeds the roofline object")
    ap.add_argument("--no-stagger", action="store_true", help="all streams start their GOP together (one all-intra step per GOP)")
    ap.add_argument("--no-phase-align", action="store_true",
                    help="spread every step's intra pictures over all lockstep groups (round 2's layout) instead of giving them to one group")
    ap.add_argument("--host-cores", type=int, default=0,
                    help="pin this rank to N of its usable cores (sched_setaffinity, after any host-made pictures are generated and before "
                         "anything touches the GPU) and size the library's worker pool from them: does the host side fit N cores per GPU?")
    ap.add_argument("--no-mix", action="store_true", help="every stream pans (round 2's content): no scene-cut / static / fast-motion classes")
    ap.add_argument("--no-batch-curve", action="store_true", help="skip the small-batch operating points (1 / 8 / 48 / 192 streams)")
    ap.add_argument("--only-batch-curve", action="store_true", help="of the extras, run only the small-batch operating points (experiments)")
    ap.add_argument("--no-host-share", action="store_true", help="skip the 2-host-cores re-run of the headline")
    ap.add_argument("--no-api-legs", action="store_true", help="skip the legs through the reference's own entry points (threads of dsv_enc / dsv_dec, 8 drop-in CLI processes)")
    ap.add_argument("--only-api-legs", action="store_true", help="of the extras, run only those legs (experiments)")
    ap.add_argument("--device-resident", action="store_true",
                    help="pictures parked in HBM before the clock starts (kernel-side figure; NOT the SURVEY 8d metric)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for exercising the N>1 path "
                                                      "on a box with fewer GPUs than ranks, together with DSV2_FORCE_DEVICE)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed and run the segment gather even with ONE rank "
                    "(exercises RCCL init + collectives on a single GPU)")
    ap.add_argument("--no-multi-rank", action="store_true", help="skip the 8-ranks-on-one-GPU leg")
    ap.add_argument("--decode-too", action="store_true", help="with --full --no-extras: still run the decode leg on the run's packets (the 2-host-core re-run uses it)")
    ap.add_argument("--profile-steps", type=int, default=6)
    ap.add_argument("--gen-procs", type=int, default=-1,
                    help="with --full: helper processes that generate the synthetic pictures on the host (default: the usable cores, 1 under "
                         "a profiler: forked children of a process with rocprofv3's tool library loaded can hang at exit)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: the stage-timing pass and its roofline, the twin and reference parity "
                         "checks, the CPU baselines, the decode leg and (at N=1) the other configurations and legs; the --no-* / --only-* "
                         "options above choose among them.  Without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed encode returned in its last step as DIR/<name>.npy (float32 / float64)")
    return ap.parse_args()


DUMP_SAMPLE_STREAMS = 64      # streams whose packets --dump-outputs writes byte for byte (a fixed, seeded choice)
DUMP_MAX_BYTES = 15 << 20     # packet bytes written at most (as float32: 60 MB; the rest of the dump is a few kB)


def dump_outputs(path, last_step):
    """--dump-outputs: what the timed encode returned in its last step (rank 0's streams).  last_step[s] = the packets stream s received.
      packet_bytes_per_stream.npy   float64 [S]   bytes of every stream's packets
      sample_streams.npy            float64 [k]   the sampled streams (seeded choice of DUMP_SAMPLE_STREAMS, ascending)
      sample_packet_offsets.npy     float64 [k+1] where each sampled stream's bytes begin in sample_packets.npy
      sample_packets.npy            float32 [n]   the sampled streams' packets, concatenated, byte values 0..255
                                                  (cut at DUMP_MAX_BYTES; the offsets still count the full lengths)"""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    S = len(last_step)
    per_stream = [b"".join(pk) for pk in last_step]
    sample = np.sort(np.random.RandomState(20240611).choice(S, min(S, DUMP_SAMPLE_STREAMS), replace=False))
    blob = b"".join(per_stream[s] for s in sample)
    offsets = np.concatenate([[0], np.cumsum([len(per_stream[s]) for s in sample])])
    np.save(os.path.join(path, "packet_bytes_per_stream.npy"), np.array([len(b) for b in per_stream], dtype=np.float64))
    np.save(os.path.join(path, "sample_streams.npy"), sample.astype(np.float64))
    np.save(os.path.join(path, "sample_packet_offsets.npy"), offsets.astype(np.float64))
    np.save(os.path.join(path, "sample_packets.npy"), np.frombuffer(blob[:DUMP_MAX_BYTES], dtype=np.uint8).astype(np.float32))


def spawn_ranks(args):
    """--gpus N without a launcher: N fresh processes, one per GPU.  This parent never touches the GPU."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    sys.exit(rc)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if args.gpus != world:
        sys.stderr.write("[bench] --gpus %d but WORLD_SIZE=%d: running %d ranks\n" % (args.gpus, world, world))
    local = int(os.environ.get("DSV2_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    # this rank's cores: those next to its GPU (before the picture generators fork, the pictures are pinned, the runtime starts)
    locality = bind_rank_to_gpu_node(local, world if "DSV2_FORCE_DEVICE" not in os.environ else 1)
    ncpu_box = usable_cpus()
    extras = args.full and not args.no_extras and world == 1

    # ---- pictures first: forked generators must not inherit an initialised GPU runtime ----
    W_, H_, GOP, QP = 1920, 1080, 48, 60
    # Content: 96 distinct videos of 64 unique frames per GPU for the headline (no input shared beyond the twin of a stream and,
    # at 768 streams, three more streams that start 2 / 4 / 6 frames into the same video) -- 19 GB of pinned pictures per rank,
    # taken only when the host has room for every rank's share twice over; else 8 x 32 (round 4's content), said on the line.
    def mem_available():
        try:
            return int(next(l for l in open("/proc/meminfo") if l.startswith("MemAvailable")).split()[1]) * 1024
        except (OSError, StopIteration, ValueError):
            return 0
    if args.streams >= 192 and not os.environ.get("DSV2_BENCH_SMALL_CONTENT") and not under_profiler_():
        NV, NF = 96, 64
        if mem_available() < 2.2 * world * NV * NF * (W_ * H_ * 3 // 2):
            NV, NF = 8, 32
        NV, NF = agree_once("content", world, (NV, NF))  # ONE decision per job: ranks that looked at /proc/meminfo at different moments must not differ
    elif args.streams >= 16:
        NV, NF = 8, 32
    else:
        NV, NF = max(1, min(4, args.streams // 2)), 24
    seeds = [1 + rank * NV + k for k in range(NV)]
    specs = [(W_, H_, "420", seeds[k], NF) for k in range(NV)]
    if extras:
        specs += [(1280, 720, "420", 101 + k, 24) for k in range(4)]
        specs += [(W_, H_, "444", 201, 12)]
        specs += [(3840, 2160, "420", 301 + k, 16) for k in range(2)]
        specs += [(1920, 800, "420", 401 + k, 16) for k in range(2)]
    t_gen = time.perf_counter()
    # A plain run makes the headline's pictures on the GPU once it is up (benchparts/synth_gpu.py: the same bytes, in a fraction of the
    # time); --full and a run under a profiler (whose kernel traces must hold the codec's kernels only) make them here, on the host.
    vids = None
    under_profiler = under_profiler_()
    if args.full or under_profiler:
        gen_procs = args.gen_procs if args.gen_procs > 0 else (1 if under_profiler else max(1, min(16, ncpu_box // (1 if locality["bound"] else max(1, world)))))
        vids = gen_videos(specs, gen_procs)
    t_gen = time.perf_counter() - t_gen
    host_pictures = vids is not None

    # ---- the host budget of this rank: pinned BEFORE the GPU runtime and the library's worker pool come up ----
    if args.host_cores > 0:
        cores = sorted(os.sched_getaffinity(0))
        k0 = (rank * args.host_cores) % max(1, len(cores))
        mine = [cores[(k0 + i) % len(cores)] for i in range(min(args.host_cores, len(cores)))]
        os.sched_setaffinity(0, mine)
    ncpu = usable_cpus() if args.host_cores <= 0 else min(usable_cpus(), args.host_cores)
    # host phases run on a worker pool inside the library: share the usable cores between the ranks
    if args.host_cores > 0:
        os.environ.setdefault("DSV2_HOST_THREADS", str(max(2, 2 * ncpu)))
    else:
        os.environ.setdefault("DSV2_HOST_THREADS", str(min(48, max(8, 3 * ncpu // (1 if locality["bound"] else max(1, world))))))

    import torch
    import dsvabi as A
    dist = None
    if world > 1 or args.force_dist:
        if world == 1 and "MASTER_PORT" not in os.environ:
            so = socket.socket()
            so.bind(("127.0.0.1", 0))
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(so.getsockname()[1]), RANK="0", WORLD_SIZE="1")
            so.close()
        import torch.distributed as dist_
        dist = dist_
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    torch.cuda.set_device(local)
    locality = bind_rank_late(locality, world if "DSV2_FORCE_DEVICE" not in os.environ else 1, torch, local)
    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0, "no HIP device: the product has no CPU path"
    hip.dsv2hip_set_device(local)
    bind_abi(hip, A)
    from conftest import load_pkg
    pkg = load_pkg()
    if vids is None:
        from benchparts.synth_gpu import DeviceVideo
        vids = [DeviceVideo(*spec, dev=torch.device("cuda", local)) for spec in specs]

    S, K, Wm = max(1, args.streams), args.steps, args.warmup
    effort = int(os.environ.get("DSV2_BENCH_EFFORT", "10"))  # (experiments only: the headline is effort 10)
    align = not args.no_phase_align
    mix = None if args.no_mix else MIX
    torch.cuda.synchronize()
    hbm_free0 = torch.cuda.mem_get_info()[0]
    t_setup = time.perf_counter()
    run = EncodeRun(hip, A, torch, W_, H_, "420", QP, GOP, effort, S, args.groups, vids[:NV], not args.no_stagger, args.device_resident,
                    seeds=seeds, phase_align=align, mix=mix, timed_from=(GOP if not args.no_stagger else 0) + Wm, timed_steps=K)
    t_setup = time.perf_counter() - t_setup
    G = run.G
    hip.dsv2hip_prof_enable(0)
    run.run(run.R + Wm)                   # untimed: GOP-phase pre-roll + warm-up (allocations, clocks)
    torch.cuda.synchronize()
    hbm_per_instance = (hbm_free0 - torch.cuda.mem_get_info()[0]) / S  # every instance has coded intra and inter pictures by now
    import resource
    thr0 = thread_cpu() if os.environ.get("DSV2_BENCH_THREADS") else None
    ru0 = resource.getrusage(resource.RUSAGE_SELF)
    g_timed = run.step
    census_on = args.full and bool(os.environ.get("DSV2_CENSUS"))
    if census_on:  # a `make census` build (DSV2HIP_LIB): resident wavefront-time per kernel, measured inside the kernels under load
        torch.cuda.synchronize()
        hip.dsv2hip_census_reset()
    elapsed = run.run(K, dist, record=True)   # timed: exactly K steps
    last_step = [run.out[s][-1] for s in range(S)] if args.dump_outputs else None  # per stream: the packets of the last timed step
    census = census_report(hip, elapsed) if census_on else None
    ru1 = resource.getrusage(resource.RUSAGE_SELF)
    if thr0 is not None:  # where the host CPU of the timed region went, by thread (name, seconds)
        thr1 = thread_cpu()
        rows = sorted(((thr1[t][1] - thr0.get(t, (None, 0.0))[1], thr1[t][0], t) for t in thr1), reverse=True)
        sys.stderr.write("[bench] host CPU by thread over %.2f s: %s\n" % (elapsed, ", ".join("%s/%d %.2f" % (nm, t, d) for d, nm, t in rows[:24] if d > 0.005)))
    if os.environ.get("DSV2_BENCH_STEP_SERIES"):  # drift inside the timed region: mean step time of each group, per dozen steps
        for g, ser in enumerate(run.step_ms):
            sys.stderr.write("[bench] group %d step ms per dozen: %s\n" % (g, " ".join("%.1f" % (sum(ser[i:i + 12]) / max(1, len(ser[i:i + 12]))) for i in range(0, len(ser), 12))))
    step_ms = sorted(x for g in run.step_ms for x in g)
    in_call_share = [round(x / elapsed, 3) for x in run.in_call_s]
    host_cpu_s = (ru1.ru_utime - ru0.ru_utime) + (ru1.ru_stime - ru0.ru_stime)
    frames_rank = run.frames_in(g_timed, g_timed + K)
    intra_rank = run.intra_in(g_timed, g_timed + K)
    classes = run.class_report(g_timed, g_timed + K)

    # stage profile: a few more steps of the SAME configuration with HIP-event stage timing on (not timed)
    stage_ms, stage_launches, stage_units, prof_steps = None, None, None, 0
    if args.full and not args.no_profile:
        hip.dsv2hip_prof_enable(1)
        run.run(args.profile_steps)
        if rank == 0:
            ms = (C.c_double * 16)()
            ln = (C.c_longlong * 16)()
            un = (C.c_longlong * 16)()
            fr = C.c_longlong(0)
            hip.dsv2hip_prof_read(ms, ln, C.byref(fr))
            hip.dsv2hip_prof_read_units(un)
            stage_ms, stage_launches, stage_units, prof_steps = list(ms), list(ln), list(un), fr.value
        hip.dsv2hip_prof_enable(0)

    # ---- parity, part 1 (every rank): twin streams in different lockstep groups produced identical packets ----
    pairs, bad = run.twins_equal() if args.full else (0, 0)
    if bad:
        sys.stderr.write("[bench] rank %d: %d of %d twin stream pairs DIFFER -- output is not deterministic\n" % (rank, bad, pairs))
        sys.exit(3)

    # final ordered gather of the segment bytes (the only exchange of the path); a rank's streams are the closed-GOP
    # segments sharding.assign_segments deals to it round-robin: global id = local index * world + rank
    xdev = "cuda" if args.backend == "nccl" else "cpu"
    t_max = torch.tensor([elapsed], device=xdev, dtype=torch.float64)
    counts = torch.tensor([frames_rank, intra_rank, pairs], device=xdev, dtype=torch.int64)
    gather_s = None
    if dist is not None:
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        assert pkg.sharding.assign_segments(S * world, world)[rank] == [pkg.sharding.segment_id(rank, world, s) for s in range(S)]
        # Every segment of the job travels to rank 0 and is checked there against its producer's md5 -- in pieces of at most
        # 256 MB that rank 0 folds into running digests and drops (sharding.gather_segments_streaming): eight ranks of the
        # headline produce ~58 GB, which no rank ever holds.  (DSV2_GATHER_OUT=<file>: rank 0 also writes every piece at its
        # final offset of that file, the `cat` of parallel_encode_yuv.sh:50.)
        out_path = os.environ.get("DSV2_GATHER_OUT")
        out_fd = os.open(out_path, os.O_RDWR | os.O_CREAT | os.O_TRUNC) if (rank == 0 and out_path) else -1
        sink = (lambda sid, base, off, piece: os.pwrite(out_fd, piece, base + off)) if out_fd >= 0 else None
        chunk = int(float(os.environ.get("DSV2_GATHER_CHUNK_MB", "256")) * (1 << 20))
        t_g = time.perf_counter()
        res = pkg.sharding.gather_segments_streaming(dist, rank, world, [pkg.sharding.segment_id(rank, world, s) for s in range(S)],
                                                     lambda sid: run.stream_bytes((sid - rank) // world), device=xdev, chunk=chunk, sink=sink)
        gather_s = time.perf_counter() - t_g
        if out_fd >= 0:
            os.close(out_fd)
        total_bytes = res["bytes"] if rank == 0 else 0
        gather_ok = None
        if rank == 0:
            gather_ok = {"segments": res["segments"], "segments_verified": res["segments_verified"], "bytes": res["bytes"], "segments_of_job": S * world,
                         "segments_over_the_wire": res["segments_over_the_wire"], "digest": res["digest"],
                         "rank0_peak_bytes_held": res["peak_bytes_held"],
                         "form": "streaming: a digest per segment folded piece by piece on a checker thread while the next piece is on the wire, pieces dropped"}
            if res["segments_verified"] != res["segments"] or res["segments"] != S * world:
                sys.stderr.write("[bench] gathered segment bytes DIFFER from what the ranks produced (%d of %d ok, job has %d)\n"
                                 % (res["segments_verified"], res["segments"], S * world))
                sys.exit(8)
        # per rank: where its host side ran and what it moved
        mine_info = {"rank": rank, "gpu": local, "pci": locality["pci"], "numa_node": locality["numa_node"], "cpus": locality["cpus"], "bound": locality["bound"],
                     "frames_per_s": round(frames_rank / elapsed, 1),
                     "h2d_GBps": 0.0 if args.device_resident else round(frames_rank * run.P / elapsed / 1e9, 2)}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine_info)
    else:
        total_bytes = sum(len(p) for s in range(S) for fr in run.out[s] for p in fr)
        gather_ok = None
        per_rank = [{"rank": 0, "gpu": local, "pci": locality["pci"], "numa_node": locality["numa_node"], "cpus": locality["cpus"], "bound": locality["bound"],
                     "frames_per_s": round(frames_rank / elapsed, 1),
                     "h2d_GBps": 0.0 if args.device_resident else round(frames_rank * run.P / elapsed / 1e9, 2)}]
    elapsed = float(t_max.item())
    frames_total, intra_total, pairs_total = (int(x) for x in counts.tolist())

    if rank != 0:
        run.free()
        if dist is not None:
            dist.destroy_process_group()
        return

    fps = frames_total / elapsed
    sb, frame_bytes = stage_bytes(W_, H_, "420")
    result = {
        "metric": "encoded frames/s, 1080p 4:2:0 qp=60 gop=48, incl. H2D upload of every frame (bit-exact .dsv)",
        "value": round(fps, 2),
        "unit": "frames/s",
        "n_gpus": world,
        "steps": K,
        "warmup": Wm,
        "ms_per_step": round(1000.0 * elapsed / K, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8/int32",
        "data": "synthetic",
        "config": {"workload": "1920x1080 4:2:0 -qp=60 -gop=48 effort=%d CRF, %d closed-GOP streams per GPU in %d lockstep groups; "
                               "pictures in %s; GOP phases %s; content: %s" %
                               (effort, S, G, "HBM before the clock starts (kernel-side figure)" if args.device_resident else
                                "pinned host memory, every frame uploaded inside the timed region (double-buffered copy stream)",
                                ("staggered over %d untimed pre-roll steps: every step codes 1/%d of the streams as intra pictures%s" %
                                 (run.R, GOP, ", all of them in ONE lockstep group (phase-aligned groups)" if run.phase_aligned else ""))
                                if run.R else "aligned: one all-intra step per GOP",
                                "of ten twin pairs seven pan, one has a scene cut inside the timed window, one is static, one moves three frames per step"
                                if mix else "every stream pans"),
                   "streams_per_gpu": S, "frames_per_step_per_gpu": S, "groups": G, "frames_timed": frames_total, "intra_frames_timed": intra_total,
                   "phase_aligned_groups": run.phase_aligned,
                   "content_classes": classes,
                   "input": "pinned_host" if not args.device_resident else "device_resident", "h2d_bytes_per_step_per_gpu": 0 if args.device_resident else S * run.P,
                   "distinct_videos_per_gpu": NV, "unique_frames_per_video": NF,
                   "hbm_bytes_per_instance": int(hbm_per_instance), "hbm_bytes_instances_total": int(hbm_per_instance * S),
                   "ms_per_frame_p50": round(step_ms[len(step_ms) // 2], 3) if step_ms else None,
                   "group_time_inside_library": in_call_share,
                   "host_cpu_cores_busy": round(host_cpu_s / elapsed, 2), "mpix_per_s": round(fps * W_ * H_ / 1e6, 1),
                   "stream_bytes_total": total_bytes, "host_cpus_usable": ncpu, "host_cores_pinned": args.host_cores or None,
                   "host_threads": int(os.environ["DSV2_HOST_THREADS"]),
                   "final_gather_s": round(gather_s, 3) if gather_s is not None else None, "final_gather_check": gather_ok,
                   "exchange_backend": (args.backend if dist is not None else None),
                   "per_rank": per_rank,
                   "setup_s": ({"generate_pictures": round(t_gen, 1)} if host_pictures else
                               {"pictures_made_on_gpu_and_encoders": round(t_setup, 1)})},
    }
    if args.full:
        result["parity_checked"] = {"twin_pairs_equal": pairs_total, "twin_pairs": pairs_total,
                                    "note": "twins = same input, different lockstep group (and GOP phase), compared frame by frame over the run"}
    if census is not None:
        result["census"] = census
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last_step)
    if stage_ms is not None and prof_steps:
        # per stage: span (HIP events on the group's stream) per stream-frame, and the algorithmic
        # bytes of SURVEY.md 8(d) moved in that span
        per_unit = {STAGES[i]: (stage_ms[i] / stage_units[i] if stage_units[i] else 0.0) for i in range(NST)}
        total_ms = {STAGES[i]: stage_ms[i] for i in range(8)}
        # The dominant KERNEL is the level-0 launch of the search (its span is measured on its own): the largest single kernel of
        # the rocprofv3 summary of this command (profiles/r05_rocprof_kernel_stats.txt).  The largest STAGE span is reported beside
        # it -- a stage is several kernels (quantise + compact + entropy is ~25 launches per plane class), and under four
        # concurrent groups its span is mostly the other groups' kernels sharing the chip.
        largest_stage = max(total_ms, key=lambda k: total_ms[k])
        dom = "hme_level0"
        i = STAGES.index(dom)
        nl = max(1, stage_launches[i])
        avg_launch_ms = stage_ms[i] / nl
        bytes_per_launch = sb[dom] * stage_units[i] / nl
        achieved = bytes_per_launch / (avg_launch_ms * 1e-3) / 1e9
        # HBM traffic per launch of the dominant kernel cannot be read inside this process: it comes from the separate
        # rocprofv3 --pmc passes of tools/profile_round.sh (profiles/pmc_traffic.json) and is only quoted for the
        # configuration those passes were taken on (streams, groups, GOP-phase layout)
        traffic, traffic_source = None, None
        try:
            pt = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
            same = (pt.get("stage") == dom and pt.get("streams_per_gpu") == S and pt.get("groups") == G and pt.get("kernel") == STAGE_KERNEL[dom]
                    and bool(pt.get("stagger", False)) == bool(run.R) and bool(pt.get("phase_aligned", False)) == run.phase_aligned)
            # ... and only for the KERNEL they were taken on: the committed figure carries a hash of the search's sources
            import hashlib
            hh = hashlib.sha256()
            for fn in ("hme.hip", "hme_fast.h", "hme.h", "blockstat.h", "dev.h"):
                hh.update(open(os.path.join(ROOT, "digital-subband-video-2_amd", "csrc", fn), "rb").read())
            fresh = pt.get("kernel_source_sha16") == hh.hexdigest()[:16]
            if same and fresh:
                traffic = pt.get("bytes_per_launch")
                traffic_source = "committed PMC passes, not this run: " + pt.get("source", "profiles/pmc_traffic.json")
            elif same:
                traffic_source = "profiles/pmc_traffic.json is STALE (taken on other search sources: kernel_source_sha16 differs): not quoted"
        except (OSError, ValueError):
            pass
        # (advisor, round 5) the stage with the largest span, priced the same way: its algorithmic bytes over its span per stream-frame
        ls_i = STAGES.index(largest_stage)
        ls_rate = (sb[largest_stage] / (per_unit[largest_stage] * 1e-3) / 1e9) if per_unit.get(largest_stage) else 0.0
        result["roofline"] = {"bound": "hbm", "kernel": STAGE_KERNEL[dom], "stage": dom,
                              "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": traffic, "traffic_source": traffic_source,
                              "avg_launch_us": round(avg_launch_ms * 1e3, 2),
                              "launches_per_step": round(nl / prof_steps * G, 1),
                              "algorithmic_bytes_per_launch": round(bytes_per_launch),
                              "stage_us_per_frame": {k: round(1e3 * v, 2) for k, v in per_unit.items()},
                              "largest_stage_span": largest_stage,
                              "largest_stage_roofline": {"stage": largest_stage, "launches_per_step": round(stage_launches[ls_i] / prof_steps * G, 1),
                                                         "algorithmic_bytes_per_frame": round(sb[largest_stage]),
                                                         "span_us_per_frame": round(1e3 * per_unit[largest_stage], 2), "achieved": round(ls_rate, 2),
                                                         "frac": round(ls_rate / HBM_PEAK_GBS, 6),
                                                         "note": "a stage is several kernels; under four concurrent groups its span is mostly other groups' kernels sharing the chip"},
                              "whole_frame_algorithmic_GBps": round(frame_bytes * fps / 1e9, 1),
                              "note": "the search is an integer kernel bound by instruction issue and dependent latencies, not by bandwidth: "
                                      "see roofline.issue for the roofline that binds the pipeline"}
        iss = issue_roofline(fps, world)
        if iss:
            result["roofline"]["issue"] = iss

    # ---- legs whose packets the reference will re-encode (collected now, compared at the end, all at once) ----
    checks = []
    sel = run.pick_reference_streams(NREF_STREAMS) if args.full else []
    for s in sel:
        checks.append(RefCheck("headline", run, s, NREF_FRAMES))

    # ---- the decoder on this run's packets (N = 1 only) ----
    # (the headline above is complete: whatever goes wrong below is reported beside it, never instead of it)
    dec_md5 = {}
    if (extras or (args.full and args.decode_too)) and not args.only_batch_curve and not args.only_api_legs:
        try:
            # The decode leg's shape: 256 decoders in 4 groups where the HOST parses the plane sections (16 cores' worth of parsing: more
            # decoders do not help); as many decoders as the run has streams (768) in 8 groups where the DEVICE parses them -- a section is one
            # wavefront's 40 ms chain whatever the batch, so that path's throughput is the decoders in flight.
            # (DSV2_DEC_GROUPS / DSV2_DEC_STREAMS: experiments.)
            hip.dsv2hip_dec_parse_mode.restype = C.c_int
            mode0 = hip.dsv2hip_dec_parse_mode()
            want = sel if (extras and not args.no_cpu_baseline) else []

            def leg_shape(on_device):
                d = int(os.environ.get("DSV2_DEC_STREAMS", str(min(S, 768) if on_device else 256)))
                g = int(os.environ.get("DSV2_DEC_GROUPS", "8" if on_device else "4"))
                return d, g
            d0, g0 = leg_shape(mode0 != 0)
            result["decode"], dec_md5 = decode_leg(hip, A, run, 32, d0, g0, want)
            result["decode"]["plane_sections_parsed_on"] = ["host", "device (P pictures)", "device"][mode0]
            # the other parser on the same packets: the device's where the library chose the host (a box with >= 12 usable cores), at its
            # own shape and at the host leg's 256 decoders; the pictures of the streams the reference checks must be identical
            if mode0 == 0 and extras:
                hip.dsv2hip_dec_set_parse_mode(1)
                try:
                    d1, g1 = leg_shape(True)
                    leg, md5b = decode_leg(hip, A, run, 32, d1, g1, want)
                    leg["plane_sections_parsed_on"] = "device (P pictures)"
                    leg["pictures_equal_to_the_host_parsed_leg"] = bool(md5b == dec_md5)
                    leg.pop("roofline", None)
                    small, md5c = decode_leg(hip, A, run, 32, d0, g0, want)
                    leg["pictures_equal_to_the_host_parsed_leg"] = leg["pictures_equal_to_the_host_parsed_leg"] and bool(md5c == dec_md5)
                    leg["at_the_host_legs_shape"] = {k: small.get(k) for k in ("value", "decoders", "groups", "host_cpu_cores_busy")}
                    result["decode_device_parse"] = leg
                finally:
                    hip.dsv2hip_dec_set_parse_mode(-1)
        except Exception as e:  # noqa: BLE001
            result["decode"] = {"error": repr(e)}
    run.free()
    del run

    # ---- the other BASELINE.json configurations and the small-batch operating points (N = 1 only) ----
    if extras and not args.only_batch_curve and not args.only_api_legs:
        try:
            result["configs"] = other_configs(hip, A, torch, args, vids, NV, S, W_, H_, seeds, checks)
        except Exception as e:  # noqa: BLE001
            result["configs"] = {"error": repr(e)}
    if extras and not args.no_batch_curve and not args.only_api_legs:
        try:
            result["batch_curve"] = batch_curve(hip, A, torch, args, vids, NV, seeds, W_, H_, QP, GOP, effort, checks)
            one = next((p for p in result["batch_curve"] if p.get("streams") == 1), None)
            if one:  # BASELINE.json config 5 as literally written: ONE closed-GOP segment per GPU at a time
                result["config5_one_stream_per_gpu"] = {
                    "value": one["value"], "unit": "frames/s per GPU", "ms_per_frame_p50": one["ms_per_frame_p50"],
                    "note": "one stream alone on the GPU: every frame is the chain coarse search levels -> level 0 -> in-loop filter sweep, "
                            "the reference's own data dependencies; the headline is the same hardware with 768 such segments in flight "
                            "(parallel_encode_yuv.sh:31-52 runs as many segments as it has processes)"}
        except Exception as e:  # noqa: BLE001
            result["batch_curve"] = {"error": repr(e)}
    if extras and not args.no_mix and not args.only_batch_curve and not args.only_api_legs:
        try:
            result["content_class_legs"] = class_legs(hip, A, torch, args, vids, NV, seeds, W_, H_, QP, GOP, effort, checks)
        except Exception as e:  # noqa: BLE001
            result["content_class_legs"] = {"error": repr(e)}

    # ---- the reference's own entry points and its own parallel recipe (row h of the round-3 review) ----
    if extras and not args.only_batch_curve and not args.no_api_legs:
        try:
            result["api_legs"] = api_thread_legs(hip, A, vids, NV, seeds, W_, H_, QP, GOP, effort, checks)
        except Exception as e:  # noqa: BLE001
            result["api_legs"] = {"error": repr(e)}
        try:
            result["api_legs"]["processes"] = api_process_leg(vids, W_, H_, QP, GOP)
        except Exception as e:  # noqa: BLE001
            result["api_legs"]["processes"] = {"error": repr(e)}

    # ---- does the host side fit the cores an 8-GPU node leaves per rank?  The headline again, pinned to 2 cores ----
    if extras and not args.no_host_share and not args.only_batch_curve and not args.only_api_legs and args.host_cores <= 0:
        result["host_share"] = host_share(args, 2, fps)

    if extras and not args.no_multi_rank and not args.only_batch_curve and not args.only_api_legs and args.host_cores <= 0:
        result["multi_rank_one_gpu"] = multi_rank_one_gpu(args, fps)

    # ---- parity, part 2 + CPU baselines: the real reference (oracle/_ref) on the host cores ----
    rc = 0
    if args.full and not args.no_cpu_baseline and os.path.exists(A.REF_SO):
        try:
            rc = reference_phase(result, checks, dec_md5, sel)
        except (OSError, AssertionError, ValueError) as e:  # the reference side failed: say so beside the headline
            result["parity_checked"]["vs_reference_error"] = repr(e)
            rc = 5
    if isinstance(result.get("decode_device_parse"), dict) and result["decode_device_parse"].get("pictures_equal_to_the_host_parsed_leg") is False:
        sys.stderr.write("[bench] pictures decoded with the device parser DIFFER from the host-parsed ones\n")
        rc = rc or 9
    print(json.dumps(result))
    if dist is not None:
        dist.destroy_process_group()
    if rc:
        sys.exit(rc)


if __name__ == "__main__":
    main()
