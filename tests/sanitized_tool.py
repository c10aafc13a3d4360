"""Builds a stand-alone check program (its own main, under tools/ or tests/) for the host with AddressSanitizer and
UndefinedBehaviorSanitizer and runs it as a child process.  Nothing sanitized is built for the GPU or loaded into Python."""
import os
import subprocess

import dsvabi as A

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(A.ROOT, "digital-subband-video-2_amd", "csrc")


def run(exe, args=(), timeout=600, abort_on_error=0):
    """runs a sanitized program; asserts that it ends clean (the tails of what it wrote are shown otherwise) and returns its stdout"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=%d" % abort_on_error, UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    return r.stdout


def build_and_run(source, workdir, args=(), timeout=600):
    """source: the program's path below the repository's root; workdir: a fresh directory for the executable and for `dump`, the
    directory that stands for "{dump}" in args.  Returns (stdout, dump directory)."""
    exe, dump = os.path.join(str(workdir), os.path.splitext(os.path.basename(source))[0]), os.path.join(str(workdir), "dump")
    os.mkdir(dump)
    # (host code only, and the sanitizers named for the host side alone)
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(A.ROOT, source), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return run(exe, [a.format(dump=dump) for a in args], timeout), dump
