#!/usr/bin/env python3
"""Block headers on the GPU: zg_headers_verify measured against the host path.

Workload: n headers cycling through the 13 real ones (tests/golden/equihash.json), all valid. Per n
in 1, 24, 1,024, 16,384: a warm-up, then the median of `reps` calls, whole-call (the upload of
n x 1487 bytes, allocation, both kernels, the status / hash / flags download) and kernel-only (HIP
events around the two kernels, zg_last_sig_kernel_ms; the Equihash kernel alone from zg_equihash_verify
over the same inputs). Beside it the host path the fallback runs per
header, timed on min(n, 1024) of the same headers: tools/bench_headers_cpu.cpp, a single-thread C++
restatement of verify_equihash_solution built here with g++ -O2 (Equihash only: the 25 SHA-256
compressions of the block hash are small against 513 BLAKE2b ones). Where no g++ is found only the
Python restatement (tests/equihash_ref.py) is timed, on 13 headers, and the row says so: that is no fair
baseline. Prints one JSON line.

    python tools/bench_headers.py [--reps K] [--n N ...] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "bench_out")


def workload(n):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "equihash.json")))
    v = [bytes.fromhex(e["header"]) for e in g["real"]]
    return b"".join(v[i % len(v)] for i in range(n)), g["max_bits"]


def cpu_baseline(headers, n):
    """-> dict: seconds per header of the host path, and which one was timed"""
    gxx = shutil.which("g++")
    if gxx:
        os.makedirs(OUT, exist_ok=True)
        exe = os.path.join(OUT, "bench_headers_cpu")
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "bench_headers_cpu.cpp")])
        m = min(n, 1024)
        path = os.path.join(OUT, "bench_headers_%d.bin" % m)
        open(path, "wb").write(headers[:1487 * m])
        reps = max(1, 256 // m)
        ok, dt = subprocess.check_output([exe, path, str(reps)], text=True).split()
        assert int(ok) == m, "the C++ restatement rejected a real header"
        return {"what": "C++ -O2 single thread, Equihash only", "headers_timed": m, "ms_per_header": float(dt) / m * 1e3}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import equihash_ref as Q
    m = min(n, 13)
    t = time.perf_counter()
    for i in range(m):
        hd = headers[1487 * i:1487 * (i + 1)]
        assert Q.verify(200, 9, hd[:140], hd[143:])
    return {"what": "Python restatement only: not a fair baseline", "headers_timed": m,
            "ms_per_header": (time.perf_counter() - t) / m * 1e3}


def run(ctx, sizes, reps):
    from zebra_amd import zg
    L = zg.lib()
    rows = []
    for n in sizes:
        headers, max_bits = workload(n)
        st = ctypes.create_string_buffer(n)
        hs = ctypes.create_string_buffer(32 * n)
        fl = ctypes.create_string_buffer(n)

        def call():
            ctx._chk(L.zg_headers_verify(ctx._p, n, headers, max_bits, st, hs, fl))
        call()
        wall, kern = [], []
        for _ in range(reps):
            t = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t) * 1e3)
            kern.append(ctx.last_sig_kernel_ms())
        assert st.raw == bytes(n) and fl.raw == bytes(n), "a real header did not verify"
        w, k = statistics.median(wall), statistics.median(kern)
        # the Equihash kernel alone (zg_equihash_verify over the same inputs and solutions)
        ins = b"".join(headers[1487 * i:1487 * i + 140] for i in range(n))
        sols = b"".join(headers[1487 * i + 143:1487 * (i + 1)] for i in range(n))
        ok = ctypes.create_string_buffer(n)
        eq = []
        for _ in range(reps + 1):
            ctx._chk(L.zg_equihash_verify(ctx._p, zg.EQ_200_9, n, ins, 140, sols, ok, None))
            eq.append(ctx.last_sig_kernel_ms())
        assert ok.raw == b"\x01" * n
        cpu = cpu_baseline(headers, n)
        rows.append({"n": n, "reps": reps, "call_ms": w, "kernel_ms": k, "call_headers_per_s": n / (w * 1e-3),
                     "kernel_headers_per_s": n / (k * 1e-3),
                     "equihash_kernel_ms": statistics.median(eq[1:]), "call_min_ms": min(wall), "kernel_min_ms": min(kern),
                     "cpu": cpu, "cpu_ms_for_n": cpu["ms_per_header"] * n,
                     "cpu_time_over_call_time": cpu["ms_per_header"] * n / w})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--n", type=int, nargs="*", default=[1, 24, 1024, 16384])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of >= 10 calls)")
    from zebra_amd import Context
    ctx = Context(device=0, max_batch=64, load_builtin=False)
    out = {"bench": "headers_verify", "rows": run(ctx, a.n, a.reps)}
    ctx.close()
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
