#!/usr/bin/env python3
"""Ed25519 JoinSplit signatures on the GPU, measured against RedJubjub.

Workload: n valid signatures cycling through the fixtures (tests/golden/ed25519.json: the three
real JoinSplit signatures of block 419221 and 48 seeded ones), packed host buffers through
zg_ed25519_verify; beside it, in the same process, n valid RedJubjub signatures
(tests/golden/sapling_sigs.json) through zg_redjubjub_verify -- the yardstick: the same curve work
(a fixed-base comb, a 252/253-bit double-and-add, one inversion) on a costlier field. Per n in
64, 4,096, 65,536: a warm-up, then the median of `reps` calls, both through the ABI (uploads,
allocation and the status download included) and kernel-only (HIP events around the kernel,
zg_last_sig_kernel_ms). Prints one JSON line.

    python tools/bench_ed25519.py [--reps K] [--n N ...]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ed_workload(n):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519.json")))
    v = [(e["pubkey"], e["sig"], e["sighash"]) for e in g["real"]] + [(e["pubkey"], e["sig"], e["msg"]) for e in g["signed"]]
    v = [tuple(bytes.fromhex(x) for x in t) for t in v]
    return [b"".join(v[i % len(v)][k] for i in range(n)) for k in range(3)]


def rj_workload(n):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "sapling_sigs.json")))
    v = [e for e in g["sigs"] + g["signed_batch"] if e["ok"]]
    v = [(bytes.fromhex(e["vk"]), bytes.fromhex(e["sig"]), bytes.fromhex(e["msg"]), bytes([e["gen"]])) for e in v]
    return [b"".join(v[i % len(v)][k] for i in range(n)) for k in range(4)]


def timed(ctx, call, reps):
    """-> (median wall ms, median kernel ms) of `reps` calls after one warm-up call"""
    call()
    wall, kern = [], []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
        kern.append(ctx.last_sig_kernel_ms())
    return statistics.median(wall), statistics.median(kern)


def run(ctx, sizes=(64, 4096, 65536), reps=11):
    from zebra_amd import zg
    L = zg.lib()
    rows = []
    for n in sizes:
        pk, sg, m = ed_workload(n)
        st = ctypes.create_string_buffer(n)

        def ed():
            ctx._chk(L.zg_ed25519_verify(ctx._p, n, pk, sg, m, st))
        ew, ek = timed(ctx, ed, reps)
        assert st.raw == bytes(n), "an Ed25519 fixture signature did not verify"
        vk, rsg, rm, gen = rj_workload(n)
        ok = ctypes.create_string_buffer(n)

        def rj():
            ctx._chk(L.zg_redjubjub_verify(ctx._p, n, vk, rsg, rm, gen, ok))
        rw, rk = timed(ctx, rj, reps)
        assert ok.raw == b"\x01" * n, "a RedJubjub fixture signature did not verify"
        rows.append({"n": n, "reps": reps,
                     "ed25519": {"abi_ms": ew, "kernel_ms": ek, "abi_sigs_per_s": n / (ew * 1e-3),
                                 "kernel_sigs_per_s": n / (ek * 1e-3)},
                     "redjubjub": {"abi_ms": rw, "kernel_ms": rk, "abi_sigs_per_s": n / (rw * 1e-3),
                                   "kernel_sigs_per_s": n / (rk * 1e-3)},
                     "ed25519_over_redjubjub_kernel_time": ek / rk})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--n", type=int, nargs="*", default=[64, 4096, 65536])
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of >= 10 calls)")
    from zebra_amd import Context
    ctx = Context(device=0, max_batch=64, load_builtin=False)
    out = {"bench": "ed25519_vs_redjubjub", "rows": run(ctx, a.n, a.reps)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
