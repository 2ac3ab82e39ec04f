#!/usr/bin/env python3
"""secp256k1 ECDSA input signatures on the GPU, measured against Ed25519.

Workload: n valid signatures cycling through the fixtures (tests/golden/ecdsa.json: the reference's
key-pair and transaction vectors that verify, and 64 seeded ones, compressed and uncompressed keys),
packed host buffers through zg_ecdsa_verify; beside it, in the same process, n valid Ed25519
signatures (tests/golden/ed25519.json) through zg_ed25519_verify -- the yardstick: the project's
other one-lane-per-signature kernel on a 9 x 29-bit field (a fixed-base comb, a ~256-step
double-and-add). Per n in 64, 4,096, 65,536: a warm-up, then the median of `reps` calls, both
through the ABI (uploads, allocation and the status download included) and kernel-only (HIP events
around the kernel, zg_last_sig_kernel_ms). Prints one JSON line.

    python tools/bench_ecdsa.py [--reps K] [--n N ...]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_ed25519 import ed_workload, timed  # noqa: E402


def ecdsa_workload(n):
    from zebra_amd import zg
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ecdsa.json")))
    v = [(e["pubkey"], e["sig"], e["sighash"]) for e in g["real"] if e["status"] == 0]
    v += [(e["pubkey"], e["sig"], e["msg"]) for e in g["signed"]]
    v = [tuple(bytes.fromhex(x) for x in t) for t in v]
    return zg.pack_ecdsa(*[[v[i % len(v)][k] for i in range(n)] for k in range(3)])


def run(ctx, sizes=(64, 4096, 65536), reps=11):
    from zebra_amd import zg
    L = zg.lib()
    rows = []
    for n in sizes:
        keys, lens, sigs, off, msg = ecdsa_workload(n)
        st = ctypes.create_string_buffer(n)

        def ec():
            ctx._chk(L.zg_ecdsa_verify(ctx._p, n, keys, lens, sigs, off, msg, st))
        cw, ck = timed(ctx, ec, reps)
        assert st.raw == bytes(n), "an ECDSA fixture signature did not verify"
        pk, sg, m = ed_workload(n)
        est = ctypes.create_string_buffer(n)

        def ed():
            ctx._chk(L.zg_ed25519_verify(ctx._p, n, pk, sg, m, est))
        ew, ek = timed(ctx, ed, reps)
        assert est.raw == bytes(n), "an Ed25519 fixture signature did not verify"
        rows.append({"n": n, "reps": reps,
                     "ecdsa": {"abi_ms": cw, "kernel_ms": ck, "abi_sigs_per_s": n / (cw * 1e-3),
                               "kernel_sigs_per_s": n / (ck * 1e-3)},
                     "ed25519": {"abi_ms": ew, "kernel_ms": ek, "abi_sigs_per_s": n / (ew * 1e-3),
                                 "kernel_sigs_per_s": n / (ek * 1e-3)},
                     "ecdsa_over_ed25519_kernel_time": ck / ek})
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
    out = {"bench": "ecdsa_vs_ed25519", "rows": run(ctx, a.n, a.reps)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
