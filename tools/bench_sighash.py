#!/usr/bin/env python3
"""Transaction signature hashes on the GPU, measured against the same routine on
the host.

Two workloads of synthesized transactions (tests/sighash_cases.py make_tx):
  * p2pkh_sapling: 65,536 input checks (25-byte script code, SIGHASH_ALL) over Sapling-format transactions
    with 2 inputs and 2 outputs -- three per-transaction BLAKE2b digests and one final BLAKE2b per item;
  * sprout_600: every input of 64 Sprout-format transactions with 600 inputs (38,400 items) -- the
    quadratic case, a double SHA-256 over about 25 KB per item.
Per workload: a warm-up, then the median of `reps` calls of zg_sighash through the ABI (parsing, ordering,
allocation, uploads and the download included) and the device time of its two kernels
(zg_last_sig_kernel_ms); beside it the host build of the same hashing routine
(tests/native/zg_hosttest_sighash.hip, -O2) on `threads` host threads, whole call. The two results are compared
byte for byte. Prints one JSON line.

    python tools/bench_sighash.py [--reps K] [--threads T] [--out FILE]
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

from tools.bench_ed25519 import timed  # noqa: E402


def workloads(scale=1):
    from tests import sighash_cases as C
    code = b"\x76\xa9\x14" + bytes(range(20)) + b"\x88\xac"
    distinct = [C.make_tx("sapling", 2, 2, seed=s, max_script=107) for s in range(1024)]
    ntx = 32768 // scale
    p2pkh = ([distinct[t % 1024] for t in range(ntx)], [C.SAPLING_BRANCH] * ntx,
             [(t, i, code, 100000 + t, 1) for t in range(ntx) for i in range(2)])
    big = [C.make_tx("v1", 600, 2, seed=s, max_script=107) for s in range(64 // scale)]
    sprout = (big, [0] * len(big), [(t, i, code, 0, 1) for t in range(len(big)) for i in range(600)])
    return {"p2pkh_sapling": p2pkh, "sprout_600": sprout}


def run(ctx, reps=11, threads=16, scale=1):
    from tests import sighash_hostlib as H
    from zebra_amd import zg
    L, HL = zg.lib(), H.lib()
    rows = {}
    for name, (txs, br, items) in workloads(scale).items():
        ntx, n = len(txs), len(items)
        arena, tx_off, branch, item_tx, index, scripts, script_off, amount, hashtype = zg.pack_sighash(txs, br, items)
        arena, scripts = arena + b"\0", scripts + b"\0"
        ts, hs, st = (ctypes.create_string_buffer(k) for k in (ntx, 32 * n, n))
        ts2, hs2, st2 = (ctypes.create_string_buffer(k) for k in (ntx, 32 * n, n))

        def gpu():
            ctx._chk(L.zg_sighash(ctx._p, ntx, arena, tx_off, branch, n, item_tx, index, scripts, script_off, amount,
                                  hashtype, ts, hs, st))
        wall, kern = timed(ctx, gpu, reps)
        assert st.raw == bytes(n) and ts.raw == bytes(ntx), "an item was not hashed"
        host = []
        for _ in range(max(3, reps // 3)):
            t = time.perf_counter()
            HL.zgh_sighash(ntx, arena, tx_off, branch, n, item_tx, index, scripts, script_off, amount, hashtype, ts2,
                           hs2, st2, threads)
            host.append((time.perf_counter() - t) * 1e3)
        assert hs.raw == hs2.raw, "the device and the host build disagree"
        hm = statistics.median(host)
        rows[name] = {"transactions": ntx, "items": n, "arena_bytes": len(arena) - 1, "reps": reps,
                      "gpu_abi_ms": wall, "gpu_kernel_ms": kern, "host_threads": threads, "host_ms": hm,
                      "gpu_abi_items_per_s": n / (wall * 1e-3), "gpu_kernel_items_per_s": n / (kern * 1e-3),
                      "host_items_per_s": n / (hm * 1e-3), "host_over_gpu_abi_time": hm / wall,
                      "host_over_gpu_kernel_time": hm / kern}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--scale", type=int, default=1, help="divide both workloads by this (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of >= 10 calls)")
    from zebra_amd import Context
    ctx = Context(device=0, max_batch=64, load_builtin=False)
    out = {"bench": "sighash_gpu_vs_host", "rows": run(ctx, a.reps, a.threads, a.scale)}
    ctx.close()
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
