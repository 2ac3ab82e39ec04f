#!/usr/bin/env python3
"""The shielded stage of a window from the transactions' bytes in one call, measured against
the six calls it replaces.

The workload: the six whole v4 transactions of tests/golden/sighash.json (two with one spend and one output, one with a
transparent input and one output, three with one Groth JoinSplit each) repeated to a window of 16,384 transactions, all
valid: 21,846 descriptions, 5,462 spend_auth and 16,384 binding signatures, 8,191 Ed25519 signatures. ms per call,
transfers included:
  (a) zg_shielded_verify through the ABI on the packed arena: one upload, everything on the device, one download;
  (b) collector.verify_block with the transactions marked shielded: (a) with its packing and the Python around it;
  (c) the parent's path: collector.verify_block over records whose fields were sliced out of the transactions on the
      host beforehand (that slicing is not timed): zg_sighash, zg_prep_batch, zg_verify_batch, zg_sapling_bvk,
      zg_redjubjub_verify, zg_ed25519_verify, joined in Python as the collector does.
The three alternate `rounds` times in one process, so drift shows in all of them; each figure is the median of `reps`
calls after a warm-up. Kernel time: for (a) zg_last_sig_kernel_ms (the call's kernels outside the Groth16 pipeline) and
the pipeline's own device time of its last batch. Prints one JSON line.

    python tools/bench_shielded.py [--reps K] [--rounds R] [--scale S] [--out FILE]
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


def timed(call, reps):
    call()
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
    return statistics.median(wall)


def run(ctx, reps=5, rounds=5, scale=1):
    from tests import shielded_cases as C
    from zebra_amd import collector, zg
    L = zg.lib()
    r = C.real()
    ntx = 16384 // scale
    txs = [r[C.SIX[t % 6]] for t in range(ntx)]
    br = [C.SAPLING_BRANCH] * ntx
    arena, tx_off, branch = zg.pack_shielded(txs, br)
    arena = arena + b"\0"
    ts, st, dt = (ctypes.create_string_buffer(ntx) for _ in range(3))
    ix = (ctypes.c_uint64 * ntx)()
    marked = [collector.Tx(raw=raw, branch_id=b, shielded=True) for raw, b in zip(txs, br)]
    six = {k: C.collector_tx(r[k]) for k in C.SIX}
    records = [six[C.SIX[t % 6]] for t in range(ntx)]
    kern, pipe = [], []

    def new_abi():
        ctx._chk(L.zg_shielded_verify(ctx._p, ntx, arena, tx_off, branch, ts, st, ix, dt, None, None, None))
        kern.append(ctx.last_sig_kernel_ms())
        pipe.append(ctx.last_timings()[6])

    def new_collector():
        assert collector.verify_block(marked, ctx=ctx) is None

    def old():
        assert collector.verify_block(records, ctx=ctx) is None
    a, b, c = [], [], []
    for _ in range(rounds):
        a.append(timed(new_abi, reps))
        b.append(timed(new_collector, reps))
        c.append(timed(old, reps))
    assert ts.raw == bytes(ntx) and st.raw == bytes(ntx), "a transaction of the workload did not verify"
    nd = sum(len(t.joinsplits) + len(t.spends) + len(t.outputs) for t in records)
    ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
    return {"transactions": ntx, "descriptions": nd, "arena_bytes": len(arena) - 1, "max_batch": ctx.max_batch,
            "reps": reps, "rounds": rounds, "shielded_verify_abi_ms": a, "shielded_verify_collector_ms": b,
            "six_calls_collector_ms": c, "shielded_verify_abi_median_ms": ma, "shielded_verify_collector_median_ms": mb,
            "six_calls_collector_median_ms": mc, "shielded_verify_abi_spread_ms": max(a) - min(a),
            "shielded_verify_collector_spread_ms": max(b) - min(b), "six_calls_collector_spread_ms": max(c) - min(c),
            "kernel_ms_outside_groth16_median": statistics.median(kern),
            "kernel_ms_outside_groth16_spread": max(kern) - min(kern),
            "groth16_last_batch_device_ms_median": statistics.median(pipe),
            "new_over_old_time": mb / mc, "transactions_per_s": ntx / (ma * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the workload by this (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from zebra_amd import Context
    ctx = Context(device=0, max_batch=32768)
    out = {"bench": "shielded_verify_vs_six_calls", "rows": run(ctx, a.reps, a.rounds, a.scale)}
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
