#!/usr/bin/env python3
"""PHGR JoinSplit transactions of a window from their bytes in one call, measured against the
four calls it replaces.

The workload: block 522's five JoinSplit transactions (tests/golden/phgr_txs.json, one with two descriptions) repeated
to a window of 8,192 transactions, all valid: 9,830 PHGR descriptions, 8,192 Ed25519 signatures. ms per call,
transfers included:
  (a)  zg_shielded_verify_flags with ZG_SHIELDED_PHGR through the ABI on the packed arena;
  (a2) Context.shielded_verify(phgr=True): (a) with its packing in Python;
  (b)  the parent's route through the same Python binding: zg_sighash, zg_prep_batch with ZG_PREP_KIND_JOINSPLIT_BN,
       zg_pghr13_verify and zg_ed25519_verify over records whose fields were sliced out of the transactions on the host
       beforehand (that slicing is not timed; the packing each binding method does is, as in (a2)).
They alternate `rounds` times in one process, so drift shows in all of them; each figure is the median of `reps` calls
after a warm-up. Prints one JSON line.

    python tools/bench_shielded_phgr.py [--reps K] [--rounds R] [--scale S] [--out FILE]
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


def run(ctx, reps=3, rounds=5, scale=1):
    from tests import shielded_phgr_cases as C
    from zebra_amd import zg
    L = zg.lib()
    r = C.real()
    ntx = 8192 // scale
    txs = [r[t % 5] for t in range(ntx)]
    br = [0] * ntx
    arena, tx_off, branch = zg.pack_shielded(txs, br)
    arena = arena + b"\0"
    ts, st, dt = (ctypes.create_string_buffer(ntx) for _ in range(3))
    ix = (ctypes.c_uint64 * ntx)()
    # the parent's records: fields, proofs, keys and signatures sliced out beforehand
    five = []
    for raw in r:
        p = C.parsed(raw)
        rows = [zg.prep_fields(zg.PREP_KIND_JOINSPLIT_BN, d[16:48], d[208:240], [d[48:80], d[80:112]],
                               [d[240:272], d[272:304]], [d[112:144], d[144:176]], int.from_bytes(d[0:8], "little"),
                               int.from_bytes(d[8:16], "little"), p["js_pubkey"]) for d in p["joinsplits"]]
        five.append((rows, [d[304:600] for d in p["joinsplits"]], p["js_pubkey"], p["js_sig"]))
    fields = b"".join(f for t in range(ntx) for f in five[t % 5][0])
    proofs = b"".join(q for t in range(ntx) for q in five[t % 5][1])
    nd = len(proofs) // 296
    kinds, nin = bytes([zg.PREP_KIND_JOINSPLIT_BN]) * nd, bytes([9]) * nd
    pks, sigs = [five[t % 5][2] for t in range(ntx)], [five[t % 5][3] for t in range(ntx)]
    items = [(t, None, b"", 0, 1) for t in range(ntx)]
    kern = []

    def new_abi():
        ctx._chk(L.zg_shielded_verify_flags(ctx._p, ntx, arena, tx_off, branch, zg.SHIELDED_PHGR, ts, st, ix, dt, None,
                                            None, None))
        kern.append(ctx.last_sig_kernel_ms())

    def new_binding():
        got = ctx.shielded_verify(txs, br, want_hashes=False, want_desc=False, phgr=True)
        assert not any(got[1])

    def old():
        _, hashes, hst = ctx.sighash(txs, br, items)
        rows, codes = ctx.prep_batch(kinds, fields)
        pst = ctx.pghr13_verify(proofs, rows, nin)
        ed = ctx.ed25519_verify(pks, sigs, hashes)
        assert not (any(hst) or any(codes) or any(pst) or any(ed))
    a, a2, b = [], [], []
    for _ in range(rounds):
        a.append(timed(new_abi, reps))
        a2.append(timed(new_binding, reps))
        b.append(timed(old, reps))
    assert ts.raw == bytes(ntx) and st.raw == bytes(ntx), "a transaction of the workload did not verify"
    ma, ma2, mb = statistics.median(a), statistics.median(a2), statistics.median(b)
    return {"transactions": ntx, "descriptions": nd, "arena_bytes": len(arena) - 1, "reps": reps, "rounds": rounds,
            "shielded_phgr_abi_ms": a, "shielded_phgr_binding_ms": a2, "four_calls_binding_ms": b,
            "shielded_phgr_abi_median_ms": ma, "shielded_phgr_binding_median_ms": ma2, "four_calls_binding_median_ms": mb,
            "shielded_phgr_abi_spread_ms": max(a) - min(a), "shielded_phgr_binding_spread_ms": max(a2) - min(a2),
            "four_calls_binding_spread_ms": max(b) - min(b),
            "kernel_ms_outside_the_proof_pipelines_median": statistics.median(kern),
            "new_over_old_time": ma2 / mb, "transactions_per_s": ntx / (ma * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the workload by this (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from zebra_amd import Context
    ctx = Context(device=0, max_batch=32768)
    out = {"bench": "shielded_verify_phgr_vs_four_calls", "rows": run(ctx, a.reps, a.rounds, a.scale)}
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
