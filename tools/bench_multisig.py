#!/usr/bin/env python3
"""P2SH 2-of-3 multisig inputs verified in one call, measured against what the parent offers
for them and against the same routines on the host.

The workload: 65,536 P2SH 2-of-3 inputs (SIGHASH_ALL, compressed keys, every signer subset in turn) over Sapling-format
transactions with 2 inputs and 2 outputs; 256 distinct signed transactions, repeated. 131,072 signature pushes,
262,144 candidate pairs (signature s can meet keys s and s + 1 in pop order). ms per call through the ABI, transfers
included, each the median of `reps` calls after a warm-up:
  (a) zg_inputs_verify with ZG_SCRIPT_TEMPLATE_MULTISIG: one upload, HASH160 of the redeem scripts, the encoding
      checks, one signature hash per push, the pair rows, ECDSA and the walk on the device, one download;
  (b) what the parent offers: zg_sighash with one item per signature push (the redeem script as script code), its
      hashes back to the host and gathered per pair there, then zg_ecdsa_verify over the same candidate pairs, their
      keys and signatures gathered beforehand (that gather -- today a host interpreter run per input -- is not timed,
      and this path does no HASH160, no encoding check and no walk);
  (c) the host build of the same routines (tests/native/zg_hosttest_multisig.hip, -O2) on `threads` threads.
(a) and (b) alternate `rounds` times in one process, so drift shows in both. The verdicts of the three are compared:
(b)'s by replaying the walk over its statuses here. Prints one JSON line.

    python tools/bench_multisig.py [--reps K] [--rounds R] [--threads T] [--out FILE]
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

SUBSETS = ((0, 1), (0, 2), (1, 2))


def workload(scale=1):
    """-> (txs, branch ids, items for inputs_verify, per item: (redeem script, keys in push order, signature pushes
    in push order))"""
    from tests import multisig_cases as C
    from tests import script_ref as R
    from tests.script_cases import set_script_sig, signed_push
    from tests.sighash_cases import SAPLING_BRANCH, make_tx
    K = C.keys(6)
    amount = 100000
    distinct = []
    for s in range(256 // scale):
        raw = make_tx("sapling", 2, 2, seed=s, max_script=0)
        rec = []
        for i in range(2):
            ks = [K[(s + i + j) % 6] for j in range(3)]
            code = C.ms_script(2, [k[1] for k in ks])
            sigs = [signed_push(raw, SAPLING_BRANCH, i, code, amount, ks[j][0], 1) for j in SUBSETS[(s + i) % 3]]
            rec.append((code, [k[1] for k in ks], sigs))
        for i, (code, _, sigs) in enumerate(rec):
            raw = set_script_sig(raw, i, b"\x00" + b"".join(R.push(x) for x in sigs) + R.push(code))
        distinct.append((raw, rec))
    ntx = 32768 // scale
    txs = [distinct[t % len(distinct)][0] for t in range(ntx)]
    recs = [distinct[t % len(distinct)][1][i] for t in range(ntx) for i in range(2)]
    items = [(t, i, C.p2sh(recs[2 * t + i][0]), amount) for t in range(ntx) for i in range(2)]
    return txs, [SAPLING_BRANCH] * ntx, items, recs


def walk(ec, m, n):
    """OP_CHECKMULTISIG's walk over the statuses of an item's m (n - m + 1) pair rows -> passed"""
    s = k = 0
    ok = True
    while s < m and ok:
        if ec[s * (n - m + 1) + k - s] == 0:
            s += 1
        k += 1
        ok = m - s <= n - k
    return ok


def run(ctx, reps=11, rounds=5, threads=16, scale=1):
    import numpy as np
    from tests import multisig_hostlib as H
    from zebra_amd import zg
    L, HL = zg.lib(), H.lib()
    txs, br, items, recs = workload(scale)
    flags = zg.SCRIPT_VERIFY_DERSIG | zg.SCRIPT_TEMPLATE_MULTISIG
    ntx, n = len(txs), len(items)
    arena, tx_off, branch, item_tx, index, prev, prev_off, amount = zg.pack_inputs_verify(txs, br, items)
    arena, prev = arena + b"\0", prev + b"\0"
    ts, st, dt = (ctypes.create_string_buffer(k) for k in (ntx, n, n))
    hs = ctypes.create_string_buffer(32 * n)
    # path (b): one signature-hash item per push, in pop order (the last pushed first); one ECDSA row per pair
    sh_items, pair_key, pair_sig, row_sig = [], [], [], []
    for (t, i, _, amt), (code, keys, sigs) in zip(items, recs):
        for s, sig in enumerate(sigs[::-1]):
            for j in range(2):
                pair_key.append(keys[::-1][s + j]), pair_sig.append(sig[:-1]), row_sig.append(len(sh_items))
            sh_items.append((t, i, code, amt, sig[-1]))
    ns, nr = len(sh_items), len(row_sig)
    _, _, _, s_tx, s_index, s_scripts, s_off, s_amount, s_type = zg.pack_sighash(txs, br, sh_items)
    s_scripts = s_scripts + b"\0"
    pk, pklen, sigs, sig_off, _ = zg.pack_ecdsa(pair_key, pair_sig, [bytes(32)] * nr)
    sigs = sigs + b"\0"
    ts2, st2, ec = (ctypes.create_string_buffer(k) for k in (ntx, ns, nr))
    hs2 = ctypes.create_string_buffer(32 * ns)
    gather = np.asarray(row_sig, dtype=np.int64)

    def new():
        ctx._chk(L.zg_inputs_verify(ctx._p, ntx, arena, tx_off, branch, n, item_tx, index, prev, prev_off, amount, flags,
                                    ts, st, dt, hs))

    def old():
        ctx._chk(L.zg_sighash(ctx._p, ntx, arena, tx_off, branch, ns, s_tx, s_index, s_scripts, s_off, s_amount, s_type,
                              ts2, hs2, st2))
        msg = np.frombuffer(hs2, dtype=np.uint8).reshape(ns, 32)[gather].tobytes()
        ctx._chk(L.zg_ecdsa_verify(ctx._p, nr, pk, pklen, sigs, sig_off, msg, ec))
    a, ak, b = [], [], []
    for _ in range(rounds):
        w, k = timed(ctx, new, reps)
        a.append(w), ak.append(k)
        b.append(timed(ctx, old, reps)[0])
    assert ts.raw == bytes(ntx) and st2.raw == bytes(ns), "a transaction or an item was not hashed"
    assert st.raw == bytes(n), "an input of the workload did not verify"
    assert all(walk(ec.raw[4 * i:4 * i + 4], 2, 3) for i in range(n)), "the two device paths disagree"
    ts3, st3, dt3 = (ctypes.create_string_buffer(k) for k in (ntx, n, n))
    hs3 = ctypes.create_string_buffer(32 * n)
    host = []
    for _ in range(2):
        t = time.perf_counter()
        HL.zgh_inputs_verify(ntx, arena, tx_off, branch, n, item_tx, index, prev, prev_off, amount, flags, ts3, st3, dt3,
                             hs3, threads)
        host.append((time.perf_counter() - t) * 1e3)
    assert (st3.raw, dt3.raw, hs3.raw) == (st.raw, dt.raw, hs.raw), "the device and the host build disagree"
    ma, mb, mh = statistics.median(a), statistics.median(b), min(host)
    return {"p2sh_2of3_sapling": {
        "transactions": ntx, "items": n, "signature_pushes": ns, "ecdsa_rows": nr, "ok_items": st.raw.count(b"\0"),
        "arena_bytes": len(arena) - 1, "reps": reps, "rounds": rounds, "inputs_verify_ms": a, "inputs_verify_kernel_ms": ak,
        "sighash_then_ecdsa_ms": b, "inputs_verify_median_ms": ma, "sighash_then_ecdsa_median_ms": mb,
        "sighash_then_ecdsa_spread_ms": max(b) - min(b), "new_over_old_time": ma / mb, "host_threads": threads,
        "host_ms": mh, "host_over_inputs_verify_time": mh / ma, "inputs_per_s": n / (ma * 1e-3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--scale", type=int, default=1, help="divide the workload by this (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of >= 10 calls)")
    from zebra_amd import Context
    ctx = Context(device=0, max_batch=64, load_builtin=False)
    out = {"bench": "multisig_inputs_verify_vs_sighash_then_ecdsa", "rows": run(ctx, a.reps, a.rounds, a.threads, a.scale)}
    ctx.close()
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
