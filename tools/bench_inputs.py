#!/usr/bin/env python3
"""Pay-to-pubkey-hash inputs verified in one call, measured against the two calls it
replaces and against the same routines on the host.

Two workloads of synthesized transactions (tests/sighash_cases.py make_tx, signed by tests/script_cases.py):
  * p2pkh_sapling: 65,536 P2PKH inputs (SIGHASH_ALL) over Sapling-format transactions with 2 inputs and 2
    outputs; 256 distinct signed transactions, repeated;
  * sprout_600: every input of 64 Sprout-format transactions with 600 inputs (38,400 items) -- the quadratic
    case. Signing 38,400 inputs in Python is out of reach: input 0 and 1 of 4 distinct transactions carry their
    own signatures, every other input a well-formed signature of another input (EVAL_FALSE after the full check:
    the hash and the double multiplication cost the same as for a signature that verifies).
Per workload, ms per call through the ABI, transfers included, each the median of `reps` calls after a warm-up:
  (a) zg_inputs_verify: one upload, HASH160 + encoding check + signature hash + ECDSA on the device, one download;
  (b) the path it replaces: zg_sighash, its hashes back to the host, then zg_ecdsa_verify with them sent up again,
      from records gathered beforehand (the gather itself -- today a host interpreter run per input -- is not
      timed, and this path does no HASH160 and no encoding check at all);
  (c) the host build of the per-input routine (tests/native/zg_hosttest_script.hip, -O2) on `threads` threads.
(a) and (b) alternate `rounds` times in one process, so drift shows in both. The verdicts of the three are compared.
Prints one JSON line.

    python tools/bench_inputs.py [--reps K] [--rounds R] [--threads T] [--out FILE]
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
    """name -> (txs, branch ids, items for inputs_verify, the gathered records of path (b): (key, DER signature,
    hashtype) per item)"""
    from tests import script_cases as C
    from tests import script_ref as R
    from tests.sighash_cases import SAPLING_BRANCH, make_tx
    keys = C.secrets()
    out = {}

    def signed(raw, branch, n_sign, amount):
        """-> the transaction with its inputs spent as P2PKH, the per-input (script_pubkey, key, DER, hashtype)"""
        n_in = R.S.parse(raw)[1]["inputs"].__len__()
        pushes, rec = [], []
        for i in range(n_in):
            d, key, _ = keys[i % len(keys)]
            spk = C.p2pkh(key)
            if i < n_sign:
                sig = C.signed_push(raw, branch, i, spk, amount, d, 1)
            else:
                sig = pushes[i % n_sign][0]
            pushes.append((sig, key, spk))
        for i, (sig, key, spk) in enumerate(pushes):
            raw = C.set_script_sig(raw, i, R.push(sig) + R.push(key))
            rec.append((spk, key, sig[:-1], sig[-1]))
        return raw, rec

    distinct = [signed(make_tx("sapling", 2, 2, seed=s, max_script=0), SAPLING_BRANCH, 2, 100000) for s in range(256 // scale)]
    ntx = 32768 // scale
    txs = [distinct[t % len(distinct)][0] for t in range(ntx)]
    recs = [distinct[t % len(distinct)][1][i] for t in range(ntx) for i in range(2)]
    out["p2pkh_sapling"] = (txs, [SAPLING_BRANCH] * ntx, [(t, i, recs[2 * t + i][0], 100000) for t in range(ntx) for i in range(2)],
                            [r[1:] for r in recs])
    n_big = 600 // scale
    big = [signed(make_tx("v1", n_big, 2, seed=s, max_script=0), 0, 2, 0) for s in range(4)]
    nb = 64 // scale
    txs = [big[t % 4][0] for t in range(nb)]
    recs = [big[t % 4][1][i] for t in range(nb) for i in range(n_big)]
    out["sprout_600"] = (txs, [0] * nb, [(t, i, recs[n_big * t + i][0], 0) for t in range(nb) for i in range(n_big)],
                         [r[1:] for r in recs])
    return out


def run(ctx, reps=11, rounds=5, threads=16, scale=1):
    from tests import script_hostlib as H
    from zebra_amd import zg
    L, HL = zg.lib(), H.lib()
    rows = {}
    for name, (txs, br, items, recs) in workloads(scale).items():
        ntx, n = len(txs), len(items)
        arena, tx_off, branch, item_tx, index, prev, prev_off, amount = zg.pack_inputs_verify(txs, br, items)
        arena, prev = arena + b"\0", prev + b"\0"
        ts, st, dt = (ctypes.create_string_buffer(k) for k in (ntx, n, n))
        hs = ctypes.create_string_buffer(32 * n)
        # path (b): the records a host run gathers, packed beforehand
        hashtype = (ctypes.c_uint32 * n)(*[r[2] for r in recs])
        pk, pklen, sigs, sig_off, _ = zg.pack_ecdsa([r[0] for r in recs], [r[1] for r in recs], [bytes(32)] * n)
        sigs = sigs + b"\0"
        ts2, st2, ec = (ctypes.create_string_buffer(k) for k in (ntx, n, n))
        hs2 = ctypes.create_string_buffer(32 * n)

        def new():
            ctx._chk(L.zg_inputs_verify(ctx._p, ntx, arena, tx_off, branch, n, item_tx, index, prev, prev_off, amount,
                                        zg.SCRIPT_VERIFY_DERSIG, ts, st, dt, hs))

        def old():
            ctx._chk(L.zg_sighash(ctx._p, ntx, arena, tx_off, branch, n, item_tx, index, prev, prev_off, amount, hashtype,
                                  ts2, hs2, st2))
            ctx._chk(L.zg_ecdsa_verify(ctx._p, n, pk, pklen, sigs, sig_off, hs2, ec))
        a, ak, b = [], [], []
        for _ in range(rounds):
            w, k = timed(ctx, new, reps)
            a.append(w), ak.append(k)
            b.append(timed(ctx, old, reps)[0])
        assert ts.raw == bytes(ntx) and st2.raw == bytes(n), "a transaction or an item was not hashed"
        assert hs.raw == hs2.raw, "the two device paths hashed differently"
        assert [zg.INPUT_EVAL_FALSE if e else zg.INPUT_OK for e in ec.raw] == list(st.raw), "the two device paths disagree"
        ts3, st3, dt3 = (ctypes.create_string_buffer(k) for k in (ntx, n, n))
        hs3 = ctypes.create_string_buffer(32 * n)
        host = []
        for _ in range(2):
            t = time.perf_counter()
            HL.zgh_inputs_verify(ntx, arena, tx_off, branch, n, item_tx, index, prev, prev_off, amount,
                                 zg.SCRIPT_VERIFY_DERSIG, ts3, st3, dt3, hs3, threads)
            host.append((time.perf_counter() - t) * 1e3)
        assert (st3.raw, dt3.raw, hs3.raw) == (st.raw, dt.raw, hs.raw), "the device and the host build disagree"
        ma, mb, mh = statistics.median(a), statistics.median(b), min(host)
        rows[name] = {"transactions": ntx, "items": n, "ok_items": st.raw.count(b"\0"), "arena_bytes": len(arena) - 1,
                      "reps": reps, "rounds": rounds, "inputs_verify_ms": a, "inputs_verify_kernel_ms": ak,
                      "sighash_then_ecdsa_ms": b, "inputs_verify_median_ms": ma, "sighash_then_ecdsa_median_ms": mb,
                      "sighash_then_ecdsa_spread_ms": max(b) - min(b), "new_over_old_time": ma / mb,
                      "host_threads": threads, "host_ms": mh, "host_over_inputs_verify_time": mh / ma,
                      "inputs_per_s": n / (ma * 1e-3)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--scale", type=int, default=1, help="divide both workloads by this (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of >= 10 calls)")
    from zebra_amd import Context
    ctx = Context(device=0, max_batch=64, load_builtin=False)
    out = {"bench": "inputs_verify_vs_sighash_then_ecdsa", "rows": run(ctx, a.reps, a.rounds, a.threads, a.scale)}
    ctx.close()
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
