#!/usr/bin/env python3
"""Block bodies on the GPU, measured against the same routines on the host.

Three windows of synthesized blocks (a fixture header, the root computed by tests/blocks_ref.py):
  * small_transparent: 4,096 blocks of 8 transparent transactions of about 190 bytes;
  * shielded_2k: 64 blocks of 1,024 Sapling-format transactions of about 1.8 KB, 65,536 in all;
  * shielded_2k_long: the same with one 100 KB transaction added, run with ZG_TXID_HOST_MIN = 0 and at a few
    thresholds, the contexts alternating call by call in one run. A threshold wins only if every call with it is
    faster than every call without it.
Per window: a warm-up, then the median of `reps` calls of zg_blocks_verify through the ABI (upload, parsing,
ordering, both kernels, download and the host's uniqueness check included) and the device time of its kernels
(zg_last_sig_kernel_ms); beside it the host build of the same routines (tests/native/zg_hosttest_blocks.hip, -O2)
on `threads` host threads, whole call. Ids and roots are compared byte for byte. Prints one JSON line.

    python tools/bench_blocks.py [--reps K] [--threads T] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIG = 1 << 40
THRESHOLDS = (16384, 65536)


def sapling_tx(tag):
    """a Sapling-format transaction with 2 spends and 1 output: 1,809 bytes"""
    body = hashlib.shake_128(b"tx%d" % tag).digest(768 + 948 + 64)
    return ((0x80000004).to_bytes(4, "little") + (0x892F2085).to_bytes(4, "little") + b"\x00\x00" + bytes(4) +
            bytes(4) + bytes(8) + b"\x02" + body[:768] + b"\x01" + body[768:768 + 948] + b"\x00" + body[-64:])


def windows(scale=1):
    from tests import blocks_cases as C
    from tests import blocks_ref as R
    hdr = C.header()
    sig, pkh = bytes(range(107)), b"\x76\xa9\x14" + bytes(range(20)) + b"\x88\xac"
    small = [R.make_block(hdr, [R.min_tx(8 * b, coinbase=True)] +
                          [R.min_tx(8 * b + i, out_script=pkh, in_script=sig) for i in range(1, 8)])
             for b in range(4096 // scale)]
    per = 1024 // scale
    shielded = [R.make_block(hdr, [R.min_tx(b, coinbase=True)] + [sapling_tx(per * b + i) for i in range(1, per)])
                for b in range(64)]
    long_tx = R.min_tx(7, out_script=b"\x6a" + bytes(100000))
    longer = shielded[:-1] + [R.make_block(hdr, [R.min_tx(63, coinbase=True), long_tx] +
                                           [sapling_tx(per * 63 + i) for i in range(1, per)])]
    return {"small_transparent": small, "shielded_2k": shielded, "shielded_2k_long": longer}


class Call:
    """one window packed for zg_blocks_verify, its output buffers"""

    def __init__(self, blocks):
        from zebra_amd import zg
        self.n = len(blocks)
        arena, self.off = zg.pack_slices(blocks)
        self.arena = arena + b"\0"
        self.ntx = sum(zg.block_layout(b)[1][0] for b in blocks)
        self.st = ctypes.create_string_buffer(self.n)
        self.roots = ctypes.create_string_buffer(32 * self.n)
        self.cnt = (ctypes.c_uint64 * (self.n + 1))()
        self.ids = ctypes.create_string_buffer(32 * self.ntx)

    def gpu(self, ctx):
        from zebra_amd import zg
        ctx._chk(zg.lib().zg_blocks_verify(ctx._p, self.n, self.arena, self.off, BIG, BIG, self.ntx, self.st, None, None,
                                           self.roots, self.cnt, self.ids))


def host(call, threads, reps):
    from tests import blocks_hostlib as H
    HL = H.lib()
    roots, ids = ctypes.create_string_buffer(32 * call.n), ctypes.create_string_buffer(32 * call.ntx)
    cnt, comp = (ctypes.c_uint64 * (call.n + 1))(), ctypes.c_uint64(0)
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        HL.zgh_blocks_roots(call.n, call.arena, call.off, roots, cnt, ids, ctypes.byref(comp), threads)
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), roots.raw, ids.raw, comp.value


def run(reps=11, threads=16, scale=1):
    from tools.bench_ed25519 import timed
    from zebra_amd import Context
    ctxs = {}
    for thr in (0,) + THRESHOLDS:
        os.environ["ZG_TXID_HOST_MIN"] = str(thr)
        ctxs[thr] = Context(device=0, max_batch=64, load_builtin=False)
    del os.environ["ZG_TXID_HOST_MIN"]
    rows = {}
    for name, blocks in windows(scale).items():
        call = Call(blocks)
        wall, kern = timed(ctxs[0], lambda: call.gpu(ctxs[0]), reps)
        assert call.st.raw == bytes(call.n), "a block was not accepted"
        hm, hroots, hids, comp = host(call, threads, max(3, reps // 3))
        assert call.roots.raw == hroots and call.ids.raw == hids, "the device and the host build disagree"
        row = {"blocks": call.n, "transactions": call.ntx, "arena_bytes": len(call.arena) - 1, "reps": reps,
               "txid_compressions": comp, "gpu_abi_ms": wall, "gpu_kernel_ms": kern, "host_threads": threads,
               "host_ms": hm, "gpu_kernel_compressions_per_s": comp / (kern * 1e-3),
               "host_compressions_per_s": comp / (hm * 1e-3), "host_over_gpu_abi_time": hm / wall,
               "host_over_gpu_kernel_time": hm / kern}
        if name == "shielded_2k_long":
            for c in ctxs.values():
                call.gpu(c)                      # warm-up
            times = {thr: [] for thr in ctxs}
            for _ in range(reps):                # alternating, call by call
                for thr, c in ctxs.items():
                    t = time.perf_counter()
                    call.gpu(c)
                    times[thr].append((time.perf_counter() - t) * 1e3)
                    assert call.roots.raw == hroots and call.ids.raw == hids, "ZG_TXID_HOST_MIN changed a result"
            row["host_min_abi_ms"] = {str(thr): {"median": statistics.median(v), "min": min(v), "max": max(v)}
                                      for thr, v in times.items()}
            row["host_min_wins"] = {str(thr): max(times[thr]) < min(times[0]) for thr in THRESHOLDS}
        rows[name] = row
    for c in ctxs.values():
        c.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--scale", type=int, default=1, help="divide the windows by this (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of >= 10 calls)")
    out = {"bench": "blocks_gpu_vs_host", "rows": run(a.reps, a.threads, a.scale)}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
