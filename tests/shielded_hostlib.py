"""ctypes loader for tests/native/libzg_hosttest_shielded.so: the plan, gather, row and fold routines the kernels of
zg_shielded_verify run (zebra_amd/csrc/zg_shielded.h) and the JoinSplit preparation of zg_prep.h, compiled for the CPU.
Test harness only. Built on demand with hipcc --offload-host-only, as tests/multisig_hostlib.py."""
import ctypes
import os
import subprocess

from tests.script_hostlib import CSRC, HERE, HOST_FLAGS

SRC = os.path.join(HERE, "native", "zg_hosttest_shielded.hip")
LIB = os.path.join(HERE, "native", "libzg_hosttest_shielded.so")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("zg_shielded.h", "zg_prep.h", "zg_sighash.h", "zg_hash.h", "zg_txparse.h",
                                                "zg_field.h")]


def build():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        subprocess.check_call(["hipcc"] + HOST_FLAGS + ["-O2", "-fPIC", "-shared", SRC, "-o", LIB + ".tmp"])
        os.replace(LIB + ".tmp", LIB)
    return LIB


def build_program(path):
    """the stand-alone program (its own main), address and undefined-behaviour sanitizers on the host code"""
    subprocess.check_call(["hipcc"] + HOST_FLAGS + ["-O1", "-g", "-DZG_SHD_MAIN", "-Xarch_host", "-fsanitize=address",
                                                    "-Xarch_host", "-fsanitize=undefined",
                                                    "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", path])
    return path


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        u8p, sz = ctypes.c_char_p, ctypes.c_size_t
        u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        L.zgh_shielded_verify.argtypes = [sz, u8p, u64p, u32p] + [u8p] * 7 + [u8p, u8p, u64p, u8p, u64p] + [u8p] * 8 + [u64p]
        L.zgh_prep_joinsplit.argtypes = [u8p, u8p, u8p]
        _lib = L
    return _lib


def prep_joinsplit(desc, pubkey):
    out = ctypes.create_string_buffer(288)
    lib().zgh_prep_joinsplit(bytes(desc), bytes(pubkey), out)
    return out.raw


def shielded_verify(txs, branch_ids, hashes, bvk, bvk_st, bind_ok, ed, spend_ok, proof):
    """the host build of zg_shielded_verify around verdicts computed by the caller. Per transaction: hashes, bvk (32
    bytes each), bvk_st, bind_ok, ed (a byte each); per description of the window: spend_ok, proof -> a dict of
    everything the routines wrote"""
    from zebra_amd import zg
    ntx = len(txs)
    arena, tx_off, branch = zg.pack_shielded(txs, branch_ids)
    cap = len(arena) // 384 + 1
    buf = lambda n: ctypes.create_string_buffer(max(n, 1))  # noqa: E731
    ts, st, dt = buf(ntx), buf(ntx), buf(ntx)
    ix, doff, counts = (ctypes.c_uint64 * max(ntx, 1))(), (ctypes.c_uint64 * (ntx + 1))(), (ctypes.c_uint64 * 4)()
    ds, kinds, codes, nin, inputs, proofs = buf(cap), buf(cap), buf(cap), buf(cap), buf(288 * cap), buf(192 * cap)
    rj, edr = buf(161 * (cap + ntx)), buf(128 * ntx)
    rc = lib().zgh_shielded_verify(ntx, arena + b"\0", tx_off, branch, b"".join(hashes) + b"\0", b"".join(bvk) + b"\0",
                                   bytes(bvk_st) + b"\0", bytes(bind_ok) + b"\0", bytes(ed) + b"\0",
                                   bytes(spend_ok) + b"\0", bytes(proof) + b"\0", ts, st, ix, dt, doff, ds, kinds, codes,
                                   nin, inputs, proofs, rj, edr, counts)
    assert rc == 0, rc
    nd, nrj, ned, ns = counts
    return {"tx_status": list(ts.raw[:ntx]), "status": list(st.raw[:ntx]), "index": list(ix[:ntx]),
            "detail": list(dt.raw[:ntx]), "desc_status": [list(ds.raw[doff[t]:doff[t + 1]]) for t in range(ntx)],
            "kinds": list(kinds.raw[:nd]), "codes": list(codes.raw[:nd]), "ninputs": list(nin.raw[:nd]),
            "inputs": [inputs.raw[288 * d:288 * d + 288] for d in range(nd)],
            "proofs": [proofs.raw[192 * d:192 * d + 192] for d in range(nd)],
            "rj": [rj.raw[161 * r:161 * r + 161] for r in range(nrj)],
            "ed": [edr.raw[128 * e:128 * e + 128] for e in range(ned)], "counts": (nd, nrj, ned, ns)}
