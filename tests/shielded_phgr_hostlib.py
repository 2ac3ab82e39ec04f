"""ctypes loader for tests/native/libzg_hosttest_shielded_phgr.so: the plan, gather, row and fold routines the kernels of
zg_shielded_verify_flags run with ZG_SHIELDED_PHGR (zebra_amd/csrc/zg_shielded.h), compiled for the CPU. Test harness
only. Built on demand with hipcc --offload-host-only, as tests/shielded_hostlib.py."""
import ctypes
import os
import subprocess

from tests import shielded_hostlib as H4
from tests.script_hostlib import HERE, HOST_FLAGS

SRC = os.path.join(HERE, "native", "zg_hosttest_shielded_phgr.hip")
LIB = os.path.join(HERE, "native", "libzg_hosttest_shielded_phgr.so")
DEPS = [SRC] + H4.DEPS


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
        L.zgh_shielded_phgr_verify.argtypes = ([sz, u8p, u64p, u32p, ctypes.c_uint32] + [u8p] * 8 +
                                               [u8p, u8p, u64p, u8p, u64p] + [u8p] * 10 + [u64p])
        _lib = L
    return _lib


def shielded_verify(txs, branch_ids, flags, hashes, bvk, bvk_st, bind_ok, ed, spend_ok, proof, pghr):
    """the host build of zg_shielded_verify_flags around verdicts computed by the caller. Per transaction of the window:
    hashes, bvk (32 bytes each), bvk_st, bind_ok, ed (a byte each); per v4 description: spend_ok, proof; per PHGR
    description: pghr (ZG_STATUS_*) -> the return code and a dict of everything the routines wrote"""
    from zebra_amd import zg
    ntx = len(txs)
    arena, tx_off, branch = zg.pack_shielded(txs, branch_ids)
    cap = len(arena) // 384 + 1
    buf = lambda n: ctypes.create_string_buffer(max(n, 1))  # noqa: E731
    ts, st, dt = buf(ntx), buf(ntx), buf(ntx)
    ix, doff, counts = (ctypes.c_uint64 * max(ntx, 1))(), (ctypes.c_uint64 * (ntx + 1))(), (ctypes.c_uint64 * 6)()
    ds, kinds, codes, nin, inputs, proofs = buf(cap), buf(cap), buf(cap), buf(cap), buf(288 * cap), buf(192 * cap)
    rj, edr, pgp, pgi = buf(161 * (cap + ntx)), buf(128 * ntx), buf(296 * cap), buf(288 * cap)
    rc = lib().zgh_shielded_phgr_verify(ntx, arena + b"\0", tx_off, branch, flags, b"".join(hashes) + b"\0",
                                        b"".join(bvk) + b"\0", bytes(bvk_st) + b"\0", bytes(bind_ok) + b"\0",
                                        bytes(ed) + b"\0", bytes(spend_ok) + b"\0", bytes(proof) + b"\0",
                                        bytes(pghr) + b"\0", ts, st, ix, dt, doff, ds, kinds, codes, nin, inputs, proofs,
                                        rj, edr, pgp, pgi, counts)
    if rc:
        return rc, None
    nd, nrj, ned, ns, np, npd = counts
    return 0, {"tx_status": list(ts.raw[:ntx]), "status": list(st.raw[:ntx]), "index": list(ix[:ntx]),
               "detail": list(dt.raw[:ntx]), "desc_status": [list(ds.raw[doff[t]:doff[t + 1]]) for t in range(ntx)],
               "kinds": list(kinds.raw[:nd]), "proofs": [proofs.raw[192 * d:192 * d + 192] for d in range(nd)],
               "ed": [edr.raw[128 * e:128 * e + 128] for e in range(ned)],
               "pg_proofs": [pgp.raw[296 * d:296 * d + 296] for d in range(npd)],
               "pg_inputs": [pgi.raw[288 * d:288 * d + 288] for d in range(npd)], "counts": (nd, nrj, ned, ns, np, npd)}
