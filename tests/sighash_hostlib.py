"""ctypes loader for tests/native/libzg_hosttest_sighash.so: the signature hash and the transaction parser the
kernels run (zebra_amd/csrc/zg_sighash.h, zg_txparse.h) compiled for the CPU. Test harness and the host
baseline of tools/bench_sighash.py only. Built on demand with hipcc --offload-host-only."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "zg_hosttest_sighash.hip")
LIB = os.path.join(HERE, "native", "libzg_hosttest_sighash.so")
CSRC = os.path.join(ROOT, "zebra_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("zg_sighash.h", "zg_hash.h", "zg_txparse.h")]
HOST_FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-Wno-psabi", "-pthread"]


def build():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        subprocess.check_call(["hipcc"] + HOST_FLAGS + ["-O2", "-fPIC", "-shared", SRC, "-o", LIB + ".tmp"])
        os.replace(LIB + ".tmp", LIB)
    return LIB


def build_program(path):
    """the stand-alone program (its own main), address and undefined-behaviour sanitizers on the host code"""
    subprocess.check_call(["hipcc"] + HOST_FLAGS + ["-O1", "-g", "-DZG_SH_MAIN", "-Xarch_host", "-fsanitize=address",
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
        L.zgh_tx_layout.argtypes = [u8p, sz, u64p]
        L.zgh_sighash.argtypes = [sz, u8p, u64p, u32p, sz, u32p, u32p, u8p, u32p, u64p, u32p, u8p, u8p, u8p, ctypes.c_int]
        _lib = L
    return _lib


def sighash(txs, branch_ids, items, threads=1):
    """Context.sighash on the host build -> (tx_status, hashes, status)"""
    from zebra_amd import zg
    ntx, n = len(txs), len(items)
    arena, tx_off, branch, item_tx, index, scripts, script_off, amount, hashtype = zg.pack_sighash(txs, branch_ids, items)
    ts = ctypes.create_string_buffer(max(ntx, 1))
    hs = ctypes.create_string_buffer(max(32 * n, 1))
    st = ctypes.create_string_buffer(max(n, 1))
    lib().zgh_sighash(ntx, arena + b"\0", tx_off, branch, n, item_tx, index, scripts + b"\0", script_off, amount,
                      hashtype, ts, hs, st, threads)
    return list(ts.raw[:ntx]), [hs.raw[32 * i:32 * i + 32] for i in range(n)], list(st.raw[:n])
