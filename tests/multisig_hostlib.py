"""ctypes loader for tests/native/libzg_hosttest_multisig.so: the matcher with the multisig classes and the routines
the multisig kernels of zg_inputs_verify run (zebra_amd/csrc/zg_script.h, zg_multisig.h) with the signature hash and
the ECDSA check behind them, compiled for the CPU. Test harness and the host baseline of tools/bench_multisig.py only.
Built on demand with hipcc --offload-host-only, as tests/script_hostlib.py."""
import ctypes
import os
import subprocess

from tests.script_hostlib import CSRC, HERE, HOST_FLAGS

SRC = os.path.join(HERE, "native", "zg_hosttest_multisig.hip")
LIB = os.path.join(HERE, "native", "libzg_hosttest_multisig.so")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("zg_script.h", "zg_inputs.h", "zg_multisig.h", "zg_sighash.h", "zg_hash.h",
                                                "zg_txparse.h", "zg_ecdsa.h", "zg_fd9.h")]


def build():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        subprocess.check_call(["hipcc"] + HOST_FLAGS + ["-O2", "-fPIC", "-shared", SRC, "-o", LIB + ".tmp"])
        os.replace(LIB + ".tmp", LIB)
    return LIB


def build_program(path):
    """the stand-alone program (its own main), address and undefined-behaviour sanitizers on the host code"""
    subprocess.check_call(["hipcc"] + HOST_FLAGS + ["-O1", "-g", "-DZG_MS_MAIN", "-Xarch_host", "-fsanitize=address",
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
        L.zgh_script_match.argtypes = [u8p, sz, u8p, sz, ctypes.c_uint32, u64p]
        L.zgh_inputs_verify.argtypes = [sz, u8p, u64p, u32p, sz, u32p, u32p, u8p, u32p, u64p, ctypes.c_uint32, u8p, u8p,
                                        u8p, u8p, ctypes.c_int]
        _lib = L
    return _lib


def script_match(script_sig, script_pubkey, flags):
    out = (ctypes.c_uint64 * 8)()
    rc = lib().zgh_script_match(bytes(script_sig) + b"\0", len(script_sig), bytes(script_pubkey) + b"\0", len(script_pubkey),
                                flags, out)
    assert rc == 0, "an offset outside the script"
    return tuple(out)


def inputs_verify(txs, branch_ids, items, flags, threads=1):
    """Context.inputs_verify on the host build -> (tx_status, status, detail, hashes)"""
    from zebra_amd import zg
    ntx, n = len(txs), len(items)
    arena, tx_off, branch, item_tx, index, prev, prev_off, amount = zg.pack_inputs_verify(txs, branch_ids, items)
    ts = ctypes.create_string_buffer(max(ntx, 1))
    st = ctypes.create_string_buffer(max(n, 1))
    dt = ctypes.create_string_buffer(max(n, 1))
    hs = ctypes.create_string_buffer(max(32 * n, 1))
    lib().zgh_inputs_verify(ntx, arena + b"\0", tx_off, branch, n, item_tx, index, prev + b"\0", prev_off, amount, flags,
                            ts, st, dt, hs, threads)
    return list(ts.raw[:ntx]), list(st.raw[:n]), list(dt.raw[:n]), [hs.raw[32 * i:32 * i + 32] for i in range(n)]
