"""ctypes loader for tests/native/libzg_hosttest_blocks.so: the block parser, the transaction-id reader and the
merkle node the kernels run (zebra_amd/csrc/zg_blocks.h, zg_txparse.h) compiled for the CPU. Test harness and the
host baseline of tools/bench_blocks.py only. Built on demand with hipcc --offload-host-only."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "zg_hosttest_blocks.hip")
LIB = os.path.join(HERE, "native", "libzg_hosttest_blocks.so")
CSRC = os.path.join(ROOT, "zebra_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("zg_blocks.h", "zg_hash.h", "zg_txparse.h")]
HOST_FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-Wno-psabi", "-pthread"]


def build():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        subprocess.check_call(["hipcc"] + HOST_FLAGS + ["-O2", "-fPIC", "-shared", SRC, "-o", LIB + ".tmp"])
        os.replace(LIB + ".tmp", LIB)
    return LIB


def build_program(path):
    """the stand-alone program (its own main), address and undefined-behaviour sanitizers on the host code"""
    subprocess.check_call(["hipcc"] + HOST_FLAGS + ["-O1", "-g", "-DZG_BLK_MAIN", "-Xarch_host", "-fsanitize=address",
                                                    "-Xarch_host", "-fsanitize=undefined",
                                                    "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", path])
    return path


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        u8p, sz, u64p = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
        L.zgh_block_layout.argtypes = [u8p, sz, u64p, u64p, sz]
        L.zgh_txids.argtypes = [sz, u8p, u64p, u8p, ctypes.c_int]
        L.zgh_merkle_root.argtypes = [sz, u8p, u8p]
        L.zgh_blocks_roots.argtypes = [sz, u8p, u64p, u8p, u64p, u8p, u64p, ctypes.c_int]
        _lib = L
    return _lib


def block_layout(raw):
    """zg.block_layout on the host build"""
    out = (ctypes.c_uint64 * 6)()
    st = lib().zgh_block_layout(bytes(raw) + b"\0", len(raw), out, None, 0)
    off = None
    if st != 1:
        buf = (ctypes.c_uint64 * (out[0] + 1))()
        lib().zgh_block_layout(bytes(raw) + b"\0", len(raw), out, buf, out[0] + 1)
        off = list(buf)
    return st, list(out), off


def txids(slices, threads=1):
    """Context.txids on the host build"""
    from zebra_amd import zg
    arena, off = zg.pack_slices(slices)
    n = len(slices)
    hs = ctypes.create_string_buffer(max(32 * n, 1))
    lib().zgh_txids(n, arena + b"\0", off, hs, threads)
    return [hs.raw[32 * i:32 * i + 32] for i in range(n)]


def merkle_root(ids):
    root = ctypes.create_string_buffer(32)
    lib().zgh_merkle_root(len(ids), b"".join(ids), root)
    return root.raw
