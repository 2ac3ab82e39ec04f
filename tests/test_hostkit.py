"""CPU tier of the host plumbing (zebra_amd/csrc/zg_host.h): offsets_ok, host_threads, seeded_bytes and the arena's
carve arithmetic, in the stand-alone program tests/native/zg_hosttest_hostkit.hip built with the address and
undefined-behaviour sanitizers on the host code (its own main, no preload, no HIP call). The thread fan-out runs a
second time under the thread sanitizer. What the helpers do on the device is tests/test_gpu_call_edges.py."""
import glob
import hashlib
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "zg_hosttest_hostkit.hip")
HOST_FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-Wno-psabi", "-pthread", "-O1", "-g"]
ASAN_UBSAN = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
              "-Xarch_host", "-fno-sanitize-recover=undefined"]
TSAN = ["-Xarch_host", "-fsanitize=thread"]
TSAN_RUNTIME = glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.tsan-x86_64.a")

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostkit") / "zg_hosttest_hostkit")
    subprocess.check_call(["hipcc"] + HOST_FLAGS + ASAN_UBSAN + [SRC, "-o", exe])
    return exe


def run(exe, part):
    p = subprocess.run([exe, part], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


@needs_hipcc
@pytest.mark.parametrize("part", ["offsets", "threads", "carve"])
def test_self_checks_under_sanitizers(program, part):
    """offsets: n = 0, equal offsets, a decreasing pair first / middle / last, spans of exactly 2^31 and 2^31 + 1,
    no limit, a nonzero first offset, both widths. threads: 0, 1, 15, 16, 17 and 1,000 items under the three
    partitionings of the tree, every index once, nt = 1 on the caller alone. carve: alignment, disjoint parts,
    the total the sizing pass gave, null for a part of no bytes."""
    out = run(program, part).split()
    assert out[:2] == [part, "ok"] and int(out[2]) > 0, out


@needs_hipcc
def test_seeded_bytes_are_blake2b_of_tag_seed_index(program):
    lines = run(program, "seeded").splitlines()
    want = []
    for tag, size in ((b"zg-batch-r", 16), (b"zg-rerand", 64), (b"zg-pghr13-rho", 64), (b"zg-pghr13-rho1", 64)):
        for seed in (0, 1, 2 ** 64 - 1):
            for i in (0, 1, 2 ** 32 + 5):
                h = hashlib.blake2b(tag + seed.to_bytes(8, "little") + i.to_bytes(8, "little"), digest_size=size)
                want.append("%s %d %d %d %s" % (tag.decode(), size, seed, i, h.hexdigest()))
    assert len(want) == 36 and lines == want


@needs_hipcc
@pytest.mark.skipif(not TSAN_RUNTIME, reason="the toolchain has no thread-sanitizer runtime")
def test_host_threads_under_the_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "zg_hosttest_hostkit_tsan")
    subprocess.check_call(["hipcc"] + HOST_FLAGS + TSAN + [SRC, "-o", exe])
    assert run(exe, "threads").split()[:2] == ["threads", "ok"]
