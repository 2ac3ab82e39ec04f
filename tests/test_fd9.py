"""The 9 x 29-bit digit field of the signature kernels (zebra_amd/csrc/zg_fd9.h) at its digit bounds, for
both moduli, on the CPU: tests/native/zg_hosttest_fd9.hip runs mul, sqr, add and sub over raw digits and
the results are compared with Python big integers.

The header's contract: a "tight" element has every digit below 2^29 + 2^14 (2^255 - 19) or 2^29 + 2^21
(2^256 - 2^32 - 977), and that is what every function returns; a product accepts the uncarried sum of two
tight elements ("loose": digits up to 2 tight - 2); add and sub take tight operands."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "zg_hosttest_fd9.hip")
LIB = os.path.join(HERE, "native", "libzg_hosttest_fd9.so")
CSRC = os.path.join(ROOT, "zebra_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# field index of zgt_fd9_op -> (p, tight bound)
FIELDS = {0: (2 ** 255 - 19, 2 ** 29 + 2 ** 14), 1: (2 ** 256 - 2 ** 32 - 977, 2 ** 29 + 2 ** 21)}
MUL, SQR, ADD, SUB = range(4)

_LIB = None


def lib():
    """built on demand like tests/hostlib.py"""
    global _LIB
    if _LIB is None:
        deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-O2", "-fPIC", "-shared",
                                   "-std=c++17", "-Wno-psabi", SRC, "-o", LIB + ".tmp"])
            os.replace(LIB + ".tmp", LIB)
        _LIB = ctypes.CDLL(LIB)
    return _LIB


def value(d):
    return sum(x << (29 * i) for i, x in enumerate(d))


def digits(x):
    assert 0 <= x < 2 ** 261
    return [(x >> (29 * i)) & (2 ** 29 - 1) for i in range(9)]


def operands(field):
    """the product operands: the widest and the tight extreme, zero, all-ones digits, p - 1, p, 2 p, and
    256 seeded random ones with digits uniform below the tight or (per operand) the loose bound"""
    p, tight = FIELDS[field]
    ops = [[2 * tight - 2] * 9, [tight - 1] * 9, [0] * 9, [2 ** 29 - 1] * 9, digits(p - 1), digits(p), digits(2 * p)]
    rnd = random.Random(1100 + field)
    for k in range(256):
        bound = tight if k % 2 == 0 else 2 * tight - 1
        ops.append([rnd.randrange(bound) for _ in range(9)])
    return ops


def pairs(field, op):
    p, tight = FIELDS[field]
    ops = operands(field)
    if op in (ADD, SUB):
        ops = [[min(x, tight - 1) for x in d] for d in ops]
    special, rnd = ops[:7], ops[7:]
    out = [(a, b) for a in special for b in special]
    out += [(rnd[i], rnd[(i + 1) % len(rnd)]) for i in range(len(rnd))]        # tight x loose, loose x tight
    out += [(rnd[i], rnd[(i + 2) % len(rnd)]) for i in range(len(rnd))]        # tight x tight, loose x loose
    out += [(s, r) for s in special for r in rnd[:8]] + [(r, s) for s in special for r in rnd[:8]]
    return out


def run(field, op, ps):
    n = len(ps)
    arr = ctypes.c_uint32 * (9 * n)
    a = arr(*[x for p_ in ps for x in p_[0]])
    b = arr(*[x for p_ in ps for x in p_[1]])
    r = arr()
    assert lib().zgt_fd9_op(field, op, ctypes.c_size_t(n), a, b, r) == 0
    return [list(r[9 * i:9 * i + 9]) for i in range(n)]


@pytest.mark.parametrize("op", [MUL, SQR, ADD, SUB])
@pytest.mark.parametrize("field", [0, 1])
def test_field_ops_at_the_digit_bounds(field, op):
    p, tight = FIELDS[field]
    ps = pairs(field, op)
    got = run(field, op, ps)
    top = 0
    for (a, b), r in zip(ps, got):
        x, y = value(a), value(b)
        want = (x * y, x * x, x + y, x - y)[op] % p
        assert value(r) % p == want, (field, op, a, b, r)
        assert max(r) < tight, (field, op, a, b, r)
        top = max(top, max(r))
    print("field %d op %d: %d cases, largest result digit 2^29 + %d" % (field, op, len(ps), top - 2 ** 29))


@pytest.mark.parametrize("field", [0, 1])
def test_canon_of_from_words(field):
    p, _ = FIELDS[field]
    xs = [0, 1, p - 1, p, p + 1, 2 ** 255, 2 ** 256 - 1]
    arr = ctypes.c_uint32 * (8 * len(xs))
    src = arr(*[(x >> (32 * i)) & 0xffffffff for x in xs for i in range(8)])
    out = arr()
    assert lib().zgt_fd9_canon(field, ctypes.c_size_t(len(xs)), src, out) == 0
    for k, x in enumerate(xs):
        got = sum(out[8 * k + i] << (32 * i) for i in range(8))
        assert got == x % p, (field, hex(x), hex(got))
