"""CPU tier of the digit-resident lane R-chain (zebra_amd/csrc/zg_lines.h lsd_double / lsd_add over
zg_fqd.h Fq2D, selected by ZG_LINES_FQD): the kernel's own step functions compiled for the host
(tests/native/zg_hosttest_digit.hip) next to the word-form ls_double / ls_add they replace.

After every one of the 68 steps the three line coefficients and the canonical (X, Y, Z) must equal
the word form's bit for bit, and the closing G2 verdict must agree, on the B and r A of every real
proof, on a B outside G2, on coordinates of 0 and p - 1, on a lane without a B to check and on an
inactive lane. The harness is built twice: plain, and with ZG_FQD_CHECK, where every intermediate
is verified against the bound its comment documents (normalized digits, value < K p)."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from oracle import bls12_381 as B
from oracle import groth16 as OG
from tests.conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "zg_hosttest_digit.hip")
CSRC = os.path.join(ROOT, "zebra_amd", "csrc")
STEPS = 68
P = B.P

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def _build(check):
    lib = os.path.join(HERE, "native", "libzg_hosttest_digit%s.so" % ("_chk" if check else ""))
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        tmp = lib + ".%d.tmp" % os.getpid()
        subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-O2", "-fPIC", "-shared", "-std=c++17",
                               "-Wno-psabi", "-Wno-duplicate-decl-specifier"] +
                              (["-DZG_FQD_CHECK"] if check else []) + [SRC, "-o", tmp])
        os.replace(tmp, lib)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "bounds"])
def L(request):
    lib = _build(request.param)
    assert lib.zgd_checking() == int(request.param)
    return lib


def fq_b(x):
    return x.to_bytes(48, "big")


def g2_b(q):
    return b"".join(fq_b(v) for v in (q[0][0], q[0][1], q[1][0], q[1][1]))


def g1_b(p):
    return fq_b(p[0]) + fq_b(p[1])


_CASES = None


def chain_cases():
    """(name, B bytes, r A bytes, chk, act, want_in_g2 or None), computed once"""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = random.Random(808)
    out = []
    real = load_golden("real_proofs.json")["proofs"]
    for i, e in enumerate(real):
        a, b, _ = OG.proof_read(bytes.fromhex(e["proof"]))
        ra = B.ec_mul(B.FQ, a, OG.batch_r(rng.randbytes(16)))
        out.append(("real_%d" % i, g2_b(b), g1_b(ra), 1, 1, True))
    a0, b0, _ = OG.proof_read(bytes.fromhex(real[0]["proof"]))
    pa = g1_b(B.ec_mul(B.FQ, a0, 12345))
    # a B on the curve but outside G2: the closing check must fail, and exactly where the word form does
    bad = _g2_outside_subgroup()
    out.append(("g2_not_in_subgroup", g2_b(bad), pa, 1, 1, False))
    # coordinates at the ends of the range (not curve points: the formulas are polynomial, any input runs)
    edge = [0, P - 1]
    for k in range(16):
        q = [edge[(k >> j) & 1] for j in range(4)]
        out.append(("edge_%x" % k, b"".join(fq_b(v) for v in q), fq_b(edge[k & 1]) + fq_b(edge[(k >> 1) & 1]), 1, 1,
                    None))
    out.append(("edge_p_pm1", g2_b(b0), fq_b(P - 1) + fq_b(0), 1, 1, True))
    out.append(("no_b_to_check", g2_b(b0), pa, 0, 1, None))       # walks (1, 1, 1), adds B all the same
    out.append(("inactive", g2_b(b0), pa, 1, 0, True))             # identity lines, B still checked
    out.append(("inactive_no_b", g2_b(b0), pa, 0, 0, None))
    _CASES = out
    return out


def _g2_outside_subgroup():
    """the fixture's point, decompressed without the subgroup check (x, then the y the flag bits select)"""
    data = bytes.fromhex(load_golden("points.json")["g2_not_in_subgroup"])
    x1 = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:48], "big")
    x0 = int.from_bytes(data[48:96], "big")
    x = (x0, x1)
    y = B.f2_sqrt(B.f2_add(B.f2_mul(B.f2_sqr(x), x), B.B2))
    assert y is not None
    ny = B.f2_neg(y)
    if not (B.f2_cmp_gt(ny, y) ^ bool(data[0] & 0x20)):   # as oracle g2_decompress picks the root
        y = ny
    assert not B.g2_in_subgroup((x, y))
    return (x, y)


def run_chain(L, q, p, chk, act):
    w, d = ctypes.create_string_buffer(STEPS * 6 * 96), ctypes.create_string_buffer(STEPS * 6 * 96)
    res = (ctypes.c_int * 3)()
    L.zgd_chain(q, p, chk, act, w, d, res)
    assert res[2] == STEPS
    return w.raw, d.raw, bool(res[0]), bool(res[1])


def test_digit_steps_equal_word_steps(L):
    ident = (fq_b(1) + fq_b(0)) * 3
    for name, q, p, chk, act, want in chain_cases():
        w, d, vw, vd = run_chain(L, q, p, chk, act)
        for n in range(STEPS):
            a, b = w[n * 576:(n + 1) * 576], d[n * 576:(n + 1) * 576]
            assert a[:288] == b[:288], (name, "lines", n)
            assert a[288:] == b[288:], (name, "point", n)
            if not act:
                assert b[:288] == ident, (name, n)
        assert vw == vd, name
        if want is not None:
            assert vd == want, name
    assert L.zgd_check_fails() == 0


def test_digit_lines_equal_g2_prepared(L):
    """and against the oracle's G2Prepared lines with ell's px / py scaling, for one real proof"""
    name, q, p, chk, act, _ = chain_cases()[0]
    e = load_golden("real_proofs.json")["proofs"][0]
    _, b, _ = OG.proof_read(bytes.fromhex(e["proof"]))
    px, py = int.from_bytes(p[:48], "big"), int.from_bytes(p[48:], "big")
    _, d, _, _ = run_chain(L, q, p, chk, act)
    for n, (c0, c1, c2) in enumerate(B.g2_prepare(b)):
        want = b"".join(fq_b(v) for v in (c2[0], c2[1], c1[0] * px % P, c1[1] * px % P, c0[0] * py % P, c0[1] * py % P))
        assert d[n * 576:n * 576 + 288] == want, n


def test_digit_products(L):
    """the Fq2D product, square, product by an Fq, and the two mixed-representation products on edge
    and random operands"""
    rng = random.Random(809)
    edge = [0, 1, 2, P - 1, P - 2, (1 << 380), (1 << 381) - 1 - P if (1 << 381) - 1 > P else 3]
    vals = [(a, b) for a in edge for b in edge] + [(rng.randrange(P), rng.randrange(P)) for _ in range(200)]
    for i, x in enumerate(vals):
        y = vals[(7 * i + 3) % len(vals)]
        s = vals[(5 * i + 1) % len(vals)][0]
        out, ref = ctypes.create_string_buffer(5 * 96), ctypes.create_string_buffer(5 * 96)
        L.zgd_products(fq_b(x[0]) + fq_b(x[1]), fq_b(y[0]) + fq_b(y[1]), fq_b(s), out, ref)
        assert out.raw == ref.raw, (x, y, s)
        xy = ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)
        assert out.raw[:96] == fq_b(xy[0]) + fq_b(xy[1])
    assert L.zgd_check_fails() == 0


GLV_EDGES = [0, 1, (1 << 64) - 1, 1 << 63, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555]


def test_glv_two_columns_with_a_table_store_equals_one_column(L):
    """g1_glv_mul_w2_t (the table behind a store parameter; here the plain-array store) against
    g1_glv_mul_d on the A point of every real proof: every pair of the edge scalars (0, 1, 2^64 - 1, a
    single top bit, alternating bits) and seeded random pairs; and against the oracle's [r] A"""
    rng = random.Random(810)
    pairs = [(a, b) for a in GLV_EDGES for b in GLV_EDGES] + \
        [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(12)]
    L.zgd_glv.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p,
                          ctypes.c_char_p]
    real = load_golden("real_proofs.json")["proofs"]
    for i, e in enumerate(real):
        pa, _, _ = OG.proof_read(bytes.fromhex(e["proof"]))
        for j, (a, b) in enumerate(pairs):
            d, w = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
            L.zgd_glv(fq_b(pa[0]), fq_b(pa[1]), a, b, d, w)
            assert d.raw == w.raw, (i, hex(a), hex(b))
            if (i + j) % 16 == 0:
                r16 = a.to_bytes(8, "little") + b.to_bytes(8, "little")
                assert w.raw == g1_b(B.ec_mul(B.FQ, pa, OG.batch_r(r16))), (i, hex(a), hex(b))
    assert L.zgd_check_fails() == 0
