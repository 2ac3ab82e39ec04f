"""CPU tier of the lazy-digit G1 point chains (zebra_amd/csrc/zg_fqd.h): the sum of two products under
one reduction (fq29d_dot2 / fqd_dot2) that closes every point formula's Y3, the formulas themselves
(g1d_dbl, g1d_add_aff, g1d_add_full, g1d_readd) and the subgroup check, as the one walk of x^2
(g1_in_subgroup_d) and as two walks of |x| (g1_in_subgroup_xx, ZG_SUBGROUP_XX), compiled for the host
(tests/native/zg_hosttest_g1d.hip) next to the word-form jac_dbl / jac_add / g1_in_subgroup and the
oracle.

The harness is built twice: plain, and with ZG_FQD_CHECK, where every intermediate is verified
against the bound its comment documents (normalized digits, value < K p)."""
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
SRC = os.path.join(HERE, "native", "zg_hosttest_g1d.hip")
CSRC = os.path.join(ROOT, "zebra_amd", "csrc")
P = B.P
X = B.BLS_X
RP = 1 << 406                 # R' of the digit form
RPI = pow(RP, -1, P)
MASK = (1 << 29) - 1

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def _build(check):
    lib = os.path.join(HERE, "native", "libzg_hosttest_g1d%s.so" % ("_chk" if check else ""))
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
    assert lib.zgg_checking() == int(request.param)
    assert lib.zgg_dot2_on() == 1   # the default is what is tested
    return lib


def fq_b(x):
    return x.to_bytes(48, "big")


def g1_b(p):
    return fq_b(p[0]) + fq_b(p[1])


def aff_b(p):
    """the harness's 97-byte affine record"""
    return b"\x01" + bytes(96) if p is None else b"\x00" + g1_b(p)


_REAL = None


def real_points():
    """the A and C of every real proof (all in G1), decoded once"""
    global _REAL
    if _REAL is None:
        _REAL = []
        for e in load_golden("real_proofs.json")["proofs"]:
            a, _, c = OG.proof_read(bytes.fromhex(e["proof"]))
            _REAL += [a, c]
    return _REAL


# ------------------------------------------------------------------ fqd_dot2
def digits(v):
    assert 0 <= v < 1 << 410
    return [(v >> (29 * i)) & MASK for i in range(13)] + [v >> 377]


def dot2(L, vals, canon):
    arr = (ctypes.c_uint32 * 56)(*[d for v in vals for d in digits(v)])
    raw, out = (ctypes.c_uint32 * 14)(), ctypes.create_string_buffer(48)
    L.zgg_dot2(arr, raw, int(canon), out)
    assert all(raw[i] <= MASK for i in range(13)), vals          # normalized
    r = sum(raw[i] << (29 * i) for i in range(14))
    a, b, c, d = vals
    assert r % P == (a * b + c * d) * RPI % P, vals
    assert r * RP < a * b + c * d + P * RP, vals                  # < (a b + c d) / 2^406 + p
    return r, out.raw


def test_dot2_against_integers(L):
    rng = random.Random(901)
    edge = [0, 1, 2, P - 1, P - 2, 1 << 380]
    pairs = [(a, b) for a in edge for b in edge]
    quads = [pairs[i] + pairs[(7 * i + 3) % len(pairs)] for i in range(len(pairs))]
    quads += [pairs[i] + pairs[(5 * i + 1) % len(pairs)] for i in range(len(pairs))]
    quads += [tuple(rng.randrange(P) for _ in range(4)) for _ in range(200)]
    for a, b, c, d in quads:
        # canonical values enter in the digit form's Montgomery representation v R' mod p
        r, out = dot2(L, [v * RP % P for v in (a, b, c, d)], True)
        assert out == fq_b((a * b + c * d) % P), (a, b, c, d)
        assert r < 2 * P
    assert L.zgg_check_fails() == 0


def test_dot2_at_the_lazy_bounds(L):
    """the largest K p each call site passes: g1d_dbl's (E < 6, W < 28, 3p - B < 3, 8B < 16), the additions'
    (rr < 43 for the loosest invariant, W < 12, k p - Y < 20, 2J < 4); and every digit at 2^29 - 1 (the
    column bound 14 (2^58 + 2^58) + 14 2^58 < 2^64 at its end)"""
    for ks in [(6, 28, 3, 16), (43, 12, 20, 4), (13, 12, 5, 4)]:
        vals = [k * P - 1 for k in ks]
        r, out = dot2(L, vals, True)
        assert r < 2 * P                                          # the < 2p the formulas rely on
        assert out == fq_b(r * RPI % P)
        r, _ = dot2(L, [k * P - 1 - (i << 200) for i, k in enumerate(ks)], True)
        assert r < 2 * P
    top = (1 << 406) - 1
    dot2(L, [top] * 4, False)
    dot2(L, [top, 1, top, top - 1], False)
    dot2(L, [top, 0, 0, top], True)
    assert L.zgg_check_fails() == 0


# ------------------------------------------------------------------ the point formulas
DBL, ADDQ, SAVE, ADDT, READD, TINF, SUBQ, ADDQF = range(8)


def walk(L, start, q, ops):
    """both forms' canonical affine points after every step; asserts they agree bit for bit"""
    n = len(ops)
    od, ow = ctypes.create_string_buffer(97 * n), ctypes.create_string_buffer(97 * n)
    L.zgg_walk(g1_b(start) if start else bytes(96), int(start is None), g1_b(q), bytes(ops), n, od, ow)
    for k in range(n):
        assert od.raw[97 * k:97 * k + 97] == ow.raw[97 * k:97 * k + 97], (k, ops[k])
    return [od.raw[97 * k:97 * k + 97] for k in range(n)]


def test_formulas_on_real_points(L):
    """every formula once from every real A and C, against the oracle's affine arithmetic"""
    pts = real_points()
    for i, p in enumerate(pts):
        q = pts[(i + 1) % len(pts)]
        p2, pq = B.ec_add(B.FQ, p, p), B.ec_add(B.FQ, p, q)
        got = walk(L, p, q, [DBL])
        assert got[0] == aff_b(p2)
        got = walk(L, p, q, [ADDQ, SUBQ, ADDQF])
        assert got == [aff_b(pq), aff_b(p), aff_b(pq)]
        # T = 2P (a Jacobian point with Z != 1), then Q + T by both full additions
        got = walk(L, p, q, [DBL, SAVE, TINF, ADDT, SAVE, DBL, ADDT, READD])
        p4 = B.ec_add(B.FQ, p2, p2)
        p6 = B.ec_add(B.FQ, p4, p2)
        assert got[7] == aff_b(B.ec_add(B.FQ, p6, p2)) and got[6] == aff_b(p6)
    assert L.zgg_check_fails() == 0


def test_formulas_special_cases(L):
    """P + P, P + (-P) and the point at infinity on either side, through every addition"""
    pts = real_points()
    for p in pts[:4]:
        p2 = B.ec_add(B.FQ, p, p)
        inf = aff_b(None)
        # mixed: P + P doubles, P - P is infinity, infinity + P is P
        assert walk(L, p, p, [ADDQ, SUBQ, SUBQ, ADDQ, SUBQ]) == [aff_b(p2), aff_b(p), inf, aff_b(p), inf]
        assert walk(L, None, p, [ADDQ, DBL]) == [aff_b(p), aff_b(p2)]
        assert walk(L, None, p, [DBL, SUBQ]) == [inf, aff_b(B.ec_neg(B.FQ, p))]
        # full, q affine as Jacobian: P + P, then 2P + P
        assert walk(L, p, p, [ADDQF, ADDQF])[0] == aff_b(p2)
        assert walk(L, None, p, [ADDQF]) == [aff_b(p)]
        # full and cached with T: T = infinity on the right, s = infinity on the left, T + T, T - T
        for add in (ADDT, READD):
            assert walk(L, p, p, [add])[0] == aff_b(p)                       # T starts as infinity
            got = walk(L, p, p, [DBL, SAVE, add, SUBQ, SUBQ, SUBQ, SUBQ, add])  # 2P + 2P; 4P - 4P = O; O + T
            p4 = B.ec_add(B.FQ, p2, p2)
            assert got[2] == aff_b(p4) and got[6] == inf and got[7] == aff_b(p2)
            # s = -T: the sum is infinity (T = 2P with Z != 1, s = -2P reached as P - 3P)
            got = walk(L, p, p, [DBL, SAVE, SUBQ, SUBQ, SUBQ, SUBQ, add])
            assert got[5] == aff_b(B.ec_neg(B.FQ, p2)) and got[6] == inf
    assert L.zgg_check_fails() == 0


def test_random_walk_keeps_the_invariant(L):
    """300 seeded steps from one state: every formula's lazy output is the next one's input"""
    rng = random.Random(902)
    pts = real_points()
    ops = [rng.choice([DBL, DBL, ADDQ, SUBQ, ADDT, READD, ADDQF, SAVE, DBL, READD]) for _ in range(300)]
    ops[0], ops[1] = DBL, SAVE
    got = walk(L, pts[0], pts[3], ops)
    # the oracle's own walk of the same steps
    s, t, q = pts[0], None, pts[3]
    for k, op in enumerate(ops):
        if op == DBL:
            s = B.ec_add(B.FQ, s, s)
        elif op in (ADDQ, ADDQF):
            s = B.ec_add(B.FQ, s, q)
        elif op == SUBQ:
            s = B.ec_add(B.FQ, s, B.ec_neg(B.FQ, q))
        elif op == SAVE:
            t = s
        else:
            s = B.ec_add(B.FQ, s, t)
        assert got[k] == aff_b(s), (k, op)
    assert L.zgg_check_fails() == 0


# ------------------------------------------------------------------ the subgroup check
def curve_order():
    """N = h r with h = (x + 1)^2 / 3 (x = -BLS_X), checked against p + 1 - t, t = x + 1"""
    u = -X
    h = (u - 1) ** 2 // 3
    assert (u - 1) ** 2 % 3 == 0
    n = h * B.R
    assert n == P + 1 - (u + 1)
    return n


_SUB = None


def subgroup_cases():
    """(name, point, in G1 by the oracle), formed once"""
    global _SUB
    if _SUB is not None:
        return _SUB
    rng = random.Random(903)
    n = curve_order()
    out = [("real_%d" % i, p) for i, p in enumerate(real_points())]
    data = bytes.fromhex(load_golden("points.json")["g1_not_in_subgroup"])
    x = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:], "big")
    y = B.fq_sqrt((x ** 3 + 4) % P)
    out.append(("g1_not_in_subgroup", (x, y)))
    out.append(("order_3_0_2", (0, 2)))

    def rand_point():
        while True:
            x = rng.randrange(P)
            y = B.fq_sqrt((x ** 3 + 4) % P)
            if y is not None:
                return (x, y)

    small = []
    for ell, k in [(3, n // 3), (11, n // 121), (10177, n // 10177 ** 2), (859267, n // 859267 ** 2),
                   (52437899, n // 52437899 ** 2)]:
        assert n % (ell * ell) == 0 or ell == 3
        while True:
            t = B.ec_mul(B.FQ, rand_point(), k)
            if t is not None:
                break
        assert B.ec_mul(B.FQ, t, ell * ell if ell != 3 else 3) is None
        small.append(("order_%d" % ell, t))
    out += small
    out += [("gen_plus_" + nm, B.ec_add(B.FQ, B.G1_GEN, t)) for nm, t in small]
    out.append(("generator", B.G1_GEN))
    _SUB = [(nm, p, B.g1_in_subgroup(p)) for nm, p in out]
    return _SUB


def test_subgroup_check_against_the_oracle(L):
    cases = subgroup_cases()
    assert all(w for nm, _, w in cases if nm.startswith("real_") or nm == "generator")
    assert not any(w for nm, _, w in cases if not (nm.startswith("real_") or nm == "generator"))
    for nm, p, want in cases:
        assert B.on_curve(B.FQ, B.B1, p), nm
        got = L.zgg_subgroup(fq_b(p[0]), fq_b(p[1]))
        assert got == (7 if want else 0), (nm, got, want)   # the default walk, the word form, the two x-walks
    assert L.zgg_check_fails() == 0
