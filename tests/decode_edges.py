"""Case builders for the point-decoder edge tests (tests/test_decode_edges.py on the CPU,
tests/test_gpu_decode_edges.py on the GPU). Every verifier starts by decoding attacker-supplied bytes
into curve points, under two rules that decide consensus: a coordinate at or above the field modulus is
an encoding error (it is NOT reduced), and a point outside the prime-order subgroup is an encoding error.

  1  Groth16 alias encodings (BLS12-381): a valid proof with one of A.x, C.x, B.x.c0, B.x.c1 replaced
     by coordinate + p (flag bits kept). A decoder that reduced silently would see the valid proof
     again and accept a second encoding of it. Rule: pairing 0.14 G1Compressed / G2Compressed
     ::into_affine reads each coordinate with Fq::from_repr, which fails with NotInField for a value
     >= p (restated in zg_curve.h g1_decompress / g2_decompress and oracle/bls12_381.py).
  2  cofactor torsion through the proof decoders: a point of every prime part of G1's cofactor as A
     and as C, of every prime part of G2's cofactor h2 as B, and G + T for each; next to every position
     a control, a subgroup point that is not the proof's (status 3 and its own term in gt_out), so
     that a status 1 given for the wrong reason shows.
  3  PGHR13 alias encodings (BN254): x + k q for every G1 point of a valid proof and every k that fits
     32 bytes; for the G2 point b, with U = c1 q + c0 the 64-byte integer, U + j q^2 with c1 + j q below
     2^256 (the c1 < q test of bn_g2_decode), U + j q^2 with a quotient of 2^256 or more (its q_big
     path), and U + m 2^256 q, whose quotient truncated to 256 bits is c1 again (only q_big rejects it).
     Rule: bn's Fq::from_slice gives NotMember, Fq2::from_slice rejects a quotient >= q.
  4  Jubjub alias encodings y + r of valid points, through the RedJubjub key and R, the spend / output
     preparation (cv, rk, epk) and the binding key's cv. Rule: edwards::Point::read, "y is not in field".
  5  uncompressed verifying-key points with x + p and, separately, y + p; and the operands of the
     lexicographic sign compare (fq_lex_greatest / f2_lex_greatest), which decides the sign of every
     decoded point and was tested on random points only.

Why the fixtures' older mutants do not hold these rules (they stay as they are): mutants.json builds
A_x_ge_p as p + 5 and B_x_c1_ge_p / B_x_c0_ge_p as p + 3. x = 5 is on the curve but outside G1 and x = 3
is not on the curve, so a decoder that reduced would still answer status 1. pghr13.json's
mut_c_x_ge_p (q + 5) does hold the rule -- BN254's G1 has cofactor 1 and x = 5 is on the curve -- for
one of seven points at one multiple; mut_b_c1_ge_p (q^2 + 1) aliases c1 = 0, c0 = 1, no proof's point.
For Jubjub only zg_jubjub_decode saw y = r and r + 1; the signature and preparation kernels saw random
flips and b[31] |= 0x7f, never y + r of a valid point.

Out of scope: a GPU case for the c1 = 0 branch of f2_lex_greatest (a B with y.c1 = 0). No subgroup
point with that property can be constructed, so that branch is tested on the host only.

Every expectation comes from the oracles: the C++ restatement of bellman's verify_proof
(tests/cpulib.verify) and oracle/groth16.py, oracle/pghr13.py with tests/cpulib.pg_verify,
oracle/sapling_sig.py and oracle/zcash.py. Nothing here touches the GPU."""
import functools
import json
import os
import random
from collections import namedtuple

from oracle import bls12_381 as B, bn254 as BN, groth16 as G, sapling_sig as S, zcash as Z
from tests import batch_edges as E, cpulib, pghr13_edges as PE
from tests.conftest import load_golden

P = B.P
FQ_ROOM = (1 << 381) - P             # x + p fits the 381 coordinate bits for x below this (about 23 %)
NVARIANTS = 9 * E.VARIANTS           # the distinct proofs of batch_edges.pool()
MIN_TWINS = 2
# coordinate -> (offset of its 48 bytes in the proof, offset of the byte that carries its point's flags)
COORDS = {"A.x": (0, 0), "B.x.c1": (48, 48), "B.x.c0": (96, 48), "C.x": (144, 144)}
POINT_OFF = {"A": (0, 48), "B": (48, 96), "C": (144, 48)}

Special = namedtuple("Special", "name role slot r status")   # role: alias | torsion | control | orig


# ------------------------------------------------------------------ 1. Groth16 alias encodings
def coord_get(proof, coord):
    off, fl = COORDS[coord]
    v = int.from_bytes(proof[off:off + 48], "big")
    return v & ((1 << 381) - 1) if off == fl else v


def coord_set(proof, coord, v):
    """the proof with one coordinate's 381 bits replaced, its flag bits left as they were"""
    off, fl = COORDS[coord]
    assert 0 <= v < 1 << 381
    p = bytearray(proof)
    flags = p[off] & 0xE0 if off == fl else 0
    p[off:off + 48] = v.to_bytes(48, "big")
    p[off] |= flags
    return bytes(p)


def flip_sign(proof, coord):
    p = bytearray(proof)
    p[COORDS[coord][1]] ^= 0x20
    return bytes(p)


def _more_variants(start, count):
    """re-randomisations start .. start + count - 1 of the nine sources, formed as batch_edges.pool() forms
    its own, verified by the oracle"""
    srcs = E.sources()
    out = []
    for i in range(start, start + count):
        e = srcs[i % 9]
        t, s = G.rerandomize_scalars(E.RERAND_SEED, i)
        p = G.proof_bytes(G.rerandomize(G.proof_read(bytes.fromhex(e["proof"])), E.pvks()[e["kind"]].vk.delta_g2, t, s))
        out.append((e["kind"], p, [bytes.fromhex(x) for x in e["inputs"]], None))
    r = random.Random(E.RERAND_SEED + start).randbytes(16 * count)
    assert E._from_slots("more", out, r).statuses == [0] * count
    return [(s, r[16 * k:16 * k + 16]) for k, s in enumerate(out)]


def _candidates(vs):
    return {c: [i for i, (s, _) in enumerate(vs) if coord_get(s[1], c) < FQ_ROOM] for c in COORDS}


@functools.lru_cache(maxsize=None)
def variants():
    """[(slot, r)]: the 36 distinct proofs of batch_edges.pool() with their scalar rows, extended nine at a
    time under further seeds while some coordinate has fewer than MIN_TWINS proofs with room for + p"""
    slots, rs = E.pool()
    vs = [(slots[i], rs[i]) for i in range(NVARIANTS)]
    while min(len(v) for v in _candidates(vs).values()) < MIN_TWINS:
        assert len(vs) < 20 * NVARIANTS
        vs += _more_variants(len(vs), 9)
    return vs


def _with_proof(slot, proof):
    return (slot[0], proof, slot[2], slot[3])


@functools.lru_cache(maxsize=None)
def alias_specials():
    """per coordinate every variant with room: the twin coordinate + p (status 1); for the first of each
    coordinate also the twin with its sign flag flipped (1), the untouched original (0) and the original with
    its sign flag flipped (the negated point: 3)"""
    vs = variants()
    out = []
    for c, idx in _candidates(vs).items():
        for q, i in enumerate(idx):
            slot, r = vs[i]
            twin = coord_set(slot[1], c, coord_get(slot[1], c) + P)
            out.append(Special("%s+p v%d" % (c, i), "alias", _with_proof(slot, twin), r, 1))
            if q == 0:
                out.append(Special("%s+p sign v%d" % (c, i), "alias", _with_proof(slot, flip_sign(twin, c)), r, 1))
                out.append(Special("%s original v%d" % (c, i), "orig", slot, r, 0))
                out.append(Special("%s original sign v%d" % (c, i), "orig", _with_proof(slot, flip_sign(slot[1], c)), r, 3))
    return out


def twin_source(sp):
    """(coordinate, variant index) of an alias special"""
    head, v = sp.name.rsplit(" v", 1)
    return head.split("+")[0], int(v)


# ------------------------------------------------------------------ 2. cofactor torsion
L6 = 402096035359507321594726366720466575392706800671181159425656785868777272553337714697862511267018014931937703598282857976535744623203249
H2_PARTS = [(13, 2), (23, 2), (2713, 1), (11953, 1), (262069, 1), (L6, 1)]


def h2():
    """the cofactor of G2 on the twist: #E'(Fp2) = h2 r"""
    x = -B.BLS_X
    h = 1
    for ell, e in H2_PARTS:
        h *= ell ** e
    assert 9 * h == x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13
    return h


def _g2_name(ell):
    return "order_l6" if ell == L6 else "order_%d" % ell


@functools.lru_cache(maxsize=None)
def g2_torsion_cases():
    """[(name, twist point, in G2 by the oracle)]: per prime part l^e of h2 a point T_l = [h2 r / l^e] (a
    seeded random twist point) that is not infinity, with [l^e] T_l = O; Q + T_l for a Q in G2; Q and the
    generator. Plain oracle arithmetic, fixed seed."""
    rng = random.Random(0x62)
    n2 = h2() * B.R

    def rand_twist():
        while True:
            x = (rng.randrange(P), rng.randrange(P))
            y = B.f2_sqrt(B.f2_add(B.f2_mul(B.f2_sqr(x), x), B.B2))
            if y is not None:
                return (x, y)

    q = B.ec_mul(B.FQ2, B.G2_GEN, rng.randrange(1, B.R))
    small = []
    for ell, e in H2_PARTS:
        assert n2 % ell ** e == 0 and n2 // ell ** e % ell != 0
        while True:
            t = B.ec_mul(B.FQ2, rand_twist(), n2 // ell ** e)
            if t is not None:
                break
        assert B.ec_mul(B.FQ2, t, ell ** e) is None
        small.append((_g2_name(ell), t))
    out = small + [("q_plus_" + nm, B.ec_add(B.FQ2, q, t)) for nm, t in small] + [("q", q), ("generator", B.G2_GEN)]
    assert all(B.on_curve(B.FQ2, B.B2, p) for _, p in out)
    return [(nm, p, B.g2_in_subgroup(p)) for nm, p in out]


def g1_torsion_cases():
    """tests/test_g1_digit_chains.subgroup_cases: T_l for l = 3, 11, 10177, 859267, 52437899, G + T_l, the
    fixture's point and (0, 2), with the oracle's verdicts"""
    from tests.test_g1_digit_chains import subgroup_cases
    return subgroup_cases()


def put_point(proof, pos, enc):
    off, ln = POINT_OFF[pos]
    assert len(enc) == ln
    return proof[:off] + enc + proof[off + ln:]


CONTROL_K = {"A": 0xA11CE, "C": 0xC0FFEE, "B": 0xB0B}


@functools.lru_cache(maxsize=None)
def torsion_specials():
    """every point outside its subgroup, compressed, in a pool proof: the G1 points as A and, separately, as
    C, the G2 points as B (status 1); per position one control [k] G in the slot of that position's first
    case (status 3, its own left-hand side in gt_out). The host proofs cycle over the variants, so over all
    three keys."""
    vs = variants()
    out, at = [], 0
    g1 = [(nm, B.g1_compress(p)) for nm, p, ok in g1_torsion_cases() if not ok]
    g2 = [(nm, B.g2_compress(p)) for nm, p, ok in g2_torsion_cases() if not ok]
    ctl = {"A": B.g1_compress(B.ec_mul(B.FQ, B.G1_GEN, CONTROL_K["A"])),
           "C": B.g1_compress(B.ec_mul(B.FQ, B.G1_GEN, CONTROL_K["C"])),
           "B": B.g2_compress(B.ec_mul(B.FQ2, B.G2_GEN, CONTROL_K["B"]))}
    controls = []
    for pos, pts in (("A", g1), ("C", g1), ("B", g2)):
        for q, (nm, enc) in enumerate(pts):
            slot, r = vs[at % NVARIANTS]
            at += 5                      # 5 is coprime to 36: hosts of every source and key
            out.append(Special("%s=%s" % (pos, nm), "torsion", _with_proof(slot, put_point(slot[1], pos, enc)), r, 1))
            if q == 0:
                controls.append(Special("%s=[k]G" % pos, "control", _with_proof(slot, put_point(slot[1], pos, ctl[pos])), r, 3))
    return out + controls


# ------------------------------------------------------------------ Groth16 batches
def specials():
    return alias_specials() + torsion_specials()


BATCH_SIZES = [65, 129]
SPECIALS_PER_BATCH = {65: 56, 129: 120}


@functools.lru_cache(maxsize=None)
def groth16_batches(n):
    """the batches of n slots that together hold every special once: an alias twin in slot 0, the rest of
    the alias side, good pool proofs as padding, the torsion side with a torsion case in slot n - 1 ->
    [(Case, [Special | None per slot])]"""
    al = sorted(alias_specials(), key=lambda s: s.role != "alias")      # twins first (stable)
    to = torsion_specials()                                            # torsion cases first, controls last
    k = -(-(len(al) + len(to)) // SPECIALS_PER_BATCH[n])
    slots, rs = E.pool()
    out = []
    for j in range(k):
        head, tail = al[j::k], to[j::k][::-1]
        assert head[0].role == "alias" and tail[-1].role == "torsion" and len(head) + len(tail) < n
        pad = n - len(head) - len(tail)
        who = head + [None] * pad + tail
        pads = [(slots[(7 * j + i) % NVARIANTS], rs[(7 * j + i) % NVARIANTS]) for i in range(pad)]
        rows = [(s.slot, s.r) for s in head] + pads + [(s.slot, s.r) for s in tail]
        case = E._from_slots("decode%d/%d" % (n, j), [s for s, _ in rows], b"".join(r for _, r in rows))
        out.append((case, who))
    return out


def expected_statuses(who):
    return [0 if s is None else s.status for s in who]


@functools.lru_cache(maxsize=None)
def single_lane_cases():
    """n = 1: one alias twin, one torsion case"""
    a = next(s for s in alias_specials() if s.role == "alias")
    t = next(s for s in torsion_specials() if s.name.startswith("B="))
    return [(E._from_slots("one:" + s.name, [s.slot], s.r), [s]) for s in (a, t)]


# ------------------------------------------------------------------ 3. PGHR13 alias encodings
BQ = BN.P
PG_G1 = {"a": 0, "a_prime": 33, "b_prime": 131, "c": 164, "c_prime": 197, "k": 230, "h": 263}
PG_B = 66
PG_KMAX = ((1 << 256) - 1) // BQ     # 5: x + k q can fit 32 bytes up to this k


def pg_g1_x(proof, point):
    o = PG_G1[point]
    return int.from_bytes(proof[o + 1:o + 33], "big")


def pg_set_g1_x(proof, point, v):
    o = PG_G1[point]
    return proof[:o + 1] + v.to_bytes(32, "big") + proof[o + 33:]


def pg_b_u(proof):
    return int.from_bytes(proof[PG_B + 1:PG_B + 65], "big")


def pg_set_b_u(proof, u):
    return proof[:PG_B + 1] + u.to_bytes(64, "big") + proof[PG_B + 65:]


def pg_valid():
    sl = PE.slots()
    return [("valid%d" % i,) + sl["valid%d" % i][:2] for i in range(9)]


@functools.lru_cache(maxsize=None)
def pghr13_twins():
    """name -> (proof, inputs, what): what = ("g1", point, k) | ("c1", j) | ("big", j, quotient) |
    ("wrap", m, quotient). Every (point, k) that fits in some valid case appears once, the case rotating;
    likewise every j with c1 + j q < 2^256; one U + j q^2 and one U + m 2^256 q with a quotient >= 2^256"""
    valid = pg_valid()
    out = {}
    for pi, point in enumerate(PG_G1):
        for k in range(1, PG_KMAX + 1):
            for t in range(9):
                nm, proof, ins = valid[(pi + k + t) % 9]
                x = pg_g1_x(proof, point)
                if x + k * BQ < 1 << 256:
                    out["%s:%s+%dq" % (nm, point, k)] = (pg_set_g1_x(proof, point, x + k * BQ), ins, ("g1", point, k))
                    break
    for j in range(1, PG_KMAX + 1):
        for t in range(9):
            nm, proof, ins = valid[(j + t) % 9]
            u = pg_b_u(proof)
            if u // BQ + j * BQ < 1 << 256:
                out["%s:b+%dq^2" % (nm, j)] = (pg_set_b_u(proof, u + j * BQ * BQ), ins, ("c1", j))
                break
    nm, proof, ins = valid[4]
    u = pg_b_u(proof)
    j = next(j for j in range(1, 32) if (u + j * BQ * BQ) // BQ >= 1 << 256)
    assert u + j * BQ * BQ < 1 << 512
    out["%s:b+%dq^2 (q_big)" % (nm, j)] = (pg_set_b_u(proof, u + j * BQ * BQ), ins, ("big", j, (u + j * BQ * BQ) // BQ))
    for m in (1, PG_KMAX - 1):
        nm, proof, ins = valid[4 + m]
        u = pg_b_u(proof)
        w = u + (m << 256) * BQ
        assert w < 1 << 512 and (w // BQ) % (1 << 256) == u // BQ and w % BQ == u % BQ
        out["%s:b+%d*2^256q (wrap)" % (nm, m)] = (pg_set_b_u(proof, w), ins, ("wrap", m, w // BQ))
    return out


class PgCase:
    """one zg_pghr13_verify call over named items (valid cases and twins), in the shape the runner of
    tests/test_gpu_pghr13_edges.py takes; statuses from tests/cpulib.pg_verify"""

    def __init__(self, name, names):
        self.name, self.names, self.n = name, list(names), len(names)

    def _items(self):
        tw, va = pghr13_twins(), {nm: (p, ins) for nm, p, ins in pg_valid()}
        return [tw[k][:2] if k in tw else va[k] for k in self.names]

    @property
    def proofs(self):
        return b"".join(p for p, _ in self._items())

    @property
    def inputs(self):
        return b"".join(b"".join(ins) + bytes(32 * (9 - len(ins))) for _, ins in self._items())

    @property
    def counts(self):
        return bytes(len(ins) for _, ins in self._items())

    @property
    def statuses(self):
        st = pghr13_statuses()
        return [st[k] for k in self.names]

    @property
    def fails(self):
        return PE.VERIFY_FAILED in self.statuses


@functools.lru_cache(maxsize=None)
def pghr13_statuses():
    """name -> status by the C++ restatement of the reference's check, twins and valid cases in one call"""
    tw = pghr13_twins()
    names = [nm for nm, _, _ in pg_valid()] + list(tw)
    items = [(p, ins) for _, p, ins in pg_valid()] + [v[:2] for v in tw.values()]
    got = cpulib.pg_verify(cpulib.load_pghr13(), [p for p, _ in items], [list(ins) for _, ins in items], threads=8)
    return dict(zip(names, got))


def pghr13_cases():
    """n = 1: a G1 twin, a c1 twin, the q_big twin and a wrap twin, each alone; past a wave: every twin in
    one call among valid proofs, twins in slot 0 and slot n - 1"""
    tw = list(pghr13_twins())
    pick = [next(k for k in tw if pghr13_twins()[k][2][0] == w) for w in ("g1", "c1", "big", "wrap")]
    ones = [PgCase("one:" + k, [k]) for k in pick]
    n = max(65, len(tw) + 9)
    if n % 64 == 0:
        n += 1
    names = ["valid%d" % (i % 9) for i in range(n)]
    names[0], names[n - 1] = tw[0], tw[-1]
    for i, k in enumerate(tw[1:-1]):
        names[1 + i * (n - 2) // (len(tw) - 2)] = k
    assert sorted(k for k in names if k in pghr13_twins()) == sorted(tw)
    return ones + [PgCase("all%d" % n, names)]


# ------------------------------------------------------------------ 4. Jubjub alias encodings
JR = B.R                              # Jubjub's base field is the BLS12-381 scalar field
JJ_ROOM = (1 << 255) - JR             # y + r fits the 255 bits for y below this (about 10 %)
JJ_SCAN = 96
JJ_MIN_POINTS = 4


def jj_alias(enc):
    """the encoding with y replaced by y + r, the sign bit kept"""
    v = int.from_bytes(enc, "little")
    y = v & ((1 << 255) - 1)
    assert y < JJ_ROOM
    return ((v >> 255 << 255) | (y + JR)).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def jj_small_y():
    """{gen: [(k, encoding of [k] G_gen)]} for k = 1 .. JJ_SCAN with y < 2^255 - r; gen 0 / 1 the RedJubjub
    generators, 2 G_v"""
    out = {}
    for gen, g in ((0, S.GENERATORS[0]), (1, S.GENERATORS[1]), (2, S.VALUE_COMMITMENT_VALUE)):
        acc, hits = S.ZERO, []
        for k in range(1, JJ_SCAN + 1):
            acc = S.add(acc, g)
            enc = S.encode(acc)
            if Z.jubjub_read(enc)[1] < JJ_ROOM:
                hits.append((k, enc))
        out[gen] = hits
    return out


RJItem = namedtuple("RJItem", "name vk sig msg gen ok")


@functools.lru_cache(maxsize=None)
def redjubjub_items():
    """per generator: an honest signature under a key with a small y (accepted), the same with the key
    encoded as y + r (the message keeps the canonical key bytes); an honest signature whose R has a small
    y (accepted), and the one made over the alias Rbar -- c = H*(Rbar || msg), S = nonce + c sk -- which a
    reducing decoder accepts and the reference rejects"""
    rng = random.Random(0x4a6a)
    items = []
    for gen in (S.GEN_SPEND_AUTH, S.GEN_BINDING):
        hits = jj_small_y()[gen]
        (sk, vk), (nonce, rbar) = hits[0], hits[-1]
        msg = vk + rng.randbytes(32)
        sig = S.redjubjub_sign(sk, msg, gen, rng.randbytes(80))
        items.append(RJItem("key small y gen %d" % gen, vk, sig, msg, gen, True))
        items.append(RJItem("key y + r gen %d" % gen, jj_alias(vk), sig, msg, gen, False))
        sk2 = rng.randrange(1, S.RJ)
        vk2 = S.public_key(sk2, gen)
        msg2 = vk2 + rng.randbytes(32)
        for name, rb, ok in (("R small y gen %d" % gen, rbar, True), ("R y + r gen %d" % gen, jj_alias(rbar), False)):
            s = (nonce + S.h_star(rb, msg2) * sk2) % S.RJ
            items.append(RJItem(name, vk2, rb + s.to_bytes(32, "little"), msg2, gen, ok))
    return items


def redjubjub_batch(n):
    """n = 1: the first alias item alone; else the items among the fixtures' valid signatures, an alias item
    in slot 0 and in slot n - 1"""
    from tests import sig_edges
    items = redjubjub_items()
    bad = [i for i in items if not i.ok]
    if n == 1:
        return [bad[0]]
    valid, _ = sig_edges.fixture_rj_items()
    rest = [i for i in items if i is not bad[0] and i is not bad[-1]]
    fill = [RJItem(v.name, v.vk, v.sig, v.msg, v.gen, v.ok) for v in valid]
    mid = rest + [fill[i % len(fill)] for i in range(n - 2 - len(rest))]
    return [bad[0]] + mid + [bad[-1]]


PrepJob = namedtuple("PrepJob", "name kind args want")    # kind "spend" | "output"; want: None or the error's name


@functools.lru_cache(maxsize=None)
def prep_jobs():
    """a real spend and a real output with cv / rk / epk replaced by small-y points (accepted), then each
    of those fields in turn as y + r: the error the oracle's restatement names"""
    tf = load_golden("input_prep.json")["tx_fields"]
    h = bytes.fromhex
    s, o = tf["spends"][0], tf["outputs"][0]
    pts = jj_small_y()
    cv, rk, epk = pts[2][0][1], pts[0][1][1], pts[1][1][1]
    spend = [cv, h(s["anchor"]), h(s["nullifier"]), rk]
    output = [cv, h(o["cmu"]), epk]
    jobs = [("spend small y", "spend", spend), ("output small y", "output", output),
            ("spend cv y + r", "spend", [jj_alias(cv)] + spend[1:]),
            ("spend rk y + r", "spend", spend[:3] + [jj_alias(rk)]),
            ("output cv y + r", "output", [jj_alias(cv)] + output[1:]),
            ("output epk y + r", "output", output[:2] + [jj_alias(epk)])]
    out = []
    for name, kind, args in jobs:
        try:
            (Z.spend_inputs if kind == "spend" else Z.output_inputs)(*args)
            want = None
        except Z.InputError as e:
            want = e.where
        out.append(PrepJob(name, kind, tuple(args), want))
    return out


def prep_oracle_rows(job):
    f = Z.spend_inputs if job.kind == "spend" else Z.output_inputs
    return [x.to_bytes(32, "little") for x in f(*job.args)]


@functools.lru_cache(maxsize=None)
def bvk_rows():
    """zg_sapling_bvk rows (spends, outputs, value balance, status, bvk): small-y cvs (status 0), then one of
    them as y + r among the spends and among the outputs (status 1)"""
    from tests.sig_edges import bvk_expect
    pts = [enc for _, enc in jj_small_y()[2][:3]]
    rows = [(pts[:2], pts[2:], 5), ([jj_alias(pts[0]), pts[1]], pts[2:], 5), (pts[:2], [jj_alias(pts[2])], 5)]
    return [(tuple(s), tuple(o), v) + bvk_expect(list(s), list(o), v) for s, o, v in rows]


# ------------------------------------------------------------------ 5. uncompressed verifying-key points
VK_FIELDS = ("alphaG1", "betaG1", "betaG2", "gammaG2", "deltaG1", "deltaG2")


def _vk_json(kind):
    return json.load(open(os.path.join(cpulib.ROOT, "zebra_amd", "res", cpulib.VK_FILES[kind])))


def _unhex(s):
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


@functools.lru_cache(maxsize=None)
def vk_alias_cases():
    """[(name, kind, fields dict, ic list)]: the builtin keys with one 48-byte coordinate of one point replaced
    by coordinate + p -- a G1 point's x, a G1 point's y, a G2 point's x (either half), a G2 point's y (either
    half); each the first such coordinate with room, over the three keys in turn. An uncompressed point's
    three flag bits are zero and stay zero."""
    wanted = {("g1", "x"): None, ("g1", "y"): None, ("g2", "x"): None, ("g2", "y"): None}
    for kind in (0, 1, 2):
        d = _vk_json(kind)
        pts = [(f, None, _unhex(d[f])) for f in VK_FIELDS] + [("ic", i, _unhex(x)) for i, x in enumerate(d["ic"])]
        for f, i, raw in pts:
            grp = "g1" if len(raw) == 96 else "g2"
            half = len(raw) // 2
            for q in range(len(raw) // 48):
                key = (grp, "x" if 48 * q < half else "y")
                v = int.from_bytes(raw[48 * q:48 * q + 48], "big")
                if wanted[key] is None and v < FQ_ROOM:
                    new = raw[:48 * q] + (v + P).to_bytes(48, "big") + raw[48 * q + 48:]
                    wanted[key] = ("%s[%s] of key %d, coordinate %d + p" % (f, i, kind, q), kind, f, i, new)
    assert all(wanted.values()), wanted
    out = []
    for name, kind, f, i, new in wanted.values():
        d = _vk_json(kind)
        fields = {k: _unhex(d[k]) for k in VK_FIELDS}
        ic = [_unhex(x) for x in d["ic"]]
        if f == "ic":
            ic[i] = new
        else:
            fields[f] = new
        out.append((name, kind, fields, ic))
    return out


def vk_json_text(fields, ic):
    d = {k: fields[k].hex() for k in VK_FIELDS}
    d["ic"] = [x.hex() for x in ic]
    return json.dumps(d)


# ------------------------------------------------------------------ 5. the lexicographic sign compare
def lex_fq_values():
    """y = (p - 1) / 2, (p + 1) / 2, 1, p - 1, 0; and (p - 1) / 2 with one 32-bit limb one higher or one lower,
    per limb and direction (the values that stay canonical)"""
    half = (P - 1) // 2
    out = [half, half + 1, 1, P - 1, 0]
    for limb in range(12):
        for d in (1, -1):
            v = half + d * (1 << (32 * limb))
            if 0 <= v < P:
                out.append(v)
    return out


def lex_f2_values():
    """every Fq case as c1 with c0 on either side of (p - 1) / 2; c1 = 0 with c0 over the Fq cases"""
    half = (P - 1) // 2
    fq = lex_fq_values()
    out = [(c0, c1) for c1 in fq if c1 for c0 in (0, 1, half, half + 1, P - 1)]
    return out + [(c0, 0) for c0 in fq]
