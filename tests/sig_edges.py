"""Vectors for the three signature kernels -- RedJubjub with the binding key and the Jubjub decode (f1),
Ed25519 (f5), secp256k1 ECDSA (f7) -- shared by tests/test_sig_edges.py (CPU tier: the vectors are
pinned against oracle/sapling_sig.py, tests/ed25519_ref.py and tests/ecdsa_ref.py) and
tests/test_gpu_sig_edges.py (GPU tier: the same vectors through the Context). Fixed seeds, no golden
file: everything is derived from those three references.

A. One accepted item per reachable entry of every fixed-base comb table d * 2^(8 w) * G (d = 1..255,
   w = 0..31, built on the device by k_jj_comb / k_ed_comb / k_ec_comb). The scalar that multiplies G
   is exactly one digit, d << 8w, so the kernel makes exactly one lookup and a wrong entry flips exactly
   one verdict; every item's name carries (table, w, d). Reachable entries and what is NOT reachable:
     RedJubjub   S < r_J (0x0e7d...): all d for w <= 30, d <= 14 for w = 31 -> 7,919 per generator
                 (spend-auth and binding); entries (w = 31, d = 15..255) are never read.
     G_v         zg_sapling_bvk multiplies by |valueBalance| <= 2^63 - 1: all d for w <= 6, d <= 127
                 for w = 7 -> 1,912, taken with both signs; entries (w = 7, d = 128..255) and all of
                 windows 8..31 are unreachable through the ABI.
     Ed25519     sig[63] & 0xE0 == 0: all d for w <= 30, d <= 31 for w = 31 -> 7,936; the S of the
                 other 224 (w = 31, d = 32..255) is ZG_ED_SIGNATURE_ENCODING, which is asserted.
     ECDSA       u1 = d << 8w < n for all 8,160.
   With a trivial key a kernel that skipped the table would still have to produce R, so every window of
   every table also gets a twin: the same scalar with the R (ECDSA: the signature) of another digit,
   which must be rejected.
B. RedJubjub items the reference accepts only because of its cofactor 8 (torsion in R, in vk), the
   boundary S = r_J - 1 / r_J, the all-trivial signature, an honest signature with S = 0, and the `gen`
   byte outside {0, 1} (include/zg.h: every value but ZG_GEN_BINDING is the spend-auth generator).
C. zg_sapling_bvk rows (ragged, failing rows next to good ones, the value-balance edges) and
   zg_jubjub_decode points (the 8 torsion points, y at the ends of the field) at the sizes where a
   wave or a block ends.
"""
import functools
import random
from collections import namedtuple

from oracle import sapling_sig as S
from oracle import zcash as Z
from tests import ecdsa_ref as EC
from tests import ed25519_ref as ED
from tests.conftest import load_golden

SIZES = (1, 63, 64, 65, 129)          # a lane, a wave less one, a wave, a second block, a third
WINDOWS, DIGITS = 32, 255
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

RJ_TOP_D = 14                         # 14 << 248 < r_J < 15 << 248
ED_TOP_D = 31                         # (d << 248) >> 248 & 0xE0 == 0
GV_TOP_W, GV_TOP_D = 7, 127           # 127 << 56 <= 2^63 - 1 < 128 << 56
RJ_ENTRIES = 31 * DIGITS + RJ_TOP_D               # 7,919 per generator
GV_ENTRIES = GV_TOP_W * DIGITS + GV_TOP_D         # 1,912 per sign
ED_ENTRIES = 31 * DIGITS + ED_TOP_D               # 7,936
ED_UNREADABLE = DIGITS - ED_TOP_D                 # 224
EC_ENTRIES = WINDOWS * DIGITS                     # 8,160

JJ_IDENTITY = (1).to_bytes(32, "little")          # edwards::Point::write of (0, 1)
ED_IDENTITY = (1).to_bytes(32, "little")

RJItem = namedtuple("RJItem", "name vk sig msg gen ok")      # gen: the byte the ABI gets
EdItem = namedtuple("EdItem", "name pubkey sig msg status")
EcItem = namedtuple("EcItem", "name pubkey sig msg status")
BvkRow = namedtuple("BvkRow", "name spends outputs value status bvk")


def rj_top_digit(w):
    return RJ_TOP_D if w == WINDOWS - 1 else DIGITS


def ed_top_digit(w):
    return ED_TOP_D if w == WINDOWS - 1 else DIGITS


def gv_top_digit(w):
    return GV_TOP_D if w == GV_TOP_W else DIGITS


def subset_digits(w, top, last_w=WINDOWS - 1):
    """the digits whose items the CPU tier sends through the reference verifier: every d of window 0
    and of the top window, d in {1, 128, largest valid} of every other window"""
    if w in (0, last_w):
        return list(range(1, top + 1))
    return sorted({1, min(128, top), top})


def comb_points(g, add, windows=WINDOWS):
    """{(w, d): d * 2^(8 w) * g} for d = 1..255 by repeated addition: 255 additions a window, the 256th
    sum being the next window's base"""
    out, base = {}, g
    for w in range(windows):
        acc = base
        for d in range(1, DIGITS + 1):
            out[w, d] = acc
            acc = add(acc, base)
        base = acc
    return out


def twin_digits(seed, top_digit, per_window=1):
    """per window per_window triples (w, d, d2), d != d2, both reachable: d's scalar goes with d2's point"""
    rng = random.Random(seed)
    out = []
    for w in range(WINDOWS):
        for d in rng.sample(range(1, top_digit(w) + 1), per_window):
            d2 = rng.choice([x for x in range(1, top_digit(w) + 1) if x != d])
            out.append((w, d, d2))
    return out


def shuffled(items, seed):
    items = list(items)
    random.Random(seed).shuffle(items)
    return items


# ----------------------------------------------------------------------------- Jubjub helpers
def jj_encode_affine(x, y):
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def jj_encode(p):
    """S.encode with the inverse by pow(-1) (the builders encode some 20,000 points)"""
    zi = pow(p[2], -1, S.R)
    return jj_encode_affine(p[0] * zi % S.R, p[1] * zi % S.R)


@functools.lru_cache(maxsize=None)
def jj_comb(gen):
    """gen 0 / 1: the RedJubjub generators, 2: G_v (the third table of k_jj_comb)"""
    g = S.VALUE_COMMITMENT_VALUE if gen == 2 else S.GENERATORS[gen]
    return comb_points(g, S.add, WINDOWS if gen < 2 else GV_TOP_W + 1)


def redjubjub_verify_no_cofactor(vk_bytes, sig, msg, gen):
    """S.redjubjub_verify without the final [8]: what a kernel that dropped its three doublings checks"""
    try:
        vk, r = S.read(vk_bytes), S.read(sig[:32])
    except S.PointError:
        return False
    s = int.from_bytes(sig[32:], "little")
    if s >= S.RJ:
        return False
    c = S.h_star(sig[:32], msg)
    return S.is_zero(S.add(S.add(S.mul(vk, c), r), S.neg(S.mul(S.GENERATORS[gen], s))))


def oracle_gen(gen_byte):
    """the generator a `gen` byte selects (include/zg.h): ZG_GEN_BINDING, else spend-auth"""
    return S.GEN_BINDING if gen_byte == S.GEN_BINDING else S.GEN_SPEND_AUTH


def rj_oracle(item):
    return S.redjubjub_verify(item.vk, item.sig, item.msg, oracle_gen(item.gen))


# ----------------------------------------------------------------------------- A. RedJubjub tables
@functools.lru_cache(maxsize=None)
def redjubjub_table_items():
    """(entries, twins): vk the identity, R = encode([S] G_gen), S = d << 8w, a random message: then
    [c] vk + R - [S] G = O whatever c is. Twins carry the R of another digit of the same window."""
    rng = random.Random(0x5e1)
    entries, twins = [], []
    for gen in (S.GEN_SPEND_AUTH, S.GEN_BINDING):
        pts = jj_comb(gen)
        enc = {(w, d): jj_encode(pts[w, d]) for w in range(WINDOWS) for d in range(1, rj_top_digit(w) + 1)}
        for (w, d), rbar in enc.items():
            s = (d << (8 * w)).to_bytes(32, "little")
            entries.append(RJItem("rj-table gen %d w %d d %d" % (gen, w, d), JJ_IDENTITY, rbar + s,
                                  rng.randbytes(64), gen, True))
        for w, d, d2 in twin_digits(0x7a0 + gen, rj_top_digit):
            s = (d << (8 * w)).to_bytes(32, "little")
            twins.append(RJItem("rj-twin gen %d w %d d %d (R of d %d)" % (gen, w, d, d2), JJ_IDENTITY,
                                enc[w, d2] + s, rng.randbytes(64), gen, False))
    return entries, twins


def rj_table_subset(entries):
    """the entries of the CPU tier's stated subset (subset_digits)"""
    keep = {"rj-table gen %d w %d d %d" % (g, w, d) for g in (0, 1) for w in range(WINDOWS)
            for d in subset_digits(w, rj_top_digit(w))}
    return [e for e in entries if e.name in keep]


# ----------------------------------------------------------------------------- A. G_v through zg_sapling_bvk
def bvk_expect(spends, outputs, value):
    """(status, bvk bytes) of one zg_sapling_bvk row from S.binding_verification_key: 1 a cv does not
    decode (checked first), 2 the value balance is INT64_MIN; a failing row returns 32 zero bytes"""
    try:
        k = S.binding_verification_key(spends, outputs, value)
    except S.PointError:
        return 1, bytes(32)
    if k is None:
        return 2, bytes(32)
    return 0, S.encode(k)


@functools.lru_cache(maxsize=None)
def gv_table_rows():
    """rows without cvs and value balance +-(d << 8w): bvk = -[v] G_v = encode(-value_balance_point(v)),
    one lookup in the G_v table. Windows 8..31 of that table (and w = 7, d >= 128) cannot be reached:
    the ABI's value balance is an int64."""
    rows = []
    for (w, d), p in jj_comb(2).items():
        if d > gv_top_digit(w):
            continue
        zi = pow(p[2], -1, S.R)
        x, y = p[0] * zi % S.R, p[1] * zi % S.R
        v = d << (8 * w)
        rows.append(BvkRow("G_v w %d d %d sign +" % (w, d), (), (), v, 0, jj_encode_affine((-x) % S.R, y)))
        rows.append(BvkRow("G_v w %d d %d sign -" % (w, d), (), (), -v, 0, jj_encode_affine(x, y)))
    return rows


def gv_table_subset(rows):
    keep = {"G_v w %d d %d sign %s" % (w, d, sg) for w in range(GV_TOP_W + 1)
            for d in subset_digits(w, gv_top_digit(w), GV_TOP_W) for sg in "+-"}
    return [r for r in rows if r.name in keep]


# ----------------------------------------------------------------------------- A. Ed25519 table
@functools.lru_cache(maxsize=None)
def ed_comb():
    return comb_points(ED.B, ED.add)


@functools.lru_cache(maxsize=None)
def ed25519_table_items():
    """(entries, twins, unreadable): A the identity, R = compress([S] B), S = d << 8w: [k](-A) = O. The
    224 digits of window 31 with a bit of 0xE0 set can never be looked up: ZG_ED_SIGNATURE_ENCODING."""
    rng = random.Random(0xed1)
    pts = ed_comb()
    enc = {k: ED.compress(p) for k, p in pts.items()}
    entries, twins, unreadable = [], [], []
    for (w, d), rbar in enc.items():
        s = (d << (8 * w)).to_bytes(32, "little")
        if d <= ed_top_digit(w):
            entries.append(EdItem("ed-table w %d d %d" % (w, d), ED_IDENTITY, rbar + s, rng.randbytes(32), ED.OK))
        else:
            unreadable.append(EdItem("ed-unreadable w %d d %d" % (w, d), ED_IDENTITY, rbar + s, rng.randbytes(32),
                                     ED.SIGNATURE_ENCODING))
    for w, d, d2 in twin_digits(0xed2, ed_top_digit):
        s = (d << (8 * w)).to_bytes(32, "little")
        twins.append(EdItem("ed-twin w %d d %d (R of d %d)" % (w, d, d2), ED_IDENTITY, enc[w, d2] + s,
                            rng.randbytes(32), ED.SIGNATURE))
    return entries, twins, unreadable


def ed_table_subset(entries):
    keep = {"ed-table w %d d %d" % (w, d) for w in range(WINDOWS) for d in subset_digits(w, ed_top_digit(w))}
    return [e for e in entries if e.name in keep]


# ----------------------------------------------------------------------------- A. ECDSA table
EC_KEY = 0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296 % EC.N
EC_NONCE = 0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5 % EC.N


def _ec_digit_signature(u1, k, t, r):
    """(s, z) with z / s = u1 and r / s = u2 = (t - u1) / k: [u1] G + [u2] [k] G = [t] G, whose x is r"""
    u2 = (t - u1) * pow(k, -1, EC.N) % EC.N
    assert u2 != 0                       # u1 == t: not for a one-digit u1 and this nonce
    s = r * pow(u2, -1, EC.N) % EC.N
    return s, u1 * s % EC.N


@functools.lru_cache(maxsize=None)
def ecdsa_table_items():
    """(entries, twins): one key Q = [k] G, one nonce point [t] G, r = its x mod n; per entry the (s,
    message) that make u1 = z / s the single digit d << 8w. Scalar arithmetic only. s is whatever it
    comes to: the kernel does not normalize it (the verdict does not depend on that). A twin is the
    signature of digit d2 with the message that makes u1 the digit d: the sum is [t + u1 - u1'] G."""
    q = EC.mul(EC_KEY, EC.G)
    r = EC.mul(EC_NONCE, EC.G)[0] % EC.N
    keys = (EC.pubkey_bytes(q, True), EC.pubkey_bytes(q, False))
    entries, twins, sig = [], [], {}
    for w in range(WINDOWS):
        for d in range(1, DIGITS + 1):
            s, z = _ec_digit_signature(d << (8 * w), EC_KEY, EC_NONCE, r)
            sig[w, d] = s
            entries.append(EcItem("ec-table w %d d %d" % (w, d), keys[len(entries) & 1], EC.der(r, s),
                                  z.to_bytes(32, "big"), EC.OK))
    for w, d, d2 in twin_digits(0xec2, lambda w: DIGITS, 2):     # two a window: 8,160 + 64 is no whole number of waves
        s = sig[w, d2]
        z = (d << (8 * w)) * s % EC.N
        twins.append(EcItem("ec-twin w %d d %d (signature of d %d)" % (w, d, d2), keys[w & 1], EC.der(r, s),
                            z.to_bytes(32, "big"), EC.SIGNATURE))
    return entries, twins


def ec_table_subset(entries):
    keep = {"ec-table w %d d %d" % (w, d) for w in range(WINDOWS) for d in subset_digits(w, DIGITS)}
    return [e for e in entries if e.name in keep]


# ----------------------------------------------------------------------------- B. RedJubjub named items
@functools.lru_cache(maxsize=None)
def torsion_generator():
    """(y, T): T = [r_J] P of order 8 for the first y = 0, 1, 2, ... that decodes to a P with such an image"""
    for y in range(256):
        try:
            p = S.read(y.to_bytes(32, "little"))
        except S.PointError:
            continue
        t = S.mul(p, S.RJ)
        if S.is_zero(S.mul(t, 8)) and not S.is_zero(S.mul(t, 4)):
            return y, t
    raise AssertionError("no point of order 8 below y = 256")


def _rj_sign_with_torsion(gen, sk, nonce, tag, r_torsion, vk_torsion):
    """vk = [sk] G + vk_torsion, R = [r] G + r_torsion, S = r + c sk: the equation leaves r_torsion +
    [c] vk_torsion, which [8] kills. The message is the first of tag || counter for which that rest is
    not the identity, so that the equation WITHOUT the cofactor rejects the item."""
    g = S.GENERATORS[gen]
    vk = S.encode(S.add(S.mul(g, sk), vk_torsion))
    rbar = S.encode(S.add(S.mul(g, nonce), r_torsion))
    for ctr in range(64):
        msg = (tag + b"/%d" % ctr).ljust(64, b".")
        c = S.h_star(rbar, msg)
        if not S.is_zero(S.add(r_torsion, S.mul(vk_torsion, c))):
            return vk, rbar + ((nonce + c * sk) % S.RJ).to_bytes(32, "little"), msg
    raise AssertionError("no message leaves torsion in the equation")


@functools.lru_cache(maxsize=None)
def redjubjub_named_items():
    """the accept-side and boundary items; `ok` is what the construction says, the CPU tier holds
    S.redjubjub_verify to it"""
    rng = random.Random(0xb0b)
    _, t = torsion_generator()
    items = []
    for gen in (S.GEN_SPEND_AUTH, S.GEN_BINDING):
        g = S.GENERATORS[gen]
        for k in (1, 2, 4):                                   # orders 8, 4, 2
            kt = S.mul(t, k)
            sk, nonce = rng.randrange(1, S.RJ), rng.randrange(1, S.RJ)
            vk, sig, msg = _rj_sign_with_torsion(gen, sk, nonce, b"torsion-R g%d k%d" % (gen, k), kt, S.ZERO)
            items.append(RJItem("torsion in R gen %d [%d]T" % (gen, k), vk, sig, msg, gen, True))
            sk, nonce = rng.randrange(1, S.RJ), rng.randrange(1, S.RJ)
            vk, sig, msg = _rj_sign_with_torsion(gen, sk, nonce, b"torsion-vk g%d k%d" % (gen, k), S.ZERO, kt)
            items.append(RJItem("torsion in vk gen %d [%d]T" % (gen, k), vk, sig, msg, gen, True))
        top = (S.RJ - 1).to_bytes(32, "little")
        minus_g, plus_g = S.encode(S.neg(g)), S.encode(g)
        items += [
            RJItem("all trivial gen %d" % gen, JJ_IDENTITY, JJ_IDENTITY + bytes(32), rng.randbytes(64), gen, True),
            RJItem("identity key S = r_J - 1 R = -G gen %d" % gen, JJ_IDENTITY, minus_g + top, rng.randbytes(64),
                   gen, True),
            RJItem("identity key S = r_J R = -G gen %d" % gen, JJ_IDENTITY, minus_g + S.RJ.to_bytes(32, "little"),
                   rng.randbytes(64), gen, False),
            RJItem("identity key S = r_J - 1 R = G gen %d" % gen, JJ_IDENTITY, plus_g + top, rng.randbytes(64),
                   gen, False),
        ]
        # an honest signature whose S is zero: R = [r] G, c = H*(R || M), the key [sk] G with sk = -r / c
        nonce, msg = rng.randrange(1, S.RJ), rng.randbytes(64)
        rbar = S.encode(S.mul(g, nonce))
        sk = (-nonce) * pow(S.h_star(rbar, msg), -1, S.RJ) % S.RJ
        items.append(RJItem("honest S = 0 gen %d" % gen, S.encode(S.mul(g, sk)), rbar + bytes(32), msg, gen, True))
    return items


GEN_BYTES = (2, 3, 0x80, 0x81, 0xfe, 0xff)


@functools.lru_cache(maxsize=None)
def redjubjub_gen_byte_items():
    """include/zg.h: ZG_GEN_BINDING selects the binding generator, every other byte the spend-auth one.
    Honest signatures under each generator, sent with each byte of GEN_BYTES (and with 0 and 1)."""
    rng = random.Random(0x9e9)
    items = []
    for made_for in (S.GEN_SPEND_AUTH, S.GEN_BINDING):
        sk, msg = rng.randrange(1, S.RJ), rng.randbytes(64)
        vk, sig = S.public_key(sk, made_for), S.redjubjub_sign(sk, msg, made_for, rng.randbytes(80))
        for b in (0, 1) + GEN_BYTES:
            items.append(RJItem("signed under gen %d, gen byte 0x%02x" % (made_for, b), vk, sig, msg, b,
                                oracle_gen(b) == made_for))
    return items


def fixture_rj_items():
    """(valid, rejected) RedJubjub items of tests/golden/sapling_sigs.json"""
    fx = load_golden("sapling_sigs.json")
    def item(i, s):
        return RJItem(s.get("name", "signed_batch[%d]" % i), bytes.fromhex(s["vk"]), bytes.fromhex(s["sig"]),
                      bytes.fromhex(s["msg"]), s["gen"], s["ok"])
    items = [item(i, s) for i, s in enumerate(fx["sigs"] + fx["signed_batch"])]
    return [i for i in items if i.ok], [i for i in items if not i.ok]


@functools.lru_cache(maxsize=None)
def redjubjub_size_batches():
    """n = 0, 1, 63, 64, 65, 129 from the valid fixtures; index 0 an item only the cofactor accepts, the
    last index a different rejected item at each size (at n = 1 the two are two batches)"""
    valid, rejected = fixture_rj_items()
    named = redjubjub_named_items()
    torsion = [i for i in named if i.name.startswith("torsion")]
    rejects = [i for i in named if not i.ok] + redjubjub_table_items()[1][:2] + rejected
    batches = [[], [torsion[0]]]
    for k, n in enumerate(SIZES):
        batch = [valid[(j + 5 * k) % len(valid)] for j in range(n)]
        batch[0] = torsion[k % len(torsion)]
        batch[-1] = rejects[k]
        batches.append(batch)
    assert len({b[-1].name for b in batches[2:]}) == len(SIZES)
    return batches


# ----------------------------------------------------------------------------- C. zg_sapling_bvk rows
def _undecodable(rng):
    while True:
        b = rng.randbytes(32)
        try:
            Z.jubjub_read(b)
        except Z.PointError:
            return b


@functools.lru_cache(maxsize=None)
def _cv_pool():
    """value commitments: the fixtures' and oracle-made ones [v] G_v + [r] G_r"""
    fx = load_golden("sapling_sigs.json")
    pool = [bytes.fromhex(c) for t in fx["txs"] for c in t["spend_cvs"] + t["output_cvs"]]
    rng = random.Random(0xc5)
    for _ in range(12):
        pool.append(S.encode(S.add(S.mul(S.VALUE_COMMITMENT_VALUE, rng.randrange(1, 1 << 40)),
                                   S.mul(S.VALUE_COMMITMENT_RANDOMNESS, rng.randrange(1, S.RJ)))))
    return pool


def _row(name, spends, outputs, value):
    st, bvk = bvk_expect(list(spends), list(outputs), value)
    return BvkRow(name, tuple(spends), tuple(outputs), value, st, bvk)


@functools.lru_cache(maxsize=None)
def bvk_batches():
    """per size of SIZES a list of rows with 0..5 cvs each. Fixed places (where the size has them):
      0..2   no spends / no outputs / neither        3  no cvs, v = 0 (the identity encoding)
      4      spends == outputs (-[v] G_v)             5  v = INT64_MIN + 1     6  v = INT64_MAX
      7      a small-order cv (the oracle adds it like any other)
      10,11  the LAST cv does not decode, then a good row     12,13  the FIRST cv does not decode, good row
      14,15  v = INT64_MIN (status 2), good row              16,17  both faults (status 1), good row
      62,63,64  failing, failing, good across the end of the first wave (sizes that have them)
      last   a failing row: another kind at each size
    Every expectation is S.binding_verification_key's."""
    pool = _cv_pool()
    _, t = torsion_generator()
    small = S.encode(t)
    out = []
    for k, n in enumerate(SIZES):
        rng = random.Random(0xb7c + n)
        bad = _undecodable(rng)

        def cvs(m):
            return [rng.choice(pool) for _ in range(m)]

        def good(name):
            total = rng.randrange(6)
            ns = rng.randrange(total + 1)
            v = rng.choice([rng.randrange(-(1 << 62), 1 << 62), rng.randrange(-1000, 1000),
                            rng.randrange(1 << 32, 1 << 33)])
            return _row(name, cvs(ns), cvs(total - ns), v)

        failing = [lambda: _row("last cv undecodable", cvs(2), cvs(2) + [bad], 77),
                   lambda: _row("INT64_MIN", cvs(1), cvs(1), INT64_MIN),
                   lambda: _row("first cv undecodable", [bad] + cvs(2), cvs(1), -5),
                   lambda: _row("only cv undecodable", [bad], [], 0),
                   lambda: _row("INT64_MIN without cvs", [], [], INT64_MIN)]
        rows = [good("row %d" % i) for i in range(n)]
        same = cvs(2)
        fixed = {0: _row("no spends", [], cvs(3), 1234567), 1: _row("no outputs", cvs(3), [], -7654321),
                 2: _row("no cvs", [], [], 1 << 40), 3: _row("no cvs, v = 0", [], [], 0),
                 4: _row("spends == outputs", same, same, 987654321987),
                 5: _row("v = INT64_MIN + 1", cvs(1), cvs(2), INT64_MIN + 1),
                 6: _row("v = INT64_MAX", cvs(2), cvs(1), INT64_MAX),
                 7: _row("small-order cv", [small] + cvs(1), cvs(1), 42),
                 10: failing[0](), 11: good("after last cv undecodable"),
                 12: failing[2](), 13: good("after first cv undecodable"),
                 14: failing[1](), 15: good("after INT64_MIN"),
                 16: _row("undecodable cv and INT64_MIN", cvs(1) + [bad], [], INT64_MIN), 17: good("after both"),
                 62: failing[3](), 63: failing[4](), 64: good("first row of the second wave")}
        for i, r in fixed.items():
            if i < n - 1:
                rows[i] = r
        rows[-1] = failing[k]()
        out.append(rows)
    return out


# ----------------------------------------------------------------------------- C. zg_jubjub_decode points
def decode_expect(b):
    """(status, x, y) of zg_jubjub_decode: Z.jubjub_read and Z.is_small_order; status 1 has zero coordinates"""
    try:
        x, y = Z.jubjub_read(b)
    except Z.PointError:
        return 1, 0, 0
    return (2 if Z.is_small_order((x, y)) else 0), x, y


@functools.lru_cache(maxsize=None)
def decode_special_points():
    """the 8 torsion points in both sign-bit forms, y at the ends of the field, y = 1 and r - 1 with bit 255"""
    _, t = torsion_generator()
    pts = []
    for k in range(8):
        v = int.from_bytes(S.encode(S.mul(t, k)), "little")
        pts += [v.to_bytes(32, "little"), (v ^ (1 << 255)).to_bytes(32, "little")]
    pts += [y.to_bytes(32, "little") for y in (0, 1, Z.R - 1, Z.R, Z.R + 1, (1 << 255) - 1)]
    pts += [(y | (1 << 255)).to_bytes(32, "little") for y in (1, Z.R - 1)]
    return pts


@functools.lru_cache(maxsize=None)
def decode_batches():
    """per size of SIZES (points, expectations): the special points first (rotated by size, so the
    single-lane call sees a torsion point of order 8), then value commitments and random bytes; the last
    index alternates an undecodable and a small-order point"""
    special = decode_special_points()
    rng = random.Random(0xdec)
    pool = special + _cv_pool() + [rng.randbytes(32) for _ in range(129)]
    out = []
    for k, n in enumerate(SIZES):
        pts = [pool[(j + 2 * (k + 1)) % len(pool)] for j in range(n)] if n < len(special) else pool[:n]
        if n > 1:
            pts[-1] = special[19] if k & 1 else special[2]       # y = r: invalid / T: small order
        out.append((pts, [decode_expect(p) for p in pts]))
    return out
