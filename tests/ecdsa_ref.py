"""Big-integer restatement of the secp256k1 ECDSA check behind OP_CHECKSIG.

  TransactionSignatureChecker::verify_signature   script/src/verify.rs:60-67
  -> keys::Public::verify                          keys/src/public.rs:38-49
  -> eth-secp256k1 (a libsecp256k1 binding, keys/Cargo.toml:11; not vendored): PublicKey::from_slice,
     Signature::from_der_lax, normalize_s, Message::from_slice, verify

The reference's own vectors pin the accept path (keys/src/keypair.rs:96-105,173-181 and the
legacy-sighash transactions of script/src/interpreter.rs:1817-1907); the edge rules are restated
from libsecp256k1 as written (secp256k1_eckey_pubkey_parse, contrib/lax_der_parsing.c,
secp256k1_ecdsa_sig_verify). verify() returns the status of zg_ecdsa_verify: the first failing
check of parse_pubkey, parse_der_lax, the curve equation.
"""
import hashlib
import hmac

OK, PUBLIC, SIGNATURE_ENCODING, SIGNATURE = 0, 1, 2, 3

P = 2 ** 256 - 2 ** 32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)
INF = (0, 1, 0)   # Jacobian, Z = 0


def dhash256(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


# ------------------------------------------------------------------ the group (Jacobian, every exceptional case explicit)
def jac(pt):
    return INF if pt is None else (pt[0], pt[1], 1)


def affine(pj):
    """-> (x, y), or None for infinity"""
    X, Y, Z = pj
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def jdbl(pj):
    X, Y, Z = pj
    if Z == 0 or Y == 0:
        return INF
    yy = Y * Y % P
    s = 4 * X * yy % P
    m = 3 * X * X % P
    x3 = (m * m - 2 * s) % P
    return x3, (m * (s - x3) - 8 * yy * yy) % P, 2 * Y * Z % P


def jadd(a, b):
    if a[2] == 0:
        return b
    if b[2] == 0:
        return a
    z1, z2 = a[2] * a[2] % P, b[2] * b[2] % P
    u1, u2 = a[0] * z2 % P, b[0] * z1 % P
    s1, s2 = a[1] * z2 * b[2] % P, b[1] * z1 * a[2] % P
    if u1 == u2:
        return jdbl(a) if s1 == s2 else INF
    h, r = (u2 - u1) % P, (s2 - s1) % P
    hh = h * h % P
    hhh, v = h * hh % P, u1 * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return x3, (r * (v - x3) - s1 * hhh) % P, h * a[2] * b[2] % P


def jmul(k, pj):
    acc = INF
    for i in range(k.bit_length() - 1, -1, -1):
        acc = jdbl(acc)
        if (k >> i) & 1:
            acc = jadd(acc, pj)
    return acc


def mul(k, pt):
    """[k] pt for an affine point (or None) -> affine point or None"""
    return affine(jmul(k % N, jac(pt)))


def add(a, b):
    return affine(jadd(jac(a), jac(b)))


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def mul2(u1, u2, q):
    """[u1] G + [u2] q (Shamir) -> Jacobian"""
    g, qj = jac(G), jac(q)
    both = jadd(g, qj)
    acc = INF
    for i in range(max(u1.bit_length(), u2.bit_length()) - 1, -1, -1):
        acc = jdbl(acc)
        sel = ((u1 >> i) & 1) | (((u2 >> i) & 1) << 1)
        if sel:
            acc = jadd(acc, (g, qj, both)[sel - 1])
    return acc


def on_curve(x, y):
    return (y * y - x * x * x - 7) % P == 0


def lift_x(x, odd):
    """the point with this x (< P) and parity, or None"""
    y = pow((x * x * x + 7) % P, (P + 1) // 4, P)
    if not on_curve(x, y):
        return None
    return x, (P - y if (y & 1) != odd else y)


# ------------------------------------------------------------------ encodings
def parse_pubkey(b):
    """Public::from_slice + PublicKey::from_slice (secp256k1_eckey_pubkey_parse) -> point or None"""
    if len(b) == 33 and b[0] in (2, 3):
        x = int.from_bytes(b[1:], "big")
        return lift_x(x, b[0] & 1) if x < P else None
    if len(b) == 65 and b[0] in (4, 6, 7):
        x, y = int.from_bytes(b[1:33], "big"), int.from_bytes(b[33:], "big")
        if x >= P or y >= P or not on_curve(x, y):
            return None
        if b[0] != 4 and (y & 1) != (b[0] & 1):
            return None
        return x, y
    return None


def pubkey_bytes(pt, compressed):
    if compressed:
        return bytes([2 | (pt[1] & 1)]) + pt[0].to_bytes(32, "big")
    return b"\x04" + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def parse_der_lax(b):
    """Signature::from_der_lax (contrib/lax_der_parsing.c) -> (r, s), or None for a parse failure;
    an integer of more than 32 significant bytes or >= N gives (0, 0), which is not a parse failure"""
    n, pos = len(b), 0
    if pos == n or b[pos] != 0x30:
        return None
    pos += 1
    if pos == n:
        return None
    lb = b[pos]
    pos += 1
    if lb & 0x80:
        lb -= 0x80
        if lb > n - pos:
            return None
        pos += lb
    vals = []
    for _ in range(2):
        if pos == n or b[pos] != 0x02:
            return None
        pos += 1
        if pos == n:
            return None
        lb = b[pos]
        pos += 1
        if lb & 0x80:
            lb -= 0x80
            if lb > n - pos:
                return None
            while lb > 0 and b[pos] == 0:
                pos += 1
                lb -= 1
            if lb >= 8:
                return None
            ln = 0
            while lb > 0:
                ln = (ln << 8) + b[pos]
                pos += 1
                lb -= 1
        else:
            ln = lb
        if ln > n - pos:
            return None
        vals.append(b[pos:pos + ln])
        pos += ln
    out, overflow = [], False
    for v in vals:
        v = v.lstrip(b"\x00")
        if len(v) > 32:
            overflow = True
        out.append(int.from_bytes(v, "big"))
    if overflow or out[0] >= N or out[1] >= N:
        return 0, 0
    return out[0], out[1]


def der(r, s):
    """strict DER of (r, s)"""
    def integer(v):
        b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
        if b[0] & 0x80:
            b = b"\x00" + b
        return b"\x02" + bytes([len(b)]) + b
    body = integer(r) + integer(s)
    return b"\x30" + bytes([len(body)]) + body


# ------------------------------------------------------------------ the check
def verify(pubkey, sig, msg):
    """-> status (OK, PUBLIC, SIGNATURE_ENCODING, SIGNATURE); msg: 32 bytes, big-endian"""
    q = parse_pubkey(bytes(pubkey))
    if q is None:
        return PUBLIC
    rs = parse_der_lax(bytes(sig))
    if rs is None:
        return SIGNATURE_ENCODING
    r, s = rs
    if s > N // 2:
        s = N - s   # normalize_s: the verdict does not depend on it (R' is negated, x(R') is kept)
    if r == 0 or s == 0:
        return SIGNATURE
    m = int.from_bytes(msg, "big") % N
    si = pow(s, -1, N)
    rp = affine(mul2(m * si % N, r * si % N, q))
    if rp is None:
        return SIGNATURE
    if rp[0] == r or (r + N < P and rp[0] == r + N):
        return OK
    return SIGNATURE


def rfc6979_nonce(d, msg):
    x, h1 = d.to_bytes(32, "big"), (int.from_bytes(msg, "big") % N).to_bytes(32, "big")
    v, k = b"\x01" * 32, b"\x00" * 32
    k = hmac.new(k, v + b"\x00" + x + h1, hashlib.sha256).digest()
    v = hmac.new(k, v, hashlib.sha256).digest()
    k = hmac.new(k, v + b"\x01" + x + h1, hashlib.sha256).digest()
    v = hmac.new(k, v, hashlib.sha256).digest()
    while True:
        v = hmac.new(k, v, hashlib.sha256).digest()
        t = int.from_bytes(v, "big")
        if 0 < t < N:
            return t
        k = hmac.new(k, v + b"\x00", hashlib.sha256).digest()
        v = hmac.new(k, v, hashlib.sha256).digest()


def sign(d, msg):
    """-> (r, s), low S, deterministic nonce (RFC 6979, HMAC-SHA256)"""
    k = rfc6979_nonce(d, msg)
    r = mul(k, G)[0] % N
    s = pow(k, -1, N) * (int.from_bytes(msg, "big") + r * d) % N
    assert r and s
    return r, min(s, N - s)


# ------------------------------------------------------------------ keys and the legacy sighash of the reference's vectors
_B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def wif_secret(s):
    """-> (secret, compressed) of a WIF private key (keys/src/private.rs)"""
    v = 0
    for c in s:
        v = v * 58 + _B58.index(c)
    raw = v.to_bytes(38 if len(s) == 52 else 37, "big")
    assert dhash256(raw[:-4])[:4] == raw[-4:] and raw[0] == 0x80
    body = raw[1:-4]
    return int.from_bytes(body[:32], "big"), len(body) == 33


def _compact(b, o):
    v = b[o]
    if v < 0xfd:
        return v, o + 1
    w = {0xfd: 2, 0xfe: 4, 0xff: 8}[v]
    return int.from_bytes(b[o + 1:o + 1 + w], "little"), o + 1 + w


def _put_compact(v):
    return bytes([v]) if v < 0xfd else b"\xfd" + v.to_bytes(2, "little")


def legacy_sighash_all(raw_tx, input_index, script_code):
    """signature_hash_sprout (script/src/sign.rs:179-246) for SIGHASH_ALL of a version-1 transaction"""
    o = 4
    n_in, o = _compact(raw_tx, o)
    out = raw_tx[:4] + _put_compact(n_in)
    for i in range(n_in):
        prev = raw_tx[o:o + 36]
        ln, o2 = _compact(raw_tx, o + 36)
        seq = raw_tx[o2 + ln:o2 + ln + 4]
        o = o2 + ln + 4
        sc = script_code if i == input_index else b""
        out += prev + _put_compact(len(sc)) + sc + seq
    return dhash256(out + raw_tx[o:] + (1).to_bytes(4, "little"))
