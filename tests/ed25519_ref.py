"""Big-int restatement of the Ed25519 check the reference runs on a JoinSplit signature.

  JoinSplitVerification::check   verification/src/accept_transaction.rs:649-653
  -> crypto::verify_ed25519      crypto/src/lib.rs:298-305
  -> ed25519-dalek 1.0.0-pre.1 over curve25519-dalek 1.1.4 and sha2 0.8.0

verify(pubkey, sig, msg) returns the status zg_ed25519_verify returns:
  0 ok, 1 PublicKey::from_bytes fails, 2 Signature::from_bytes fails, 3 verify fails;
the checks run in that order and the first failing one is the status.

How well this is pinned. The crates' sources are not vendored by the reference. The ACCEPT path is
pinned by the reference's own data: the three JoinSplit signatures of block 419221 over the
oracle's ZIP-243 no-input sighash verify here, and so does RFC 8032 TEST 1. Three EDGE rules are
restated from the crates' source as remembered, and no reference-held vector covers them:
  * S >= l is accepted while S < 2^253 (Signature::from_bytes only rejects sig[63] & 0xE0, and
    verify uses Scalar::from_bits);
  * a non-canonical y (y >= p in the low 255 bits) and the "-0" keys (x = 0 with bit 255 set) are
    accepted by CompressedEdwardsY::decompress; no small-order or identity rejection;
  * R is compared as bytes with compress(R'), so a non-canonical R never verifies.
They are deliberately NOT "fixed" towards RFC 8032 or libsodium behaviour.
"""
import hashlib

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)

OK, PUBLIC_ENCODING, SIGNATURE_ENCODING, SIGNATURE = 0, 1, 2, 3


def _recover_x(y, sign):
    """CompressedEdwardsY::decompress, step 1 and 2: y any integer (taken mod p); None = not a point"""
    y %= P
    u = (y * y - 1) % P
    v = (D * y * y + 1) % P
    v3 = v * v % P * v % P
    v7 = v3 * v3 % P * v % P
    x = u * v3 % P * pow(u * v7 % P, (P - 5) // 8, P) % P
    chk = v * x % P * x % P
    if chk == u:
        pass
    elif chk == (-u) % P:
        x = x * SQRT_M1 % P
    else:
        return None
    if x & 1:
        x = P - x
    if sign:
        x = (-x) % P  # also for x = 0
    return x


def decompress(b):
    """32 bytes -> extended point (X, Y, Z, T) or None; no y < p check"""
    n = int.from_bytes(b, "little")
    y = (n & ((1 << 255) - 1)) % P
    x = _recover_x(y, n >> 255)
    if x is None:
        return None
    return (x, y, 1, x * y % P)


def add(p, q):
    """add-2008-hwcd-3 (a = -1): complete, d is a non-square"""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = t1 * 2 * D * t2 % P
    d = z1 * 2 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def neg(p):
    return ((-p[0]) % P, p[1], p[2], (-p[3]) % P)


IDENTITY = (0, 1, 1, 0)


def mul(k, p):
    acc = IDENTITY
    while k:
        if k & 1:
            acc = add(acc, p)
        p = add(p, p)
        k >>= 1
    return acc


def compress(p):
    zi = pow(p[2], P - 2, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


BY = 4 * pow(5, P - 2, P) % P
B = (_recover_x(BY, 0), BY, 1, _recover_x(BY, 0) * BY % P)


def verify(pubkey, sig, msg):
    """status 0..3 as the reference classifies the item (msg: any length; the product passes 32 bytes)"""
    a = decompress(pubkey)
    if a is None:
        return PUBLIC_ENCODING
    if sig[63] & 0xE0:
        return SIGNATURE_ENCODING
    s = int.from_bytes(sig[32:], "little")  # Scalar::from_bits: not reduced, not required < l
    k = int.from_bytes(hashlib.sha512(sig[:32] + pubkey + msg).digest(), "little") % L
    r = add(mul(s, B), mul(k, neg(a)))
    return OK if compress(r) == sig[:32] else SIGNATURE


def public_key(seed):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a = (a & ((1 << 254) - 8)) | (1 << 254)
    return compress(mul(a, B))


def sign(seed, msg):
    """RFC 8032 section 5.1.6"""
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a = (a & ((1 << 254) - 8)) | (1 << 254)
    pk = compress(mul(a, B))
    r = int.from_bytes(hashlib.sha512(h[32:] + msg).digest(), "little") % L
    rb = compress(mul(r, B))
    k = int.from_bytes(hashlib.sha512(rb + pk + msg).digest(), "little") % L
    return rb + ((r + k * a) % L).to_bytes(32, "little")


def joinsplit_sig_from_raw(raw, has_binding_sig):
    """the JoinSplit signature of a serialized v4 transaction: the 64 bytes before binding_sig, or
    the last 64 bytes when there is none (oracle/sapling_sig.parse_tx_raw drops it)"""
    return raw[-128:-64] if has_binding_sig else raw[-64:]


RFC8032_TEST1 = {
    "seed": "9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
    "pubkey": "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a",
    "msg": "",
    "sig": "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e06522490155"
           "5fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b",
}
