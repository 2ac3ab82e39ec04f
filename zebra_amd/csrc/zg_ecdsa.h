// zg_ecdsa.h -- secp256k1 ECDSA verification on gfx950: the signature check
// behind OP_CHECKSIG / OP_CHECKMULTISIG of a transparent input, batched on the GPU, one lane per
// signature.
//
//   TransactionEval::check                          verification/src/accept_transaction.rs:363-422
//   -> verify_script -> check_signature             script/src/interpreter.rs:12-31
//   -> TransactionSignatureChecker::verify_signature script/src/verify.rs:60-67
//   -> keys::Public::verify                         keys/src/public.rs:38-49
//   -> eth-secp256k1, a libsecp256k1 binding (keys/Cargo.toml:11; not vendored: restated in
//      tests/ecdsa_ref.py, which the reference's key-pair vectors and legacy-sighash transactions pin
//      on the accept path; the edge rules below are restated from libsecp256k1 as written)
//
// Per item pubkey[len], sig[sig_len] (DER, no hashtype byte), msg[32] -> status ZG_ECDSA_*; the first
// failing check is the status:
//   1. Public::from_slice + PublicKey::from_slice (secp256k1_eckey_pubkey_parse): len 33 with prefix
//      02/03: x < p, y = sqrt(x^3 + 7) with the prefix's parity, no root fails; len 65 with prefix
//      04/06/07: x < p, y < p, on the curve, for 06/07 the parity of y = the prefix's low bit;
//      anything else is ZG_ECDSA_PUBLIC
//   2. Signature::from_der_lax (contrib/lax_der_parsing.c): 0x30; a sequence length byte whose
//      long-form length bytes are skipped and whose value is ignored; for R then S: tag 0x02, a short
//      length or a long-form one (leading zero length bytes skipped, then fewer than 8 bytes) that fits
//      in what remains, leading zero bytes of the integer skipped, no sign check; bytes after S are
//      ignored; a parse failure is ZG_ECDSA_SIGNATURE_ENCODING. More than 32 significant bytes or a
//      value >= n in either integer sets r = s = 0 (not a parse failure)
//   3. normalize_s, Message::from_slice (any 32 bytes, taken mod n), verify: r = 0 or s = 0 fails;
//      R' = (m / s) G + (r / s) Q, infinity fails; ok iff x(R') = r, or r + n < p and x(R') = r + n;
//      a failure is ZG_ECDSA_SIGNATURE. normalize_s replaces s by n - s when s > n / 2: that negates
//      R' and keeps x(R'), so the verdict does not depend on it and the kernel does not do it
//
// Field p = 2^256 - 2^32 - 977: the 9 x 29-bit digit field of zg_fd9.h (the fold is 2^261 = 2^37 +
// 31264); sf_mul21 here takes a tight operand only.
// Scalars mod n = 2^256 - c, c < 2^129: 8 saturated 32-bit words, any value below 2^256 in, the
// canonical value out. A 512-bit product is folded three times with 2^256 = c (mod n), every carry
// kept (n leaves no headroom in 256 bits: the generic Fp<M> add would drop the carry). One Fermat
// inversion per lane; the values are public.
// Points: homogeneous projective (X : Y : Z), infinity = (0 : 1 : 0), the complete formulas of
// Renes-Costello-Batina 2016 for a = 0 (algorithms 7 and 9, b3 = 21): secp256k1 has prime order, so
// they are correct for every pair of inputs -- P + P, P + (-P), infinity as an operand or the result.
#pragma once
#include "zg_fd9.h"

namespace zg {

#define ZG_EC_COMB_W 32
#define ZG_EC_COMB_D 255
#define ZG_EC_COMB_WORDS 18  // x, y: 9 digits each
#define ZG_EC_COMB_POINTS (ZG_EC_COMB_W * ZG_EC_COMB_D)

struct EcFM {  // 2^256 - 2^32 - 977
  static constexpr int BITS = 256, C1SH = 32;
  static constexpr uint32_t C0 = 977;
};
using Sf = Fd9<EcFM>;
static constexpr uint32_t EC_P[8] = {0xfffffc2fu, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
static constexpr uint32_t EC_N[8] = {0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
static constexpr uint32_t EC_NM2[8] = {0xd036413fu, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu};  // n - 2
static constexpr uint32_t EC_C[5] = {0x2fc9bebfu, 0x402da173u, 0x50b75fc4u, 0x45512319u, 0x00000001u};  // 2^256 - n
static constexpr uint32_t EC_PMN[8] = {0x2fc9baeeu, 0x402da172u, 0x50b75fc4u, 0x45512319u, 0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u};  // p - n
static constexpr uint32_t EC_GX[8] = {0x16f81798u, 0x59f2815bu, 0x2dce28d9u, 0x029bfcdbu, 0xce870b07u, 0x55a06295u, 0xf9dcbbacu, 0x79be667eu};
static constexpr uint32_t EC_GY[8] = {0xfb10d4b8u, 0x9c47d08fu, 0xa6855419u, 0xfd17b448u, 0x0e1108a8u, 0x5da4fbfcu, 0x26a3c465u, 0x483ada77u};

// 21 a (b3 = 3 * 7 of the point formulas), a tight
ZG_INL Sf sf_mul21(const Sf& a) {
  uint32_t f = 21u;
  zg_opaque(f);
  Sf r;
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    c = fd_mad(a.d[k], f, c);
    r.d[k] = (uint32_t)c & Sf::MASK;
    c >>= 29;
  }
  r.fold_in((uint32_t)c);  // < 32
  return r;
}

// z^(2^223 - 1) 2^23 z^(2^22 - 1), the common head of the square root and the inverse; *x2 = z^3
ZG_INL Sf sf_pow_head(const Sf& z, Sf* x2) {
  *x2 = fd_mul(fd_sqr(z), z);
  const Sf x3 = fd_mul(fd_sqr(*x2), z);
  const Sf x6 = fd_mul(fd_sqr_n(x3, 3), x3);
  const Sf x9 = fd_mul(fd_sqr_n(x6, 3), x3);
  const Sf x11 = fd_mul(fd_sqr_n(x9, 2), *x2);
  const Sf x22 = fd_mul(fd_sqr_n(x11, 11), x11);
  const Sf x44 = fd_mul(fd_sqr_n(x22, 22), x22);
  const Sf x88 = fd_mul(fd_sqr_n(x44, 44), x44);
  const Sf x176 = fd_mul(fd_sqr_n(x88, 88), x88);
  const Sf x220 = fd_mul(fd_sqr_n(x176, 44), x44);
  const Sf x223 = fd_mul(fd_sqr_n(x220, 3), x3);
  return fd_mul(fd_sqr_n(x223, 23), x22);
}
ZG_INL Sf sf_inv(const Sf& z) {  // z^(p - 2)
  Sf x2;
  Sf t = sf_pow_head(z, &x2);
  t = fd_mul(fd_sqr_n(t, 5), z);
  t = fd_mul(fd_sqr_n(t, 3), x2);
  return fd_mul(fd_sqr_n(t, 2), z);
}
ZG_INL Sf sf_sqrt_candidate(const Sf& z) {  // z^((p + 1) / 4): a root iff z is a square
  Sf x2;
  const Sf t = sf_pow_head(z, &x2);
  return fd_sqr_n(fd_mul(fd_sqr_n(t, 6), x2), 2);
}

// ---- 256-bit words
ZG_INL bool ec_words_lt(const uint32_t* a, const uint32_t* b) {  // a < b
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)a[i] - b[i] - borrow;
    borrow = (uint32_t)(t >> 63);
  }
  return borrow != 0;
}
ZG_INL bool ec_words_zero(const uint32_t* a) {
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) acc |= a[i];
  return acc == 0;
}
// 32 big-endian bytes -> 8 LE words
ZG_INL void ec_load_be(const uint8_t* b, uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = b + 4 * (7 - i);
    w[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
  }
}

// ---- scalars mod n: 8 saturated words
// r[0 .. NA + NB) = a b
template <int NA, int NB>
ZG_INL void sc_mp_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {
#pragma unroll
  for (int i = 0; i < NA + NB; i++) r[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const uint64_t t = fd_mad(a[i], b[j], (uint64_t)r[i + j] + carry);
      r[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    r[i + NB] = (uint32_t)carry;
  }
}
// z (8 words) += k c; returns the carry out of 2^256
ZG_INL uint32_t sc_add_kc(uint32_t* z, uint32_t k, const uint32_t* c) {
  zg_opaque(k);
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = i < 5 ? fd_mad(k, c[i], (uint64_t)z[i] + carry) : (uint64_t)z[i] + carry;
    z[i] = (uint32_t)t;
    carry = t >> 32;
  }
  return (uint32_t)carry;
}
// a 512-bit integer (16 LE words) mod n, canonical
ZG_INL void sc_reduce512(const uint32_t* t, uint32_t* out) {
  uint32_t c[5];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    c[i] = EC_C[i];
    zg_opaque(c[i]);
  }
  // t = lo + hi 2^256 = lo + hi c: below 2^385 + 2^256, 13 words
  uint32_t u[13], v[13];
  sc_mp_mul<8, 5>(u, t + 8, c);
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 13; i++) {
    const uint64_t s = (uint64_t)u[i] + (i < 8 ? t[i] : 0u) + carry;
    v[i] = (uint32_t)s;
    carry = s >> 32;
  }
  // again: the 5 high words times c is below 2^258, the sum below 2^259: 9 words
  uint32_t u2[10], w[9];
  sc_mp_mul<5, 5>(u2, v + 8, c);
  carry = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const uint64_t s = (uint64_t)u2[i] + (i < 8 ? v[i] : 0u) + carry;
    w[i] = (uint32_t)s;
    carry = s >> 32;
  }
  // w[8] < 8: one more fold leaves at most one carry, whose fold cannot carry again
  if (sc_add_kc(w, w[8], c)) sc_add_kc(w, 1u, c);
  // w < 2^256 < 2 n: w >= n iff w + c carries, and then w + c - 2^256 = w - n
  uint32_t x[8];
#pragma unroll
  for (int i = 0; i < 8; i++) x[i] = w[i];
  const bool ge = sc_add_kc(x, 1u, c) != 0;
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = ge ? x[i] : w[i];
}
ZG_INL void sc_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {  // any a, b < 2^256
  uint32_t t[16];
  sc_mp_mul<8, 8>(t, a, b);
  sc_reduce512(t, r);
}
// a^(n - 2): the inverse of a mod n (a not 0 mod n). The exponent sits in a 256-bit shift register,
// so no array is indexed by a run-time value
ZG_INL void sc_inv(uint32_t* r, const uint32_t* a) {
  uint32_t e[8], acc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    e[i] = EC_NM2[i];
    acc[i] = i == 0 ? 1u : 0u;
  }
  for (int i = 0; i < 256; i++) {
    sc_mul(acc, acc, acc);
    if (e[7] >> 31) sc_mul(acc, acc, a);
#pragma unroll
    for (int j = 7; j > 0; j--) e[j] = (e[j] << 1) | (e[j - 1] >> 31);
    e[0] <<= 1;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = acc[i];
}

// ---- points
struct EcP {
  Sf X, Y, Z;  // x = X / Z, y = Y / Z; infinity = (0 : 1 : 0)
};
ZG_INL EcP ec_infinity() { return {Sf::zero(), Sf::small(1), Sf::zero()}; }
// Renes-Costello-Batina algorithm 7 (a = 0): complete
ZG_INL EcP ec_add(const EcP& p, const EcP& q) {
  Sf t0 = fd_mul(p.X, q.X), t1 = fd_mul(p.Y, q.Y), t2 = fd_mul(p.Z, q.Z);
  const Sf t3 = fd_sub(fd_mul(fd_add_nc(p.X, p.Y), fd_add_nc(q.X, q.Y)), fd_add(t0, t1));  // X1 Y2 + X2 Y1
  const Sf t4 = fd_sub(fd_mul(fd_add_nc(p.Y, p.Z), fd_add_nc(q.Y, q.Z)), fd_add(t1, t2));  // Y1 Z2 + Y2 Z1
  Sf y3 = fd_sub(fd_mul(fd_add_nc(p.X, p.Z), fd_add_nc(q.X, q.Z)), fd_add(t0, t2));        // X1 Z2 + X2 Z1
  t0 = fd_add(fd_add(t0, t0), t0);
  t2 = sf_mul21(t2);
  Sf z3 = fd_add(t1, t2);
  t1 = fd_sub(t1, t2);
  y3 = sf_mul21(y3);
  const Sf x3 = fd_sub(fd_mul(t3, t1), fd_mul(t4, y3));
  y3 = fd_add(fd_mul(y3, t0), fd_mul(t1, z3));
  z3 = fd_add(fd_mul(z3, t4), fd_mul(t0, t3));
  return {x3, y3, z3};
}
// algorithm 9 (a = 0): complete
ZG_INL EcP ec_dbl(const EcP& p) {
  Sf t0 = fd_sqr(p.Y);
  Sf z3 = fd_add(t0, t0);
  z3 = fd_add(z3, z3);
  z3 = fd_add(z3, z3);
  const Sf t1 = fd_mul(p.Y, p.Z);
  Sf t2 = sf_mul21(fd_sqr(p.Z));
  const Sf x3 = fd_mul(t2, z3);
  Sf y3 = fd_add(t0, t2);
  z3 = fd_mul(t1, z3);
  t2 = fd_add(fd_add(t2, t2), t2);
  t0 = fd_sub(t0, t2);
  y3 = fd_add(fd_mul(t0, y3), x3);
  const Sf xy = fd_mul(t0, fd_mul(p.X, p.Y));
  return {fd_add(xy, xy), y3, z3};
}
// [k] p for the low nbits of k (8 LE words), the scalar in a shift register
ZG_INL EcP ec_mul(const EcP& p, const uint32_t* k, int nbits) {
  uint32_t e[8];
#pragma unroll
  for (int i = 0; i < 8; i++) e[i] = k[i];
  for (int i = nbits; i < 256; i++) {
#pragma unroll
    for (int j = 7; j > 0; j--) e[j] = (e[j] << 1) | (e[j - 1] >> 31);
    e[0] <<= 1;
  }
  EcP acc = ec_infinity();
  for (int i = 0; i < nbits; i++) {
    acc = ec_dbl(acc);
    if (e[7] >> 31) acc = ec_add(acc, p);
#pragma unroll
    for (int j = 7; j > 0; j--) e[j] = (e[j] << 1) | (e[j - 1] >> 31);
    e[0] <<= 1;
  }
  return acc;
}
// acc + [s] G for any 256-bit s (LE words): 32 byte-digit lookups in the comb table
ZG_INL EcP ec_add_fixed(EcP acc, const uint32_t* comb, const uint32_t* s) {
  uint32_t e[8];
#pragma unroll
  for (int i = 0; i < 8; i++) e[i] = s[i];
  for (int w = 0; w < ZG_EC_COMB_W; w++) {
    const int dg = e[0] & 0xff;
#pragma unroll
    for (int j = 0; j < 7; j++) e[j] = (e[j] >> 8) | (e[j + 1] << 24);
    e[7] >>= 8;
    if (!dg) continue;
    const uint32_t* t = comb + ((size_t)w * ZG_EC_COMB_D + (dg - 1)) * ZG_EC_COMB_WORDS;
    EcP q;
#pragma unroll
    for (int l = 0; l < 9; l++) {
      q.X.d[l] = t[l];
      q.Y.d[l] = t[9 + l];
    }
    q.Z = Sf::small(1);
    acc = ec_add(acc, q);
  }
  return acc;
}

// Public::from_slice + PublicKey::from_slice -> the affine point; false = ZG_ECDSA_PUBLIC. Bytes past
// len are not read, and none at all for a length other than 33 or 65
ZG_INL bool ec_parse_pubkey(const uint8_t* pk, int len, EcP* out) {
  if (len != 33 && len != 65) return false;
  const uint32_t pre = pk[0];
  if (len == 33 ? (pre != 2 && pre != 3) : (pre != 4 && pre != 6 && pre != 7)) return false;
  uint32_t p[8], xw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = EC_P[i];
  ec_load_be(pk + 1, xw);
  if (!ec_words_lt(xw, p)) return false;
  const Sf x = Sf::from_words(xw);
  const Sf rhs = fd_add(fd_mul(fd_sqr(x), x), Sf::small(7));
  Sf y;
  if (len == 33) {
    y = sf_sqrt_candidate(rhs);
    if (!fd_eq(fd_sqr(y), rhs)) return false;
    uint32_t yc[8];
    fd_canon(y, yc);
    if ((yc[0] & 1u) != (pre & 1u)) y = fd_neg(y);
  } else {
    uint32_t yw[8];
    ec_load_be(pk + 33, yw);
    if (!ec_words_lt(yw, p)) return false;
    if (pre != 4 && (yw[0] & 1u) != (pre & 1u)) return false;
    y = Sf::from_words(yw);
    if (!fd_eq(fd_sqr(y), rhs)) return false;
  }
  *out = {x, y, Sf::small(1)};
  return true;
}

// one INTEGER of Signature::from_der_lax at sig[*pos .. n): false = parse failure; else v = its value
// (8 LE words) and *overflow is set when it has more than 32 significant bytes. No byte at or past n
// is read, whatever the length bytes claim
ZG_INL bool ec_der_integer(const uint8_t* sig, uint32_t n, uint32_t* pos, uint32_t* v, bool* overflow) {
  uint32_t o = *pos;
  if (o == n || sig[o] != 0x02) return false;
  o++;
  if (o == n) return false;
  uint32_t lb = sig[o++], len;
  if (lb & 0x80) {
    lb -= 0x80;
    if (lb > n - o) return false;
    while (lb > 0 && sig[o] == 0) {
      o++;
      lb--;
    }
    if (lb >= 8) return false;
    uint64_t l64 = 0;
    while (lb > 0) {
      l64 = (l64 << 8) + sig[o];
      o++;
      lb--;
    }
    if (l64 > (uint64_t)(n - o)) return false;
    len = (uint32_t)l64;
  } else {
    len = lb;
    if (len > n - o) return false;
  }
  *pos = o + len;
  while (len > 0 && sig[o] == 0) {
    o++;
    len--;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = 0;
  if (len > 32) {
    *overflow = true;
    return true;
  }
#pragma unroll
  for (int j = 0; j < 32; j++) {  // byte j from the end; every index into v is a compile-time constant
    const uint32_t b = (uint32_t)j < len ? sig[o + len - 1 - j] : 0u;
    v[j >> 2] |= b << (8 * (j & 3));
  }
  return true;
}
// Signature::from_der_lax -> r, s (both 0 after an overflow); false = ZG_ECDSA_SIGNATURE_ENCODING
ZG_INL bool ec_parse_der_lax(const uint8_t* sig, uint32_t n, uint32_t* r, uint32_t* s) {
  uint32_t pos = 0;
  if (pos == n || sig[pos] != 0x30) return false;
  pos++;
  if (pos == n) return false;
  uint32_t lb = sig[pos++];
  if (lb & 0x80) {
    lb -= 0x80;
    if (lb > n - pos) return false;
    pos += lb;
  }
  bool overflow = false;
  if (!ec_der_integer(sig, n, &pos, r, &overflow)) return false;
  if (!ec_der_integer(sig, n, &pos, s, &overflow)) return false;
  uint32_t nn[8];
#pragma unroll
  for (int i = 0; i < 8; i++) nn[i] = EC_N[i];
  if (overflow || !ec_words_lt(r, nn) || !ec_words_lt(s, nn)) {
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = s[i] = 0;
  }
  return true;
}

// the whole check of one item -> ZG_ECDSA_* (0 ok, 1 public key, 2 signature encoding, 3 signature)
ZG_INL uint8_t ecdsa_verify_one(const uint8_t* pubkey, int pubkey_len, const uint8_t* sig, uint32_t sig_len,
                                const uint8_t* msg, const uint32_t* comb) {
  EcP Q;
  if (!ec_parse_pubkey(pubkey, pubkey_len, &Q)) return 1;
  uint32_t r[8], s[8];
  if (!ec_parse_der_lax(sig, sig_len, r, s)) return 2;
  if (ec_words_zero(r) || ec_words_zero(s)) return 3;
  uint32_t m[8], si[8], u1[8], u2[8];
  ec_load_be(msg, m);
  sc_inv(si, s);
  sc_mul(u1, m, si);  // any m below 2^256: the product is taken mod n
  sc_mul(u2, r, si);
  EcP R = ec_mul(Q, u2, 256);
  R = ec_add_fixed(R, comb, u1);
  if (fd_is_zero(R.Z)) return 3;
  // x(R') = X / Z: compare X with r Z, and with (r + n) Z when r + n < p
  if (fd_eq(R.X, fd_mul(Sf::from_words(r), R.Z))) return 0;
  uint32_t pmn[8];
#pragma unroll
  for (int i = 0; i < 8; i++) pmn[i] = EC_PMN[i];
  if (!ec_words_lt(r, pmn)) return 3;
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)r[i] + EC_N[i] + carry;
    r[i] = (uint32_t)t;
    carry = t >> 32;
  }
  return fd_eq(R.X, fd_mul(Sf::from_words(r), R.Z)) ? 0 : 3;
}

// comb table entry t: (d + 1) 2^(8 w) G as affine (x, y), canonical digits
ZG_INL void ec_comb_entry(int t, uint32_t* e) {
  const int d = t % ZG_EC_COMB_D + 1, w = t / ZG_EC_COMB_D;
  uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = (i == (w >> 2)) ? (uint32_t)d << (8 * (w & 3)) : 0u;
  uint32_t g[8];
#pragma unroll
  for (int i = 0; i < 8; i++) g[i] = EC_GX[i];
  const Sf gx = Sf::from_words(g);
#pragma unroll
  for (int i = 0; i < 8; i++) g[i] = EC_GY[i];
  const Sf gy = Sf::from_words(g);
  const EcP p = ec_mul({gx, gy, Sf::small(1)}, k, 8 * w + 8);
  const Sf zi = sf_inv(p.Z);
  uint32_t c[8];
  fd_canon(fd_mul(p.X, zi), c);
  const Sf x = Sf::from_words(c);
  fd_canon(fd_mul(p.Y, zi), c);
  const Sf y = Sf::from_words(c);
  for (int l = 0; l < 9; l++) {
    e[l] = x.d[l];
    e[9 + l] = y.d[l];
  }
}

// debug entries (zg_debug_field_mul fields 7 and 8), 8-word operands of any value and canonical result
ZG_INL void ec_debug_sf_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  fd_canon(fd_mul(Sf::from_words(a), Sf::from_words(b)), r);
}
ZG_INL void ec_debug_sc_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) { sc_mul(r, a, b); }

}  // namespace zg
