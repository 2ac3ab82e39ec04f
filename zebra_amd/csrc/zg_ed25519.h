// zg_ed25519.h -- Ed25519 verification on gfx950: the JoinSplit signature
// check of a Sprout-bearing transaction, batched on the GPU, one lane per signature.
//
//   JoinSplitVerification::check   verification/src/accept_transaction.rs:649-653
//   -> crypto::verify_ed25519      crypto/src/lib.rs:298-305
//   -> ed25519-dalek 1.0.0-pre.1 over curve25519-dalek 1.1.4 and sha2 0.8.0 (Cargo.lock:399,466,1559;
//      not vendored: restated in tests/ed25519_ref.py, which the reference's real transactions pin on
//      the accept path; the edge rules below are restated from the crates' source as remembered)
//
// Per item pubkey[32], sig[64] = R || S, msg[32] -> status ZG_ED_*; the first failing check is the status:
//   1. key decode (CompressedEdwardsY::decompress): y = low 255 bits mod p, NO y < p check;
//      u = y^2 - 1, v = d y^2 + 1, x = (u v^3)(u v^7)^((p-5)/8); v x^2 = u, or = -u (then x *= sqrt(-1)),
//      else ZG_ED_PUBLIC_ENCODING; the even root, negated if bit 255 is set (also for x = 0); no
//      small-order or identity rejection
//   2. signature decode: ZG_ED_SIGNATURE_ENCODING iff sig[63] & 0xE0; S is the 256-bit integer as
//      given (Scalar::from_bits: S >= l is accepted); R is not decoded
//   3. k = SHA-512(R || pubkey || msg) mod l (the 96 bytes as given: one block);
//      R' = [S]B + [k](-A), cofactorless; ZG_ED_OK iff compress(R') == the 32 bytes of R, else
//      ZG_ED_SIGNATURE (a non-canonical R never verifies)
//
// Field 2^255 - 19: 9 unsaturated digits of 29 bits. A product is 81 carry-free
// v_mad_u64_u32 into 17 columns; the digit string is 261 bits long, so the fold is 2^261 = 2^6 * 19 =
// 1216 (mod p): the high columns are carried to 29-bit digits, multiplied by 1216 into the low ones,
// and one more carry pass finishes. No digit is ever masked narrower than 29 bits and the small
// factors are hidden behind zg_opaque, so no multiply-add sees two operands it knows to fit 24 bits
// (the compiler finding of DESIGN.md section 4; zg_debug_field_mul field 5 is the guard).
//   "tight" element: every digit < 2^29 + 2^14 (what every function here returns);
//   products accept digits < 1.4e9 (9 x^2 + the folds stay below 2^64), i.e. also an uncarried sum
//   of two tight elements (fe_add_nc).
// Points: extended coordinates, a = -1 (add-2008-hwcd-3, dbl-2008-hwcd); d is a non-square, so the
// addition is complete for every input, small-order points included.
#pragma once
#include "zg_field.h"

namespace zg {

#define ZG_ED_COMB_W 32
#define ZG_ED_COMB_D 255
#define ZG_ED_COMB_WORDS 27  // y + x, y - x, 2 d x y: 9 digits each
#define ZG_ED_COMB_POINTS (ZG_ED_COMB_W * ZG_ED_COMB_D)

struct Fe {
  uint32_t d[9];
};
static constexpr uint32_t ED_MASK = 0x1fffffffu;
static constexpr uint32_t ED_D[9] = {0x135978a3u, 0x0f5a6e50u, 0x10762addu, 0x00149a82u, 0x1e898007u, 0x003cbbbcu, 0x19ce331du, 0x1dc56dffu, 0x0052036cu};  // -121665/121666
static constexpr uint32_t ED_2D[9] = {0x06b2f159u, 0x1eb4dca1u, 0x00ec55bau, 0x00293505u, 0x1d13000eu, 0x00797779u, 0x139c663au, 0x1b8adbffu, 0x002406d9u};
static constexpr uint32_t ED_SQRTM1[9] = {0x0a0ea0b0u, 0x0770d93au, 0x0bf91e31u, 0x06300d5au, 0x1d7a72f4u, 0x004c9efdu, 0x1c2cad34u, 0x1009f83bu, 0x002b8324u};
static constexpr uint32_t ED_BX[9] = {0x0f25d51au, 0x0ab16b04u, 0x0969ecb2u, 0x198ec12au, 0x0dc5c692u, 0x1118feebu, 0x0ffb0293u, 0x1a79adcau, 0x00216936u};
static constexpr uint32_t ED_BY[9] = {0x06666658u, 0x13333333u, 0x19999999u, 0x0cccccccu, 0x06666666u, 0x13333333u, 0x19999999u, 0x0cccccccu, 0x00666666u};  // 4/5
// the group order l = 2^252 + 27742317777372353535851937790883648493 and its Montgomery constants
static constexpr uint32_t ED_L[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0x00000000u, 0x00000000u, 0x00000000u, 0x10000000u};
static constexpr uint32_t ED_L_INV = 0x12547e1bu;  // -l^-1 mod 2^32
static constexpr uint32_t ED_L_C252[8] = {0x5432c2a3u, 0xd6cd0540u, 0x86929507u, 0x6b5a2d83u, 0x217f5be6u, 0xdceec73du, 0xb7c309a3u, 0x0b399411u};  // 2^252 2^256 mod l
static constexpr uint32_t ED_L_C504[8] = {0xfb8f8555u, 0xdac469f6u, 0xa4992644u, 0x6731498bu, 0x6c04ec5bu, 0xc78065dcu, 0x773599ceu, 0x019e530bu};  // 2^504 2^256 mod l

struct EdLM {
  static constexpr int N = 8;
  static constexpr uint32_t INV = ED_L_INV;
  ZG_INL static uint32_t p(int i) { return ED_L[i]; }
};
using EdS = Fp<EdLM>;

ZG_INL uint64_t ed_mad(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }

ZG_INL Fe fe_const(const uint32_t* c) {
  Fe r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.d[i] = c[i];
  return r;
}
ZG_INL Fe fe_zero() {
  Fe r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.d[i] = 0;
  return r;
}
ZG_INL Fe fe_one() {
  Fe r = fe_zero();
  r.d[0] = 1;
  return r;
}

// one carry pass with the 2^261 = 1216 fold: digits < 2^31 in -> tight out (the value is unchanged mod p)
ZG_INL void fe_carry(Fe& r) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    r.d[k + 1] += r.d[k] >> 29;
    r.d[k] &= ED_MASK;
  }
  const uint32_t t = r.d[8] >> 29;
  r.d[8] &= ED_MASK;
  r.d[0] += t * 1216u;
}
ZG_INL Fe fe_add_nc(const Fe& a, const Fe& b) {  // a product operand only
  Fe r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.d[i] = a.d[i] + b.d[i];
  return r;
}
ZG_INL Fe fe_add(const Fe& a, const Fe& b) {
  Fe r = fe_add_nc(a, b);
  fe_carry(r);
  return r;
}
// a - b: a + 2 (2^261 - 1216) - b digit by digit (every digit of the offset >= a tight digit)
ZG_INL Fe fe_sub(const Fe& a, const Fe& b) {
  Fe r;
  r.d[0] = a.d[0] + (0x40000000u - 2432u) - b.d[0];
#pragma unroll
  for (int i = 1; i < 9; i++) r.d[i] = a.d[i] + 0x3ffffffeu - b.d[i];
  fe_carry(r);
  return r;
}
ZG_INL Fe fe_neg(const Fe& a) { return fe_sub(fe_zero(), a); }

// 17 columns (each < 2^64 - 2^47) -> tight element
ZG_INL Fe fe_fold(uint64_t* c) {
  uint32_t h[9];
#pragma unroll
  for (int k = 9; k < 16; k++) {
    h[k - 9] = (uint32_t)c[k] & ED_MASK;
    c[k + 1] += c[k] >> 29;
  }
  h[7] = (uint32_t)c[16] & ED_MASK;
  h[8] = (uint32_t)(c[16] >> 29);  // < 2^32 by the operand bound
  uint32_t f = 1216u;
  zg_opaque(f);
#pragma unroll
  for (int k = 0; k < 9; k++) c[k] = ed_mad(h[k], f, c[k]);
  Fe r;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    r.d[k] = (uint32_t)c[k] & ED_MASK;
    c[k + 1] += c[k] >> 29;
  }
  r.d[8] = (uint32_t)c[8] & ED_MASK;
  const uint64_t t = c[8] >> 29;  // < 2^35: folds into digits 0 and 1
  uint32_t tl = (uint32_t)t & ED_MASK, th = (uint32_t)(t >> 29);
  zg_opaque(th);
  const uint64_t c0 = ed_mad(tl, f, r.d[0]);
  const uint64_t c1 = ed_mad(th, f, (uint64_t)r.d[1] + (c0 >> 29));
  r.d[0] = (uint32_t)c0 & ED_MASK;
  r.d[1] = (uint32_t)c1 & ED_MASK;
  r.d[2] += (uint32_t)(c1 >> 29);
  return r;
}

ZG_INL Fe fe_mul(const Fe& a, const Fe& b) {
  uint64_t c[17];
#pragma unroll
  for (int k = 0; k < 17; k++) {
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int j = k - i;
      if (j < 0 || j > 8) continue;
      s = ed_mad(a.d[i], b.d[j], s);
    }
    c[k] = s;
  }
  return fe_fold(c);
}
ZG_INL Fe fe_sqr(const Fe& a) {
  uint32_t a2[9];
#pragma unroll
  for (int i = 0; i < 9; i++) a2[i] = a.d[i] << 1;
  uint64_t c[17];
#pragma unroll
  for (int k = 0; k < 17; k++) {
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int j = k - i;
      if (j < 0 || j > 8 || i > j) continue;
      s = ed_mad(i < j ? a2[i] : a.d[i], a.d[j], s);
    }
    c[k] = s;
  }
  return fe_fold(c);
}
ZG_INL Fe fe_sqr_n(Fe a, int n) {
  for (int i = 0; i < n; i++) a = fe_sqr(a);
  return a;
}

// a 256-bit integer (8 LE words, any value) -> digits (tight: the top digit has 24 bits)
ZG_INL Fe fe_from_words(const uint32_t* w) {
  Fe r;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int bit = 29 * k, wi = bit >> 5, sh = bit & 31;
    uint32_t v = w[wi] >> sh;
    if (sh > 3 && wi + 1 < 8) v |= w[wi + 1] << (32 - sh);
    r.d[k] = v & ED_MASK;
  }
  return r;
}
// the canonical value (< p) as 8 LE words
ZG_INL void fe_canon(const Fe& a, uint32_t* w) {
  Fe t = a;
  fe_carry(t);
  fe_carry(t);  // every digit < 2^29: the value is < 2^261
  const uint32_t q = t.d[8] >> 23;
  t.d[8] &= 0x7fffffu;
  t.d[0] += 19u * q;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    t.d[k + 1] += t.d[k] >> 29;
    t.d[k] &= ED_MASK;
  }
  // t < 2^255 + 2^11: t >= p iff t + 19 reaches bit 255
  Fe u = t;
  u.d[0] += 19u;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    u.d[k + 1] += u.d[k] >> 29;
    u.d[k] &= ED_MASK;
  }
  const bool ge = (u.d[8] >> 23) != 0;
  u.d[8] &= 0x7fffffu;
  uint64_t acc = 0;
  int bits = 0, wi = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    acc |= (uint64_t)(ge ? u.d[k] : t.d[k]) << bits;
    bits += 29;
    if (bits >= 32) {
      w[wi++] = (uint32_t)acc;
      acc >>= 32;
      bits -= 32;
    }
  }
}
ZG_INL bool fe_eq(const Fe& a, const Fe& b) {
  uint32_t x[8], y[8], acc = 0;
  fe_canon(a, x);
  fe_canon(b, y);
#pragma unroll
  for (int i = 0; i < 8; i++) acc |= x[i] ^ y[i];
  return acc == 0;
}

// z^(2^250 - 1); *z11 = z^11
ZG_INL Fe fe_pow250(const Fe& z, Fe* z11) {
  const Fe z2 = fe_sqr(z);
  const Fe z9 = fe_mul(fe_sqr_n(z2, 2), z);
  *z11 = fe_mul(z9, z2);
  const Fe t5 = fe_mul(fe_sqr(*z11), z9);             // 2^5 - 1
  const Fe t10 = fe_mul(fe_sqr_n(t5, 5), t5);         // 2^10 - 1
  const Fe t20 = fe_mul(fe_sqr_n(t10, 10), t10);      // 2^20 - 1
  const Fe t40 = fe_mul(fe_sqr_n(t20, 20), t20);      // 2^40 - 1
  const Fe t50 = fe_mul(fe_sqr_n(t40, 10), t10);      // 2^50 - 1
  const Fe t100 = fe_mul(fe_sqr_n(t50, 50), t50);     // 2^100 - 1
  const Fe t200 = fe_mul(fe_sqr_n(t100, 100), t100);  // 2^200 - 1
  return fe_mul(fe_sqr_n(t200, 50), t50);             // 2^250 - 1
}
ZG_INL Fe fe_inv(const Fe& z) {  // z^(p - 2) = z^(2^255 - 21)
  Fe z11;
  const Fe t = fe_pow250(z, &z11);
  return fe_mul(fe_sqr_n(t, 5), z11);
}
ZG_INL Fe fe_pow22523(const Fe& z) {  // z^((p - 5) / 8) = z^(2^252 - 3)
  Fe z11;
  const Fe t = fe_pow250(z, &z11);
  return fe_mul(fe_sqr_n(t, 2), z);
}

// ---- points
struct EdP {
  Fe X, Y, Z, T;  // x = X / Z, y = Y / Z, x y = T / Z
};
struct EdCached {
  Fe YpX, YmX, Z2, T2d;  // Y + X, Y - X, 2 Z, 2 d T
};
ZG_INL EdP ed_identity() { return {fe_zero(), fe_one(), fe_one(), fe_zero()}; }
ZG_INL EdP ed_neg(const EdP& p) { return {fe_neg(p.X), p.Y, p.Z, fe_neg(p.T)}; }
ZG_INL EdCached ed_cache(const EdP& p) {
  return {fe_add(p.Y, p.X), fe_sub(p.Y, p.X), fe_add(p.Z, p.Z), fe_mul(p.T, fe_const(ED_2D))};
}
ZG_INL EdP ed_dbl(const EdP& p) {
  const Fe A = fe_sqr(p.X), B = fe_sqr(p.Y), Z2 = fe_sqr(p.Z);
  const Fe C = fe_add(Z2, Z2);
  const Fe S = fe_add(A, B);  // -H
  const Fe E = fe_sub(fe_sqr(fe_add_nc(p.X, p.Y)), S);
  const Fe G = fe_sub(B, A), F = fe_sub(G, C), H = fe_neg(S);
  return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}
ZG_INL EdP ed_add(const EdP& p, const EdCached& q) {
  const Fe A = fe_mul(fe_sub(p.Y, p.X), q.YmX);
  const Fe B = fe_mul(fe_add_nc(p.Y, p.X), q.YpX);
  const Fe C = fe_mul(p.T, q.T2d);
  const Fe D = fe_mul(p.Z, q.Z2);
  const Fe E = fe_sub(B, A), F = fe_sub(D, C), G = fe_add(D, C), H = fe_add(B, A);
  return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}
// q affine: (y + x, y - x, 2 d x y)
ZG_INL EdP ed_add_aff(const EdP& p, const Fe& ypx, const Fe& ymx, const Fe& xy2d) {
  const Fe A = fe_mul(fe_sub(p.Y, p.X), ymx);
  const Fe B = fe_mul(fe_add_nc(p.Y, p.X), ypx);
  const Fe C = fe_mul(p.T, xy2d);
  const Fe D = fe_add(p.Z, p.Z);
  const Fe E = fe_sub(B, A), F = fe_sub(D, C), G = fe_add(D, C), H = fe_add(B, A);
  return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}
// [k] p, k little-endian 32-bit limbs, nbits from the top
ZG_INL EdP ed_mul(const EdP& p, const uint32_t* k, int nbits) {
  const EdCached q = ed_cache(p);
  EdP acc = ed_identity();
  for (int i = nbits - 1; i >= 0; i--) {
    acc = ed_dbl(acc);
    if ((k[i >> 5] >> (i & 31)) & 1u) acc = ed_add(acc, q);
  }
  return acc;
}
// acc + [s] B for any 256-bit s (LE limbs): 32 byte-digit lookups in the comb table
ZG_INL EdP ed_add_fixed(EdP acc, const uint32_t* comb, const uint32_t* s) {
  for (int w = 0; w < ZG_ED_COMB_W; w++) {
    const int dg = (s[w >> 2] >> (8 * (w & 3))) & 0xff;
    if (!dg) continue;
    const uint32_t* e = comb + ((size_t)w * ZG_ED_COMB_D + (dg - 1)) * ZG_ED_COMB_WORDS;
    Fe ypx, ymx, xy2d;
#pragma unroll
    for (int l = 0; l < 9; l++) {
      ypx.d[l] = e[l];
      ymx.d[l] = e[9 + l];
      xy2d.d[l] = e[18 + l];
    }
    acc = ed_add_aff(acc, ypx, ymx, xy2d);
  }
  return acc;
}
// compress: canonical y (8 LE words) with the parity of canonical x in bit 255
ZG_INL void ed_compress(const EdP& p, uint32_t* out) {
  const Fe zi = fe_inv(p.Z);
  uint32_t x[8];
  fe_canon(fe_mul(p.X, zi), x);
  fe_canon(fe_mul(p.Y, zi), out);
  out[7] |= (x[0] & 1u) << 31;
}
// CompressedEdwardsY::decompress of 8 LE words; false = not a point
ZG_INL bool ed_decompress(const uint32_t* in, EdP* out) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = in[i];
  const bool sign = w[7] >> 31;
  w[7] &= 0x7fffffffu;
  const Fe y = fe_from_words(w);  // not required to be below p
  const Fe y2 = fe_sqr(y);
  const Fe u = fe_sub(y2, fe_one());
  const Fe v = fe_add(fe_mul(y2, fe_const(ED_D)), fe_one());
  const Fe v3 = fe_mul(fe_sqr(v), v);
  const Fe v7 = fe_mul(fe_sqr(v3), v);
  Fe x = fe_mul(fe_mul(u, v3), fe_pow22523(fe_mul(u, v7)));
  const Fe chk = fe_mul(v, fe_sqr(x));
  if (!fe_eq(chk, u)) {
    if (!fe_eq(chk, fe_neg(u))) return false;
    x = fe_mul(x, fe_const(ED_SQRTM1));
  }
  uint32_t xc[8];
  fe_canon(x, xc);
  if ((bool)(xc[0] & 1u) != sign) x = fe_neg(x);  // the even root, negated when the sign bit is set
  *out = {x, y, fe_one(), fe_mul(x, y)};
  return true;
}

// ---- SHA-512 of one 128-byte block (16 big-endian words, already padded)
#define ED_SHA512_K_VALUES \
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, \
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, \
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, \
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, \
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, \
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, \
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, \
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull, \
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull, \
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, \
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, \
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, \
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, \
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, \
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull, \
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, \
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, \
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull, \
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, \
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull
__device__ __constant__ const uint64_t ED_SHA512_K[80] = {ED_SHA512_K_VALUES};
#if defined(__HIP_DEVICE_COMPILE__)
#define ED_K(t) ED_SHA512_K[t]
#else
static const uint64_t ED_SHA512_K_HOST[80] = {ED_SHA512_K_VALUES};  // host pass (tests): no device symbol
#define ED_K(t) ED_SHA512_K_HOST[t]
#endif
ZG_INL uint64_t ed_rotr(uint64_t x, int k) { return (x >> k) | (x << (64 - k)); }
// w: the block, used as the rolling 16-word schedule (every index a compile-time constant); out: H0..H7
ZG_INL void ed_sha512_block(uint64_t* w, uint64_t* out) {
  uint64_t a = 0x6a09e667f3bcc908ull, b = 0xbb67ae8584caa73bull, c = 0x3c6ef372fe94f82bull,
           d = 0xa54ff53a5f1d36f1ull, e = 0x510e527fade682d1ull, f = 0x9b05688c2b3e6c1full,
           g = 0x1f83d9abfb41bd6bull, h = 0x5be0cd19137e2179ull;
#pragma unroll
  for (int t = 0; t < 80; t++) {
    if (t >= 16) {
      const uint64_t x = w[(t - 15) & 15], y = w[(t - 2) & 15];
      w[t & 15] += (ed_rotr(x, 1) ^ ed_rotr(x, 8) ^ (x >> 7)) + w[(t - 7) & 15] +
                   (ed_rotr(y, 19) ^ ed_rotr(y, 61) ^ (y >> 6));
    }
    const uint64_t t1 = h + (ed_rotr(e, 14) ^ ed_rotr(e, 18) ^ ed_rotr(e, 41)) + ((e & f) ^ (~e & g)) + ED_K(t) +
                        w[t & 15];
    const uint64_t t2 = (ed_rotr(a, 28) ^ ed_rotr(a, 34) ^ ed_rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + t2;
  }
  out[0] = a + 0x6a09e667f3bcc908ull;
  out[1] = b + 0xbb67ae8584caa73bull;
  out[2] = c + 0x3c6ef372fe94f82bull;
  out[3] = d + 0xa54ff53a5f1d36f1ull;
  out[4] = e + 0x510e527fade682d1ull;
  out[5] = f + 0x9b05688c2b3e6c1full;
  out[6] = g + 0x1f83d9abfb41bd6bull;
  out[7] = h + 0x5be0cd19137e2179ull;
}

// a 512-bit integer (16 LE words) mod l, canonical: x0 + x1 2^252 + x2 2^504 with every chunk below
// 2^252 < l, so each Montgomery product has both operands below l
ZG_INL EdS ed_mod_l(const uint32_t* w) {
  EdS x0, x1, x2, c1, c2;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    x0.l[i] = w[i];
    x1.l[i] = (w[7 + i] >> 28) | (w[8 + i] << 4);
    x2.l[i] = 0;
    c1.l[i] = ED_L_C252[i];
    c2.l[i] = ED_L_C504[i];
  }
  x0.l[7] &= 0x0fffffffu;
  x1.l[7] &= 0x0fffffffu;
  x2.l[0] = w[15] >> 24;
  return fp_add<EdLM>(fp_add<EdLM>(x0, fp_mul_inl<EdLM>(x1, c1)), fp_mul_inl<EdLM>(x2, c2));
}

ZG_INL void ed_load_words(const uint8_t* b, int nwords, uint32_t* w) {
  for (int i = 0; i < nwords; i++)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
           ((uint32_t)b[4 * i + 3] << 24);
}
ZG_INL uint32_t ed_bswap(uint32_t x) { return __builtin_bswap32(x); }

// the whole check of one item -> ZG_ED_* (0 ok, 1 key encoding, 2 signature encoding, 3 signature)
ZG_INL uint8_t ed25519_verify_one(const uint8_t* pubkey, const uint8_t* sig, const uint8_t* msg,
                                  const uint32_t* comb) {
  uint32_t pk[8], rs[16], m[8];
  ed_load_words(pubkey, 8, pk);
  ed_load_words(sig, 16, rs);
  ed_load_words(msg, 8, m);
  EdP A;
  if (!ed_decompress(pk, &A)) return 1;
  if (rs[15] & 0xe0000000u) return 2;
  // k = SHA-512(R || pubkey || msg) mod l
  uint64_t w[16], h[8];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    w[i] = ((uint64_t)ed_bswap(rs[2 * i]) << 32) | ed_bswap(rs[2 * i + 1]);
    w[4 + i] = ((uint64_t)ed_bswap(pk[2 * i]) << 32) | ed_bswap(pk[2 * i + 1]);
    w[8 + i] = ((uint64_t)ed_bswap(m[2 * i]) << 32) | ed_bswap(m[2 * i + 1]);
  }
  w[12] = 0x8000000000000000ull;
  w[13] = w[14] = 0;
  w[15] = 96 * 8;
  ed_sha512_block(w, h);
  uint32_t hw[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    hw[2 * i] = ed_bswap((uint32_t)(h[i] >> 32));
    hw[2 * i + 1] = ed_bswap((uint32_t)h[i]);
  }
  const EdS k = ed_mod_l(hw);
  EdP p = ed_mul(ed_neg(A), k.l, 253);  // k < l < 2^253
  p = ed_add_fixed(p, comb, rs + 8);
  uint32_t rc[8], acc = 0;
  ed_compress(p, rc);
#pragma unroll
  for (int i = 0; i < 8; i++) acc |= rc[i] ^ rs[i];
  return acc == 0 ? 0 : 3;
}

// comb table entry t: (d + 1) 2^(8 w) B as (y + x, y - x, 2 d x y), canonical digits
ZG_INL void ed_comb_entry(int t, uint32_t* e) {
  const int d = t % ZG_ED_COMB_D + 1, w = t / ZG_ED_COMB_D;
  uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  k[w >> 2] = (uint32_t)d << (8 * (w & 3));
  const Fe bx = fe_const(ED_BX), by = fe_const(ED_BY);
  const EdP p = ed_mul({bx, by, fe_one(), fe_mul(bx, by)}, k, 256);
  const Fe zi = fe_inv(p.Z);
  const Fe x = fe_mul(p.X, zi), y = fe_mul(p.Y, zi);
  uint32_t c[8];
  fe_canon(fe_add(y, x), c);
  const Fe ypx = fe_from_words(c);
  fe_canon(fe_sub(y, x), c);
  const Fe ymx = fe_from_words(c);
  fe_canon(fe_mul(fe_mul(x, y), fe_const(ED_2D)), c);
  const Fe xy2d = fe_from_words(c);
  for (int l = 0; l < 9; l++) {
    e[l] = ypx.d[l];
    e[9 + l] = ymx.d[l];
    e[18 + l] = xy2d.d[l];
  }
}

// debug entries (zg_debug_field_mul fields 5 and 6), 8-word operands and result
ZG_INL void ed_debug_fe_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  fe_canon(fe_mul(fe_from_words(a), fe_from_words(b)), r);
}
ZG_INL void ed_debug_mod_l(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  uint32_t w[16];
  for (int i = 0; i < 8; i++) {
    w[i] = a[i];
    w[8 + i] = b[i];
  }
  const EdS k = ed_mod_l(w);
  for (int i = 0; i < 8; i++) r[i] = k.l[i];
}

}  // namespace zg
