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
// Field 2^255 - 19: the 9 x 29-bit digit field of zg_fd9.h (the fold is 2^261 = 2^6 * 19 = 1216).
// Points: extended coordinates, a = -1 (add-2008-hwcd-3, dbl-2008-hwcd); d is a non-square, so the
// addition is complete for every input, small-order points included.
#pragma once
#include "zg_fd9.h"
#include "zg_hash.h"

namespace zg {

#define ZG_ED_COMB_W 32
#define ZG_ED_COMB_D 255
#define ZG_ED_COMB_WORDS 27  // y + x, y - x, 2 d x y: 9 digits each
#define ZG_ED_COMB_POINTS (ZG_ED_COMB_W * ZG_ED_COMB_D)

struct EdFM {  // 2^255 - 19
  static constexpr int BITS = 255, C1SH = 0;
  static constexpr uint32_t C0 = 19;
};
using Fe = Fd9<EdFM>;
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

ZG_INL Fe fe_const(const uint32_t* c) {
  Fe r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.d[i] = c[i];
  return r;
}

// z^(2^250 - 1); *z11 = z^11
ZG_INL Fe fe_pow250(const Fe& z, Fe* z11) {
  const Fe z2 = fd_sqr(z);
  const Fe z9 = fd_mul(fd_sqr_n(z2, 2), z);
  *z11 = fd_mul(z9, z2);
  const Fe t5 = fd_mul(fd_sqr(*z11), z9);             // 2^5 - 1
  const Fe t10 = fd_mul(fd_sqr_n(t5, 5), t5);         // 2^10 - 1
  const Fe t20 = fd_mul(fd_sqr_n(t10, 10), t10);      // 2^20 - 1
  const Fe t40 = fd_mul(fd_sqr_n(t20, 20), t20);      // 2^40 - 1
  const Fe t50 = fd_mul(fd_sqr_n(t40, 10), t10);      // 2^50 - 1
  const Fe t100 = fd_mul(fd_sqr_n(t50, 50), t50);     // 2^100 - 1
  const Fe t200 = fd_mul(fd_sqr_n(t100, 100), t100);  // 2^200 - 1
  return fd_mul(fd_sqr_n(t200, 50), t50);             // 2^250 - 1
}
ZG_INL Fe fe_inv(const Fe& z) {  // z^(p - 2) = z^(2^255 - 21)
  Fe z11;
  const Fe t = fe_pow250(z, &z11);
  return fd_mul(fd_sqr_n(t, 5), z11);
}
ZG_INL Fe fe_pow22523(const Fe& z) {  // z^((p - 5) / 8) = z^(2^252 - 3)
  Fe z11;
  const Fe t = fe_pow250(z, &z11);
  return fd_mul(fd_sqr_n(t, 2), z);
}

// ---- points
struct EdP {
  Fe X, Y, Z, T;  // x = X / Z, y = Y / Z, x y = T / Z
};
struct EdCached {
  Fe YpX, YmX, Z2, T2d;  // Y + X, Y - X, 2 Z, 2 d T
};
ZG_INL EdP ed_identity() { return {Fe::zero(), Fe::one(), Fe::one(), Fe::zero()}; }
ZG_INL EdP ed_neg(const EdP& p) { return {fd_neg(p.X), p.Y, p.Z, fd_neg(p.T)}; }
ZG_INL EdCached ed_cache(const EdP& p) {
  return {fd_add(p.Y, p.X), fd_sub(p.Y, p.X), fd_add(p.Z, p.Z), fd_mul(p.T, fe_const(ED_2D))};
}
ZG_INL EdP ed_dbl(const EdP& p) {
  const Fe A = fd_sqr(p.X), B = fd_sqr(p.Y), Z2 = fd_sqr(p.Z);
  const Fe C = fd_add(Z2, Z2);
  const Fe S = fd_add(A, B);  // -H
  const Fe E = fd_sub(fd_sqr(fd_add_nc(p.X, p.Y)), S);
  const Fe G = fd_sub(B, A), F = fd_sub(G, C), H = fd_neg(S);
  return {fd_mul(E, F), fd_mul(G, H), fd_mul(F, G), fd_mul(E, H)};
}
ZG_INL EdP ed_add(const EdP& p, const EdCached& q) {
  const Fe A = fd_mul(fd_sub(p.Y, p.X), q.YmX);
  const Fe B = fd_mul(fd_add_nc(p.Y, p.X), q.YpX);
  const Fe C = fd_mul(p.T, q.T2d);
  const Fe D = fd_mul(p.Z, q.Z2);
  const Fe E = fd_sub(B, A), F = fd_sub(D, C), G = fd_add(D, C), H = fd_add(B, A);
  return {fd_mul(E, F), fd_mul(G, H), fd_mul(F, G), fd_mul(E, H)};
}
// q affine: (y + x, y - x, 2 d x y)
ZG_INL EdP ed_add_aff(const EdP& p, const Fe& ypx, const Fe& ymx, const Fe& xy2d) {
  const Fe A = fd_mul(fd_sub(p.Y, p.X), ymx);
  const Fe B = fd_mul(fd_add_nc(p.Y, p.X), ypx);
  const Fe C = fd_mul(p.T, xy2d);
  const Fe D = fd_add(p.Z, p.Z);
  const Fe E = fd_sub(B, A), F = fd_sub(D, C), G = fd_add(D, C), H = fd_add(B, A);
  return {fd_mul(E, F), fd_mul(G, H), fd_mul(F, G), fd_mul(E, H)};
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
  fd_canon(fd_mul(p.X, zi), x);
  fd_canon(fd_mul(p.Y, zi), out);
  out[7] |= (x[0] & 1u) << 31;
}
// CompressedEdwardsY::decompress of 8 LE words; false = not a point
ZG_INL bool ed_decompress(const uint32_t* in, EdP* out) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = in[i];
  const bool sign = w[7] >> 31;
  w[7] &= 0x7fffffffu;
  const Fe y = Fe::from_words(w);  // not required to be below p
  const Fe y2 = fd_sqr(y);
  const Fe u = fd_sub(y2, Fe::one());
  const Fe v = fd_add(fd_mul(y2, fe_const(ED_D)), Fe::one());
  const Fe v3 = fd_mul(fd_sqr(v), v);
  const Fe v7 = fd_mul(fd_sqr(v3), v);
  Fe x = fd_mul(fd_mul(u, v3), fe_pow22523(fd_mul(u, v7)));
  const Fe chk = fd_mul(v, fd_sqr(x));
  if (!fd_eq(chk, u)) {
    if (!fd_eq(chk, fd_neg(u))) return false;
    x = fd_mul(x, fe_const(ED_SQRTM1));
  }
  uint32_t xc[8];
  fd_canon(x, xc);
  if ((bool)(xc[0] & 1u) != sign) x = fd_neg(x);  // the even root, negated when the sign bit is set
  *out = {x, y, Fe::one(), fd_mul(x, y)};
  return true;
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
  sha512_block(w, h);
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
  const EdP p = ed_mul({bx, by, Fe::one(), fd_mul(bx, by)}, k, 256);
  const Fe zi = fe_inv(p.Z);
  const Fe x = fd_mul(p.X, zi), y = fd_mul(p.Y, zi);
  uint32_t c[8];
  fd_canon(fd_add(y, x), c);
  const Fe ypx = Fe::from_words(c);
  fd_canon(fd_sub(y, x), c);
  const Fe ymx = Fe::from_words(c);
  fd_canon(fd_mul(fd_mul(x, y), fe_const(ED_2D)), c);
  const Fe xy2d = Fe::from_words(c);
  for (int l = 0; l < 9; l++) {
    e[l] = ypx.d[l];
    e[9 + l] = ymx.d[l];
    e[18 + l] = xy2d.d[l];
  }
}

// debug entries (zg_debug_field_mul fields 5 and 6), 8-word operands and result
ZG_INL void ed_debug_fe_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  fd_canon(fd_mul(Fe::from_words(a), Fe::from_words(b)), r);
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
