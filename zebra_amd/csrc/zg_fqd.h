// zg_fqd.h -- lazy digit-resident Fq and G1 Jacobian arithmetic for point-operation chains
// (the decode kernels' subgroup checks and GLV products r_i A_i).
//
// FqD holds an Fq value as 14 normalized 29-bit digits in Montgomery form R' = 2^406 (the
// representation of zg_fq29_gen.h fq29d_*), NOT reduced mod p: the value is below K p for a bound
// K that the formulas below track by hand (comments: bounds in units of p). A product
// (fq29d_mul / fq29d_sqr; their column sums stay below 2^64 for any normalized 14-digit inputs)
// of a < Ka p and b < Kb p returns (a b + m p) / 2^406 < (Ka Kb p / 2^406 + 1) p < 2p whenever
// Ka Kb < 2^25 (p < 2^381). Sums and differences are digit-wise with one carry normalization and
// are never reduced. A chain of point operations therefore splits, repacks and canonicalises
// nothing between its products (the word form of zg_field.h does all three in every fq_mul) and
// pays one conversion in and one out per point.
//
// A difference c_a a - c_b b is formed as c_a a + (k p - c_b b) with k p held in "borrowed"
// digits (digits 0..12 raised by c_b 2^29, digits 1..13 lowered by c_b): each digit of
// k p - c_b b is non-negative for normalized b with c_b b <= (k - 1) p and c_b <= 13
// (floor(p / 2^377) = 13 covers the lowered top digit).
#pragma once
#include "zg_curve.h"

namespace zg {

struct FqD {
  uint32_t d[14];
};

// k p in digits 0..13, digits 0..12 raised by s 2^29 and digits 1..13 lowered by s
struct FqDK {
  uint32_t d[14];
};
constexpr FqDK fqd_kp(uint32_t k, uint32_t s) {
  uint32_t w[13] = {};
  uint64_t c = 0;
  for (int i = 0; i < 12; i++) {
    const uint64_t m = (uint64_t)FQ_P[i] * k + c;
    w[i] = (uint32_t)m;
    c = m >> 32;
  }
  w[12] = (uint32_t)c;
  FqDK r = {};
  for (int L = 0; L < 14; L++) {
    const int bit = 29 * L, wi = bit >> 5, off = bit & 31;
    uint64_t v = (uint64_t)w[wi] >> off;
    if (wi + 1 < 13) v |= (uint64_t)w[wi + 1] << (32 - off);
    r.d[L] = L < 13 ? (uint32_t)(v & 0x1fffffffu) : (uint32_t)v;
  }
  for (int L = 0; L < 14; L++) {
    if (L < 13) r.d[L] += s << 29;
    if (L > 0) r.d[L] -= s;
  }
  return r;
}

// R' mod p = 2^406 mod p: the FqD form of 1
static constexpr uint32_t FQD_ONE[14] = {0x03a9fb84u, 0x0ba00690u, 0x071288f1u, 0x0f59bcc5u, 0x126cb614u,
                                         0x0585bf36u, 0x1b85ac3du, 0x1cf856fau, 0x1891ecbdu, 0x1a7eec05u,
                                         0x155a88f0u, 0x0741ac6du, 0x1317c30fu, 0x00000009u};

// carry normalization (value unchanged); digits must leave room for the carries (< 2^32 - 8)
ZG_INL void fqd_norm(uint32_t* d) {
#pragma unroll
  for (int i = 0; i < 13; i++) {
    d[i + 1] += d[i] >> 29;
    d[i] &= FQ29_MASK;
  }
}

ZG_INL FqD fqd_one() {
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = FQD_ONE[i];
  return r;
}
ZG_INL FqD fqd_zero() {
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = 0u;
  return r;
}
// ZG_FQD_CALL (default 1): the products are two out-of-line functions with register arguments
// (as fq_mul_v / fq_sqr_v), so a chain's code stays small (a fully inlined subgroup check is
// ~16 k instructions, past the instruction cache a decode wave shares); 0 inlines them
#ifndef ZG_FQD_CALL
#define ZG_FQD_CALL 1
#endif
#if ZG_FQD_CALL
ZG_NOINL inline u32x16 fqd_mul_v(u32x16 a, u32x16 b) {
  uint32_t x[14], y[14], r[14];
#pragma unroll
  for (int i = 0; i < 14; i++) {
    x[i] = a[i];
    y[i] = b[i];
  }
  fq29d_mul(r, x, y);
  u32x16 o;
#pragma unroll
  for (int i = 0; i < 14; i++) o[i] = r[i];
  o[14] = o[15] = 0;
  return o;
}
ZG_NOINL inline u32x16 fqd_sqr_v(u32x16 a) {
  uint32_t x[14], r[14];
#pragma unroll
  for (int i = 0; i < 14; i++) x[i] = a[i];
  fq29d_sqr(r, x);
  u32x16 o;
#pragma unroll
  for (int i = 0; i < 14; i++) o[i] = r[i];
  o[14] = o[15] = 0;
  return o;
}
ZG_INL u32x16 fqd_pack(const FqD& a) {
  u32x16 v;
#pragma unroll
  for (int i = 0; i < 14; i++) v[i] = a.d[i];
  v[14] = v[15] = 0;
  return v;
}
ZG_INL FqD fqd_unpack(const u32x16& v) {
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = v[i];
  return r;
}
ZG_INL FqD fqd_mul(const FqD& a, const FqD& b) { return fqd_unpack(fqd_mul_v(fqd_pack(a), fqd_pack(b))); }
ZG_INL FqD fqd_sqr(const FqD& a) { return fqd_unpack(fqd_sqr_v(fqd_pack(a))); }
#else
ZG_INL FqD fqd_mul(const FqD& a, const FqD& b) {  // < 2p for Ka Kb < 2^25
  FqD r;
  fq29d_mul(r.d, a.d, b.d);
  return r;
}
ZG_INL FqD fqd_sqr(const FqD& a) {  // < 2p for Ka < 2^12
  FqD r;
  fq29d_sqr(r.d, a.d);
  return r;
}
#endif
// c a (c a small positive integer)
template <int C>
ZG_INL FqD fqd_smul(const FqD& a) {
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = C * a.d[i];
  fqd_norm(r.d);
  return r;
}
ZG_INL FqD fqd_add(const FqD& a, const FqD& b) {
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = a.d[i] + b.d[i];
  fqd_norm(r.d);
  return r;
}
// CA a - CB b + K p   (requires CB b <= (K - 1) p, CB <= 13; result < CA a + K p)
template <int K, int CA, int CB>
ZG_INL FqD fqd_sub(const FqD& a, const FqD& b) {
  constexpr FqDK kp = fqd_kp(K, CB);
  static_assert(CB >= 1 && CB <= 13 && CA >= 0 && CA + CB <= 6, "digit budget");
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = CA * a.d[i] + (kp.d[i] - CB * b.d[i]);
  fqd_norm(r.d);
  return r;
}
// a - b - c + K p   (requires b + c <= (K - 1) p; result < a + K p)
template <int K>
ZG_INL FqD fqd_sub2(const FqD& a, const FqD& b, const FqD& c) {
  constexpr FqDK kp = fqd_kp(K, 2);
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = a.d[i] + (kp.d[i] - b.d[i] - c.d[i]);
  fqd_norm(r.d);
  return r;
}
// -x for x < 2p: 3p - x < 3p
ZG_INL FqD fqd_neg2(const FqD& x) { return fqd_sub<3, 0, 1>(fqd_zero(), x); }
// (a b + c d) / 2^406 mod p under one reduction (fq29d_dot2), all four operands normalized:
// < 2p for Ka Kb + Kc Kd < 2^25. Four operands do not fit the register arguments of an out-of-line
// product (two u32x16 fill v0..v31), so it is inlined at its call sites: one per point formula.
ZG_INL FqD fqd_dot2(const FqD& a, const FqD& b, const FqD& c, const FqD& d) {
  FqD r;
  fq29d_dot2(r.d, a.d, b.d, c.d, d.d);
  return r;
}
// v == 0 mod p for a product output or any v < 2p (normalized digits are unique: v is 0 or p)
ZG_INL bool fqd_is_zero2(const FqD& v) {
  constexpr FqDK p1 = fqd_kp(1, 0);
  bool z0 = true, z1 = true;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    z0 = z0 && v.d[i] == 0u;
    z1 = z1 && v.d[i] == p1.d[i];
  }
  return z0 || z1;
}
// v == 0 mod p for v < 4p
ZG_INL bool fqd_is_zero4(const FqD& v) {
  constexpr FqDK p1 = fqd_kp(1, 0), p2 = fqd_kp(2, 0), p3 = fqd_kp(3, 0);
  bool z0 = true, z1 = true, z2 = true, z3 = true;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    z0 = z0 && v.d[i] == 0u;
    z1 = z1 && v.d[i] == p1.d[i];
    z2 = z2 && v.d[i] == p2.d[i];
    z3 = z3 && v.d[i] == p3.d[i];
  }
  return z0 || z1 || z2 || z3;
}

// word Montgomery form (R = 2^384, any value < 2^384) -> FqD (< 2p)
ZG_INL FqD fqd_from(const Fq& a) {
  FqD r;
  fq29d_from_mont(r.d, a.l);
  return r;
}
// FqD (any value < 2^21 p) -> canonical word Montgomery form
ZG_INL Fq fqd_to(const FqD& a) {
  Fq r;
  fq29d_to_mont(r.l, a.d);
  return r;
}

// ------------------------------------------------------------------ bound checking (host only)
// A build with ZG_FQD_CHECK verifies every FQD_CHK(v, K) on the host: v's digits 0..12 are
// normalized and v < K p. Violations are counted (fqd_check_fails()), never on the device.
#if defined(ZG_FQD_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
inline int& fqd_check_fails() {
  static int n = 0;
  return n;
}
inline void fqd_check(const FqD& v, uint32_t K) {
  const FqDK kp = fqd_kp(K, 0);
  bool ok = true, lt = false;
  for (int i = 0; i < 13; i++) ok = ok && v.d[i] <= FQ29_MASK;
  for (int i = 13; i >= 0 && !lt; i--) {
    if (v.d[i] > kp.d[i]) break;
    lt = v.d[i] < kp.d[i];
  }
  if (!ok || !lt) fqd_check_fails()++;
}
#define FQD_CHK(v, K) fqd_check(v, K)
#else
#define FQD_CHK(v, K) ((void)0)
#endif

// ------------------------------------------------------------------ Fq2 = Fq[u] / (u^2 + 1) in lazy digits
// Fq2D holds both coefficients as FqD (R' = 2^406, normalized digits, value below a tracked K p).
// The products are schoolbook with one reduction per coefficient (the MAC structure of f2_mul29 /
// f2_sqr29 / f2_mul_fq29 of zg_fq29_gen.h, without their splits, repacks and canonicalisation):
//   value: an output is < S / 2^406 + p for its column sum S, so < 2p whenever S < 2^25 p^2;
//   digits: an operand pair may have one side unnormalized (digits < 2^30), see fq29d_mul2.
// Mixed representations cost nothing: REDC' of an R' operand (x 2^406) and an R operand (x 2^384, the
// word form's digits as they are) is the product in R form, i.e. the word form's Montgomery value,
// and a canonical word-form value shifted left by 22 bits is its R' form below 2^22 p.
struct Fq2D {
  FqD c0, c1;
};
#define F2D_CHK(v, K) (FQD_CHK((v).c0, K), FQD_CHK((v).c1, K))

ZG_INL Fq2D f2d_one() { return {fqd_one(), fqd_zero()}; }
ZG_INL Fq2D f2d_from(const Fq2& a) { return {fqd_from(a.c0), fqd_from(a.c1)}; }
ZG_INL Fq2D f2d_add(const Fq2D& a, const Fq2D& b) { return {fqd_add(a.c0, b.c0), fqd_add(a.c1, b.c1)}; }
template <int C>
ZG_INL Fq2D f2d_smul(const Fq2D& a) {
  return {fqd_smul<C>(a.c0), fqd_smul<C>(a.c1)};
}
template <int K, int CA, int CB>
ZG_INL Fq2D f2d_sub(const Fq2D& a, const Fq2D& b) {
  return {fqd_sub<K, CA, CB>(a.c0, b.c0), fqd_sub<K, CA, CB>(a.c1, b.c1)};
}
template <int K>
ZG_INL Fq2D f2d_sub2(const Fq2D& a, const Fq2D& b, const Fq2D& c) {
  return {fqd_sub2<K>(a.c0, b.c0, c.c0), fqd_sub2<K>(a.c1, b.c1, c.c1)};
}
// the 32-bit budget of a digit-wise sum before fqd_norm: digit i holds at most kp_i plus ca normalized
// digits, plus the carry out of digit i - 1 (below 8 when that digit stayed below 2^32)
constexpr bool fqd_budget_ok(const FqDK& kp, uint32_t ca) {
  for (int i = 0; i < 14; i++)
    if ((uint64_t)kp.d[i] + (uint64_t)ca * FQ29_MASK + (i > 0 ? 7u : 0u) > 0xffffffffull) return false;
  return true;
}
// a - b - c - 4d + K p   (requires b + c + 4d <= (K - 1) p; result < a + K p). The budget is exactly
// full: a borrowed digit of K p is at most 2^29 - 1 + 6 2^29 - 6, a adds at most 2^29 - 1 (2^32 - 8),
// and the carry into it is at most 7; digit 0 (not lowered by 6) takes no carry.
template <int K>
ZG_INL FqD fqd_sub114(const FqD& a, const FqD& b, const FqD& c, const FqD& d) {
  constexpr FqDK kp = fqd_kp(K, 6);
  static_assert(fqd_budget_ok(kp, 1), "digit budget");
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = a.d[i] + (kp.d[i] - b.d[i] - c.d[i] - 4u * d.d[i]);
  fqd_norm(r.d);
  return r;
}
// Unnormalized forms for a product's scalar-side operand (digits < 3 2^29): 2a, and K p - 2a
// (requires 2a <= (K - 1) p; value < K p)
ZG_INL Fq2D f2d_dbl_raw(const Fq2D& a) {
  Fq2D r;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    r.c0.d[i] = 2u * a.c0.d[i];
    r.c1.d[i] = 2u * a.c1.d[i];
  }
  return r;
}
template <int K>
ZG_INL Fq2D f2d_negdbl_raw(const Fq2D& a) {
  constexpr FqDK kp = fqd_kp(K, 2);
  Fq2D r;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    r.c0.d[i] = kp.d[i] - 2u * a.c0.d[i];
    r.c1.d[i] = kp.d[i] - 2u * a.c1.d[i];
  }
  return r;
}

// x y for x, y normalized, y.c1 <= (KY - 1) p: < 2p per coefficient for |x| (|y| + KY) < 2^24 (in units of p)
template <int KY>
ZG_INL Fq2D f2d_mul(const Fq2D& x, const Fq2D& y) {
  constexpr FqDK kp = fqd_kp(KY, 1);
  uint32_t n1[14];
#pragma unroll
  for (int i = 0; i < 14; i++) n1[i] = kp.d[i] - y.c1.d[i];
  Fq2D r;
  f2d_mul29(r.c0.d, r.c1.d, x.c0.d, x.c1.d, y.c0.d, y.c1.d, n1);
  return r;
}
// a^2 for a normalized, a.c1 <= (K - 1) p: c0 = (a0 + a1)(a0 - a1 + K p), c1 = a0 (2 a1); < 2p
template <int K>
ZG_INL Fq2D f2d_sqr(const Fq2D& a) {
  const FqD dif = fqd_sub<K, 1, 1>(a.c0, a.c1);
  uint32_t s[14], t[14];
#pragma unroll
  for (int i = 0; i < 14; i++) {
    s[i] = a.c0.d[i] + a.c1.d[i];
    t[i] = a.c1.d[i] << 1;
  }
  Fq2D r;
  fq29d_mul2(r.c0.d, r.c1.d, s, dif.d, a.c0.d, t);
  return r;
}
// x q for a canonical word-form q (a G2 coordinate read from memory), result in R' digits:
// q enters as 2^22 q (< 2^22 p), so the result is < (|x| 2^23 / 2^25 + 1) p
ZG_INL Fq2D f2d_mul_w22(const Fq2D& x, const Fq2& q) {
  const Fq nq1 = fq_neg(q.c1);
  uint32_t y0[14], y1[14], n1[14];
  fq29d_split22(y0, q.c0.l);
  fq29d_split22(y1, q.c1.l);
  fq29d_split22(n1, nq1.l);
  Fq2D r;
  f2d_mul29(r.c0.d, r.c1.d, x.c0.d, x.c1.d, y0, y1, n1);
  return r;
}
// x q for a canonical word-form q, result in the canonical word form (x R' times q R is x q R)
ZG_INL Fq2 f2d_mul_to_w(const Fq2D& x, const Fq2& q) {
  constexpr FqDK kp = fqd_kp(2, 1);
  uint32_t y0[14], y1[14], n1[14], u0[14], u1[14];
  fq29d_split(y0, q.c0.l);
  fq29d_split(y1, q.c1.l);
#pragma unroll
  for (int i = 0; i < 14; i++) n1[i] = kp.d[i] - y1[i];
  f2d_mul29(u0, u1, x.c0.d, x.c1.d, y0, y1, n1);
  Fq2 r;
  fq29d_pack(r.c0.l, u0);
  fq29d_pack(r.c1.l, u1);
  return r;
}
// (x0 s, x1 s) for a canonical word-form s, result in the canonical word form; x may be
// unnormalized (digits < 3 2^29), |x| < 2^24
ZG_INL Fq2 f2d_mulfq_to_w(const Fq2D& x, const Fq& s) {
  uint32_t sd[14], u0[14], u1[14];
  fq29d_split(sd, s.l);
  fq29d_mul2(u0, u1, x.c0.d, sd, x.c1.d, sd);
  Fq2 r;
  fq29d_pack(r.c0.l, u0);
  fq29d_pack(r.c1.l, u1);
  return r;
}
// R' digits (normalized, < 2^22 p) -> the canonical word form
ZG_INL Fq2 f2d_to_w(const Fq2D& a) {
  Fq2 r;
  fq29d_red22(r.c0.l, a.c0.d);
  fq29d_red22(r.c1.l, a.c1.d);
  return r;
}

// ------------------------------------------------------------------ G1 Jacobian (y^2 = x^3 + 4)
// ZG_G1D_DOT2 (default 1): every point formula closes its Y3 as one sum of two products under one
// reduction (fqd_dot2), and the doubling forms D = 4 X B as a product: one reduction fewer per
// doubling and per addition; 0: dbl-2009-l / madd-2007-bl / add-2007-bl with Y3 as two reduced
// products and a difference (the A/B reference). The same elements of Fq either way.
#ifndef ZG_G1D_DOT2
#define ZG_G1D_DOT2 1
#endif
// Invariant of every G1D below: X < G1D_KX p, Y < G1D_KY p, Z < 4p; infinity is Z == 0 mod p.
// With fqd_dot2 X < 19p (a doubling's X3), Y < 4p (an affine operand's -y; every formula's Y3 < 2p);
// without it X < 35p, Y < 19p.
#if ZG_G1D_DOT2
static constexpr int G1D_KX = 19, G1D_KY = 4;
#else
static constexpr int G1D_KX = 35, G1D_KY = 19;
#endif
struct G1D {
  FqD x, y, z;
};
#define G1D_CHK(p) (FQD_CHK((p).x, G1D_KX), FQD_CHK((p).y, G1D_KY), FQD_CHK((p).z, 4))

ZG_INL bool g1d_is_inf(const G1D& p) { return fqd_is_zero4(p.z); }
ZG_INL G1D g1d_from_aff(const FqD& x, const FqD& y) { return {x, y, fqd_one()}; }
ZG_INL G1D g1d_infinity() { return {fqd_one(), fqd_one(), fqd_zero()}; }
// canonical word-form Jacobian (the same point; Z = 0 stays infinity)
ZG_INL G1J g1d_to_jac(const G1D& p) { return {fqd_to(p.x), fqd_to(p.y), fqd_to(p.z)}; }

#if ZG_G1D_DOT2
// dbl-2009-l (a = 0) with D = 2((X + B)^2 - A - C) = 4 X B as one product and
// Y3 = E (D - X3) - 8C = E W + (3p - B)(8B) under one reduction: C = B^2 and T = (X + B)^2 are
// never formed. 6 reductions. In: the invariant. Out: X < 19p, Y < 2p, Z < 4p.
// Infinity (Z = 0) doubles to Z = 2 Y Z = 0.
ZG_INL G1D g1d_dbl(const G1D& p) {
  G1D_CHK(p);
  const FqD A = fqd_sqr(p.x);                              // < 2
  const FqD B = fqd_sqr(p.y);                              // < 2
  const FqD D = fqd_smul<4>(fqd_mul(p.x, B));              // 4 (19 x 2 -> < 2): < 8
  const FqD E = fqd_smul<3>(A);                            // < 6
  const FqD F = fqd_sqr(E);                                // < 2
  const FqD X3 = fqd_sub<17, 1, 2>(F, D);                  // F - 2D + 17p: < 19 (2D < 16)
  const FqD W = fqd_sub<20, 1, 1>(D, X3);                  // D - X3 + 20p: < 28 (X3 < 19)
  const FqD nB = fqd_neg2(B), B8 = fqd_smul<8>(B);         // 3p - B < 3, 8B < 16 (both normalized)
  const FqD Y3 = fqd_dot2(E, W, nB, B8);                   // 6 x 28 + 3 x 16 = 216: < 2
  const FqD Z3 = fqd_smul<2>(fqd_mul(p.y, p.z));           // < 4
  FQD_CHK(D, 8), FQD_CHK(X3, 19), FQD_CHK(W, 28), FQD_CHK(nB, 3), FQD_CHK(B8, 16), FQD_CHK(Y3, 2), FQD_CHK(Z3, 4);
  return {X3, Y3, Z3};
}
#else
// dbl-2009-l (a = 0), 7 products. In: the invariant. Out: X < 31p, Y < 19p, Z < 4p.
// Infinity (Z = 0) doubles to Z = 2 Y Z = 0.
ZG_INL G1D g1d_dbl(const G1D& p) {
  const FqD A = fqd_sqr(p.x);                              // < 2
  const FqD B = fqd_sqr(p.y);                              // < 2
  const FqD C = fqd_sqr(B);                                // < 2
  const FqD T = fqd_sqr(fqd_add(p.x, B));                  // (X + B < 37)^2: < 2
  const FqD D = fqd_smul<2>(fqd_sub2<5>(T, A, C));         // 2 (T - A - C + 5p): < 14 (A + C < 4)
  const FqD E = fqd_smul<3>(A);                            // < 6
  const FqD F = fqd_sqr(E);                                // < 2
  const FqD X3 = fqd_sub<29, 1, 2>(F, D);                  // F - 2D + 29p: < 31 (2D < 28)
  const FqD Y3a = fqd_mul(E, fqd_sub<32, 1, 1>(D, X3));    // (D - X3 + 32p < 46) E: < 2
  const FqD Y3 = fqd_sub<17, 1, 1>(Y3a, fqd_smul<8>(C));   // - 8C + 17p: < 19 (8C < 16)
  const FqD Z3 = fqd_smul<2>(fqd_mul(p.y, p.z));           // < 4
  return {X3, Y3, Z3};
}
#endif

// g1d_dbl on a whole wave for a lone doubling chain (K4's top-window scaling, zg_msm.hip): the same
// formulas and bounds, so the same digits, with the products in three levels of independent
// products, one per lane, exchanged through `xch` (3 FqD of LDS, the wave's own). With fqd_dot2:
// {A = X^2, B = Y^2, YZ}, {X B, F = (3A)^2}, {Y3 = E W + (3p - B)(8B)}, the last on every lane
// alike (its operands are wave-uniform: nothing to exchange). Without: {A, B, YZ},
// {C = B^2, T = (X + B)^2, F}, {E (D - X3)}. Every lane of the wave calls it with the same p and
// gets the result.
ZG_INL FqD fqd_pick3(int k, const FqD& a, const FqD& b, const FqD& c) {
  FqD r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = k == 0 ? a.d[i] : k == 1 ? b.d[i] : c.d[i];
  return r;
}
ZG_INL void fqd_xch_put(FqD* xch, int lane, const FqD& v) {
  if (lane < 3) xch[lane] = v;
  __syncthreads();
}
ZG_INL G1D g1d_dbl_wave(const G1D& p, FqD* xch) {
  const int lane = threadIdx.x & 63, k = lane < 3 ? lane : 0;
  // level 1: A = X X, B = Y Y, YZ = Y Z
  const FqD m1 = fqd_mul(fqd_pick3(k, p.x, p.y, p.y), fqd_pick3(k, p.x, p.y, p.z));
  fqd_xch_put(xch, lane, m1);
  const FqD A = xch[0], B = xch[1], YZ = xch[2];
  __syncthreads();
  const FqD E = fqd_smul<3>(A);
#if ZG_G1D_DOT2
  // level 2: X B, F = E E (lane 2 repeats F)
  const FqD m2 = fqd_mul(fqd_pick3(k, p.x, E, E), fqd_pick3(k, B, E, E));
  fqd_xch_put(xch, lane, m2);
  const FqD XB = xch[0], F = xch[1];
  __syncthreads();
  const FqD D = fqd_smul<4>(XB);
  const FqD X3 = fqd_sub<17, 1, 2>(F, D);
  // level 3: one sum of two products, the same on every lane
  const FqD Y3 = fqd_dot2(E, fqd_sub<20, 1, 1>(D, X3), fqd_neg2(B), fqd_smul<8>(B));
#else
  // level 2: C = B^2, T = (X + B)^2, F = E^2 with E = 3 A
  const FqD m2 = fqd_sqr(fqd_pick3(k, B, fqd_add(p.x, B), E));
  fqd_xch_put(xch, lane, m2);
  const FqD C = xch[0], T = xch[1], F = xch[2];
  __syncthreads();
  const FqD D = fqd_smul<2>(fqd_sub2<5>(T, A, C));
  const FqD X3 = fqd_sub<29, 1, 2>(F, D);
  // level 3: E (D - X3)
  const FqD m3 = fqd_mul(E, fqd_sub<32, 1, 1>(D, X3));
  fqd_xch_put(xch, lane, m3);
  const FqD Y3a = xch[0];
  __syncthreads();
  const FqD Y3 = fqd_sub<17, 1, 1>(Y3a, fqd_smul<8>(C));
#endif
  const FqD Z3 = fqd_smul<2>(YZ);
  return {X3, Y3, Z3};
}

// The close of both additions: X3 = rr^2 - J - 2V, Y3 = rr (V - X3) - 2 Y J for Y = Y1 (mixed) or
// S1 (full), Y < KYB p, rr < 43p. With fqd_dot2 Y3 = rr W + ((KYB + 1) p - Y)(2J) under one
// reduction (< 2p); without, two reduced products and a difference (< 7p, needs Y J < 2p).
template <int KYB>
ZG_INL void g1d_add_close(FqD& X3, FqD& Y3, const FqD& rr, const FqD& RR, const FqD& J, const FqD& V, const FqD& Y) {
  X3 = fqd_sub2<7>(RR, J, fqd_smul<2>(V));                 // rr^2 - J - 2V + 7p: < 9 (J + 2V < 6)
  const FqD W = fqd_sub<10, 1, 1>(V, X3);                  // V - X3 + 10p: < 12
#if ZG_G1D_DOT2
  const FqD nY = fqd_sub<KYB + 1, 0, 1>(fqd_zero(), Y);    // (KYB + 1) p - Y: < KYB + 1 (normalized)
  const FqD J2 = fqd_smul<2>(J);                           // < 4
  Y3 = fqd_dot2(rr, W, nY, J2);                            // 43 x 12 + 5 x 4 = 536: < 2
  FQD_CHK(nY, KYB + 1), FQD_CHK(J2, 4), FQD_CHK(Y3, 2);
#else
  Y3 = fqd_sub<5, 1, 2>(fqd_mul(rr, W), fqd_mul(Y, J));    // rr W - 2 Y J + 5p: < 7 (2 Y J < 4)
  FQD_CHK(Y3, 7);
#endif
  FQD_CHK(X3, 9), FQD_CHK(W, 12);
}

// madd-2007-bl with complete case handling: p + q for q affine and finite, qx < 2p, qy < 4p.
// In: the invariant. Out: X < 9p, Y < 2p (7p without fqd_dot2), Z < 4p (or g1d_dbl's, or q itself).
// 10 reductions (11 without fqd_dot2).
ZG_INL G1D g1d_add_aff(const G1D& p, const FqD& qx, const FqD& qy) {
  G1D_CHK(p), FQD_CHK(qx, 2), FQD_CHK(qy, 4);
  if (g1d_is_inf(p)) return g1d_from_aff(qx, qy);
  const FqD Z1Z1 = fqd_sqr(p.z);                           // < 2
  const FqD U2 = fqd_mul(qx, Z1Z1);                        // < 2
  const FqD S2 = fqd_mul(fqd_mul(qy, p.z), Z1Z1);          // < 2
  const FqD H = fqd_sub<G1D_KX + 1, 1, 1>(U2, p.x);        // U2 - X1 + (KX + 1) p: < KX + 3 (22; 38)
  const FqD rr = fqd_sub<2 * G1D_KY + 1, 2, 2>(S2, p.y);   // 2 S2 - 2 Y1 + (2 KY + 1) p: < 2 KY + 5 (13; 43)
  const FqD HH = fqd_sqr(H);                               // < 2
  const FqD RR = fqd_sqr(rr);                              // < 2
  FQD_CHK(H, G1D_KX + 3), FQD_CHK(rr, 2 * G1D_KY + 5);
  // H == 0 mod p <=> H^2 == 0 (and rr likewise): P == +-Q
  if (fqd_is_zero2(HH)) {
    if (fqd_is_zero2(RR)) return g1d_dbl(p);
    return g1d_infinity();
  }
  const FqD I = fqd_smul<4>(HH);                           // < 8
  const FqD J = fqd_mul(H, I);                             // < 2
  const FqD V = fqd_mul(p.x, I);                           // < 2
  G1D r;
  g1d_add_close<G1D_KY>(r.x, r.y, rr, RR, J, V, p.y);      // Y1 < KY (Y1 J < 2)
  r.z = fqd_smul<2>(fqd_mul(p.z, H));                      // (Z1 + H)^2 - Z1Z1 - HH = 2 Z1 H: < 4
  return r;
}

// add-2007-bl with complete case handling and q's Z2Z2 = Z2^2, Z2C = Z2^3 given (both < 2p; a chain
// that adds one Jacobian point again and again forms them once): p + q, both in the invariant
// (either may be infinity). q is read from a store Hold where it is used -- get(k): 0 X2, 1 Y2,
// 2 Z2, 3 Z2^2, 4 Z2^3 -- so a chain may hold it outside its registers (G1HoldLds, zg_decode.h).
// Out: X < 9p, Y < 2p (7p without fqd_dot2), Z < 4p (or g1d_dbl's, or p / q itself).
// 13 reductions (14 without fqd_dot2).
template <class Hold>
ZG_INL G1D g1d_readd_t(const G1D& p, const Hold& h) {
  G1D_CHK(p);
  if (g1d_is_inf(p)) return {h.get(0), h.get(1), h.get(2)};
  if (fqd_is_zero4(h.get(2))) return p;
  const FqD Z1Z1 = fqd_sqr(p.z);                           // (Z1 < 4)^2: < 2
  const FqD U1 = fqd_mul(p.x, h.get(3));                   // KX x 2: < 2
  const FqD U2 = fqd_mul(h.get(0), Z1Z1);                  // < 2
  const FqD S1 = fqd_mul(p.y, h.get(4));                   // KY x 2: < 2
  const FqD S2 = fqd_mul(fqd_mul(h.get(1), p.z), Z1Z1);    // (KY x 4 -> < 2) x 2: < 2
  const FqD H = fqd_sub<3, 1, 1>(U2, U1);                  // U2 - U1 + 3p: < 5 (U1 < 2)
  const FqD rr = fqd_sub<5, 2, 2>(S2, S1);                 // 2 S2 - 2 S1 + 5p: < 9 (2 S1 < 4)
  const FqD HH = fqd_sqr(H);                               // < 2
  const FqD RR = fqd_sqr(rr);                              // < 2
  FQD_CHK(H, 5), FQD_CHK(rr, 9);
  // H == 0 mod p <=> H^2 == 0 (and rr likewise): P == +-Q
  if (fqd_is_zero2(HH)) {
    if (fqd_is_zero2(RR)) return g1d_dbl(p);
    return g1d_infinity();
  }
  const FqD I = fqd_smul<4>(HH);                           // (2H)^2: < 8
  const FqD J = fqd_mul(H, I);                             // 5 x 8: < 2
  const FqD V = fqd_mul(U1, I);                            // < 2
  G1D r;
  g1d_add_close<2>(r.x, r.y, rr, RR, J, V, S1);            // S1 < 2 (S1 J < 2)
  r.z = fqd_smul<2>(fqd_mul(fqd_mul(p.z, h.get(2)), H));   // 2 Z1 Z2 H: (16 -> < 2) x 5 -> < 2, x 2: < 4
  return r;
}
// the plain store: five FqD of the caller's own (registers, or the private segment)
struct G1Hold {
  FqD v[5];
  ZG_HD void put(int k, const FqD& x) { v[k] = x; }
  ZG_HD FqD get(int k) const { return v[k]; }
};
ZG_INL G1D g1d_readd(const G1D& p, const G1D& q, const FqD& Z2Z2, const FqD& Z2C) {
  G1D_CHK(q), FQD_CHK(Z2Z2, 2), FQD_CHK(Z2C, 2);
  return g1d_readd_t(p, G1Hold{{q.x, q.y, q.z, Z2Z2, Z2C}});
}

// add-2007-bl with complete case handling: p + q, both in the invariant (either may be infinity):
// g1d_readd after Z2^2 and Z2^3. 15 reductions (16 without fqd_dot2).
ZG_INL G1D g1d_add_full(const G1D& p, const G1D& q) {
  if (g1d_is_inf(p)) return q;
  if (g1d_is_inf(q)) return p;
  const FqD Z2Z2 = fqd_sqr(q.z);                           // < 2
  return g1d_readd(p, q, Z2Z2, fqd_mul(q.z, Z2Z2));        // 4 x 2: < 2
}

// G1 subgroup check (zg_curve.h g1_in_subgroup, same test): sigma(P) == -[x^2] P in FqD.
// ZG_SUBGROUP_XX (default 0: built, measured, off -- DESIGN.md 4f): [x^2] P = [|x|]([|x|] P), two
// walks of |x| = 0xd201000000010000 (weight 6): 63 doublings and 5 additions each, 126 + 10 point
// operations against the 127 + 16 of one walk of the 128-bit x^2 (weight 17). Both walks run the
// same loop body, g1d_dbl and g1d_readd_t of a held Jacobian point T with T.z^2 and T.z^3 beside
// it: T = (P.x, P.y, 1) first (three products by 1 per addition more than a mixed addition, 15 in
// all, for one copy of the code), then T = Q = [|x|] P. T lives in the store `hold` (five FqD: held
// in registers beside the walk's state they cost the decode kernel 588 spilled VGPRs; the kernel
// keeps them in LDS, G1HoldLds of zg_decode.h). Every case is handled by g1d_readd_t: for a point
// outside G1 Q or any intermediate may be the point at infinity or +-T. 0: the one walk of x^2
// with mixed additions of P.
#ifndef ZG_SUBGROUP_XX
#define ZG_SUBGROUP_XX 0
#endif
template <class Hold>
ZG_INL bool g1_in_subgroup_xx(const G1A& p, Hold& hold) {
  if (p.inf) return true;
  G1D q = g1d_from_aff(fqd_from(p.x), fqd_from(p.y));
  hold.put(0, q.x);
  hold.put(1, q.y);
  for (int k = 2; k < 5; k++) hold.put(k, fqd_one());
  for (int pass = 0; pass < 2; pass++) {
    for (int i = 62; i >= 0; i--) {  // bit 63 of |x| is the leading one
      q = g1d_dbl(q);
      if ((BLS_X >> i) & 1ull) q = g1d_readd_t(q, hold);
    }
    if (pass == 0) {
      const FqD zz = fqd_sqr(q.z);
      hold.put(0, q.x);
      hold.put(1, q.y);
      hold.put(2, q.z);
      hold.put(3, zz);
      hold.put(4, fqd_mul(q.z, zz));
    }
  }
  const G1A s = {fq_mul(p.x, fq_const(G1_BETA)), fq_neg(p.y), false};
  return jac_eq_aff(g1d_to_jac(q), s);
}
ZG_DEC_INL inline bool g1_in_subgroup_d(const G1A& p) {
#if ZG_SUBGROUP_XX
  G1Hold hold;
  return g1_in_subgroup_xx(p, hold);
#else
  if (p.inf) return true;
  const FqD px = fqd_from(p.x), py = fqd_from(p.y);
  G1D q = g1d_from_aff(px, py);
  for (int i = 126; i >= 0; i--) {  // bit 127 of x^2 is the leading one
    q = g1d_dbl(q);
    if ((X2_ABS[i >> 5] >> (i & 31)) & 1u) q = g1d_add_aff(q, px, py);
  }
  const G1A s = {fq_mul(p.x, fq_const(G1_BETA)), fq_neg(p.y), false};
  return jac_eq_aff(g1d_to_jac(q), s);
#endif
}

}  // namespace zg
