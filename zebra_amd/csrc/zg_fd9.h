// zg_fd9.h -- a prime field p = 2^BITS - C0 - [2^C1SH] in 9 unsaturated digits of 29 bits, once for
// the curves whose kernels run one lane per item:
//   Ed25519    p = 2^255 - 19             BITS = 255, C0 = 19,  no second term (C1SH = 0)   zg_ed25519.h
//   secp256k1  p = 2^256 - 2^32 - 977     BITS = 256, C0 = 977, C1SH = 32                   zg_ecdsa.h
// A curve header gives the three constants in a struct M and names Fd9<M>; everything else is derived
// here at compile time, and the second term is an `if constexpr`, never a run-time branch.
//
// A product is 81 carry-free v_mad_u64_u32 into 17 columns. The digit string is 261 bits long, so the
// fold is 2^261 = FOLD [+ 2^(29 + FOLD_SH)] (mod p) with FOLD = C0 2^(261 - BITS): 1216 for Ed25519;
// 31264 and a shift by 8 into the next digit for secp256k1, whose 2^37 + 31264 does not fit one
// 32-bit factor. The high columns are carried to 29-bit digits h, FOLD h goes into the low column of
// the same index (one multiply-add) and h 2^FOLD_SH into the next one (a shift), and one more carry
// pass finishes.
//   "tight" element: every digit < 2^29 + 2^14 (no second term) or < 2^29 + 2^21 (with one); this is
//   what every function here returns;
//   products accept digits < 1.4e9, i.e. also an uncarried sum of two tight elements (fd_add_nc):
//   9 x^2 plus the folds stay below 2^64; fd_sub takes tight operands only.
// No digit is ever masked narrower than 29 bits and the small factors are hidden behind zg_opaque, so
// no multiply-add sees two operands it knows to fit 24 bits (the compiler finding of DESIGN.md
// section 4; zg_debug_field_mul fields 5 and 7 are the guards).
#pragma once
#include "zg_field.h"

namespace zg {

ZG_INL uint64_t fd_mad(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }

template <class M>
struct Fd9 {
  static constexpr uint32_t MASK = 0x1fffffffu;
  static constexpr bool TWO = M::C1SH != 0;                     // p has the second term
  static constexpr uint32_t FOLD = M::C0 << (261 - M::BITS);    // 2^261 = FOLD + [2^(29 + FOLD_SH)]
  static constexpr int FOLD_SH = TWO ? M::C1SH + 261 - M::BITS - 29 : 0;
  static constexpr int TOP = M::BITS - 232;                     // bits of digit 8 below 2^BITS
  static constexpr uint32_t TOP_MASK = (1u << TOP) - 1u;
  static constexpr uint32_t C1 = TWO ? 1u << (M::C1SH - 29) : 0u;  // 2^C1SH in units of digit 1

  uint32_t d[9];

  ZG_INL static Fd9 zero() {
    Fd9 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.d[i] = 0;
    return r;
  }
  ZG_INL static Fd9 small(uint32_t v) {  // v < 2^29
    Fd9 r = zero();
    r.d[0] = v;
    return r;
  }
  ZG_INL static Fd9 one() { return small(1); }
  // a 256-bit integer (8 LE words, any value) -> digits (tight: the top digit has 24 bits)
  ZG_INL static Fd9 from_words(const uint32_t* w) {
    Fd9 r;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const int bit = 29 * k, wi = bit >> 5, sh = bit & 31;
      uint32_t v = w[wi] >> sh;
      if (sh > 3 && wi + 1 < 8) v |= w[wi + 1] << (32 - sh);
      r.d[k] = v & MASK;
    }
    return r;
  }
  // r += t 2^261 (t small enough for the digits it lands in)
  ZG_INL void fold_in(uint32_t t) {
    d[0] += t * FOLD;
    if constexpr (TWO) d[1] += t << FOLD_SH;
  }
  // carry digits 0..7 upwards; digit 8 keeps what it receives
  ZG_INL void ripple() {
#pragma unroll
    for (int k = 0; k < 8; k++) {
      d[k + 1] += d[k] >> 29;
      d[k] &= MASK;
    }
  }
};

// one carry pass with the 2^261 fold: digits < 2^31 in -> tight out (the value is unchanged mod p)
template <class M>
ZG_INL void fd_carry(Fd9<M>& r) {
  r.ripple();
  const uint32_t t = r.d[8] >> 29;
  r.d[8] &= Fd9<M>::MASK;
  r.fold_in(t);
}
template <class M>
ZG_INL Fd9<M> fd_add_nc(const Fd9<M>& a, const Fd9<M>& b) {  // a product operand only
  Fd9<M> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template <class M>
ZG_INL Fd9<M> fd_add(const Fd9<M>& a, const Fd9<M>& b) {
  Fd9<M> r = fd_add_nc(a, b);
  fd_carry(r);
  return r;
}
// a - b: a + 2 (2^261 - the fold) - b digit by digit: the offset's digits are 2^30 - 2 FOLD,
// 2^30 - 2 - [2 2^FOLD_SH], 2^30 - 2, ..., each >= a tight digit
template <class M>
ZG_INL Fd9<M> fd_sub(const Fd9<M>& a, const Fd9<M>& b) {
  using F = Fd9<M>;
  F r;
  r.d[0] = a.d[0] + (0x40000000u - 2u * F::FOLD) - b.d[0];
#pragma unroll
  for (int i = 1; i < 9; i++)
    r.d[i] = a.d[i] + (0x3ffffffeu - (F::TWO && i == 1 ? 2u << F::FOLD_SH : 0u)) - b.d[i];
  fd_carry(r);
  return r;
}
template <class M>
ZG_INL Fd9<M> fd_neg(const Fd9<M>& a) {
  return fd_sub(Fd9<M>::zero(), a);
}

// 17 columns (each < 2^64 - 2^59) -> tight element
template <class M>
ZG_INL Fd9<M> fd_fold(uint64_t* c) {
  using F = Fd9<M>;
  uint32_t h[9];
#pragma unroll
  for (int k = 9; k < 16; k++) {
    h[k - 9] = (uint32_t)c[k] & F::MASK;
    c[k + 1] += c[k] >> 29;
  }
  h[7] = (uint32_t)c[16] & F::MASK;
  h[8] = (uint32_t)(c[16] >> 29);  // < 2^32 by the operand bound
  uint32_t f = F::FOLD;
  zg_opaque(f);
#pragma unroll
  for (int k = 0; k < 9; k++) c[k] = fd_mad(h[k], f, c[k]);
  uint64_t c9 = 0;
  if constexpr (F::TWO) {
#pragma unroll
    for (int k = 0; k < 8; k++) c[k + 1] += (uint64_t)h[k] << F::FOLD_SH;
    c9 = (uint64_t)h[8] << F::FOLD_SH;
  }
  F r;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    r.d[k] = (uint32_t)c[k] & F::MASK;
    c[k + 1] += c[k] >> 29;
  }
  r.d[8] = (uint32_t)c[8] & F::MASK;
  c9 += c[8] >> 29;  // < 2^35 (< 2^41 with the second term): folds into digits 0, 1 (and 2)
  uint32_t tl = (uint32_t)c9 & F::MASK, th = (uint32_t)(c9 >> 29);
  zg_opaque(th);
  const uint64_t c0 = fd_mad(tl, f, r.d[0]);
  uint64_t c1 = (uint64_t)r.d[1] + (c0 >> 29);
  if constexpr (F::TWO) c1 += (uint64_t)tl << F::FOLD_SH;
  c1 = fd_mad(th, f, c1);
  r.d[0] = (uint32_t)c0 & F::MASK;
  r.d[1] = (uint32_t)c1 & F::MASK;
  r.d[2] += (uint32_t)(c1 >> 29);
  if constexpr (F::TWO) r.d[2] += th << F::FOLD_SH;
  return r;
}

template <class M>
ZG_INL Fd9<M> fd_mul(const Fd9<M>& a, const Fd9<M>& b) {
  uint64_t c[17];
#pragma unroll
  for (int k = 0; k < 17; k++) {
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int j = k - i;
      if (j < 0 || j > 8) continue;
      s = fd_mad(a.d[i], b.d[j], s);
    }
    c[k] = s;
  }
  return fd_fold<M>(c);
}
template <class M>
ZG_INL Fd9<M> fd_sqr(const Fd9<M>& a) {
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
      s = fd_mad(i < j ? a2[i] : a.d[i], a.d[j], s);
    }
    c[k] = s;
  }
  return fd_fold<M>(c);
}
template <class M>
ZG_INL Fd9<M> fd_sqr_n(Fd9<M> a, int n) {
  for (int i = 0; i < n; i++) a = fd_sqr(a);
  return a;
}

// the canonical value (< p) as 8 LE words
template <class M>
ZG_INL void fd_canon(const Fd9<M>& a, uint32_t* w) {
  using F = Fd9<M>;
  F t = a;
  fd_carry(t);
  fd_carry(t);  // every digit < 2^29: the value is < 2^261
  const uint32_t q = t.d[8] >> F::TOP;
  t.d[8] &= F::TOP_MASK;
  t.d[0] += M::C0 * q;  // 2^BITS = C0 + [2^C1SH]
  if constexpr (F::TWO) t.d[1] += q * F::C1;
  t.ripple();
  // t < 2^BITS + 2^38: t >= p iff t + C0 + [2^C1SH] reaches bit BITS
  F u = t;
  u.d[0] += M::C0;
  if constexpr (F::TWO) u.d[1] += F::C1;
  u.ripple();
  const bool ge = (u.d[8] >> F::TOP) != 0;
  u.d[8] &= F::TOP_MASK;
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
template <class M>
ZG_INL bool fd_eq(const Fd9<M>& a, const Fd9<M>& b) {
  uint32_t x[8], y[8], acc = 0;
  fd_canon(a, x);
  fd_canon(b, y);
#pragma unroll
  for (int i = 0; i < 8; i++) acc |= x[i] ^ y[i];
  return acc == 0;
}
template <class M>
ZG_INL bool fd_is_zero(const Fd9<M>& a) {
  uint32_t x[8], acc = 0;
  fd_canon(a, x);
#pragma unroll
  for (int i = 0; i < 8; i++) acc |= x[i];
  return acc == 0;
}

}  // namespace zg
