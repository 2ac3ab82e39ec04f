// zg_lines.h -- the straight-line R-chain step functions (lane = proof): pairing 0.14.2's
// doubling_step / addition_step (zg_pairing.h line_double / line_add, the same formulas) in the
// 29-bit-digit Fq2 products, each scaled line coefficient stored as soon as it is known. Used by
// k_batch_lines_lane (zg_lines.hip); __host__ __device__, so tests/native runs the same code.
#pragma once
#include <stddef.h>
#include "zg_batch.h"

// ZG_LINES_FQD (default 1): k_batch_lines_lane walks the chain in lazy digits (lsd_double / lsd_add
// below); 0: the word-form steps (ls_double / ls_add), kept for A/B runs (tools/build_variant.py) and
// as the comparison of tests/native/zg_hosttest_digit.hip
#ifndef ZG_LINES_FQD
#define ZG_LINES_FQD 1
#endif

namespace zg {

// x^2 (canonical x), x y (x < 2p per coefficient, y canonical), x s: the 29-bit-digit forms.
// Each product is fenced by scheduling barriers: the scheduler would otherwise interleave the
// independent products of a step for ILP and keep all their digit vectors live at once (742
// spilled VGPRs); fenced, only the step's live values plus one product's digits are resident.
#if defined(__HIP_DEVICE_COMPILE__)
#define LS_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define LS_FENCE() ((void)0)
#endif
ZG_INL Fq2 ls_sqr(const Fq2& a) {
  LS_FENCE();
  const Fq d = fq_sub(a.c0, a.c1);
  Fq2 r;
  f2_sqr29(r.c0.l, r.c1.l, a.c0.l, a.c1.l, d.l);
  LS_FENCE();
  return r;
}
ZG_INL Fq2 ls_mul(const Fq2& a, const Fq2& b) {
  LS_FENCE();
  Fq2 r;
  f2_mul29(r.c0.l, r.c1.l, a.c0.l, a.c1.l, b.c0.l, b.c1.l);
  LS_FENCE();
  return r;
}
ZG_INL Fq2 ls_mulfq(const Fq2& a, const Fq& s) {
  LS_FENCE();
  Fq2 r;
  f2_mul_fq29(r.c0.l, r.c1.l, a.c0.l, a.c1.l, s.l);
  LS_FENCE();
  return r;
}

// The running point R = (X, Y, Z) lives in a per-lane state store St (get / put of coordinate 0, 1,
// 2): LDS on the device (LinesLds, conflict-free lane-contiguous rows), a plain struct on the host.
// Each coordinate is read where a product needs it and rewritten as soon as its new value is known,
// so registers hold at most four step temporaries next to one product's digits: the step fits 256
// VGPRs (two waves per SIMD) without the 672 B/lane of scratch spills of round 3's register-resident
// state.
struct LinesHost {
  Fq2 v[3];
  ZG_HD Fq2 get(int i) const { return v[i]; }
  ZG_HD void put(int i, const Fq2& x) { v[i] = x; }
};

// pairing doubling_step (line_double of zg_pairing.h), the scaled line stored as soon as each
// coefficient is known. tmp4 = 3 tmp0 is re-formed where used (two additions) instead of held.
template <class St>
ZG_INL void ls_double(St& st, const G1A* pa, Fq2* dst, bool act) {
  const Fq2 tmp1 = ls_sqr(st.get(1));
  const Fq2 zsq = ls_sqr(st.get(2));
  {
    const Fq2 nz = f2_sub(f2_sub(ls_sqr(f2_add(st.get(2), st.get(1))), tmp1), zsq);
    dst[2] = act ? ls_mulfq(f2_dbl(ls_mul(nz, zsq)), pa->y) : f2_one();  // c0 py
    st.put(2, nz);
  }
  const Fq2 tmp0 = ls_sqr(st.get(0));
  dst[1] = act ? ls_mulfq(f2_neg(f2_dbl(ls_mul(f2_add(f2_dbl(tmp0), tmp0), zsq))), pa->x) : f2_one();  // c1 px
  const Fq2 tmp5 = ls_sqr(f2_add(f2_dbl(tmp0), tmp0));
  dst[0] = act ? f2_sub(f2_sub(f2_sub(ls_sqr(f2_add(st.get(0), f2_add(f2_dbl(tmp0), tmp0))), tmp0), tmp5),
                        f2_dbl(f2_dbl(tmp1)))
               : f2_one();
  const Fq2 tmp2 = ls_sqr(tmp1);
  const Fq2 tmp3 = f2_dbl(f2_sub(f2_sub(ls_sqr(f2_add(tmp1, st.get(0))), tmp0), tmp2));
  const Fq2 nx = f2_sub(f2_sub(tmp5, tmp3), tmp3);
  st.put(0, nx);
  st.put(1, f2_sub(ls_mul(f2_sub(tmp3, nx), f2_add(f2_dbl(tmp0), tmp0)), f2_dbl(f2_dbl(f2_dbl(tmp2)))));
}

// pairing addition_step (line_add of zg_pairing.h) with q affine (read from HBM where used), scaled
// line. qy^2 is formed twice (one squaring per addition step, 5 per loop) instead of held.
template <class St>
ZG_INL void ls_add(St& st, const G2A* pq, const G1A* pa, Fq2* dst, bool act) {
  const Fq2 zsq = ls_sqr(st.get(2));
  const Fq2 t2 = f2_sub(ls_mul(zsq, pq->x), st.get(0));
  const Fq2 t6 = f2_sub(f2_sub(ls_mul(f2_sub(f2_sub(ls_sqr(f2_add(pq->y, st.get(2))), ls_sqr(pq->y)), zsq), zsq),
                               st.get(1)),
                        st.get(1));
  const Fq2 t3 = ls_sqr(t2);
  st.put(2, f2_sub(f2_sub(ls_sqr(f2_add(st.get(2), t2)), zsq), t3));  // nz
  dst[2] = act ? ls_mulfq(f2_dbl(st.get(2)), pa->y) : f2_one();       // c0 py
  dst[1] = act ? ls_mulfq(f2_dbl(f2_neg(t6)), pa->x) : f2_one();      // c1 px
  {
    const Fq2 nz = st.get(2);
    const Fq2 t10 = f2_sub(f2_sub(ls_sqr(f2_add(pq->y, nz)), ls_sqr(pq->y)), ls_sqr(nz));
    dst[0] = act ? f2_sub(f2_dbl(ls_mul(t6, pq->x)), t10) : f2_one();
  }
  const Fq2 t4 = f2_dbl(f2_dbl(t3));
  const Fq2 t5 = ls_mul(t4, t2);
  const Fq2 t7 = ls_mul(t4, st.get(0));
  const Fq2 nx = f2_sub(f2_sub(f2_sub(ls_sqr(t6), t5), t7), t7);
  const Fq2 ny = f2_sub(ls_mul(f2_sub(t7, nx), t6), f2_dbl(ls_mul(st.get(1), t5)));
  st.put(0, nx);
  st.put(1, ny);
}

// B in G2 given r = [x] B (Jacobian, canonical): psi(B) = [u] B = -[x] B  <=>  X = psi_x Z^2,
// Y = -psi_y Z^3, Z != 0 (the step formulas are exact unless they degenerate, which only a B outside
// G2 can make happen, and then Z = 0)
ZG_INL bool ls_in_g2(const G2J& r, const G2A& q) {
  const G2A s = g2_psi(q);
  const Fq2 z2 = ls_sqr(r.z), z3 = ls_mul(z2, r.z);
  return !f2_is_zero(r.z) && f2_eq(r.x, ls_mul(s.x, z2)) && f2_eq(r.y, f2_neg(ls_mul(s.y, z3)));
}

// ---- the digit-resident R-chain (ZG_LINES_FQD, zg_fqd.h Fq2D) ----
// The same two steps with (X, Y, Z) and every temporary as Fq2D: 14 lazy 29-bit digits per
// coefficient in Montgomery form R' = 2^406, never reduced mod p. A product splits, repacks and
// canonicalises nothing; sums and differences are digit-wise with one carry normalization, and the
// comments give each value's bound in units of p. Only what leaves the chain is canonical:
//   c0 py, c1 px   the scalar product takes px / py as the word form's own digits (R = 2^384), so
//                  REDC' returns the word form's Montgomery value directly (f2d_mulfq_to_w);
//   c2 (doubling)  one 22-bit Montgomery step (f2d_to_w: 14 m p products per coefficient);
//   c2 (addition)  both of its products take the word-form qx / qy (f2d_mul_to_w).
// The addition step's (qy + Z)^2 - qy^2 - Z^2 is formed as the product 2 qy Z (the same value mod p
// for one product instead of two squarings; the word form squares because pairing does).
// px, py, qx and qy are NOT held as digits across the chain (the issue that asked for this chain
// proposed converting them once per proof): 4 x 14 more live registers would not fit beside a step's
// temporaries at 256 VGPRs, and LDS is full (19.5 of 20 KB). They are re-read from memory (L1 / L2
// hits, as the word form re-reads them) and split where a product takes them, about 14 VALU
// instructions per operand -- a split only, never a conversion product.
// Invariant of the state between steps: X < 31p, Y < 19p, Z < 7p, normalized (after an addition
// step X < 9p, Y < 7p, Z < 7p; the first step starts from X, Y < 2p, Z = 1). So the top digit of a
// stored coordinate is below 31 * 14 < 2^9 (LinesPackD).
ZG_INL Fq2D lsd_fence(const Fq2D& r) {
  LS_FENCE();
  return r;
}
#define LSD_PRODUCT(expr) (LS_FENCE(), lsd_fence(expr))

// A stored coordinate: 2 x 13 words, the top digit (< 2^9) in bits 29..31 of digits 0, 1, 2
struct LinesPackD {
  uint32_t w[26];
};
ZG_INL void lsd_pack1(uint32_t* w, const FqD& a) {
  const uint32_t t = a.d[13];
#pragma unroll
  for (int i = 0; i < 13; i++) w[i] = a.d[i];
  w[0] |= t << 29;
  w[1] |= (t >> 3) << 29;
  w[2] |= (t >> 6) << 29;
}
ZG_INL FqD lsd_unpack1(const uint32_t* w) {
  FqD a;
#pragma unroll
  for (int i = 0; i < 13; i++) a.d[i] = w[i] & FQ29_MASK;
  a.d[13] = (w[0] >> 29) | ((w[1] >> 29) << 3) | ((w[2] >> 29) << 6);
  return a;
}
ZG_INL LinesPackD lsd_pack(const Fq2D& a) {
  F2D_CHK(a, 36);  // top digit < 2^9
  LinesPackD p;
  lsd_pack1(p.w, a.c0);
  lsd_pack1(p.w + 13, a.c1);
  return p;
}
ZG_INL Fq2D lsd_unpack(const LinesPackD& p) { return {lsd_unpack1(p.w), lsd_unpack1(p.w + 13)}; }

// the host's state store (the device's is LinesLdsD of zg_lines.hip): the same packed words
struct LinesHostD {
  LinesPackD v[3];
  ZG_HD Fq2D get(int i) const { return lsd_unpack(v[i]); }
  ZG_HD void put(int i, const Fq2D& x) { v[i] = lsd_pack(x); }
  ZG_HD void put1(int i, int coef, const FqD& x) { lsd_pack1(v[i].w + 13 * coef, x); }
};

// ls_double in digits. In: the invariant. Out: X < 31p, Y < 19p, Z < 7p.
template <class St>
ZG_INL void lsd_double(St& st, const G1A* pa, Fq2* dst, bool act) {
  const Fq2D tmp1 = LSD_PRODUCT(f2d_sqr<20>(st.get(1)));                         // Y^2: < 2
  const Fq2D zsq = LSD_PRODUCT(f2d_sqr<8>(st.get(2)));                           // Z^2: < 2
  F2D_CHK(tmp1, 2);
  F2D_CHK(zsq, 2);
  {
    const Fq2D s = f2d_add(st.get(2), st.get(1));                                // Z + Y: < 26
    const Fq2D nz = f2d_sub2<5>(LSD_PRODUCT(f2d_sqr<27>(s)), tmp1, zsq);         // - Y^2 - Z^2 + 5p: < 7
    F2D_CHK(s, 26);
    F2D_CHK(nz, 7);
    const Fq2D m = LSD_PRODUCT(f2d_mul<3>(nz, zsq));                             // < 2
    F2D_CHK(m, 2);
    // (py split from memory here, on purpose: see the note on px, py, qx, qy above)
    dst[2] = act ? f2d_mulfq_to_w(f2d_dbl_raw(m), pa->y) : f2_one();             // c0 py = 2 nz Z^2 py
    LS_FENCE();
    st.put(2, nz);
  }
  const Fq2D tmp0 = LSD_PRODUCT(f2d_sqr<32>(st.get(0)));                         // X^2: < 2
  const Fq2D e3 = f2d_smul<3>(tmp0);                                             // tmp4 = 3 X^2: < 6
  F2D_CHK(tmp0, 2);
  F2D_CHK(e3, 6);
  {
    const Fq2D m = LSD_PRODUCT(f2d_mul<3>(e3, zsq));                             // < 2
    F2D_CHK(m, 2);
    dst[1] = act ? f2d_mulfq_to_w(f2d_negdbl_raw<5>(m), pa->x) : f2_one();       // c1 px = (5p - 2m) px
    LS_FENCE();
  }
  const Fq2D tmp5 = LSD_PRODUCT(f2d_sqr<7>(e3));                                 // < 2
  F2D_CHK(tmp5, 2);
  {
    const Fq2D s = f2d_add(st.get(0), e3);                                       // X + tmp4: < 37
    const Fq2D q = LSD_PRODUCT(f2d_sqr<38>(s));                                  // < 2
    // c2 = tmp6 - tmp0 - tmp5 - 4 tmp1 + 13p: < 15 (the subtrahends < 2 + 2 + 8)
    const Fq2D c2 = {fqd_sub114<13>(q.c0, tmp0.c0, tmp5.c0, tmp1.c0), fqd_sub114<13>(q.c1, tmp0.c1, tmp5.c1, tmp1.c1)};
    F2D_CHK(s, 37);
    F2D_CHK(c2, 15);
    dst[0] = act ? f2d_to_w(c2) : f2_one();
    LS_FENCE();
  }
  const Fq2D tmp2 = LSD_PRODUCT(f2d_sqr<3>(tmp1));                               // < 2
  F2D_CHK(tmp2, 2);
  const Fq2D s3 = f2d_add(tmp1, st.get(0));                                      // tmp1 + X: < 33
  // tmp3 = 2 ((tmp1 + X)^2 - tmp0 - tmp2 + 5p): < 14
  const Fq2D tmp3 = f2d_smul<2>(f2d_sub2<5>(LSD_PRODUCT(f2d_sqr<34>(s3)), tmp0, tmp2));
  const Fq2D nx = f2d_sub<29, 1, 2>(tmp5, tmp3);                                 // tmp5 - 2 tmp3 + 29p: < 31
  F2D_CHK(s3, 33);
  F2D_CHK(tmp3, 14);
  F2D_CHK(nx, 31);
  st.put(0, nx);
  const Fq2D d = f2d_sub<32, 1, 1>(tmp3, nx);                                    // tmp3 - X3 + 32p: < 46
  const Fq2D ny = f2d_sub<17, 1, 1>(LSD_PRODUCT(f2d_mul<7>(d, e3)), f2d_smul<8>(tmp2));  // - 8 tmp2 + 17p: < 19
  F2D_CHK(d, 46);
  F2D_CHK(ny, 19);
  st.put(1, ny);
}

// ls_add in digits, q affine in the word form (read where used). In: the invariant.
// Out: X < 9p, Y < 7p, Z < 7p.
template <class St>
ZG_INL void lsd_add(St& st, const G2A* pq, const G1A* pa, Fq2* dst, bool act) {
  const Fq2D zsq = LSD_PRODUCT(f2d_sqr<8>(st.get(2)));                           // < 2
  F2D_CHK(zsq, 2);
  // (qx, qy split from memory at each use, on purpose: see the note on px, py, qx, qy above)
  const Fq2D t2 = f2d_sub<32, 1, 1>(LSD_PRODUCT(f2d_mul_w22(zsq, pq->x)), st.get(0));  // qx Z^2 - X + 32p: < 34
  F2D_CHK(t2, 34);
  Fq2D t6;
  {
    const Fq2D yz = LSD_PRODUCT(f2d_mul_w22(st.get(2), pq->y));                  // qy Z (|Z| < 7): < 3
    F2D_CHK(yz, 3);
    const Fq2D m = LSD_PRODUCT(f2d_mul<3>(yz, zsq));                             // < 2
    t6 = f2d_sub<39, 2, 2>(m, st.get(1));                                        // 2 qy Z^3 - 2Y + 39p: < 43
    F2D_CHK(m, 2);
    F2D_CHK(t6, 43);
  }
  const Fq2D t3 = LSD_PRODUCT(f2d_sqr<35>(t2));                                  // < 2
  F2D_CHK(t3, 2);
  {
    const Fq2D s = f2d_add(st.get(2), t2);                                       // Z + t2: < 41
    const Fq2D nz = f2d_sub2<5>(LSD_PRODUCT(f2d_sqr<42>(s)), zsq, t3);           // < 7
    F2D_CHK(s, 41);
    F2D_CHK(nz, 7);
    st.put(2, nz);
  }
  const Fq2D t4 = f2d_smul<4>(t3);                                               // < 8
  const Fq2D t5 = LSD_PRODUCT(f2d_mul<35>(t4, t2));                              // < 2
  const Fq2D t7 = LSD_PRODUCT(f2d_mul<32>(t4, st.get(0)));                       // < 2
  F2D_CHK(t4, 8);
  F2D_CHK(t5, 2);
  F2D_CHK(t7, 2);
  const Fq2D nx = f2d_sub2<7>(LSD_PRODUCT(f2d_sqr<44>(t6)), t5, f2d_smul<2>(t7));  // t6^2 - t5 - 2 t7 + 7p: < 9
  F2D_CHK(nx, 9);
  st.put(0, nx);
  const Fq2D d = f2d_sub<10, 1, 1>(t7, nx);                                      // t7 - X3 + 10p: < 12
  const Fq2D m2 = LSD_PRODUCT(f2d_mul<3>(st.get(1), t5));                        // Y t5: < 2
  const Fq2D m1 = LSD_PRODUCT(f2d_mul<44>(d, t6));                               // < 2
  const Fq2D ny = f2d_sub<5, 1, 2>(m1, m2);                                      // - 2 Y t5 + 5p: < 7
  F2D_CHK(d, 12);
  F2D_CHK(m1, 2);
  F2D_CHK(m2, 2);
  F2D_CHK(ny, 7);
  st.put(1, ny);
  // the line, last: only t6 and the new Z (re-read) are still needed, so the step's other
  // temporaries are dead while the four line products run
  dst[1] = act ? f2d_mulfq_to_w(f2d_negdbl_raw<87>(t6), pa->x) : f2_one();       // c1 px = (87p - 2 t6) px
  LS_FENCE();
  // c2 = 2 t6 qx - t10, t10 = (qy + nz)^2 - qy^2 - nz^2 = 2 qy nz
  const Fq2 a = f2d_mul_to_w(t6, pq->x);
  LS_FENCE();
  const Fq2D nz = st.get(2);
  dst[2] = act ? f2d_mulfq_to_w(f2d_dbl_raw(nz), pa->y) : f2_one();              // c0 py = 2 nz py
  LS_FENCE();
  const Fq2 t10 = f2_dbl(f2d_mul_to_w(nz, pq->y));
  LS_FENCE();
  dst[0] = act ? f2_sub(f2_dbl(a), t10) : f2_one();
}

// the chain's start: B (or (1, 1) for a lane without a B to check) and Z = 1, in digits
template <class St>
ZG_INL void lsd_init(St& st, const G2A* pq, bool chk) {
  if (chk) {
    // x.c0, x.c1, y.c0, y.c1 as one array of four Fq: the layout this indexing relies on
    static_assert(offsetof(G2A, x) == 0 && offsetof(G2A, y) == 2 * sizeof(Fq) && sizeof(Fq2) == 2 * sizeof(Fq) &&
                      offsetof(Fq2, c1) == sizeof(Fq),
                  "G2A coordinates are four contiguous Fq");
    const Fq* c = reinterpret_cast<const Fq*>(pq);
#pragma nounroll
    for (int k = 0; k < 4; k++) {  // one conversion's code for the four coefficients
      LS_FENCE();
      const FqD v = fqd_from(c[k]);  // < 2
      LS_FENCE();
      st.put1(k >> 1, k & 1, v);
    }
  } else {
    st.put(0, f2d_one());
    st.put(1, f2d_one());
  }
  st.put(2, f2d_one());
}
// the chain's end: [x] B as a canonical Jacobian point
template <class St>
ZG_INL G2J lsd_result(const St& st) {
  return {f2d_to_w(st.get(0)), f2d_to_w(st.get(1)), f2d_to_w(st.get(2))};
}

// ---- the affine R-chain (ZG_LINES_AFFINE, round 6; zg_lines.hip k_batch_lines_aff) ----
// Fq products in 29-bit digits, fenced like the Fq2 ones above
ZG_INL Fq ls_fqmul(const Fq& a, const Fq& b) {
  LS_FENCE();
  Fq r;
  fq29_mul(r.l, a.l, b.l);
  LS_FENCE();
  return r;
}
ZG_INL Fq ls_fqsqr(const Fq& a) {
  LS_FENCE();
  Fq r;
  fq29_sqr(r.l, a.l);
  LS_FENCE();
  return r;
}
// N(d) = d0^2 + d1^2 (u^2 = -1): 1 / d = conj(d) / N(d); N(d) = 0 only for d = 0 (-1 is a non-residue mod p)
ZG_INL Fq ls_norm(const Fq2& d) { return fq_add(ls_fqsqr(d.c0), ls_fqsqr(d.c1)); }

// the G2 generator (Montgomery): the point an R-chain lane without a B to check walks, so that its
// denominators never vanish (its lines are not used)
ZG_HD inline G2A g2_generator() {
  static constexpr uint32_t X0[12] = {0x02940a10u, 0xf5f28fa2u, 0x87b4961au, 0xb3f5fb26u, 0x3e2ae580u, 0xa1a893b5u,
                                      0x1a3caee9u, 0x9894999du, 0x1863366bu, 0x6f67b763u, 0x4350bcd7u, 0x05819192u};
  static constexpr uint32_t X1[12] = {0x9e23f606u, 0xa5a9c075u, 0xbccd60c3u, 0xaaa0c59du, 0xe2867806u, 0x3bb17e18u,
                                      0x8541b367u, 0x1b1ab6ccu, 0xf2158547u, 0xc2b6ed0eu, 0x7360edf3u, 0x11922a09u};
  static constexpr uint32_t Y0[12] = {0x60494c4au, 0x4c730af8u, 0x5e369c5au, 0x597cfa1fu, 0xaa0a635au, 0xe7e6856cu,
                                      0x6e0d495fu, 0xbbefb5e9u, 0xf0ef25a2u, 0x07d3a975u, 0x7e80dae5u, 0x0083fd8eu};
  static constexpr uint32_t Y1[12] = {0xdf64b05du, 0xadc0fc92u, 0x2b1461dcu, 0x18aa270au, 0x3be4eba0u, 0x86adac6au,
                                      0xc93da33au, 0x79495c4eu, 0xa43ccaedu, 0xe7175850u, 0x63de1bf2u, 0x0b2bc2a1u};
  G2A g;
  for (int i = 0; i < 12; i++) {
    g.x.c0.l[i] = X0[i];
    g.x.c1.l[i] = X1[i];
    g.y.c0.l[i] = Y0[i];
    g.y.c1.l[i] = Y1[i];
  }
  g.inf = false;
  return g;
}

// One affine step of G2Prepared's chain, given 1 / N(d) for its denominator d (2y for a doubling,
// xQ - x for an addition): lambda = num conj(d) / N(d), (x, y) <- (lambda^2 - x - x', lambda (x - x3) - y),
// and the line through the point with slope lambda normalised by its v w coefficient and by py:
//   a = (lambda x - y) / py, b = -lambda px / py   (ab = (1/py, px/py); 0 for a proof without a line:
//   the line v w, FE-trivial). Same group law as ls_double / ls_add (pairing's doubling_step /
//   addition_step, which give these lines times an element of Fq2).
ZG_INL void ls_aff_step(Fq2& x, Fq2& y, const G2A* q, bool dbl, const Fq& ninv, const Fq2& ab, Fq2* a_out,
                        Fq2* b_out) {
  const Fq2 d = dbl ? f2_dbl(y) : f2_sub(q->x, x);
  const Fq2 dinv = ls_mulfq(f2_conj(d), ninv);
  Fq2 num;
  if (dbl) {
    const Fq2 x2 = ls_sqr(x);
    num = f2_add(f2_dbl(x2), x2);
  } else {
    num = f2_sub(q->y, y);
  }
  const Fq2 lam = ls_mul(num, dinv);
  const Fq2 x3 = f2_sub(ls_sqr(lam), dbl ? f2_dbl(x) : f2_add(x, q->x));
  const Fq2 c2 = f2_sub(ls_mul(lam, x), y);
  *a_out = ls_mulfq(c2, ab.c0);
  *b_out = f2_neg(ls_mulfq(lam, ab.c1));
  y = f2_sub(c2, ls_mul(lam, x3));
  x = x3;
}

}  // namespace zg
