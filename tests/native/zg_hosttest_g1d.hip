// TEST HARNESS ONLY -- the lazy-digit G1 point formulas (zebra_amd/csrc/zg_fqd.h fqd_dot2, g1d_dbl,
// g1d_add_aff, g1d_add_full, g1d_readd, g1_in_subgroup_d) next to the word-form jac_dbl / jac_add /
// g1_in_subgroup, on the CPU. Built on demand by tests/test_g1_digit_chains.py, once plain and once
// with -DZG_FQD_CHECK (every documented digit bound verified). Never linked into, or loaded by, the
// product library.
#include <string.h>
#include "../../zebra_amd/csrc/zg_groth16.h"

using namespace zg;

static Fq ld_fq(const uint8_t* b) { return fq_to_mont(fq_limbs_from_be(b)); }
static void st_fq(const Fq& a, uint8_t* b) { fq_limbs_to_be(fq_from_mont(a), b); }
// 97 bytes: 1 for infinity, then the canonical affine x, y (zero bytes for infinity)
static void st_aff(const G1J& j, uint8_t* o) {
  const G1A a = jac_to_aff(j);
  memset(o, 0, 97);
  o[0] = a.inf;
  if (!a.inf) {
    st_fq(a.x, o + 1);
    st_fq(a.y, o + 49);
  }
}

extern "C" {

// number of bound violations seen so far (always 0 in a build without ZG_FQD_CHECK)
int zgg_check_fails() {
#if defined(ZG_FQD_CHECK)
  return fqd_check_fails();
#else
  return 0;
#endif
}
int zgg_checking() {
#if defined(ZG_FQD_CHECK)
  return 1;
#else
  return 0;
#endif
}
int zgg_dot2_on() { return ZG_G1D_DOT2; }

// fqd_dot2 on raw digits: in = a, b, c, d (4 x 14 digits, each normalized, any value), raw = the 14
// output digits, canon = the output through fqd_to, as 48-byte BE (the output times 2^-406 mod p;
// only for outputs below 2^21 p, do_canon = 0 otherwise)
void zgg_dot2(const uint32_t* in, uint32_t* raw, int do_canon, uint8_t* canon) {
  FqD v[4];
  for (int k = 0; k < 4; k++)
    for (int i = 0; i < 14; i++) v[k].d[i] = in[14 * k + i];
  const FqD r = fqd_dot2(v[0], v[1], v[2], v[3]);
  for (int i = 0; i < 14; i++) raw[i] = r.d[i];
  if (do_canon) st_fq(fqd_to(r), canon);
}

// One walk of point operations from one state, in lazy digits (G1D, never canonicalised between the
// steps: the invariant carries from each formula's output to the next one's input) and in the word
// form. start: affine x || y (96 B BE) or the point at infinity (start_inf); q: an affine, finite
// point. After every step the canonical affine point of both forms goes to out_d / out_w (97 B).
//   0 s = 2s          1 s += q (mixed)       2 T = s (with T.z^2, T.z^3 cached)   3 s += T (full)
//   4 s += T (cached) 5 T = infinity         6 s += -q (mixed, the lazy 3p - y)   7 s += q (full)
void zgg_walk(const uint8_t* start, int start_inf, const uint8_t* q, const uint8_t* ops, int n, uint8_t* out_d,
              uint8_t* out_w) {
  const G1A qa = {ld_fq(q), ld_fq(q + 48), false};
  const G1A nqa = {qa.x, fq_neg(qa.y), false};
  const FqD qx = fqd_from(qa.x), qy = fqd_from(qa.y);
  G1D s = g1d_infinity();
  G1J w = jac_infinity<Fq>();
  if (!start_inf) {
    const G1A sa = {ld_fq(start), ld_fq(start + 48), false};
    s = g1d_from_aff(fqd_from(sa.x), fqd_from(sa.y));
    w = jac_from_aff(sa);
  }
  G1D T = g1d_infinity();
  G1J Tw = jac_infinity<Fq>();
  FqD zz = fqd_zero(), zc = fqd_zero();
  for (int k = 0; k < n; k++) {
    switch (ops[k]) {
      case 0:
        s = g1d_dbl(s);
        w = jac_dbl(w);
        break;
      case 1:
        s = g1d_add_aff(s, qx, qy);
        w = jac_add_aff(w, qa);
        break;
      case 2:
        T = s;
        Tw = w;
        zz = fqd_sqr(s.z);
        zc = fqd_mul(s.z, zz);
        break;
      case 3:
        s = g1d_add_full(s, T);
        w = jac_add(w, Tw);
        break;
      case 4:
        s = g1d_readd(s, T, zz, zc);
        w = jac_add(w, Tw);
        break;
      case 5:
        T = g1d_infinity();
        Tw = jac_infinity<Fq>();
        zz = zc = fqd_zero();
        break;
      case 6:
        s = g1d_add_aff(s, qx, fqd_neg2(qy));
        w = jac_add_aff(w, nqa);
        break;
      default:
        s = g1d_add_full(s, g1d_from_aff(qx, qy));
        w = jac_add(w, jac_from_aff(qa));
        break;
    }
    st_aff(g1d_to_jac(s), out_d + (size_t)k * 97);
    st_aff(w, out_w + (size_t)k * 97);
  }
}

// the subgroup check of an affine curve point: bit 0 g1_in_subgroup_d (the build's default walk),
// bit 1 the word-form g1_in_subgroup, bit 2 the two walks of |x| (g1_in_subgroup_xx, plain store)
int zgg_subgroup(const uint8_t* x, const uint8_t* y) {
  const G1A p = {ld_fq(x), ld_fq(y), false};
  G1Hold hold;
  return (g1_in_subgroup_d(p) ? 1 : 0) | (g1_in_subgroup(p) ? 2 : 0) | (g1_in_subgroup_xx(p, hold) ? 4 : 0);
}
}
