// TEST HARNESS ONLY -- the lane R-chain's digit-form steps (zebra_amd/csrc/zg_lines.h lsd_double /
// lsd_add, zg_fqd.h Fq2D) next to the word-form ls_double / ls_add, on the CPU. Built on demand by
// tests/test_digit_chains.py, once plain and once with -DZG_FQD_CHECK (every documented digit bound
// verified). Never linked into, or loaded by, the product library.
#include <string.h>
#include "../../zebra_amd/csrc/zg_lines.h"

using namespace zg;

static Fq ld_fq(const uint8_t* b) { return fq_to_mont(fq_limbs_from_be(b)); }
static void st_fq(const Fq& a, uint8_t* b) { fq_limbs_to_be(fq_from_mont(a), b); }
static void st_f2(const Fq2& v, uint8_t* o) {
  st_fq(v.c0, o);
  st_fq(v.c1, o + 48);
}

extern "C" {

// number of bound violations seen so far (always 0 in a build without ZG_FQD_CHECK)
int zgd_check_fails() {
#if defined(ZG_FQD_CHECK)
  return fqd_check_fails();
#else
  return 0;
#endif
}
int zgd_checking() {
#if defined(ZG_FQD_CHECK)
  return 1;
#else
  return 0;
#endif
}

// The chain of k_batch_lines_lane for one lane, in both forms: q = B (x.c0 x.c1 y.c0 y.c1), p = r A
// (x y), 48-byte BE each (any values below p); chk / act as in the kernel (a lane without a B to
// check starts from (1, 1, 1) and adds B all the same; an inactive lane writes identity lines).
// Per step (68): the three line coefficients (3 x 96 B) and the canonical (X, Y, Z) after the step
// (3 x 96 B), to out_w (word form) and out_d (digit form). res[0..1]: the closing G2 verdicts.
void zgd_chain(const uint8_t* q, const uint8_t* p, int chk, int act, uint8_t* out_w, uint8_t* out_d, int* res) {
  const G2A B = {{ld_fq(q), ld_fq(q + 48)}, {ld_fq(q + 96), ld_fq(q + 144)}, false};
  const G1A P = {ld_fq(p), ld_fq(p + 48), false};
  LinesHost w = {{chk ? B.x : f2_one(), chk ? B.y : f2_one(), f2_one()}};
  LinesHostD d;
  lsd_init(d, &B, chk != 0);
  Fq2 l[3];
  int n = 0;
  auto emit = [&](uint8_t* out, const G2J& r) {
    uint8_t* o = out + (size_t)n * 6 * 96;
    for (int j = 0; j < 3; j++) st_f2(l[j], o + j * 96);
    st_f2(r.x, o + 3 * 96);
    st_f2(r.y, o + 4 * 96);
    st_f2(r.z, o + 5 * 96);
  };
  for (int i = ZG_XH_TOP; i >= -1; i--) {
    ls_double(w, &P, l, act != 0);
    emit(out_w, G2J{w.get(0), w.get(1), w.get(2)});
    lsd_double(d, &P, l, act != 0);
    emit(out_d, lsd_result(d));
    n++;
    if (i >= 0 && ((ZG_XH >> i) & 1ull)) {
      ls_add(w, &B, &P, l, act && chk);
      emit(out_w, G2J{w.get(0), w.get(1), w.get(2)});
      lsd_add(d, &B, &P, l, act && chk);
      emit(out_d, lsd_result(d));
      n++;
    }
  }
  res[0] = ls_in_g2(G2J{w.get(0), w.get(1), w.get(2)}, B);
  res[1] = ls_in_g2(lsd_result(d), B);
  res[2] = n;
}

// the digit products against the word form on arbitrary canonical operands (48-byte BE):
// out = x y || x^2 || x s (96 B each) from the digit forms, ref the same from the word form
void zgd_products(const uint8_t* x, const uint8_t* y, const uint8_t* s, uint8_t* out, uint8_t* ref) {
  const Fq2 a = {ld_fq(x), ld_fq(x + 48)}, b = {ld_fq(y), ld_fq(y + 48)};
  const Fq sc = ld_fq(s);
  const Fq2D ad = f2d_from(a), bd = f2d_from(b);
  st_f2(f2d_to_w(f2d_mul<3>(ad, bd)), out);
  st_f2(f2d_to_w(f2d_sqr<3>(ad)), out + 96);
  st_f2(f2d_mulfq_to_w(ad, sc), out + 192);
  st_f2(f2d_to_w(f2d_mul_w22(ad, b)), out + 288);
  st_f2(f2d_mul_to_w(ad, b), out + 384);
  st_f2(ls_mul(a, b), ref);
  st_f2(ls_sqr(a), ref + 96);
  st_f2(ls_mulfq(a, sc), ref + 192);
  st_f2(ls_mul(a, b), ref + 288);
  st_f2(ls_mul(a, b), ref + 384);
}
}

// the store-parameterised two-column GLV product (zg_groth16.h g1_glv_mul_w2_t, plain-array store)
// against the one-column g1_glv_mul_d for an affine G1 point (x, y: 48-byte BE) and the scalar pair
// (a, b): out_d / out_w2 the affine results (96 B, zero bytes for infinity)
extern "C" void zgd_glv(const uint8_t* x, const uint8_t* y, uint64_t a, uint64_t b, uint8_t* out_d, uint8_t* out_w2) {
  const G1A p = {ld_fq(x), ld_fq(y), false};
  GlvTabHost tab;
  G1J w;
  g1_glv_mul_w2_t(&w, &p, a, b, tab);
  const G1A r[2] = {jac_to_aff(g1_glv_mul_d(p, a, b)), jac_to_aff(w)};
  uint8_t* o[2] = {out_d, out_w2};
  for (int k = 0; k < 2; k++) {
    memset(o[k], 0, 96);
    if (!r[k].inf) {
      st_fq(r[k].x, o[k]);
      st_fq(r[k].y, o[k] + 48);
    }
  }
}
