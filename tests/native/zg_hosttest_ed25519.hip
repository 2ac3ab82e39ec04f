// TEST HARNESS ONLY -- runs the Ed25519 kernel's own per-item routine (zebra_amd/csrc/zg_ed25519.h) on
// the CPU, over a comb table built on the host by the comb kernel's entry routine, so the CPU-only test
// tier can check it against tests/ed25519_ref.py without a GPU. Never linked into, or loaded by, the
// product library.
#include <stdlib.h>
#include "../../zebra_amd/csrc/zg_ed25519.h"

using namespace zg;

static uint32_t* g_comb = nullptr;

extern "C" {

// status[i] = ed25519_verify_one of item i; the arguments of zg_ed25519_verify. Every item is copied
// into buffers of exactly its own lengths first, so a read outside the item is a read outside an
// allocation
int zgt_ed25519_verify(size_t n, const uint8_t* pubkey, const uint8_t* sig, const uint8_t* msg, uint8_t* status) {
  if (!g_comb) {
    uint32_t* t = (uint32_t*)malloc(sizeof(uint32_t) * ZG_ED_COMB_WORDS * ZG_ED_COMB_POINTS);
    if (!t) return -1;
    for (int i = 0; i < ZG_ED_COMB_POINTS; i++) ed_comb_entry(i, t + (size_t)i * ZG_ED_COMB_WORDS);
    g_comb = t;
  }
  for (size_t i = 0; i < n; i++) {
    uint8_t* pk = (uint8_t*)malloc(32);
    uint8_t* sg = (uint8_t*)malloc(64);
    uint8_t* m = (uint8_t*)malloc(32);
    if (!pk || !sg || !m) return -1;
    for (int k = 0; k < 32; k++) pk[k] = pubkey[32 * i + k], m[k] = msg[32 * i + k];
    for (int k = 0; k < 64; k++) sg[k] = sig[64 * i + k];
    status[i] = ed25519_verify_one(pk, sg, m, g_comb);
    free(pk);
    free(sg);
    free(m);
  }
  return 0;
}

// field 5 / 6 of zg_debug_field_mul: a b mod 2^255 - 19 / (a + b 2^256) mod l, 32-byte LE operands of
// any value
void zgt_ed25519_field_mul(int field, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  for (size_t i = 0; i < n; i++) {
    if (field == 5)
      ed_debug_fe_mul(out + 8 * i, a + 8 * i, b + 8 * i);
    else
      ed_debug_mod_l(out + 8 * i, a + 8 * i, b + 8 * i);
  }
}

}
