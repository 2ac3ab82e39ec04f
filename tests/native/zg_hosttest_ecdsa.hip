// TEST HARNESS ONLY -- runs the ECDSA kernel's own per-item routine (zebra_amd/csrc/zg_ecdsa.h) on the
// CPU, over a comb table built on the host by the comb kernel's entry routine, so the CPU-only test
// tier can check it against tests/ecdsa_ref.py without a GPU. Never linked into, or loaded by, the
// product library.
#include <stdlib.h>
#include "../../zebra_amd/csrc/zg_ecdsa.h"

using namespace zg;

static uint32_t* g_comb = nullptr;

extern "C" {

// status[i] = ecdsa_verify_one of item i; the arguments of zg_ecdsa_verify. Every item is copied
// into a buffer of exactly its own length first, so a read outside the item is a read outside an
// allocation
int zgt_ecdsa_verify(size_t n, const uint8_t* pubkeys, const uint8_t* pubkey_len, const uint8_t* sigs,
                     const uint32_t* sig_off, const uint8_t* msg, uint8_t* status) {
  if (!g_comb) {
    uint32_t* t = (uint32_t*)malloc(sizeof(uint32_t) * ZG_EC_COMB_WORDS * ZG_EC_COMB_POINTS);
    if (!t) return -1;
    for (int i = 0; i < ZG_EC_COMB_POINTS; i++) ec_comb_entry(i, t + (size_t)i * ZG_EC_COMB_WORDS);
    g_comb = t;
  }
  for (size_t i = 0; i < n; i++) {
    const uint32_t len = sig_off[i + 1] - sig_off[i];
    uint8_t* s = (uint8_t*)malloc(len ? len : 1);
    if (!s) return -1;
    for (uint32_t k = 0; k < len; k++) s[k] = sigs[sig_off[i] + k];
    status[i] = ecdsa_verify_one(pubkeys + 65 * i, pubkey_len[i], s, len, msg + 32 * i, g_comb);
    free(s);
  }
  return 0;
}

// field 7 / 8 of zg_debug_field_mul: a b mod p / mod n, 32-byte LE operands of any value
void zgt_ecdsa_field_mul(int field, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  for (size_t i = 0; i < n; i++) {
    if (field == 7)
      ec_debug_sf_mul(out + 8 * i, a + 8 * i, b + 8 * i);
    else
      ec_debug_sc_mul(out + 8 * i, a + 8 * i, b + 8 * i);
  }
}

}
