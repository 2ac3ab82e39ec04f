// zg_multisig.h -- the per-item, per-signature and fold routines of zg_inputs_verify's multisig classes (SURVEY.md
// 8(f) row f16), as host/device code: the kernels of zg_multisig.hip and a host-only build run the same routines.
// For an input that zg_script.h matched as m-of-n OP_CHECKMULTISIG, bare or behind pay-to-script-hash, they do
//   OP_HASH160 <20> OP_EQUAL over the redeem script     script/src/interpreter.rs:228-286 (P2SH), 756-758
//   check_signature_encoding under DERSIG               script/src/interpreter.rs:159-180, once per signature push
//   OP_CHECKMULTISIG's walk over signatures and keys    script/src/interpreter.rs:786-840
// The walk's signature checks are evaluated ahead of it, one k_ecdsa row per candidate pair: signature s (pop
// order, the last pushed first) can only ever meet keys s .. s + (n - m), so an item has m (n - m + 1) rows, row
// s (n - m + 1) + (k - s) for the pair (s, k). The fold then replays the walk over the rows' statuses. Every offset
// in a record was validated by the matcher on the host; nothing here follows one it did not.
#pragma once
#include "zg_inputs.h"

namespace zg {

constexpr uint32_t MS_NO_PAIR = 0xffffffffu;
constexpr uint32_t MS_INPUT_OK = 0, MS_INPUT_SIGNATURE_DER = 2, MS_INPUT_EVAL_FALSE = 3;  // include/zg.h ZG_INPUT_*

// One multisig item
struct MsDevItem {
  uint32_t p2sh;              // 1: the script is the redeem script, in the arena; 0: the previous script
  uint32_t m, n;
  uint32_t keys_off;          // the first key push instruction: in the arena (P2SH) or the previous scripts (bare)
  uint32_t red_off, red_len;  // P2SH: the redeem script in the arena
  uint32_t h160_off;          // P2SH: the 20 bytes of the previous script, in the previous scripts
  uint32_t sig0;              // signature s (pop order) is record sig_at[sig0 + s]
};

// One signature push, in the order of the signature-hash items planned for them (record g signs hash g of those)
struct MsDevSig {
  uint32_t item;              // its MsDevItem
  uint32_t s;                 // its place in pop order
  uint32_t sig_off, sig_len;  // the push in the arena (hashtype byte included; may be empty)
  uint32_t row0;              // its first pair row, counted from the first pair row of the call
  uint32_t der0;              // where its first row's DER bytes start in the buffer k_ecdsa reads
};

// -> 1 where the redeem script's HASH160 is not the script's 20 bytes (the script then leaves a false top:
// EvalFalse before the redeem script runs); 0 for a bare item
ZG_SH_HD uint32_t ms_item_hash(const uint8_t* arena, const uint8_t* prev, const MsDevItem& d) {
  if (!d.p2sh) return 0;
  uint32_t h[5];
  sc_hash160(arena + d.red_off, d.red_len, h);
  const uint8_t* want = prev + d.h160_off;
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint32_t w = (uint32_t)want[4 * i] | ((uint32_t)want[4 * i + 1] << 8) | ((uint32_t)want[4 * i + 2] << 16) |
                       ((uint32_t)want[4 * i + 3] << 24);
    diff |= w ^ h[i];
  }
  return diff ? 1 : 0;
}

// The rows of signature g: for each key it can meet, the key, its length, the DER bytes (the push without its
// hashtype byte), the row's end in sig_off and the 32-byte message, copied from the signature's hash, where
// k_ecdsa reads them. pubkeys, pubkey_len, sig_off and msg point at the call's first pair row; sigs is the whole
// buffer. -> 1 where the push is not empty and fails is_valid_signature_encoding.
ZG_SH_HD uint32_t ms_sig_rows(const uint8_t* arena, const uint8_t* prev, const MsDevItem& d, const MsDevSig& g,
                              const uint8_t* hash, uint8_t* pubkeys, uint8_t* pubkey_len, uint8_t* sigs,
                              uint32_t* sig_off, uint8_t* msg) {
  const uint8_t* sig = arena + g.sig_off;
  const uint32_t der_len = g.sig_len ? g.sig_len - 1 : 0;
  const uint8_t* p = (d.p2sh ? arena : prev) + d.keys_off;
  // key pushes in push order: push i is key n - 1 - i in pop order, and signature s meets keys s .. s + (n - m)
  for (uint32_t i = 0; i + g.s < d.n; i++) {
    const uint32_t key_len = p[0];  // 0x21 or 0x41: the matcher saw to it
    if (i + g.s + 1 >= d.m) {
      const uint32_t j = d.n - 1 - i - g.s, row = g.row0 + j;
      uint8_t* pk = pubkeys + (size_t)SC_PUBKEY_STRIDE * row;
      for (uint32_t b = 0; b < SC_PUBKEY_STRIDE; b++) pk[b] = b < key_len ? p[1 + b] : (uint8_t)0;
      pubkey_len[row] = (uint8_t)key_len;
      uint8_t* der = sigs + g.der0 + der_len * j;
      for (uint32_t b = 0; b < der_len; b++) der[b] = sig[b];
      sig_off[row + 1] = g.der0 + der_len * (j + 1);
      for (uint32_t b = 0; b < 32; b++) msg[(size_t)32 * row + b] = hash[b];
    }
    p += 1 + key_len;
  }
  return g.sig_len && !is_valid_signature_encoding(sig, g.sig_len) ? 1 : 0;
}

// OP_CHECKMULTISIG's walk (interpreter.rs:803-821) over what was computed ahead of it: hash_bad of ms_item_hash,
// enc_bad[g] of ms_sig_rows and ec[row], the ZG_ECDSA_* byte of each pair row (ec points at the call's first pair
// row). -> the item's ZG_INPUT_* status; *detail, the ZG_ECDSA_* status of the last pair checked where the walk
// failed; *last, the row of the last pair the walk checked, MS_NO_PAIR where it checked none.
ZG_SH_HD uint32_t ms_fold(const MsDevItem& d, const MsDevSig* sigs, const uint32_t* sig_at, uint32_t hash_bad,
                          const uint8_t* enc_bad, const uint8_t* ec, uint32_t dersig, uint32_t* detail, uint32_t* last) {
  *detail = 0, *last = MS_NO_PAIR;
  if (hash_bad) return MS_INPUT_EVAL_FALSE;
  uint32_t s = 0, k = 0, e = 0;
  bool success = true;
  while (s < d.m && success && k < d.n) {  // (k < n holds whenever the other two do: the bound is for the reader)
    const uint32_t g = sig_at[d.sig0 + s];
    if (dersig && enc_bad[g]) {
      *last = MS_NO_PAIR;
      return MS_INPUT_SIGNATURE_DER;
    }
    *last = sigs[g].row0 + (k - s);  // k - s <= n - m: success held
    e = ec[*last];
    if (e == 0) s++;
    k++;
    success = d.m - s <= d.n - k;
  }
  if (success) return MS_INPUT_OK;
  *detail = e;
  return MS_INPUT_EVAL_FALSE;
}

}  // namespace zg
