// zg_inputs.h -- the per-input routine of zg_inputs_verify, as host/device code: the
// kernel of zg_script.hip and a host-only build run the same routine. For one input that zg_script.h
// classified as a template it does what the interpreter does before the signature check:
//   OP_DUP OP_HASH160 <20> OP_EQUALVERIFY           script/src/interpreter.rs:756-758 (dhash160:
//                                                   crypto/src/lib.rs:158-166, 202-206), P2PKH only
//   check_signature_encoding under DERSIG           script/src/interpreter.rs:159-180
// and lays the key and the DER signature (the push without its hashtype byte) out as k_ecdsa takes them.
// The pushes are read in place: the signature and a P2PKH key from the transaction arena, a P2PK key from
// the previous scripts. Every offset in a record was validated by the matcher (zg_script.h) on the host.
#pragma once
#include "zg_script.h"
#include "zg_sighash.h"  // ShSha256, sh_absorb: SHA-256 over bytes at any alignment, the block in registers

namespace zg {

constexpr uint32_t SC_F_EQUALVERIFY = 1, SC_F_SIGNATURE_DER = 2;  // what a lane reports; the host folds
constexpr uint32_t SC_PUBKEY_STRIDE = 65;                         // include/zg.h ZG_ECDSA_PUBKEY_STRIDE

// One launched item, in the order of the signature-hash items (item k here signs hash k there)
struct ScDevItem {
  uint32_t cls;               // SCRIPT_P2PKH or SCRIPT_P2PK
  uint32_t sig_off, sig_len;  // the signature push in the arena (hashtype byte included; may be empty)
  uint32_t key_off, key_len;  // the key push: in the arena (P2PKH) or in the previous scripts (P2PK)
  uint32_t h160_off;          // P2PKH: the 20 bytes of the previous script, in the previous scripts
  uint32_t der_off;           // where this item's DER signature starts in the buffer k_ecdsa reads
  uint32_t pad;
};

struct ScBytesGen {  // one range, then the end
  const uint8_t* p;
  uint32_t len, done;
  ZG_SH_HD bool next(ShSeg& s) {
    if (done++) return false;
    seg_range(s, p, len);
    return true;
  }
};

// dhash160: RIPEMD-160 of SHA-256 of p[0..len) -> h[5], the digest's 20 bytes as little-endian words
ZG_SH_HD void sc_hash160(const uint8_t* p, uint32_t len, uint32_t h[5]) {
  ShSha256 sha;
  sha.init();
  ScBytesGen g{p, len, 0};
  sh_absorb(sha, g);
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 8; i++) x[i] = __builtin_bswap32(sha.st[i]), x[8 + i] = 0;
  x[8] = 0x80;
  x[14] = 256;  // the bit length, little-endian
  ripemd160_iv(h);
  ripemd160_compress(h, x);
}

// -> SC_F_* of item d; pubkey (65 bytes), *pubkey_len and der (d.sig_len - 1 bytes, none for an empty push):
// the item's row of k_ecdsa's buffers. A key of a length other than 33 or 65 is handed on as length 0
// (ZG_ECDSA_PUBLIC, its bytes are not read).
ZG_SH_HD uint32_t script_item(const uint8_t* arena, const uint8_t* prev, const ScDevItem& d, uint32_t flags,
                              uint8_t* pubkey, uint8_t* pubkey_len, uint8_t* der) {
  const uint8_t* key = (d.cls == SCRIPT_P2PKH ? arena : prev) + d.key_off;
  const uint8_t* sig = arena + d.sig_off;
  uint32_t out = 0;
  if (d.cls == SCRIPT_P2PKH) {
    uint32_t h[5];
    sc_hash160(key, d.key_len, h);
    const uint8_t* want = prev + d.h160_off;
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      const uint32_t w = (uint32_t)want[4 * i] | ((uint32_t)want[4 * i + 1] << 8) | ((uint32_t)want[4 * i + 2] << 16) |
                         ((uint32_t)want[4 * i + 3] << 24);
      diff |= w ^ h[i];
    }
    if (diff) out |= SC_F_EQUALVERIFY;
  }
  if ((flags & 1u) && d.sig_len && !is_valid_signature_encoding(sig, d.sig_len)) out |= SC_F_SIGNATURE_DER;
  const bool takes = d.key_len == 33 || d.key_len == 65;
  *pubkey_len = (uint8_t)(takes ? d.key_len : 0);
  for (uint32_t i = 0; i < SC_PUBKEY_STRIDE; i++) pubkey[i] = takes && i < d.key_len ? key[i] : (uint8_t)0;
  for (uint32_t i = 0; i + 1 < d.sig_len; i++) der[i] = sig[i];
  return out;
}

}  // namespace zg
