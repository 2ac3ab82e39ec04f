// zg_script.h -- the script templates zg_inputs_verify evaluates, host side
// (no HIP runtime: a stand-alone program includes it, like zg_txparse.h). Restates, for a pay-to-pubkey-hash
// or pay-to-pubkey output spent by a script_sig of pushes only,
//   verify_script / eval_script                     script/src/interpreter.rs:288-360, 361-1120
//   is_valid_signature_encoding                     script/src/interpreter.rs:49-136
//   check_signature_encoding (DERSIG alone)         script/src/interpreter.rs:159-180
// under the flags the acceptor passes (verification/src/accept_transaction.rs:334-358: strictenc, nulldummy,
// sigpushonly, cleanstack off; low_s and minimaldata at their default, off). Every other script is
// ZG_SCRIPT_HOST: the interpreter runs it on the host. Every offset the matcher hands out is inside the
// script it refers to; nothing downstream checks again.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZG_SCRIPT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ZG_SCRIPT_HD inline
#endif

namespace zg {

constexpr uint32_t SCRIPT_HOST = 0, SCRIPT_P2PKH = 1, SCRIPT_P2PK = 2;  // include/zg.h ZG_SCRIPT_*
constexpr uint32_t SCRIPT_MAX_PUSH = 520;                               // script/src/script.rs MAX_SCRIPT_ELEMENT_SIZE

struct ScriptClass {
  uint32_t cls;
  uint32_t sig_off, sig_len;  // the signature push (with its hashtype byte) in script_sig
  uint32_t key_off, key_len;  // the key push: in script_sig (P2PKH) or in script_pubkey (P2PK)
};

// One push instruction at s[*o .. n): opcode 0x00, 0x01..0x4b or OP_PUSHDATA1/2/4, its data wholly inside
// the script and at most 520 bytes. -> where the data lies, *o after it. Anything else is false.
inline bool script_push(const uint8_t* s, size_t n, size_t* o, uint32_t* off, uint32_t* len) {
  size_t p = *o;
  if (p >= n) return false;
  const uint32_t op = s[p++];
  uint64_t l;
  if (op <= 0x4b) {
    l = op;
  } else if (op <= 0x4e) {
    const size_t w = op == 0x4c ? 1 : op == 0x4d ? 2 : 4;
    if (n - p < w) return false;
    l = 0;
    for (size_t i = w; i-- > 0;) l = (l << 8) | s[p + i];
    p += w;
  } else {
    return false;
  }
  if (l > SCRIPT_MAX_PUSH || l > n - p) return false;
  *off = (uint32_t)p, *len = (uint32_t)l;
  *o = p + (size_t)l;
  return true;
}

// The template matcher over one (script_sig, script_pubkey) pair.
//   P2PKH: script_pubkey = 76 a9 14 <20> 88 ac; script_sig = <sig> <key>, nothing else
//   P2PK:  script_pubkey = 21 <33> ac or 41 <65> ac; script_sig = <sig>, nothing else
inline ScriptClass script_class(const uint8_t* sig, size_t sig_len, const uint8_t* pk, size_t pk_len) {
  ScriptClass c{SCRIPT_HOST, 0, 0, 0, 0}, none = c;
  size_t o = 0;
  if (pk_len == 25 && pk[0] == 0x76 && pk[1] == 0xa9 && pk[2] == 0x14 && pk[23] == 0x88 && pk[24] == 0xac) {
    if (!script_push(sig, sig_len, &o, &c.sig_off, &c.sig_len)) return none;
    if (!script_push(sig, sig_len, &o, &c.key_off, &c.key_len)) return none;
    c.cls = SCRIPT_P2PKH;
  } else if ((pk_len == 35 && pk[0] == 0x21 && pk[34] == 0xac) || (pk_len == 67 && pk[0] == 0x41 && pk[66] == 0xac)) {
    if (!script_push(sig, sig_len, &o, &c.sig_off, &c.sig_len)) return none;
    c.key_off = 1, c.key_len = (uint32_t)pk_len - 2;
    c.cls = SCRIPT_P2PK;
  } else {
    return none;
  }
  return o == sig_len ? c : none;
}

// ---- m-of-n OP_CHECKMULTISIG, bare or behind pay-to-script-hash (the rules: include/zg.h)
constexpr uint32_t SCRIPT_MULTISIG = 3, SCRIPT_P2SH_MULTISIG = 4;  // include/zg.h ZG_SCRIPT_*
constexpr uint32_t SCRIPT_TEMPLATE_MULTISIG = 0x100;               // ZG_SCRIPT_TEMPLATE_MULTISIG
constexpr uint32_t SCRIPT_MAX_KEYS = 16;                           // the counts are the opcodes OP_1..OP_16

struct ScriptMatch {
  uint32_t cls;
  ScriptClass one;                 // P2PKH, P2PK: the record script_class gives
  uint32_t m, n;                   // multisig: signatures and keys
  uint32_t red_off, red_len;       // P2SH: the redeem script (the last push's data) in script_sig; bare: 0, 0
  uint32_t sigs_at;                // where the first signature push instruction starts in script_sig, after the dummy
  uint32_t sig_off[SCRIPT_MAX_KEYS], sig_len[SCRIPT_MAX_KEYS];  // the m signature pushes in script_sig, in push order
  uint32_t pairs() const { return cls >= SCRIPT_MULTISIG ? m * (n - m + 1) : cls ? 1 : 0; }
};

// s[0..len) = OP_m <key>...<key> OP_n ae: OP_m and OP_n the opcodes 51..60, 1 <= m <= n, exactly n key pushes, each
// the direct push 21 or 41 with its bytes inside the script, nothing after ae. The first key push is at s[1].
inline bool script_multisig_form(const uint8_t* s, size_t len, uint32_t* m, uint32_t* n) {
  if (len < 3 || s[0] < 0x51 || s[0] > 0x60) return false;
  size_t o = 1;
  uint32_t keys = 0;
  while (o < len && (s[o] == 0x21 || s[o] == 0x41)) {
    if (len - o < (size_t)s[o] + 1 || ++keys > SCRIPT_MAX_KEYS) return false;
    o += (size_t)s[o] + 1;
  }
  if (len - o != 2 || s[o] < 0x51 || s[o] > 0x60 || s[o + 1] != 0xae) return false;
  *m = s[0] - 0x50u, *n = s[o] - 0x50u;
  return *n == keys && *m <= *n;
}

// script_class, and with SCRIPT_TEMPLATE_MULTISIG in flags the two multisig classes:
//   MULTISIG:      script_pubkey of the form above; script_sig = <dummy> <sig> x m, push instructions, nothing else
//   P2SH_MULTISIG: script_pubkey = a9 14 <20> 87; script_sig = <dummy> <sig> x m <redeem script of the form above>
inline ScriptMatch script_match(const uint8_t* sig, size_t sig_len, const uint8_t* pk, size_t pk_len, uint32_t flags) {
  ScriptMatch r{};
  r.one = script_class(sig, sig_len, pk, pk_len);
  r.cls = r.one.cls;
  if (r.cls != SCRIPT_HOST) {
    r.m = r.n = 1;
    return r;
  }
  const ScriptMatch none = r;
  if (!(flags & SCRIPT_TEMPLATE_MULTISIG)) return none;
  const bool p2sh = pk_len == 23 && pk[0] == 0xa9 && pk[1] == 0x14 && pk[22] == 0x87;
  if (!p2sh && !script_multisig_form(pk, pk_len, &r.m, &r.n)) return none;
  // the pushes of script_sig: the dummy, at most 16 signatures, the redeem script
  uint32_t off[SCRIPT_MAX_KEYS + 2], len[SCRIPT_MAX_KEYS + 2], np = 0;
  size_t o = 0, second = 0;
  while (o < sig_len) {
    if (np == SCRIPT_MAX_KEYS + 2 || !script_push(sig, sig_len, &o, &off[np], &len[np])) return none;
    if (!np++) second = o;
  }
  if (p2sh) {
    if (np < 3 || !script_multisig_form(sig + off[np - 1], len[np - 1], &r.m, &r.n)) return none;
    r.red_off = off[--np], r.red_len = len[np];
  }
  if (np != r.m + 1) return none;
  for (uint32_t s = 0; s < r.m; s++) r.sig_off[s] = off[s + 1], r.sig_len[s] = len[s + 1];
  r.sigs_at = (uint32_t)second;
  r.cls = p2sh ? SCRIPT_P2SH_MULTISIG : SCRIPT_MULTISIG;
  return r;
}

// is_valid_signature_encoding (interpreter.rs:49-136) over the n bytes of a signature push, hashtype byte
// included; the checks in the reference's order. No byte at or past n is read.
ZG_SCRIPT_HD bool is_valid_signature_encoding(const uint8_t* sig, uint32_t n) {
  if (n < 9 || n > 73) return false;
  if (sig[0] != 0x30) return false;
  if (sig[1] != n - 3) return false;
  const uint32_t len_r = sig[3];
  if (len_r + 5 >= n) return false;
  const uint32_t len_s = sig[len_r + 5];
  if (len_r + len_s + 7 != n) return false;
  if (sig[2] != 2) return false;
  if (len_r == 0) return false;
  if (sig[4] & 0x80) return false;
  if (len_r > 1 && sig[4] == 0 && !(sig[5] & 0x80)) return false;
  if (sig[len_r + 4] != 2) return false;
  if (len_s == 0) return false;
  if (sig[len_r + 6] & 0x80) return false;
  if (len_s > 1 && sig[len_r + 6] == 0 && !(sig[len_r + 7] & 0x80)) return false;
  return true;
}

}  // namespace zg
