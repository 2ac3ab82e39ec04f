// zg_sighash.h -- the transaction signature hash, as host/device code: the kernels
// of zg_sighash.hip and a host-only build run the same routines.
//   TransactionInputSigner::signature_hash           script/src/sign.rs:152-176
//   signature_hash_sprout (double SHA-256)           script/src/sign.rs:179-246
//   signature_hash_post_overwinter (BLAKE2b-256)     script/src/sign.rs:249-329, compute_hash_* :344-474
// over the layout record of zg_txparse.h: the transaction is never re-serialized, the stream the
// reference hashes is generated as a sequence of segments -- a byte range of the transaction arena, up
// to eight literal bytes, or a run of one byte -- and absorbed by one loop per hash.
//
// The 16-word message block stays in registers: words enter at the top of a shift register (w[15], the
// others moving down one), so no array is indexed by a run-time value; each absorb loop holds the one
// call of its compression function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zg_hash.h"
#include "zg_txparse.h"

#define ZG_SH_HD __host__ __device__ __forceinline__

namespace zg {

constexpr uint32_t SIGHASH_NO_INPUT = 0xFFFFFFFFu;  // include/zg.h ZG_SIGHASH_NO_INPUT
constexpr int SH_PREVOUTS = 0, SH_SEQUENCES = 1, SH_OUTPUTS = 2, SH_JOINSPLITS = 3, SH_SPENDS = 4, SH_SOUTPUTS = 5;
constexpr int SH_DIGESTS = 6;

// ---- a piece of the hashed stream
struct ShSeg {
  const uint8_t* p;  // RANGE: the bytes
  uint64_t imm;      // IMM: up to 8 bytes, the first in the low byte; FILL: the byte
  uint32_t len;
  uint32_t kind;
};
constexpr uint32_t SEG_RANGE = 0, SEG_IMM = 1, SEG_FILL = 2;

ZG_SH_HD void seg_range(ShSeg& s, const uint8_t* p, uint32_t len) { s.p = p, s.imm = 0, s.len = len, s.kind = SEG_RANGE; }
ZG_SH_HD void seg_imm(ShSeg& s, uint64_t v, uint32_t len) { s.p = nullptr, s.imm = v, s.len = len, s.kind = SEG_IMM; }
ZG_SH_HD void seg_fill(ShSeg& s, uint32_t byte, uint32_t len) { s.p = nullptr, s.imm = byte, s.len = len, s.kind = SEG_FILL; }
// CompactInteger::serialize of a value < 2^32 (compact_integer.rs:61-83)
ZG_SH_HD void seg_compact(ShSeg& s, uint32_t v) {
  if (v < 0xfd)
    seg_imm(s, v, 1);
  else if (v <= 0xffff)
    seg_imm(s, 0xfdull | ((uint64_t)v << 8), 3);
  else
    seg_imm(s, 0xfeull | ((uint64_t)v << 8), 5);
}

// ---- SHA-256 (FIPS 180-4), the block as big-endian words in a shift register
struct ShSha256 {
  typedef uint32_t word;
  static constexpr uint32_t WB = 4;
  uint32_t st[8], w[16], cnt;

  ZG_SH_HD void init() {
    sha256_iv(st);
    cnt = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0;
  }
  // byte k of a word under construction: big-endian
  static ZG_SH_HD uint32_t put(uint32_t acc, uint32_t b, uint32_t) { return (acc << 8) | b; }
  static ZG_SH_HD uint32_t load(const uint8_t* p) {
    uint32_t x;
    __builtin_memcpy(&x, p, 4);
    return __builtin_bswap32(x);
  }
  // the next whole word of a stream that stands nb bytes into one: acc's bytes, then the first 4 - nb of x;
  // the rest of x stays in acc
  static ZG_SH_HD uint32_t merge(uint32_t& acc, uint32_t nb, uint32_t x) {
    const uint64_t t = ((uint64_t)acc << 32) | x;
    acc = x & ((1u << (8 * nb)) - 1u);
    return (uint32_t)(t >> (8 * nb));
  }
  // `last` is unused: the padding makes the stream a whole number of blocks, each compressed as it fills
  ZG_SH_HD void push(uint32_t x, bool) {
#pragma unroll
    for (int i = 0; i < 15; i++) w[i] = w[i + 1];
    w[15] = x;
    if (++cnt == 16) {
      sha256_compress(st, w);
      cnt = 0;
    }
  }
  // the padding after `total` message bytes, as segments: 0x80, zeros to 56 mod 64, the bit length big-endian
  ZG_SH_HD bool pad(uint32_t step, uint32_t total, ShSeg& s) const {
    if (step == 0) {
      seg_imm(s, 0x80, 1);
    } else if (step == 1) {
      seg_fill(s, 0, (55u - total) & 63u);
    } else if (step == 2) {
      seg_imm(s, __builtin_bswap64((uint64_t)total << 3), 8);
    } else {
      return false;
    }
    return true;
  }
  ZG_SH_HD void finish(uint32_t) {}
  // SHA-256 of the 32 digest bytes, then the bytes of that digest
  ZG_SH_HD void second_and_store(uint8_t* out) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = st[i], w[8 + i] = 0;
    w[8] = 0x80000000u;
    w[15] = 256;
    sha256_iv(st);
    sha256_compress(st, w);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      out[4 * i] = (uint8_t)(st[i] >> 24), out[4 * i + 1] = (uint8_t)(st[i] >> 16);
      out[4 * i + 2] = (uint8_t)(st[i] >> 8), out[4 * i + 3] = (uint8_t)st[i];
    }
  }
};

// ---- BLAKE2b-256 (RFC 7693), unkeyed, personalized; the block as little-endian words in a shift register.
// The last block carries the final flag even when it is full, so a full block waits for the next word
// (or the end) before it is compressed: the one call site takes the flag as a value.
struct ShBlake2b {
  typedef uint64_t word;
  static constexpr uint32_t WB = 8;
  uint64_t h[8], m[16];
  uint32_t cnt, blocks;

  ZG_SH_HD void init(uint64_t p0, uint64_t p1) {
    blake2b_init(h, 32, p0, p1);
    cnt = 0, blocks = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = 0;
  }
  static ZG_SH_HD uint64_t put(uint64_t acc, uint32_t b, uint32_t k) { return acc | ((uint64_t)b << (8 * k)); }
  static ZG_SH_HD uint64_t load(const uint8_t* p) {
    uint64_t x;
    __builtin_memcpy(&x, p, 8);
    return x;
  }
  static ZG_SH_HD uint64_t merge(uint64_t& acc, uint32_t nb, uint64_t x) {
    const uint64_t w = nb ? acc | (x << (8 * nb)) : x;
    acc = nb ? x >> (64 - 8 * nb) : 0;
    return w;
  }
  // `last`: x is no word of the stream but the end of it; total: the message length
  ZG_SH_HD void push(uint64_t x, bool last, uint32_t total = 0) {
    if (cnt == 16 || last) {
      if (!last) blocks++;
      blake2b_compress(h, m, last ? (uint64_t)total : (uint64_t)blocks * 128u, last);
      cnt = 0;
    }
    if (!last) {
#pragma unroll
      for (int i = 0; i < 15; i++) m[i] = m[i + 1];
      m[15] = x;
      cnt++;
    }
  }
  // zeros up to a whole block (a whole block of them for the empty message)
  ZG_SH_HD bool pad(uint32_t step, uint32_t total, ShSeg& s) const {
    if (step) return false;
    seg_fill(s, 0, total == 0 ? 128u : (128u - (total & 127u)) & 127u);
    return true;
  }
  ZG_SH_HD void store(uint8_t* out) const {
#pragma unroll
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(h[i / 8] >> (8 * (i % 8)));
  }
};

// ---- the one loop: the generator's segments, then the sink's padding, a word at a time into the sink.
// A range is read a whole word at a time wherever the stream stands within a word (the arena is read at any
// alignment; a literal before it usually leaves the stream off a word boundary), its last bytes one by one.
// Returns the message length.
template <class Sink, class Gen>
ZG_SH_HD uint32_t sh_absorb(Sink& sink, Gen& gen) {
  typename Sink::word acc = 0;
  uint32_t nb = 0, total = 0, padstep = 0;
  bool padding = false;
  ShSeg s;
  for (;;) {
    if (!padding) {
      if (!gen.next(s)) {
        padding = true;
        continue;
      }
      total += s.len;
    } else if (!sink.pad(padstep++, total, s)) {
      break;
    }
    while (s.len) {
      typename Sink::word x;
      if (s.kind == SEG_RANGE && s.len >= Sink::WB) {
        x = Sink::merge(acc, nb, Sink::load(s.p));
        s.p += Sink::WB;
        s.len -= Sink::WB;
      } else {
        uint32_t b;
        if (s.kind == SEG_RANGE) {
          b = *s.p++;
        } else {
          b = (uint32_t)(s.imm & 0xff);
          if (s.kind == SEG_IMM) s.imm >>= 8;
        }
        s.len--;
        acc = Sink::put(acc, b, nb);
        if (++nb < Sink::WB) continue;
        x = acc;
        acc = 0;
        nb = 0;
      }
      sink.push(x, false);
    }
  }
  return total;
}

// ---- generators
// one of the six per-transaction digests of an overwintered transaction (sign.rs:344-474)
struct ShDigestGen {
  const uint8_t* tx;
  const TxLayout* L;
  const uint32_t* in_off;  // this transaction's n_in + 1
  const uint32_t* out_off;
  int which;
  uint32_t i;

  ZG_SH_HD bool next(ShSeg& s) {
    const uint32_t k = i++;
    switch (which) {
      case SH_PREVOUTS:
        if (k >= L->n_in) return false;
        seg_range(s, tx + in_off[k], 36);
        return true;
      case SH_SEQUENCES:
        if (k >= L->n_in) return false;
        seg_range(s, tx + in_off[k + 1] - 4, 4);
        return true;
      case SH_OUTPUTS:
        if (k) return false;
        seg_range(s, tx + out_off[0], out_off[L->n_out] - out_off[0]);
        return true;
      case SH_JOINSPLITS:  // the descriptions, then the pubkey that follows them
        if (k) return false;
        seg_range(s, tx + L->js_off, L->n_js * L->js_size + 32);
        return true;
      case SH_SPENDS:  // cv, anchor, nullifier, rk, proof: the first 320 of the 384 bytes
        if (k >= L->n_spend) return false;
        seg_range(s, tx + L->spend_off + 384u * k, 320);
        return true;
      default:
        if (k) return false;
        seg_range(s, tx + L->sout_off, 948u * L->n_sout);
        return true;
    }
  }
};

ZG_SH_HD uint64_t sh_le64(const char* c) {
  uint64_t v = 0;
  for (int b = 7; b >= 0; b--) v = (v << 8) | (uint8_t)c[b];
  return v;
}

// digest `which` of an overwintered transaction whose list is not empty where the reference tests that
// (JoinSplits, spends, Sapling outputs); the prevouts, sequences and outputs digests of empty lists are
// BLAKE2b of the empty message, as there
ZG_SH_HD void sighash_digest(const uint8_t* tx, const TxLayout& L, const uint32_t* in_off, const uint32_t* out_off,
                             int which, uint8_t* out) {
  const char* person = which == SH_PREVOUTS ? "ZcashPrevoutHash" : which == SH_SEQUENCES ? "ZcashSequencHash"
                     : which == SH_OUTPUTS  ? "ZcashOutputsHash" : which == SH_JOINSPLITS ? "ZcashJSplitsHash"
                     : which == SH_SPENDS   ? "ZcashSSpendsHash" : "ZcashSOutputHash";
  ShBlake2b b;
  b.init(sh_le64(person), sh_le64(person + 8));
  ShDigestGen g{tx, &L, in_off, out_off, which, 0};
  const uint32_t total = sh_absorb(b, g);
  b.push(0, true, total);
  b.store(out);
}

// what of the hashtype the branches look at (Sighash::from_u32, script/src/sign.rs)
constexpr uint32_t SH_ALL = 1, SH_NONE = 2, SH_SINGLE = 3;
ZG_SH_HD uint32_t sh_base(uint32_t hashtype) {
  const uint32_t b = hashtype & 0x1f;
  return b == 2 ? SH_NONE : b == 3 ? SH_SINGLE : SH_ALL;
}

struct ShItem {
  const uint8_t* tx;
  const TxLayout* L;
  const uint32_t* in_off;
  const uint32_t* out_off;
  const uint8_t* digests;  // overwintered: SH_DIGESTS x 32, those this item reads
  const uint8_t* script;
  uint32_t script_len, index, hashtype, branch_id;
  uint64_t amount;
};

// the serialization signature_hash_sprout hashes (sign.rs:184-244 over Transaction::serialize)
struct ShSproutGen {
  const ShItem* it;
  uint32_t base, acp, phase, i, n_emit;

  ZG_SH_HD void init(const ShItem* item) {
    it = item;
    base = sh_base(it->hashtype);
    acp = it->hashtype & 0x80;
    phase = 0;
    i = 0;
    n_emit = 0;
  }
  ZG_SH_HD bool next(ShSeg& s) {
    const TxLayout& L = *it->L;
    const uint8_t* tx = it->tx;
    switch (phase) {
      case 0:  // the header word, the input count
        seg_imm(s, L.header, 4);
        phase = 1;
        return true;
      case 1:
        seg_compact(s, acp ? 1 : L.n_in);
        i = acp ? it->index : 0;
        n_emit = acp ? it->index + 1 : L.n_in;
        phase = i < n_emit ? 2 : 6;
        return true;
      case 2:
        seg_range(s, tx + it->in_off[i], 36);
        phase = 3;
        return true;
      case 3:
        seg_compact(s, i == it->index ? it->script_len : 0);
        phase = 4;
        return true;
      case 4:
        seg_range(s, it->script, i == it->index ? it->script_len : 0);
        phase = 5;
        return true;
      case 5:
        if (!acp && i != it->index && base != SH_ALL)
          seg_imm(s, 0, 4);
        else
          seg_range(s, tx + it->in_off[i + 1] - 4, 4);
        phase = ++i < n_emit ? 2 : 6;
        return true;
      case 6:  // the output count
        n_emit = base == SH_ALL ? L.n_out : base == SH_NONE ? 0 : (it->index + 1 < L.n_out ? it->index + 1 : L.n_out);
        seg_compact(s, n_emit);
        i = 0;
        phase = base == SH_ALL ? 7 : n_emit ? 8 : 10;
        return true;
      case 7:
        seg_range(s, tx + it->out_off[0], it->out_off[L.n_out] - it->out_off[0]);
        phase = 10;
        return true;
      case 8:  // Single: the output at the index, TransactionOutput::default() (value 2^64 - 1, no script) before
        if (i == it->index)
          seg_range(s, tx + it->out_off[i], it->out_off[i + 1] - it->out_off[i]);
        else
          seg_fill(s, 0xff, 8);
        phase = 9;
        return true;
      case 9:
        seg_imm(s, 0, i == it->index ? 0 : 1);
        phase = ++i < n_emit ? 8 : 10;
        return true;
      case 10:
        seg_range(s, tx + L.lock_off, 4);
        phase = L.header >= 2 ? 11 : 14;
        return true;
      case 11:
        seg_compact(s, L.n_js);
        phase = L.n_js ? 12 : 14;
        return true;
      case 12:
        seg_range(s, tx + L.js_off, L.n_js * L.js_size + 32);
        phase = 13;
        return true;
      case 13:  // the null signature
        seg_fill(s, 0, 64);
        phase = 14;
        return true;
      case 14:
        seg_imm(s, it->hashtype, 4);
        phase = 15;
        return true;
      default:
        return false;
    }
  }
};

// pass 0: the one output of hash_outputs for Single (sign.rs:398-402); pass 1: the final stream (:300-326)
struct ShOverwinterGen {
  const ShItem* it;
  uint32_t pass, phase, base, acp;
  const uint8_t* single_digest;  // pass 0's digest

  ZG_SH_HD void zero_or(ShSeg& s, bool take, int which) {
    if (take)
      seg_range(s, it->digests + 32 * which, 32);
    else
      seg_fill(s, 0, 32);
  }
  ZG_SH_HD bool next(ShSeg& s) {
    const TxLayout& L = *it->L;
    const uint8_t* tx = it->tx;
    const bool sapling = L.sigver == 2;
    const bool given = it->index != SIGHASH_NO_INPUT;
    if (pass == 0) {
      if (phase++) return false;
      seg_range(s, tx + it->out_off[it->index], it->out_off[it->index + 1] - it->out_off[it->index]);
      return true;
    }
    switch (phase++) {
      case 0:
        seg_imm(s, (uint64_t)L.header | ((uint64_t)L.vgid << 32), 8);
        return true;
      case 1:
        zero_or(s, !acp, SH_PREVOUTS);
        return true;
      case 2:
        zero_or(s, !acp && base == SH_ALL, SH_SEQUENCES);
        return true;
      case 3:  // Single: pass 0 left its digest in the output buffer
        if (base == SH_SINGLE && given && it->index < L.n_out)
          seg_range(s, single_digest, 32);
        else
          zero_or(s, base == SH_ALL, SH_OUTPUTS);
        return true;
      case 4:
      case 5:
      case 6:
        seg_imm(s, 0, 0);
        return true;
      case 7:
        zero_or(s, L.n_js != 0, SH_JOINSPLITS);
        return true;
      case 8:
        if (sapling)
          zero_or(s, L.n_spend != 0, SH_SPENDS);
        else
          seg_imm(s, 0, 0);
        return true;
      case 9:
        if (sapling)
          zero_or(s, L.n_sout != 0, SH_SOUTPUTS);
        else
          seg_imm(s, 0, 0);
        return true;
      case 10:  // lock_time, expiry_height and (v4) the balancing value lie next to each other
        seg_range(s, tx + L.lock_off, sapling ? 16 : 8);
        return true;
      case 11:
        seg_imm(s, it->hashtype, 4);
        return true;
      case 12:
        if (!given) return false;
        seg_range(s, tx + it->in_off[it->index], 36);
        return true;
      case 13:
        seg_compact(s, it->script_len);
        return true;
      case 14:
        seg_range(s, it->script, it->script_len);
        return true;
      case 15:
        seg_imm(s, it->amount, 8);
        return true;
      case 16:
        seg_range(s, tx + it->in_off[it->index + 1] - 4, 4);
        return true;
      default:
        return false;
    }
  }
};

// ---- what zg_sighash puts on the device next to the arena, the layouts and the offset tables
struct ShDevTx {
  TxLayout L;
  uint32_t base;       // the transaction's first byte in the arena
  uint32_t branch_id;
  uint32_t dig;        // its row of SH_DIGESTS x 32 bytes in the digest buffer (overwintered with an item)
};
struct ShDevItem {
  uint32_t tx, index, script_off, script_len, hashtype, slot;  // slot: the caller's item number
  uint64_t amount;
};

ZG_SH_HD ShItem sh_item(const uint8_t* arena, const ShDevTx* txs, const uint32_t* in_off, const uint32_t* out_off,
                        const uint8_t* digests, const uint8_t* scripts, const ShDevItem& d) {
  const ShDevTx& t = txs[d.tx];
  ShItem it;
  it.tx = arena + t.base;
  it.L = &t.L;
  it.in_off = in_off + t.L.in_idx;
  it.out_off = out_off + t.L.out_idx;
  it.digests = digests + (size_t)32 * SH_DIGESTS * t.dig;
  it.script = scripts + d.script_off;
  it.script_len = d.script_len, it.index = d.index, it.hashtype = d.hashtype, it.branch_id = t.branch_id;
  it.amount = d.amount;
  return it;
}

// One item whose transaction parsed (ZG_TX_OK) and, if overwintered, whose index is NO_INPUT or < inputs.
// out: 32 bytes, H256 storage order.
ZG_SH_HD void sighash_item(const ShItem& it, uint8_t* out) {
  const TxLayout& L = *it.L;
  const uint32_t base = sh_base(it.hashtype), acp = it.hashtype & 0x80;
  if (L.sigver == 0) {
    if (it.index >= L.n_in && (acp || base == SH_SINGLE)) {  // None included: NO_INPUT >= any count
      for (int i = 0; i < 32; i++) out[i] = 0;
      return;
    }
    ShSha256 sha;
    sha.init();
    ShSproutGen g;
    g.init(&it);
    sh_absorb(sha, g);
    sha.second_and_store(out);
    return;
  }
  ShOverwinterGen g;
  g.it = &it, g.base = base, g.acp = acp;
  g.single_digest = out;
  const bool single = base == SH_SINGLE && it.index != SIGHASH_NO_INPUT && it.index < L.n_out;
  for (uint32_t pass = single ? 0 : 1; pass < 2; pass++) {
    ShBlake2b b;
    if (pass == 0)
      b.init(sh_le64("ZcashOutputsHash"), sh_le64(&"ZcashOutputsHash"[8]));
    else  // "ZcashSigHash" || LE32(branch id)
      b.init(sh_le64("ZcashSigHash"), 0x68736148ull | ((uint64_t)it.branch_id << 32));
    g.pass = pass, g.phase = 0;
    const uint32_t total = sh_absorb(b, g);
    b.push(0, true, total);
    b.store(out);  // pass 0: read back by pass 1, which then overwrites it
  }
}

}  // namespace zg
