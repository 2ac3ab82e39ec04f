// zg_blocks.h -- block bodies, as host/device code: the kernels of zg_blocks.hip
// and a host-only build run the same routines.
//   IndexedTransaction::hash (dhash256 of the serialized transaction)   chain/src/read_and_hash.rs:16-32
//   merkle_root, merkle_node_hash                                       chain/src/merkle_root.rs:14-38
//   Block::deserialize                                                  chain/src/block.rs:10-14
//   transaction_sigops (bip16_active = false)                           verification/src/sigops.rs:9-41
//   Script::sigops_count(false), Script::get_instruction                script/src/script.rs:289-317, :199-236
//   Opcode::from_u8                                                     script/src/opcode.rs:224-434
//   Transaction::is_coinbase, OutPoint::is_null                         chain/src/transaction.rs:153-155, :44-46
//
// A transaction id hashes one contiguous byte range, so its reader is not the word funnel of zg_sighash.h:
// a 64-byte message block is fetched as five 16-byte loads at 16-byte-aligned addresses (the slice's first
// byte lies anywhere in the first of them), brought to the slice's own alignment in registers -- a shift by
// whole words under two conditions, then one funnel shift per word -- and the loads of the next block are
// issued before this one is compressed. No array is indexed by a run-time value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "zg_hash.h"
#include "zg_txparse.h"

#define ZG_BLK_HD __host__ __device__ __forceinline__

namespace zg {

// ---- the arena rule. A routine below reads the arena in aligned 16-byte pieces, up to 80 bytes from the
// aligned address at or below a message block's first byte; the last block of a slice of `len` bytes starts
// less than len + 9 bytes into it. So it touches no byte outside an arena whose first byte is 16-byte aligned
// and whose allocation is txid_arena_bytes(bytes): every buffer the routines run on, device or host, is
// allocated by this one rule (the bytes past the data are read and masked away, whatever they hold).
constexpr size_t TXID_ARENA_PAD = 96;
constexpr size_t txid_arena_bytes(size_t bytes) { return bytes + TXID_ARENA_PAD; }

// one slice of the arena and the row of the output its hash goes to
struct TxidSlice {
  uint32_t off, len, slot, pad_;
};
// one block of zg_blocks_verify: where its header starts in the arena, its rows of the id buffer
struct MerkleBlk {
  uint32_t hdr_off, row0, n, pad_;
};

// the 80 bytes at the aligned offset a (five chunks, as 20 LE words)
ZG_BLK_HD void txid_load(const uint8_t* arena, size_t a, uint32_t q[20]) {
#pragma unroll
  for (int j = 0; j < 5; j++) {
    uint4 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(arena + a + 16 * j, 16), 16);
    q[4 * j] = v.x, q[4 * j + 1] = v.y, q[4 * j + 2] = v.z, q[4 * j + 3] = v.w;
  }
}

// the 16 message words (big-endian values) that start sh bytes (0..15) into q; q is clobbered
ZG_BLK_HD void txid_words(uint32_t q[20], uint32_t sh, uint32_t w[16]) {
  if (sh & 8) {
#pragma unroll
    for (int i = 0; i < 18; i++) q[i] = q[i + 2];
  }
  if (sh & 4) {
#pragma unroll
    for (int i = 0; i < 17; i++) q[i] = q[i + 1];
  }
  const uint32_t s = 8 * (sh & 3);
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = __builtin_bswap32((uint32_t)((((uint64_t)q[i + 1] << 32) | q[i]) >> s));
}

// message block k of a message of len bytes, when it is not all data: what lies past the data is replaced by
// the padding (0x80, zeros; in the last block the bit length)
ZG_BLK_HD void txid_pad(uint32_t w[16], uint32_t k, uint32_t len, bool last) {
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int64_t rem = (int64_t)len - ((int64_t)64 * k + 4 * i);  // data bytes from this word on
    if (rem <= 0)
      w[i] = rem == 0 ? 0x80000000u : 0u;
    else if (rem < 4)
      w[i] = (w[i] & ~(0xffffffffu >> (8 * rem))) | (0x80000000u >> (8 * rem));
  }
  if (last) {
    w[14] = len >> 29;
    w[15] = len << 3;
  }
}

// SHA-256 of the 32 digest bytes in st, from the IV; out: the 8 words of the result in H256 storage order
ZG_BLK_HD void sha256_second(const uint32_t st[8], uint32_t out[8]) {
  uint32_t w[16], s2[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = st[i], w[8 + i] = 0;
  w[8] = 0x80000000u;
  w[15] = 256;
  sha256_iv(s2);
  sha256_compress(s2, w);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = __builtin_bswap32(s2[i]);
}

// dhash256 of arena[off .. off + len), len <= 2^31, under the arena rule above
ZG_BLK_HD void txid_hash(const uint8_t* arena, size_t off, uint32_t len, uint32_t out[8]) {
  const size_t a = off & ~(size_t)15;
  const uint32_t sh = (uint32_t)(off & 15);
  const uint32_t nb = (uint32_t)(((uint64_t)len + 72) / 64);  // the data, 0x80 and the 8 length bytes
  uint32_t st[8], cur[20], nxt[20], w[16];
  sha256_iv(st);
  txid_load(arena, a, cur);
  for (uint32_t k = 0; k < nb; k++) {
    // the next block's loads go out first (after the last block: that block's again, never past it)
    txid_load(arena, a + (size_t)64 * (k + 1 < nb ? k + 1 : k), nxt);
    txid_words(cur, sh, w);
    if ((uint64_t)64 * k + 64 > len) txid_pad(w, k, len, k + 1 == nb);
    sha256_compress(st, w);
#pragma unroll
    for (int i = 0; i < 20; i++) cur[i] = nxt[i];
  }
  sha256_second(st, out);
}

// merkle_node_hash: dhash256 of left || right (8 + 8 words, H256 storage order), out likewise
ZG_BLK_HD void merkle_node(const uint32_t l[8], const uint32_t r[8], uint32_t out[8]) {
  uint32_t st[8], w[16];
  sha256_iv(st);
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = __builtin_bswap32(l[i]), w[8 + i] = __builtin_bswap32(r[i]);
  // the 64 bytes, their padding block, then the digest's own block from the IV: one call site
#pragma unroll 1
  for (int pass = 0; pass < 3; pass++) {
    if (pass) {
#pragma unroll
      for (int i = 0; i < 16; i++)
        w[i] = pass == 2 ? (i < 8 ? st[i] : i == 8 ? 0x80000000u : i == 15 ? 256u : 0u)
                         : (i == 0 ? 0x80000000u : i == 15 ? 512u : 0u);
      if (pass == 2) sha256_iv(st);
    }
    sha256_compress(st, w);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = __builtin_bswap32(st[i]);
}

// ---- host side: a host buffer under the arena rule, the block parser, the signature-operation count
struct alignas(16) TxidChunk {
  uint8_t b[16];
};
struct TxidArena {
  std::vector<TxidChunk> v;
  uint8_t* data() { return v.empty() ? nullptr : v[0].b; }
  void assign(const uint8_t* p, size_t bytes) {
    v.resize((txid_arena_bytes(bytes) + 15) / 16);
    if (bytes) memcpy(data(), p, bytes);
  }
};
// dhash256 of p[0..len) on the host, through the same reader: the bytes are copied under the arena rule
inline void txid_hash_bytes(const uint8_t* p, uint32_t len, TxidArena& tmp, uint8_t out[32]) {
  tmp.assign(p, len);
  uint32_t h[8];
  txid_hash(tmp.data(), 0, len, h);
  memcpy(out, h, 32);
}

// Script::sigops_count(false): the count so far at the first byte Opcode::from_u8 does not know (0xab and
// everything above 0xb9) or the first push that runs past the script
inline uint64_t script_sigops(const uint8_t* s, uint64_t n) {
  uint64_t pc = 0, total = 0;
  while (pc < n) {
    const uint32_t op = s[pc];
    if (op == 0xab || op > 0xb9) return total;
    if (op <= 0x4b) {
      if (pc + 1 + op > n) return total;
      pc += 1 + op;
    } else if (op <= 0x4e) {
      const uint32_t lb = op == 0x4c ? 1 : op == 0x4d ? 2 : 4;
      if (pc + 1 + lb > n) return total;
      uint64_t v = 0;
      for (uint32_t i = 0; i < lb; i++) v |= (uint64_t)s[pc + 1 + i] << (8 * i);
      if (pc + 1 + lb + v > n) return total;
      pc += 1 + lb + v;
    } else {
      if (op == 0xac || op == 0xad) total += 1;
      if (op == 0xae || op == 0xaf) total += 20;  // MAX_PUBKEYS_PER_MULTISIG
      pc += 1;
    }
  }
  return total;
}

constexpr size_t BLOCK_HEADER_BYTES = 1487;  // include/zg.h ZG_HEADER_BYTES
constexpr uint64_t BLOCK_NO_INDEX = ~0ull;

struct BlockLayout {
  uint64_t n_tx = 0, size = 0, sigops = 0, coinbase0 = 0, extra_coinbase = BLOCK_NO_INDEX, consumed = 0;
  std::vector<uint64_t> tx_off;  // n_tx + 1 offsets from the block's first byte (ZG_TXP_OK / NONCANONICAL)
};

// Block::deserialize over exactly b[0..len), len <= 2^31 -> ZG_TXP_*. MALFORMED: truncated anywhere, bytes
// 140..142 not fd 40 05, a malformed transaction, bytes left over (B is then as constructed). NONCANONICAL: a
// non-minimal compact size anywhere, the transaction count included; B is filled as for OK, size being what
// the reference's writer would emit.
inline uint32_t block_layout(const uint8_t* b, size_t len, BlockLayout& B) {
  B = BlockLayout{};
  if (len < BLOCK_HEADER_BYTES + 1 || b[140] != 0xfd || b[141] != 0x40 || b[142] != 0x05) return ZG_TXP_MALFORMED;
  TxReader r{b, len};
  r.o = BLOCK_HEADER_BYTES;
  const uint64_t n = r.count(10);  // header 4, two counts, lock_time 4: the shortest transaction
  if (r.bad) return ZG_TXP_MALFORMED;
  BlockLayout L;
  L.n_tx = n;
  L.tx_off.reserve((size_t)n + 1);
  std::vector<uint32_t> in_off, out_off;
  uint64_t excess = r.excess;
  bool nc = r.noncanonical;
  for (uint64_t t = 0; t < n; t++) {
    const uint8_t* tx = b + r.o;
    TxLayout T;
    uint64_t ex = 0;
    in_off.clear();
    out_off.clear();
    const uint32_t st = tx_parse_prefix(tx, r.left(), T, in_off, out_off, &ex);
    if (st == ZG_TXP_MALFORMED) return ZG_TXP_MALFORMED;
    nc |= st == ZG_TXP_NONCANONICAL;
    excess += ex;
    bool coinbase = T.n_in == 1;
    if (coinbase) {
      for (int i = 0; i < 32; i++) coinbase &= tx[in_off[0] + i] == 0;
      for (int i = 32; i < 36; i++) coinbase &= tx[in_off[0] + i] == 0xff;
    }
    if (coinbase && t == 0) L.coinbase0 = 1;
    if (coinbase && t != 0 && L.extra_coinbase == BLOCK_NO_INDEX) L.extra_coinbase = t;
    // the scripts: each behind its compact length, which the parser has already walked
    for (uint32_t i = 0; i < T.n_out; i++) {
      TxReader s{tx, out_off[i + 1]};
      s.o = out_off[i] + 8;
      const uint64_t sl = s.compact();
      L.sigops += script_sigops(tx + s.o, sl);
    }
    for (uint32_t i = 0; i < T.n_in && !coinbase; i++) {
      TxReader s{tx, in_off[i + 1]};
      s.o = in_off[i] + 36;
      const uint64_t sl = s.compact();
      L.sigops += script_sigops(tx + s.o, sl);
    }
    L.tx_off.push_back(r.o);
    r.o += T.consumed;
  }
  L.tx_off.push_back(r.o);
  if (r.o != len) return ZG_TXP_MALFORMED;
  L.consumed = r.o;
  L.size = r.o - excess;
  B = std::move(L);
  return nc ? ZG_TXP_NONCANONICAL : ZG_TXP_OK;
}

}  // namespace zg
