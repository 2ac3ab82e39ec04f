// zg_txparse.h -- the layout of one serialized transaction, host side (no HIP runtime: a stand-alone
// program includes it). Restates over one exact byte slice
//   Transaction::deserialize          chain/src/transaction.rs:249-330
//   deserialize_join_split            chain/src/join_split.rs:149-186
//   CompactInteger::deserialize       serialization/src/compact_integer.rs:95-105
// and keeps, instead of the parsed values, where the pieces the signature hash covers (zg_sighash.h)
// lie in the slice. Every offset it hands out is inside the slice; nothing downstream checks again.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zg {

// One record per transaction; every *_off is a byte offset from the transaction's first byte.
struct TxLayout {
  uint32_t header, vgid;        // the header word (version | overwintered << 31); the version group id (0: none)
  uint32_t n_in, in_idx;        // inputs; where this transaction's n_in + 1 input offsets start in the table
  uint32_t n_out, out_idx;      // outputs; likewise n_out + 1 output offsets
  uint32_t lock_off, expiry_off, value_off;  // lock_time; expiry_height (overwintered); the balancing value (v4)
  uint32_t n_spend, spend_off;  // Sapling spends, 384 B each
  uint32_t n_sout, sout_off;    // Sapling outputs, 948 B each
  uint32_t n_js, js_size, js_off, jspub_off;  // JoinSplit descriptions (1802 B PHGR / 1698 B Groth), the pubkey
  uint32_t sigver;              // 0 Sprout, 1 Overwinter, 2 Sapling (script/src/sign.rs:331-341)
  uint32_t consumed;            // bytes read: the slice's length
};

constexpr uint32_t ZG_TXP_OK = 0, ZG_TXP_MALFORMED = 1, ZG_TXP_NONCANONICAL = 2;  // include/zg.h ZG_TX_*
constexpr uint32_t OVERWINTER_VGID = 0x03C48270u, SAPLING_VGID = 0x892F2085u;

struct TxReader {
  const uint8_t* d;
  size_t len, o = 0;
  bool bad = false, noncanonical = false;
  uint64_t excess = 0;  // bytes the non-minimal compact sizes read so far take beyond their shortest forms

  size_t left() const { return len - o; }
  bool skip(uint64_t k) {
    if (bad || k > left()) return !(bad = true);
    o += (size_t)k;
    return true;
  }
  uint64_t le(int bytes) {
    if (bad || (size_t)bytes > left()) {
      bad = true;
      return 0;
    }
    uint64_t v = 0;
    for (int i = bytes - 1; i >= 0; i--) v = (v << 8) | d[o + i];
    o += bytes;
    return v;
  }
  // the reference's reader takes any of the four forms for any value; its writer emits the shortest
  uint64_t compact() {
    const uint64_t b = le(1);
    if (bad || b < 0xfd) return b;
    const uint64_t v = le(b == 0xfd ? 2 : b == 0xfe ? 4 : 8);
    if (b == 0xfd ? v < 0xfd : b == 0xfe ? v <= 0xffff : v <= 0xffffffffull) {
      noncanonical = true;
      excess += (b == 0xfd ? 3 : b == 0xfe ? 5 : 9) - (v < 0xfd ? 1 : v <= 0xffff ? 3 : v <= 0xffffffffull ? 5 : 9);
    }
    return v;
  }
  // a list count: `min_size` bytes at least per element must still be there (checked before the caller
  // stores anything per element, so what a transaction makes the tables grow by is bounded by its length)
  uint64_t count(size_t min_size) {
    const uint64_t n = compact();
    if (!bad && n > left() / min_size) bad = true;
    return bad ? 0 : n;
  }
};

// The one parser behind tx_parse and tx_parse_prefix. exact: the transaction must end where the slice
// does; otherwise it ends where its last field does and L.consumed says where (the list counts are then
// bounded by what is left of the slice, whatever follows the transaction in it). keep_nc: a
// non-canonical transaction keeps its layout and its offsets like a canonical one. excess (optional):
// the bytes its non-minimal compact sizes take beyond their shortest forms.
inline uint32_t tx_parse_impl(const uint8_t* tx, size_t len, bool exact, bool keep_nc, TxLayout& L,
                              std::vector<uint32_t>& in_off, std::vector<uint32_t>& out_off, uint64_t* excess) {
  const size_t in0 = in_off.size(), out0 = out_off.size();
  L = TxLayout{};
  TxReader r{tx, len};
  L.header = (uint32_t)r.le(4);
  const bool ow = (L.header & 0x80000000u) != 0;
  const uint32_t version = L.header & 0x7fffffffu;
  L.vgid = ow ? (uint32_t)r.le(4) : 0;
  if (r.bad) return ZG_TXP_MALFORMED;
  const bool is_ow = ow && version == 3 && L.vgid == OVERWINTER_VGID;
  const bool is_sap = ow && version == 4 && L.vgid == SAPLING_VGID;
  if (ow && !is_ow && !is_sap) return ZG_TXP_MALFORMED;
  L.sigver = !ow ? 0 : L.vgid == SAPLING_VGID ? 2 : 1;

  auto fail = [&]() {
    in_off.resize(in0);
    out_off.resize(out0);
    return ZG_TXP_MALFORMED;
  };
  L.n_in = (uint32_t)r.count(41);  // outpoint 36, script length 1, sequence 4
  if (r.bad) return fail();
  L.in_idx = (uint32_t)in0;
  for (uint32_t i = 0; i < L.n_in; i++) {
    in_off.push_back((uint32_t)r.o);
    r.skip(36);
    r.skip(r.compact());
    r.skip(4);
    if (r.bad) return fail();
  }
  in_off.push_back((uint32_t)r.o);
  L.n_out = (uint32_t)r.count(9);  // value 8, script length 1
  if (r.bad) return fail();
  L.out_idx = (uint32_t)out0;
  for (uint32_t i = 0; i < L.n_out; i++) {
    out_off.push_back((uint32_t)r.o);
    r.skip(8);
    r.skip(r.compact());
    if (r.bad) return fail();
  }
  out_off.push_back((uint32_t)r.o);
  L.lock_off = (uint32_t)r.o;
  r.skip(4);
  L.expiry_off = (uint32_t)r.o;
  if (ow) r.skip(4);
  L.value_off = (uint32_t)r.o;
  if (is_sap) {
    r.skip(8);
    L.n_spend = (uint32_t)r.count(384);
    L.spend_off = (uint32_t)r.o;
    r.skip((uint64_t)384 * L.n_spend);
    L.n_sout = (uint32_t)r.count(948);
    L.sout_off = (uint32_t)r.o;
    r.skip((uint64_t)948 * L.n_sout);
  }
  if (r.bad) return fail();
  if (version >= 2) {
    L.js_size = is_sap ? 1698 : 1802;  // Groth16 proof 192 B, PHGR proof 296 B
    L.n_js = (uint32_t)r.count(L.js_size);
    L.js_off = (uint32_t)r.o;
    r.skip((uint64_t)L.js_size * L.n_js);
    L.jspub_off = (uint32_t)r.o;
    if (L.n_js) r.skip(32 + 64);  // the pubkey and the signature
  }
  if (is_sap && (L.n_spend || L.n_sout)) r.skip(64);  // the binding signature
  if (r.bad || (exact && r.o != len)) return fail();
  L.consumed = (uint32_t)r.o;
  if (excess) *excess = r.excess;
  if (r.noncanonical) {
    if (!keep_nc) {
      in_off.resize(in0);
      out_off.resize(out0);
    }
    return ZG_TXP_NONCANONICAL;
  }
  return ZG_TXP_OK;
}

// Parses tx[0..len), len <= 2^31. On ZG_TXP_OK fills L and appends n_in + 1 input offsets and n_out + 1
// output offsets (the last of each: the end of the list) to in_off / out_off, L.in_idx / L.out_idx being
// where they start. On any other status the two vectors are as they were.
inline uint32_t tx_parse(const uint8_t* tx, size_t len, TxLayout& L, std::vector<uint32_t>& in_off,
                         std::vector<uint32_t>& out_off) {
  return tx_parse_impl(tx, len, true, false, L, in_off, out_off, nullptr);
}

// The prefix form (zg_blocks.h: the transactions of a block lie back to back): the same rules over the
// transaction that starts at p, of which `left` bytes of the block remain; it ends where its last field
// does, L.consumed bytes on. A non-canonical transaction keeps its layout and offsets (the caller still
// walks its scripts); *excess: see tx_parse_impl. On ZG_TXP_MALFORMED the two vectors are as they were.
inline uint32_t tx_parse_prefix(const uint8_t* p, size_t left, TxLayout& L, std::vector<uint32_t>& in_off,
                                std::vector<uint32_t>& out_off, uint64_t* excess) {
  return tx_parse_impl(p, left, false, true, L, in_off, out_off, excess);
}

}  // namespace zg
