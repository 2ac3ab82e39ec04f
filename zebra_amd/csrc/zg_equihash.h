// zg_equihash.h -- the block-header checks on gfx950: the Equihash solution
// (verification/src/equihash.rs), the block hash (chain/src/block_header.rs:64-66) and the proof of
// work (verification/src/work.rs:21-34, primitives/src/compact.rs:45-66).
//
// Equihash<N, K>, one lane per leaf (2^K leaves), 2^K lanes per solution, a 512-lane workgroup per
// (200, 9) header and 8 solutions per 256-lane workgroup for the 32-leaf instances:
//   1. each lane unpacks its (N/(K+1) + 1)-bit index from the big-endian bit stream (expand_array);
//   2. BLAKE2b(person = "ZcashPoW" || LE32(N) || LE32(K), out = (512/N) N/8) over input || LE32(index /
//      (512/N)): the input is staged once per solution in LDS (zero-padded to 256 bytes); when it has
//      128 bytes or more the first compression is the same for every leaf, so one lane computes that
//      midstate and each lane runs only the final compression;
//   3. the lane's N-bit string goes to LDS as big-endian packed words (7 / 3 / 2 words: the chunks
//      are bit ranges of them, not the reference's padded bytes);
//   4. K levels of a pairwise XOR tree, a barrier per level: at level l the merged row's chunk l
//      must be zero (has_collision), and every leaf of a right subtree compares its index with the
//      first index of the left sibling subtree -- the subtree's first leaf must be larger
//      (indices_before(row2, row1) false and, with the equality case, distinct_indices' i = 0
//      pass), every other leaf must differ (distinct_indices AS WRITTEN, equihash.rs:258-274: `j` is
//      never reset, so only the left row's FIRST index is compared with the right row). An accepted
//      pair keeps its order in merge_rows, so a row's first index is its leftmost leaf's;
//   5. the last chunk of the root must be zero (equihash.rs:171).
// The verdict is the reference's, including the solutions with a repeated index it accepts; whether
// any two of the 2^K indices are equal (the specification's rule) is reported beside it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zg_hash.h"  // blake2b_init, blake2b_compress, sha256_compress

#define ZG_HD __host__ __device__

namespace zg {

// ---- Compact::to_u256 (compact.rs:45-66) as written: `word` is shifted BEFORE the sign and overflow
// tests when size <= 3, so 0x01803456 is no negative number; the value is truncated to 256 bits like
// U256's <<. out: 8 LE words. false = Err (negative or overflow).
ZG_HD inline bool compact_to_u256(uint32_t c, uint32_t out[8]) {
  const uint32_t size = c >> 24;
  uint32_t word = c & 0x007fffffu;
  for (int i = 0; i < 8; i++) out[i] = 0;
  if (size <= 3) {
    word >>= 8 * (3 - size);
    out[0] = word;
  } else {
    const uint32_t sh = size - 3;  // bytes
    for (uint32_t b = 0; b < 3; b++) {
      const uint32_t pos = sh + b;
      if (pos < 32) out[pos >> 2] |= ((word >> (8 * b)) & 0xffu) << (8 * (pos & 3));
    }
  }
  const bool is_negative = word != 0 && (c & 0x00800000u) != 0;
  const bool is_overflow = (word != 0 && size > 34) || (word > 0xff && size > 33) || (word > 0xffff && size > 32);
  return !(is_negative || is_overflow);
}

// a <= b over 8 LE words
ZG_HD inline bool u256_le(const uint32_t a[8], const uint32_t b[8]) {
  for (int i = 7; i >= 0; i--) {
    if (a[i] < b[i]) return true;
    if (a[i] > b[i]) return false;
  }
  return true;
}

// is_valid_proof_of_work (work.rs:21-34); hash: 8 LE words of the H256 in storage order (the value
// is U256::from(hash.reversed()), i.e. the storage bytes read little-endian)
ZG_HD inline bool pow_valid_words(uint32_t max_bits, uint32_t bits, const uint32_t hash[8]) {
  uint32_t maximum[8], target[8];
  if (!compact_to_u256(max_bits, maximum)) return false;
  if (!compact_to_u256(bits, target)) return false;
  return u256_le(target, maximum) && u256_le(hash, target);
}

}  // namespace zg
