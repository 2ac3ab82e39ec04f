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

#ifdef __HIPCC__
// ---- BLAKE2b (RFC 7693) compression on one lane, 64-bit words in plain C++. The rotation by 32 is a
// renaming of the register pair; those by 24, 16 and 63 are written over the two halves with the
// 32-bit funnel shift (v_alignbit_b32, one per half): left as (x >> k) | (x << (64 - k)) the compiler
// emits a 64-bit shift, a 32-bit shift and an or per rotation.
template <int K>
ZG_HD __forceinline__ uint64_t b2_rotr(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (K == 32) return ((uint64_t)lo << 32) | hi;
  if (K < 32)
    return ((uint64_t)__builtin_amdgcn_alignbit(lo, hi, K) << 32) | __builtin_amdgcn_alignbit(hi, lo, K);
  return ((uint64_t)__builtin_amdgcn_alignbit(hi, lo, K - 32) << 32) | __builtin_amdgcn_alignbit(lo, hi, K - 32);
#else
  return (x >> K) | (x << (64 - K));
#endif
}

ZG_HD __forceinline__ void blake2b_init(uint64_t h[8], uint32_t outlen, uint64_t person0, uint64_t person1) {
  const uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                          0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = iv[i];
  h[0] ^= 0x01010000ull ^ (uint64_t)outlen;
  h[6] ^= person0;  // parameter block bytes 48..63
  h[7] ^= person1;
}

#define ZG_B2_G(a, b, c, d, x, y) \
  do {                            \
    v[a] = v[a] + v[b] + (x);     \
    v[d] = b2_rotr<32>(v[d] ^ v[a]); \
    v[c] = v[c] + v[d];           \
    v[b] = b2_rotr<24>(v[b] ^ v[c]); \
    v[a] = v[a] + v[b] + (y);     \
    v[d] = b2_rotr<16>(v[d] ^ v[a]); \
    v[c] = v[c] + v[d];           \
    v[b] = b2_rotr<63>(v[b] ^ v[c]); \
  } while (0)

// h <- F(h, m, t, last); t < 2^64 (the high counter word is zero)
ZG_HD __forceinline__ void blake2b_compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) {
  constexpr uint8_t S[12][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
  const uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                          0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  uint64_t v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    v[i] = h[i];
    v[i + 8] = iv[i];
  }
  v[12] ^= t;
  if (last) v[14] = ~v[14];
#pragma unroll
  for (int r = 0; r < 12; r++) {
    ZG_B2_G(0, 4, 8, 12, m[S[r][0]], m[S[r][1]]);
    ZG_B2_G(1, 5, 9, 13, m[S[r][2]], m[S[r][3]]);
    ZG_B2_G(2, 6, 10, 14, m[S[r][4]], m[S[r][5]]);
    ZG_B2_G(3, 7, 11, 15, m[S[r][6]], m[S[r][7]]);
    ZG_B2_G(0, 5, 10, 15, m[S[r][8]], m[S[r][9]]);
    ZG_B2_G(1, 6, 11, 12, m[S[r][10]], m[S[r][11]]);
    ZG_B2_G(2, 7, 8, 13, m[S[r][12]], m[S[r][13]]);
    ZG_B2_G(3, 4, 9, 14, m[S[r][14]], m[S[r][15]]);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}
#endif  // __HIPCC__

}  // namespace zg
