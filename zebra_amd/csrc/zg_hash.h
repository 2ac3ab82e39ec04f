// zg_hash.h -- the compression functions of SHA-256, SHA-512 (FIPS 180-4), BLAKE2b (RFC 7693) and
// RIPEMD-160 (Dobbertin, Bosselaers, Preneel 1996), once,
// as force-inlined host/device code on one lane. The callers keep what differs
// between them: how the message words are gathered, the padding and the chaining over blocks
// (zg_merkle.h, zg_equihash.hip, zg_sighash.h, zg_jubjub.h, zg_ed25519.h, zg_blake2b.h, zg_script.hip).
// Every table is constexpr data indexed by unrolled loop counters, so no array is indexed by a run-time
// value and the constants are immediates of the instructions (SHA-512's excepted, see there). Also
// compiles as plain C++ (the host baseline of tools/bench_headers.py).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZG_HASH_HD __host__ __device__ __forceinline__
#else
#define ZG_HASH_HD inline
#endif

namespace zg {

ZG_HASH_HD uint32_t sha_rotr(uint32_t x, int k) { return (x >> k) | (x << (32 - k)); }
ZG_HASH_HD uint64_t sha_rotr64(uint64_t x, int k) { return (x >> k) | (x << (64 - k)); }

// ---- SHA-256: one compression chained on st (6.2.2). w: the 16 message words, big-endian values, used
// as the rolling schedule (clobbered; every index a compile-time constant)
constexpr uint32_t SHA256_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
ZG_HASH_HD void sha256_compress(uint32_t st[8], uint32_t w[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int t = 0; t < 64; t++) {
    uint32_t wt;
    if (t < 16) {
      wt = w[t];
    } else {
      const uint32_t w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
      const uint32_t s0 = sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10);
      wt = w[t & 15] = w[t & 15] + s0 + w[(t - 7) & 15] + s1;
    }
    const uint32_t t1 = h + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) +
                        SHA256_K[t] + wt;
    const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
  }
  st[0] += a, st[1] += b, st[2] += c, st[3] += d, st[4] += e, st[5] += f, st[6] += g, st[7] += h;
}
ZG_HASH_HD void sha256_iv(uint32_t st[8]) {
  const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                          0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = iv[i];
}
// the compression of one 64-byte block from the IV, no padding. lw, rw: the 32 + 32 message bytes as LE
// words (the byte order of H256); out likewise
ZG_HASH_HD void sha256_compress_words(const uint32_t* lw, const uint32_t* rw, uint32_t* out) {
  uint32_t st[8], w[16];
  sha256_iv(st);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    w[i] = __builtin_bswap32(lw[i]);
    w[8 + i] = __builtin_bswap32(rw[i]);
  }
  sha256_compress(st, w);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = __builtin_bswap32(st[i]);
}

// ---- SHA-512 of one 128-byte block (16 big-endian words, already padded). w: the block, used as the
// rolling schedule; out: H0..H7. On the device the round constants are read from a copy of the table in
// constant memory: as 64-bit immediates they cost k_ed25519 4 VGPRs and 127 instructions (DESIGN.md
// section 7f)
struct Sha512K {
  uint64_t k[80];
};
constexpr Sha512K SHA512_K = {{
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull}};
#if defined(__HIPCC__)
__device__ __constant__ const Sha512K SHA512_K_DEV = SHA512_K;
#endif
ZG_HASH_HD void sha512_block(uint64_t* w, uint64_t* out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t* K = SHA512_K_DEV.k;
#else
  const uint64_t* K = SHA512_K.k;
#endif
  uint64_t a = 0x6a09e667f3bcc908ull, b = 0xbb67ae8584caa73bull, c = 0x3c6ef372fe94f82bull,
           d = 0xa54ff53a5f1d36f1ull, e = 0x510e527fade682d1ull, f = 0x9b05688c2b3e6c1full,
           g = 0x1f83d9abfb41bd6bull, h = 0x5be0cd19137e2179ull;
#pragma unroll
  for (int t = 0; t < 80; t++) {
    if (t >= 16) {
      const uint64_t x = w[(t - 15) & 15], y = w[(t - 2) & 15];
      w[t & 15] += (sha_rotr64(x, 1) ^ sha_rotr64(x, 8) ^ (x >> 7)) + w[(t - 7) & 15] +
                   (sha_rotr64(y, 19) ^ sha_rotr64(y, 61) ^ (y >> 6));
    }
    const uint64_t t1 = h + (sha_rotr64(e, 14) ^ sha_rotr64(e, 18) ^ sha_rotr64(e, 41)) + ((e & f) ^ (~e & g)) +
                        K[t] + w[t & 15];
    const uint64_t t2 = (sha_rotr64(a, 28) ^ sha_rotr64(a, 34) ^ sha_rotr64(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + t2;
  }
  out[0] = a + 0x6a09e667f3bcc908ull;
  out[1] = b + 0xbb67ae8584caa73bull;
  out[2] = c + 0x3c6ef372fe94f82bull;
  out[3] = d + 0xa54ff53a5f1d36f1ull;
  out[4] = e + 0x510e527fade682d1ull;
  out[5] = f + 0x9b05688c2b3e6c1full;
  out[6] = g + 0x1f83d9abfb41bd6bull;
  out[7] = h + 0x5be0cd19137e2179ull;
}

// ---- BLAKE2b compression, 64-bit words in plain C++. The rotation by 32 is a renaming of the
// register pair; those by 24, 16 and 63 are written over the two halves with the 32-bit funnel shift
// (v_alignbit_b32, one per half): left as (x >> k) | (x << (64 - k)) the compiler emits a 64-bit
// shift, a 32-bit shift and an or per rotation.
template <int K>
ZG_HASH_HD uint64_t b2_rotr(uint64_t x) {
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

// unkeyed, outlen bytes of digest; person0 / person1: the personalization (parameter block bytes 48..63)
// as two LE words, 0 for none
ZG_HASH_HD void blake2b_init(uint64_t h[8], uint32_t outlen, uint64_t person0, uint64_t person1) {
  const uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                          0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = iv[i];
  h[0] ^= 0x01010000ull ^ (uint64_t)outlen;
  h[6] ^= person0;
  h[7] ^= person1;
}
// 16 personalization bytes as the LE word w (0 or 1) of blake2b_init
ZG_HASH_HD uint64_t blake2b_person(const void* personal, int w) {
  uint64_t p = 0;
  for (int b = 7; b >= 0; b--) p = (p << 8) | ((const uint8_t*)personal)[8 * w + b];
  return p;
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
ZG_HASH_HD void blake2b_compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) {
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
#undef ZG_B2_G
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}

// ---- RIPEMD-160: one compression chained on st (h0..h4). x: the 16 message words, little-endian values
// (not clobbered). The two lines' word orders and rotation amounts are tables indexed by the unrolled
// round counter; a rotation is one 32-bit funnel shift (v_alignbit_b32 with both operands the word).
template <int K>
ZG_HASH_HD uint32_t rmd_rotl(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(x, x, 32 - K);
#else
  return (x << K) | (x >> (32 - K));
#endif
}
// f_j of round group G (0..4): the left line uses group j / 16, the right line 4 - j / 16
template <int G>
ZG_HASH_HD uint32_t rmd_f(uint32_t x, uint32_t y, uint32_t z) {
  return G == 0 ? x ^ y ^ z : G == 1 ? (x & y) | (~x & z) : G == 2 ? (x | ~y) ^ z : G == 3 ? (x & z) | (y & ~z)
                                                                                         : x ^ (y | ~z);
}
struct Rmd160Tables {
  uint8_t rl[80], rr[80], sl[80], sr[80];
};
constexpr Rmd160Tables RMD160_T = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 7, 4, 13, 1, 10, 6, 15, 3, 12, 0, 9, 5, 2, 14, 11, 8,
     3, 10, 14, 4, 9, 15, 8, 1, 2, 7, 0, 6, 13, 11, 5, 12, 1, 9, 11, 10, 0, 8, 12, 4, 13, 3, 7, 15, 14, 5, 6, 2,
     4, 0, 5, 9, 7, 12, 2, 10, 14, 1, 3, 8, 11, 6, 15, 13},
    {5, 14, 7, 0, 9, 2, 11, 4, 13, 6, 15, 8, 1, 10, 3, 12, 6, 11, 3, 7, 0, 13, 5, 10, 14, 15, 8, 12, 4, 9, 1, 2,
     15, 5, 1, 3, 7, 14, 6, 9, 11, 8, 12, 2, 10, 0, 4, 13, 8, 6, 4, 1, 3, 11, 15, 0, 5, 12, 2, 13, 9, 7, 10, 14,
     12, 15, 10, 4, 1, 5, 8, 7, 6, 2, 13, 14, 0, 3, 9, 11},
    {11, 14, 15, 12, 5, 8, 7, 9, 11, 13, 14, 15, 6, 7, 9, 8, 7, 6, 8, 13, 11, 9, 7, 15, 7, 12, 15, 9, 11, 7, 13, 12,
     11, 13, 6, 7, 14, 9, 13, 15, 14, 8, 13, 6, 5, 12, 7, 5, 11, 12, 14, 15, 14, 15, 9, 8, 9, 14, 5, 6, 8, 6, 5, 12,
     9, 15, 5, 11, 6, 8, 13, 12, 5, 12, 13, 14, 11, 8, 5, 6},
    {8, 9, 9, 11, 13, 15, 15, 5, 7, 7, 8, 11, 14, 14, 12, 6, 9, 13, 15, 7, 12, 8, 9, 11, 7, 7, 12, 7, 6, 15, 13, 11,
     9, 7, 15, 11, 8, 6, 6, 14, 12, 13, 5, 14, 13, 13, 7, 5, 15, 5, 8, 11, 14, 14, 6, 14, 6, 9, 12, 9, 12, 5, 15, 8,
     8, 5, 12, 9, 12, 5, 14, 6, 8, 13, 6, 5, 15, 13, 11, 11}};
constexpr uint32_t RMD160_KL[5] = {0x00000000u, 0x5a827999u, 0x6ed9eba1u, 0x8f1bbcdcu, 0xa953fd4eu};
constexpr uint32_t RMD160_KR[5] = {0x50a28be6u, 0x5c4dd124u, 0x6d703ef3u, 0x7a6d76e9u, 0x00000000u};

// one step of a line: (a, b, c, d, e) <- (e, rotl_s(a + f(b, c, d) + x + k) + e, b, rotl_10(c), d)
template <int G, int S>
ZG_HASH_HD void rmd_step(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t& e, uint32_t x, uint32_t k) {
  const uint32_t t = rmd_rotl<S>(a + rmd_f<G>(b, c, d) + x + k) + e;
  a = e, e = d, d = rmd_rotl<10>(c), c = b, b = t;
}
// the 16 steps of round group G on both lines (J: the step within the group, counted down by recursion so
// that the table entries are template arguments)
template <int G, int J>
struct RmdRound {
  static ZG_HASH_HD void run(uint32_t* l, uint32_t* r, const uint32_t* x) {
    constexpr int j = 16 * G + J;
    rmd_step<G, RMD160_T.sl[j]>(l[0], l[1], l[2], l[3], l[4], x[RMD160_T.rl[j]], RMD160_KL[G]);
    rmd_step<4 - G, RMD160_T.sr[j]>(r[0], r[1], r[2], r[3], r[4], x[RMD160_T.rr[j]], RMD160_KR[G]);
    RmdRound<G, J + 1>::run(l, r, x);
  }
};
template <int G>
struct RmdRound<G, 16> {
  static ZG_HASH_HD void run(uint32_t*, uint32_t*, const uint32_t*) {}
};
ZG_HASH_HD void ripemd160_iv(uint32_t st[5]) {
  st[0] = 0x67452301u, st[1] = 0xefcdab89u, st[2] = 0x98badcfeu, st[3] = 0x10325476u, st[4] = 0xc3d2e1f0u;
}
ZG_HASH_HD void ripemd160_compress(uint32_t st[5], const uint32_t x[16]) {
  uint32_t l[5], r[5];
#pragma unroll
  for (int i = 0; i < 5; i++) l[i] = r[i] = st[i];
  RmdRound<0, 0>::run(l, r, x);
  RmdRound<1, 0>::run(l, r, x);
  RmdRound<2, 0>::run(l, r, x);
  RmdRound<3, 0>::run(l, r, x);
  RmdRound<4, 0>::run(l, r, x);
  const uint32_t t = st[1] + l[2] + r[3];
  st[1] = st[2] + l[3] + r[4];
  st[2] = st[3] + l[4] + r[0];
  st[3] = st[4] + l[0] + r[1];
  st[4] = st[0] + l[1] + r[2];
  st[0] = t;
}

}  // namespace zg
