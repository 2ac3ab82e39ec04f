// zg_equihash.hip -- the kernels of zg_equihash.h and zg_pow_valid.
//   k_equihash<N, K>   verify_equihash_solution (verification/src/equihash.rs:80-172), 2^K lanes per solution
//   k_header_pow       one lane per header: the block hash (dhash256 of the 1487 serialized bytes,
//                      chain/src/block_header.rs:64-66), is_valid_proof_of_work, and the status / flags
//                      of zg_headers_verify from the Equihash verdicts of k_equihash<200, 9>
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_equihash.h"

namespace zg {

template <int N, int K>
struct EqParams {
  static constexpr int CB = N / (K + 1);          // chunk (collision) bits
  static constexpr int IB = CB + 1;               // index bits
  static constexpr int LEAVES = 1 << K;
  static constexpr int SPH = 512 / N;             // strings per hash
  static constexpr int NB = N / 8;                // bytes per string
  static constexpr int HASH_BYTES = SPH * NB;
  static constexpr int SOL_BYTES = LEAVES * IB / 8;
  static constexpr int W = (N + 31) / 32;         // LDS words per string
  static constexpr int SPW = LEAVES >= 256 ? 1 : 256 / LEAVES;  // solutions per workgroup
  static constexpr int BLOCK = LEAVES * SPW;
  static_assert(CB * (K + 1) == N && N % 8 == 0 && IB <= 25 && CB <= 32, "unsupported Equihash instance");
};

// byte i (a constant) of the BLAKE2b output held in h
#define ZG_B2_BYTE(h, i) ((uint32_t)((h)[(i) >> 3] >> (8 * ((i) & 7))) & 0xffu)

// the CB bits from bit `start` (0 = the most significant bit of word 0) of big-endian packed words
template <int CB>
ZG_HD __forceinline__ uint32_t eq_chunk(const uint32_t* w, int start) {
  const int wi = start >> 5, off = start & 31;
  const uint32_t mask = CB == 32 ? 0xffffffffu : ((1u << CB) - 1u);
  if (off + CB <= 32) return (w[wi] >> (32 - off - CB)) & mask;
  return ((w[wi] << (off + CB - 32)) | (w[wi + 1] >> (64 - off - CB))) & mask;
}

// m = the 128 message bytes of block `blk` (staged, zero-padded, as LE words) with LE32(g) at byte in_len
ZG_HD __forceinline__ void eq_block(uint64_t m[16], const uint64_t* msg, int blk, int in_len, uint32_t g) {
  const int p = in_len - 128 * blk;  // where the index starts in this block (may lie outside)
#pragma unroll
  for (int w = 0; w < 16; w++) {
    uint64_t x = msg[16 * blk + w];
    const int sh = p - 8 * w;  // bytes
    if (sh >= 0 && sh < 8) x |= (uint64_t)g << (8 * sh);
    if (sh < 0 && sh > -4) x |= (uint64_t)g >> (8 * -sh);
    m[w] = x;
  }
}

template <int N, int K>
__global__ void __launch_bounds__((EqParams<N, K>::BLOCK))
k_equihash(const uint8_t* __restrict__ inputs, size_t in_stride, int in_len, const uint8_t* __restrict__ sols,
           size_t sol_stride, int n, uint8_t* __restrict__ ok, uint8_t* __restrict__ repeated) {
  using P = EqParams<N, K>;
  __shared__ __attribute__((aligned(16))) uint32_t s_idx[P::SPW][P::LEAVES];
  __shared__ uint32_t s_rows[P::SPW][P::LEAVES][P::W];
  __shared__ __attribute__((aligned(16))) uint64_t s_msg[P::SPW][32];
  __shared__ uint64_t s_mid[P::SPW][8];
  __shared__ int s_fail[P::SPW], s_rep[P::SPW];

  const int s = threadIdx.x / P::LEAVES, leaf = threadIdx.x % P::LEAVES;
  const long long item_raw = (long long)blockIdx.x * P::SPW + s;
  // the tail workgroup's spare groups redo the last item (every lane reaches every barrier) and write nothing
  const bool live = item_raw < n;
  const size_t item = live ? (size_t)item_raw : (size_t)(n - 1);
  const uint8_t* in = inputs + item * in_stride;
  const uint8_t* sol = sols + item * sol_stride;

  // 1. this leaf's index: IB bits at bit leaf * IB of the big-endian stream (never past SOL_BYTES)
  uint32_t idx;
  {
    const int bit = leaf * P::IB, o = bit >> 3;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) v = (v << 8) | (o + b < P::SOL_BYTES ? (uint32_t)sol[o + b] : 0u);
    idx = (v >> (32 - (bit & 7) - P::IB)) & ((1u << P::IB) - 1u);
  }
  s_idx[s][leaf] = idx;
  if (leaf == 0) s_fail[s] = 0, s_rep[s] = 0;
  // the input, zero-padded to two BLAKE2b blocks
  {
    uint8_t* mb = (uint8_t*)s_msg[s];
    for (int j = leaf; j < 256; j += P::LEAVES) mb[j] = j < in_len ? in[j] : (uint8_t)0;
  }
  __syncthreads();

  // 2. BLAKE2b(input || LE32(idx / SPH))
  const uint32_t g = idx / P::SPH;
  const int total = in_len + 4;  // 5..256
  uint64_t h[8], m[16];
  blake2b_init(h, P::HASH_BYTES, 0x576f50687361635aull /* "ZcashPoW" */, (uint64_t)N | ((uint64_t)K << 32));
  if (in_len >= 128) {  // uniform: the first block holds no index byte, one lane per solution compresses it
    if (leaf == 0) {
#pragma unroll
      for (int w = 0; w < 16; w++) m[w] = s_msg[s][w];
      blake2b_compress(h, m, 128, false);
#pragma unroll
      for (int i = 0; i < 8; i++) s_mid[s][i] = h[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = s_mid[s][i];
  } else if (total > 128) {  // 125..127 input bytes: the index straddles the blocks
    eq_block(m, s_msg[s], 0, in_len, g);
    blake2b_compress(h, m, 128, false);
  }
  eq_block(m, s_msg[s], total > 128 ? 1 : 0, in_len, g);
  blake2b_compress(h, m, (uint64_t)total, true);

  // 3. the lane's string (bytes r NB .. r NB + NB of the hash) as big-endian packed words
  {
    const uint32_t r = idx % P::SPH;
    uint32_t row[P::W];
#pragma unroll
    for (int j = 0; j < P::W; j++) row[j] = 0;
#pragma unroll
    for (int rr = 0; rr < P::SPH; rr++) {
      if ((uint32_t)rr == r) {
#pragma unroll
        for (int b = 0; b < P::NB; b++) row[b >> 2] |= ZG_B2_BYTE(h, rr * P::NB + b) << (24 - 8 * (b & 3));
      }
    }
#pragma unroll
    for (int j = 0; j < P::W; j++) s_rows[s][leaf][j] = row[j];
  }
  __syncthreads();

  // 4. index rules of every level for this leaf, then the XOR tree
  bool bad = false;
#pragma unroll
  for (int l = 0; l < K; l++) {
    if (leaf & (1 << l)) {
      const uint32_t first = s_idx[s][leaf & ~((2 << l) - 1)];  // the left sibling subtree's first index
      const bool head = (leaf & ((1 << l) - 1)) == 0;              // this leaf is its subtree's first
      bad |= head ? (first >= idx) : (first == idx);
    }
  }
  // any two indices equal (the specification's rule; reported, not part of the verdict)
  {
    int same = 0;
    const uint4* q = (const uint4*)s_idx[s];
    for (int j = 0; j < P::LEAVES / 4; j++) {
      const uint4 a = q[j];
      same += (a.x == idx) + (a.y == idx) + (a.z == idx) + (a.w == idx);
    }
    if (same > 1) s_rep[s] = 1;
  }
#pragma unroll
  for (int l = 0; l < K; l++) {
    if ((leaf & ((2 << l) - 1)) == 0) {
      uint32_t* a = s_rows[s][leaf];
      const uint32_t* b = s_rows[s][leaf + (1 << l)];
#pragma unroll
      for (int j = 0; j < P::W; j++) a[j] ^= b[j];
      bad |= eq_chunk<P::CB>(a, l * P::CB) != 0;
    }
    __syncthreads();
  }
  // 5. the root's last chunk
  if (leaf == 0) bad |= eq_chunk<P::CB>(s_rows[s][0], K * P::CB) != 0;
  if (bad) s_fail[s] = 1;
  __syncthreads();
  if (leaf == 0 && live) {
    ok[item] = s_fail[s] ? 0 : 1;
    if (repeated) repeated[item] = (uint8_t)s_rep[s];
  }
}

template <int N, int K>
static hipError_t launch_eq(hipStream_t st, const uint8_t* inputs, size_t in_stride, int in_len, const uint8_t* sols,
                            size_t sol_stride, int n, uint8_t* ok, uint8_t* repeated) {
  using P = EqParams<N, K>;
  hipLaunchKernelGGL((k_equihash<N, K>), dim3((n + P::SPW - 1) / P::SPW), dim3(P::BLOCK), 0, st, inputs, in_stride,
                     in_len, sols, sol_stride, n, ok, repeated);
  return hipGetLastError();
}

int equihash_solution_bytes(int params) {
  switch (params) {
    case ZG_EQ_200_9: return EqParams<200, 9>::SOL_BYTES;
    case ZG_EQ_96_5: return EqParams<96, 5>::SOL_BYTES;
    case ZG_EQ_48_5: return EqParams<48, 5>::SOL_BYTES;
  }
  return 0;
}

// 1 <= in_len <= 252 (input || LE32(index) fits two BLAKE2b blocks)
hipError_t launch_equihash(hipStream_t st, int params, const uint8_t* inputs, size_t in_stride, int in_len,
                           const uint8_t* sols, size_t sol_stride, int n, uint8_t* ok, uint8_t* repeated) {
  if (in_len < 1 || in_len > 252) return hipErrorInvalidValue;
  switch (params) {
    case ZG_EQ_200_9: return launch_eq<200, 9>(st, inputs, in_stride, in_len, sols, sol_stride, n, ok, repeated);
    case ZG_EQ_96_5: return launch_eq<96, 5>(st, inputs, in_stride, in_len, sols, sol_stride, n, ok, repeated);
    case ZG_EQ_48_5: return launch_eq<48, 5>(st, inputs, in_stride, in_len, sols, sol_stride, n, ok, repeated);
  }
  return hipErrorInvalidValue;
}

// eq_ok / eq_rep: the verdicts of k_equihash<200, 9> over the same headers (same stream, launched before)
__global__ void __launch_bounds__(64)
k_header_pow(const uint8_t* __restrict__ headers, int n, uint32_t max_bits, const uint8_t* __restrict__ eq_ok,
             const uint8_t* __restrict__ eq_rep, uint8_t* __restrict__ status, uint8_t* __restrict__ hashes,
             uint8_t* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = headers + (size_t)i * ZG_HEADER_BYTES;
  // SHA-256 of 1487 bytes: 23 full blocks, then 15 bytes || 80 || zeros || the bit length
  uint32_t st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  constexpr int BLOCKS = (ZG_HEADER_BYTES + 9 + 63) / 64;
#pragma unroll 1
  for (int b = 0; b < BLOCKS; b++) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      uint32_t x = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int j = 64 * b + 4 * k + q;
        const uint32_t byte = j < ZG_HEADER_BYTES ? (uint32_t)p[j] : (j == ZG_HEADER_BYTES ? 0x80u : 0u);
        x = (x << 8) | byte;
      }
      w[k] = x;
    }
    if (b == BLOCKS - 1) w[15] = 8u * ZG_HEADER_BYTES;
    sha256_compress(st, w);
  }
  // SHA-256 of those 32 bytes: one block from the IV
  uint32_t lw[8], rw[8], hash[8];
#pragma unroll
  for (int k = 0; k < 8; k++) lw[k] = __builtin_bswap32(st[k]), rw[k] = 0;
  rw[0] = 0x00000080u;
  rw[7] = 0x00010000u;  // 256 bits, big-endian, read as an LE word
  sha256_compress_words(lw, rw, hash);

  const uint32_t bits = (uint32_t)p[104] | ((uint32_t)p[105] << 8) | ((uint32_t)p[106] << 16) | ((uint32_t)p[107] << 24);
  const bool pow = pow_valid_words(max_bits, bits, hash);
  const bool malformed = p[140] != 0xfd || p[141] != 0x40 || p[142] != 0x05;  // the compact size of 1344
  const bool eq = eq_ok[i] != 0;
  status[i] = malformed ? ZG_HDR_MALFORMED : !eq ? ZG_HDR_EQUIHASH : !pow ? ZG_HDR_POW : ZG_HDR_OK;
  if (flags) flags[i] = (uint8_t)((eq ? 0 : ZG_HDR_F_EQUIHASH) | (pow ? 0 : ZG_HDR_F_POW) | (eq_rep[i] ? ZG_HDR_F_REPEATED : 0));
  if (hashes) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
      hashes[(size_t)32 * i + 4 * k + 0] = (uint8_t)hash[k];
      hashes[(size_t)32 * i + 4 * k + 1] = (uint8_t)(hash[k] >> 8);
      hashes[(size_t)32 * i + 4 * k + 2] = (uint8_t)(hash[k] >> 16);
      hashes[(size_t)32 * i + 4 * k + 3] = (uint8_t)(hash[k] >> 24);
    }
  }
}

// the two kernels of zg_headers_verify: eq_ok / eq_rep are n-byte device scratch
hipError_t launch_headers(hipStream_t st, const uint8_t* headers, int n, uint32_t max_bits, uint8_t* eq_ok,
                          uint8_t* eq_rep, uint8_t* status, uint8_t* hashes, uint8_t* flags) {
  hipError_t e = launch_eq<200, 9>(st, headers, ZG_HEADER_BYTES, 140, headers + 143, ZG_HEADER_BYTES, n, eq_ok, eq_rep);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_header_pow, dim3((n + 63) / 64), dim3(64), 0, st, headers, n, max_bits, eq_ok, eq_rep, status,
                     hashes, flags);
  return hipGetLastError();
}

}  // namespace zg

extern "C" int zg_pow_valid(uint32_t max_bits, uint32_t bits, const uint8_t hash[32]) {
  if (!hash) return ZG_E_INVAL;
  uint32_t w[8];
  for (int k = 0; k < 8; k++)
    w[k] = (uint32_t)hash[4 * k] | ((uint32_t)hash[4 * k + 1] << 8) | ((uint32_t)hash[4 * k + 2] << 16) |
           ((uint32_t)hash[4 * k + 3] << 24);
  return zg::pow_valid_words(max_bits, bits, w) ? 1 : 0;
}
