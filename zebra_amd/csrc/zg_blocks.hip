// zg_blocks.hip -- the kernels of zg_blocks.h and zg_block_layout. k_txid: lane per
// slice, dhash256 of a contiguous range of the arena; the host hands the slices over longest first, so a
// wave's lanes run similar lengths, each hash going to the row its slice names. k_block_merkle: workgroup
// per block, the Bitcoin merkle tree over that block's rows, the root compared with the header's field.
// Every offset a lane follows was checked by the host (zg_calls.hip: zg_txids, zg_blocks_verify).
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_blocks.h"

namespace zg {

constexpr int MERKLE_THREADS = 256;

// 128 VGPRs at most: four waves per SIMD, which the read-ahead needs to have something to switch to
__global__ void __launch_bounds__(64, 4)
k_txid(const uint8_t* __restrict__ arena, const TxidSlice* __restrict__ slices, int n, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 sv = *(const uint4*)(slices + i);
  uint32_t h[8];
  txid_hash(arena, sv.x, sv.y, h);
  uint4* o = (uint4*)(out + (size_t)32 * sv.z);
  o[0] = make_uint4(h[0], h[1], h[2], h[3]);
  o[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

ZG_BLK_HD void row_load(const uint8_t* rows, size_t i, uint32_t x[8]) {
  const uint4* p = (const uint4*)(rows + 32 * i);
  const uint4 a = p[0], b = p[1];
  x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
}

// ids: the rows k_txid wrote (read only). ping, pong: as many rows each; a level reads one buffer and writes
// the other, a barrier between levels, so no lane overwrites a row another lane has yet to read.
// roots: 32 B per block (zero for a block without rows); match: 1 when the root is the header's bytes 36..67.
__global__ void __launch_bounds__(MERKLE_THREADS)
k_block_merkle(const uint8_t* __restrict__ arena, const MerkleBlk* __restrict__ blks, const uint8_t* ids,
               uint8_t* ping, uint8_t* pong, uint8_t* __restrict__ roots, uint8_t* __restrict__ match) {
  const MerkleBlk b = blks[blockIdx.x];
  const uint8_t* src = ids + (size_t)32 * b.row0;
  uint8_t* dst = ping + (size_t)32 * b.row0;
  uint8_t* other = pong + (size_t)32 * b.row0;
  uint32_t cur = b.n;  // uniform over the workgroup, and so is every branch on it
  while (cur > 1) {
    const uint32_t m = (cur + 1) / 2;
    for (uint32_t i = threadIdx.x; i < m; i += MERKLE_THREADS) {
      uint32_t l[8], r[8], o[8];
      row_load(src, 2 * i, l);
      row_load(src, 2 * i + 1 < cur ? 2 * i + 1 : 2 * i, r);  // an odd row: its last element with itself
      merkle_node(l, r, o);
      uint4* q = (uint4*)(dst + (size_t)32 * i);
      q[0] = make_uint4(o[0], o[1], o[2], o[3]);
      q[1] = make_uint4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
    src = dst;
    uint8_t* t = dst;
    dst = other;
    other = t;
    cur = m;
  }
  if (threadIdx.x == 0) {
    uint8_t* root = roots + (size_t)32 * blockIdx.x;
    bool same = cur == 1;
    for (int i = 0; i < 32; i++) {
      const uint8_t v = cur == 1 ? src[i] : (uint8_t)0;
      root[i] = v;
      same &= v == arena[(size_t)b.hdr_off + 36 + i];
    }
    match[blockIdx.x] = same ? 1 : 0;
  }
}

hipError_t launch_txid(hipStream_t st, const uint8_t* arena, const TxidSlice* slices, int n, uint8_t* out) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_txid, dim3((n + 63) / 64), dim3(64), 0, st, arena, slices, n, out);
  return hipGetLastError();
}

hipError_t launch_block_merkle(hipStream_t st, const uint8_t* arena, const MerkleBlk* blks, int nblk,
                               const uint8_t* ids, uint8_t* ping, uint8_t* pong, uint8_t* roots, uint8_t* match) {
  if (!nblk) return hipSuccess;
  hipLaunchKernelGGL(k_block_merkle, dim3(nblk), dim3(MERKLE_THREADS), 0, st, arena, blks, ids, ping, pong, roots,
                     match);
  return hipGetLastError();
}

}  // namespace zg

extern "C" int zg_block_layout(const uint8_t* block, size_t len, uint64_t* out, uint64_t* tx_off, size_t tx_off_cap) {
  if (!block || !out || len > ((size_t)1 << 31)) return ZG_E_INVAL;
  zg::BlockLayout B;
  const uint32_t st = zg::block_layout(block, len, B);
  for (int i = 0; i < 6; i++) out[i] = 0;
  if (st != zg::ZG_TXP_MALFORMED) {
    out[0] = B.n_tx, out[1] = B.size, out[2] = B.sigops, out[3] = B.coinbase0, out[4] = B.extra_coinbase;
    out[5] = B.consumed;
    if (tx_off && tx_off_cap >= B.tx_off.size())
      for (size_t i = 0; i < B.tx_off.size(); i++) tx_off[i] = B.tx_off[i];
  }
  return (int)st;
}
