// zg_sighash.hip -- the kernels of zg_sighash.h and zg_tx_layout. Two launches:
// the per-transaction digests of the overwintered transactions some item reads, lane per (transaction,
// digest); then lane per item, the final BLAKE2b of an overwintered item or the streamed double SHA-256 of
// a Sprout one. The host hands the items over ordered by their compression count, so a wave's lanes run
// similar lengths, and validated (zg_txparse.h): every loop is bounded by a count checked there.
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_sighash.h"

namespace zg {

// jobs: (transaction << 3) | digest
__global__ void __launch_bounds__(64)
k_sighash_digests(const uint8_t* __restrict__ arena, const ShDevTx* __restrict__ txs, const uint32_t* __restrict__ in_off,
                  const uint32_t* __restrict__ out_off, const uint32_t* __restrict__ jobs, int njobs,
                  uint8_t* __restrict__ digests) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= njobs) return;
  const uint32_t job = jobs[j];
  const ShDevTx& t = txs[job >> 3];
  const int which = (int)(job & 7);
  sighash_digest(arena + t.base, t.L, in_off + t.L.in_idx, out_off + t.L.out_idx, which,
                 digests + (size_t)32 * (SH_DIGESTS * t.dig + which));
}

// hashes: 32 bytes per launched item, in launch order (the host scatters them to the items' slots)
__global__ void __launch_bounds__(64)
k_sighash_items(const uint8_t* __restrict__ arena, const ShDevTx* __restrict__ txs, const uint32_t* __restrict__ in_off,
                const uint32_t* __restrict__ out_off, const uint8_t* __restrict__ digests,
                const uint8_t* __restrict__ scripts, const ShDevItem* __restrict__ items, int n,
                uint8_t* __restrict__ hashes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ShItem it = sh_item(arena, txs, in_off, out_off, digests, scripts, items[i]);
  sighash_item(it, hashes + (size_t)32 * i);
}

hipError_t launch_sighash_digests(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const uint32_t* in_off,
                                  const uint32_t* out_off, const uint32_t* jobs, int njobs, uint8_t* digests) {
  if (!njobs) return hipSuccess;
  hipLaunchKernelGGL(k_sighash_digests, dim3((njobs + 63) / 64), dim3(64), 0, st, arena, txs, in_off, out_off, jobs,
                     njobs, digests);
  return hipGetLastError();
}

hipError_t launch_sighash_items(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const uint32_t* in_off,
                                const uint32_t* out_off, const uint8_t* digests, const uint8_t* scripts,
                                const ShDevItem* items, int n, uint8_t* hashes) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_sighash_items, dim3((n + 63) / 64), dim3(64), 0, st, arena, txs, in_off, out_off, digests,
                     scripts, items, n, hashes);
  return hipGetLastError();
}

}  // namespace zg

extern "C" int zg_tx_layout(const uint8_t* tx, size_t len, uint64_t* out) {
  if (!tx || !out || len > ((size_t)1 << 31)) return ZG_E_INVAL;
  zg::TxLayout L;
  std::vector<uint32_t> in_off, out_off;
  const uint32_t st = zg::tx_parse(tx, len, L, in_off, out_off);
  for (int i = 0; i < 8; i++) out[i] = 0;
  if (st != zg::ZG_TXP_MALFORMED) {
    out[0] = L.header, out[1] = L.n_in, out[2] = L.n_out, out[3] = L.n_js, out[4] = L.n_spend, out[5] = L.n_sout;
    out[6] = L.sigver, out[7] = L.consumed;
  }
  return (int)st;
}
