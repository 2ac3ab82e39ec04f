// zg_shielded_phgr.hip -- the kernels of the PHGR routines of zg_shielded.h, which
// zg_shielded_verify_flags launches with ZG_SHIELDED_PHGR beside those of zg_shielded.hip, around the signature-hash
// kernels, k_ed25519 and the PGHR13 pipeline (zg_pghr13.hip) over device-resident rows:
//   k_shp_gather  lane per PHGR description: its 296-byte proof and its nine BN254 inputs (hSig, one BLAKE2b block,
//                 and the 253-bit packing)
//   k_shp_rows    lane per transaction before v4, after the hashes: its Ed25519 row
//   k_shp_fold    lane per transaction before v4, after every check: its descriptions' classes from their PGHR13
//                 statuses, and the reference's first error, its index and its class
// Byte gathers at any alignment and a short fold: no LDS, one lane per item. The host validated every offset a
// lane follows (tx_parse).
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_shielded.h"

namespace zg {

__global__ void __launch_bounds__(64)
k_shp_gather(const uint8_t* __restrict__ arena, const ShDevTx* __restrict__ txs, const ShpTx* __restrict__ ptx,
             const ShpDesc* __restrict__ desc, int nd, uint8_t* __restrict__ proofs, uint8_t* __restrict__ inputs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nd) return;
  shp_gather(arena, txs, ptx, desc[i], (size_t)i, proofs, inputs);
}

__global__ void __launch_bounds__(64)
k_shp_rows(const uint8_t* __restrict__ arena, const ShDevTx* __restrict__ txs, const ShpTx* __restrict__ ptx, int np,
           const uint8_t* __restrict__ hashes, uint8_t* __restrict__ ed_pk, uint8_t* __restrict__ ed_sig,
           uint8_t* __restrict__ ed_msg) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= np) return;
  shp_tx_rows(arena, txs, ptx[s], hashes, ed_pk, ed_sig, ed_msg);
}

__global__ void __launch_bounds__(64)
k_shp_fold(const ShDevTx* __restrict__ txs, const ShpTx* __restrict__ ptx, int np,
           const uint8_t* __restrict__ proof_status, const uint8_t* __restrict__ ed, uint8_t* __restrict__ desc_status,
           uint8_t* __restrict__ status, uint32_t* __restrict__ index, uint8_t* __restrict__ detail) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= np) return;
  const ShpTx S = ptx[s];
  uint32_t ix, dt;
  status[s] = (uint8_t)shp_tx_fold(txs[S.tx].L, S, proof_status, ed, desc_status, &ix, &dt);
  index[s] = ix;
  detail[s] = (uint8_t)dt;
}

hipError_t launch_shp_gather(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const ShpTx* ptx,
                             const ShpDesc* desc, int nd, uint8_t* proofs, uint8_t* inputs) {
  if (!nd) return hipSuccess;
  hipLaunchKernelGGL(k_shp_gather, dim3((nd + 63) / 64), dim3(64), 0, st, arena, txs, ptx, desc, nd, proofs, inputs);
  return hipGetLastError();
}

hipError_t launch_shp_rows(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const ShpTx* ptx, int np,
                           const uint8_t* hashes, uint8_t* ed_pk, uint8_t* ed_sig, uint8_t* ed_msg) {
  if (!np) return hipSuccess;
  hipLaunchKernelGGL(k_shp_rows, dim3((np + 63) / 64), dim3(64), 0, st, arena, txs, ptx, np, hashes, ed_pk, ed_sig,
                     ed_msg);
  return hipGetLastError();
}

hipError_t launch_shp_fold(hipStream_t st, const ShDevTx* txs, const ShpTx* ptx, int np, const uint8_t* proof_status,
                           const uint8_t* ed, uint8_t* desc_status, uint8_t* status, uint32_t* index, uint8_t* detail) {
  if (!np) return hipSuccess;
  hipLaunchKernelGGL(k_shp_fold, dim3((np + 63) / 64), dim3(64), 0, st, txs, ptx, np, proof_status, ed, desc_status,
                     status, index, detail);
  return hipGetLastError();
}

}  // namespace zg
