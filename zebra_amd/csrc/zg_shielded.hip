// zg_shielded.hip -- the kernels of zg_shielded.h. Around the kernels zg_shielded_verify
// runs unchanged over device-resident rows (the two signature-hash kernels, k_prep_sapling, k_sapling_bvk,
// k_redjubjub, k_ed25519 and the Groth16 batch pipeline):
//   k_shd_gather  lane per description: kind, proof, the Sapling field row and value commitment, a JoinSplit's
//                 nine public inputs (hSig, one BLAKE2b block, and the 254-bit packing)
//   k_shd_rows    lane per description, then per v4 transaction, after the hashes and the binding keys: the
//                 device-written input counts, the RedJubjub and Ed25519 rows
//   k_shd_descs   lane per description, after every check: its own first failing class
//   k_shd_fold    lane per v4 transaction: the reference's first error, its index and its class
// Byte gathers at any alignment and a short fold: no LDS, one lane per item. The host validated every offset a
// lane follows (tx_parse).
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_shielded.h"

namespace zg {

__global__ void __launch_bounds__(64)
k_shd_gather(const uint8_t* __restrict__ arena, const ShDevTx* __restrict__ txs, const ShdTx* __restrict__ stx,
             const ShdDesc* __restrict__ desc, int nd, uint8_t* __restrict__ kinds, uint8_t* __restrict__ fields,
             uint8_t* __restrict__ proofs, uint8_t* __restrict__ inputs, uint8_t* __restrict__ codes,
             uint8_t* __restrict__ cvs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nd) return;
  shd_gather(arena, txs, stx, desc[i], (size_t)i, kinds, fields, proofs, inputs, codes, cvs);
}

__global__ void __launch_bounds__(64)
k_shd_rows(const uint8_t* __restrict__ arena, const ShDevTx* __restrict__ txs, const ShdTx* __restrict__ stx, int ns,
           const ShdDesc* __restrict__ desc, int nd, const uint8_t* __restrict__ codes,
           const uint8_t* __restrict__ hashes, const uint8_t* __restrict__ bvk, uint8_t* __restrict__ ninputs,
           uint8_t* __restrict__ rj_vk, uint8_t* __restrict__ rj_sig, uint8_t* __restrict__ rj_msg,
           uint8_t* __restrict__ rj_gen, uint8_t* __restrict__ ed_pk, uint8_t* __restrict__ ed_sig,
           uint8_t* __restrict__ ed_msg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nd)
    shd_desc_rows(arena, txs, stx, desc[i], (size_t)i, codes, hashes, ninputs, rj_vk, rj_sig, rj_msg, rj_gen);
  else if (i - nd < ns)
    shd_tx_rows(arena, txs, stx[i - nd], (size_t)(i - nd), hashes, bvk, rj_vk, rj_sig, rj_msg, rj_gen, ed_pk, ed_sig,
                ed_msg);
}

__global__ void __launch_bounds__(64)
k_shd_descs(const ShdDesc* __restrict__ desc, int nd, const uint8_t* __restrict__ codes,
            const uint8_t* __restrict__ rj_ok, const uint8_t* __restrict__ proof_status,
            uint8_t* __restrict__ desc_status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nd) return;
  desc_status[i] = (uint8_t)shd_desc_status(desc[i], codes[i], rj_ok, proof_status[i]);
}

__global__ void __launch_bounds__(64)
k_shd_fold(const ShDevTx* __restrict__ txs, const ShdTx* __restrict__ stx, int ns,
           const uint8_t* __restrict__ desc_status, const uint8_t* __restrict__ ed, const uint8_t* __restrict__ rj_ok,
           const uint8_t* __restrict__ bvk_st, uint8_t* __restrict__ status, uint32_t* __restrict__ index,
           uint8_t* __restrict__ detail) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ns) return;
  const ShdTx S = stx[s];
  uint32_t ix, dt;
  status[s] = (uint8_t)shd_tx_fold(txs[S.tx].L, S, desc_status, ed, rj_ok, bvk_st[s], &ix, &dt);
  index[s] = ix;
  detail[s] = (uint8_t)dt;
}

hipError_t launch_shd_gather(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const ShdTx* stx,
                             const ShdDesc* desc, int nd, uint8_t* kinds, uint8_t* fields, uint8_t* proofs,
                             uint8_t* inputs, uint8_t* codes, uint8_t* cvs) {
  if (!nd) return hipSuccess;
  hipLaunchKernelGGL(k_shd_gather, dim3((nd + 63) / 64), dim3(64), 0, st, arena, txs, stx, desc, nd, kinds, fields,
                     proofs, inputs, codes, cvs);
  return hipGetLastError();
}

hipError_t launch_shd_rows(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const ShdTx* stx, int ns,
                           const ShdDesc* desc, int nd, const uint8_t* codes, const uint8_t* hashes,
                           const uint8_t* bvk, uint8_t* ninputs, uint8_t* rj_vk, uint8_t* rj_sig, uint8_t* rj_msg,
                           uint8_t* rj_gen, uint8_t* ed_pk, uint8_t* ed_sig, uint8_t* ed_msg) {
  hipLaunchKernelGGL(k_shd_rows, dim3((nd + ns + 63) / 64), dim3(64), 0, st, arena, txs, stx, ns, desc, nd, codes,
                     hashes, bvk, ninputs, rj_vk, rj_sig, rj_msg, rj_gen, ed_pk, ed_sig, ed_msg);
  return hipGetLastError();
}

hipError_t launch_shd_fold(hipStream_t st, const ShDevTx* txs, const ShdTx* stx, int ns, const ShdDesc* desc, int nd,
                           const uint8_t* codes, const uint8_t* rj_ok, const uint8_t* proof_status, const uint8_t* ed,
                           const uint8_t* bvk_st, uint8_t* desc_status, uint8_t* status, uint32_t* index,
                           uint8_t* detail) {
  if (nd) {
    hipLaunchKernelGGL(k_shd_descs, dim3((nd + 63) / 64), dim3(64), 0, st, desc, nd, codes, rj_ok, proof_status,
                       desc_status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_shd_fold, dim3((ns + 63) / 64), dim3(64), 0, st, txs, stx, ns, desc_status, ed, rj_ok, bvk_st,
                     status, index, detail);
  return hipGetLastError();
}

}  // namespace zg
