// zg_multisig.hip -- the kernels of zg_multisig.h and zg_script_match. Around the two
// signature-hash kernels and k_ecdsa, which zg_inputs_verify runs unchanged over the template rows and the pair
// rows together:
//   k_multisig_items  lane per multisig item: HASH160 of the redeem script against the script's 20 bytes
//   k_multisig_rows   lane per signature push, after the signature hashes: the BIP66 encoding check, and key, key
//                     length, DER bytes and message of each of its n - m + 1 candidate pairs laid out for k_ecdsa
//   k_multisig_fold   lane per multisig item, after k_ecdsa: OP_CHECKMULTISIG's walk over the flags and statuses
// The host validated every offset a lane follows (zg_script.h).
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_multisig.h"

namespace zg {

__global__ void __launch_bounds__(64)
k_multisig_items(const uint8_t* __restrict__ arena, const uint8_t* __restrict__ prev, const MsDevItem* __restrict__ items,
                 int n, uint8_t* __restrict__ hash_bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  hash_bad[i] = (uint8_t)ms_item_hash(arena, prev, items[i]);
}

// hashes: the hash of signature g at 32 g; the other pointers at the call's first pair row (sigs: the whole buffer)
__global__ void __launch_bounds__(64)
k_multisig_rows(const uint8_t* __restrict__ arena, const uint8_t* __restrict__ prev, const MsDevItem* __restrict__ items,
                const MsDevSig* __restrict__ sigrec, int n, const uint8_t* __restrict__ hashes,
                uint8_t* __restrict__ pubkeys, uint8_t* __restrict__ pubkey_len, uint8_t* __restrict__ sigs,
                uint32_t* __restrict__ sig_off, uint8_t* __restrict__ msg, uint8_t* __restrict__ enc_bad) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const MsDevSig r = sigrec[g];
  const MsDevItem d = items[r.item];
  enc_bad[g] = (uint8_t)ms_sig_rows(arena, prev, d, r, hashes + (size_t)32 * g, pubkeys, pubkey_len, sigs, sig_off, msg);
}

__global__ void __launch_bounds__(64)
k_multisig_fold(const MsDevItem* __restrict__ items, const MsDevSig* __restrict__ sigrec,
                const uint32_t* __restrict__ sig_at, int n, const uint8_t* __restrict__ hash_bad,
                const uint8_t* __restrict__ enc_bad, const uint8_t* __restrict__ ec, uint32_t flags,
                uint8_t* __restrict__ status, uint8_t* __restrict__ detail, uint32_t* __restrict__ last) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t dt, la;
  status[i] = (uint8_t)ms_fold(items[i], sigrec, sig_at, hash_bad[i], enc_bad, ec, flags & ZG_SCRIPT_VERIFY_DERSIG, &dt, &la);
  detail[i] = (uint8_t)dt;
  last[i] = la;
}

hipError_t launch_multisig_items(hipStream_t st, const uint8_t* arena, const uint8_t* prev, const MsDevItem* items, int n,
                                 uint8_t* hash_bad) {
  hipLaunchKernelGGL(k_multisig_items, dim3((n + 63) / 64), dim3(64), 0, st, arena, prev, items, n, hash_bad);
  return hipGetLastError();
}

hipError_t launch_multisig_rows(hipStream_t st, const uint8_t* arena, const uint8_t* prev, const MsDevItem* items,
                                const MsDevSig* sigrec, int n, const uint8_t* hashes, uint8_t* pubkeys,
                                uint8_t* pubkey_len, uint8_t* sigs, uint32_t* sig_off, uint8_t* msg, uint8_t* enc_bad) {
  hipLaunchKernelGGL(k_multisig_rows, dim3((n + 63) / 64), dim3(64), 0, st, arena, prev, items, sigrec, n, hashes,
                     pubkeys, pubkey_len, sigs, sig_off, msg, enc_bad);
  return hipGetLastError();
}

hipError_t launch_multisig_fold(hipStream_t st, const MsDevItem* items, const MsDevSig* sigrec, const uint32_t* sig_at,
                                int n, const uint8_t* hash_bad, const uint8_t* enc_bad, const uint8_t* ec, uint32_t flags,
                                uint8_t* status, uint8_t* detail, uint32_t* last) {
  hipLaunchKernelGGL(k_multisig_fold, dim3((n + 63) / 64), dim3(64), 0, st, items, sigrec, sig_at, n, hash_bad, enc_bad,
                     ec, flags, status, detail, last);
  return hipGetLastError();
}

}  // namespace zg

extern "C" int zg_script_match(const uint8_t* script_sig, size_t sig_len, const uint8_t* script_pubkey, size_t pk_len,
                               uint32_t flags, uint64_t out[8]) {
  if (!out || (sig_len && !script_sig) || (pk_len && !script_pubkey) ||
      (flags & ~(uint32_t)(ZG_SCRIPT_VERIFY_DERSIG | ZG_SCRIPT_TEMPLATE_MULTISIG)))
    return ZG_E_INVAL;
  const zg::ScriptMatch c = zg::script_match(script_sig, sig_len, script_pubkey, pk_len, flags);
  out[0] = c.cls, out[1] = c.m, out[2] = c.n, out[3] = c.red_off, out[4] = c.red_len, out[5] = c.pairs();
  out[6] = c.sigs_at, out[7] = 0;
  return ZG_OK;
}
