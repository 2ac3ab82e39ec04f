// zg_ecdsa.hip -- the secp256k1 ECDSA kernels (zg_ecdsa.h): lane per signature. Their own translation
// unit, everything inlined into the two kernels (no call frames, so no private segment).
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_ecdsa.h"

namespace zg {

// comb table: lane per (window w, digit d) -> d * 2^(8 w) * G as affine (x, y)
__global__ void __launch_bounds__(64) k_ec_comb(uint32_t* table) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ZG_EC_COMB_POINTS) return;
  ec_comb_entry(t, table + (size_t)t * ZG_EC_COMB_WORDS);
}

// Public::from_slice + Signature::from_der_lax + verify -> ZG_ECDSA_*. sigs starts at the byte
// sig_off[0] of the caller's buffer; item i is the bytes [sig_off[i], sig_off[i+1]) of it
__global__ void __launch_bounds__(64) k_ecdsa(const uint8_t* pubkeys, const uint8_t* pubkey_len, const uint8_t* sigs,
                                              const uint32_t* sig_off, const uint8_t* msg, int n,
                                              const uint32_t* comb, uint8_t* status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t lo = sig_off[i], hi = sig_off[i + 1];
  status[i] = ecdsa_verify_one(pubkeys + (size_t)ZG_ECDSA_PUBKEY_STRIDE * i, pubkey_len[i], sigs + (lo - sig_off[0]),
                               hi - lo, msg + (size_t)32 * i, comb);
}

hipError_t launch_ec_comb(hipStream_t st, uint32_t* table) {
  hipLaunchKernelGGL(k_ec_comb, dim3((ZG_EC_COMB_POINTS + 63) / 64), dim3(64), 0, st, table);
  return hipGetLastError();
}
hipError_t launch_ecdsa(hipStream_t st, const uint8_t* pubkeys, const uint8_t* pubkey_len, const uint8_t* sigs,
                        const uint32_t* sig_off, const uint8_t* msg, int n, const uint32_t* comb, uint8_t* status) {
  hipLaunchKernelGGL(k_ecdsa, dim3((n + 63) / 64), dim3(64), 0, st, pubkeys, pubkey_len, sigs, sig_off, msg, n, comb,
                     status);
  return hipGetLastError();
}

}  // namespace zg
