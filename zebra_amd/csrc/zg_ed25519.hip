// zg_ed25519.hip -- the Ed25519 kernels (zg_ed25519.h): lane per signature. Their own translation
// unit, everything inlined into the two kernels (no call frames, so no private segment).
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_ed25519.h"

namespace zg {

// comb table: lane per (window w, digit d) -> d * 2^(8 w) * B as (y + x, y - x, 2 d x y)
__global__ void __launch_bounds__(64) k_ed_comb(uint32_t* table) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ZG_ED_COMB_POINTS) return;
  ed_comb_entry(t, table + (size_t)t * ZG_ED_COMB_WORDS);
}

// PublicKey::from_bytes + Signature::from_bytes + verify -> ZG_ED_*
__global__ void __launch_bounds__(64) k_ed25519(const uint8_t* pubkey, const uint8_t* sig, const uint8_t* msg, int n,
                                                const uint32_t* comb, uint8_t* status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  status[i] = ed25519_verify_one(pubkey + (size_t)32 * i, sig + (size_t)64 * i, msg + (size_t)32 * i, comb);
}

hipError_t launch_ed_comb(hipStream_t st, uint32_t* table) {
  hipLaunchKernelGGL(k_ed_comb, dim3((ZG_ED_COMB_POINTS + 63) / 64), dim3(64), 0, st, table);
  return hipGetLastError();
}
hipError_t launch_ed25519(hipStream_t st, const uint8_t* pubkey, const uint8_t* sig, const uint8_t* msg, int n,
                          const uint32_t* comb, uint8_t* status) {
  hipLaunchKernelGGL(k_ed25519, dim3((n + 63) / 64), dim3(64), 0, st, pubkey, sig, msg, n, comb, status);
  return hipGetLastError();
}

}  // namespace zg
