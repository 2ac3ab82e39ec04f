// zg_script.hip -- the kernel of zg_inputs.h and zg_script_class. One launch, lane
// per template input: HASH160 of the key push against the script's 20 bytes, the BIP66 encoding check, and
// the key and the DER signature laid out for k_ecdsa (zg_ecdsa.hip), which runs on them after the two
// signature-hash kernels (zg_sighash.hip). The host validated every offset a lane follows (zg_script.h).
#include <hip/hip_runtime.h>

#include "../../include/zg.h"
#include "zg_inputs.h"

namespace zg {

// sigs: the buffer k_ecdsa reads; item i's DER signature starts at items[i].der_off of it
__global__ void __launch_bounds__(64)
k_script_items(const uint8_t* __restrict__ arena, const uint8_t* __restrict__ prev, const ScDevItem* __restrict__ items,
               int n, uint32_t flags, uint8_t* __restrict__ pubkeys, uint8_t* __restrict__ pubkey_len,
               uint8_t* __restrict__ sigs, uint8_t* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ScDevItem d = items[i];
  status[i] = (uint8_t)script_item(arena, prev, d, flags, pubkeys + (size_t)SC_PUBKEY_STRIDE * i, pubkey_len + i,
                                   sigs + d.der_off);
}

hipError_t launch_script_items(hipStream_t st, const uint8_t* arena, const uint8_t* prev, const ScDevItem* items, int n,
                               uint32_t flags, uint8_t* pubkeys, uint8_t* pubkey_len, uint8_t* sigs, uint8_t* status) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_script_items, dim3((n + 63) / 64), dim3(64), 0, st, arena, prev, items, n, flags, pubkeys,
                     pubkey_len, sigs, status);
  return hipGetLastError();
}

}  // namespace zg

extern "C" int zg_script_class(const uint8_t* script_sig, size_t sig_len, const uint8_t* script_pubkey, size_t pk_len,
                               uint64_t out[5]) {
  if (!out || (sig_len && !script_sig) || (pk_len && !script_pubkey)) return ZG_E_INVAL;
  const zg::ScriptClass c = zg::script_class(script_sig, sig_len, script_pubkey, pk_len);
  out[0] = c.cls, out[1] = c.sig_off, out[2] = c.sig_len, out[3] = c.key_off, out[4] = c.key_len;
  return ZG_OK;
}
