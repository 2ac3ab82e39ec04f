// mb_fe25519.hip -- ISA count of the two candidate digit forms of the field 2^255 - 19:
// 9 x 29-bit digits with the 2^261 = 1216 fold (zg_fd9.h fd_mul / fd_sqr over Fe of zg_ed25519.h) against 10 x 25.5-bit
// digits with 19 b pre-folded. Not run: compiled to assembly and counted.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 --offload-device-only -S -Izebra_amd/csrc -Iinclude
//         -o mb_fe25519.s tools/mb_fe25519.hip, then count the instructions of each kernel
// (profiles/f5_fe25519_isa.txt: product 156 VALU / 92 v_mad_u64_u32 against 155 / 101; square 125 / 56).
#include <hip/hip_runtime.h>
#include "zg_ed25519.h"
using namespace zg;
// 10 x 25.5-bit digits (widths 26,25,...), 19*b pre-folded, odd*odd doubled: 100 MACs
__device__ __forceinline__ void mul255(uint32_t* r, const uint32_t* f, const uint32_t* g) {
  uint32_t g19[10], f2[10];
#pragma unroll
  for (int i = 0; i < 10; i++) { g19[i] = 19u * g[i]; f2[i] = (i & 1) ? 2u * f[i] : f[i]; }
  uint64_t c[10];
#pragma unroll
  for (int k = 0; k < 10; k++) {
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      int j = k - i; bool wrap = j < 0; if (wrap) j += 10;
      const uint32_t a = ((i & 1) && (j & 1)) ? f2[i] : f[i];
      s = fd_mad(a, wrap ? g19[j] : g[j], s);
    }
    c[k] = s;
  }
#pragma unroll
  for (int k = 0; k < 9; k++) { const int w = (k & 1) ? 25 : 26; c[k + 1] += c[k] >> w; r[k] = (uint32_t)c[k] & ((1u << w) - 1); }
  uint64_t t = c[9] >> 25; r[9] = (uint32_t)c[9] & ((1u << 25) - 1);
  uint64_t c0 = r[0] + 19 * t; r[0] = (uint32_t)c0 & ((1u << 26) - 1); r[1] += (uint32_t)(c0 >> 26);
}
__global__ void k_mul29(uint32_t* o, const uint32_t* a, const uint32_t* b) {
  Fe x, y; for (int i = 0; i < 9; i++) { x.d[i] = a[threadIdx.x * 9 + i]; y.d[i] = b[threadIdx.x * 9 + i]; }
  Fe r = fd_mul(x, y); for (int i = 0; i < 9; i++) o[threadIdx.x * 9 + i] = r.d[i];
}
__global__ void k_sqr29(uint32_t* o, const uint32_t* a) {
  Fe x; for (int i = 0; i < 9; i++) x.d[i] = a[threadIdx.x * 9 + i];
  Fe r = fd_sqr(x); for (int i = 0; i < 9; i++) o[threadIdx.x * 9 + i] = r.d[i];
}
__global__ void k_mul255(uint32_t* o, const uint32_t* a, const uint32_t* b) {
  uint32_t x[10], y[10], r[10]; for (int i = 0; i < 10; i++) { x[i] = a[threadIdx.x * 10 + i]; y[i] = b[threadIdx.x * 10 + i]; }
  mul255(r, x, y); for (int i = 0; i < 10; i++) o[threadIdx.x * 10 + i] = r[i];
}
