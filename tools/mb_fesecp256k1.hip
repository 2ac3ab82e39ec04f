// mb_fesecp256k1.hip -- ISA count of the two candidate forms of the field 2^256 - 2^32 - 977:
// 9 x 29-bit digits with the 2^261 = 2^37 + 31264 fold (zg_fd9.h fd_mul / fd_sqr over Sf of zg_ecdsa.h) against 8 x 32-bit
// saturated words with the 2^256 = 2^32 + 977 fold. Not run: compiled to assembly and counted.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 --offload-device-only -S -Izebra_amd/csrc -Iinclude
//         -o mb_fesecp256k1.s tools/mb_fesecp256k1.hip, then count the instructions of each kernel
// (profiles/f7_fesecp256k1_isa.txt).
#include <hip/hip_runtime.h>
#include "zg_ecdsa.h"
using namespace zg;
// 8 x 32 saturated: the 16-word schoolbook product (64 multiply-adds with carry chains), then twice
// lo + hi (2^32 + 977), then one conditional subtraction of p; canonical in and out
__device__ __forceinline__ void mul32(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  uint32_t t[16];
  sc_mp_mul<8, 8>(t, a, b);
  uint32_t f = 977u;
  zg_opaque(f);
  // u = lo + hi 977 + hi 2^32: 10 words
  uint32_t u[10];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    uint64_t s = c + (i < 8 ? t[i] : 0u) + (i >= 1 && i <= 8 ? t[7 + i] : 0u);
    uint64_t m = i < 8 ? (uint64_t)t[8 + i] * f : 0u;
    c = (s >> 32) + (m >> 32);
    s = (s & 0xffffffffu) + (m & 0xffffffffu);
    c += s >> 32;
    u[i] = (uint32_t)s;
  }
  // v = u[0..8) + (u[8] + u[9] 2^32) (2^32 + 977): 8 words and a carry bit
  uint32_t v[8];
  c = 0;
  uint32_t h0 = u[8], h1 = u[9];
  zg_opaque(h1);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t s = c + u[i] + (i == 1 ? h0 : i == 2 ? h1 : 0u);
    uint64_t m = i == 0 ? (uint64_t)h0 * f : i == 1 ? (uint64_t)h1 * f : 0u;
    c = (s >> 32) + (m >> 32);
    s = (s & 0xffffffffu) + (m & 0xffffffffu);
    c += s >> 32;
    v[i] = (uint32_t)s;
  }
  // the carry bit folds once more (it cannot carry again); then v >= p iff v + 2^32 + 977 carries
  uint32_t k = (uint32_t)c;
  uint64_t cc = (uint64_t)v[0] + 977u * k;
  v[0] = (uint32_t)cc;
  cc = (cc >> 32) + v[1] + k;
  v[1] = (uint32_t)cc;
#pragma unroll
  for (int i = 2; i < 8; i++) {
    cc = (cc >> 32) + v[i];
    v[i] = (uint32_t)cc;
  }
  uint32_t w[8];
  cc = (uint64_t)v[0] + 977u;
  w[0] = (uint32_t)cc;
  cc = (cc >> 32) + v[1] + 1u;
  w[1] = (uint32_t)cc;
#pragma unroll
  for (int i = 2; i < 8; i++) {
    cc = (cc >> 32) + v[i];
    w[i] = (uint32_t)cc;
  }
  const bool ge = (cc >> 32) != 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = ge ? w[i] : v[i];
}
__global__ void k_mul29(uint32_t* o, const uint32_t* a, const uint32_t* b) {
  Sf x, y; for (int i = 0; i < 9; i++) { x.d[i] = a[threadIdx.x * 9 + i]; y.d[i] = b[threadIdx.x * 9 + i]; }
  Sf r = fd_mul(x, y); for (int i = 0; i < 9; i++) o[threadIdx.x * 9 + i] = r.d[i];
}
__global__ void k_sqr29(uint32_t* o, const uint32_t* a) {
  Sf x; for (int i = 0; i < 9; i++) x.d[i] = a[threadIdx.x * 9 + i];
  Sf r = fd_sqr(x); for (int i = 0; i < 9; i++) o[threadIdx.x * 9 + i] = r.d[i];
}
__global__ void k_mul32(uint32_t* o, const uint32_t* a, const uint32_t* b) {
  uint32_t x[8], y[8], r[8]; for (int i = 0; i < 8; i++) { x[i] = a[threadIdx.x * 8 + i]; y[i] = b[threadIdx.x * 8 + i]; }
  mul32(r, x, y); for (int i = 0; i < 8; i++) o[threadIdx.x * 8 + i] = r[i];
}
