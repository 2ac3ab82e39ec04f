// TEST HARNESS ONLY -- the 9 x 29-bit digit field (zebra_amd/csrc/zg_fd9.h) over raw digits on the CPU,
// for both moduli the kernels use, so the CPU-only test tier can drive it at its digit bounds. Never
// linked into, or loaded by, the product library.
#include "../../zebra_amd/csrc/zg_ecdsa.h"
#include "../../zebra_amd/csrc/zg_ed25519.h"

using namespace zg;

template <class F>
static void fd9_op(int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  for (size_t i = 0; i < n; i++) {
    F x, y, z;
    for (int k = 0; k < 9; k++) x.d[k] = a[9 * i + k], y.d[k] = b[9 * i + k];
    z = op == 0 ? fd_mul(x, y) : op == 1 ? fd_sqr(x) : op == 2 ? fd_add(x, y) : fd_sub(x, y);
    for (int k = 0; k < 9; k++) r[9 * i + k] = z.d[k];
  }
}

extern "C" {

// field: 0 = 2^255 - 19 (Fe), 1 = 2^256 - 2^32 - 977 (Sf); op: 0 mul, 1 sqr (b unused), 2 add, 3 sub;
// a, b, r: n elements of 9 raw digits
int zgt_fd9_op(int field, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  if (field < 0 || field > 1 || op < 0 || op > 3) return -1;
  if (field == 0)
    fd9_op<Fe>(op, n, a, b, r);
  else
    fd9_op<Sf>(op, n, a, b, r);
  return 0;
}

// out = canon(from_words(x)): n values of 8 LE words in and out
int zgt_fd9_canon(int field, size_t n, const uint32_t* x, uint32_t* out) {
  if (field < 0 || field > 1) return -1;
  for (size_t i = 0; i < n; i++) {
    if (field == 0)
      fd_canon(Fe::from_words(x + 8 * i), out + 8 * i);
    else
      fd_canon(Sf::from_words(x + 8 * i), out + 8 * i);
  }
  return 0;
}

}
