// zg_blake2b.h -- BLAKE2b (RFC 7693), host side, unkeyed, optional 16-byte personalization: the
// streaming form over the compression of zg_hash.h.
// Used for the Sprout hSig (personal "ZcashComputehSig", verification/src/sprout.rs:16-32),
// seeded-mode batch scalars and synthetic re-randomization scalars (the product's production
// mode draws r_i from the OS RNG).
#pragma once
#include <stdint.h>
#include <string.h>

#include "zg_hash.h"

namespace zg {

struct Blake2b {
  uint64_t h[8];
  uint64_t t;
  uint8_t buf[128];
  size_t n;
  size_t outlen;

  explicit Blake2b(size_t out, const uint8_t* personal = nullptr) : t(0), n(0), outlen(out) {
    blake2b_init(h, (uint32_t)out, personal ? blake2b_person(personal, 0) : 0, personal ? blake2b_person(personal, 1) : 0);
  }
  void compress(bool last) {
    uint64_t m[16];
    for (int i = 0; i < 16; i++) {
      uint64_t w = 0;
      for (int b = 7; b >= 0; b--) w = (w << 8) | buf[8 * i + b];
      m[i] = w;
    }
    blake2b_compress(h, m, t, last);
  }
  void update(const void* data, size_t len) {
    const uint8_t* p = (const uint8_t*)data;
    while (len) {
      if (n == 128) {
        t += 128;
        compress(false);
        n = 0;
      }
      size_t k = 128 - n < len ? 128 - n : len;
      memcpy(buf + n, p, k);
      n += k;
      p += k;
      len -= k;
    }
  }
  void final(uint8_t* out) {
    t += n;
    memset(buf + n, 0, 128 - n);
    compress(true);
    for (size_t i = 0; i < outlen; i++) out[i] = (uint8_t)(h[i / 8] >> (8 * (i % 8)));
  }
};

}  // namespace zg
