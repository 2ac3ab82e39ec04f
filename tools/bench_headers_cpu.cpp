// bench_headers_cpu.cpp -- single-thread host baseline of tools/bench_headers.py: the Equihash (200, 9)
// check of n serialized headers the way the reference runs it (verification/src/equihash.rs:80-172):
// one BLAKE2b context over the 140 input bytes, cloned per index; rows of padded bytes (30 hash bytes +
// big-endian indices); per level has_collision, indices_before, distinct_indices (as written) and
// merge_rows. The block hash and the proof of work (25 SHA-256 compressions against 513 BLAKE2b ones
// per header) are not part of it. Built and run by the tool:
//     g++ -O2 -std=c++17 -o bench_out/bench_headers_cpu tools/bench_headers_cpu.cpp
//     bench_out/bench_headers_cpu <file of n x 1487 bytes> <reps>   -> "<accepted> <seconds per pass>"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zebra_amd/csrc/zg_blake2b.h"

static const int N = 200, K = 9, IDX_BYTES = 3, LEAVES = 512, HASH_LEN = 30, ROW = 2 * IDX_BYTES + 4 * LEAVES;

static bool indices_before(const uint8_t* a, const uint8_t* b, int len, int ilen) {
  const int c = memcmp(a + len, b + len, ilen);
  return c < 0;
}

static bool verify(const uint8_t* hdr) {
  static const uint8_t person[16] = {'Z', 'c', 'a', 's', 'h', 'P', 'o', 'W', 200, 0, 0, 0, 9, 0, 0, 0};
  zg::Blake2b base(50, person);
  base.update(hdr, 140);
  const uint8_t* sol = hdr + 143;
  std::vector<uint8_t> r1(LEAVES * ROW), r2(LEAVES * ROW / 2);
  uint8_t* cur = r1.data();
  uint8_t* nxt = r2.data();
  uint32_t acc = 0;
  int bits = 0, leaf = 0;
  for (int i = 0; i < 1344; i++) {  // expand_array over 21-bit indices
    acc = (acc << 8) | sol[i];
    bits += 8;
    if (bits >= 21) {
      bits -= 21;
      const uint32_t index = (acc >> bits) & 0x1fffff;
      zg::Blake2b c = base;
      const uint32_t g = index / 2;
      const uint8_t le[4] = {(uint8_t)g, (uint8_t)(g >> 8), (uint8_t)(g >> 16), (uint8_t)(g >> 24)};
      c.update(le, 4);
      uint8_t h[50];
      c.final(h);
      const uint8_t* sub = h + (index % 2) * 25;
      uint8_t* row = cur + (size_t)leaf * ROW;
      for (int k = 0; k < 5; k++) {  // two 20-bit chunks per 5 bytes, each padded to 3 bytes
        const uint8_t* s = sub + 5 * k;
        row[6 * k + 0] = s[0] >> 4;
        row[6 * k + 1] = (uint8_t)((s[0] << 4) | (s[1] >> 4));
        row[6 * k + 2] = (uint8_t)((s[1] << 4) | (s[2] >> 4));
        row[6 * k + 3] = s[2] & 0x0f;
        row[6 * k + 4] = s[3];
        row[6 * k + 5] = s[4];
      }
      row[HASH_LEN + 0] = (uint8_t)(index >> 24), row[HASH_LEN + 1] = (uint8_t)(index >> 16);
      row[HASH_LEN + 2] = (uint8_t)(index >> 8), row[HASH_LEN + 3] = (uint8_t)index;
      leaf++;
    }
  }
  int hash_len = HASH_LEN, ilen = 4, count = LEAVES;
  while (count > 1) {
    for (int p = 0; p < count / 2; p++) {
      const uint8_t* a = cur + (size_t)(2 * p) * ROW;
      const uint8_t* b = a + ROW;
      if (memcmp(a, b, IDX_BYTES)) return false;
      if (indices_before(b, a, hash_len, ilen)) return false;
      for (int j = 0; j < ilen; j += 4)  // distinct_indices as written: only the left row's first index
        if (!memcmp(a + hash_len, b + hash_len + j, 4)) return false;
      uint8_t* m = nxt + (size_t)p * ROW;
      for (int i = IDX_BYTES; i < hash_len; i++) m[i - IDX_BYTES] = a[i] ^ b[i];
      const bool ab = indices_before(a, b, hash_len, ilen);
      memcpy(m + hash_len - IDX_BYTES, (ab ? a : b) + hash_len, ilen);
      memcpy(m + hash_len - IDX_BYTES + ilen, (ab ? b : a) + hash_len, ilen);
    }
    std::swap(cur, nxt);
    hash_len -= IDX_BYTES;
    ilen *= 2;
    count /= 2;
  }
  for (int i = 0; i < hash_len; i++)
    if (cur[i]) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> data;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + k);
  fclose(f);
  const size_t n = data.size() / 1487;
  const int reps = atoi(argv[2]);
  size_t ok = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < reps; r++) {
    ok = 0;
    for (size_t i = 0; i < n; i++) ok += verify(data.data() + 1487 * i);
  }
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / reps;
  printf("%zu %.9f\n", ok, dt);
  return 0;
}
