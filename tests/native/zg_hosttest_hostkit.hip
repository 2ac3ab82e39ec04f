// zg_hosttest_hostkit.hip -- the helpers of zebra_amd/csrc/zg_host.h that need no device, in a stand-alone
// program (hipcc --offload-host-only, its own main; tests/test_hostkit.py builds it with the address and
// undefined-behaviour sanitizers, and the thread part a second time with the thread sanitizer). No HIP call.
//   zg_hosttest_hostkit offsets | threads | carve    self-checks; "<part> ok <checks>" and exit 0, or the
//                                                     failing check's line and exit 1
//   zg_hosttest_hostkit seeded                        "<tag> <digest bytes> <seed> <i> <hex>" per derivation,
//                                                     for the caller to compare with its own BLAKE2b
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../zebra_amd/csrc/zg_host.h"

using namespace zg;

static long g_checks = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    g_checks++;                                                      \
    if (!(cond)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      exit(1);                                                       \
    }                                                                \
  } while (0)

// ---------------------------------------------------------------- offsets_ok
template <class T>
static void offsets_width() {
  const uint64_t lim = 1ull << 31;
  // n = 0: nothing is read beyond off[0], whatever the limit
  const T one[1] = {7};
  CHECK(offsets_ok(one, 0, 0) && offsets_ok(one, 0, lim) && offsets_ok(one, 0, 1));
  // equal offsets (empty slices), at zero and at a nonzero first offset
  const T eq0[5] = {0, 0, 0, 0, 0}, eq9[5] = {9, 9, 9, 9, 9};
  CHECK(offsets_ok(eq0, 4, 0) && offsets_ok(eq0, 4, lim) && offsets_ok(eq9, 4, 0) && offsets_ok(eq9, 4, lim));
  // one decreasing pair: first, middle, last position (exact-size heap arrays: a read past n + 1 entries faults)
  for (size_t n : {1, 2, 5, 64})
    for (size_t bad = 0; bad < n; bad++) {
      if (bad != 0 && bad != n / 2 && bad != n - 1) continue;
      std::vector<T> off(n + 1);
      for (size_t i = 0; i <= n; i++) off[i] = (T)(100 + 10 * i);
      CHECK(offsets_ok(off.data(), n, 0) && offsets_ok(off.data(), n, lim));
      off[bad + 1] = (T)(off[bad] - 1);
      for (size_t i = bad + 2; i <= n; i++) off[i] = (T)(off[bad + 1] + 10 * (i - bad - 1));  // rising again after it
      CHECK(!offsets_ok(off.data(), n, 0) && !offsets_ok(off.data(), n, lim));
    }
  // the span limit is inclusive, counts from off[0], and 0 means none
  for (T first : {(T)0, (T)1, (T)12345}) {
    const T at[4] = {first, (T)(first + 5), (T)(first + 5), (T)(first + lim)};
    const T over[4] = {first, (T)(first + 5), (T)(first + 5), (T)(first + lim + 1)};
    CHECK(offsets_ok(at, 3, lim) && offsets_ok(at, 3, 0));
    CHECK(!offsets_ok(over, 3, lim) && offsets_ok(over, 3, 0) && offsets_ok(over, 3, lim + 1));
    CHECK(offsets_ok(over, 2, lim));  // the span is off[n] - off[0], not the array's
    const T single[2] = {first, (T)(first + lim + 1)};
    CHECK(!offsets_ok(single, 1, lim) && offsets_ok(single, 1, 0));
  }
  const T top[3] = {(T)0, (T)1, (T) ~(T)0};  // the widest span of the type
  CHECK(offsets_ok(top, 2, 0) && !offsets_ok(top, 2, lim) && offsets_ok(top, 2, (uint64_t) ~(T)0));
}

static int part_offsets() {
  offsets_width<uint32_t>();
  offsets_width<uint64_t>();
  printf("offsets ok %ld\n", g_checks);
  return 0;
}

// ---------------------------------------------------------------- host_threads
// the three partitionings of the tree (zg_calls.hip): strided (txid_host_rows), an atomic counter (the block
// layouts of zg_blocks_verify), contiguous ranges with nt from count / 64 + 1 (the JoinSplit rows of zg_prep_batch)
static void visit_all(size_t count, int how, size_t nt) {
  std::vector<int> hits(count + 1, 0);  // plain ints: two threads on one index is a race the thread sanitizer reports
  std::atomic<size_t> next{0}, calls{0}, off_caller{0};
  const std::thread::id caller = std::this_thread::get_id();
  host_threads(nt, [&](size_t t, size_t n) {
    calls++;
    if (std::this_thread::get_id() != caller) off_caller++;
    if (n != nt || t >= nt || (t == 0) != (std::this_thread::get_id() == caller)) abort();
    if (how == 0)
      for (size_t k = t; k < count; k += n) hits[k]++;
    else if (how == 1)
      for (size_t k; (k = next.fetch_add(1)) < count;) hits[k]++;
    else
      for (size_t k = count * t / n; k < count * (t + 1) / n; k++) hits[k]++;
  });
  CHECK(calls == nt);
  CHECK(off_caller == (nt ? nt - 1 : 0));  // nt = 1: fn ran once, on the caller, so no thread was made
  for (size_t k = 0; k < count; k++) CHECK(hits[k] == 1);
  CHECK(hits[count] == 0);
}

static int part_threads() {
  CHECK(host_nt(0) == 0 && host_nt(1) == 1 && host_nt(1000) <= 16 && host_nt(1000) >= 1);
  CHECK(host_nt(1000) == std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency())));
  for (size_t count : {0, 1, 15, 16, 17, 1000}) {
    visit_all(count, 0, host_nt(count));
    if (count) visit_all(count, 1, host_nt(count));  // (zg_blocks_verify returns before its fan-out at no blocks)
    visit_all(count, 2, host_nt(count / 64 + 1));
    // and at fixed thread counts, whatever this machine has: one (the caller alone), fewer, as many, more than items
    for (size_t nt : {1, 2, 3, 16, 17})
      for (int how = 0; how < 3; how++) visit_all(count, how, nt);
  }
  printf("threads ok %ld\n", g_checks);
  return 0;
}

// ---------------------------------------------------------------- the arena's carve
struct Got {
  size_t off, bytes;
  bool null;
};
template <class T>
static void take(Carve& c, size_t count, size_t align, std::vector<Got>& got, size_t* need) {
  *need += Carve::span(sizeof(T) * count, align);
  T* p = c.carve<T>(count, align);
  got.push_back(Got{p ? (size_t)((char*)p - c.base) : 0, sizeof(T) * count, p == nullptr});
}

static int part_carve() {
  CHECK(Carve::span(0, 256) == 0 && Carve::span(1, 256) == 256 && Carve::span(256, 256) == 256 &&
        Carve::span(257, 256) == 512 && Carve::span(77, 1) == 77 && Carve::span(0, 1) == 0);
  for (size_t align : {1, 8, 256}) {
    for (size_t n : {0, 1, 8, 65, 200}) {
      // the shapes of the three users: bytes, words and structs, zero-size parts first, between and last
      std::vector<Got> got;
      size_t need = 0;
      void* mem = nullptr;
      if (posix_memalign(&mem, 256, 1 << 20)) abort();
      Carve c;
      c.base = (char*)mem;
      take<uint8_t>(c, 0, align, got, &need);
      take<uint8_t>(c, 296 * n, align, got, &need);
      take<uint8_t>(c, n, align, got, &need);
      take<uint8_t>(c, 0, align, got, &need);  // bn_pghr13_verify's dni without n_inputs
      take<uint64_t>(c, n + 1, align, got, &need);
      struct S24 {
        uint32_t w[6];
      };
      take<S24>(c, 3 * n + 1, align, got, &need);
      take<uint32_t>(c, 8 * (size_t)(n / 2), align, got, &need);
      take<char>(c, 1, align, got, &need);
      take<char>(c, 0, align, got, &need);
      CHECK(c.used == need && need <= (1u << 20));  // the carve ends where the sizing pass said
      size_t end = 0;
      for (const Got& g : got) {
        CHECK(g.null == (g.bytes == 0));
        if (g.null) continue;
        CHECK(g.off % align == 0);
        CHECK(g.off >= end);  // parts are in order and disjoint
        end = g.off + g.bytes;
        memset(c.base + g.off, 0xA5, g.bytes);  // within the block (the address sanitizer checks)
      }
      CHECK(end <= need);
      if (align == 1) CHECK(end == need);  // byte-packed: no gaps at all (zg_prep_batch's layout)
      free(mem);
    }
  }
  // zg_prep_batch's layout: kinds | fields | rows | codes at fixed byte offsets
  {
    const size_t n = 77, F = 304;
    void* mem = malloc(n * (2 + F + 288) + 64);
    Carve c;
    c.base = (char*)mem;
    uint8_t* dk = c.carve<uint8_t>(n, 1);
    uint8_t* df = c.carve<uint8_t>(F * n, 1);
    uint8_t* din = c.carve<uint8_t>(288 * n, 1);
    uint8_t* dc = c.carve<uint8_t>(n, 1);
    CHECK((char*)dk == c.base && df == dk + n && din == df + F * n && dc == din + 288 * n);
    CHECK(c.used == n * (2 + F + 288));
    free(mem);
  }
  printf("carve ok %ld\n", g_checks);
  return 0;
}

// ---------------------------------------------------------------- seeded_bytes
static int part_seeded() {
  const struct {
    const char* tag;
    size_t len;
  } tags[] = {{"zg-batch-r", 16}, {"zg-rerand", 64}, {"zg-pghr13-rho", 64}, {"zg-pghr13-rho1", 64}};
  for (const auto& t : tags)
    for (uint64_t seed : {(uint64_t)0, (uint64_t)1, ~(uint64_t)0})
      for (uint64_t i : {(uint64_t)0, (uint64_t)1, ((uint64_t)1 << 32) + 5}) {
        std::vector<uint8_t> out(t.len);  // exactly the digest: a longer write faults
        seeded_bytes(t.tag, seed, i, out.data(), t.len);
        printf("%s %zu %llu %llu ", t.tag, t.len, (unsigned long long)seed, (unsigned long long)i);
        for (uint8_t b : out) printf("%02x", b);
        printf("\n");
      }
  return 0;
}

int main(int argc, char** argv) {
  const char* part = argc > 1 ? argv[1] : "";
  if (!strcmp(part, "offsets")) return part_offsets();
  if (!strcmp(part, "threads")) return part_threads();
  if (!strcmp(part, "carve")) return part_carve();
  if (!strcmp(part, "seeded")) return part_seeded();
  fprintf(stderr, "usage: %s offsets|threads|carve|seeded\n", argv[0]);
  return 2;
}
