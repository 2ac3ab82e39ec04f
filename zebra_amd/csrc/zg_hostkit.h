// zg_hostkit.h -- host plumbing that needs HIP and include/zg.h alone: the HIP call check, the owners of
// device memory, the fan-out over host threads, the offset check, and the host interface of zg_merkle.hip
// and zg_pghr13.hip. Host code only, and no kernel. Those two units include this header (below their
// kernels) and not zg_host.h: a __constant__ table of a header comes out in the device object of every
// unit that includes it, and zg_host.h's Groth16 and BLAKE2b headers hold some.
#pragma once
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zg.h"

// ------------------------------------------------------------------ the HIP call check
// HIPCHK_TO(sink, expr): a failing call leaves "<expr>: <hipGetErrorString>" in *sink and
// returns ZG_E_HIP from the calling function. HIPCHK(expr) is that with the context's message
// (the calling function has a zg_ctx* ctx).
namespace zg {
inline bool hip_failed(hipError_t e, const char* expr, std::string* sink) {
  if (e == hipSuccess) return false;
  *sink = std::string(expr) + ": " + hipGetErrorString(e);
  return true;
}
}  // namespace zg
#define HIPCHK_TO(sink, expr)                                     \
  do {                                                            \
    if (zg::hip_failed((expr), #expr, (sink))) return ZG_E_HIP;   \
  } while (0)
#define HIPCHK(expr)                                              \
  do {                                                            \
    if (zg::hip_failed((expr), #expr, &ctx->err)) return ZG_E_HIP; \
  } while (0)

namespace zg {

// ------------------------------------------------------------------ device memory
// Device buffers with one owner, freed when it goes: the buffers of one call (a local, so
// every return path frees them) or those of a context (zg_ctx::own).
struct DevScratch {
  std::vector<void*> p;
  DevScratch() = default;
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() {
    for (void* q : p) hipFree(q);
  }
  template <class T>
  hipError_t alloc(T** x, size_t bytes) {
    hipError_t e = hipMalloc((void**)x, bytes ? bytes : 1);
    if (e == hipSuccess) p.push_back(*x);
    return e;
  }
  // x leaves this owner: whoever takes it frees it
  template <class T>
  T* release(T* x) {
    p.erase(std::remove(p.begin(), p.end(), (void*)x), p.end());
    return x;
  }
  // alloc, then the host's bytes into it on st (no copy of nothing)
  template <class T>
  hipError_t up(T** x, const void* host, size_t bytes, hipStream_t st) {
    const hipError_t e = alloc(x, bytes);
    return e != hipSuccess || !bytes ? e : hipMemcpyAsync(*x, host, bytes, hipMemcpyHostToDevice, st);
  }
};

// The bump carve of an arena: parts in call order, each spanning its size rounded up to
// `align`, so with a base aligned to `align` every part starts aligned; a part of no bytes
// is a null pointer. span() is the same arithmetic for sizing the arena before the carve.
struct Carve {
  char* base = nullptr;
  size_t used = 0;
  static size_t span(size_t bytes, size_t align) { return (bytes + align - 1) / align * align; }
  template <class T>
  T* carve(size_t count, size_t align) {
    const size_t bytes = sizeof(T) * count;
    T* const part = bytes ? (T*)(base + used) : nullptr;
    used += span(bytes, align);
    return part;
  }
};

// Grow-only device memory of a context that one entry's calls reuse (allocating per call cost
// more wall time than most kernels): reserve() what the call needs, then carve() it.
struct DevArena : Carve {
  size_t cap = 0;
  DevArena() = default;
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() {
    if (base) hipFree(base);
  }
  // an arena that is too small is replaced, once the work st still has on it has drained
  hipError_t reserve(size_t need, hipStream_t st) {
    used = 0;
    if (cap >= need) return hipSuccess;
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    if (base) hipFree(base);
    base = nullptr;
    cap = 0;
    e = hipMalloc((void**)&base, need);
    if (e == hipSuccess) cap = need;
    return e;
  }
};

// ------------------------------------------------------------------ host threads
// the threads for `limit` pieces of host work: at most 16, the machine's, one per piece
inline size_t host_nt(size_t limit) {
  return std::min<size_t>({16, std::max(1u, std::thread::hardware_concurrency()), limit});
}
// fn(t, nt) for t in [0, nt): t = 0 on the caller, the others on threads of their own, joined
// before the return. How the work divides over t is fn's business.
template <class Fn>
void host_threads(size_t nt, Fn fn) {
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back([&fn, t, nt] { fn(t, nt); });
  if (nt) fn((size_t)0, nt);
  for (auto& t : th) t.join();
}

// ------------------------------------------------------------------ arguments, randomness, events
// off[0 .. n] never decreases and, with max_span set, off[n] - off[0] <= max_span: the buffer a
// call copies to the device and the lanes index by 32-bit differences
template <class T>
bool offsets_ok(const T* off, size_t n, uint64_t max_span) {
  static_assert(std::is_same<T, uint32_t>::value || std::is_same<T, uint64_t>::value, "offsets are u32 or u64");
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return !(n && max_span && (uint64_t)(off[n] - off[0]) > max_span);
}

inline bool os_random(void* buf, size_t len) {
  uint8_t* p = (uint8_t*)buf;
  size_t off = 0;
  while (off < len) {
    ssize_t got = getrandom(p + off, len - off, 0);
    if (got < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    off += (size_t)got;
  }
  return true;
}

// Wait for an event by polling (hipEventQuery + a short sleep) instead of hipEventSynchronize /
// hipStreamSynchronize: the host loop of batches in flight calls into the runtime from two threads
// (batch launches / harvests on the main one, the verdicts' final exponentiations on a worker), and
// a blocking synchronize on one thread held up the other's calls until the GPU work it waited for
// had finished (8k shards: every relaunch came ~1 ms after the verdict's final exponentiation).
inline hipError_t wait_event(hipEvent_t e) {
  for (;;) {
    const hipError_t r = hipEventQuery(e);
    if (r != hipErrorNotReady) return r;
    std::this_thread::sleep_for(std::chrono::microseconds(10));
  }
}

// ------------------------------------------------------------------ the other host units
// zg_merkle.hip
struct MerkleDev;
MerkleDev* merkle_dev_new();
void merkle_dev_free(MerkleDev* m);
int merkle_combine(MerkleDev* m, hipStream_t st, int kind, size_t n, const uint8_t* l, const uint8_t* r,
                   const uint8_t* depth, uint8_t* out, std::string* err);
int merkle_empty_roots(MerkleDev* m, hipStream_t st, int kind, size_t levels, uint8_t* out, std::string* err);
size_t merkle_state_max_bytes(int height);
int merkle_tree_roots(MerkleDev* m, hipStream_t st, int kind, int height, const uint8_t* state, size_t state_len,
                      size_t n, const void* leaves, int leaves_on_device, size_t nmarks, const uint64_t* marks,
                      uint8_t* roots, uint8_t* state_out, size_t* state_out_len, float* kernel_ms,
                      DevArena& arena, std::string* err);
// zg_pghr13.hip
struct BnDev;
struct BnKey;
BnDev* bn_dev_new();
void bn_dev_free(BnDev* d);
int bn_load_vk_json(BnDev* d, hipStream_t st, const char* json, size_t len, const BnKey** out, std::string* err);
void bn_key_release(BnDev* d, const BnKey* k);
void bn_pghr13_shape(size_t n, int forced_b, int forced_k, int* B, int* K, int* halves, int* p7_side);
int bn_pghr13_verify(const BnKey* k, hipStream_t st, hipStream_t side, size_t n, int forced_b, int forced_k,
                     const uint8_t* proofs, const uint8_t* inputs, const uint8_t* ninputs, const uint8_t* rho,
                     uint8_t* status, float* kernel_ms, bool* batch_failed, DevArena& arena, std::string* err,
                     bool on_device = false);  // on_device: proofs, inputs, ninputs, status are device buffers
int bn_pairing(hipStream_t st, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, std::string* err);

}  // namespace zg
