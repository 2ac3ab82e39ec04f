// zg_hosttest_blocks.hip -- the block parser, the transaction-id reader and the merkle node of
// zebra_amd/csrc/zg_blocks.h compiled for the CPU (hipcc --offload-host-only): the routines the kernels and
// zg_blocks_verify run. Test harness only. Built two ways:
//   * a shared library (tests/blocks_hostlib.py): zgh_block_layout, zgh_txids (with a thread count: the host
//     baseline of tools/bench_blocks.py), zgh_merkle_root (k_block_merkle's level loop on one thread);
//   * with -DZG_BLK_MAIN a stand-alone program, meant to be built with -fsanitize=address,undefined: it reads
//     cases from a text file, copies every block and every proper prefix of it into heap blocks of exactly
//     their size for the parser, and runs the reader over arenas allocated exactly as the entry allocates them
//     (16-byte aligned, txid_arena_bytes(bytes) long), every slice at every start alignment.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "../../zebra_amd/csrc/zg_blocks.h"

using namespace zg;

extern "C" int zgh_block_layout(const uint8_t* block, size_t len, uint64_t* out, uint64_t* tx_off, size_t tx_off_cap) {
  BlockLayout B;
  const uint32_t st = block_layout(block, len, B);
  for (int i = 0; i < 6; i++) out[i] = 0;
  if (st != ZG_TXP_MALFORMED) {
    out[0] = B.n_tx, out[1] = B.size, out[2] = B.sigops, out[3] = B.coinbase0, out[4] = B.extra_coinbase;
    out[5] = B.consumed;
    if (tx_off && tx_off_cap >= B.tx_off.size())
      for (size_t i = 0; i < B.tx_off.size(); i++) tx_off[i] = B.tx_off[i];
  }
  return (int)st;
}

// an arena by the rule of zg_blocks.h: aligned, exactly txid_arena_bytes(bytes) long
static uint8_t* arena_alloc(const uint8_t* p, size_t bytes) {
  void* q = nullptr;
  if (posix_memalign(&q, 16, txid_arena_bytes(bytes))) abort();
  if (bytes) memcpy(q, p, bytes);
  return (uint8_t*)q;
}

// zg_txids without the context: the caller's bytes are copied into an arena by the rule
extern "C" int zgh_txids(size_t n, const uint8_t* bytes, const uint64_t* off, uint8_t* hashes, int threads) {
  if (!n) return 0;
  const uint64_t base0 = off[0];
  uint8_t* arena = arena_alloc(bytes + base0, (size_t)(off[n] - base0));
  if (threads < 1) threads = 1;
  std::vector<std::thread> th;
  for (int k = 0; k < threads; k++)
    th.emplace_back([&, k]() {
      for (size_t i = k; i < n; i += threads) {
        uint32_t h[8];
        txid_hash(arena, (size_t)(off[i] - base0), (uint32_t)(off[i + 1] - off[i]), h);
        memcpy(hashes + 32 * i, h, 32);
      }
    });
  for (auto& t : th) t.join();
  free(arena);
  return 0;
}

// merkle_root over n >= 1 ids, level by level as k_block_merkle does
extern "C" int zgh_merkle_root(size_t n, const uint8_t* ids, uint8_t* root) {
  std::vector<uint32_t> cur(8 * n), nxt;
  memcpy(cur.data(), ids, 32 * n);
  while (n > 1) {
    const size_t m = (n + 1) / 2;
    nxt.assign(8 * m, 0);
    for (size_t i = 0; i < m; i++) merkle_node(&cur[16 * i], &cur[8 * (2 * i + 1 < n ? 2 * i + 1 : 2 * i)], &nxt[8 * i]);
    cur.swap(nxt);
    n = m;
  }
  memcpy(root, cur.data(), 32);
  return 0;
}

// a window on host threads, what zg_blocks_verify hashes: per block the parser, the ids and the root (blocks
// are dealt to the threads in turn; a block that is not ZG_TXP_OK or is empty gets a zero root and no rows).
// tx_count: nblk + 1 cumulative counts; txids: tx_count[nblk] rows, sized by the caller from a first call with
// txids NULL. The bytes are copied once into an arena by the rule. compressions (optional): SHA-256
// compressions of the ids alone
extern "C" int zgh_blocks_roots(size_t nblk, const uint8_t* blocks, const uint64_t* blk_off, uint8_t* roots,
                                uint64_t* tx_count, uint8_t* txids, uint64_t* compressions, int threads) {
  if (!nblk) return 0;
  if (threads < 1) threads = 1;
  const uint64_t base0 = blk_off[0];
  std::vector<BlockLayout> B(nblk);
  std::vector<uint32_t> st(nblk);
  auto run = [&](auto&& body) {
    std::vector<std::thread> th;
    for (int k = 0; k < threads; k++)
      th.emplace_back([&, k]() {
        for (size_t b = k; b < nblk; b += threads) body(b);
      });
    for (auto& t : th) t.join();
  };
  run([&](size_t b) { st[b] = block_layout(blocks + blk_off[b], (size_t)(blk_off[b + 1] - blk_off[b]), B[b]); });
  tx_count[0] = 0;
  uint64_t comp = 0;
  for (size_t b = 0; b < nblk; b++) {
    tx_count[b + 1] = tx_count[b] + (st[b] == ZG_TXP_OK ? B[b].n_tx : 0);
    if (st[b] == ZG_TXP_OK)
      for (size_t t = 0; t < B[b].n_tx; t++) comp += (B[b].tx_off[t + 1] - B[b].tx_off[t] + 72) / 64 + 1;
  }
  if (compressions) *compressions = comp;
  if (!txids) return 0;
  uint8_t* arena = arena_alloc(blocks + base0, (size_t)(blk_off[nblk] - base0));
  run([&](size_t b) {
    memset(roots + 32 * b, 0, 32);
    if (st[b] != ZG_TXP_OK || !B[b].n_tx) return;
    uint8_t* ids = txids + 32 * tx_count[b];
    for (size_t t = 0; t < B[b].n_tx; t++) {
      uint32_t h[8];
      txid_hash(arena, (size_t)(blk_off[b] - base0 + B[b].tx_off[t]), (uint32_t)(B[b].tx_off[t + 1] - B[b].tx_off[t]), h);
      memcpy(ids + 32 * t, h, 32);
    }
    zgh_merkle_root((size_t)B[b].n_tx, ids, roots + 32 * b);
  });
  free(arena);
  return 0;
}

#ifdef ZG_BLK_MAIN
static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> b;
  if (s == "-") return b;
  for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return b;
}

static uint8_t* exact(const uint8_t* p, size_t len) {
  uint8_t* q = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(q, p, len);
  return q;
}

// lines: B block want_status want_root(- none) sweep(0/1)   |   S bytes want_hash
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char kind[8], a[1 << 20], h[80];
  int cases = 0, bad = 0;
  long prefixes = 0, prefix_parsed = 0, slices = 0;
  while (fscanf(f, "%7s %1048575s", kind, a) == 2) {
    const std::vector<uint8_t> data = unhex(a);
    if (kind[0] == 'B') {
      int want_status, sweep;
      if (fscanf(f, "%d %79s %d", &want_status, h, &sweep) != 3) return 2;
      const std::vector<uint8_t> want = unhex(h);
      if (sweep)
        for (size_t k = 0; k < data.size(); k++) {
          uint8_t* p = exact(data.data(), k);
          uint64_t out[6];
          prefixes++;
          if (zgh_block_layout(p, k, out, nullptr, 0) != (int)ZG_TXP_MALFORMED) prefix_parsed++;
          free(p);
        }
      uint8_t* p = exact(data.data(), data.size());
      uint64_t out[6];
      int st = zgh_block_layout(p, data.size(), out, nullptr, 0);
      std::vector<uint64_t> off((size_t)out[0] + 1);
      st = zgh_block_layout(p, data.size(), out, off.data(), off.size());
      bool ok = st == want_status;
      if (ok && st == (int)ZG_TXP_OK && out[0]) {
        std::vector<uint8_t> ids(32 * (size_t)out[0]);
        uint8_t root[32];
        zgh_txids((size_t)out[0], p, off.data(), ids.data(), 1);
        zgh_merkle_root((size_t)out[0], ids.data(), root);
        ok = want.size() == 32 && !memcmp(root, want.data(), 32);
      }
      if (!ok) {
        printf("MISMATCH case %d: status %d (want %d)\n", cases, st, want_status);
        bad++;
      }
      free(p);
    } else {
      if (fscanf(f, "%79s", h) != 1) return 2;
      const std::vector<uint8_t> want = unhex(h);
      for (size_t lead = 0; lead < 16; lead++) {  // the slice ends on the arena's last byte
        std::vector<uint8_t> buf(lead, 0xa5);
        buf.insert(buf.end(), data.begin(), data.end());
        uint8_t* arena = arena_alloc(buf.data(), buf.size());
        uint32_t got[8];
        txid_hash(arena, lead, (uint32_t)data.size(), got);
        slices++;
        if (want.size() != 32 || memcmp(got, want.data(), 32)) {
          printf("MISMATCH case %d: slice of %zu bytes at alignment %zu\n", cases, data.size(), lead);
          bad++;
        }
        free(arena);
      }
    }
    cases++;
  }
  fclose(f);
  printf("cases %d mismatches %d prefixes %ld prefixes_parsed %ld slices %ld\n", cases, bad, prefixes, prefix_parsed,
         slices);
  return bad ? 1 : 0;
}
#endif
