// zg_hosttest_sighash.hip -- the signature hash of zebra_amd/csrc/zg_sighash.h and the parser of zg_txparse.h
// compiled for the CPU (hipcc --offload-host-only): the routines the kernels run, with the host side of
// zg_sighash (statuses, which digests an item reads) restated around them. Test harness only. Built two ways:
//   * a shared library (tests/sighash_hostlib.py): zgh_sighash, zg_sighash's arguments without the context plus a
//     thread count (tools/bench_sighash.py's host baseline);
//   * with -DZG_SH_MAIN a stand-alone program, meant to be built with -fsanitize=address,undefined: it reads
//     cases from a text file, copies every transaction, every proper prefix of it and every script into heap
//     blocks of exactly their size, and runs the parser and the hasher over them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "../../zebra_amd/csrc/zg_sighash.h"

using namespace zg;

extern "C" int zgh_tx_layout(const uint8_t* tx, size_t len, uint64_t* out) {
  TxLayout L;
  std::vector<uint32_t> in_off, out_off;
  const uint32_t st = tx_parse(tx, len, L, in_off, out_off);
  for (int i = 0; i < 8; i++) out[i] = 0;
  if (st != ZG_TXP_MALFORMED) {
    out[0] = L.header, out[1] = L.n_in, out[2] = L.n_out, out[3] = L.n_js, out[4] = L.n_spend, out[5] = L.n_sout;
    out[6] = L.sigver, out[7] = L.consumed;
  }
  return (int)st;
}

extern "C" int zgh_sighash(size_t ntx, const uint8_t* txs, const uint64_t* tx_off, const uint32_t* tx_branch_id,
                           size_t n, const uint32_t* item_tx, const uint32_t* input_index, const uint8_t* scripts,
                           const uint32_t* script_off, const uint64_t* amount, const uint32_t* hashtype,
                           uint8_t* tx_status, uint8_t* hashes, uint8_t* status, int threads) {
  std::vector<ShDevTx> dtx(ntx ? ntx : 1);
  std::vector<uint32_t> in_off, out_off;
  for (size_t t = 0; t < ntx; t++) {
    tx_status[t] = (uint8_t)tx_parse(txs + tx_off[t], (size_t)(tx_off[t + 1] - tx_off[t]), dtx[t].L, in_off, out_off);
    dtx[t].base = (uint32_t)(tx_off[t] - tx_off[0]);
    dtx[t].branch_id = tx_branch_id[t];
    dtx[t].dig = (uint32_t)t;
  }
  const uint8_t* arena = ntx ? txs + tx_off[0] : txs;
  std::vector<ShDevItem> items;
  std::vector<uint8_t> need(ntx ? ntx : 1, 0);
  for (size_t i = 0; i < n; i++) {
    const TxLayout& L = dtx[item_tx[i]].L;
    const uint8_t ts = tx_status[item_tx[i]];
    memset(hashes + 32 * i, 0, 32);
    status[i] = ts ? ts : (L.sigver && input_index[i] != SIGHASH_NO_INPUT && input_index[i] >= L.n_in) ? 3 : 0;
    if (status[i]) continue;
    items.push_back(ShDevItem{item_tx[i], input_index[i], script_off[i] - script_off[0], script_off[i + 1] - script_off[i],
                              hashtype[i], (uint32_t)i, amount[i]});
    if (L.sigver) need[item_tx[i]] = 1;
  }
  if (threads < 1) threads = 1;
  // the digests of every overwintered transaction with an item (all six that its lists call for)
  std::vector<uint8_t> dig((size_t)32 * SH_DIGESTS * (ntx ? ntx : 1), 0);
  auto run = [&](auto&& body, size_t count) {
    std::vector<std::thread> th;
    for (int k = 0; k < threads; k++)
      th.emplace_back([&, k]() {
        for (size_t j = k; j < count; j += threads) body(j);
      });
    for (auto& t : th) t.join();
  };
  run([&](size_t j) {
    const size_t t = j / SH_DIGESTS;
    const int which = (int)(j % SH_DIGESTS);
    const TxLayout& L = dtx[t].L;
    if (!need[t]) return;
    if ((which == SH_JOINSPLITS && !L.n_js) || (which == SH_SPENDS && !L.n_spend) || (which == SH_SOUTPUTS && !L.n_sout))
      return;
    sighash_digest(arena + dtx[t].base, L, in_off.data() + L.in_idx, out_off.data() + L.out_idx, which,
                   dig.data() + 32 * (SH_DIGESTS * t + which));
  }, ntx * SH_DIGESTS);
  const uint8_t* sc = scripts + script_off[0];
  run([&](size_t k) {
    const ShItem it = sh_item(arena, dtx.data(), in_off.data(), out_off.data(), dig.data(), sc, items[k]);
    sighash_item(it, hashes + (size_t)32 * items[k].slot);
  }, items.size());
  return 0;
}

#ifdef ZG_SH_MAIN
static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> b;
  if (s == "-") return b;
  for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return b;
}

// a heap block of exactly the bytes: one byte past it is the sanitizer's
static uint8_t* exact(const uint8_t* p, size_t len) {
  uint8_t* q = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(q, p, len);
  return q;
}

// lines: tx script index(-1: none) amount hashtype branch expected_hash expected_status sweep(0/1)
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char a[1 << 20], b[1 << 16], h[80];
  long long index;
  unsigned long long amount;
  unsigned hashtype, branch;
  int want_status, sweep;
  int cases = 0, bad = 0;
  long prefixes = 0, prefix_parsed = 0;
  while (fscanf(f, "%1048575s %65535s %lld %llu %u %u %79s %d %d", a, b, &index, &amount, &hashtype, &branch, h,
                &want_status, &sweep) == 9) {
    const std::vector<uint8_t> tx = unhex(a), script = unhex(b), want = unhex(h);
    if (sweep)
      for (size_t k = 0; k < tx.size(); k++) {
        uint8_t* p = exact(tx.data(), k);
        uint64_t out[8];
        prefixes++;
        if (zgh_tx_layout(p, k, out) != (int)ZG_TXP_MALFORMED) prefix_parsed++;
        free(p);
      }
    uint8_t* ptx = exact(tx.data(), tx.size());
    uint8_t* psc = exact(script.data(), script.size());
    const uint64_t tx_off[2] = {0, tx.size()};
    const uint32_t script_off[2] = {0, (uint32_t)script.size()};
    const uint32_t item_tx = 0, idx = index < 0 ? SIGHASH_NO_INPUT : (uint32_t)index;
    const uint64_t amt = amount;
    uint8_t tx_status = 0, status = 0, hash[32];
    zgh_sighash(1, ptx, tx_off, &branch, 1, &item_tx, &idx, psc, script_off, &amt, &hashtype, &tx_status, hash, &status, 1);
    if (status != want_status || want.size() != 32 || memcmp(hash, want.data(), 32)) {
      printf("MISMATCH case %d: status %d (want %d)\n", cases, status, want_status);
      bad++;
    }
    free(ptx);
    free(psc);
    cases++;
  }
  fclose(f);
  printf("cases %d mismatches %d prefixes %ld prefixes_parsed %ld\n", cases, bad, prefixes, prefix_parsed);
  return bad ? 1 : 0;
}
#endif
