// zg_hosttest_script.hip -- the template matcher of zebra_amd/csrc/zg_script.h and the per-input routine of
// zg_inputs.h compiled for the CPU (hipcc --offload-host-only): the routines zg_inputs_verify and its kernel run,
// with the signature hash (zg_sighash.h) and the ECDSA check (zg_ecdsa.h) behind them and the host side of
// zg_inputs_verify (statuses, the fold) restated around them. Test harness only. Built two ways:
//   * a shared library (tests/script_hostlib.py): zgh_script_class and zgh_inputs_verify, zg_inputs_verify's
//     arguments without the context plus a thread count (tools/bench_inputs.py's host baseline);
//   * with -DZG_SC_MAIN a stand-alone program, meant to be built with -fsanitize=address,undefined: it reads
//     (script_sig, script_pubkey, expected class record) lines, copies both scripts and every proper prefix of the
//     script_sig into heap blocks of exactly their size, runs the matcher over them and the encoding check over
//     the signature push it finds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "../../zebra_amd/csrc/zg_inputs.h"
#ifndef ZG_SC_MAIN
#include "../../zebra_amd/csrc/zg_ecdsa.h"
#endif

using namespace zg;

extern "C" int zgh_script_class(const uint8_t* sig, size_t sig_len, const uint8_t* pk, size_t pk_len, uint64_t* out) {
  const ScriptClass c = script_class(sig, sig_len, pk, pk_len);
  out[0] = c.cls, out[1] = c.sig_off, out[2] = c.sig_len, out[3] = c.key_off, out[4] = c.key_len;
  return 0;
}

extern "C" int zgh_signature_encoding(const uint8_t* sig, size_t n) { return is_valid_signature_encoding(sig, (uint32_t)n); }

#ifndef ZG_SC_MAIN
extern "C" int zgh_inputs_verify(size_t ntx, const uint8_t* txs, const uint64_t* tx_off, const uint32_t* tx_branch_id,
                                 size_t n, const uint32_t* item_tx, const uint32_t* input_index,
                                 const uint8_t* prev_scripts, const uint32_t* prev_off, const uint64_t* amount,
                                 uint32_t flags, uint8_t* tx_status, uint8_t* status, uint8_t* detail, uint8_t* hashes,
                                 int threads) {
  static uint32_t* comb = nullptr;
  if (!comb) {
    comb = (uint32_t*)malloc(sizeof(uint32_t) * ZG_EC_COMB_WORDS * ZG_EC_COMB_POINTS);
    for (int i = 0; i < ZG_EC_COMB_POINTS; i++) ec_comb_entry(i, comb + (size_t)i * ZG_EC_COMB_WORDS);
  }
  std::vector<ShDevTx> dtx(ntx ? ntx : 1);
  std::vector<uint32_t> in_off, out_off;
  for (size_t t = 0; t < ntx; t++) {
    tx_status[t] = (uint8_t)tx_parse(txs + tx_off[t], (size_t)(tx_off[t + 1] - tx_off[t]), dtx[t].L, in_off, out_off);
    dtx[t].base = (uint32_t)(tx_off[t] - tx_off[0]);
    dtx[t].branch_id = tx_branch_id[t];
    dtx[t].dig = (uint32_t)t;
  }
  const uint8_t* arena = ntx ? txs + tx_off[0] : txs;
  const uint8_t* prev = n ? prev_scripts + prev_off[0] : prev_scripts;
  std::vector<ShDevItem> items;
  std::vector<ScDevItem> rec;
  std::vector<uint8_t> need(ntx ? ntx : 1, 0);
  for (size_t i = 0; i < n; i++) {
    const ShDevTx& d = dtx[item_tx[i]];
    const uint8_t ts = tx_status[item_tx[i]];
    detail[i] = 0;
    memset(hashes + 32 * i, 0, 32);
    status[i] = ts == ZG_TXP_MALFORMED ? 5 : ts == ZG_TXP_NONCANONICAL ? 6 : input_index[i] >= d.L.n_in ? 7 : 4;
    if (status[i] != 4) continue;
    const uint8_t* tx = arena + d.base;
    const uint32_t* io = in_off.data() + d.L.in_idx;
    const uint32_t o = io[input_index[i]] + 36, tag = tx[o];
    const uint32_t so = o + (tag < 0xfd ? 1 : tag == 0xfd ? 3 : tag == 0xfe ? 5 : 9), sl = io[input_index[i] + 1] - 4 - so;
    const uint32_t poff = prev_off[i] - prev_off[0], pl = prev_off[i + 1] - prev_off[i];
    const ScriptClass c = script_class(tx + so, sl, prev + poff, pl);
    if (c.cls == SCRIPT_HOST) continue;
    status[i] = 0;
    ScDevItem r;
    r.cls = c.cls, r.sig_off = d.base + so + c.sig_off, r.sig_len = c.sig_len;
    r.key_off = c.cls == SCRIPT_P2PKH ? d.base + so + c.key_off : poff + c.key_off, r.key_len = c.key_len;
    r.h160_off = poff + 3, r.der_off = 0, r.pad = 0;
    rec.push_back(r);
    items.push_back(ShDevItem{item_tx[i], input_index[i], poff, pl,
                              c.sig_len ? (uint32_t)tx[so + c.sig_off + c.sig_len - 1] : 1u, (uint32_t)i, amount[i]});
    if (d.L.sigver) need[item_tx[i]] = 1;
  }
  if (threads < 1) threads = 1;
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
  run([&](size_t k) {
    const size_t i = items[k].slot;
    uint8_t pubkey[SC_PUBKEY_STRIDE], klen, hash[32];
    std::vector<uint8_t> der(rec[k].sig_len + 1);
    const uint32_t f = script_item(arena, prev, rec[k], flags, pubkey, &klen, der.data());
    const ShItem it = sh_item(arena, dtx.data(), in_off.data(), out_off.data(), dig.data(), prev, items[k]);
    sighash_item(it, hash);
    const uint8_t ec = ecdsa_verify_one(pubkey, klen, der.data(), rec[k].sig_len ? rec[k].sig_len - 1 : 0, hash, comb);
    status[i] = f & SC_F_EQUALVERIFY ? 1 : f & SC_F_SIGNATURE_DER ? 2 : ec ? 3 : 0;
    if (status[i] == 3) detail[i] = ec;
    if (!f && rec[k].sig_len && (rec[k].key_len == 33 || rec[k].key_len == 65)) memcpy(hashes + 32 * i, hash, 32);
  }, items.size());
  return 0;
}
#endif

#ifdef ZG_SC_MAIN
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

// lines: script_sig script_pubkey class sig_off sig_len key_off key_len encoding_ok(of the signature push)
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char a[1 << 16], b[1 << 16];
  unsigned long long w[5];
  int enc;
  int cases = 0, bad = 0;
  long prefixes = 0, prefix_templates = 0;
  while (fscanf(f, "%65535s %65535s %llu %llu %llu %llu %llu %d", a, b, &w[0], &w[1], &w[2], &w[3], &w[4], &enc) == 8) {
    const std::vector<uint8_t> sig = unhex(a), pk = unhex(b);
    uint8_t* ppk = exact(pk.data(), pk.size());
    uint64_t out[5];
    for (size_t k = 0; k <= sig.size(); k++) {  // every proper prefix, then the script itself
      uint8_t* p = exact(sig.data(), k);
      zgh_script_class(p, k, ppk, pk.size(), out);
      if (out[0] != SCRIPT_HOST) {
        uint8_t* q = exact(p + out[1], (size_t)out[2]);  // the signature push alone
        const int e = zgh_signature_encoding(q, (size_t)out[2]);
        free(q);
        if (k == sig.size() && e != enc) {
          printf("MISMATCH case %d: encoding %d (want %d)\n", cases, e, enc);
          bad++;
        }
        if (out[1] + out[2] > k || (out[0] == SCRIPT_P2PKH ? out[3] + out[4] > k : out[3] + out[4] > pk.size())) {
          printf("MISMATCH case %d: an offset outside the script\n", cases);
          bad++;
        }
      }
      if (k < sig.size()) {
        prefixes++;
        if (out[0] != SCRIPT_HOST) prefix_templates++;
      }
      free(p);
    }
    if (out[0] != w[0] || out[1] != w[1] || out[2] != w[2] || out[3] != w[3] || out[4] != w[4]) {
      printf("MISMATCH case %d: class %llu (want %llu)\n", cases, (unsigned long long)out[0], w[0]);
      bad++;
    }
    free(ppk);
    cases++;
  }
  fclose(f);
  printf("cases %d mismatches %d prefixes %ld prefix_templates %ld\n", cases, bad, prefixes, prefix_templates);
  return bad ? 1 : 0;
}
#endif
