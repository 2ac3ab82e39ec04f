// zg_hosttest_multisig.hip -- the matcher of zebra_amd/csrc/zg_script.h with the multisig classes and the routines
// of zg_multisig.h compiled for the CPU (hipcc --offload-host-only): what zg_inputs_verify and its multisig kernels
// run, with the per-input routine of zg_inputs.h, the signature hash (zg_sighash.h) and the ECDSA check (zg_ecdsa.h)
// behind them and the host side of zg_inputs_verify restated around them, item by item. Test harness only. Built
// two ways:
//   * a shared library (tests/multisig_hostlib.py): zgh_script_match and zgh_inputs_verify, zg_inputs_verify's
//     arguments without the context plus a thread count (tools/bench_multisig.py's host baseline);
//   * with -DZG_MS_MAIN a stand-alone program, meant to be built with -fsanitize=address,undefined: it reads
//     (script_sig, script_pubkey, flags, the eight expected words) lines, copies the scripts, every proper prefix of
//     the script_sig and every proper prefix of the script_pubkey into heap blocks of exactly their size and runs the
//     matcher over them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "../../zebra_amd/csrc/zg_multisig.h"
#ifndef ZG_MS_MAIN
#include "../../zebra_amd/csrc/zg_ecdsa.h"
#endif

using namespace zg;

extern "C" int zgh_script_match(const uint8_t* sig, size_t sig_len, const uint8_t* pk, size_t pk_len, uint32_t flags,
                                uint64_t* out) {
  const ScriptMatch c = script_match(sig, sig_len, pk, pk_len, flags);
  out[0] = c.cls, out[1] = c.m, out[2] = c.n, out[3] = c.red_off, out[4] = c.red_len, out[5] = c.pairs();
  out[6] = c.sigs_at, out[7] = 0;
  // every offset the matcher hands out lies inside the script it refers to
  if (c.cls >= SCRIPT_MULTISIG) {
    if ((size_t)c.red_off + c.red_len > sig_len) return 1;
    for (uint32_t s = 0; s < c.m; s++)
      if ((size_t)c.sig_off[s] + c.sig_len[s] > sig_len) return 1;
  }
  return 0;
}

#ifndef ZG_MS_MAIN
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
  struct Work {
    size_t i;
    ScriptMatch c;
    uint32_t so, poff, pl;  // the script_sig in the arena, the previous script in prev
  };
  std::vector<Work> work;
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
    const ScriptMatch c = script_match(tx + so, sl, prev + poff, pl, flags);
    if (c.cls == SCRIPT_HOST) continue;
    work.push_back(Work{i, c, d.base + so, poff, pl});
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
  auto sighash = [&](size_t i, const uint8_t* scripts, uint32_t off, uint32_t len, uint32_t hashtype, uint8_t* hash) {
    const ShDevItem d{item_tx[i], input_index[i], off, len, hashtype, (uint32_t)i, amount[i]};
    sighash_item(sh_item(arena, dtx.data(), in_off.data(), out_off.data(), dig.data(), scripts, d), hash);
  };
  run([&](size_t w) {
    const Work& W = work[w];
    const size_t i = W.i;
    const ScriptMatch& c = W.c;
    if (c.cls < SCRIPT_MULTISIG) {  // as zg_hosttest_script.hip
      ScDevItem r;
      r.cls = c.cls, r.sig_off = W.so + c.one.sig_off, r.sig_len = c.one.sig_len;
      r.key_off = c.cls == SCRIPT_P2PKH ? W.so + c.one.key_off : W.poff + c.one.key_off, r.key_len = c.one.key_len;
      r.h160_off = W.poff + 3, r.der_off = 0, r.pad = 0;
      uint8_t pubkey[SC_PUBKEY_STRIDE], klen, hash[32];
      std::vector<uint8_t> der(r.sig_len + 1);
      const uint32_t f = script_item(arena, prev, r, flags, pubkey, &klen, der.data());
      sighash(i, prev, W.poff, W.pl, r.sig_len ? (uint32_t)arena[r.sig_off + r.sig_len - 1] : 1u, hash);
      const uint8_t ec = ecdsa_verify_one(pubkey, klen, der.data(), r.sig_len ? r.sig_len - 1 : 0, hash, comb);
      status[i] = f & SC_F_EQUALVERIFY ? 1 : f & SC_F_SIGNATURE_DER ? 2 : ec ? 3 : 0;
      if (status[i] == 3) detail[i] = ec;
      if (!f && r.sig_len && (r.key_len == 33 || r.key_len == 65)) memcpy(hashes + 32 * i, hash, 32);
      return;
    }
    // a multisig item: its records as zg_inputs_verify builds them, the item's rows in buffers of its own
    const bool p2sh = c.cls == SCRIPT_P2SH_MULTISIG;
    const uint32_t per = c.n - c.m + 1, rows = c.pairs();
    const MsDevItem d{p2sh, c.m, c.n, p2sh ? W.so + c.red_off + 1 : W.poff + 1, W.so + c.red_off, c.red_len, W.poff + 2, 0};
    std::vector<MsDevSig> sg(c.m);
    std::vector<uint32_t> sig_at(c.m), sig_off(rows + 1, 0);
    std::vector<uint8_t> hash(32 * c.m), pubkeys((size_t)SC_PUBKEY_STRIDE * rows), klen(rows), msg(32 * rows), enc(c.m), ec(rows);
    uint32_t der_bytes = 0;
    for (uint32_t s = 0; s < c.m; s++) {
      const uint32_t o = c.sig_off[c.m - 1 - s], l = c.sig_len[c.m - 1 - s];
      sg[s] = MsDevSig{0, s, W.so + o, l, s * per, der_bytes};
      sig_at[s] = s;
      der_bytes += per * (l ? l - 1 : 0);
    }
    std::vector<uint8_t> ders(der_bytes + 1);
    const uint32_t hash_bad = ms_item_hash(arena, prev, d);
    for (uint32_t s = 0; s < c.m; s++) {
      const uint32_t ht = sg[s].sig_len ? (uint32_t)arena[sg[s].sig_off + sg[s].sig_len - 1] : 1u;
      if (p2sh)
        sighash(i, arena, d.red_off, d.red_len, ht, hash.data() + 32 * s);
      else
        sighash(i, prev, W.poff, W.pl, ht, hash.data() + 32 * s);
      enc[s] = (uint8_t)ms_sig_rows(arena, prev, d, sg[s], hash.data() + 32 * s, pubkeys.data(), klen.data(), ders.data(),
                                    sig_off.data(), msg.data());
    }
    for (uint32_t r = 0; r < rows; r++)
      ec[r] = ecdsa_verify_one(pubkeys.data() + (size_t)SC_PUBKEY_STRIDE * r, klen[r], ders.data() + sig_off[r],
                               sig_off[r + 1] - sig_off[r], msg.data() + 32 * r, comb);
    uint32_t dt, last;
    status[i] = (uint8_t)ms_fold(d, sg.data(), sig_at.data(), hash_bad, enc.data(), ec.data(), flags & 1u, &dt, &last);
    detail[i] = (uint8_t)dt;
    if (last != MS_NO_PAIR && sg[last / per].sig_len) memcpy(hashes + 32 * i, hash.data() + 32 * (last / per), 32);
  }, work.size());
  return 0;
}
#endif

#ifdef ZG_MS_MAIN
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

// lines: script_sig script_pubkey flags class m n redeem_off redeem_len pairs sigs_at zero
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char a[1 << 16], b[1 << 16];
  unsigned long long w[8];
  unsigned flags;
  int cases = 0, bad = 0;
  long prefixes = 0, prefix_templates = 0;
  while (fscanf(f, "%65535s %65535s %u %llu %llu %llu %llu %llu %llu %llu %llu", a, b, &flags, &w[0], &w[1], &w[2], &w[3],
                &w[4], &w[5], &w[6], &w[7]) == 11) {
    const std::vector<uint8_t> sig = unhex(a), pk = unhex(b);
    uint64_t out[8];
    uint8_t* ppk = exact(pk.data(), pk.size());
    for (size_t k = 0; k <= sig.size(); k++) {  // every proper prefix of the script_sig, then the script_sig itself
      uint8_t* p = exact(sig.data(), k);
      if (zgh_script_match(p, k, ppk, pk.size(), flags, out)) {
        printf("MISMATCH case %d: an offset outside the script\n", cases);
        bad++;
      }
      if (k < sig.size()) prefixes++, prefix_templates += out[0] != SCRIPT_HOST;
      free(p);
    }
    for (int j = 0; j < 8; j++)
      if (out[j] != w[j]) {
        printf("MISMATCH case %d: word %d is %llu (want %llu)\n", cases, j, (unsigned long long)out[j], w[j]);
        bad++;
      }
    free(ppk);
    uint8_t* psig = exact(sig.data(), sig.size());
    for (size_t k = 0; k < pk.size(); k++) {  // every proper prefix of the script_pubkey
      uint8_t* p = exact(pk.data(), k);
      uint64_t o2[8];
      if (zgh_script_match(psig, sig.size(), p, k, flags, o2)) {
        printf("MISMATCH case %d: an offset outside the script\n", cases);
        bad++;
      }
      prefixes++, prefix_templates += o2[0] != SCRIPT_HOST;
      free(p);
    }
    free(psig);
    cases++;
  }
  fclose(f);
  printf("cases %d mismatches %d prefixes %ld prefix_templates %ld\n", cases, bad, prefixes, prefix_templates);
  return bad ? 1 : 0;
}
#endif
