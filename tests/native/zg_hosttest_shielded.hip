// zg_hosttest_shielded.hip -- the plan, gather, row and fold routines of zebra_amd/csrc/zg_shielded.h compiled for the
// CPU (hipcc --offload-host-only): what zg_shielded_verify and its kernels run, lane by lane, with the host side of the
// entry restated around them. The checks that other kernels make on the device (the signature hash, the binding key,
// RedJubjub, Ed25519, the Groth16 batch) are fed in by the caller, which computes them with the test oracle; the
// Sapling preparation is prep_spend / prep_output of zg_prep.h over the gathered field rows. Test harness only.
// Built two ways:
//   * a shared library (tests/shielded_hostlib.py): zgh_shielded_verify and zgh_prep_joinsplit;
//   * with -DZG_SHD_MAIN a stand-alone program, meant to be built with -fsanitize=address,undefined: it reads
//     (branch id, transaction) lines, copies each transaction and every proper prefix of it into a heap block of
//     exactly its size and runs the same routines over it with all-passing verdicts.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../zebra_amd/csrc/zg_shielded.h"

using namespace zg;

// per v4 transaction t (window order, 32 / 1 bytes each): hashes, bvk, bvk_st, bind_ok, ed; per description (window
// order): spend_ok (read for spends), proof. Rows out: rj 161 bytes each (vk, sig, msg, gen), the spends' in
// description order then the binding rows; ed 128 bytes each (pubkey, sig, msg). counts: descriptions, RedJubjub
// rows, Ed25519 rows, v4 transactions.
extern "C" int zgh_shielded_verify(size_t ntx, const uint8_t* txs, const uint64_t* tx_off, const uint32_t* tx_branch_id,
                                   const uint8_t* hashes, const uint8_t* bvk, const uint8_t* bvk_st,
                                   const uint8_t* bind_ok, const uint8_t* ed, const uint8_t* spend_ok,
                                   const uint8_t* proof, uint8_t* tx_status, uint8_t* status, uint64_t* index,
                                   uint8_t* detail, uint64_t* desc_off, uint8_t* desc_status, uint8_t* kinds,
                                   uint8_t* codes, uint8_t* ninputs, uint8_t* inputs, uint8_t* proofs, uint8_t* rj,
                                   uint8_t* edrows, uint64_t* counts) {
  std::vector<ShDevTx> dtx(ntx ? ntx : 1);
  std::vector<uint32_t> in_off, out_off;
  for (size_t t = 0; t < ntx; t++) {
    tx_status[t] = (uint8_t)tx_parse(txs + tx_off[t], (size_t)(tx_off[t + 1] - tx_off[t]), dtx[t].L, in_off, out_off);
    dtx[t].base = (uint32_t)(tx_off[t] - tx_off[0]);
    dtx[t].branch_id = tx_branch_id[t];
    dtx[t].dig = 0;
  }
  const uint8_t* arena = ntx ? txs + tx_off[0] : txs;
  ShdPlan Q;
  if (!shd_plan(dtx, ntx, arena, tx_status, status, Q)) return 1;
  const size_t ns = Q.stx.size(), nd = Q.desc.size();
  counts[0] = nd, counts[1] = Q.nrj, counts[2] = Q.ned, counts[3] = ns;
  desc_off[0] = 0;
  for (size_t t = 0, s = 0; t < ntx; t++) {
    index[t] = 0, detail[t] = 0;
    const bool here = s < ns && Q.stx[s].tx == t;
    desc_off[t + 1] = here ? (s + 1 < ns ? Q.stx[s + 1].desc0 : nd) : desc_off[t];
    s += here;
  }
  if (!ns) return 0;
  for (size_t s = 0; s < ns; s++) Q.stx[s].hash = (uint32_t)s;
  std::vector<uint8_t> fields((size_t)SHD_FIELD_BYTES * nd + 1), cvs(32 * Q.ncv() + 1), hs(32 * ns), bv(32 * ns), bst(ns),
      vk(32 * Q.nrj), sig(64 * Q.nrj), msg(64 * Q.nrj), gen(Q.nrj), ok(Q.nrj), epk(32 * Q.ned + 1), esig(64 * Q.ned + 1),
      emsg(32 * Q.ned + 1), est(Q.ned + 1);
  for (size_t s = 0; s < ns; s++) {
    memcpy(&hs[32 * s], hashes + 32 * Q.stx[s].tx, 32);
    memcpy(&bv[32 * s], bvk + 32 * Q.stx[s].tx, 32);
    bst[s] = bvk_st[Q.stx[s].tx];
    ok[Q.stx[s].rj] = bind_ok[Q.stx[s].tx];
    if (Q.stx[s].ed != SHD_NO_ROW) est[Q.stx[s].ed] = ed[Q.stx[s].tx];
  }
  for (size_t d = 0; d < nd; d++) {
    shd_gather(arena, dtx.data(), Q.stx.data(), Q.desc[d], d, kinds, fields.data(), proofs, inputs, codes, cvs.data());
    if (Q.desc[d].kind == SHD_KIND_JOINSPLIT) continue;
    // k_prep_sapling's part: the same codes and rows (zg_prep.h)
    const uint8_t* f = &fields[(size_t)SHD_FIELD_BYTES * d];
    memset(inputs + 288 * d, 0, 288);
    codes[d] = (uint8_t)(Q.desc[d].kind == SHD_KIND_SPEND ? prep_spend(f, f + 32, f + 64, f + 96, inputs + 288 * d)
                                                           : prep_output(f, f + 32, f + 64, inputs + 288 * d));
    if (codes[d]) memset(inputs + 288 * d, 0, 288);
    if (memcmp(&cvs[32 * Q.desc[d].cv], f, 32)) return 2;
    if (Q.desc[d].kind == SHD_KIND_SPEND) ok[Q.desc[d].rj] = spend_ok[d];
  }
  for (size_t d = 0; d < nd; d++)
    shd_desc_rows(arena, dtx.data(), Q.stx.data(), Q.desc[d], d, codes, hs.data(), ninputs, vk.data(), sig.data(),
                  msg.data(), gen.data());
  for (size_t s = 0; s < ns; s++)
    shd_tx_rows(arena, dtx.data(), Q.stx[s], s, hs.data(), bv.data(), vk.data(), sig.data(), msg.data(), gen.data(),
                epk.data(), esig.data(), emsg.data());
  for (size_t r = 0; r < Q.nrj; r++) {
    memcpy(rj + 161 * r, &vk[32 * r], 32);
    memcpy(rj + 161 * r + 32, &sig[64 * r], 64);
    memcpy(rj + 161 * r + 96, &msg[64 * r], 64);
    rj[161 * r + 160] = gen[r];
  }
  for (size_t e = 0; e < Q.ned; e++) {
    memcpy(edrows + 128 * e, &epk[32 * e], 32);
    memcpy(edrows + 128 * e + 32, &esig[64 * e], 64);
    memcpy(edrows + 128 * e + 96, &emsg[32 * e], 32);
  }
  for (size_t d = 0; d < nd; d++) desc_status[d] = (uint8_t)shd_desc_status(Q.desc[d], codes[d], ok.data(), proof[d]);
  for (size_t s = 0; s < ns; s++) {
    uint32_t ix, dt;
    const size_t t = Q.stx[s].tx;
    status[t] = (uint8_t)shd_tx_fold(dtx[t].L, Q.stx[s], desc_status, est.data(), ok.data(), bst[s], &ix, &dt);
    index[t] = ix, detail[t] = (uint8_t)dt;
  }
  return 0;
}

// the device's JoinSplit preparation over a serialized description and the pubkey, as shd_gather calls it
extern "C" void zgh_prep_joinsplit(const uint8_t* p, const uint8_t* pubkey, uint8_t* out) {
  prep_joinsplit_bits(p + 16, p + 208, p + 48, p + 80, p + 240, p + 272, p + 112, p + 144, p, p + 8, pubkey, 254, out);
}

#ifdef ZG_SHD_MAIN
static int run_exact(const uint8_t* tx, size_t len, uint32_t branch, uint64_t* sum) {
  uint8_t* blk = (uint8_t*)malloc(len ? len : 1);  // exactly the slice: a read past it is the sanitizer's to report
  memcpy(blk, tx, len);
  const uint64_t off[2] = {0, len};
  const size_t cap = len / 384 + 1;
  std::vector<uint8_t> zero(32 + cap), one(cap + 1, 1), ds(cap), kinds(cap), codes(cap), nin(cap), inputs(288 * cap),
      proofs(192 * cap), rj(161 * (cap + 1)), ed(128);
  uint8_t ts, st, dt;
  uint64_t ix, doff[2], counts[4];
  const int rc = zgh_shielded_verify(1, blk, off, &branch, zero.data(), zero.data(), zero.data(), one.data(), zero.data(),
                                     one.data(), zero.data(), &ts, &st, &ix, &dt, doff, ds.data(), kinds.data(),
                                     codes.data(), nin.data(), inputs.data(), proofs.data(), rj.data(), ed.data(), counts);
  free(blk);
  *sum = *sum * 31 + ts * 7 + st;
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char line[1 << 21];
  uint64_t sum = 0;
  size_t n = 0;
  while (fgets(line, sizeof line, f)) {
    unsigned branch;
    int at = 0;
    if (sscanf(line, "%x %n", &branch, &at) != 1) return 3;
    std::vector<uint8_t> tx;
    for (const char* p = line + at; p[0] && p[1] && p[0] != '\n'; p += 2) {
      unsigned b;
      if (sscanf(p, "%2x", &b) != 1) return 3;
      tx.push_back((uint8_t)b);
    }
    if (run_exact(tx.data(), tx.size(), branch, &sum)) return 4;
    for (size_t k = 0; k < tx.size(); k++)
      if (run_exact(tx.data(), k, branch, &sum)) return 4;
    n++;
  }
  fclose(f);
  printf("%zu transactions, checksum %016llx\n", n, (unsigned long long)sum);
  return 0;
}
#endif
