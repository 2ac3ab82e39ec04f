// zg_hosttest_shielded_phgr.hip -- the PHGR plan, gather, row and fold routines of zebra_amd/csrc/zg_shielded.h compiled
// for the CPU (hipcc --offload-host-only): what zg_shielded_verify_flags and the kernels of zg_shielded_phgr.hip run,
// lane by lane, with the host side of the entry restated around them (the flag check, the two plans, the window's
// description offsets and the merge of the two plans' description classes). The v4 part of a window is
// zgh_shielded_verify of zg_hosttest_shielded.hip, included here as it is. The checks that other kernels make on the
// device (the signature hash, Ed25519, the PGHR13 pipeline and everything Sapling) are fed in by the caller, which
// computes them with the test oracle. Test harness only. Built two ways:
//   * a shared library (tests/shielded_phgr_hostlib.py): zgh_shielded_phgr_verify;
//   * with -DZG_SHD_MAIN a stand-alone program, meant to be built with -fsanitize=address,undefined: it reads
//     (branch id, transaction) lines, copies each transaction and, unless the line starts with '=', every proper
//     prefix of it into a heap block of exactly its size and runs the same routines over it with ZG_SHIELDED_PHGR and
//     all-passing verdicts.
#ifdef ZG_SHD_MAIN
#define ZG_SHP_MAIN
#undef ZG_SHD_MAIN  // the included file's own main stays out
#endif
#include "zg_hosttest_shielded.hip"

// As zgh_shielded_verify, with flags (-> -2, ZG_E_INVAL, for an unknown bit). hashes and ed are per transaction of the
// window, v4 or not; spend_ok and proof per v4 description in their order, pghr (ZG_STATUS_*) per PHGR description in
// theirs. Rows out, beside the v4 ones: pg_proofs 296 bytes and pg_inputs 288 bytes per PHGR description; the Ed25519
// rows of the transactions before v4 follow the v4 ones'. counts: v4 descriptions, RedJubjub rows, Ed25519 rows
// (all), v4 transactions, planned transactions before v4, PHGR descriptions.
extern "C" int zgh_shielded_phgr_verify(size_t ntx, const uint8_t* txs, const uint64_t* tx_off, const uint32_t* tx_branch_id,
                                        uint32_t flags, const uint8_t* hashes, const uint8_t* bvk, const uint8_t* bvk_st,
                                        const uint8_t* bind_ok, const uint8_t* ed, const uint8_t* spend_ok,
                                        const uint8_t* proof, const uint8_t* pghr, uint8_t* tx_status, uint8_t* status,
                                        uint64_t* index, uint8_t* detail, uint64_t* desc_off, uint8_t* desc_status,
                                        uint8_t* kinds, uint8_t* codes, uint8_t* ninputs, uint8_t* inputs, uint8_t* proofs,
                                        uint8_t* rj, uint8_t* edrows, uint8_t* pg_proofs, uint8_t* pg_inputs,
                                        uint64_t* counts) {
  if (flags & ~SHD_PHGR) return -2;
  size_t cap = 1;
  if (ntx) cap += (size_t)(tx_off[ntx] - tx_off[0]) / 384;
  std::vector<uint64_t> voff(ntx + 1);
  std::vector<uint8_t> vds(cap);
  counts[0] = counts[1] = counts[2] = counts[3] = counts[4] = counts[5] = 0;
  int rc = zgh_shielded_verify(ntx, txs, tx_off, tx_branch_id, hashes, bvk, bvk_st, bind_ok, ed, spend_ok, proof, tx_status,
                               status, index, detail, voff.data(), vds.data(), kinds, codes, ninputs, inputs, proofs, rj,
                               edrows, counts);
  if (rc) return rc;
  // the two plans again, as the entry holds them
  std::vector<ShDevTx> dtx(ntx ? ntx : 1);
  std::vector<uint32_t> in_off, out_off;
  std::vector<uint8_t> ts(ntx + 1), st4(ntx + 1);
  for (size_t t = 0; t < ntx; t++) {
    ts[t] = (uint8_t)tx_parse(txs + tx_off[t], (size_t)(tx_off[t + 1] - tx_off[t]), dtx[t].L, in_off, out_off);
    dtx[t].base = (uint32_t)(tx_off[t] - tx_off[0]);
    dtx[t].branch_id = tx_branch_id[t];
    dtx[t].dig = 0;
  }
  const uint8_t* arena = ntx ? txs + tx_off[0] : txs;
  ShdPlan Q;
  if (!shd_plan(dtx, ntx, arena, ts.data(), st4.data(), Q)) return 1;
  ShpPlan R;
  if ((flags & SHD_PHGR) && !shp_plan(dtx, ntx, Q.desc.size(), Q.ned, status, R)) return 1;
  const size_t ns = Q.stx.size(), np = R.ptx.size(), npd = R.desc.size();
  if (counts[3] != ns || counts[2] != Q.ned) return 3;
  counts[2] += np, counts[4] = np, counts[5] = npd;
  shd_desc_offsets(Q, R, ntx, desc_off);
  for (size_t q = 0; q < np; q++) R.ptx[q].hash = (uint32_t)q;
  std::vector<uint8_t> hs(32 * np + 1), epk(32 * (Q.ned + np) + 1), esig(64 * (Q.ned + np) + 1), emsg(32 * (Q.ned + np) + 1),
      est(Q.ned + np + 1), pds(npd + 1);
  for (size_t q = 0; q < np; q++) {
    memcpy(&hs[32 * q], hashes + 32 * R.ptx[q].tx, 32);
    est[R.ptx[q].ed] = ed[R.ptx[q].tx];
  }
  for (size_t d = 0; d < npd; d++) shp_gather(arena, dtx.data(), R.ptx.data(), R.desc[d], d, pg_proofs, pg_inputs);
  for (size_t q = 0; q < np; q++) {
    shp_tx_rows(arena, dtx.data(), R.ptx[q], hs.data(), epk.data(), esig.data(), emsg.data());
    const size_t e = R.ptx[q].ed;
    memcpy(edrows + 128 * e, &epk[32 * e], 32);
    memcpy(edrows + 128 * e + 32, &esig[64 * e], 64);
    memcpy(edrows + 128 * e + 96, &emsg[32 * e], 32);
  }
  for (size_t q = 0; q < np; q++) {
    uint32_t ix, dt;
    const size_t t = R.ptx[q].tx;
    status[t] = (uint8_t)shp_tx_fold(dtx[t].L, R.ptx[q], pghr, est.data(), pds.data(), &ix, &dt);
    index[t] = ix, detail[t] = (uint8_t)dt;
  }
  for (size_t s = 0; s < ns; s++) {
    const size_t t = Q.stx[s].tx;
    memcpy(desc_status + desc_off[t], vds.data() + Q.stx[s].desc0, (size_t)(desc_off[t + 1] - desc_off[t]));
  }
  for (size_t q = 0; q < np; q++) {
    const size_t t = R.ptx[q].tx;
    memcpy(desc_status + desc_off[t], pds.data() + R.ptx[q].desc0, (size_t)(desc_off[t + 1] - desc_off[t]));
  }
  return 0;
}

#ifdef ZG_SHP_MAIN
static int run_exact_phgr(const uint8_t* tx, size_t len, uint32_t branch, uint64_t* sum) {
  uint8_t* blk = (uint8_t*)malloc(len ? len : 1);  // exactly the slice: a read past it is the sanitizer's to report
  memcpy(blk, tx, len);
  const uint64_t off[2] = {0, len};
  const size_t cap = len / 384 + 1;
  std::vector<uint8_t> zero(32 + cap), one(cap + 1, 1), ds(cap), kinds(cap), codes(cap), nin(cap), inputs(288 * cap),
      proofs(192 * cap), rj(161 * (cap + 1)), ed(128), pgp(296 * cap), pgi(288 * cap);
  uint8_t ts, st, dt;
  uint64_t ix, doff[2], counts[6];
  const int rc = zgh_shielded_phgr_verify(1, blk, off, &branch, SHD_PHGR, zero.data(), zero.data(), zero.data(), one.data(),
                                          zero.data(), one.data(), zero.data(), zero.data(), &ts, &st, &ix, &dt, doff,
                                          ds.data(), kinds.data(), codes.data(), nin.data(), inputs.data(), proofs.data(),
                                          rj.data(), ed.data(), pgp.data(), pgi.data(), counts);
  free(blk);
  *sum = *sum * 31 + ts * 7 + st + counts[5];
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
    const bool whole_only = line[0] == '=';
    unsigned branch;
    int at = 0;
    if (sscanf(line + whole_only, "%x %n", &branch, &at) != 1) return 3;
    std::vector<uint8_t> tx;
    for (const char* p = line + whole_only + at; p[0] && p[1] && p[0] != '\n'; p += 2) {
      unsigned b;
      if (sscanf(p, "%2x", &b) != 1) return 3;
      tx.push_back((uint8_t)b);
    }
    if (run_exact_phgr(tx.data(), tx.size(), branch, &sum)) return 4;
    for (size_t k = 0; !whole_only && k < tx.size(); k++)
      if (run_exact_phgr(tx.data(), k, branch, &sum)) return 4;
    n++;
  }
  fclose(f);
  printf("%zu transactions, checksum %016llx\n", n, (unsigned long long)sum);
  return 0;
}
#endif
