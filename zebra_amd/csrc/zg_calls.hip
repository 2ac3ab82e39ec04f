// zg_calls.hip -- the one-shot entries of the C ABI (include/zg.h): signatures, signature hashes, template inputs, block
// bodies and headers, input preparation, note-commitment trees and PGHR13 proofs. Each validates its
// arguments, takes the context's lock and device, moves its buffers (zg_host.h) and calls the launch_*,
// merkle_* or bn_* of the unit that holds the kernels; none is launched from here. The Groth16 batch
// pipeline and the context's lifecycle are zg.hip.
#include <array>
#include <type_traits>

#include "zg_host.h"
#include "zg_blocks.h"
#include "zg_ecdsa.h"    // ZG_EC_COMB_*
#include "zg_ed25519.h"  // ZG_ED_COMB_*
#include "zg_inputs.h"
#include "zg_jubjub.h"   // ZG_JJ_COMB_*
#include "zg_multisig.h"
#include "zg_prep.h"
#include "zg_shielded.h"
#include "zg_sighash.h"
#include "zg_vk_embed.h"  // generated from zebra_amd/res/*.json by zebra_amd/build.py

using namespace zg;

namespace zg {
hipError_t launch_jj_comb(hipStream_t st, uint32_t* table);                                    // zg_jubjub.hip
hipError_t launch_redjubjub(hipStream_t st, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                            const uint8_t* gen, int n, const uint32_t* comb, uint8_t* ok);
hipError_t launch_jj_decode(hipStream_t st, const uint8_t* pts, int n, uint8_t* status, uint8_t* xy);
hipError_t launch_ed_comb(hipStream_t st, uint32_t* table);                                    // zg_ed25519.hip
hipError_t launch_ec_comb(hipStream_t st, uint32_t* table);                                    // zg_ecdsa.hip
hipError_t launch_ecdsa(hipStream_t st, const uint8_t* pubkeys, const uint8_t* pubkey_len, const uint8_t* sigs,
                        const uint32_t* sig_off, const uint8_t* msg, int n, const uint32_t* comb, uint8_t* status);
hipError_t launch_ed25519(hipStream_t st, const uint8_t* pubkey, const uint8_t* sig, const uint8_t* msg, int n,
                          const uint32_t* comb, uint8_t* status);
hipError_t launch_sighash_digests(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const uint32_t* in_off,
                                  const uint32_t* out_off, const uint32_t* jobs, int njobs, uint8_t* digests);  // zg_sighash.hip
hipError_t launch_sighash_items(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const uint32_t* in_off,
                                const uint32_t* out_off, const uint8_t* digests, const uint8_t* scripts,
                                const ShDevItem* items, int n, uint8_t* hashes);
hipError_t launch_script_items(hipStream_t st, const uint8_t* arena, const uint8_t* prev, const ScDevItem* items, int n,
                               uint32_t flags, uint8_t* pubkeys, uint8_t* pubkey_len, uint8_t* sigs,
                               uint8_t* status);                                                   // zg_script.hip
hipError_t launch_multisig_items(hipStream_t st, const uint8_t* arena, const uint8_t* prev, const MsDevItem* items, int n,
                                 uint8_t* hash_bad);                                               // zg_multisig.hip
hipError_t launch_multisig_rows(hipStream_t st, const uint8_t* arena, const uint8_t* prev, const MsDevItem* items,
                                const MsDevSig* sigrec, int n, const uint8_t* hashes, uint8_t* pubkeys,
                                uint8_t* pubkey_len, uint8_t* sigs, uint32_t* sig_off, uint8_t* msg, uint8_t* enc_bad);
hipError_t launch_multisig_fold(hipStream_t st, const MsDevItem* items, const MsDevSig* sigrec, const uint32_t* sig_at,
                                int n, const uint8_t* hash_bad, const uint8_t* enc_bad, const uint8_t* ec, uint32_t flags,
                                uint8_t* status, uint8_t* detail, uint32_t* last);
hipError_t launch_txid(hipStream_t st, const uint8_t* arena, const TxidSlice* slices, int n, uint8_t* out);  // zg_blocks.hip
hipError_t launch_block_merkle(hipStream_t st, const uint8_t* arena, const MerkleBlk* blks, int nblk,
                               const uint8_t* ids, uint8_t* ping, uint8_t* pong, uint8_t* roots, uint8_t* match);
int equihash_solution_bytes(int params);                                                      // zg_equihash.hip
hipError_t launch_equihash(hipStream_t st, int params, const uint8_t* inputs, size_t in_stride, int in_len,
                           const uint8_t* sols, size_t sol_stride, int n, uint8_t* ok, uint8_t* repeated);
hipError_t launch_headers(hipStream_t st, const uint8_t* headers, int n, uint32_t max_bits, uint8_t* eq_ok,
                          uint8_t* eq_rep, uint8_t* status, uint8_t* hashes, uint8_t* flags);
hipError_t launch_prep_sapling(hipStream_t st, const uint8_t* kinds, const uint8_t* fields, int n, uint8_t* inputs,
                               uint8_t* codes);
hipError_t launch_sapling_bvk(hipStream_t st, int ntx, const uint32_t* off, const uint32_t* nspends,
                              const uint8_t* cvs, const int64_t* vb, const uint32_t* comb, uint8_t* bvk,
                              uint8_t* status);
hipError_t launch_shd_gather(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const ShdTx* stx,
                             const ShdDesc* desc, int nd, uint8_t* kinds, uint8_t* fields, uint8_t* proofs,
                             uint8_t* inputs, uint8_t* codes, uint8_t* cvs);                        // zg_shielded.hip
hipError_t launch_shd_rows(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const ShdTx* stx, int ns,
                           const ShdDesc* desc, int nd, const uint8_t* codes, const uint8_t* hashes,
                           const uint8_t* bvk, uint8_t* ninputs, uint8_t* rj_vk, uint8_t* rj_sig, uint8_t* rj_msg,
                           uint8_t* rj_gen, uint8_t* ed_pk, uint8_t* ed_sig, uint8_t* ed_msg);
hipError_t launch_shd_fold(hipStream_t st, const ShDevTx* txs, const ShdTx* stx, int ns, const ShdDesc* desc, int nd,
                           const uint8_t* codes, const uint8_t* rj_ok, const uint8_t* proof_status, const uint8_t* ed,
                           const uint8_t* bvk_st, uint8_t* desc_status, uint8_t* status, uint32_t* index,
                           uint8_t* detail);
hipError_t launch_shp_gather(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const ShpTx* ptx,
                             const ShpDesc* desc, int nd, uint8_t* proofs, uint8_t* inputs);       // zg_shielded_phgr.hip
hipError_t launch_shp_rows(hipStream_t st, const uint8_t* arena, const ShDevTx* txs, const ShpTx* ptx, int np,
                           const uint8_t* hashes, uint8_t* ed_pk, uint8_t* ed_sig, uint8_t* ed_msg);
hipError_t launch_shp_fold(hipStream_t st, const ShDevTx* txs, const ShpTx* ptx, int np, const uint8_t* proof_status,
                           const uint8_t* ed, uint8_t* desc_status, uint8_t* status, uint32_t* index, uint8_t* detail);
}  // namespace zg

// ------------------------------------------------------------------ signature and header calls: shared pieces
// a fixed-base comb table of the device (*slot, a member of zg_dev), built on first use by `launch`
static int comb_table(zg_ctx* ctx, uint32_t** slot, size_t bytes, hipError_t (*launch)(hipStream_t, uint32_t*),
                      const char* what, const uint32_t** out) {
  std::lock_guard<std::mutex> g(ctx->dev->mu);
  if (!*slot) {
    DevScratch s;
    uint32_t* t = nullptr;
    HIPCHK(s.alloc(&t, bytes));
    hipError_t e = launch(ctx->stream, t);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ZG_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    *slot = s.release(t);  // built: the device keeps it (dev_release frees it)
  }
  *out = *slot;
  return ZG_OK;
}

// The two events around a call's kernels (created on first use): sig_timed brackets the launch, sig_sync
// waits for the stream after the copies back and keeps the kernel time for zg_last_sig_kernel_ms
template <class Launch>
static hipError_t sig_timed(zg_ctx* ctx, Launch launch) {
  for (hipEvent_t& e : ctx->sig_ev)
    if (!e) {
      const hipError_t r = hipEventCreate(&e);
      if (r != hipSuccess) return r;
    }
  hipError_t r = hipEventRecord(ctx->sig_ev[0], ctx->stream);
  if (r == hipSuccess) r = launch();
  if (r == hipSuccess) r = hipEventRecord(ctx->sig_ev[1], ctx->stream);
  return r;
}
static hipError_t sig_sync(zg_ctx* ctx) {
  const hipError_t r = hipStreamSynchronize(ctx->stream);
  if (r == hipSuccess) hipEventElapsedTime(&ctx->sig_ms, ctx->sig_ev[0], ctx->sig_ev[1]);
  return r;
}

extern "C" int zg_last_sig_kernel_ms(zg_ctx* ctx, float* ms) {
  if (!ctx || !ms) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  *ms = ctx->sig_ms;
  return ZG_OK;
}

// ------------------------------------------------------------------ Sapling signatures (zg_jubjub.h)
extern "C" int zg_redjubjub_verify(zg_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                                   const uint8_t* gen, uint8_t* ok) {
  if (!ctx || (n && (!vk || !sig || !msg || !gen || !ok)) || n > (1u << 30)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!n) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const uint32_t* comb = nullptr;
  int rc = comb_table(ctx, &ctx->dev->jj_comb, sizeof(uint32_t) * ZG_JJ_COMB_WORDS * ZG_JJ_COMB_POINTS, launch_jj_comb,
                      "Jubjub comb tables", &comb);
  if (rc) return rc;
  DevScratch s;
  uint8_t *dvk, *dsig, *dmsg, *dgen, *dok;
  HIPCHK(s.up(&dvk, vk, 32 * n, ctx->stream));
  HIPCHK(s.up(&dsig, sig, 64 * n, ctx->stream));
  HIPCHK(s.up(&dmsg, msg, 64 * n, ctx->stream));
  HIPCHK(s.up(&dgen, gen, n, ctx->stream));
  HIPCHK(s.alloc(&dok, n));
  HIPCHK(sig_timed(ctx, [&] { return launch_redjubjub(ctx->stream, dvk, dsig, dmsg, dgen, (int)n, comb, dok); }));
  HIPCHK(hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  return ZG_OK;
}

// ------------------------------------------------------------------ JoinSplit signatures (zg_ed25519.h)
extern "C" int zg_ed25519_verify(zg_ctx* ctx, size_t n, const uint8_t* pubkey, const uint8_t* sig, const uint8_t* msg,
                                 uint8_t* status) {
  if (!ctx || (n && (!pubkey || !sig || !msg || !status)) || n > (1u << 30)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!n) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const uint32_t* comb = nullptr;
  int rc = comb_table(ctx, &ctx->dev->ed_comb, sizeof(uint32_t) * ZG_ED_COMB_WORDS * ZG_ED_COMB_POINTS, launch_ed_comb,
                      "Ed25519 comb table", &comb);
  if (rc) return rc;
  DevScratch s;
  uint8_t *dpk, *dsig, *dmsg, *dst;
  HIPCHK(s.up(&dpk, pubkey, 32 * n, ctx->stream));
  HIPCHK(s.up(&dsig, sig, 64 * n, ctx->stream));
  HIPCHK(s.up(&dmsg, msg, 32 * n, ctx->stream));
  HIPCHK(s.alloc(&dst, n));
  HIPCHK(sig_timed(ctx, [&] { return launch_ed25519(ctx->stream, dpk, dsig, dmsg, (int)n, comb, dst); }));
  HIPCHK(hipMemcpyAsync(status, dst, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  return ZG_OK;
}

// ------------------------------------------------------------------ transparent input signatures (zg_ecdsa.h)
extern "C" int zg_ecdsa_verify(zg_ctx* ctx, size_t n, const uint8_t* pubkeys, const uint8_t* pubkey_len,
                               const uint8_t* sigs, const uint32_t* sig_off, const uint8_t* msg, uint8_t* status) {
  if (!ctx || (n && (!pubkeys || !pubkey_len || !sigs || !sig_off || !msg || !status)) || n > (1u << 30))
    return ZG_E_INVAL;
  // a lane reads sigs[sig_off[i] .. sig_off[i+1]) of a buffer of sig_off[n] bytes
  if (!offsets_ok(sig_off, n, 0)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!n) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const uint32_t* comb = nullptr;
  int rc = comb_table(ctx, &ctx->dev->ec_comb, sizeof(uint32_t) * ZG_EC_COMB_WORDS * ZG_EC_COMB_POINTS, launch_ec_comb,
                      "secp256k1 comb table", &comb);
  if (rc) return rc;
  const size_t sig_bytes = (size_t)sig_off[n] - sig_off[0];
  DevScratch s;
  uint8_t *dpk, *dlen, *dsig, *dmsg, *dst;
  uint32_t* doff;
  HIPCHK(s.up(&dpk, pubkeys, ZG_ECDSA_PUBKEY_STRIDE * n, ctx->stream));
  HIPCHK(s.up(&dlen, pubkey_len, n, ctx->stream));
  HIPCHK(s.up(&dsig, sigs + sig_off[0], sig_bytes, ctx->stream));
  HIPCHK(s.up(&doff, sig_off, sizeof(uint32_t) * (n + 1), ctx->stream));
  HIPCHK(s.up(&dmsg, msg, 32 * n, ctx->stream));
  HIPCHK(s.alloc(&dst, n));
  // the device buffer starts at sig_off[0]: the kernel subtracts it
  HIPCHK(sig_timed(ctx, [&] { return launch_ecdsa(ctx->stream, dpk, dlen, dsig, doff, dmsg, (int)n, comb, dst); }));
  HIPCHK(hipMemcpyAsync(status, dst, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  return ZG_OK;
}

// ------------------------------------------------------------------ signature hashes (zg_sighash.h)
// The planning half of a signature-hash launch, shared by zg_sighash and zg_inputs_verify: the layouts
// (sh_plan_txs), the items a lane takes as the caller gathers them (sh_plan_add), then the launch order and the
// digest jobs (sh_plan_finish)
struct ShPlan {
  std::vector<ShDevTx> dtx;
  std::vector<uint32_t> in_off, out_off;
  std::vector<ShDevItem> items;  // as gathered; sh_plan_finish orders them by cost, the dearest first
  std::vector<uint64_t> cost;    // per gathered item
  std::vector<uint8_t> need;     // per transaction: the digests its items read
  std::vector<uint32_t> jobs;    // (transaction << 3) | digest
  uint32_t ndig = 0;
};
// the layouts: every offset a lane follows is checked here
static void sh_plan_txs(ShPlan& P, size_t ntx, const uint8_t* txs, const uint64_t* tx_off, const uint32_t* tx_branch_id,
                        uint8_t* tx_status) {
  const uint64_t base0 = ntx ? tx_off[0] : 0;
  P.dtx.assign(ntx ? ntx : 1, ShDevTx{});
  for (size_t t = 0; t < ntx; t++) {
    ShDevTx& d = P.dtx[t];
    tx_status[t] = (uint8_t)tx_parse(txs + tx_off[t], (size_t)(tx_off[t + 1] - tx_off[t]), d.L, P.in_off, P.out_off);
    d.base = (uint32_t)(tx_off[t] - base0);
    d.branch_id = tx_branch_id[t];
    d.dig = 0;
  }
  P.need.assign(ntx ? ntx : 1, 0);
}
// an item of a transaction that parsed, its index in range where the format asks for that
static void sh_plan_add(ShPlan& P, const ShDevItem& it) {
  const TxLayout& L = P.dtx[it.tx].L;
  const uint32_t base = sh_base(it.hashtype), acp = it.hashtype & 0x80;
  const uint32_t slen = it.script_len;
  P.items.push_back(it);
  if (L.sigver) {
    P.need[it.tx] |= (uint8_t)((acp ? 0 : 1 << SH_PREVOUTS) | (!acp && base == SH_ALL ? 1 << SH_SEQUENCES : 0) |
                               (base == SH_ALL ? 1 << SH_OUTPUTS : 0) | (L.n_js ? 1 << SH_JOINSPLITS : 0) |
                               (L.sigver == 2 && L.n_spend ? 1 << SH_SPENDS : 0) |
                               (L.sigver == 2 && L.n_sout ? 1 << SH_SOUTPUTS : 0));
    P.cost.push_back(2 * (uint64_t)(512 + slen));  // a BLAKE2b compression per 128 bytes, about two SHA-256 ones
  } else {
    P.cost.push_back(acp ? 256 + (uint64_t)slen + L.consumed - L.lock_off : (uint64_t)L.consumed + slen);
  }
}
static void sh_plan_finish(ShPlan& P, size_t ntx) {
  const std::vector<uint64_t>& cost = P.cost;
  const std::vector<uint8_t>& need = P.need;
  std::vector<uint32_t> order(P.items.size());
  for (size_t k = 0; k < order.size(); k++) order[k] = (uint32_t)k;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
  std::vector<ShDevItem> sorted(P.items.size());
  for (size_t k = 0; k < order.size(); k++) sorted[k] = P.items[order[k]];
  P.items.swap(sorted);
  for (size_t t = 0; t < ntx; t++)
    if (need[t]) {
      P.dtx[t].dig = P.ndig++;
      for (int w = 0; w < SH_DIGESTS; w++)
        if (need[t] >> w & 1) P.jobs.push_back((uint32_t)(t << 3) | (uint32_t)w);
    }
}
// what the two kernels read and write, on the device
struct ShDev {
  uint8_t *arena, *scripts, *dig, *hash;  // hash: 32 bytes per planned item, in the plan's order
  ShDevTx* txs;
  ShDevItem* items;
  uint32_t *in, *out, *jobs;
};
// the buffers' sizes, in the order sh_upload asks its owner for them
static std::array<size_t, 9> sh_dev_bytes(const ShPlan& P, size_t ntx, size_t arena_bytes, size_t script_bytes) {
  const size_t m = P.items.size();
  return {arena_bytes + 8,  // (most of these are longer than what is copied into them)
          script_bytes + 8, (size_t)32 * SH_DIGESTS * (P.ndig ? P.ndig : 1), 32 * m, sizeof(ShDevTx) * ntx,
          sizeof(ShDevItem) * m, sizeof(uint32_t) * (P.in_off.size() + 1), sizeof(uint32_t) * (P.out_off.size() + 1),
          sizeof(uint32_t) * (P.jobs.size() + 1)};
}
// alloc(&pointer, bytes) -> hipError_t: the call's own allocations (zg_sighash) or parts of a context's arena.
// tail: further script bytes, which follow `scripts` on the device (items index them from script_bytes on)
template <class Alloc>
static int sh_upload(zg_ctx* ctx, Alloc alloc, const ShPlan& P, size_t ntx, const uint8_t* arena, size_t arena_bytes,
                     const uint8_t* scripts, size_t script_bytes, ShDev& D, const uint8_t* tail = nullptr,
                     size_t tail_bytes = 0) {
  const size_t m = P.items.size();
  const std::array<size_t, 9> b = sh_dev_bytes(P, ntx, arena_bytes, script_bytes + tail_bytes);
  HIPCHK(alloc(&D.arena, b[0]));
  HIPCHK(alloc(&D.scripts, b[1]));
  HIPCHK(alloc(&D.dig, b[2]));
  HIPCHK(alloc(&D.hash, b[3]));
  HIPCHK(alloc(&D.txs, b[4]));
  HIPCHK(alloc(&D.items, b[5]));
  HIPCHK(alloc(&D.in, b[6]));
  HIPCHK(alloc(&D.out, b[7]));
  HIPCHK(alloc(&D.jobs, b[8]));
  HIPCHK(hipMemcpyAsync(D.arena, arena, arena_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (script_bytes) HIPCHK(hipMemcpyAsync(D.scripts, scripts, script_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (tail_bytes) HIPCHK(hipMemcpyAsync(D.scripts + script_bytes, tail, tail_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(D.txs, P.dtx.data(), sizeof(ShDevTx) * ntx, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(D.items, P.items.data(), sizeof(ShDevItem) * m, hipMemcpyHostToDevice, ctx->stream));
  if (!P.in_off.empty())
    HIPCHK(hipMemcpyAsync(D.in, P.in_off.data(), sizeof(uint32_t) * P.in_off.size(), hipMemcpyHostToDevice, ctx->stream));
  if (!P.out_off.empty())
    HIPCHK(hipMemcpyAsync(D.out, P.out_off.data(), sizeof(uint32_t) * P.out_off.size(), hipMemcpyHostToDevice, ctx->stream));
  if (!P.jobs.empty())
    HIPCHK(hipMemcpyAsync(D.jobs, P.jobs.data(), sizeof(uint32_t) * P.jobs.size(), hipMemcpyHostToDevice, ctx->stream));
  return ZG_OK;
}
static hipError_t sh_launch(zg_ctx* ctx, const ShPlan& P, const ShDev& D) {
  const hipError_t e = launch_sighash_digests(ctx->stream, D.arena, D.txs, D.in, D.out, D.jobs, (int)P.jobs.size(), D.dig);
  if (e != hipSuccess) return e;
  return launch_sighash_items(ctx->stream, D.arena, D.txs, D.in, D.out, D.dig, D.scripts, D.items, (int)P.items.size(),
                              D.hash);
}

extern "C" int zg_sighash(zg_ctx* ctx, size_t ntx, const uint8_t* txs, const uint64_t* tx_off,
                          const uint32_t* tx_branch_id, size_t n, const uint32_t* item_tx, const uint32_t* input_index,
                          const uint8_t* scripts, const uint32_t* script_off, const uint64_t* amount,
                          const uint32_t* hashtype, uint8_t* tx_status, uint8_t* hashes, uint8_t* status) {
  if (!ctx || (ntx && (!txs || !tx_off || !tx_branch_id || !tx_status)) ||
      (n && (!item_tx || !input_index || !scripts || !script_off || !amount || !hashtype || !hashes || !status)) ||
      ntx > (1u << 30) || n > (1u << 30))
    return ZG_E_INVAL;
  if (!offsets_ok(tx_off, ntx, 1ull << 31) || !offsets_ok(script_off, n, 0)) return ZG_E_INVAL;
  for (size_t i = 0; i < n; i++)
    if (item_tx[i] >= ntx) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!ntx && !n) return ZG_OK;

  ShPlan P;
  sh_plan_txs(P, ntx, txs, tx_off, tx_branch_id, tx_status);
  // the items a lane takes
  P.items.reserve(n);
  for (size_t i = 0; i < n; i++) {
    const TxLayout& L = P.dtx[item_tx[i]].L;
    const uint8_t ts = tx_status[item_tx[i]];
    memset(hashes + 32 * i, 0, 32);
    status[i] = ts == ZG_TX_MALFORMED ? ZG_SIGHASH_TX_MALFORMED : ts == ZG_TX_NONCANONICAL ? ZG_SIGHASH_TX_NONCANONICAL
              : L.sigver && input_index[i] != ZG_SIGHASH_NO_INPUT && input_index[i] >= L.n_in ? ZG_SIGHASH_INPUT_RANGE
                                                                                             : ZG_SIGHASH_OK;
    if (status[i] != ZG_SIGHASH_OK) continue;
    const uint32_t base = sh_base(hashtype[i]), acp = hashtype[i] & 0x80;
    if (!L.sigver && input_index[i] >= L.n_in && (acp || base == SH_SINGLE)) continue;  // the zero hash, OK
    sh_plan_add(P, ShDevItem{item_tx[i], input_index[i], script_off[i] - script_off[0],
                             script_off[i + 1] - script_off[i], hashtype[i], (uint32_t)i, amount[i]});
  }
  sh_plan_finish(P, ntx);
  const size_t m = P.items.size();
  if (!m) return ZG_OK;

  HIPCHK(hipSetDevice(ctx->device));
  const uint64_t base0 = tx_off[0];
  DevScratch s;
  ShDev D;
  const int rc = sh_upload(ctx, [&](auto** p, size_t bytes) { return s.alloc(p, bytes); }, P, ntx, txs + base0,
                           (size_t)(tx_off[ntx] - base0), scripts + script_off[0],
                           (size_t)script_off[n] - script_off[0], D);
  if (rc) return rc;
  HIPCHK(sig_timed(ctx, [&] { return sh_launch(ctx, P, D); }));
  std::vector<uint8_t> hh(32 * m);
  HIPCHK(hipMemcpyAsync(hh.data(), D.hash, 32 * m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  for (size_t k = 0; k < m; k++) memcpy(hashes + (size_t)32 * P.items[k].slot, hh.data() + 32 * k, 32);
  return ZG_OK;
}

// ------------------------------------------------------------------ template inputs (zg_script.h, zg_inputs.h)
// where input k's script_sig lies in a parsed, canonical transaction: after the outpoint and the compact size
static void input_script_sig(const uint8_t* tx, const uint32_t* in_off, uint32_t k, uint32_t* off, uint32_t* len) {
  const uint32_t o = in_off[k] + 36, tag = tx[o];
  const uint32_t w = tag < 0xfd ? 1 : tag == 0xfd ? 3 : tag == 0xfe ? 5 : 9;
  *off = o + w;
  *len = in_off[k + 1] - 4 - *off;
}

extern "C" int zg_inputs_verify(zg_ctx* ctx, size_t ntx, const uint8_t* txs, const uint64_t* tx_off,
                                const uint32_t* tx_branch_id, size_t n, const uint32_t* item_tx,
                                const uint32_t* input_index, const uint8_t* prev_scripts, const uint32_t* prev_off,
                                const uint64_t* amount, uint32_t flags, uint8_t* tx_status, uint8_t* status,
                                uint8_t* detail, uint8_t* hashes) {
  if (!ctx || (ntx && (!txs || !tx_off || !tx_branch_id || !tx_status)) ||
      (n && (!item_tx || !input_index || !prev_scripts || !prev_off || !amount || !status)) || ntx > (1u << 30) ||
      n > (1u << 30) || (flags & ~(uint32_t)(ZG_SCRIPT_VERIFY_DERSIG | ZG_SCRIPT_TEMPLATE_MULTISIG)))
    return ZG_E_INVAL;
  if (!offsets_ok(tx_off, ntx, 1ull << 31) || !offsets_ok(prev_off, n, 0)) return ZG_E_INVAL;
  for (size_t i = 0; i < n; i++)
    if (item_tx[i] >= ntx) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!ntx && !n) return ZG_OK;

  ShPlan P;
  sh_plan_txs(P, ntx, txs, tx_off, tx_branch_id, tx_status);
  // the template inputs: the matcher validates every offset a lane of k_script_items follows
  const uint32_t prev0 = n ? prev_off[0] : 0;
  const size_t prev_bytes = n ? (size_t)prev_off[n] - prev0 : 0;
  std::vector<ScDevItem> rec(n ? n : 1);
  // the multisig items (zg_multisig.h): their records, the caller's item of each, their signature pushes as
  // gathered, and the redeem scripts, which follow the previous scripts on the device as script codes
  std::vector<MsDevItem> ms;
  std::vector<uint32_t> ms_slot;
  std::vector<MsDevSig> ms_sig;
  std::vector<uint8_t> redeem;
  uint64_t pair_rows = 0;
  P.items.reserve(n);
  for (size_t i = 0; i < n; i++) {
    const ShDevTx& d = P.dtx[item_tx[i]];
    const uint8_t ts = tx_status[item_tx[i]];
    if (detail) detail[i] = 0;
    if (hashes) memset(hashes + 32 * i, 0, 32);
    status[i] = ts == ZG_TX_MALFORMED ? ZG_INPUT_TX_MALFORMED : ts == ZG_TX_NONCANONICAL ? ZG_INPUT_TX_NONCANONICAL
              : input_index[i] >= d.L.n_in ? ZG_INPUT_RANGE : ZG_INPUT_HOST;
    if (status[i] != ZG_INPUT_HOST) continue;
    const uint8_t* tx = txs + tx_off[item_tx[i]];
    uint32_t so, sl;
    input_script_sig(tx, P.in_off.data() + d.L.in_idx, input_index[i], &so, &sl);
    const uint8_t* pk = prev_scripts + prev_off[i];
    const uint32_t pl = prev_off[i + 1] - prev_off[i];
    const ScriptMatch sm = script_match(tx + so, sl, pk, pl, flags);
    if (sm.cls == SCRIPT_HOST) continue;
    status[i] = ZG_INPUT_OK;
    const uint32_t poff = prev_off[i] - prev0;
    if (sm.cls >= SCRIPT_MULTISIG) {
      const bool p2sh = sm.cls == SCRIPT_P2SH_MULTISIG;
      if (prev_bytes + redeem.size() + sm.red_len > 0xffffffffull)
        return fail(ctx, ZG_E_INVAL, "zg_inputs_verify: the script codes exceed 4 GiB");
      // the script code: the script being evaluated, whole (interpreter.rs:814)
      const uint32_t code_off = p2sh ? (uint32_t)(prev_bytes + redeem.size()) : poff, code_len = p2sh ? sm.red_len : pl;
      if (p2sh) redeem.insert(redeem.end(), tx + so + sm.red_off, tx + so + sm.red_off + sm.red_len);
      ms.push_back(MsDevItem{p2sh, sm.m, sm.n, p2sh ? d.base + so + sm.red_off + 1 : poff + 1, d.base + so + sm.red_off,
                             sm.red_len, poff + 2, (uint32_t)ms_sig.size()});
      ms_slot.push_back((uint32_t)i);
      for (uint32_t s = 0; s < sm.m; s++) {  // pop order: the last pushed first
        const uint32_t o = sm.sig_off[sm.m - 1 - s], l = sm.sig_len[sm.m - 1 - s];
        // one signature hash per push; its slot, past the caller's items, names the push
        sh_plan_add(P, ShDevItem{item_tx[i], input_index[i], code_off, code_len, l ? tx[so + o + l - 1] : 1u,
                                 (uint32_t)(n + ms_sig.size()), amount[i]});
        ms_sig.push_back(MsDevSig{(uint32_t)ms.size() - 1, s, d.base + so + o, l, 0, 0});
      }
      pair_rows += sm.pairs();
      if (pair_rows > (1u << 30)) return fail(ctx, ZG_E_INVAL, "zg_inputs_verify: more than 2^30 ECDSA rows");
      continue;
    }
    const ScriptClass& c = sm.one;
    ScDevItem& r = rec[i];
    r.cls = c.cls;
    r.sig_off = d.base + so + c.sig_off, r.sig_len = c.sig_len;
    r.key_off = c.cls == SCRIPT_P2PKH ? d.base + so + c.key_off : poff + c.key_off, r.key_len = c.key_len;
    r.h160_off = poff + 3;
    r.der_off = 0, r.pad = 0;
    // the hashtype: the signature's last byte (check_signature, interpreter.rs:27); none for an empty push,
    // whose hash no verdict reads
    const uint32_t hashtype = c.sig_len ? tx[so + c.sig_off + c.sig_len - 1] : 1;
    sh_plan_add(P, ShDevItem{item_tx[i], input_index[i], poff, pl, hashtype, (uint32_t)i, amount[i]});
  }
  sh_plan_finish(P, ntx);
  const size_t m = P.items.size();
  if (!m) return ZG_OK;  // HOST, range and transaction errors only: nothing is launched
  // The planned items, dearest first within each part: the mt template items, whose ECDSA rows are rows 0 .. mt,
  // then the ng signature pushes of the multisig items; the pair rows of push g follow those of push g - 1
  const size_t ng = ms_sig.size(), mt = m - ng, nq = ms.size(), rows = mt + (size_t)pair_rows;
  if (rows > (1u << 30)) return fail(ctx, ZG_E_INVAL, "zg_inputs_verify: more than 2^30 ECDSA rows");
  if (ng) std::stable_partition(P.items.begin(), P.items.end(), [&](const ShDevItem& it) { return it.slot < n; });

  std::vector<ScDevItem> srec(mt);
  std::vector<uint32_t> sig_off(mt + 1);
  uint64_t der_bytes = 0;  // (items may name one input many times: the sum is not bounded by the arena's size)
  for (size_t k = 0; k < mt; k++) {
    srec[k] = rec[P.items[k].slot];
    srec[k].der_off = sig_off[k] = (uint32_t)der_bytes;
    der_bytes += srec[k].sig_len ? srec[k].sig_len - 1 : 0;
    if (der_bytes > 0xffffffffull) return fail(ctx, ZG_E_INVAL, "zg_inputs_verify: the signatures exceed 4 GiB");
  }
  sig_off[mt] = (uint32_t)der_bytes;
  std::vector<MsDevSig> gsig(ng);
  std::vector<uint32_t> sig_at(ng), row_sig((size_t)pair_rows);  // (item, s) -> push; pair row -> push
  for (size_t g = 0, row = 0; g < ng; g++) {
    MsDevSig& r = gsig[g] = ms_sig[P.items[mt + g].slot - n];
    const MsDevItem& q = ms[r.item];
    const uint32_t per = q.n - q.m + 1;
    r.row0 = (uint32_t)row, r.der0 = (uint32_t)der_bytes;
    sig_at[q.sig0 + r.s] = (uint32_t)g;
    for (uint32_t j = 0; j < per; j++) row_sig[row++] = (uint32_t)g;
    der_bytes += (uint64_t)per * (r.sig_len ? r.sig_len - 1 : 0);
    if (der_bytes > 0xffffffffull) return fail(ctx, ZG_E_INVAL, "zg_inputs_verify: the signatures exceed 4 GiB");
  }

  HIPCHK(hipSetDevice(ctx->device));
  const uint32_t* comb = nullptr;
  int rc = comb_table(ctx, &ctx->dev->ec_comb, sizeof(uint32_t) * ZG_EC_COMB_WORDS * ZG_EC_COMB_POINTS, launch_ec_comb,
                      "secp256k1 comb table", &comb);
  if (rc) return rc;
  // the context's arena (allocating per call costs more wall time than the kernels), every part 256-aligned
  const uint64_t base0 = tx_off[0];
  const size_t arena_bytes = (size_t)(tx_off[ntx] - base0);
  // the template rows' parts, sized for the pair rows as well where k_ecdsa reads them; then the multisig parts:
  // item and push records, sig_at, the messages of all rows, the hash and encoding flags, the fold's three outputs
  const size_t own[16] = {sizeof(ScDevItem) * mt, sizeof(uint32_t) * (rows + 1), (size_t)ZG_ECDSA_PUBKEY_STRIDE * rows,
                          rows, (size_t)der_bytes + 1, mt, rows,
                          sizeof(MsDevItem) * nq, sizeof(MsDevSig) * ng, sizeof(uint32_t) * ng, ng ? 32 * rows : 0, nq, ng,
                          nq, nq, sizeof(uint32_t) * nq};
  size_t need = 0;
  for (size_t b : sh_dev_bytes(P, ntx, arena_bytes, prev_bytes + redeem.size())) need += Carve::span(b, 256);
  for (size_t b : own) need += Carve::span(b, 256);
  DevArena& A = ctx->inputs_arena;
  HIPCHK(A.reserve(need, ctx->stream));
  ShDev D;
  rc = sh_upload(ctx, [&](auto** p, size_t bytes) {
    using T = typename std::remove_pointer<typename std::remove_pointer<decltype(p)>::type>::type;
    *p = (T*)A.carve<uint8_t>(bytes, 256);  // (no part is empty: sh_dev_bytes)
    return hipSuccess;
  }, P, ntx, txs + base0, arena_bytes, prev_scripts + prev0, prev_bytes, D, redeem.data(), redeem.size());
  if (rc) return rc;
  ScDevItem* const drec = (ScDevItem*)A.carve<uint8_t>(own[0], 256);
  uint32_t* const doff = (uint32_t*)A.carve<uint8_t>(own[1], 256);
  uint8_t* const dpk = A.carve<uint8_t>(own[2], 256);
  uint8_t* const dlen = A.carve<uint8_t>(own[3], 256);
  uint8_t* const dsig = A.carve<uint8_t>(own[4], 256);
  uint8_t* const dsc = A.carve<uint8_t>(own[5], 256);
  uint8_t* const dec = A.carve<uint8_t>(own[6], 256);
  MsDevItem* const dms = (MsDevItem*)A.carve<uint8_t>(own[7], 256);
  MsDevSig* const dgs = (MsDevSig*)A.carve<uint8_t>(own[8], 256);
  uint32_t* const dat = (uint32_t*)A.carve<uint8_t>(own[9], 256);
  uint8_t* const dmsg = A.carve<uint8_t>(own[10], 256);
  uint8_t* const dhb = A.carve<uint8_t>(own[11], 256);
  uint8_t* const denc = A.carve<uint8_t>(own[12], 256);
  uint8_t* const dfs = A.carve<uint8_t>(own[13], 256);
  uint8_t* const dfd = A.carve<uint8_t>(own[14], 256);
  uint32_t* const dfl = (uint32_t*)A.carve<uint8_t>(own[15], 256);
  if (mt) HIPCHK(hipMemcpyAsync(drec, srec.data(), own[0], hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(doff, sig_off.data(), sizeof(uint32_t) * (mt + 1), hipMemcpyHostToDevice, ctx->stream));
  if (ng) {
    HIPCHK(hipMemcpyAsync(dms, ms.data(), own[7], hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dgs, gsig.data(), own[8], hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dat, sig_at.data(), own[9], hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(sig_timed(ctx, [&] {
    hipError_t e = launch_script_items(ctx->stream, D.arena, D.scripts, drec, (int)mt, flags, dpk, dlen, dsig, dsc);
    if (e == hipSuccess && ng) e = launch_multisig_items(ctx->stream, D.arena, D.scripts, dms, (int)nq, dhb);
    if (e == hipSuccess) e = sh_launch(ctx, P, D);
    if (!ng) return e != hipSuccess ? e : launch_ecdsa(ctx->stream, dpk, dlen, dsig, doff, D.hash, (int)mt, comb, dec);
    // the messages of all rows in one buffer: the template rows' hashes, then what the pushes' lanes gather
    if (e == hipSuccess && mt) e = hipMemcpyAsync(dmsg, D.hash, 32 * mt, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess)
      e = launch_multisig_rows(ctx->stream, D.arena, D.scripts, dms, dgs, (int)ng, D.hash + 32 * mt,
                               dpk + (size_t)ZG_ECDSA_PUBKEY_STRIDE * mt, dlen + mt, dsig, doff + mt, dmsg + 32 * mt, denc);
    if (e == hipSuccess) e = launch_ecdsa(ctx->stream, dpk, dlen, dsig, doff, dmsg, (int)rows, comb, dec);
    if (e == hipSuccess)
      e = launch_multisig_fold(ctx->stream, dms, dgs, dat, (int)nq, dhb, denc, dec + mt, flags, dfs, dfd, dfl);
    return e;
  }));
  std::vector<uint8_t> hsc(mt), hec(mt), hh(hashes ? 32 * m : 0), hfs(nq), hfd(nq);
  std::vector<uint32_t> hfl(nq);
  if (mt) {
    HIPCHK(hipMemcpyAsync(hsc.data(), dsc, mt, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(hec.data(), dec, mt, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (ng) {
    HIPCHK(hipMemcpyAsync(hfs.data(), dfs, nq, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(hfd.data(), dfd, nq, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(hfl.data(), dfl, sizeof(uint32_t) * nq, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (hashes) HIPCHK(hipMemcpyAsync(hh.data(), D.hash, 32 * m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  // a multisig item: what the fold wrote; the hash is that of the last pair the walk checked, where the reference
  // computes one (check_signature, interpreter.rs:23-30: the push is not empty)
  for (size_t q = 0; q < nq; q++) {
    const size_t i = ms_slot[q];
    status[i] = hfs[q];
    if (detail) detail[i] = hfd[q];
    if (hashes && hfl[q] != MS_NO_PAIR && gsig[row_sig[hfl[q]]].sig_len)
      memcpy(hashes + 32 * i, hh.data() + 32 * (mt + row_sig[hfl[q]]), 32);
  }
  // the interpreter's order: OP_EQUALVERIFY, the encoding check, then the signature check
  for (size_t k = 0; k < mt; k++) {
    const size_t i = P.items[k].slot;
    // the hash the reference computes: check_signature reaches the checker with a key of 33 or 65 bytes and a
    // signature that is not empty (interpreter.rs:18-30), whatever the key and the signature then parse to
    const bool hashed = !(hsc[k] & (SC_F_EQUALVERIFY | SC_F_SIGNATURE_DER)) && srec[k].sig_len &&
                        (srec[k].key_len == 33 || srec[k].key_len == 65);
    status[i] = hsc[k] & SC_F_EQUALVERIFY ? ZG_INPUT_EQUALVERIFY : hsc[k] & SC_F_SIGNATURE_DER ? ZG_INPUT_SIGNATURE_DER
              : hec[k] != ZG_ECDSA_OK ? ZG_INPUT_EVAL_FALSE : ZG_INPUT_OK;
    if (detail && status[i] == ZG_INPUT_EVAL_FALSE) detail[i] = hec[k];
    if (hashes && hashed) memcpy(hashes + 32 * i, hh.data() + 32 * k, 32);
  }
  return ZG_OK;
}

// ------------------------------------------------------------------ shielded transactions (zg_shielded.h)
static int pghr13_load_locked(zg_ctx* ctx, const char* json, size_t len);
static bool pghr13_rho(zg_ctx* ctx, size_t n, std::vector<uint8_t>& rho);

// The PGHR13 pipeline over the npd gathered rows where they are, ctx->pghr_chunk at a time as zg_pghr13_verify
// runs it, its scratch in ctx->bn_arena; the statuses stay on the device for the fold. One PGHR13 call in zg_stats.
static int shielded_pghr13(zg_ctx* ctx, size_t npd, const uint8_t* dproofs, const uint8_t* dinputs, uint8_t* dstatus) {
  std::vector<uint8_t> rho;
  if (!pghr13_rho(ctx, npd, rho)) return fail(ctx, ZG_E_INVAL, "getrandom failed");
  bool any_failed = false;
  const size_t chunk = ctx->pghr_chunk;
  for (size_t o = 0; o < npd; o += chunk) {
    const size_t m = npd - o < chunk ? npd - o : chunk;
    bool batch_failed = false;
    const int rc = bn_pghr13_verify(ctx->bn_key, ctx->stream, ctx->side, m, ctx->pghr_straus_b, ctx->pghr_bseg_k,
                                    dproofs + 296 * o, dinputs + 9 * 32 * o, nullptr, rho.data() + 80 * o, dstatus + o,
                                    nullptr, &batch_failed, ctx->bn_arena, &ctx->err, true);
    if (rc != ZG_OK) return rc;
    any_failed = any_failed || batch_failed;
  }
  ctx->stats[8]++;
  if (any_failed) ctx->stats[9]++;
  return ZG_OK;
}

static int shielded_verify(zg_ctx* ctx, size_t ntx, const uint8_t* txs, const uint64_t* tx_off,
                           const uint32_t* tx_branch_id, uint32_t flags, uint8_t* tx_status, uint8_t* status,
                           uint64_t* index, uint8_t* detail, uint8_t* hashes, uint64_t* desc_off, uint8_t* desc_status) {
  if (!ctx || (ntx && (!txs || !tx_off || !tx_branch_id || !tx_status || !status || !index || !detail)) ||
      ntx > (1u << 30) || (desc_status && !desc_off) || (flags & ~(uint32_t)ZG_SHIELDED_PHGR))
    return ZG_E_INVAL;
  if (!offsets_ok(tx_off, ntx, 1ull << 31)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (desc_off) desc_off[0] = 0;
  if (!ntx) return ZG_OK;
  for (int k = 0; k < ZG_NKINDS; k++)
    if (!ctx->vk_loaded[k]) return fail(ctx, ZG_E_NOVK, "zg_shielded_verify needs all three verifying keys loaded");

  ShPlan P;
  sh_plan_txs(P, ntx, txs, tx_off, tx_branch_id, tx_status);
  const uint64_t base0 = tx_off[0];
  ShdPlan Q;
  if (!shd_plan(P.dtx, ntx, txs + base0, tx_status, status, Q))
    return fail(ctx, ZG_E_INVAL, "zg_shielded_verify: more than 2^30 descriptions");
  // with ZG_SHIELDED_PHGR the transactions shd_plan left HOST: a plan of their own (np, npd: no effect on the v4 rows)
  ShpPlan R;
  if ((flags & ZG_SHIELDED_PHGR) && !shp_plan(P.dtx, ntx, Q.desc.size(), Q.ned, status, R))
    return fail(ctx, ZG_E_INVAL, "zg_shielded_verify: more than 2^30 descriptions");
  const size_t ns = Q.stx.size(), nd = Q.desc.size(), nrj = Q.nrj, ncv = Q.ncv();
  const size_t np = R.ptx.size(), npd = R.desc.size(), ned = Q.ned + np, nsh = ns + np;
  for (size_t t = 0; t < ntx; t++) {
    index[t] = 0, detail[t] = 0;
    if (hashes) memset(hashes + 32 * t, 0, 32);
  }
  if (desc_off) shd_desc_offsets(Q, R, ntx, desc_off);
  if (!nsh) return ZG_OK;  // NONE, HOST and transaction errors only: nothing is launched
  // the no-input hash the acceptor computes (accept_transaction.rs:374-387): hashtype 1, no script; the slots of
  // the transactions before v4 follow the v4 transactions'
  P.items.reserve(nsh);
  for (size_t s = 0; s < ns; s++) sh_plan_add(P, ShDevItem{Q.stx[s].tx, ZG_SIGHASH_NO_INPUT, 0, 0, 1, (uint32_t)s, 0});
  for (size_t q = 0; q < np; q++)
    sh_plan_add(P, ShDevItem{R.ptx[q].tx, ZG_SIGHASH_NO_INPUT, 0, 0, 1, (uint32_t)(ns + q), 0});
  sh_plan_finish(P, ntx);
  for (size_t k = 0; k < nsh; k++) {
    const size_t slot = P.items[k].slot;
    (slot < ns ? Q.stx[slot].hash : R.ptx[slot - ns].hash) = (uint32_t)k;
  }

  HIPCHK(hipSetDevice(ctx->device));
  int rc = ZG_OK;
  if (npd && !ctx->bn_key)  // first use: the builtin key, as zg_pghr13_verify
    rc = pghr13_load_locked(ctx, ZG_PGHR13_VK_JSON, strlen(ZG_PGHR13_VK_JSON));
  if (rc) return rc;
  const uint32_t *jj = nullptr, *edc = nullptr;
  if (ns)
    rc = comb_table(ctx, &ctx->dev->jj_comb, sizeof(uint32_t) * ZG_JJ_COMB_WORDS * ZG_JJ_COMB_POINTS, launch_jj_comb,
                    "Jubjub comb tables", &jj);
  if (!rc && ned)
    rc = comb_table(ctx, &ctx->dev->ed_comb, sizeof(uint32_t) * ZG_ED_COMB_WORDS * ZG_ED_COMB_POINTS, launch_ed_comb,
                    "Ed25519 comb table", &edc);
  if (rc) return rc;
  // the context's arena, every part 256-aligned: the plan's records, the Groth16 rows of all descriptions, the
  // value commitments and binding keys, the RedJubjub and Ed25519 rows, the verdicts; then the PHGR plan's records,
  // its PGHR13 rows and verdicts (all empty without ZG_SHIELDED_PHGR)
  const size_t arena_bytes = (size_t)(tx_off[ntx] - base0);
  const size_t pres_bytes = Carve::span(2 * np, 4) + sizeof(uint32_t) * np;
  const size_t own[32] = {sizeof(ShdTx) * ns, sizeof(ShdDesc) * nd, sizeof(uint32_t) * (ns + 1), sizeof(uint32_t) * ns,
                          sizeof(int64_t) * ns, nd, (size_t)SHD_FIELD_BYTES * nd, 192 * nd, 288 * nd, nd, nd, 32 * ncv,
                          32 * ns, ns, 32 * nrj, 64 * nrj, 64 * nrj, nrj, nrj, 32 * ned, 64 * ned, 32 * ned, ned,
                          nd, nd, Carve::span(2 * ns, 4) + sizeof(uint32_t) * ns,
                          sizeof(ShpTx) * np, sizeof(ShpDesc) * npd, (size_t)SHD_PHGR_PROOF_BYTES * npd, 288 * npd, npd,
                          Carve::span(npd, 256) + pres_bytes};
  size_t need = 0;
  for (size_t b : sh_dev_bytes(P, ntx, arena_bytes, 0)) need += Carve::span(b, 256);
  for (size_t b : own) need += Carve::span(b, 256);
  DevArena& A = ctx->shielded_arena;
  HIPCHK(A.reserve(need, ctx->stream));
  ShDev D;
  rc = sh_upload(ctx, [&](auto** p, size_t bytes) {
    using T = typename std::remove_pointer<typename std::remove_pointer<decltype(p)>::type>::type;
    *p = (T*)A.carve<uint8_t>(bytes, 256);  // (no part is empty: sh_dev_bytes)
    return hipSuccess;
  }, P, ntx, txs + base0, arena_bytes, nullptr, 0, D);
  if (rc) return rc;
  size_t part = 0;
  auto carve = [&] { return A.carve<uint8_t>(own[part++], 256); };
  ShdTx* const dstx = (ShdTx*)carve();
  ShdDesc* const ddesc = (ShdDesc*)carve();
  uint32_t* const dcvoff = (uint32_t*)carve();
  uint32_t* const dnsp = (uint32_t*)carve();
  int64_t* const dvb = (int64_t*)carve();
  uint8_t *const dkinds = carve(), *const dfields = carve(), *const dproofs = carve(), *const dinputs = carve();
  uint8_t *const dcodes = carve(), *const dnin = carve(), *const dcvs = carve(), *const dbvk = carve();
  uint8_t *const dbst = carve(), *const drjvk = carve(), *const drjsig = carve(), *const drjmsg = carve();
  uint8_t *const drjgen = carve(), *const drjok = carve(), *const dedpk = carve(), *const dedsig = carve();
  uint8_t *const dedmsg = carve(), *const dedst = carve(), *const dpst = carve(), *const ddst = carve();
  uint8_t* const dres = carve();  // status and detail, a byte each per v4 transaction, then the indices
  uint32_t* const dindex = dres ? (uint32_t*)(dres + Carve::span(2 * ns, 4)) : nullptr;
  ShpTx* const dptx = (ShpTx*)carve();
  ShpDesc* const dpdesc = (ShpDesc*)carve();
  uint8_t *const dpgproofs = carve(), *const dpginputs = carve(), *const dpgst = carve();
  uint8_t* const dpdst = carve();  // the PHGR descriptions' classes, then status, detail and the indices as dres
  uint8_t* const dpres = dpdst ? dpdst + Carve::span(npd, 256) : nullptr;
  uint32_t* const dpindex = dpres ? (uint32_t*)(dpres + Carve::span(2 * np, 4)) : nullptr;
  if (ns) {
    HIPCHK(hipMemcpyAsync(dstx, Q.stx.data(), own[0], hipMemcpyHostToDevice, ctx->stream));
    if (nd) HIPCHK(hipMemcpyAsync(ddesc, Q.desc.data(), own[1], hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dcvoff, Q.cv_off.data(), own[2], hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dnsp, Q.nspend.data(), own[3], hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dvb, Q.vb.data(), own[4], hipMemcpyHostToDevice, ctx->stream));
  }
  if (np) {
    HIPCHK(hipMemcpyAsync(dptx, R.ptx.data(), own[26], hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dpdesc, R.desc.data(), own[27], hipMemcpyHostToDevice, ctx->stream));
  }
  // everything outside the proof pipelines before them: the gathers, the preparation, the hashes, the binding keys,
  // the rows, the signatures (one Ed25519 launch: the rows of the transactions before v4 follow the v4 ones')
  HIPCHK(sig_timed(ctx, [&] {
    hipError_t e = hipSuccess;
    if (ns) e = launch_shd_gather(ctx->stream, D.arena, D.txs, dstx, ddesc, (int)nd, dkinds, dfields, dproofs, dinputs,
                                  dcodes, dcvs);
    if (e == hipSuccess && nd) e = launch_prep_sapling(ctx->stream, dkinds, dfields, (int)nd, dinputs, dcodes);
    if (e == hipSuccess) e = launch_shp_gather(ctx->stream, D.arena, D.txs, dptx, dpdesc, (int)npd, dpgproofs, dpginputs);
    if (e == hipSuccess) e = sh_launch(ctx, P, D);
    if (e == hipSuccess && ns) e = launch_sapling_bvk(ctx->stream, (int)ns, dcvoff, dnsp, dcvs, dvb, jj, dbvk, dbst);
    if (e == hipSuccess && ns)
      e = launch_shd_rows(ctx->stream, D.arena, D.txs, dstx, (int)ns, ddesc, (int)nd, dcodes, D.hash, dbvk, dnin, drjvk,
                          drjsig, drjmsg, drjgen, dedpk, dedsig, dedmsg);
    if (e == hipSuccess) e = launch_shp_rows(ctx->stream, D.arena, D.txs, dptx, (int)np, D.hash, dedpk, dedsig, dedmsg);
    if (e == hipSuccess && ns) e = launch_redjubjub(ctx->stream, drjvk, drjsig, drjmsg, drjgen, (int)nrj, jj, drjok);
    if (e == hipSuccess && ned) e = launch_ed25519(ctx->stream, dedpk, dedsig, dedmsg, (int)ned, edc, dedst);
    return e;
  }));
  // the context's own batch pipeline over the rows where they are, max_batch at a time; its statuses go back for
  // the fold (a status does not depend on how the rows are grouped into batches)
  std::vector<uint8_t> pst(nd + 1);
  for (size_t o = 0; o < nd; o += ctx->cap) {
    const size_t m = nd - o < ctx->cap ? nd - o : ctx->cap;
    rc = batch_verify_device_locked(ctx, m, dproofs + 192 * o, dkinds + o, dinputs + 288 * o, dnin + o, &pst[o]);
    if (rc) return rc;
  }
  // the PGHR13 pipeline over its rows where they are; its statuses stay on the device for the fold
  if (npd) {
    rc = shielded_pghr13(ctx, npd, dpgproofs, dpginputs, dpgst);
    if (rc) return rc;
  }
  float ms_before = 0.0f;
  HIPCHK(hipEventSynchronize(ctx->sig_ev[1]));
  HIPCHK(hipEventElapsedTime(&ms_before, ctx->sig_ev[0], ctx->sig_ev[1]));
  if (nd) HIPCHK(hipMemcpyAsync(dpst, pst.data(), nd, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(sig_timed(ctx, [&] {
    hipError_t e = hipSuccess;
    if (ns) e = launch_shd_fold(ctx->stream, D.txs, dstx, (int)ns, ddesc, (int)nd, dcodes, drjok, dpst, dedst, dbst, ddst,
                                dres, dindex, dres + ns);
    if (e == hipSuccess)
      e = launch_shp_fold(ctx->stream, D.txs, dptx, (int)np, dpgst, dedst, dpdst, dpres, dpindex, dpres + np);
    return e;
  }));
  // one download per plan: the parts from the descriptions' statuses to the indices lie one after another in the arena
  const size_t res_bytes = Carve::span(2 * ns, 4) + sizeof(uint32_t) * ns, dst_span = Carve::span(nd, 256);
  std::vector<uint8_t> back(dst_span + res_bytes), hh(hashes ? 32 * nsh : 0), pback(np ? own[31] : 0);
  const uint8_t* const from = nd ? ddst : dres;
  const size_t skip = nd ? dst_span : 0;
  if (ns) HIPCHK(hipMemcpyAsync(back.data(), from, skip + res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (np) HIPCHK(hipMemcpyAsync(pback.data(), dpdst, own[31], hipMemcpyDeviceToHost, ctx->stream));
  if (hashes) HIPCHK(hipMemcpyAsync(hh.data(), D.hash, 32 * nsh, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  ctx->sig_ms += ms_before;
  const uint8_t* res = back.data() + skip;
  for (size_t s = 0; s < ns; s++) {
    const size_t t = Q.stx[s].tx;
    uint32_t ix;
    memcpy(&ix, res + Carve::span(2 * ns, 4) + 4 * s, 4);
    status[t] = res[s], detail[t] = res[ns + s], index[t] = ix;
    if (hashes) memcpy(hashes + 32 * t, hh.data() + 32 * Q.stx[s].hash, 32);
  }
  const uint8_t* pres = pback.data() + Carve::span(npd, 256);
  for (size_t q = 0; q < np; q++) {
    const size_t t = R.ptx[q].tx;
    uint32_t ix;
    memcpy(&ix, pres + Carve::span(2 * np, 4) + 4 * q, 4);
    status[t] = pres[q], detail[t] = pres[np + q], index[t] = ix;
    if (hashes) memcpy(hashes + 32 * t, hh.data() + 32 * R.ptx[q].hash, 32);
  }
  if (desc_status && nd && !np) memcpy(desc_status, back.data(), nd);
  if (desc_status && np) {  // both plans: each transaction's descriptions to their place in the window's order
    for (size_t s = 0; s < ns; s++) {
      const size_t t = Q.stx[s].tx;
      memcpy(desc_status + desc_off[t], back.data() + Q.stx[s].desc0, (size_t)(desc_off[t + 1] - desc_off[t]));
    }
    for (size_t q = 0; q < np; q++) {
      const size_t t = R.ptx[q].tx;
      memcpy(desc_status + desc_off[t], pback.data() + R.ptx[q].desc0, (size_t)(desc_off[t + 1] - desc_off[t]));
    }
  }
  return ZG_OK;
}

extern "C" int zg_shielded_verify(zg_ctx* ctx, size_t ntx, const uint8_t* txs, const uint64_t* tx_off,
                                  const uint32_t* tx_branch_id, uint8_t* tx_status, uint8_t* status, uint64_t* index,
                                  uint8_t* detail, uint8_t* hashes, uint64_t* desc_off, uint8_t* desc_status) {
  return shielded_verify(ctx, ntx, txs, tx_off, tx_branch_id, 0, tx_status, status, index, detail, hashes, desc_off,
                         desc_status);
}

extern "C" int zg_shielded_verify_flags(zg_ctx* ctx, size_t ntx, const uint8_t* txs, const uint64_t* tx_off,
                                        const uint32_t* tx_branch_id, uint32_t flags, uint8_t* tx_status,
                                        uint8_t* status, uint64_t* index, uint8_t* detail, uint8_t* hashes,
                                        uint64_t* desc_off, uint8_t* desc_status) {
  return shielded_verify(ctx, ntx, txs, tx_off, tx_branch_id, flags, tx_status, status, index, detail, hashes, desc_off,
                         desc_status);
}

// ------------------------------------------------------------------ block bodies (zg_blocks.h)
// The slices of one call: the kernel's, longest first (a wave's lanes then run similar lengths and the
// longest chains start first), and those of at least ZG_TXID_HOST_MIN bytes, which host threads hash beside it
struct TxidPlan {
  std::vector<TxidSlice> dev, host;
};
static void txid_plan(const zg_ctx* ctx, const std::vector<TxidSlice>& all, TxidPlan& P) {
  for (const TxidSlice& s : all) (ctx->txid_host_min && s.len >= ctx->txid_host_min ? P.host : P.dev).push_back(s);
  std::stable_sort(P.dev.begin(), P.dev.end(), [](const TxidSlice& a, const TxidSlice& b) { return a.len > b.len; });
}
// rows[32 k ..]: the hash of hs[k], by the kernel's routine on up to 16 threads (each slice copied under the
// arena rule of zg_blocks.h: the caller's buffer is neither aligned nor padded)
static void txid_host_rows(const uint8_t* arena, const std::vector<TxidSlice>& hs, std::vector<uint8_t>& rows) {
  rows.assign(32 * hs.size() + 1, 0);
  host_threads(host_nt(hs.size()), [&](size_t t, size_t nt) {
    TxidArena tmp;
    for (size_t k = t; k < hs.size(); k += nt) txid_hash_bytes(arena + hs[k].off, hs[k].len, tmp, &rows[32 * k]);
  });
}

extern "C" int zg_txids(zg_ctx* ctx, size_t n, const uint8_t* arena, const uint64_t* off, uint8_t* hashes) {
  if (!ctx || (n && (!arena || !off || !hashes)) || n > (1u << 30)) return ZG_E_INVAL;
  if (!offsets_ok(off, n, 1ull << 31)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!n) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const uint64_t base0 = off[0];
  const size_t bytes = (size_t)(off[n] - base0);
  std::vector<TxidSlice> all(n);
  for (size_t i = 0; i < n; i++) all[i] = TxidSlice{(uint32_t)(off[i] - base0), (uint32_t)(off[i + 1] - off[i]), (uint32_t)i, 0};
  TxidPlan P;
  txid_plan(ctx, all, P);
  DevScratch s;
  uint8_t *darena, *dids;
  TxidSlice* dsl;
  HIPCHK(s.alloc(&darena, txid_arena_bytes(bytes)));
  HIPCHK(s.alloc(&dids, 32 * n));
  HIPCHK(s.alloc(&dsl, sizeof(TxidSlice) * (P.dev.size() + 1)));
  if (bytes) HIPCHK(hipMemcpyAsync(darena, arena + base0, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (!P.dev.empty())
    HIPCHK(hipMemcpyAsync(dsl, P.dev.data(), sizeof(TxidSlice) * P.dev.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(sig_timed(ctx, [&] { return launch_txid(ctx->stream, darena, dsl, (int)P.dev.size(), dids); }));
  std::vector<uint8_t> hrows;
  txid_host_rows(arena + base0, P.host, hrows);  // while the kernel runs
  HIPCHK(hipMemcpyAsync(hashes, dids, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  for (size_t k = 0; k < P.host.size(); k++) memcpy(hashes + (size_t)32 * P.host[k].slot, &hrows[32 * k], 32);
  return ZG_OK;
}

extern "C" int zg_blocks_verify(zg_ctx* ctx, size_t nblk, const uint8_t* blocks, const uint64_t* blk_off,
                                uint64_t max_block_size, uint64_t max_block_sigops, size_t txid_cap, uint8_t* status,
                                uint8_t* flags, uint64_t* detail, uint8_t* roots, uint64_t* tx_count, uint8_t* txids) {
  if (!ctx || (nblk && (!blocks || !blk_off || !status || !tx_count)) || nblk > (1u << 20)) return ZG_E_INVAL;
  if (!offsets_ok(blk_off, nblk, 1ull << 31)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (tx_count) tx_count[0] = 0;
  if (!nblk) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const uint64_t base0 = blk_off[0];
  const size_t bytes = (size_t)(blk_off[nblk] - base0);
  DevScratch s;
  uint8_t* darena;
  HIPCHK(s.alloc(&darena, txid_arena_bytes(bytes)));
  if (bytes) HIPCHK(hipMemcpyAsync(darena, blocks + base0, bytes, hipMemcpyHostToDevice, ctx->stream));

  // the layouts, on host threads while the arena travels: every offset a lane follows is checked here
  std::vector<BlockLayout> B(nblk);
  std::vector<uint32_t> pst(nblk);
  {
    std::atomic<size_t> next{0};
    host_threads(host_nt(nblk), [&](size_t, size_t) {
      for (size_t b; (b = next.fetch_add(1)) < nblk;)
        pst[b] = block_layout(blocks + blk_off[b], (size_t)(blk_off[b + 1] - blk_off[b]), B[b]);
    });
  }
  std::vector<uint32_t> hb;  // the blocks that are hashed: parsed, canonical, not empty
  for (size_t b = 0; b < nblk; b++) {
    const bool hashed = pst[b] == ZG_TXP_OK && B[b].n_tx > 0;
    if (hashed) hb.push_back((uint32_t)b);
    tx_count[b + 1] = tx_count[b] + (hashed ? B[b].n_tx : 0);
  }
  const size_t total = (size_t)tx_count[nblk];
  if (txids && total > txid_cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return fail(ctx, ZG_E_NOMEM, "zg_blocks_verify: the window holds more transactions than txid_cap");
  }

  std::vector<uint8_t> ids(32 * total + 1), hroots(32 * hb.size() + 1), hmatch(hb.size() + 1), hrows;
  if (total) {
    std::vector<TxidSlice> all;
    std::vector<MerkleBlk> mb;
    all.reserve(total);
    for (uint32_t b : hb) {
      const uint32_t o = (uint32_t)(blk_off[b] - base0);
      mb.push_back(MerkleBlk{o, (uint32_t)tx_count[b], (uint32_t)B[b].n_tx, 0});
      for (size_t t = 0; t < B[b].n_tx; t++)
        all.push_back(TxidSlice{o + (uint32_t)B[b].tx_off[t], (uint32_t)(B[b].tx_off[t + 1] - B[b].tx_off[t]),
                                (uint32_t)(tx_count[b] + t), 0});
    }
    TxidPlan P;
    txid_plan(ctx, all, P);
    uint8_t *dids, *dping, *dpong, *droots, *dmatch;
    TxidSlice* dsl;
    MerkleBlk* dmb;
    HIPCHK(s.alloc(&dids, 32 * total));
    HIPCHK(s.alloc(&dping, 32 * total));
    HIPCHK(s.alloc(&dpong, 32 * total));
    HIPCHK(s.alloc(&droots, 32 * mb.size()));
    HIPCHK(s.alloc(&dmatch, mb.size()));
    HIPCHK(s.alloc(&dsl, sizeof(TxidSlice) * (P.dev.size() + 1)));
    HIPCHK(s.alloc(&dmb, sizeof(MerkleBlk) * mb.size()));
    if (!P.dev.empty())
      HIPCHK(hipMemcpyAsync(dsl, P.dev.data(), sizeof(TxidSlice) * P.dev.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dmb, mb.data(), sizeof(MerkleBlk) * mb.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(sig_timed(ctx, [&] {
      hipError_t e = launch_txid(ctx->stream, darena, dsl, (int)P.dev.size(), dids);
      if (e != hipSuccess) return e;
      if (!P.host.empty()) {  // the host's share while k_txid runs; its rows join the kernel's before the trees
        txid_host_rows(blocks + base0, P.host, hrows);
        for (size_t k = 0; k < P.host.size() && e == hipSuccess; k++)
          e = hipMemcpyAsync(dids + (size_t)32 * P.host[k].slot, &hrows[32 * k], 32, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
      }
      return launch_block_merkle(ctx->stream, darena, dmb, (int)mb.size(), dids, dping, dpong, droots, dmatch);
    }));
    HIPCHK(hipMemcpyAsync(ids.data(), dids, 32 * total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(hroots.data(), droots, 32 * mb.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(hmatch.data(), dmatch, mb.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(sig_sync(ctx));
  } else {
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  if (txids && total) memcpy(txids, ids.data(), 32 * total);

  // BlockVerifier::check's order (verify_block.rs:31-40); uniqueness from the ids, on the host
  size_t h = 0;
  std::vector<std::array<uint8_t, 32>> set;
  for (size_t b = 0; b < nblk; b++) {
    if (roots) memset(roots + 32 * b, 0, 32);
    if (flags) flags[b] = 0;
    if (detail) detail[b] = 0;
    if (pst[b] != ZG_TXP_OK) {
      status[b] = pst[b] == ZG_TXP_MALFORMED ? ZG_BLK_MALFORMED : ZG_BLK_NONCANONICAL;
      continue;
    }
    const BlockLayout& L = B[b];
    uint32_t f = 0;
    if (L.n_tx == 0) f |= ZG_BLK_F_EMPTY;
    if (!L.coinbase0) f |= ZG_BLK_F_COINBASE;
    if (L.size > max_block_size) f |= ZG_BLK_F_SIZE;
    if (L.extra_coinbase != BLOCK_NO_INDEX) f |= ZG_BLK_F_EXTRA_COINBASE;
    if (L.sigops > max_block_sigops) f |= ZG_BLK_F_SIGOPS;
    if (L.n_tx) {
      set.resize((size_t)L.n_tx);
      memcpy(set.data(), &ids[32 * (size_t)tx_count[b]], 32 * (size_t)L.n_tx);
      std::sort(set.begin(), set.end());
      if (std::adjacent_find(set.begin(), set.end()) != set.end()) f |= ZG_BLK_F_DUPLICATED;
      if (!hmatch[h]) f |= ZG_BLK_F_MERKLE_ROOT;
      if (roots) memcpy(roots + 32 * b, &hroots[32 * h], 32);
      h++;
    }
    status[b] = f & ZG_BLK_F_EMPTY ? ZG_BLK_EMPTY : f & ZG_BLK_F_COINBASE ? ZG_BLK_COINBASE : f & ZG_BLK_F_SIZE ? ZG_BLK_SIZE
              : f & ZG_BLK_F_EXTRA_COINBASE ? ZG_BLK_EXTRA_COINBASE : f & ZG_BLK_F_DUPLICATED ? ZG_BLK_DUPLICATED
              : f & ZG_BLK_F_SIGOPS ? ZG_BLK_SIGOPS : f & ZG_BLK_F_MERKLE_ROOT ? ZG_BLK_MERKLE_ROOT : ZG_BLK_OK;
    if (flags) flags[b] = (uint8_t)f;
    if (detail) detail[b] = status[b] == ZG_BLK_SIZE ? L.size : status[b] == ZG_BLK_EXTRA_COINBASE ? L.extra_coinbase : 0;
  }
  return ZG_OK;
}

// ------------------------------------------------------------------ block headers (zg_equihash.h)
extern "C" int zg_equihash_verify(zg_ctx* ctx, int params, size_t n, const uint8_t* inputs, size_t input_len,
                                  const uint8_t* solutions, uint8_t* ok, uint8_t* repeated) {
  const size_t sb = (size_t)equihash_solution_bytes(params);
  if (!ctx || !sb || input_len < 1 || input_len > 252 || (n && (!inputs || !solutions || !ok)) || n > (1u << 30))
    return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!n) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  DevScratch s;
  uint8_t *din, *dsol, *dok, *drep;
  HIPCHK(s.up(&din, inputs, input_len * n, ctx->stream));
  HIPCHK(s.up(&dsol, solutions, sb * n, ctx->stream));
  HIPCHK(s.alloc(&dok, n));
  HIPCHK(s.alloc(&drep, n));
  HIPCHK(sig_timed(ctx, [&] {
    return launch_equihash(ctx->stream, params, din, input_len, (int)input_len, dsol, sb, (int)n, dok, drep);
  }));
  HIPCHK(hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, ctx->stream));
  if (repeated) HIPCHK(hipMemcpyAsync(repeated, drep, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  return ZG_OK;
}

extern "C" int zg_headers_verify(zg_ctx* ctx, size_t n, const uint8_t* headers, uint32_t max_bits, uint8_t* status,
                                 uint8_t* hashes, uint8_t* flags) {
  if (!ctx || (n && (!headers || !status)) || n > (1u << 20)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!n) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  DevScratch s;
  uint8_t *dh, *dok, *drep, *dst, *dhash, *dfl;
  HIPCHK(s.up(&dh, headers, (size_t)ZG_HEADER_BYTES * n, ctx->stream));
  HIPCHK(s.alloc(&dok, n));
  HIPCHK(s.alloc(&drep, n));
  HIPCHK(s.alloc(&dst, n));
  HIPCHK(s.alloc(&dhash, 32 * n));
  HIPCHK(s.alloc(&dfl, n));
  HIPCHK(sig_timed(ctx, [&] { return launch_headers(ctx->stream, dh, (int)n, max_bits, dok, drep, dst, dhash, dfl); }));
  HIPCHK(hipMemcpyAsync(status, dst, n, hipMemcpyDeviceToHost, ctx->stream));
  if (hashes) HIPCHK(hipMemcpyAsync(hashes, dhash, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
  if (flags) HIPCHK(hipMemcpyAsync(flags, dfl, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(sig_sync(ctx));
  return ZG_OK;
}

extern "C" int zg_sapling_bvk(zg_ctx* ctx, size_t ntx, const uint32_t* n_spends, const uint32_t* n_outputs,
                              const uint8_t* cvs, const int64_t* value_balance, uint8_t* bvk, uint8_t* status) {
  if (!ctx || (ntx && (!n_spends || !n_outputs || !value_balance || !bvk || !status)) || ntx > (1u << 30))
    return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!ntx) return ZG_OK;
  std::vector<uint32_t> off(ntx + 1, 0);
  for (size_t t = 0; t < ntx; t++) {
    const uint64_t next = (uint64_t)off[t] + n_spends[t] + n_outputs[t];
    if (next > (1u << 30)) return fail(ctx, ZG_E_INVAL, "too many value commitments");
    off[t + 1] = (uint32_t)next;
  }
  if (off[ntx] && !cvs) return ZG_E_INVAL;
  HIPCHK(hipSetDevice(ctx->device));
  const uint32_t* comb = nullptr;
  int rc = comb_table(ctx, &ctx->dev->jj_comb, sizeof(uint32_t) * ZG_JJ_COMB_WORDS * ZG_JJ_COMB_POINTS, launch_jj_comb,
                      "Jubjub comb tables", &comb);
  if (rc) return rc;
  DevScratch s;
  uint32_t *doff, *dns;
  uint8_t *dcv, *dbvk, *dst;
  int64_t* dvb;
  HIPCHK(s.up(&doff, off.data(), sizeof(uint32_t) * (ntx + 1), ctx->stream));
  HIPCHK(s.up(&dns, n_spends, sizeof(uint32_t) * ntx, ctx->stream));
  HIPCHK(s.up(&dcv, cvs, (size_t)32 * off[ntx], ctx->stream));
  HIPCHK(s.up(&dvb, value_balance, sizeof(int64_t) * ntx, ctx->stream));
  HIPCHK(s.alloc(&dbvk, 32 * ntx));
  HIPCHK(s.alloc(&dst, ntx));
  HIPCHK(launch_sapling_bvk(ctx->stream, (int)ntx, doff, dns, dcv, dvb, comb, dbvk, dst));
  HIPCHK(hipMemcpyAsync(bvk, dbvk, 32 * ntx, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(status, dst, ntx, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ZG_OK;
}

extern "C" int zg_jubjub_decode(zg_ctx* ctx, size_t n, const uint8_t* points, uint8_t* status, uint8_t* xy) {
  if (!ctx || (n && (!points || !status)) || n > (1u << 30)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!n) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  DevScratch s;
  uint8_t *dp, *dst, *dxy = nullptr;
  HIPCHK(s.up(&dp, points, 32 * n, ctx->stream));
  HIPCHK(s.alloc(&dst, n));
  if (xy) HIPCHK(s.alloc(&dxy, 64 * n));
  HIPCHK(launch_jj_decode(ctx->stream, dp, (int)n, dst, dxy));
  HIPCHK(hipMemcpyAsync(status, dst, n, hipMemcpyDeviceToHost, ctx->stream));
  if (xy) HIPCHK(hipMemcpyAsync(xy, dxy, 64 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ZG_OK;
}

// ------------------------------------------------------------------ host input preparation
// (zg_prep.h). CPU only: no context, no GPU.
extern "C" int zg_prep_spend(const uint8_t cv[32], const uint8_t anchor[32], const uint8_t nullifier[32],
                             const uint8_t rk[32], uint8_t inputs[7 * 32]) {
  if (!cv || !anchor || !nullifier || !rk || !inputs) return ZG_E_INVAL;
  return prep_spend(cv, anchor, nullifier, rk, inputs);
}

extern "C" int zg_prep_output(const uint8_t cv[32], const uint8_t cmu[32], const uint8_t epk[32],
                              uint8_t inputs[5 * 32]) {
  if (!cv || !cmu || !epk || !inputs) return ZG_E_INVAL;
  return prep_output(cv, cmu, epk, inputs);
}

// A window's preparation in one call: the Sapling descriptions on the GPU (k_prep_sapling, zg_jubjub.hip),
// the JoinSplits on host threads while it runs (BLAKE2b is host code; ~17 us each), then their rows
// over the kernel's. Per description the same results as the single functions above (tests/
// test_gpu_prep_batch.py): a window of 9,609 descriptions took ~380 ms through per-description host
// calls from a Python thread pool (its per-task overhead under the GIL, not the C, was the bound).
extern "C" int zg_prep_batch(zg_ctx* ctx, size_t n, const uint8_t* kinds, const uint8_t* fields, uint8_t* inputs,
                             uint8_t* codes) {
  if (!ctx || (n && (!kinds || !fields || !inputs || !codes)) || n > (1u << 26)) return ZG_E_INVAL;
  std::vector<size_t> js;
  size_t nsap = 0;
  for (size_t i = 0; i < n; i++) {
    if (kinds[i] > ZG_PREP_KIND_JOINSPLIT_BN) return ZG_E_INVAL;
    if (kinds[i] <= ZG_PREP_KIND_OUTPUT)
      nsap++;
    else
      js.push_back(i);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!n) return ZG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (nsap) {  // the context's arena, byte-packed: kinds | fields | rows | codes
    DevArena& a = ctx->prep_arena;
    HIPCHK(a.reserve(n * (2 + ZG_PREP_FIELD_BYTES + 288) + 64, ctx->stream));
    uint8_t* const dk = a.carve<uint8_t>(n, 1);
    uint8_t* const df = a.carve<uint8_t>((size_t)ZG_PREP_FIELD_BYTES * n, 1);
    uint8_t* const din = a.carve<uint8_t>((size_t)288 * n, 1);
    uint8_t* const dc = a.carve<uint8_t>(n, 1);
    HIPCHK(hipMemcpyAsync(dk, kinds, n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(df, fields, (size_t)ZG_PREP_FIELD_BYTES * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_prep_sapling(ctx->stream, dk, df, (int)n, din, dc));
    HIPCHK(hipMemcpyAsync(inputs, din, (size_t)288 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(codes, dc, n, hipMemcpyDeviceToHost, ctx->stream));
  }
  // the JoinSplits meanwhile, into their own rows (written over the copied-back buffer after the sync)
  std::vector<uint8_t> jrows(js.size() * 288, 0);
  auto work = [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      const uint8_t* f = fields + (size_t)ZG_PREP_FIELD_BYTES * js[k];
      uint64_t vo = 0, vn = 0;
      for (int b = 7; b >= 0; b--) {
        vo = (vo << 8) | f[288 + b];
        vn = (vn << 8) | f[296 + b];
      }
      prep_joinsplit_bits(f, f + 32, f + 64, f + 96, f + 128, f + 160, f + 192, f + 224, vo, vn, f + 256,
                          kinds[js[k]] == ZG_PREP_KIND_JOINSPLIT ? 254 : 253, &jrows[288 * k]);
    }
  };
  host_threads(host_nt(js.size() / 64 + 1),
               [&](size_t t, size_t nt) { work(js.size() * t / nt, js.size() * (t + 1) / nt); });
  if (nsap) {
    HIPCHK(hipEventRecord(ctx->ev[13], ctx->stream));
    HIPCHK(wait_event(ctx->ev[13]));
  }
  for (size_t k = 0; k < js.size(); k++) {
    memcpy(inputs + (size_t)288 * js[k], &jrows[288 * k], 288);
    codes[js[k]] = ZG_PREP_OK;
  }
  return ZG_OK;
}

extern "C" int zg_hsig(const uint8_t random_seed[32], const uint8_t nf0[32], const uint8_t nf1[32],
                       const uint8_t pubkey[32], uint8_t out[32]) {
  if (!random_seed || !nf0 || !nf1 || !pubkey || !out) return ZG_E_INVAL;
  prep_hsig(random_seed, nf0, nf1, pubkey, out);
  return ZG_OK;
}

extern "C" int zg_prep_joinsplit(const uint8_t anchor[32], const uint8_t random_seed[32],
                                 const uint8_t nullifiers[64], const uint8_t macs[64],
                                 const uint8_t commitments[64], uint64_t vpub_old, uint64_t vpub_new,
                                 const uint8_t pubkey[32], uint8_t inputs[9 * 32]) {
  if (!anchor || !random_seed || !nullifiers || !macs || !commitments || !pubkey || !inputs) return ZG_E_INVAL;
  prep_joinsplit(anchor, random_seed, nullifiers, nullifiers + 32, macs, macs + 32, commitments, commitments + 32,
                 vpub_old, vpub_new, pubkey, inputs);
  return ZG_OK;
}

extern "C" int zg_prep_joinsplit_bn(const uint8_t anchor[32], const uint8_t random_seed[32],
                                    const uint8_t nullifiers[64], const uint8_t macs[64],
                                    const uint8_t commitments[64], uint64_t vpub_old, uint64_t vpub_new,
                                    const uint8_t pubkey[32], uint8_t inputs[9 * 32]) {
  if (!anchor || !random_seed || !nullifiers || !macs || !commitments || !pubkey || !inputs) return ZG_E_INVAL;
  prep_joinsplit_bits(anchor, random_seed, nullifiers, nullifiers + 32, macs, macs + 32, commitments,
                      commitments + 32, vpub_old, vpub_new, pubkey, 253, inputs);
  return ZG_OK;
}

// ------------------------------------------------------------------ note-commitment trees (zg_merkle.hip)
static zg::MerkleDev* merkle_dev(zg_ctx* ctx) {
  zg_dev* d = ctx->dev;
  std::lock_guard<std::mutex> g(d->mu);
  if (!d->merkle) d->merkle = merkle_dev_new();
  return d->merkle;
}

extern "C" int zg_merkle_combine(zg_ctx* ctx, int kind, size_t n, const uint8_t* left, const uint8_t* right,
                                 const uint8_t* depth, uint8_t* out) {
  if (!ctx || (kind != ZG_TREE_SPROUT && kind != ZG_TREE_SAPLING) || (n && (!left || !right || !out)) ||
      n > (1u << 30))
    return ZG_E_INVAL;
  if (kind == ZG_TREE_SAPLING && depth)
    for (size_t i = 0; i < n; i++)
      if (depth[i] >= 63) return fail(ctx, ZG_E_INVAL, "MerkleTree depth must be < 63");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  return merkle_combine(merkle_dev(ctx), ctx->stream, kind, n, left, right, depth, out, &ctx->err);
}

extern "C" int zg_tree_empty_roots(zg_ctx* ctx, int kind, size_t levels, uint8_t* out) {
  if (!ctx || (kind != ZG_TREE_SPROUT && kind != ZG_TREE_SAPLING) || levels > 64 || (levels && !out))
    return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  return merkle_empty_roots(merkle_dev(ctx), ctx->stream, kind, levels, out, &ctx->err);
}

extern "C" size_t zg_tree_state_max_bytes(int height) { return merkle_state_max_bytes(height); }

static int tree_roots(zg_ctx* ctx, int kind, int height, const uint8_t* state, size_t state_len, size_t n,
                      const void* leaves, int on_device, size_t n_marks, const uint64_t* marks, uint8_t* roots,
                      uint8_t* state_out, size_t* state_out_len, float* kernel_ms) {
  if (!ctx || (kind != ZG_TREE_SPROUT && kind != ZG_TREE_SAPLING) || height < 1 || height > 62 ||
      (n && !leaves) || (n_marks && (!marks || !roots)) || (state_len && !state) || n > (1ull << 40) ||
      n_marks > (1u << 30))
    return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  return merkle_tree_roots(merkle_dev(ctx), ctx->stream, kind, height, state, state_len, n, leaves, on_device,
                           n_marks, marks, roots, state_out, state_out_len, kernel_ms, ctx->tree_arena, &ctx->err);
}

extern "C" int zg_tree_roots(zg_ctx* ctx, int kind, int height, const uint8_t* state, size_t state_len,
                             size_t n_leaves, const uint8_t* leaves, size_t n_marks, const uint64_t* marks,
                             uint8_t* roots, uint8_t* state_out, size_t* state_out_len) {
  return tree_roots(ctx, kind, height, state, state_len, n_leaves, leaves, 0, n_marks, marks, roots, state_out,
                    state_out_len, nullptr);
}

extern "C" int zg_tree_roots_device(zg_ctx* ctx, int kind, int height, const uint8_t* state, size_t state_len,
                                    size_t n_leaves, const void* d_leaves, size_t n_marks, const uint64_t* marks,
                                    uint8_t* roots, uint8_t* state_out, size_t* state_out_len, float* kernel_ms) {
  return tree_roots(ctx, kind, height, state, state_len, n_leaves, d_leaves, 1, n_marks, marks, roots, state_out,
                    state_out_len, kernel_ms);
}

// ------------------------------------------------------------------ PGHR13 Sprout proofs (zg_pghr13.hip)
static zg::BnDev* bn_dev(zg_ctx* ctx) {
  zg_dev* d = ctx->dev;
  std::lock_guard<std::mutex> g(d->mu);
  if (!d->bn) d->bn = bn_dev_new();
  return d->bn;
}

// a key is parsed, prepared into fresh buffers and published in the device cache, then this
// context points at it (other contexts keep theirs); a failed load leaves the context's key as it was
static int pghr13_load_locked(zg_ctx* ctx, const char* json, size_t len) {
  HIPCHK(hipSetDevice(ctx->device));
  const zg::BnKey* k = nullptr;
  zg::BnDev* d = bn_dev(ctx);
  const int rc = bn_load_vk_json(d, ctx->stream, json, len, &k, &ctx->err);
  if (rc == ZG_OK) {
    if (ctx->bn_key) bn_key_release(d, ctx->bn_key);  // the old key goes once no context uses it
    ctx->bn_key = k;
  }
  return rc;
}

extern "C" int zg_pghr13_vk_load_json(zg_ctx* ctx, const char* json, size_t len) {
  if (!ctx || !json) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  return pghr13_load_locked(ctx, json, len);
}

extern "C" int zg_pghr13_vk_load_builtin(zg_ctx* ctx) {
  return zg_pghr13_vk_load_json(ctx, ZG_PGHR13_VK_JSON, strlen(ZG_PGHR13_VK_JSON));
}

// the equality weights rho_2..rho_5 and rho_1 of n proofs (16 bytes each, zg_pghr13.hip ZG_PGHR_RHO_BYTES):
// seeded contexts (tests) derive them, others take them from the OS. -> false: getrandom failed
static bool pghr13_rho(zg_ctx* ctx, size_t n, std::vector<uint8_t>& rho) {
  rho.resize(80 * n);
  if (!ctx->seeded) return os_random(rho.data(), rho.size());
  for (size_t i = 0; i < n; i++) {
    uint8_t h1[64];
    seeded_bytes("zg-pghr13-rho", ctx->seed, i, &rho[80 * i], 64);
    seeded_bytes("zg-pghr13-rho1", ctx->seed, i, h1, 64);
    memcpy(&rho[80 * i + 64], h1, 16);
  }
  return true;
}

extern "C" int zg_pghr13_verify(zg_ctx* ctx, size_t n, const uint8_t* proofs, const uint8_t* inputs,
                                const uint8_t* n_inputs, uint8_t* status, float* kernel_ms) {
  if (!ctx || (n && (!proofs || !inputs || !status)) || n > (1u << 24)) return ZG_E_INVAL;
  if (n_inputs)
    for (size_t i = 0; i < n; i++)
      if (n_inputs[i] > 9) return fail(ctx, ZG_E_INVAL, "at most 9 PGHR13 inputs per proof");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!ctx->bn_key) {  // first use: the builtin key (res/sprout-verifying-key.json)
    int rc = pghr13_load_locked(ctx, ZG_PGHR13_VK_JSON, strlen(ZG_PGHR13_VK_JSON));
    if (rc) return rc;
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (!n) return ZG_OK;
  std::vector<uint8_t> rho;
  if (!pghr13_rho(ctx, n, rho)) return fail(ctx, ZG_E_INVAL, "getrandom failed");
  // one batch check per chunk of at most ctx->pghr_chunk proofs: the call's arena (~27 KB per proof,
  // mostly the b lines) stays bounded at the chunk size however large the caller's window is
  if (kernel_ms) *kernel_ms = 0;
  bool any_failed = false;
  const size_t chunk = ctx->pghr_chunk;
  for (size_t o = 0; o < n; o += chunk) {
    const size_t m = n - o < chunk ? n - o : chunk;
    bool batch_failed = false;
    float ms = 0;
    const int rc = bn_pghr13_verify(ctx->bn_key, ctx->stream, ctx->side, m, ctx->pghr_straus_b, ctx->pghr_bseg_k,
                                    proofs + 296 * o, inputs + 9 * 32 * o, n_inputs ? n_inputs + o : nullptr,
                                    rho.data() + 80 * o, status + o, kernel_ms ? &ms : nullptr, &batch_failed,
                                    ctx->bn_arena, &ctx->err);
    if (rc != ZG_OK) return rc;
    if (kernel_ms) *kernel_ms += ms;
    any_failed = any_failed || batch_failed;
  }
  if (n) {  // once per call, however many chunks it took (include/zg.h zg_stats [8], [9])
    ctx->stats[8]++;
    if (any_failed) ctx->stats[9]++;
  }
  return ZG_OK;
}

extern "C" int zg_pghr13_shape(zg_ctx* ctx, size_t n, int* straus_b, int* bseg_k, size_t* chunk, int* halves,
                               int* p7_side) {
  if (!ctx) return ZG_E_INVAL;
  const size_t first = n < ctx->pghr_chunk ? n : ctx->pghr_chunk;
  int B, K, hv, p7;
  bn_pghr13_shape(first, ctx->pghr_straus_b, ctx->pghr_bseg_k, &B, &K, &hv, &p7);
  if (straus_b) *straus_b = B;
  if (bseg_k) *bseg_k = K;
  if (chunk) *chunk = ctx->pghr_chunk;
  if (halves) *halves = hv;
  if (p7_side) *p7_side = p7;
  return ZG_OK;
}

extern "C" int zg_bn254_pairing(zg_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt) {
  if (!ctx || (n && (!g1 || !g2 || !gt)) || n > (1u << 20)) return ZG_E_INVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  return bn_pairing(ctx->stream, n, g1, g2, gt, &ctx->err);
}
