// zg_shielded.h -- the plan, gather, row and fold routines of zg_shielded_verify, as
// host/device code: the kernels of zg_shielded.hip and a host-only build run the same routines. For a v4
// transaction they lay out, from its serialized bytes, what the existing kernels check
//   JoinSplitVerification::check   verification/src/accept_transaction.rs:649-657  the Ed25519 signature
//   JoinSplitProof::check          accept_transaction.rs:575-596 -> sprout::verify  sprout.rs:34-84 (Groth16 branch)
//   SaplingProof::check            accept_transaction.rs:707-714 -> accept_sapling  sapling.rs:75-244
// and fold the verdicts into the reference's first error. The descriptions of a window are numbered JoinSplits,
// spends, outputs, transaction after transaction; description d is row d of the Groth16 batch. The RedJubjub rows
// are the spends' spend_auth_sig checks and one binding_sig check per v4 transaction; the Ed25519 rows one per
// transaction with JoinSplits. Every offset a lane follows comes from a TxLayout that tx_parse validated.
#pragma once
#include <vector>

#include "zg_prep.h"
#include "zg_sighash.h"

namespace zg {

// include/zg.h ZG_SHTX_*
constexpr uint32_t SHTX_OK = 0, SHTX_NONE = 1, SHTX_JOINSPLIT_SIGNATURE = 2, SHTX_INVALID_JOINSPLIT = 3,
                   SHTX_INVALID_SAPLING = 4, SHTX_HOST = 5, SHTX_TX_MALFORMED = 6, SHTX_TX_NONCANONICAL = 7;
// include/zg.h ZG_SHD_*: 1..8 are the PREP_* classes of zg_prep.h
constexpr uint32_t SHD_OK = 0, SHD_SPEND_AUTH_SIG = 9, SHD_PROOF_INVALID = 10, SHD_PROOF_SYNTHESIS = 11,
                   SHD_PROOF_FAILED = 12, SHD_BALANCE_VALUE = 13, SHD_BINDING_SIGNATURE = 14,
                   SHD_JOINSPLIT_ENCODING = 15, SHD_JOINSPLIT_PROOF = 16, SHD_ED_BASE = 16;  // + ZG_ED_* (1..3)
constexpr uint32_t SHD_KIND_SPEND = 0, SHD_KIND_OUTPUT = 1, SHD_KIND_JOINSPLIT = 2;  // ZG_KIND_*, ZG_PREP_KIND_*
constexpr uint32_t SHD_NO_ROW = 0xffffffffu;
constexpr uint32_t SHD_JS_BYTES = 1698, SHD_SPEND_BYTES = 384, SHD_OUTPUT_BYTES = 948, SHD_FIELD_BYTES = 304;
constexpr uint32_t SHD_ST_DECODE_INVALID = 1, SHD_ST_MALFORMED_VK = 2, SHD_ST_VERIFY_FAILED = 3;  // ZG_STATUS_*

// One description
struct ShdDesc {
  uint32_t stx;   // its ShdTx
  uint32_t kind;  // SHD_KIND_*
  uint32_t idx;   // its place in its list
  uint32_t cv;    // spends and outputs: its value commitment's row (k_sapling_bvk reads them)
  uint32_t rj;    // spends: the RedJubjub row of its spend_auth_sig
};

// One v4 transaction
struct ShdTx {
  uint32_t tx;     // its ShDevTx
  uint32_t desc0;  // its first description
  uint32_t hash;   // the row of its no-input signature hash
  uint32_t rj;     // the RedJubjub row of its binding signature
  uint32_t ed;     // the Ed25519 row of its JoinSplit signature, SHD_NO_ROW without JoinSplits
};

ZG_SH_HD void shd_copy(uint8_t* to, const uint8_t* from, int n) {
  for (int b = 0; b < n; b++) to[b] = from[b];
}

// where description d lies in the arena
ZG_SH_HD const uint8_t* shd_desc_at(const uint8_t* arena, const ShDevTx& T, const ShdDesc& d) {
  const uint8_t* tx = arena + T.base;
  return d.kind == SHD_KIND_JOINSPLIT ? tx + T.L.js_off + (size_t)SHD_JS_BYTES * d.idx
         : d.kind == SHD_KIND_SPEND   ? tx + T.L.spend_off + (size_t)SHD_SPEND_BYTES * d.idx
                                      : tx + T.L.sout_off + (size_t)SHD_OUTPUT_BYTES * d.idx;
}

// Description `row`: its kind, its proof, and what its public inputs come from. A spend's (cv, anchor, nullifier,
// rk) and an output's (cv, cmu, epk) are the field row k_prep_sapling takes, as they lie in the transaction; a
// JoinSplit's nine inputs are written here (hSig and the 254-bit packing, zg_prep.h), with code 0: its
// preparation cannot fail.
ZG_SH_HD void shd_gather(const uint8_t* arena, const ShDevTx* txs, const ShdTx* stx, const ShdDesc& d, size_t row,
                         uint8_t* kinds, uint8_t* fields, uint8_t* proofs, uint8_t* inputs, uint8_t* codes,
                         uint8_t* cvs) {
  const ShDevTx& T = txs[stx[d.stx].tx];
  const uint8_t* p = shd_desc_at(arena, T, d);
  kinds[row] = (uint8_t)d.kind;
  if (d.kind == SHD_KIND_JOINSPLIT) {
    // vpub_old 0, vpub_new 8, anchor 16, nullifiers 48, commitments 112, ephemeral_key 176, random_seed 208,
    // macs 240, zkproof 304 (chain/src/join_split.rs:51-66)
    prep_joinsplit_bits(p + 16, p + 208, p + 48, p + 80, p + 240, p + 272, p + 112, p + 144, p, p + 8,
                        arena + T.base + T.L.jspub_off, 254, inputs + 288 * row);
    codes[row] = 0;
    shd_copy(proofs + 192 * row, p + 304, 192);
    return;
  }
  const bool spend = d.kind == SHD_KIND_SPEND;
  shd_copy(fields + (size_t)SHD_FIELD_BYTES * row, p, spend ? 128 : 96);
  shd_copy(cvs + (size_t)32 * d.cv, p, 32);
  shd_copy(proofs + 192 * row, p + (spend ? 128 : SHD_OUTPUT_BYTES - 192), 192);
}

// After the preparation and the signature hashes. Description `row`: the number of inputs its proof is checked
// against, 0 where its preparation failed (the batch then reports ZG_STATUS_MALFORMED_VK for it and leaves it
// out of the product: no other row's status changes); a spend's RedJubjub row, message rk || sighash
ZG_SH_HD void shd_desc_rows(const uint8_t* arena, const ShDevTx* txs, const ShdTx* stx, const ShdDesc& d, size_t row,
                            const uint8_t* codes, const uint8_t* hashes, uint8_t* ninputs, uint8_t* rj_vk,
                            uint8_t* rj_sig, uint8_t* rj_msg, uint8_t* rj_gen) {
  ninputs[row] = codes[row] ? 0 : d.kind == SHD_KIND_JOINSPLIT ? 9 : d.kind == SHD_KIND_SPEND ? 7 : 5;
  if (d.kind != SHD_KIND_SPEND) return;
  const ShdTx& S = stx[d.stx];
  const uint8_t* p = shd_desc_at(arena, txs[S.tx], d);
  shd_copy(rj_vk + (size_t)32 * d.rj, p + 96, 32);
  shd_copy(rj_sig + (size_t)64 * d.rj, p + 320, 64);
  shd_copy(rj_msg + (size_t)64 * d.rj, p + 96, 32);
  shd_copy(rj_msg + (size_t)64 * d.rj + 32, hashes + (size_t)32 * S.hash, 32);
  rj_gen[d.rj] = 0;  // ZG_GEN_SPEND_AUTH
}

// Transaction s, after k_sapling_bvk: its binding row, message bvk || sighash, the signature the transaction
// carries or, without spends and outputs, the reference's default of 64 zero bytes (chain/src/transaction.rs:
// 291-303); its Ed25519 row over the same hash
ZG_SH_HD void shd_tx_rows(const uint8_t* arena, const ShDevTx* txs, const ShdTx& S, size_t s, const uint8_t* hashes,
                          const uint8_t* bvk, uint8_t* rj_vk, uint8_t* rj_sig, uint8_t* rj_msg, uint8_t* rj_gen,
                          uint8_t* ed_pk, uint8_t* ed_sig, uint8_t* ed_msg) {
  const ShDevTx& T = txs[S.tx];
  const uint8_t* tx = arena + T.base;
  const uint8_t* h = hashes + (size_t)32 * S.hash;
  shd_copy(rj_vk + (size_t)32 * S.rj, bvk + 32 * s, 32);
  shd_copy(rj_msg + (size_t)64 * S.rj, bvk + 32 * s, 32);
  shd_copy(rj_msg + (size_t)64 * S.rj + 32, h, 32);
  const bool has_sig = T.L.n_spend || T.L.n_sout;
  const uint8_t* sig = tx + T.L.jspub_off + (T.L.n_js ? 96 : 0);
  for (int b = 0; b < 64; b++) rj_sig[(size_t)64 * S.rj + b] = has_sig ? sig[b] : 0;
  rj_gen[S.rj] = 1;  // ZG_GEN_BINDING
  if (S.ed == SHD_NO_ROW) return;
  shd_copy(ed_pk + (size_t)32 * S.ed, tx + T.L.jspub_off, 32);
  shd_copy(ed_sig + (size_t)64 * S.ed, tx + T.L.jspub_off + 32, 64);
  shd_copy(ed_msg + (size_t)32 * S.ed, h, 32);
}

// A description's own first failing class, whatever happened before it: accept_spend's order is cv, anchor, rk
// (the preparation code), spend_auth_sig, proof; accept_output's cv, cmu, epk, proof; sprout::verify's the proof's
// encoding, then the proof
ZG_SH_HD uint32_t shd_desc_status(const ShdDesc& d, uint32_t code, const uint8_t* rj_ok, uint32_t proof) {
  if (d.kind == SHD_KIND_JOINSPLIT)
    return proof == 0 ? SHD_OK : proof == SHD_ST_DECODE_INVALID ? SHD_JOINSPLIT_ENCODING : SHD_JOINSPLIT_PROOF;
  if (code) return code;
  if (d.kind == SHD_KIND_SPEND && !rj_ok[d.rj]) return SHD_SPEND_AUTH_SIG;
  return proof == 0 ? SHD_OK : proof == SHD_ST_DECODE_INVALID ? SHD_PROOF_INVALID
         : proof == SHD_ST_VERIFY_FAILED ? SHD_PROOF_FAILED : SHD_PROOF_SYNTHESIS;
}

// The reference's first error of transaction s: the Ed25519 signature, the JoinSplits in order, the spends, the
// outputs, the balance value, the binding signature. bvk_st: k_sapling_bvk's (2: the value is i64::MIN; 1, a cv
// that does not decode, has failed its own description before)
ZG_SH_HD uint32_t shd_tx_fold(const TxLayout& L, const ShdTx& S, const uint8_t* desc_status, const uint8_t* ed,
                              const uint8_t* rj_ok, uint32_t bvk_st, uint32_t* index, uint32_t* detail) {
  *index = 0;
  if (S.ed != SHD_NO_ROW && ed[S.ed]) {
    *detail = SHD_ED_BASE + ed[S.ed];
    return SHTX_JOINSPLIT_SIGNATURE;
  }
  const uint8_t* ds = desc_status + S.desc0;
  const uint32_t nd = L.n_js + L.n_spend + L.n_sout;
  for (uint32_t j = 0; j < nd; j++)
    if (ds[j]) {
      *detail = ds[j];
      *index = j < L.n_js ? j : j < L.n_js + L.n_spend ? j - L.n_js : j - L.n_js - L.n_spend;
      return j < L.n_js ? SHTX_INVALID_JOINSPLIT : SHTX_INVALID_SAPLING;
    }
  *detail = bvk_st == 2 ? SHD_BALANCE_VALUE : bvk_st || !rj_ok[S.rj] ? SHD_BINDING_SIGNATURE : SHD_OK;
  return *detail ? SHTX_INVALID_SAPLING : SHTX_OK;
}

// ------------------------------------------------------------------ the plan (host)
struct ShdPlan {
  std::vector<ShdTx> stx;
  std::vector<ShdDesc> desc;
  std::vector<uint32_t> cv_off, nspend;  // k_sapling_bvk's: per v4 transaction its first cv row (+ the end), its spends
  std::vector<int64_t> vb;               // ... and its balancing value
  uint32_t nrj = 0, ned = 0;
  size_t ncv() const { return cv_off.empty() ? 0 : cv_off.back(); }
};

// The class of every transaction of the window from its layout, and the rows of those that are checked here. A
// transaction before v4 has join_split = None when the count is 0 (chain/src/join_split.rs:149-153): NONE; with
// JoinSplits its proofs are PHGR: HOST. A v4 transaction always has sapling = Some: it is planned, OK until the
// fold says otherwise. -> false: more than 2^30 descriptions
inline bool shd_plan(const std::vector<ShDevTx>& dtx, size_t ntx, const uint8_t* arena, const uint8_t* tx_status,
                     uint8_t* status, ShdPlan& P) {
  P.cv_off.assign(1, 0);
  for (size_t t = 0; t < ntx; t++) {
    const TxLayout& L = dtx[t].L;
    status[t] = tx_status[t] == ZG_TXP_MALFORMED ? SHTX_TX_MALFORMED : tx_status[t] == ZG_TXP_NONCANONICAL ? SHTX_TX_NONCANONICAL
              : L.sigver == 2 ? SHTX_OK : L.n_js ? SHTX_HOST : SHTX_NONE;
    if (status[t] != SHTX_OK) continue;
    const uint32_t s = (uint32_t)P.stx.size();
    if (P.desc.size() + (uint64_t)L.n_js + L.n_spend + L.n_sout > (1u << 30)) return false;
    P.stx.push_back(ShdTx{(uint32_t)t, (uint32_t)P.desc.size(), 0, 0, L.n_js ? P.ned++ : SHD_NO_ROW});
    uint32_t cv = P.cv_off.back();
    for (uint32_t j = 0; j < L.n_js; j++) P.desc.push_back(ShdDesc{s, SHD_KIND_JOINSPLIT, j, 0, 0});
    for (uint32_t j = 0; j < L.n_spend; j++) P.desc.push_back(ShdDesc{s, SHD_KIND_SPEND, j, cv++, P.nrj++});
    for (uint32_t j = 0; j < L.n_sout; j++) P.desc.push_back(ShdDesc{s, SHD_KIND_OUTPUT, j, cv++, 0});
    P.cv_off.push_back(cv);
    P.nspend.push_back(L.n_spend);
    uint64_t v = 0;
    for (int b = 7; b >= 0; b--) v = (v << 8) | arena[dtx[t].base + L.value_off + b];
    P.vb.push_back((int64_t)v);
  }
  for (ShdTx& S : P.stx) S.rj = P.nrj++;  // the binding rows follow the spends'
  return true;
}

}  // namespace zg
