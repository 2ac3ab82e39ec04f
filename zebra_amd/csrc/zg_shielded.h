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
// With ZG_SHIELDED_PHGR (row f18) the v2 / v3 transactions with JoinSplits are planned too, in records of their own
// (ShpTx, ShpDesc, below the v4 routines): their descriptions are the rows of the PGHR13 pipeline, numbered apart
// from the Groth16 rows, and their Ed25519 rows follow the v4 transactions'. Nothing of the v4 plan changes.
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
constexpr uint32_t SHD_KIND_JOINSPLIT_BN = 3;                                        // ZG_PREP_KIND_JOINSPLIT_BN
constexpr uint32_t SHD_JOINSPLIT_PGHR_PROOF = 20, SHD_PHGR = 1;                      // ZG_SHD_*, ZG_SHIELDED_PHGR
constexpr uint32_t SHD_PHGR_JS_BYTES = 1802, SHD_PHGR_PROOF_BYTES = 296;
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

// ------------------------------------------------------------------ PHGR JoinSplits (ZG_SHIELDED_PHGR, row f18)
// What JoinSplitVerification::check and JoinSplitProof::check run for a transaction before v4
// (accept_transaction.rs:575-596,649-657; sprout.rs:34-68, the PHGR branch; crypto/src/pghr13.rs:69-105): the Ed25519
// signature over the no-input hash, then Pghr13Proof::from_raw and verify per description. Such a transaction has no
// Sapling part: no binding row, no value commitments, no RedJubjub rows.
struct ShpDesc {
  uint32_t stx;  // its ShpTx
  uint32_t idx;  // its place among the transaction's JoinSplits; its row in the PGHR13 rows is its own number
};
struct ShpTx {
  uint32_t tx;     // its ShDevTx
  uint32_t desc0;  // its first description (PHGR numbering)
  uint32_t hash;   // the row of its no-input signature hash
  uint32_t ed;     // its Ed25519 row
};

// PHGR description `row`: its 296-byte proof and its nine BN254 inputs, 253 bits each (Input::into_bn_frs), from the
// fields where they lie; the descriptions of a transaction are L.js_size bytes apart
ZG_SH_HD void shp_gather(const uint8_t* arena, const ShDevTx* txs, const ShpTx* ptx, const ShpDesc& d, size_t row,
                         uint8_t* proofs, uint8_t* inputs) {
  const ShDevTx& T = txs[ptx[d.stx].tx];
  const uint8_t* p = arena + T.base + T.L.js_off + (size_t)T.L.js_size * d.idx;
  prep_joinsplit_bits(p + 16, p + 208, p + 48, p + 80, p + 240, p + 272, p + 112, p + 144, p, p + 8,
                      arena + T.base + T.L.jspub_off, 253, inputs + 288 * row);
  shd_copy(proofs + (size_t)SHD_PHGR_PROOF_BYTES * row, p + 304, (int)SHD_PHGR_PROOF_BYTES);
}

// after the signature hashes: the transaction's Ed25519 row over its hash
ZG_SH_HD void shp_tx_rows(const uint8_t* arena, const ShDevTx* txs, const ShpTx& S, const uint8_t* hashes,
                          uint8_t* ed_pk, uint8_t* ed_sig, uint8_t* ed_msg) {
  const ShDevTx& T = txs[S.tx];
  const uint8_t* pub = arena + T.base + T.L.jspub_off;
  shd_copy(ed_pk + (size_t)32 * S.ed, pub, 32);
  shd_copy(ed_sig + (size_t)64 * S.ed, pub + 32, 64);
  shd_copy(ed_msg + (size_t)32 * S.ed, hashes + (size_t)32 * S.hash, 32);
}

// sprout::verify's class from the PGHR13 status: from_raw fails -> InvalidEncoding, verify false -> InvalidPGHRProof.
// ZG_STATUS_INPUT_NONCANONICAL cannot occur (a 253-bit chunk is below r); it would count as the proof's failure
ZG_SH_HD uint32_t shp_desc_status(uint32_t proof) {
  return proof == 0 ? SHD_OK : proof == SHD_ST_DECODE_INVALID ? SHD_JOINSPLIT_ENCODING : SHD_JOINSPLIT_PGHR_PROOF;
}

// The reference's first error of a transaction before v4: the Ed25519 signature, then the JoinSplits in order; there
// the fold stops (no balance value, no binding signature). Writes the classes of its n_js descriptions as it goes.
ZG_SH_HD uint32_t shp_tx_fold(const TxLayout& L, const ShpTx& S, const uint8_t* proof_status, const uint8_t* ed,
                              uint8_t* desc_status, uint32_t* index, uint32_t* detail) {
  uint32_t st = SHTX_OK;
  *index = 0, *detail = SHD_OK;
  if (ed[S.ed]) {
    *detail = SHD_ED_BASE + ed[S.ed];
    st = SHTX_JOINSPLIT_SIGNATURE;
  }
  for (uint32_t j = 0; j < L.n_js; j++) {
    const uint32_t c = shp_desc_status(proof_status[S.desc0 + j]);
    desc_status[S.desc0 + j] = (uint8_t)c;
    if (c && st == SHTX_OK) {
      *detail = c, *index = j;
      st = SHTX_INVALID_JOINSPLIT;
    }
  }
  return st;
}

struct ShpPlan {
  std::vector<ShpTx> ptx;
  std::vector<ShpDesc> desc;
};

// After shd_plan: every transaction it left SHTX_HOST (before v4, with JoinSplits) is planned, OK until the fold says
// otherwise; its Ed25519 row follows the ned rows of the v4 plan. -> false: more than 2^30 descriptions with the
// nd of the v4 plan
inline bool shp_plan(const std::vector<ShDevTx>& dtx, size_t ntx, size_t nd, uint32_t ned, uint8_t* status, ShpPlan& R) {
  for (size_t t = 0; t < ntx; t++) {
    if (status[t] != SHTX_HOST) continue;
    const TxLayout& L = dtx[t].L;
    if (nd + R.desc.size() + (uint64_t)L.n_js > (1u << 30)) return false;
    const uint32_t s = (uint32_t)R.ptx.size();
    R.ptx.push_back(ShpTx{(uint32_t)t, (uint32_t)R.desc.size(), 0, ned + s});
    for (uint32_t j = 0; j < L.n_js; j++) R.desc.push_back(ShpDesc{s, j});
    status[t] = SHTX_OK;
  }
  return true;
}

// desc_off of the window, both plans: the descriptions of transaction t, v4 or before, follow those of t - 1
inline void shd_desc_offsets(const ShdPlan& Q, const ShpPlan& R, size_t ntx, uint64_t* desc_off) {
  const size_t ns = Q.stx.size(), np = R.ptx.size();
  desc_off[0] = 0;
  for (size_t t = 0, s = 0, q = 0; t < ntx; t++) {
    uint64_t n = 0;
    if (s < ns && Q.stx[s].tx == t) {
      n = (s + 1 < ns ? Q.stx[s + 1].desc0 : Q.desc.size()) - Q.stx[s].desc0;
      s++;
    } else if (q < np && R.ptx[q].tx == t) {
      n = (q + 1 < np ? R.ptx[q + 1].desc0 : R.desc.size()) - R.ptx[q].desc0;
      q++;
    }
    desc_off[t + 1] = desc_off[t] + n;
  }
}

}  // namespace zg
