//! verification/src/gpu/ffi.rs -- the `extern "C"` declarations of include/zg.h, one for one.
//! tests/test_rust_binding.py checks every signature here against the C header (no cargo in
//! the build image, so the binding is verified textually, not compiled there).
#![allow(dead_code)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ZgConfig {
    /// HIP device ordinal (one process per GPU)
    pub device: c_int,
    /// capacity of one batch (proofs); 0 -> 65536
    pub max_batch: u32,
    /// 1: batch scalars from BLAKE2b(seed, i) (tests); 0: OS-random ChaCha20 key per batch
    pub seeded: c_int,
    pub seed: u64,
}

/// opaque batch slot (include/zg.h `zg_ctx`)
#[repr(C)]
pub struct ZgCtx {
    _private: [u8; 0],
}

pub const ZG_KIND_SPEND: u8 = 0;
pub const ZG_KIND_OUTPUT: u8 = 1;
pub const ZG_KIND_SPROUT: u8 = 2;

pub const ZG_STATUS_OK: u8 = 0;
pub const ZG_STATUS_DECODE_INVALID: u8 = 1;
pub const ZG_STATUS_MALFORMED_VK: u8 = 2;
pub const ZG_STATUS_VERIFY_FAILED: u8 = 3;
pub const ZG_STATUS_INPUT_NONCANONICAL: u8 = 4;

pub const ZG_OK: c_int = 0;
pub const ZG_E_INVAL: c_int = -1;
pub const ZG_E_HIP: c_int = -2;
pub const ZG_E_NOVK: c_int = -3;
pub const ZG_E_VK: c_int = -4;
pub const ZG_E_NOMEM: c_int = -5;
pub const ZG_E_STATE: c_int = -6;
pub const ZG_E_TREE_FULL: c_int = -7;
pub const ZG_E_DEBUG: c_int = -8;

pub const ZG_PREP_KIND_SPEND: u8 = 0;
pub const ZG_PREP_KIND_OUTPUT: u8 = 1;
pub const ZG_PREP_KIND_JOINSPLIT: u8 = 2;
pub const ZG_PREP_KIND_JOINSPLIT_BN: u8 = 3;
pub const ZG_PREP_FIELD_BYTES: usize = 304;

pub const ZG_PROOF_BYTES: usize = 192;
pub const ZG_FR_BYTES: usize = 32;
pub const ZG_MAX_INPUTS: usize = 9;
pub const ZG_INPUT_STRIDE: usize = ZG_MAX_INPUTS * ZG_FR_BYTES;
pub const ZG_GT_BYTES: usize = 576;
pub const ZG_R_BYTES: usize = 16;

pub const ZG_GEN_SPEND_AUTH: u8 = 0;
pub const ZG_GEN_BINDING: u8 = 1;
// zg_ed25519_verify statuses: the reference's crypto::Error class of the JoinSplit signature check
pub const ZG_ED_OK: u8 = 0;
pub const ZG_ED_PUBLIC_ENCODING: u8 = 1;
pub const ZG_ED_SIGNATURE_ENCODING: u8 = 2;
pub const ZG_ED_SIGNATURE: u8 = 3;
// zg_ecdsa_verify statuses: keys::Public::verify of a transparent input's signature (Ok(true), Error::InvalidPublic,
// Error::InvalidSignature from from_der_lax, Ok(false)) and the stride of one key in `pubkeys`
pub const ZG_ECDSA_OK: u8 = 0;
pub const ZG_ECDSA_PUBLIC: u8 = 1;
pub const ZG_ECDSA_SIGNATURE_ENCODING: u8 = 2;
pub const ZG_ECDSA_SIGNATURE: u8 = 3;
pub const ZG_ECDSA_PUBKEY_STRIDE: usize = 65;
// zg_tx_layout / zg_sighash: the parser's verdict on a transaction, an item's status, and the input index
// that stands for the reference's None
pub const ZG_TX_OK: u8 = 0;
pub const ZG_TX_MALFORMED: u8 = 1;
pub const ZG_TX_NONCANONICAL: u8 = 2;
pub const ZG_SIGHASH_OK: u8 = 0;
pub const ZG_SIGHASH_TX_MALFORMED: u8 = 1;
pub const ZG_SIGHASH_TX_NONCANONICAL: u8 = 2;
pub const ZG_SIGHASH_INPUT_RANGE: u8 = 3;
pub const ZG_SIGHASH_NO_INPUT: u32 = 0xFFFF_FFFF;
// zg_script_class / zg_inputs_verify: the template of a (script_sig, script_pubkey) pair, the one script flag a
// template run reads, and an item's status (the interpreter's error, or why there is no verdict)
pub const ZG_SCRIPT_HOST: u8 = 0;
pub const ZG_SCRIPT_P2PKH: u8 = 1;
pub const ZG_SCRIPT_P2PK: u8 = 2;
pub const ZG_SCRIPT_MULTISIG: u8 = 3;
pub const ZG_SCRIPT_P2SH_MULTISIG: u8 = 4;
pub const ZG_SCRIPT_VERIFY_DERSIG: u32 = 1;
pub const ZG_SCRIPT_TEMPLATE_MULTISIG: u32 = 256;
pub const ZG_INPUT_OK: u8 = 0;
pub const ZG_INPUT_EQUALVERIFY: u8 = 1;
pub const ZG_INPUT_SIGNATURE_DER: u8 = 2;
pub const ZG_INPUT_EVAL_FALSE: u8 = 3;
pub const ZG_INPUT_HOST: u8 = 4;
pub const ZG_INPUT_TX_MALFORMED: u8 = 5;
pub const ZG_INPUT_TX_NONCANONICAL: u8 = 6;
pub const ZG_INPUT_RANGE: u8 = 7;
// zg_shielded_verify: a transaction's status (the reference's first error, or why there is no verdict) and the
// inner error class (also a description's own first failing class)
pub const ZG_SHTX_OK: u8 = 0;
pub const ZG_SHTX_NONE: u8 = 1;
pub const ZG_SHTX_JOINSPLIT_SIGNATURE: u8 = 2;
pub const ZG_SHTX_INVALID_JOINSPLIT: u8 = 3;
pub const ZG_SHTX_INVALID_SAPLING: u8 = 4;
pub const ZG_SHTX_HOST: u8 = 5;
pub const ZG_SHTX_TX_MALFORMED: u8 = 6;
pub const ZG_SHTX_TX_NONCANONICAL: u8 = 7;
pub const ZG_SHD_OK: u8 = 0;
pub const ZG_SHD_VALUE_COMMITMENT_INVALID: u8 = 1;
pub const ZG_SHD_VALUE_COMMITMENT_SMALL_ORDER: u8 = 2;
pub const ZG_SHD_ANCHOR: u8 = 3;
pub const ZG_SHD_RANDOMIZED_KEY_INVALID: u8 = 4;
pub const ZG_SHD_RANDOMIZED_KEY_SMALL_ORDER: u8 = 5;
pub const ZG_SHD_NOTE_COMMITMENT: u8 = 6;
pub const ZG_SHD_EPHEMERAL_KEY_INVALID: u8 = 7;
pub const ZG_SHD_EPHEMERAL_KEY_SMALL_ORDER: u8 = 8;
pub const ZG_SHD_SPEND_AUTH_SIG: u8 = 9;
pub const ZG_SHD_PROOF_INVALID: u8 = 10;
pub const ZG_SHD_PROOF_SYNTHESIS: u8 = 11;
pub const ZG_SHD_PROOF_FAILED: u8 = 12;
pub const ZG_SHD_BALANCE_VALUE: u8 = 13;
pub const ZG_SHD_BINDING_SIGNATURE: u8 = 14;
pub const ZG_SHD_JOINSPLIT_ENCODING: u8 = 15;
pub const ZG_SHD_JOINSPLIT_PROOF: u8 = 16;
pub const ZG_SHD_ED_PUBLIC_ENCODING: u8 = 17;
pub const ZG_SHD_ED_SIGNATURE_ENCODING: u8 = 18;
pub const ZG_SHD_ED_SIGNATURE: u8 = 19;
pub const ZG_SHD_JOINSPLIT_PGHR_PROOF: u8 = 20;
// zg_shielded_verify_flags: v2 / v3 transactions with PHGR JoinSplits are checked in the call
pub const ZG_SHIELDED_PHGR: u32 = 1;
// zg_blocks_verify: the first failing check of BlockVerifier::check (after the parser's two verdicts), and
// the flags of every check that fails
pub const ZG_BLK_OK: u8 = 0;
pub const ZG_BLK_MALFORMED: u8 = 1;
pub const ZG_BLK_NONCANONICAL: u8 = 2;
pub const ZG_BLK_EMPTY: u8 = 3;
pub const ZG_BLK_COINBASE: u8 = 4;
pub const ZG_BLK_SIZE: u8 = 5;
pub const ZG_BLK_EXTRA_COINBASE: u8 = 6;
pub const ZG_BLK_DUPLICATED: u8 = 7;
pub const ZG_BLK_SIGOPS: u8 = 8;
pub const ZG_BLK_MERKLE_ROOT: u8 = 9;
pub const ZG_BLK_F_EMPTY: u8 = 1;
pub const ZG_BLK_F_COINBASE: u8 = 2;
pub const ZG_BLK_F_SIZE: u8 = 4;
pub const ZG_BLK_F_EXTRA_COINBASE: u8 = 8;
pub const ZG_BLK_F_DUPLICATED: u8 = 16;
pub const ZG_BLK_F_SIGOPS: u8 = 32;
pub const ZG_BLK_F_MERKLE_ROOT: u8 = 64;
// zg_equihash_verify instances, zg_headers_verify statuses (the first failing check) and flags (every check)
pub const ZG_EQ_200_9: c_int = 0;
pub const ZG_EQ_96_5: c_int = 1;
pub const ZG_EQ_48_5: c_int = 2;
pub const ZG_HEADER_BYTES: usize = 1487;
pub const ZG_HDR_OK: u8 = 0;
pub const ZG_HDR_MALFORMED: u8 = 1;
pub const ZG_HDR_EQUIHASH: u8 = 2;
pub const ZG_HDR_POW: u8 = 3;
pub const ZG_HDR_F_EQUIHASH: u8 = 1;
pub const ZG_HDR_F_POW: u8 = 2;
pub const ZG_HDR_F_REPEATED: u8 = 4;
pub const ZG_TREE_SPROUT: c_int = 0;
pub const ZG_TREE_SAPLING: c_int = 1;

pub const ZG_PREP_OK: c_int = 0;
pub const ZG_PREP_VALUE_COMMITMENT_INVALID: c_int = 1;
pub const ZG_PREP_VALUE_COMMITMENT_SMALL_ORDER: c_int = 2;
pub const ZG_PREP_ANCHOR: c_int = 3;
pub const ZG_PREP_RANDOMIZED_KEY_INVALID: c_int = 4;
pub const ZG_PREP_RANDOMIZED_KEY_SMALL_ORDER: c_int = 5;
pub const ZG_PREP_NOTE_COMMITMENT: c_int = 6;
pub const ZG_PREP_EPHEMERAL_KEY_INVALID: c_int = 7;
pub const ZG_PREP_EPHEMERAL_KEY_SMALL_ORDER: c_int = 8;

#[link(name = "zg")]
extern "C" {
    pub fn zg_create(cfg: *const ZgConfig) -> *mut ZgCtx;
    pub fn zg_destroy(ctx: *mut ZgCtx);
    pub fn zg_last_error(ctx: *mut ZgCtx) -> *const c_char;
    pub fn zg_version() -> *const c_char;

    pub fn zg_vk_load_builtin(ctx: *mut ZgCtx, kind: c_int) -> c_int;
    pub fn zg_vk_load_json(ctx: *mut ZgCtx, kind: c_int, json: *const c_char, len: usize) -> c_int;
    pub fn zg_vk_load_uncompressed(ctx: *mut ZgCtx, kind: c_int, alpha_g1: *const u8, beta_g1: *const u8,
                                   beta_g2: *const u8, gamma_g2: *const u8, delta_g1: *const u8,
                                   delta_g2: *const u8, n_ic: usize, ic: *const u8) -> c_int;
    pub fn zg_vk_alpha_beta(ctx: *mut ZgCtx, kind: c_int, gt: *mut u8) -> c_int;

    pub fn zg_verify_one_gt(ctx: *mut ZgCtx, kind: c_int, proof: *const u8, inputs: *const u8, n_inputs: usize,
                            status: *mut u8, gt: *mut u8) -> c_int;
    pub fn zg_verify_each(ctx: *mut ZgCtx, n: usize, proofs: *const u8, kinds: *const u8, inputs: *const u8,
                          n_inputs: *const u8, status: *mut u8, gts: *mut u8) -> c_int;
    pub fn zg_verify_batch(ctx: *mut ZgCtx, n: usize, proofs: *const u8, kinds: *const u8, inputs: *const u8,
                           n_inputs: *const u8, r: *const u8, status: *mut u8, gt_out: *mut u8) -> c_int;

    pub fn zg_batch_begin(ctx: *mut ZgCtx, n: usize, proofs: *const u8, kinds: *const u8, inputs: *const u8,
                          n_inputs: *const u8, r: *const u8) -> c_int;
    pub fn zg_batch_begin_device(ctx: *mut ZgCtx, n: usize, d_proofs: *const c_void, d_kinds: *const c_void,
                                 d_inputs: *const c_void, d_n_inputs: *const c_void, d_r: *const c_void) -> c_int;
    pub fn zg_batch_partial(ctx: *mut ZgCtx, partial: *mut u8) -> c_int;
    pub fn zg_batch_ready(ctx: *mut ZgCtx) -> c_int;
    pub fn zg_gt_check(ctx: *mut ZgCtx, count: usize, partials: *const u8, ok: *mut c_int) -> c_int;
    pub fn zg_gt_check_many(ctx: *mut ZgCtx, nsets: usize, counts: *const usize, partials: *const u8,
                            ok: *mut c_int) -> c_int;
    pub fn zg_batch_finish(ctx: *mut ZgCtx, batch_ok: c_int, status: *mut u8) -> c_int;
    pub fn zg_set_priority(ctx: *mut ZgCtx, high: c_int) -> c_int;

    pub fn zg_prep_spend(cv: *const u8, anchor: *const u8, nullifier: *const u8, rk: *const u8,
                         inputs: *mut u8) -> c_int;
    pub fn zg_prep_output(cv: *const u8, cmu: *const u8, epk: *const u8, inputs: *mut u8) -> c_int;
    pub fn zg_prep_joinsplit(anchor: *const u8, random_seed: *const u8, nullifiers: *const u8, macs: *const u8,
                             commitments: *const u8, vpub_old: u64, vpub_new: u64, pubkey: *const u8,
                             inputs: *mut u8) -> c_int;
    pub fn zg_prep_joinsplit_bn(anchor: *const u8, random_seed: *const u8, nullifiers: *const u8, macs: *const u8,
                                commitments: *const u8, vpub_old: u64, vpub_new: u64, pubkey: *const u8,
                                inputs: *mut u8) -> c_int;
    pub fn zg_hsig(random_seed: *const u8, nf0: *const u8, nf1: *const u8, pubkey: *const u8, out: *mut u8) -> c_int;
    pub fn zg_prep_batch(ctx: *mut ZgCtx, n: usize, kinds: *const u8, fields: *const u8, inputs: *mut u8,
                         codes: *mut u8) -> c_int;

    pub fn zg_redjubjub_verify(ctx: *mut ZgCtx, n: usize, vk: *const u8, sig: *const u8, msg: *const u8,
                               gen: *const u8, ok: *mut u8) -> c_int;
    pub fn zg_sapling_bvk(ctx: *mut ZgCtx, ntx: usize, n_spends: *const u32, n_outputs: *const u32, cvs: *const u8,
                          value_balance: *const i64, bvk: *mut u8, status: *mut u8) -> c_int;
    pub fn zg_jubjub_decode(ctx: *mut ZgCtx, n: usize, points: *const u8, status: *mut u8, xy: *mut u8) -> c_int;
    pub fn zg_ed25519_verify(ctx: *mut ZgCtx, n: usize, pubkey: *const u8, sig: *const u8, msg: *const u8,
                             status: *mut u8) -> c_int;
    pub fn zg_ecdsa_verify(ctx: *mut ZgCtx, n: usize, pubkeys: *const u8, pubkey_len: *const u8, sigs: *const u8,
                           sig_off: *const u32, msg: *const u8, status: *mut u8) -> c_int;
    pub fn zg_tx_layout(tx: *const u8, len: usize, out: *mut u64) -> c_int;
    pub fn zg_sighash(ctx: *mut ZgCtx, ntx: usize, txs: *const u8, tx_off: *const u64, tx_branch_id: *const u32,
                      n: usize, item_tx: *const u32, input_index: *const u32, scripts: *const u8,
                      script_off: *const u32, amount: *const u64, hashtype: *const u32, tx_status: *mut u8,
                      hashes: *mut u8, status: *mut u8) -> c_int;
    pub fn zg_script_class(script_sig: *const u8, sig_len: usize, script_pubkey: *const u8, pk_len: usize,
                           out: *mut u64) -> c_int;
    pub fn zg_script_match(script_sig: *const u8, sig_len: usize, script_pubkey: *const u8, pk_len: usize,
                           flags: u32, out: *mut u64) -> c_int;
    pub fn zg_inputs_verify(ctx: *mut ZgCtx, ntx: usize, txs: *const u8, tx_off: *const u64, tx_branch_id: *const u32,
                            n: usize, item_tx: *const u32, input_index: *const u32, prev_scripts: *const u8,
                            prev_off: *const u32, amount: *const u64, flags: u32, tx_status: *mut u8,
                            status: *mut u8, detail: *mut u8, hashes: *mut u8) -> c_int;
    pub fn zg_shielded_verify(ctx: *mut ZgCtx, ntx: usize, txs: *const u8, tx_off: *const u64, tx_branch_id: *const u32,
                              tx_status: *mut u8, status: *mut u8, index: *mut u64, detail: *mut u8, hashes: *mut u8,
                              desc_off: *mut u64, desc_status: *mut u8) -> c_int;
    pub fn zg_shielded_verify_flags(ctx: *mut ZgCtx, ntx: usize, txs: *const u8, tx_off: *const u64,
                                    tx_branch_id: *const u32, flags: u32, tx_status: *mut u8, status: *mut u8,
                                    index: *mut u64, detail: *mut u8, hashes: *mut u8, desc_off: *mut u64,
                                    desc_status: *mut u8) -> c_int;
    pub fn zg_block_layout(block: *const u8, len: usize, out: *mut u64, tx_off: *mut u64, tx_off_cap: usize) -> c_int;
    pub fn zg_txids(ctx: *mut ZgCtx, n: usize, arena: *const u8, off: *const u64, hashes: *mut u8) -> c_int;
    pub fn zg_blocks_verify(ctx: *mut ZgCtx, nblk: usize, blocks: *const u8, blk_off: *const u64,
                            max_block_size: u64, max_block_sigops: u64, txid_cap: usize, status: *mut u8,
                            flags: *mut u8, detail: *mut u64, roots: *mut u8, tx_count: *mut u64,
                            txids: *mut u8) -> c_int;
    pub fn zg_last_sig_kernel_ms(ctx: *mut ZgCtx, ms: *mut f32) -> c_int;
    pub fn zg_equihash_verify(ctx: *mut ZgCtx, params: c_int, n: usize, inputs: *const u8, input_len: usize,
                              solutions: *const u8, ok: *mut u8, repeated: *mut u8) -> c_int;
    pub fn zg_headers_verify(ctx: *mut ZgCtx, n: usize, headers: *const u8, max_bits: u32, status: *mut u8,
                             hashes: *mut u8, flags: *mut u8) -> c_int;
    pub fn zg_pow_valid(max_bits: u32, bits: u32, hash: *const u8) -> c_int;

    pub fn zg_pghr13_vk_load_builtin(ctx: *mut ZgCtx) -> c_int;
    pub fn zg_pghr13_vk_load_json(ctx: *mut ZgCtx, json: *const c_char, len: usize) -> c_int;
    pub fn zg_pghr13_verify(ctx: *mut ZgCtx, n: usize, proofs: *const u8, inputs: *const u8, n_inputs: *const u8,
                            status: *mut u8, kernel_ms: *mut f32) -> c_int;
    pub fn zg_pghr13_shape(ctx: *mut ZgCtx, n: usize, straus_b: *mut c_int, bseg_k: *mut c_int, chunk: *mut usize,
                           halves: *mut c_int, p7_side: *mut c_int) -> c_int;
    pub fn zg_bn254_pairing(ctx: *mut ZgCtx, n: usize, g1: *const u8, g2: *const u8, gt: *mut u8) -> c_int;

    pub fn zg_merkle_combine(ctx: *mut ZgCtx, kind: c_int, n: usize, left: *const u8, right: *const u8,
                             depth: *const u8, out: *mut u8) -> c_int;
    pub fn zg_tree_empty_roots(ctx: *mut ZgCtx, kind: c_int, levels: usize, out: *mut u8) -> c_int;
    pub fn zg_tree_state_max_bytes(height: c_int) -> usize;
    pub fn zg_tree_roots(ctx: *mut ZgCtx, kind: c_int, height: c_int, state: *const u8, state_len: usize,
                         n_leaves: usize, leaves: *const u8, n_marks: usize, marks: *const u64, roots: *mut u8,
                         state_out: *mut u8, state_out_len: *mut usize) -> c_int;
    pub fn zg_tree_roots_device(ctx: *mut ZgCtx, kind: c_int, height: c_int, state: *const u8, state_len: usize,
                                n_leaves: usize, d_leaves: *const c_void, n_marks: usize, marks: *const u64,
                                roots: *mut u8, state_out: *mut u8, state_out_len: *mut usize,
                                kernel_ms: *mut f32) -> c_int;

    pub fn zg_synth_rerandomize(ctx: *mut ZgCtx, n_src: usize, src_proofs: *const u8, src_kinds: *const u8,
                                n: usize, src_index: *const u32, seed: u64, out_proofs: *mut u8) -> c_int;
    pub fn zg_last_timings(ctx: *mut ZgCtx, ms7: *mut f32) -> c_int;
    pub fn zg_last_phase_ms(ctx: *mut ZgCtx, ms: *mut f32, n: usize) -> c_int;
    pub fn zg_stats(ctx: *mut ZgCtx, out: *mut u64, n: usize) -> c_int;
    pub fn zg_chacha20_blocks(ctx: *mut ZgCtx, key: *const u8, nonce: *const u8, counter: u32, nblocks: usize,
                              out: *mut u8) -> c_int;
    pub fn zg_bench_mad_rate(ctx: *mut ZgCtx, macs_per_s: *mut f64) -> c_int;
    pub fn zg_bench_mad_rate_clock(ctx: *mut ZgCtx, macs_per_s: *mut f64, clock_hz: *mut f64) -> c_int;
    pub fn zg_debug_field_mul(device: c_int, field: c_int, n: usize, a: *const u8, b: *const u8, out: *mut u8)
                              -> c_int;
}
