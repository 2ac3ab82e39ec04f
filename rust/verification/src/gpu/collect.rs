//! verification/src/gpu/collect.rs -- block-level Groth16 collection with the reference's error
//! precedence (a transcription of zebra_amd/collector.py).
//!
//!   ChainAcceptor::check_transactions  verification/src/accept_chain.rs:76-81
//!       the LOWEST failing tx index wins (rayon fold/reduce)
//!   TransactionAcceptor::check         verification/src/accept_transaction.rs:68-84
//!       ... -> eval -> join_split.check -> sapling.check
//!   JoinSplitVerification::check       accept_transaction.rs:649-657
//!       ed25519 sig -> per description: proof (InvalidJoinSplit(i)), tree root -> nullifiers
//!   SaplingVerification                accept_transaction.rs:700-714
//!       per spend (prep, spend_auth_sig, proof), per output (prep, proof), binding sig
//!       -> InvalidSapling; then nullifiers
//!
//! The checks that are not proofs or Sapling signatures are evaluated by the caller as today and
//! handed in as outcomes; the window's public inputs are prepared in ONE `Backend::prep_batch` call
//! (zg_prep_batch, from 64 descriptions); every Groth16 proof of the window goes through ONE `Backend::verify`
//! call and every PHGR JoinSplit proof (sprout.rs:61-67) through ONE `Backend::pghr13_verify`
//! call. A PHGR failure (InvalidEncoding / InvalidPGHRProof) is InvalidJoinSplit(index) at its
//! place among the descriptions, before that description's tree_cache.continue_root
//! (accept_transaction.rs:575-592).
//!
//! Backends: `GpuVerifier` (the product) and `cpu::CpuBackend` (the reference's own per-proof
//! calls). `verify_block_or_cpu` runs the window on the GPU and, on a GpuError, re-runs the
//! whole window on the CPU backend, so an import never stops on a device fault.
use std::collections::HashMap;
use std::convert::TryInto;
use std::sync::Arc;

use super::cpu::CpuBackend;
use super::{prep_joinsplit, prep_joinsplit_bn, prep_output, prep_spend, GpuError, GpuVerifier, InputItem, Item, SighashItem};
use super::ffi::{ZG_INPUT_EQUALVERIFY, ZG_INPUT_EVAL_FALSE, ZG_INPUT_OK, ZG_INPUT_SIGNATURE_DER, ZG_SCRIPT_VERIFY_DERSIG};
use super::ffi::{ZG_ECDSA_OK, ZG_SIGHASH_OK, ZG_ED_OK, ZG_GEN_BINDING, ZG_GEN_SPEND_AUTH, ZG_PREP_FIELD_BYTES, ZG_PREP_KIND_JOINSPLIT, ZG_PREP_KIND_JOINSPLIT_BN,
                 ZG_PREP_KIND_OUTPUT, ZG_PREP_KIND_SPEND};
use super::{ZG_KIND_OUTPUT, ZG_KIND_SPEND, ZG_KIND_SPROUT, ZG_STATUS_OK};

#[derive(Clone)]
pub struct JoinSplit {
    pub anchor: [u8; 32],
    pub random_seed: [u8; 32],
    pub nullifiers: [[u8; 32]; 2],
    pub macs: [[u8; 32]; 2],
    pub commitments: [[u8; 32]; 2],
    pub vpub_old: u64,
    pub vpub_new: u64,
    /// 192-byte Groth16 proof (v4+); None for a PGHR13 description
    pub groth_proof: Option<[u8; 192]>,
    /// 296-byte PHGR proof of a pre-Sapling description (verified in the window's PGHR13 call)
    pub pghr_proof: Option<[u8; 296]>,
    /// a PGHR13 verdict the caller already holds (overrides pghr_proof)
    pub pghr_ok: Option<bool>,
    /// the caller's tree_cache.continue_root outcome (accept_transaction.rs:589)
    pub tree_error: Option<String>,
}

#[derive(Clone)]
pub struct Spend {
    pub cv: [u8; 32],
    pub anchor: [u8; 32],
    pub nullifier: [u8; 32],
    pub rk: [u8; 32],
    pub zkproof: [u8; 192],
    /// the caller's RedJubjub spend_auth_sig verdict, used when spend_auth_sig is None
    pub sig_ok: bool,
    /// the signature, verified on the GPU when the transaction carries its sighash
    pub spend_auth_sig: Option<[u8; 64]>,
}

#[derive(Clone)]
pub struct Output {
    pub cv: [u8; 32],
    pub cmu: [u8; 32],
    pub epk: [u8; 32],
    pub zkproof: [u8; 192],
}

/// one signature check a script run asked its checker for (TransactionSignatureChecker::
/// verify_signature, script/src/verify.rs:60-67): the key and the DER signature without its hashtype
/// byte as the script pushed them, and the 32-byte sighash of that input
#[derive(Clone)]
pub struct EcdsaCheck {
    pub input_index: usize,
    pub pubkey: Vec<u8>,
    pub sig: Vec<u8>,
    pub sighash: [u8; 32],
}

/// an EcdsaCheck whose sighash is still to be computed: what the checker would pass to
/// TransactionInputSigner::signature_hash (script/src/sign.rs:152-160) -- the script code, the hashtype byte the
/// signature carried and the amount of the output the input spends. Needs Tx::raw
#[derive(Clone)]
pub struct EcdsaRequest {
    pub input_index: usize,
    pub pubkey: Vec<u8>,
    pub sig: Vec<u8>,
    pub script_code: Vec<u8>,
    pub hashtype: u32,
    pub amount: u64,
}

/// the output an input spends: its script and its value
#[derive(Clone)]
pub struct Prevout {
    pub script_pubkey: Vec<u8>,
    pub amount: u64,
}

/// lookup(input_index, pubkey, sig, script_code, hashtype) -> the verdict of a request's check: answerable
/// without the host computing a sighash
pub type RequestLookup<'a> = dyn FnMut(usize, &[u8], &[u8], &[u8], u32) -> Result<bool, GpuError> + 'a;
/// eval_rerun for a transaction that carries ecdsa_requests
pub type EvalRerunRequests = Arc<dyn Fn(&mut RequestLookup) -> Result<Option<TxError>, GpuError> + Send + Sync>;

/// lookup(pubkey, sig, sighash) -> the signature check's verdict
pub type EcdsaLookup<'a> = dyn FnMut(&[u8], &[u8], &[u8; 32]) -> Result<bool, GpuError> + 'a;
/// the caller's second TransactionEval::check (accept_transaction.rs:363-422) with `lookup` as the
/// checker: the reference's eval error, or None
pub type EvalRerun = Arc<dyn Fn(&mut EcdsaLookup) -> Result<Option<TxError>, GpuError> + Send + Sync>;

#[derive(Default, Clone)]
pub struct Tx {
    /// first failing check before the JoinSplit stage (version ... eval)
    pub pre_error: Option<String>,
    pub js_pubkey: Option<[u8; 32]>,
    /// the caller's Ed25519 JoinSplit signature verdict, used when js_sig is None
    pub js_sig_ok: bool,
    pub joinsplits: Vec<JoinSplit>,
    pub js_nullifier_error: Option<String>,
    pub spends: Vec<Spend>,
    pub outputs: Vec<Output>,
    /// the caller's binding_sig verdict, used when binding_sig is None
    pub binding_ok: bool,
    pub sapling_nullifier_error: Option<String>,
    /// the no-input ZIP-243 sighash (accept_transaction.rs:374-386): with it, the spend_auth and
    /// binding signatures are verified on the GPU
    pub sighash: Option<[u8; 32]>,
    pub value_balance: i64,
    pub binding_sig: Option<[u8; 64]>,
    /// the Ed25519 JoinSplit signature over the same sighash (accept_transaction.rs:649-653): with
    /// it (and js_pubkey, sighash) the signature is verified on the GPU instead of js_sig_ok
    pub js_sig: Option<[u8; 64]>,
    /// the transparent inputs' ECDSA checks, recorded by one run of
    /// TransactionEval::check with a checker that answers true: all of the window's are verified in ONE
    /// zg_ecdsa_verify call; if every one of a transaction's is ZG_ECDSA_OK that run was the
    /// reference's run (pre_error then covers only the checks before eval) ...
    pub ecdsa_checks: Vec<EcdsaCheck>,
    /// ... otherwise this repeats the run with the real verdicts and its value is the eval error
    pub eval_rerun: Option<EvalRerun>,
    /// the signature hashes on the GPU: the serialized transaction and its consensus
    /// branch id. With raw set and sighash None, the no-input sighash (hashtype 1) is computed in the window's
    /// ONE sighash call; ecdsa_requests are resolved to ecdsa_checks by the same call, and a transaction that
    /// has requests is re-run through eval_rerun_requests
    pub raw: Option<Vec<u8>>,
    pub branch_id: u32,
    pub ecdsa_requests: Vec<EcdsaRequest>,
    pub eval_rerun_requests: Option<EvalRerunRequests>,
    /// the whole script check of template inputs on the GPU: one Prevout per input, set only
    /// when script_class names every input of the transaction a template (P2PKH or P2PK). Needs raw; ecdsa_checks,
    /// ecdsa_requests and both reruns must then be empty: no interpreter runs for this transaction
    pub prevouts: Option<Vec<Prevout>>,
}

#[derive(Debug, Clone, PartialEq)]
pub enum TxError {
    Caller(String),
    /// TransactionError::Signature(input index, script error) of the eval stage, from eval_rerun
    Signature(usize, String),
    JoinSplitSignature,
    InvalidJoinSplit(usize),
    InvalidSapling,
}

/// What verifies a window: the GPU (`GpuVerifier`) or the reference's CPU calls (`CpuBackend`).
pub trait Backend {
    /// Groth16 statuses (ZG_STATUS_*), one per item, exact per proof
    fn verify(&self, items: &[Item]) -> Result<Vec<u8>, GpuError>;
    /// PGHR13 statuses for (296-byte proof, into_bn_frs inputs)
    fn pghr13_verify(&self, items: &[([u8; 296], Vec<[u8; 32]>)]) -> Result<Vec<u8>, GpuError>;
    /// RedJubjub verdicts for (vk, sig, msg, generator)
    fn redjubjub_verify(&self, items: &[([u8; 32], [u8; 64], [u8; 64], u8)]) -> Result<Vec<bool>, GpuError>;
    /// (status, bvk) per (spend cvs, output cvs, valueBalance)
    fn sapling_bvk(&self, txs: &[(Vec<[u8; 32]>, Vec<[u8; 32]>, i64)]) -> Result<Vec<(u8, [u8; 32])>, GpuError>;
    /// Ed25519 statuses (ZG_ED_*) for (pubkey, signature, 32-byte message)
    fn ed25519_verify(&self, items: &[([u8; 32], [u8; 64], [u8; 32])]) -> Result<Vec<u8>, GpuError>;
    /// ECDSA statuses (ZG_ECDSA_*) for (public key, DER signature, 32-byte sighash)
    fn ecdsa_verify(&self, items: &[(Vec<u8>, Vec<u8>, [u8; 32])]) -> Result<Vec<u8>, GpuError>;
    /// TransactionInputSigner::signature_hash per item over (serialized transaction, branch id) ->
    /// (ZG_TX_* per transaction, hash per item, ZG_SIGHASH_* per item)
    fn sighash(&self, _txs: &[(Vec<u8>, u32)], _items: &[SighashItem]) -> Result<(Vec<u8>, Vec<[u8; 32]>, Vec<u8>), GpuError> {
        Err(GpuError { code: -1, message: "this backend computes no signature hashes".to_string() })
    }
    /// verify_script of template inputs over (serialized transaction, branch id) under `flags` ->
    /// (ZG_TX_* per transaction, ZG_INPUT_* per item, ZG_ECDSA_* detail per item, the hash checked per item)
    fn inputs_verify(&self, _txs: &[(Vec<u8>, u32)], _items: &[InputItem], _flags: u32)
                     -> Result<(Vec<u8>, Vec<u8>, Vec<u8>, Vec<[u8; 32]>), GpuError> {
        Err(GpuError { code: -1, message: "this backend verifies no template inputs".to_string() })
    }
    /// header statuses (ZG_HDR_*: the first failing of deserialize / Equihash / proof of work) for
    /// serialized 1487-byte headers against the compact `max_bits`
    fn headers_verify(&self, headers: &[Vec<u8>], max_bits: u32) -> Result<Vec<u8>, GpuError>;
    /// BlockVerifier::check (verify_block.rs:31-40) over the window's serialized blocks in one call ->
    /// per block (status ZG_BLK_*: the first failing check in the reference's order, the detail word:
    /// the size for ZG_BLK_SIZE, the index for ZG_BLK_EXTRA_COINBASE, the transaction ids in H256
    /// storage order: none for a block that was not hashed)
    fn blocks_verify(&self, blocks: &[Vec<u8>], max_block_size: u64, max_block_sigops: u64)
                     -> Result<Vec<(u8, u64, Vec<[u8; 32]>)>, GpuError>;
    /// a window's public-input preparation in one call (zg_prep_batch: kinds ZG_PREP_KIND_*, fields
    /// n x ZG_PREP_FIELD_BYTES) -> Some((inputs n x 288 B, codes ZG_PREP_*)); None: the backend has no
    /// batched form and the window is prepared with the per-description host functions
    fn prep_batch(&self, _kinds: &[u8], _fields: &[u8]) -> Result<Option<(Vec<u8>, Vec<u8>)>, GpuError> {
        Ok(None)
    }
}

impl Backend for GpuVerifier {
    fn verify(&self, items: &[Item]) -> Result<Vec<u8>, GpuError> {
        GpuVerifier::verify(self, items)
    }
    fn pghr13_verify(&self, items: &[([u8; 296], Vec<[u8; 32]>)]) -> Result<Vec<u8>, GpuError> {
        GpuVerifier::pghr13_verify(self, items)
    }
    fn redjubjub_verify(&self, items: &[([u8; 32], [u8; 64], [u8; 64], u8)]) -> Result<Vec<bool>, GpuError> {
        GpuVerifier::redjubjub_verify(self, items)
    }
    fn sapling_bvk(&self, txs: &[(Vec<[u8; 32]>, Vec<[u8; 32]>, i64)]) -> Result<Vec<(u8, [u8; 32])>, GpuError> {
        GpuVerifier::sapling_bvk(self, txs)
    }
    fn ed25519_verify(&self, items: &[([u8; 32], [u8; 64], [u8; 32])]) -> Result<Vec<u8>, GpuError> {
        GpuVerifier::ed25519_verify(self, items)
    }
    fn ecdsa_verify(&self, items: &[(Vec<u8>, Vec<u8>, [u8; 32])]) -> Result<Vec<u8>, GpuError> {
        GpuVerifier::ecdsa_verify(self, items)
    }
    fn sighash(&self, txs: &[(Vec<u8>, u32)], items: &[SighashItem]) -> Result<(Vec<u8>, Vec<[u8; 32]>, Vec<u8>), GpuError> {
        GpuVerifier::sighash(self, txs, items)
    }
    fn inputs_verify(&self, txs: &[(Vec<u8>, u32)], items: &[InputItem], flags: u32)
                     -> Result<(Vec<u8>, Vec<u8>, Vec<u8>, Vec<[u8; 32]>), GpuError> {
        GpuVerifier::inputs_verify(self, txs, items, flags)
    }
    fn headers_verify(&self, headers: &[Vec<u8>], max_bits: u32) -> Result<Vec<u8>, GpuError> {
        Ok(GpuVerifier::headers_verify(self, headers, max_bits)?.into_iter().map(|r| r.0).collect())
    }
    fn blocks_verify(&self, blocks: &[Vec<u8>], max_block_size: u64, max_block_sigops: u64)
                     -> Result<Vec<(u8, u64, Vec<[u8; 32]>)>, GpuError> {
        GpuVerifier::blocks_verify(self, blocks, max_block_size, max_block_sigops)
    }
    fn prep_batch(&self, kinds: &[u8], fields: &[u8]) -> Result<Option<(Vec<u8>, Vec<u8>)>, GpuError> {
        Ok(Some(GpuVerifier::prep_batch(self, kinds, fields)?))
    }
}

enum Plan {
    Proof(usize),
    Pghr(usize),
    Caller(bool),
    Prep,
}

type Plans = Vec<(Vec<Plan>, Vec<Plan>, Vec<Plan>)>;

/// windows from this many descriptions are prepared in one `Backend::prep_batch` call (the GPU), smaller
/// ones with the per-description host functions (collector.py _GPU_PREP_MIN: a 9-description block
/// took 6.6 ms with host preparation and 8.6 ms through the batched call)
const GPU_PREP_MIN: usize = 64;

/// one description's preparation job: (ZG_PREP_KIND_*, its zg_prep_batch field row)
fn prep_jobs(txs: &[Tx]) -> Vec<(u8, Vec<u8>)> {
    let mut jobs = Vec::new();
    for tx in txs {
        for d in &tx.joinsplits {
            let kind = match (&d.groth_proof, &d.pghr_proof, d.pghr_ok, &tx.js_pubkey) {
                (Some(_), _, _, Some(_)) => ZG_PREP_KIND_JOINSPLIT,
                (None, Some(_), None, Some(_)) => ZG_PREP_KIND_JOINSPLIT_BN,
                _ => continue,
            };
            let mut f = Vec::with_capacity(ZG_PREP_FIELD_BYTES);
            f.extend_from_slice(&d.anchor);
            f.extend_from_slice(&d.random_seed);
            for x in d.nullifiers.iter().chain(d.macs.iter()).chain(d.commitments.iter()) {
                f.extend_from_slice(x);
            }
            f.extend_from_slice(tx.js_pubkey.as_ref().unwrap());
            f.extend_from_slice(&d.vpub_old.to_le_bytes());
            f.extend_from_slice(&d.vpub_new.to_le_bytes());
            jobs.push((kind, f));
        }
        for s in &tx.spends {
            let mut f = [s.cv, s.anchor, s.nullifier, s.rk].concat();
            f.resize(ZG_PREP_FIELD_BYTES, 0);
            jobs.push((ZG_PREP_KIND_SPEND, f));
        }
        for o in &tx.outputs {
            let mut f = [o.cv, o.cmu, o.epk].concat();
            f.resize(ZG_PREP_FIELD_BYTES, 0);
            jobs.push((ZG_PREP_KIND_OUTPUT, f));
        }
    }
    jobs
}

/// per job: its inputs (7 / 5 / 9 Fr) or the ZG_PREP_* error class
fn prepare<B: Backend>(v: &B, jobs: &[(u8, Vec<u8>)]) -> Result<Vec<Result<Vec<[u8; 32]>, i32>>, GpuError> {
    let nin = |k: u8| match k {
        ZG_PREP_KIND_SPEND => 7,
        ZG_PREP_KIND_OUTPUT => 5,
        _ => 9,
    };
    if jobs.len() >= GPU_PREP_MIN {
        let kinds: Vec<u8> = jobs.iter().map(|(k, _)| *k).collect();
        let fields: Vec<u8> = jobs.iter().flat_map(|(_, f)| f.iter().copied()).collect();
        if let Some((rows, codes)) = v.prep_batch(&kinds, &fields)? {
            return Ok(jobs
                .iter()
                .enumerate()
                .map(|(i, (k, _))| {
                    if codes[i] != 0 {
                        return Err(codes[i] as i32);
                    }
                    Ok(rows[288 * i..288 * i + 32 * nin(*k)].chunks(32).map(|c| c.try_into().unwrap()).collect())
                })
                .collect());
        }
    }
    Ok(jobs
        .iter()
        .map(|(k, f)| {
            let a = |i: usize| -> [u8; 32] { f[32 * i..32 * i + 32].try_into().unwrap() };
            match *k {
                ZG_PREP_KIND_SPEND => prep_spend(&a(0), &a(1), &a(2), &a(3)),
                ZG_PREP_KIND_OUTPUT => prep_output(&a(0), &a(1), &a(2)),
                _ => {
                    let vo = u64::from_le_bytes(f[288..296].try_into().unwrap());
                    let vn = u64::from_le_bytes(f[296..304].try_into().unwrap());
                    let (nf, mac, cm) = ([a(2), a(3)], [a(4), a(5)], [a(6), a(7)]);
                    if *k == ZG_PREP_KIND_JOINSPLIT {
                        Ok(prep_joinsplit(&a(0), &a(1), &nf, &mac, &cm, vo, vn, &a(8)))
                    } else {
                        Ok(prep_joinsplit_bn(&a(0), &a(1), &nf, &mac, &cm, vo, vn, &a(8)))
                    }
                }
            }
        })
        .collect())
}

fn queue<B: Backend>(v: &B, txs: &[Tx]) -> Result<(Vec<Item>, Vec<([u8; 296], Vec<[u8; 32]>)>, Plans), GpuError> {
    let mut res = prepare(v, &prep_jobs(txs))?.into_iter();
    let mut items = Vec::new();
    let mut pghr = Vec::new();
    let mut plans = Vec::new();
    for tx in txs {
        let (mut js, mut sp, mut out) = (Vec::new(), Vec::new(), Vec::new());
        for d in &tx.joinsplits {
            match (&d.groth_proof, &d.pghr_proof, d.pghr_ok, &tx.js_pubkey) {
                (Some(p), _, _, Some(_)) => {
                    let inputs = res.next().unwrap().expect("the JoinSplit preparation has no error class");
                    js.push(Plan::Proof(items.len()));
                    items.push(Item { proof: *p, kind: ZG_KIND_SPROUT, inputs });
                }
                (None, Some(p), None, Some(_)) => {
                    let inputs = res.next().unwrap().expect("the JoinSplit preparation has no error class");
                    js.push(Plan::Pghr(pghr.len()));
                    pghr.push((*p, inputs));
                }
                (_, _, v, _) => js.push(Plan::Caller(v.unwrap_or(false))),
            }
        }
        for s in &tx.spends {
            match res.next().unwrap() {
                Ok(inputs) => {
                    sp.push(Plan::Proof(items.len()));
                    items.push(Item { proof: s.zkproof, kind: ZG_KIND_SPEND, inputs });
                }
                Err(_) => sp.push(Plan::Prep),
            }
        }
        for o in &tx.outputs {
            match res.next().unwrap() {
                Ok(inputs) => {
                    out.push(Plan::Proof(items.len()));
                    items.push(Item { proof: o.zkproof, kind: ZG_KIND_OUTPUT, inputs });
                }
                Err(_) => out.push(Plan::Prep),
            }
        }
        plans.push((js, sp, out));
    }
    Ok((items, pghr, plans))
}

/// (per-tx spend_auth verdicts, per-tx binding verdict): the GPU's for transactions with a
/// sighash (one zg_sapling_bvk + one zg_redjubjub_verify call for the window), else the caller's
fn sig_verdicts<B: Backend>(v: &B, txs: &[Tx]) -> Result<(Vec<Vec<bool>>, Vec<bool>), GpuError> {
    let mut sp: Vec<Vec<bool>> = txs.iter().map(|t| t.spends.iter().map(|s| s.sig_ok).collect()).collect();
    let mut bind: Vec<bool> = txs.iter().map(|t| t.binding_ok).collect();
    let need: Vec<usize> =
        (0..txs.len()).filter(|&i| txs[i].sighash.is_some() && (!txs[i].spends.is_empty() || !txs[i].outputs.is_empty())).collect();
    if need.is_empty() {
        return Ok((sp, bind));
    }
    let rows: Vec<(Vec<[u8; 32]>, Vec<[u8; 32]>, i64)> = need
        .iter()
        .map(|&i| (txs[i].spends.iter().map(|s| s.cv).collect(), txs[i].outputs.iter().map(|o| o.cv).collect(),
                   txs[i].value_balance))
        .collect();
    let bvks = v.sapling_bvk(&rows)?;
    let mut items = Vec::new();
    let mut at = Vec::new();
    for (&i, (st, bvk)) in need.iter().zip(bvks.iter()) {
        let tx = &txs[i];
        let sh = tx.sighash.unwrap();
        for (j, s) in tx.spends.iter().enumerate() {
            if let Some(sig) = s.spend_auth_sig {
                let mut m = [0u8; 64];
                m[..32].copy_from_slice(&s.rk);
                m[32..].copy_from_slice(&sh);
                items.push((s.rk, sig, m, ZG_GEN_SPEND_AUTH));
                at.push((i, Some(j)));
            }
        }
        if let Some(sig) = tx.binding_sig {
            if *st == 0 {
                let mut m = [0u8; 64];
                m[..32].copy_from_slice(bvk);
                m[32..].copy_from_slice(&sh);
                items.push((*bvk, sig, m, ZG_GEN_BINDING));
                at.push((i, None));
            } else {
                bind[i] = false;  // a cv that does not decode / InvalidBalanceValue
            }
        }
    }
    if !items.is_empty() {
        for ((i, j), ok) in at.into_iter().zip(v.redjubjub_verify(&items)?) {
            match j {
                Some(j) => sp[i][j] = ok,
                None => bind[i] = ok,
            }
        }
    }
    Ok((sp, bind))
}

/// per-tx JoinSplit signature verdict: the backend's for transactions with JoinSplits that carry
/// js_sig and js_pubkey (ONE zg_ed25519_verify call for the window; any non-zero status is the
/// reference's JoinSplitSignature error), else the caller's js_sig_ok. js_sig without a sighash is
/// a caller error.
fn js_sig_verdicts<B: Backend>(v: &B, txs: &[Tx]) -> Result<Vec<bool>, GpuError> {
    let mut ok: Vec<bool> = txs.iter().map(|t| t.js_sig_ok).collect();
    let mut items = Vec::new();
    let mut at = Vec::new();
    for (i, tx) in txs.iter().enumerate() {
        if let (Some(sig), Some(pk), false) = (tx.js_sig, tx.js_pubkey, tx.joinsplits.is_empty()) {
            let sh = match tx.sighash {
                Some(h) => h,
                None => return Err(GpuError { code: -1, message: "a transaction carries js_sig but no sighash".to_string() }),
            };
            items.push((pk, sig, sh));
            at.push(i);
        }
    }
    if !items.is_empty() {
        for (i, st) in at.into_iter().zip(v.ed25519_verify(&items)?) {
            ok[i] = st == ZG_ED_OK;
        }
    }
    Ok(ok)
}

type EcdsaKey = (Vec<u8>, Vec<u8>, [u8; 32]);
/// (window index, input index or None, script code, hashtype) -> the sighash
type SighashKey = (usize, Option<u32>, Vec<u8>, u32);

/// one sighash call over the transactions `pairs` names; any status but ZG_SIGHASH_OK is an explicit error:
/// the caller hashes that transaction on the host, it is never accepted silently
fn run_sighash<B: Backend>(v: &B, txs: &[Tx], pairs: &[(usize, Option<u32>, Vec<u8>, u64, u32)]) -> Result<Vec<[u8; 32]>, GpuError> {
    let mut idx: Vec<usize> = pairs.iter().map(|p| p.0).collect();
    idx.sort();
    idx.dedup();
    let raws: Vec<(Vec<u8>, u32)> = idx.iter().map(|&i| (txs[i].raw.clone().unwrap_or_default(), txs[i].branch_id)).collect();
    let items: Vec<SighashItem> = pairs
        .iter()
        .map(|p| SighashItem { tx: idx.binary_search(&p.0).unwrap() as u32, input_index: p.1, script_code: p.2.clone(), amount: p.3, hashtype: p.4 })
        .collect();
    let (_, hashes, status) = v.sighash(&raws, &items)?;
    for (p, st) in pairs.iter().zip(&status) {
        if *st != ZG_SIGHASH_OK {
            return Err(GpuError { code: -1, message: format!("transaction {}: the signature hash of input {:?} was not computed (ZG_SIGHASH status {}); hash this transaction on the host", p.0, p.1, st) });
        }
    }
    Ok(hashes)
}

/// the window with every sighash in place: transactions that carry raw bytes and lack their no-input sighash
/// or carry ecdsa_requests are cloned with sighash set and the requests appended to ecdsa_checks, all from
/// ONE sighash call; a window that uses neither field is returned as it is (None) and asks for no call
fn resolve_sighashes<B: Backend>(v: &B, txs: &[Tx]) -> Result<Option<(Vec<Tx>, HashMap<SighashKey, [u8; 32]>)>, GpuError> {
    if let Some(i) = txs.iter().position(|t| t.raw.is_none() && !t.ecdsa_requests.is_empty()) {
        return Err(GpuError { code: -1, message: format!("transaction {} carries ecdsa_requests but no raw bytes", i) });
    }
    let need: Vec<usize> =
        (0..txs.len()).filter(|&i| txs[i].raw.is_some() && (txs[i].sighash.is_none() || !txs[i].ecdsa_requests.is_empty())).collect();
    if need.is_empty() {
        return Ok(None);
    }
    let mut pairs = Vec::new();
    for &i in &need {
        if txs[i].sighash.is_none() {
            pairs.push((i, None, Vec::new(), 0u64, 1u32));
        }
        for r in &txs[i].ecdsa_requests {
            pairs.push((i, Some(r.input_index as u32), r.script_code.clone(), r.amount, r.hashtype));
        }
    }
    let hashes = run_sighash(v, txs, &pairs)?;
    let known: HashMap<SighashKey, [u8; 32]> =
        pairs.iter().zip(hashes).map(|(p, h)| ((p.0, p.1, p.2.clone(), p.4), h)).collect();
    let mut out = txs.to_vec();
    for &i in &need {
        if out[i].sighash.is_none() {
            out[i].sighash = Some(known[&(i, None, Vec::new(), 1u32)]);
        }
        for r in &txs[i].ecdsa_requests {
            let sighash = known[&(i, Some(r.input_index as u32), r.script_code.clone(), r.hashtype)];
            out[i].ecdsa_checks.push(EcdsaCheck { input_index: r.input_index, pubkey: r.pubkey.clone(), sig: r.sig.clone(), sighash });
        }
    }
    Ok(Some((out, known)))
}

/// the verdict table of the window's recorded ECDSA checks: ONE ecdsa_verify call for all of them (any
/// non-zero status is false, verify.rs:60-67 unwrap_or(false))
fn ecdsa_table<B: Backend>(v: &B, txs: &[Tx]) -> Result<HashMap<EcdsaKey, bool>, GpuError> {
    let keys: Vec<EcdsaKey> =
        txs.iter().flat_map(|t| t.ecdsa_checks.iter().map(|c| (c.pubkey.clone(), c.sig.clone(), c.sighash))).collect();
    if keys.is_empty() {
        return Ok(HashMap::new());
    }
    let sts = v.ecdsa_verify(&keys)?;
    Ok(keys.into_iter().zip(sts).map(|(k, st)| (k, st == ZG_ECDSA_OK)).collect())
}

/// the eval error of one transaction: None when every recorded check is ZG_ECDSA_OK, else eval_rerun's
/// value with the table as the checker; a triple the optimistic runs never asked for (OP_CHECKMULTISIG
/// tries other pairs once one fails) is verified in a further call
fn eval_error<B: Backend>(v: &B, txs: &[Tx], idx: usize, table: &mut HashMap<EcdsaKey, bool>,
                          known: &mut HashMap<SighashKey, [u8; 32]>) -> Result<Option<TxError>, GpuError> {
    let tx = &txs[idx];
    if tx.ecdsa_checks.iter().all(|c| table[&(c.pubkey.clone(), c.sig.clone(), c.sighash)]) {
        return Ok(None);
    }
    if !tx.ecdsa_requests.is_empty() {
        let rerun = match &tx.eval_rerun_requests {
            Some(r) => r.clone(),
            None => return Err(GpuError { code: -1, message: "a transaction's requested ECDSA check failed but it carries no eval_rerun_requests".to_string() }),
        };
        // a request the optimistic run never made (another script code or pair): one further sighash call
        // with the amount the input's other requests carry, then one further ecdsa_verify call
        let mut lookup = |input: usize, pk: &[u8], sig: &[u8], code: &[u8], hashtype: u32| -> Result<bool, GpuError> {
            let key = (idx, Some(input as u32), code.to_vec(), hashtype);
            let sighash = match known.get(&key) {
                Some(h) => *h,
                None => {
                    let amount = match tx.ecdsa_requests.iter().find(|r| r.input_index == input) {
                        Some(r) => r.amount,
                        None => return Err(GpuError { code: -1, message: format!("transaction {}: no amount is known for input {}", idx, input) }),
                    };
                    let h = run_sighash(v, txs, &[(idx, Some(input as u32), code.to_vec(), amount, hashtype)])?[0];
                    known.insert(key, h);
                    h
                }
            };
            let k = (pk.to_vec(), sig.to_vec(), sighash);
            if let Some(ok) = table.get(&k) {
                return Ok(*ok);
            }
            let ok = v.ecdsa_verify(&[k.clone()])?[0] == ZG_ECDSA_OK;
            table.insert(k, ok);
            Ok(ok)
        };
        return (*rerun)(&mut lookup);
    }
    let rerun = match &tx.eval_rerun {
        Some(r) => r.clone(),
        None => return Err(GpuError { code: -1, message: "a transaction's ECDSA check failed but it carries no eval_rerun".to_string() }),
    };
    let mut lookup = |pk: &[u8], sig: &[u8], sighash: &[u8; 32]| -> Result<bool, GpuError> {
        let k = (pk.to_vec(), sig.to_vec(), *sighash);
        if let Some(ok) = table.get(&k) {
            return Ok(*ok);
        }
        let ok = v.ecdsa_verify(&[k.clone()])?[0] == ZG_ECDSA_OK;
        table.insert(k, ok);
        Ok(ok)
    };
    (*rerun)(&mut lookup)
}

/// the eval errors of the transactions that carry prevouts, by window index: every input of theirs goes through ONE
/// inputs_verify call; a transaction's error is Signature(lowest failing input, the interpreter's error). An input
/// without a verdict (not a template, out of range, a transaction the GPU does not parse) is an Err: the caller's
fn input_errors<B: Backend>(v: &B, txs: &[Tx], script_flags: u32) -> Result<HashMap<usize, Option<TxError>>, GpuError> {
    let need: Vec<usize> = (0..txs.len()).filter(|&i| txs[i].prevouts.is_some()).collect();
    let mut errors = HashMap::new();
    for &i in &need {
        let tx = &txs[i];
        if tx.raw.is_none() {
            return Err(GpuError { code: -1, message: format!("transaction {} carries prevouts but no raw bytes", i) });
        }
        if !tx.ecdsa_checks.is_empty() || !tx.ecdsa_requests.is_empty() || tx.eval_rerun.is_some() || tx.eval_rerun_requests.is_some() {
            return Err(GpuError { code: -1, message: format!("transaction {} carries prevouts and ecdsa_checks, ecdsa_requests or a rerun", i) });
        }
        errors.insert(i, None);
    }
    if need.is_empty() {
        return Ok(errors);
    }
    let raws: Vec<(Vec<u8>, u32)> = need.iter().map(|&i| (txs[i].raw.clone().unwrap(), txs[i].branch_id)).collect();
    let mut items = Vec::new();
    for (k, &i) in need.iter().enumerate() {
        for (j, p) in txs[i].prevouts.as_ref().unwrap().iter().enumerate() {
            items.push(InputItem { tx: k as u32, input_index: j as u32, script_pubkey: p.script_pubkey.clone(), amount: p.amount });
        }
    }
    let (_, status, _, _) = v.inputs_verify(&raws, &items, script_flags)?;
    for (it, st) in items.iter().zip(status) {
        let i = need[it.tx as usize];
        let name = match st {
            ZG_INPUT_OK => continue,
            ZG_INPUT_EQUALVERIFY => "EqualVerify",
            ZG_INPUT_SIGNATURE_DER => "SignatureDer",
            ZG_INPUT_EVAL_FALSE => "EvalFalse",
            _ => return Err(GpuError { code: -1, message: format!("transaction {}: input {} was not verified (ZG_INPUT status {}); run its script on the host", i, it.input_index, st) }),
        };
        if errors[&i].is_none() {
            errors.insert(i, Some(TxError::Signature(it.input_index as usize, name.to_string())));
        }
    }
    Ok(errors)
}

fn tx_error(tx: &Tx, plan: &(Vec<Plan>, Vec<Plan>, Vec<Plan>), status: &[u8], pghr_status: &[u8], sp_ok: &[bool],
            bind_ok: bool, js_sig_ok: bool, eval: Option<TxError>) -> Option<TxError> {
    let (js, sp, out) = plan;
    if let Some(e) = &tx.pre_error {
        return Some(TxError::Caller(e.clone()));
    }
    if eval.is_some() {
        return eval;
    }
    if !tx.joinsplits.is_empty() {
        if !js_sig_ok {
            return Some(TxError::JoinSplitSignature);
        }
        for (i, (d, p)) in tx.joinsplits.iter().zip(js).enumerate() {
            let ok = match p {
                Plan::Proof(k) => status[*k] == ZG_STATUS_OK,
                Plan::Pghr(k) => pghr_status[*k] == ZG_STATUS_OK,
                Plan::Caller(v) => *v,
                Plan::Prep => false,
            };
            if !ok {
                return Some(TxError::InvalidJoinSplit(i));
            }
            if let Some(e) = &d.tree_error {
                return Some(TxError::Caller(e.clone()));
            }
        }
        if let Some(e) = &tx.js_nullifier_error {
            return Some(TxError::Caller(e.clone()));
        }
    }
    if !tx.spends.is_empty() || !tx.outputs.is_empty() {
        for (ok, p) in sp_ok.iter().zip(sp) {
            let bad = match p {
                Plan::Proof(k) => !*ok || status[*k] != ZG_STATUS_OK,
                _ => true,
            };
            if bad {
                return Some(TxError::InvalidSapling);
            }
        }
        for p in out {
            let bad = match p {
                Plan::Proof(k) => status[*k] != ZG_STATUS_OK,
                _ => true,
            };
            if bad {
                return Some(TxError::InvalidSapling);
            }
        }
        if !bind_ok {
            return Some(TxError::InvalidSapling);
        }
        if let Some(e) = &tx.sapling_nullifier_error {
            return Some(TxError::Caller(e.clone()));
        }
    }
    None
}

/// Check the shielded proofs of a block (or an import window: transactions in chain order).
/// Ok(None) if every transaction passes, else Ok(Some((tx_index, error))) with the error the
/// reference reports; Err only for a backend (GPU / runtime) failure.
pub fn verify_block<B: Backend>(v: &B, txs: &[Tx]) -> Result<Option<(usize, TxError)>, GpuError> {
    verify_block_flags(v, txs, ZG_SCRIPT_VERIFY_DERSIG)
}

/// verify_block with the script flags the window's template inputs (Tx::prevouts) are verified under (bip66_height
/// is 0 on every network of network/src/consensus.rs: ZG_SCRIPT_VERIFY_DERSIG)
pub fn verify_block_flags<B: Backend>(v: &B, txs: &[Tx], script_flags: u32) -> Result<Option<(usize, TxError)>, GpuError> {
    let template = input_errors(v, txs, script_flags)?;
    // the sighashes the window leaves to the backend (Tx::raw), before the signature batches
    let resolved = resolve_sighashes(v, txs)?;
    let (owned, mut known) = match resolved {
        Some((t, k)) => (Some(t), k),
        None => (None, HashMap::new()),
    };
    let txs: &[Tx] = match &owned {
        Some(t) => &t[..],
        None => txs,
    };
    let (items, pghr, plans) = queue(v, txs)?;
    let status = if items.is_empty() { Vec::new() } else { v.verify(&items)? };
    let pghr_status = if pghr.is_empty() { Vec::new() } else { v.pghr13_verify(&pghr)? };
    let (sp_ok, bind_ok) = sig_verdicts(v, txs)?;
    let js_ok = js_sig_verdicts(v, txs)?;
    let mut table = ecdsa_table(v, txs)?;
    for (idx, (tx, plan)) in txs.iter().zip(&plans).enumerate() {
        // precedence: pre_error, then the eval error, then the JoinSplit and Sapling stages
        let eval = if let Some(e) = template.get(&idx) { e.clone() }
                   else if tx.pre_error.is_none() && !tx.ecdsa_checks.is_empty() { eval_error(v, txs, idx, &mut table, &mut known)? } else { None };
        if let Some(e) = tx_error(tx, plan, &status, &pghr_status, &sp_ok[idx], bind_ok[idx], js_ok[idx], eval) {
            return Ok(Some((idx, e)));
        }
    }
    Ok(None)
}

/// The degradation path: the window on the GPU; on any GpuError (HIP error, lost device,
/// ZG_E_DEBUG) the WHOLE window again on the reference's own CPU calls (`cpu::CpuBackend`:
/// verify_proof, pghr13_verify, redjubjub), which cannot fail this way. The window's
/// statuses never mix the two backends. `on_gpu_error` is told what failed (log it, and stop
/// using the device if it keeps failing).
pub fn verify_block_or_cpu(gpu: Option<&GpuVerifier>, cpu: &CpuBackend, txs: &[Tx],
                           on_gpu_error: &dyn Fn(&GpuError)) -> Option<(usize, TxError)> {
    if let Some(g) = gpu {
        match verify_block(g, txs) {
            Ok(r) => return r,
            Err(e) => on_gpu_error(&e),
        }
    }
    verify_block(cpu, txs).expect("the CPU backend does not fail")
}
