//! verification/src/gpu/mod.rs -- the MI355X batch Groth16 verifier behind Zebra's proof checks.
//!
//! A thin safe layer over the C ABI of include/zg.h (libzg.so, HIP for gfx950, built by
//! build.rs). It replaces, for a whole block or import window, the per-description
//! `Proof::<Bls12>::read` + `bellman::groth16::verify_proof` calls of
//! verification/src/sapling.rs:157-167,202-212 and verification/src/sprout.rs:69-80; the
//! queueing and re-injection in reference order is `collect` (a transcription of
//! zebra_amd/collector.py, which tests/test_collector.py checks against the reference's real
//! transactions).
pub mod collect;
pub mod cpu;
pub mod ffi;
pub mod writer;

use std::ffi::CStr;
use std::os::raw::c_int;
use std::sync::Mutex;

pub use ffi::{ZG_KIND_OUTPUT, ZG_KIND_SPEND, ZG_KIND_SPROUT};
pub use ffi::{ZG_STATUS_DECODE_INVALID, ZG_STATUS_MALFORMED_VK, ZG_STATUS_OK, ZG_STATUS_VERIFY_FAILED};

/// A C-ABI error: the ZG_E_* code and zg_last_error's text.
#[derive(Debug, Clone)]
pub struct GpuError {
    pub code: i32,
    pub message: String,
}

/// One queued Groth16 check: the 192 proof bytes, the kind (= verifying key) and its public
/// inputs as canonical little-endian Fr (`FrRepr::write_le`), 7 / 5 / 9 of them.
#[derive(Clone)]
pub struct Item {
    pub proof: [u8; 192],
    pub kind: u8,
    pub inputs: Vec<[u8; 32]>,
}

/// One signature hash to compute (GpuVerifier::sighash): the arguments of
/// TransactionInputSigner::signature_hash (script/src/sign.rs:152-160) over transaction number `tx` of the call.
#[derive(Clone, Debug, PartialEq, Eq, Hash)]
pub struct SighashItem {
    pub tx: u32,
    pub input_index: Option<u32>,
    pub script_code: Vec<u8>,
    pub amount: u64,
    pub hashtype: u32,
}

/// zg_tx_layout: the parser's verdict (ffi::ZG_TX_*) on one serialized transaction and, unless it is
/// MALFORMED, [header word, inputs, outputs, JoinSplits, Sapling spends, Sapling outputs, signature
/// version, bytes consumed]. CPU, no context.
pub fn tx_layout(raw: &[u8]) -> (u8, [u64; 8]) {
    let mut out = [0u64; 8];
    let pad = [0u8; 1];
    let p = if raw.is_empty() { pad.as_ptr() } else { raw.as_ptr() };
    let rc = unsafe { ffi::zg_tx_layout(p, raw.len(), out.as_mut_ptr()) };
    (rc as u8, out)
}

/// One template input to verify (GpuVerifier::inputs_verify): input `input_index` of transaction number `tx` of the
/// call, spending an output of value `amount` whose script is `script_pubkey`.
#[derive(Clone, Debug, PartialEq, Eq, Hash)]
pub struct InputItem {
    pub tx: u32,
    pub input_index: u32,
    pub script_pubkey: Vec<u8>,
    pub amount: u64,
}

/// zg_script_class: the template matcher zg_inputs_verify runs -> [class (ffi::ZG_SCRIPT_*), offset and length of the
/// signature push in script_sig, offset and length of the key push (P2PKH: in script_sig, P2PK: in script_pubkey)];
/// all zero for ZG_SCRIPT_HOST. CPU, no context.
pub fn script_class(script_sig: &[u8], script_pubkey: &[u8]) -> [u64; 5] {
    let mut out = [0u64; 5];
    let pad = [0u8; 1];
    let s = if script_sig.is_empty() { pad.as_ptr() } else { script_sig.as_ptr() };
    let p = if script_pubkey.is_empty() { pad.as_ptr() } else { script_pubkey.as_ptr() };
    unsafe { ffi::zg_script_class(s, script_sig.len(), p, script_pubkey.len(), out.as_mut_ptr()) };
    out
}

/// zg_script_match: script_class, and with ffi::ZG_SCRIPT_TEMPLATE_MULTISIG in `flags` the two multisig classes ->
/// [class, m, n, offset and length of the redeem script in script_sig (0, 0 unless P2SH), candidate pairs
/// m (n - m + 1), where the first signature push instruction starts in script_sig, 0]; all zero for ZG_SCRIPT_HOST.
/// CPU, no context. An undefined flag bit is an error.
pub fn script_match(script_sig: &[u8], script_pubkey: &[u8], flags: u32) -> Result<[u64; 8], GpuError> {
    let mut out = [0u64; 8];
    let pad = [0u8; 1];
    let s = if script_sig.is_empty() { pad.as_ptr() } else { script_sig.as_ptr() };
    let p = if script_pubkey.is_empty() { pad.as_ptr() } else { script_pubkey.as_ptr() };
    let rc = unsafe { ffi::zg_script_match(s, script_sig.len(), p, script_pubkey.len(), flags, out.as_mut_ptr()) };
    if rc < 0 {
        return Err(GpuError { code: rc, message: "zg_script_match".to_string() });
    }
    Ok(out)
}

/// One batch slot on one GPU (device buffers only; the streams and the prepared verifying keys
/// are shared per device inside libzg). Several slots keep several windows in flight.
pub struct GpuVerifier {
    ctx: *mut ffi::ZgCtx,
    max_batch: usize,
    lock: Mutex<()>,
}
unsafe impl Send for GpuVerifier {}
unsafe impl Sync for GpuVerifier {}

fn last_error(ctx: *mut ffi::ZgCtx) -> String {
    unsafe { CStr::from_ptr(ffi::zg_last_error(ctx)) }.to_string_lossy().into_owned()
}

fn check(ctx: *mut ffi::ZgCtx, rc: c_int) -> Result<(), GpuError> {
    if rc == ffi::ZG_OK {
        Ok(())
    } else {
        Err(GpuError { code: rc, message: last_error(ctx) })
    }
}

/// the flat layouts of zg_verify_batch: n x 192 proof bytes, n kinds, n x 288 input bytes, n counts
fn pack(items: &[Item]) -> (Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>) {
    let n = items.len();
    let mut proofs = Vec::with_capacity(ffi::ZG_PROOF_BYTES * n);
    let mut kinds = Vec::with_capacity(n);
    let mut inputs = vec![0u8; ffi::ZG_INPUT_STRIDE * n];
    let mut counts = Vec::with_capacity(n);
    for (i, it) in items.iter().enumerate() {
        proofs.extend_from_slice(&it.proof);
        kinds.push(it.kind);
        counts.push(it.inputs.len().min(255) as u8);
        for (j, x) in it.inputs.iter().enumerate().take(ffi::ZG_MAX_INPUTS) {
            let o = ffi::ZG_INPUT_STRIDE * i + ffi::ZG_FR_BYTES * j;
            inputs[o..o + ffi::ZG_FR_BYTES].copy_from_slice(x);
        }
    }
    (proofs, kinds, inputs, counts)
}

impl GpuVerifier {
    /// A slot on `device` for batches of up to `max_batch` proofs, with the three unchanged
    /// verifying keys of res/*.json (embedded at build time) prepared on the GPU.
    pub fn new(device: i32, max_batch: u32) -> Result<Self, GpuError> {
        // seeded = 0: every batch draws a fresh 256-bit getrandom(2) key, expanded on the GPU
        // by ChaCha20 into the 128-bit batch scalars
        let cfg = ffi::ZgConfig { device, max_batch, seeded: 0, seed: 0 };
        let ctx = unsafe { ffi::zg_create(&cfg) };
        if ctx.is_null() {
            return Err(GpuError { code: ffi::ZG_E_HIP, message: last_error(std::ptr::null_mut()) });
        }
        let v = GpuVerifier { ctx, max_batch: if max_batch == 0 { 65536 } else { max_batch as usize }, lock: Mutex::new(()) };
        for k in [ZG_KIND_SPEND, ZG_KIND_OUTPUT, ZG_KIND_SPROUT] {
            check(ctx, unsafe { ffi::zg_vk_load_builtin(ctx, k as c_int) })?;
        }
        Ok(v)
    }

    pub fn max_batch(&self) -> usize {
        self.max_batch
    }

    /// Every item's status (ZG_STATUS_*), exact per proof: a failing batch is bisected on the
    /// GPU. Windows larger than max_batch go as consecutive batches.
    pub fn verify(&self, items: &[Item]) -> Result<Vec<u8>, GpuError> {
        let _g = self.lock.lock().unwrap();
        let mut out = Vec::with_capacity(items.len());
        for chunk in items.chunks(self.max_batch.max(1)) {
            let (proofs, kinds, inputs, counts) = pack(chunk);
            let mut status = vec![0u8; chunk.len()];
            check(self.ctx, unsafe {
                ffi::zg_verify_batch(self.ctx, chunk.len(), proofs.as_ptr(), kinds.as_ptr(), inputs.as_ptr(),
                                     counts.as_ptr(), std::ptr::null(), status.as_mut_ptr(), std::ptr::null_mut())
            })?;
            out.extend_from_slice(&status);
        }
        Ok(out)
    }

    /// Multi-GPU split (one process per GPU): queue this rank's shard and return its 576-byte
    /// Miller partial. Gather the partials of all ranks (RCCL all-gather), then `verdict` and
    /// `finish` on every rank.
    pub fn begin_partial(&self, items: &[Item]) -> Result<[u8; 576], GpuError> {
        let (proofs, kinds, inputs, counts) = pack(items);
        check(self.ctx, unsafe {
            ffi::zg_batch_begin(self.ctx, items.len(), proofs.as_ptr(), kinds.as_ptr(), inputs.as_ptr(),
                                counts.as_ptr(), std::ptr::null())
        })?;
        let mut part = [0u8; 576];
        check(self.ctx, unsafe { ffi::zg_batch_partial(self.ctx, part.as_mut_ptr()) })?;
        Ok(part)
    }

    /// ONE final exponentiation of the product of all ranks' partials: the batch verdict.
    pub fn verdict(&self, partials: &[[u8; 576]]) -> Result<bool, GpuError> {
        let flat: Vec<u8> = partials.iter().flat_map(|p| p.iter().copied()).collect();
        let mut ok: c_int = 0;
        check(self.ctx, unsafe { ffi::zg_gt_check(self.ctx, partials.len(), flat.as_ptr(), &mut ok) })?;
        Ok(ok != 0)
    }

    /// Per-proof statuses of this rank's shard; a false verdict bisects the shard.
    pub fn finish(&self, n: usize, batch_ok: bool) -> Result<Vec<u8>, GpuError> {
        let mut status = vec![0u8; n];
        check(self.ctx, unsafe { ffi::zg_batch_finish(self.ctx, batch_ok as c_int, status.as_mut_ptr()) })?;
        Ok(status)
    }
}

impl GpuVerifier {
    /// RedJubjub PublicKey::read(vk) + verify(msg, sig, generator) for every item, on the GPU
    /// (spend_auth_sig: vk = rk, msg = rk || sighash, ZG_GEN_SPEND_AUTH; binding_sig: vk = bvk,
    /// msg = bvk || sighash, ZG_GEN_BINDING).
    pub fn redjubjub_verify(&self, items: &[([u8; 32], [u8; 64], [u8; 64], u8)]) -> Result<Vec<bool>, GpuError> {
        let _g = self.lock.lock().unwrap();
        let n = items.len();
        let mut vk = Vec::with_capacity(32 * n);
        let mut sig = Vec::with_capacity(64 * n);
        let mut msg = Vec::with_capacity(64 * n);
        let mut gen = Vec::with_capacity(n);
        for (v, s, m, g) in items {
            vk.extend_from_slice(v);
            sig.extend_from_slice(s);
            msg.extend_from_slice(m);
            gen.push(*g);
        }
        let mut ok = vec![0u8; n];
        check(self.ctx, unsafe {
            ffi::zg_redjubjub_verify(self.ctx, n, vk.as_ptr(), sig.as_ptr(), msg.as_ptr(), gen.as_ptr(), ok.as_mut_ptr())
        })?;
        Ok(ok.into_iter().map(|b| b == 1).collect())
    }

    /// Ed25519 JoinSplit signatures (accept_transaction.rs:649-653 -> crypto::verify_ed25519,
    /// crypto/src/lib.rs:298-305): per item (pubkey, signature R || S, the 32-byte sighash) ->
    /// ZG_ED_* (OK, PUBLIC_ENCODING, SIGNATURE_ENCODING, SIGNATURE: the reference's error class).
    pub fn ed25519_verify(&self, items: &[([u8; 32], [u8; 64], [u8; 32])]) -> Result<Vec<u8>, GpuError> {
        let _g = self.lock.lock().unwrap();
        let n = items.len();
        let mut pk = Vec::with_capacity(32 * n);
        let mut sig = Vec::with_capacity(64 * n);
        let mut msg = Vec::with_capacity(32 * n);
        for (p, s, m) in items {
            pk.extend_from_slice(p);
            sig.extend_from_slice(s);
            msg.extend_from_slice(m);
        }
        let mut status = vec![0u8; n];
        check(self.ctx, unsafe {
            ffi::zg_ed25519_verify(self.ctx, n, pk.as_ptr(), sig.as_ptr(), msg.as_ptr(), status.as_mut_ptr())
        })?;
        Ok(status)
    }

    /// secp256k1 ECDSA checks of transparent inputs (TransactionSignatureChecker::verify_signature,
    /// script/src/verify.rs:60-67 -> keys::Public::verify, keys/src/public.rs:38-49): per item (public
    /// key as pushed, DER signature without its hashtype byte, the 32-byte sighash) -> ZG_ECDSA_* (OK,
    /// PUBLIC, SIGNATURE_ENCODING, SIGNATURE). A key longer than 255 bytes is sent as length 0.
    pub fn ecdsa_verify(&self, items: &[(Vec<u8>, Vec<u8>, [u8; 32])]) -> Result<Vec<u8>, GpuError> {
        let _g = self.lock.lock().unwrap();
        let n = items.len();
        let mut pk = vec![0u8; ffi::ZG_ECDSA_PUBKEY_STRIDE * n];
        let mut len = Vec::with_capacity(n);
        let mut sig = Vec::new();
        let mut off = Vec::with_capacity(n + 1);
        let mut msg = Vec::with_capacity(32 * n);
        for (i, (p, s, m)) in items.iter().enumerate() {
            let k = p.len().min(ffi::ZG_ECDSA_PUBKEY_STRIDE);
            pk[ffi::ZG_ECDSA_PUBKEY_STRIDE * i..ffi::ZG_ECDSA_PUBKEY_STRIDE * i + k].copy_from_slice(&p[..k]);
            len.push(if p.len() <= 255 { p.len() as u8 } else { 0 });
            off.push(sig.len() as u32);
            sig.extend_from_slice(s);
            msg.extend_from_slice(m);
        }
        if sig.len() > u32::max_value() as usize {
            return Err(GpuError { code: -1, message: "ecdsa_verify: the signatures exceed 4 GiB".to_string() });
        }
        off.push(sig.len() as u32);
        sig.push(0);
        let mut status = vec![0u8; n];
        check(self.ctx, unsafe {
            ffi::zg_ecdsa_verify(self.ctx, n, pk.as_ptr(), len.as_ptr(), sig.as_ptr(), off.as_ptr(), msg.as_ptr(),
                                 status.as_mut_ptr())
        })?;
        Ok(status)
    }

    /// TransactionInputSigner::signature_hash (script/src/sign.rs:152-329) of every item over the serialized
    /// transactions `txs` (raw bytes, consensus branch id). An item: the transaction's number, the input
    /// index (None as the reference's None), the script code, the input's amount, the hashtype.
    /// -> (ZG_TX_* per transaction, the 32-byte hash per item in H256 storage order, ZG_SIGHASH_* per item).
    /// A hash is zero unless its status is ZG_SIGHASH_OK.
    pub fn sighash(&self, txs: &[(Vec<u8>, u32)], items: &[SighashItem])
                   -> Result<(Vec<u8>, Vec<[u8; 32]>, Vec<u8>), GpuError> {
        let _g = self.lock.lock().unwrap();
        let (ntx, n) = (txs.len(), items.len());
        let mut arena = Vec::new();
        let mut tx_off = Vec::with_capacity(ntx + 1);
        let mut branch = Vec::with_capacity(ntx + 1);
        for (raw, b) in txs.iter() {
            tx_off.push(arena.len() as u64);
            arena.extend_from_slice(raw);
            branch.push(*b);
        }
        tx_off.push(arena.len() as u64);
        arena.push(0);
        branch.push(0);
        let mut scripts = Vec::new();
        let mut script_off = Vec::with_capacity(n + 1);
        for it in items.iter() {
            script_off.push(scripts.len() as u32);
            scripts.extend_from_slice(&it.script_code);
        }
        if scripts.len() > u32::max_value() as usize {
            return Err(GpuError { code: -1, message: "sighash: the script codes exceed 4 GiB".to_string() });
        }
        script_off.push(scripts.len() as u32);
        scripts.push(0);
        let item_tx: Vec<u32> = items.iter().map(|it| it.tx).chain(Some(0)).collect();
        let index: Vec<u32> = items.iter().map(|it| it.input_index.unwrap_or(ffi::ZG_SIGHASH_NO_INPUT)).chain(Some(0)).collect();
        let amount: Vec<u64> = items.iter().map(|it| it.amount).chain(Some(0)).collect();
        let hashtype: Vec<u32> = items.iter().map(|it| it.hashtype).chain(Some(0)).collect();
        let mut tx_status = vec![0u8; ntx + 1];
        let mut hashes = vec![0u8; 32 * n + 1];
        let mut status = vec![0u8; n + 1];
        check(self.ctx, unsafe {
            ffi::zg_sighash(self.ctx, ntx, arena.as_ptr(), tx_off.as_ptr(), branch.as_ptr(), n, item_tx.as_ptr(),
                            index.as_ptr(), scripts.as_ptr(), script_off.as_ptr(), amount.as_ptr(), hashtype.as_ptr(),
                            tx_status.as_mut_ptr(), hashes.as_mut_ptr(), status.as_mut_ptr())
        })?;
        tx_status.truncate(ntx);
        status.truncate(n);
        let hs = (0..n).map(|i| { let mut h = [0u8; 32]; h.copy_from_slice(&hashes[32 * i..32 * i + 32]); h }).collect();
        Ok((tx_status, hs, status))
    }

    /// verify_script (script/src/interpreter.rs:288-360) of pay-to-pubkey-hash and pay-to-pubkey inputs over the
    /// serialized transactions `txs` (raw bytes, consensus branch id), under `flags` (ffi::ZG_SCRIPT_VERIFY_DERSIG
    /// or 0) -> (ZG_TX_* per transaction, ZG_INPUT_* per item, the ZG_ECDSA_* detail of an EVAL_FALSE item, the
    /// signature hash that was checked or zero). ZG_INPUT_HOST: not a template, the caller runs verify_script.
    pub fn inputs_verify(&self, txs: &[(Vec<u8>, u32)], items: &[InputItem], flags: u32)
                         -> Result<(Vec<u8>, Vec<u8>, Vec<u8>, Vec<[u8; 32]>), GpuError> {
        let _g = self.lock.lock().unwrap();
        let (ntx, n) = (txs.len(), items.len());
        let mut arena = Vec::new();
        let mut tx_off = Vec::with_capacity(ntx + 1);
        let mut branch = Vec::with_capacity(ntx + 1);
        for (raw, b) in txs.iter() {
            tx_off.push(arena.len() as u64);
            arena.extend_from_slice(raw);
            branch.push(*b);
        }
        tx_off.push(arena.len() as u64);
        arena.push(0);
        branch.push(0);
        let mut prev = Vec::new();
        let mut prev_off = Vec::with_capacity(n + 1);
        for it in items.iter() {
            prev_off.push(prev.len() as u32);
            prev.extend_from_slice(&it.script_pubkey);
        }
        if prev.len() > u32::max_value() as usize {
            return Err(GpuError { code: -1, message: "inputs_verify: the previous scripts exceed 4 GiB".to_string() });
        }
        prev_off.push(prev.len() as u32);
        prev.push(0);
        let item_tx: Vec<u32> = items.iter().map(|it| it.tx).chain(Some(0)).collect();
        let index: Vec<u32> = items.iter().map(|it| it.input_index).chain(Some(0)).collect();
        let amount: Vec<u64> = items.iter().map(|it| it.amount).chain(Some(0)).collect();
        let mut tx_status = vec![0u8; ntx + 1];
        let mut status = vec![0u8; n + 1];
        let mut detail = vec![0u8; n + 1];
        let mut hashes = vec![0u8; 32 * n + 1];
        check(self.ctx, unsafe {
            ffi::zg_inputs_verify(self.ctx, ntx, arena.as_ptr(), tx_off.as_ptr(), branch.as_ptr(), n, item_tx.as_ptr(),
                                  index.as_ptr(), prev.as_ptr(), prev_off.as_ptr(), amount.as_ptr(), flags,
                                  tx_status.as_mut_ptr(), status.as_mut_ptr(), detail.as_mut_ptr(), hashes.as_mut_ptr())
        })?;
        tx_status.truncate(ntx);
        status.truncate(n);
        detail.truncate(n);
        let hs = (0..n).map(|i| { let mut h = [0u8; 32]; h.copy_from_slice(&hashes[32 * i..32 * i + 32]); h }).collect();
        Ok((tx_status, status, detail, hs))
    }

    /// JoinSplitVerification::check and SaplingProof::check (accept_transaction.rs:575-596,649-657,707-714) of every
    /// transaction of a window from its serialized bytes, ONE call. txs: (serialized transaction, consensus branch id)
    /// -> per transaction (ffi::ZG_TX_*, ffi::ZG_SHTX_*: the reference's first error, the failing description's index
    /// in its list, the ffi::ZG_SHD_* inner class, the no-input signature hash of a v4 transaction or zero) and, per
    /// transaction, its descriptions' own ffi::ZG_SHD_* classes (JoinSplits, spends, outputs). ZG_SHTX_HOST: PHGR
    /// JoinSplits, which stay with pghr13_verify and ed25519_verify. The caller keeps tree_cache.continue_root and the
    /// nullifier checks; include/zg.h says where they go around the status.
    pub fn shielded_verify(&self, txs: &[(Vec<u8>, u32)])
                           -> Result<(Vec<u8>, Vec<u8>, Vec<u64>, Vec<u8>, Vec<[u8; 32]>, Vec<Vec<u8>>), GpuError> {
        self.shielded_verify_flags(txs, 0)
    }

    /// The same with flags. ffi::ZG_SHIELDED_PHGR: a v2 / v3 transaction with JoinSplits is checked in the call too
    /// (the Ed25519 signature, then Pghr13Proof::from_raw and verify per description: detail
    /// ffi::ZG_SHD_JOINSPLIT_ENCODING or ffi::ZG_SHD_JOINSPLIT_PGHR_PROOF) instead of coming back ZG_SHTX_HOST; its
    /// hash and its descriptions' classes are returned as a v4 transaction's are.
    pub fn shielded_verify_flags(&self, txs: &[(Vec<u8>, u32)], flags: u32)
                                 -> Result<(Vec<u8>, Vec<u8>, Vec<u64>, Vec<u8>, Vec<[u8; 32]>, Vec<Vec<u8>>), GpuError> {
        let _g = self.lock.lock().unwrap();
        let ntx = txs.len();
        let mut arena = Vec::new();
        let mut tx_off = Vec::with_capacity(ntx + 1);
        let mut branch = Vec::with_capacity(ntx + 1);
        for (raw, b) in txs.iter() {
            tx_off.push(arena.len() as u64);
            arena.extend_from_slice(raw);
            branch.push(*b);
        }
        tx_off.push(arena.len() as u64);
        arena.push(0);
        branch.push(0);
        let mut tx_status = vec![0u8; ntx + 1];
        let mut status = vec![0u8; ntx + 1];
        let mut index = vec![0u64; ntx + 1];
        let mut detail = vec![0u8; ntx + 1];
        let mut hashes = vec![0u8; 32 * ntx + 1];
        let mut desc_off = vec![0u64; ntx + 1];
        let mut desc = vec![0u8; arena.len() / 384 + 1];   // a description takes at least 384 bytes of its transaction
        check(self.ctx, unsafe {
            ffi::zg_shielded_verify_flags(self.ctx, ntx, arena.as_ptr(), tx_off.as_ptr(), branch.as_ptr(), flags,
                                          tx_status.as_mut_ptr(), status.as_mut_ptr(), index.as_mut_ptr(),
                                          detail.as_mut_ptr(), hashes.as_mut_ptr(), desc_off.as_mut_ptr(),
                                          desc.as_mut_ptr())
        })?;
        tx_status.truncate(ntx);
        status.truncate(ntx);
        index.truncate(ntx);
        detail.truncate(ntx);
        let hs = (0..ntx).map(|i| { let mut h = [0u8; 32]; h.copy_from_slice(&hashes[32 * i..32 * i + 32]); h }).collect();
        let ds = (0..ntx).map(|t| desc[desc_off[t] as usize..desc_off[t + 1] as usize].to_vec()).collect();
        Ok((tx_status, status, index, detail, hs, ds))
    }

    /// verify_equihash_solution (equihash.rs:80-172) for the instance `params` (ffi::ZG_EQ_*): per item
    /// (input, solution), inputs of one common length 1..=252 -> (ok, repeated) per item. `ok` is the
    /// reference's verdict, which accepts some solutions with a repeated index (distinct_indices,
    /// equihash.rs:258-274, compares only the left row's first index); `repeated` tells them apart.
    pub fn equihash_verify(&self, params: i32, items: &[(Vec<u8>, Vec<u8>)]) -> Result<(Vec<bool>, Vec<bool>), GpuError> {
        let _g = self.lock.lock().unwrap();
        let n = items.len();
        let ilen = items.first().map(|i| i.0.len()).unwrap_or(1);
        let slen = match params { 0 => 1344, 1 => 68, 2 => 36, _ => 0 };
        if slen == 0 || items.iter().any(|i| i.0.len() != ilen || i.1.len() != slen) {
            return Err(GpuError { code: ffi::ZG_E_INVAL, message: "equihash_verify: item sizes".to_string() });
        }
        let mut inputs = Vec::with_capacity(ilen * n);
        let mut sols = Vec::with_capacity(slen * n);
        for (i, s) in items {
            inputs.extend_from_slice(i);
            sols.extend_from_slice(s);
        }
        let mut ok = vec![0u8; n];
        let mut rep = vec![0u8; n];
        check(self.ctx, unsafe {
            ffi::zg_equihash_verify(self.ctx, params, n, inputs.as_ptr(), ilen, sols.as_ptr(), ok.as_mut_ptr(),
                                    rep.as_mut_ptr())
        })?;
        Ok((ok.into_iter().map(|b| b == 1).collect(), rep.into_iter().map(|b| b == 1).collect()))
    }

    /// HeaderEquihashSolution::check + HeaderProofOfWork::check (verify_header.rs:48-54,116-124) over
    /// serialized 1487-byte headers in ONE call -> per header (status ZG_HDR_*, block hash in H256
    /// storage order, flags ZG_HDR_F_*). max_bits: `consensus.network.max_bits().into()` as u32.
    pub fn headers_verify(&self, headers: &[Vec<u8>], max_bits: u32) -> Result<Vec<(u8, [u8; 32], u8)>, GpuError> {
        let _g = self.lock.lock().unwrap();
        let n = headers.len();
        if headers.iter().any(|h| h.len() != ffi::ZG_HEADER_BYTES) {
            return Err(GpuError { code: ffi::ZG_E_INVAL, message: "headers_verify: 1487-byte headers".to_string() });
        }
        let flat: Vec<u8> = headers.iter().flat_map(|h| h.iter().cloned()).collect();
        let mut status = vec![0u8; n];
        let mut hashes = vec![0u8; 32 * n];
        let mut flags = vec![0u8; n];
        check(self.ctx, unsafe {
            ffi::zg_headers_verify(self.ctx, n, flat.as_ptr(), max_bits, status.as_mut_ptr(), hashes.as_mut_ptr(),
                                   flags.as_mut_ptr())
        })?;
        Ok((0..n)
            .map(|i| {
                let mut h = [0u8; 32];
                h.copy_from_slice(&hashes[32 * i..32 * i + 32]);
                (status[i], h, flags[i])
            })
            .collect())
    }

    /// BlockVerifier::check (verify_block.rs:31-40) over serialized blocks in ONE call (zg_blocks_verify)
    /// -> per block (status ZG_BLK_*, detail word, transaction ids in H256 storage order). The id buffer
    /// is sized from the bytes: no transaction is shorter than 10 bytes.
    pub fn blocks_verify(&self, blocks: &[Vec<u8>], max_block_size: u64, max_block_sigops: u64)
                         -> Result<Vec<(u8, u64, Vec<[u8; 32]>)>, GpuError> {
        let _g = self.lock.lock().unwrap();
        let n = blocks.len();
        let mut off = vec![0u64; n + 1];
        for (i, b) in blocks.iter().enumerate() {
            off[i + 1] = off[i] + b.len() as u64;
        }
        let mut flat: Vec<u8> = blocks.iter().flat_map(|b| b.iter().cloned()).collect();
        flat.push(0);
        let cap = flat.len() / 10 + 1;
        let mut status = vec![0u8; n.max(1)];
        let mut detail = vec![0u64; n.max(1)];
        let mut counts = vec![0u64; n + 1];
        let mut ids = vec![0u8; 32 * cap];
        check(self.ctx, unsafe {
            ffi::zg_blocks_verify(self.ctx, n, flat.as_ptr(), off.as_ptr(), max_block_size, max_block_sigops, cap,
                                  status.as_mut_ptr(), std::ptr::null_mut(), detail.as_mut_ptr(), std::ptr::null_mut(),
                                  counts.as_mut_ptr(), ids.as_mut_ptr())
        })?;
        Ok((0..n)
            .map(|b| {
                let rows = (counts[b] as usize..counts[b + 1] as usize)
                    .map(|r| {
                        let mut h = [0u8; 32];
                        h.copy_from_slice(&ids[32 * r..32 * r + 32]);
                        h
                    })
                    .collect();
                (status[b], detail[b], rows)
            })
            .collect())
    }

    /// PHGR JoinSplit proofs (sprout.rs:61-67): per item the 296-byte proof and its
    /// into_bn_frs inputs (`prep_joinsplit_bn`) -> ZG_STATUS_* (DECODE_INVALID = InvalidEncoding,
    /// VERIFY_FAILED = InvalidPGHRProof). The builtin res/sprout-verifying-key.json is loaded on
    /// first use.
    pub fn pghr13_verify(&self, items: &[([u8; 296], Vec<[u8; 32]>)]) -> Result<Vec<u8>, GpuError> {
        let _g = self.lock.lock().unwrap();
        let n = items.len();
        let mut proofs = Vec::with_capacity(296 * n);
        let mut inputs = vec![0u8; ffi::ZG_INPUT_STRIDE * n];
        let mut counts = Vec::with_capacity(n);
        for (i, (p, x)) in items.iter().enumerate() {
            proofs.extend_from_slice(p);
            counts.push(x.len().min(ffi::ZG_MAX_INPUTS) as u8);
            for (j, v) in x.iter().enumerate().take(ffi::ZG_MAX_INPUTS) {
                let o = ffi::ZG_INPUT_STRIDE * i + ffi::ZG_FR_BYTES * j;
                inputs[o..o + ffi::ZG_FR_BYTES].copy_from_slice(v);
            }
        }
        let mut status = vec![0u8; n];
        check(self.ctx, unsafe {
            ffi::zg_pghr13_verify(self.ctx, n, proofs.as_ptr(), inputs.as_ptr(), counts.as_ptr(), status.as_mut_ptr(),
                                  std::ptr::null_mut())
        })?;
        Ok(status)
    }

    /// zg_prep_batch: a window's public-input preparation in one call (kinds ZG_PREP_KIND_*, fields
    /// n x ZG_PREP_FIELD_BYTES; the Sapling descriptions on the GPU, the JoinSplits on host threads)
    /// -> (inputs n x 288 bytes, codes ZG_PREP_*)
    pub fn prep_batch(&self, kinds: &[u8], fields: &[u8]) -> Result<(Vec<u8>, Vec<u8>), GpuError> {
        let n = kinds.len();
        assert_eq!(fields.len(), n * ffi::ZG_PREP_FIELD_BYTES, "fields must be n x ZG_PREP_FIELD_BYTES");
        let _g = self.lock.lock().unwrap();
        let mut inputs = vec![0u8; ffi::ZG_INPUT_STRIDE * n];
        let mut codes = vec![0u8; n];
        check(self.ctx, unsafe {
            ffi::zg_prep_batch(self.ctx, n, kinds.as_ptr(), fields.as_ptr(), inputs.as_mut_ptr(), codes.as_mut_ptr())
        })?;
        Ok((inputs, codes))
    }

    /// binding verification keys: per tx (spend cvs, output cvs, valueBalance) -> (status, bvk)
    pub fn sapling_bvk(&self, txs: &[(Vec<[u8; 32]>, Vec<[u8; 32]>, i64)]) -> Result<Vec<(u8, [u8; 32])>, GpuError> {
        let _g = self.lock.lock().unwrap();
        let n = txs.len();
        let ns: Vec<u32> = txs.iter().map(|t| t.0.len() as u32).collect();
        let no: Vec<u32> = txs.iter().map(|t| t.1.len() as u32).collect();
        let vb: Vec<i64> = txs.iter().map(|t| t.2).collect();
        let mut cvs = Vec::new();
        for t in txs {
            for c in t.0.iter().chain(t.1.iter()) {
                cvs.extend_from_slice(c);
            }
        }
        let mut bvk = vec![0u8; 32 * n];
        let mut st = vec![0u8; n];
        check(self.ctx, unsafe {
            ffi::zg_sapling_bvk(self.ctx, n, ns.as_ptr(), no.as_ptr(), cvs.as_ptr(), vb.as_ptr(), bvk.as_mut_ptr(),
                                st.as_mut_ptr())
        })?;
        Ok((0..n).map(|i| (st[i], bvk[32 * i..32 * i + 32].try_into().unwrap())).collect())
    }

    /// Note-commitment tree roots over an import window (storage::TreeState, serialized as the
    /// reference stores it): from `state` (empty = TreeState::new()) append `leaves` and return the
    /// root after each `marks[k]` of them (one per block for BlockSaplingRoot / the Sprout block
    /// root, one per JoinSplit for TreeCache::continue_root) and the serialized final state.
    /// kind: ffi::ZG_TREE_SPROUT (H29) or ffi::ZG_TREE_SAPLING (H32). Err(ZG_E_TREE_FULL) when the
    /// leaves overflow the tree ("Appending to full tree").
    pub fn tree_roots(&self, kind: c_int, height: c_int, state: &[u8], leaves: &[[u8; 32]], marks: &[u64])
                      -> Result<(Vec<[u8; 32]>, Vec<u8>), GpuError> {
        let _g = self.lock.lock().unwrap();
        let flat: Vec<u8> = leaves.iter().flat_map(|h| h.iter().copied()).collect();
        let mut roots = vec![0u8; 32 * marks.len()];
        let mut out_len = unsafe { ffi::zg_tree_state_max_bytes(height) };
        let mut out = vec![0u8; out_len];
        check(self.ctx, unsafe {
            ffi::zg_tree_roots(self.ctx, kind, height, state.as_ptr(), state.len(), leaves.len(), flat.as_ptr(),
                               marks.len(), marks.as_ptr(), roots.as_mut_ptr(), out.as_mut_ptr(), &mut out_len)
        })?;
        out.truncate(out_len);
        Ok((roots.chunks(32).map(|c| c.try_into().unwrap()).collect(), out))
    }
}

impl Drop for GpuVerifier {
    fn drop(&mut self) {
        unsafe { ffi::zg_destroy(self.ctx) }
    }
}

/// The Groth16 public-input preparation of the reference, restated in libzg (CPU only):
/// accept_spend (sapling.rs:101-155) -> 7 Fr, or the ZG_PREP_* error class.
pub fn prep_spend(cv: &[u8; 32], anchor: &[u8; 32], nullifier: &[u8; 32], rk: &[u8; 32]) -> Result<Vec<[u8; 32]>, i32> {
    let mut out = [0u8; 7 * 32];
    let rc = unsafe { ffi::zg_prep_spend(cv.as_ptr(), anchor.as_ptr(), nullifier.as_ptr(), rk.as_ptr(), out.as_mut_ptr()) };
    if rc != 0 {
        return Err(rc);
    }
    Ok(out.chunks(32).map(|c| c.try_into().unwrap()).collect())
}

/// accept_output (sapling.rs:171-200) -> 5 Fr
pub fn prep_output(cv: &[u8; 32], cmu: &[u8; 32], epk: &[u8; 32]) -> Result<Vec<[u8; 32]>, i32> {
    let mut out = [0u8; 5 * 32];
    let rc = unsafe { ffi::zg_prep_output(cv.as_ptr(), cmu.as_ptr(), epk.as_ptr(), out.as_mut_ptr()) };
    if rc != 0 {
        return Err(rc);
    }
    Ok(out.chunks(32).map(|c| c.try_into().unwrap()).collect())
}

/// sprout::verify's input (sprout.rs:34-58,86-153) -> 9 BLS12-381 Fr (into_bls_frs, the
/// Groth16 branch); `bn = true`: the same bits as 9 BN254 Fr (into_bn_frs, the PHGR branch)
#[allow(clippy::too_many_arguments)]
fn prep_joinsplit_any(bn: bool, anchor: &[u8; 32], random_seed: &[u8; 32], nullifiers: &[[u8; 32]; 2],
                      macs: &[[u8; 32]; 2], commitments: &[[u8; 32]; 2], vpub_old: u64, vpub_new: u64,
                      pubkey: &[u8; 32]) -> Vec<[u8; 32]> {
    let cat = |x: &[[u8; 32]; 2]| -> [u8; 64] {
        let mut o = [0u8; 64];
        o[..32].copy_from_slice(&x[0]);
        o[32..].copy_from_slice(&x[1]);
        o
    };
    let (nf, mc, cm) = (cat(nullifiers), cat(macs), cat(commitments));
    let mut out = [0u8; 9 * 32];
    unsafe {
        if bn {
            ffi::zg_prep_joinsplit_bn(anchor.as_ptr(), random_seed.as_ptr(), nf.as_ptr(), mc.as_ptr(), cm.as_ptr(),
                                      vpub_old, vpub_new, pubkey.as_ptr(), out.as_mut_ptr());
        } else {
            ffi::zg_prep_joinsplit(anchor.as_ptr(), random_seed.as_ptr(), nf.as_ptr(), mc.as_ptr(), cm.as_ptr(),
                                   vpub_old, vpub_new, pubkey.as_ptr(), out.as_mut_ptr());
        }
    }
    out.chunks(32).map(|c| c.try_into().unwrap()).collect()
}

#[allow(clippy::too_many_arguments)]
pub fn prep_joinsplit(anchor: &[u8; 32], random_seed: &[u8; 32], nullifiers: &[[u8; 32]; 2], macs: &[[u8; 32]; 2],
                      commitments: &[[u8; 32]; 2], vpub_old: u64, vpub_new: u64, pubkey: &[u8; 32]) -> Vec<[u8; 32]> {
    prep_joinsplit_any(false, anchor, random_seed, nullifiers, macs, commitments, vpub_old, vpub_new, pubkey)
}

#[allow(clippy::too_many_arguments)]
pub fn prep_joinsplit_bn(anchor: &[u8; 32], random_seed: &[u8; 32], nullifiers: &[[u8; 32]; 2], macs: &[[u8; 32]; 2],
                         commitments: &[[u8; 32]; 2], vpub_old: u64, vpub_new: u64, pubkey: &[u8; 32]) -> Vec<[u8; 32]> {
    prep_joinsplit_any(true, anchor, random_seed, nullifiers, macs, commitments, vpub_old, vpub_new, pubkey)
}
