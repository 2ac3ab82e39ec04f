"""ctypes binding of the C ABI (include/zg.h) -- the same calls a Rust `verification/gpu`
module makes over `extern "C"`. Loads the in-tree zebra_amd/libzg.so and
fails loudly if it is missing: there is no CPU fallback in the product path.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libzg.so")
# A/B experiments (tooling): ZG_LIB_VARIANT=name loads zebra_amd/libzg_<name>.so, a build of the same
# sources with other compile-time switches (tools/build_variant.py); never set in production
if os.environ.get("ZG_LIB_VARIANT"):
    LIB_PATH = os.path.join(HERE, "libzg_%s.so" % os.environ["ZG_LIB_VARIANT"])

KIND_SPEND, KIND_OUTPUT, KIND_SPROUT = 0, 1, 2
GEN_SPEND_AUTH, GEN_BINDING = 0, 1   # include/zg.h ZG_GEN_*
# include/zg.h ZG_ED_*: the reference's error class of an Ed25519 JoinSplit signature check
ED_OK, ED_PUBLIC_ENCODING, ED_SIGNATURE_ENCODING, ED_SIGNATURE = 0, 1, 2, 3
# include/zg.h ZG_ECDSA_*: keys::Public::verify of a transparent input's signature (Ok(true), Error::InvalidPublic,
# Error::InvalidSignature, Ok(false)); the stride of one key in zg_ecdsa_verify's pubkeys
ECDSA_OK, ECDSA_PUBLIC, ECDSA_SIGNATURE_ENCODING, ECDSA_SIGNATURE = 0, 1, 2, 3
ECDSA_PUBKEY_STRIDE = 65
# include/zg.h ZG_TX_* (zg_tx_layout's verdict on a serialized transaction), ZG_SIGHASH_* (an item of zg_sighash) and
# the input index that stands for the reference's None
TX_OK, TX_MALFORMED, TX_NONCANONICAL = 0, 1, 2
SIGHASH_OK, SIGHASH_TX_MALFORMED, SIGHASH_TX_NONCANONICAL, SIGHASH_INPUT_RANGE = 0, 1, 2, 3
SIGHASH_NO_INPUT = 0xFFFFFFFF
# include/zg.h ZG_SCRIPT_* (zg_script_class: the template of a (script_sig, script_pubkey) pair; the one script flag a
# template run reads) and ZG_INPUT_* (an item of zg_inputs_verify: the interpreter's error, or why there is no verdict)
SCRIPT_HOST, SCRIPT_P2PKH, SCRIPT_P2PK, SCRIPT_MULTISIG, SCRIPT_P2SH_MULTISIG = 0, 1, 2, 3, 4
SCRIPT_VERIFY_DERSIG = 1
SCRIPT_TEMPLATE_MULTISIG = 0x100   # zg_inputs_verify evaluates the two multisig classes as well (opt-in)
(INPUT_OK, INPUT_EQUALVERIFY, INPUT_SIGNATURE_DER, INPUT_EVAL_FALSE, INPUT_HOST, INPUT_TX_MALFORMED,
 INPUT_TX_NONCANONICAL, INPUT_RANGE) = range(8)
INPUT_ERRORS = {INPUT_EQUALVERIFY: "EqualVerify", INPUT_SIGNATURE_DER: "SignatureDer", INPUT_EVAL_FALSE: "EvalFalse"}
# include/zg.h ZG_SHTX_* (a transaction of zg_shielded_verify: the reference's first error, or why there is no verdict)
# and ZG_SHD_* (the inner error class; a description's own first failing class)
(SHTX_OK, SHTX_NONE, SHTX_JOINSPLIT_SIGNATURE, SHTX_INVALID_JOINSPLIT, SHTX_INVALID_SAPLING, SHTX_HOST,
 SHTX_TX_MALFORMED, SHTX_TX_NONCANONICAL) = range(8)
SHD_JOINSPLIT_PGHR_PROOF = 20   # ErrorKind::InvalidPGHRProof: a PHGR description under SHIELDED_PHGR
SHIELDED_PHGR = 1               # zg_shielded_verify_flags: v2 / v3 transactions with JoinSplits are checked in the call
SHTX_ERRORS = {SHTX_JOINSPLIT_SIGNATURE: "JoinSplitSignature", SHTX_INVALID_JOINSPLIT: "InvalidJoinSplit",
               SHTX_INVALID_SAPLING: "InvalidSapling"}
(SHD_OK, SHD_VALUE_COMMITMENT_INVALID, SHD_VALUE_COMMITMENT_SMALL_ORDER, SHD_ANCHOR, SHD_RANDOMIZED_KEY_INVALID,
 SHD_RANDOMIZED_KEY_SMALL_ORDER, SHD_NOTE_COMMITMENT, SHD_EPHEMERAL_KEY_INVALID, SHD_EPHEMERAL_KEY_SMALL_ORDER,
 SHD_SPEND_AUTH_SIG, SHD_PROOF_INVALID, SHD_PROOF_SYNTHESIS, SHD_PROOF_FAILED, SHD_BALANCE_VALUE,
 SHD_BINDING_SIGNATURE, SHD_JOINSPLIT_ENCODING, SHD_JOINSPLIT_PROOF, SHD_ED_PUBLIC_ENCODING,
 SHD_ED_SIGNATURE_ENCODING, SHD_ED_SIGNATURE) = range(20)
# include/zg.h ZG_EQ_* (Equihash instances), ZG_HDR_* (the first failing header check) and ZG_HDR_F_* (every check)
EQ_200_9, EQ_96_5, EQ_48_5 = 0, 1, 2
EQ_SOLUTION_BYTES = {EQ_200_9: 1344, EQ_96_5: 68, EQ_48_5: 36}
HEADER_BYTES = 1487
HDR_OK, HDR_MALFORMED, HDR_EQUIHASH, HDR_POW = 0, 1, 2, 3
HDR_F_EQUIHASH, HDR_F_POW, HDR_F_REPEATED = 1, 2, 4
# include/zg.h ZG_BLK_* (the first failing check of BlockVerifier::check) and ZG_BLK_F_* (every check that fails)
(BLK_OK, BLK_MALFORMED, BLK_NONCANONICAL, BLK_EMPTY, BLK_COINBASE, BLK_SIZE, BLK_EXTRA_COINBASE, BLK_DUPLICATED,
 BLK_SIGOPS, BLK_MERKLE_ROOT) = range(10)
(BLK_F_EMPTY, BLK_F_COINBASE, BLK_F_SIZE, BLK_F_EXTRA_COINBASE, BLK_F_DUPLICATED, BLK_F_SIGOPS,
 BLK_F_MERKLE_ROOT) = 1, 2, 4, 8, 16, 32, 64
BLK_NO_INDEX = (1 << 64) - 1
E_NOMEM = -5
TREE_SPROUT, TREE_SAPLING = 0, 1     # include/zg.h ZG_TREE_*
SPROUT_HEIGHT, SAPLING_HEIGHT = 29, 32   # storage/src/tree_state.rs H29 / H32
E_TREE_FULL = -7
E_DEBUG = -8     # ZG_DEBUG_EACH=1: batch statuses differ from the per-proof re-check
KIND_NINPUTS = {KIND_SPEND: 7, KIND_OUTPUT: 5, KIND_SPROUT: 9}
STATUS_OK, STATUS_DECODE_INVALID, STATUS_MALFORMED_VK, STATUS_VERIFY_FAILED, STATUS_INPUT_NONCANONICAL = 0, 1, 2, 3, 4
STATUS_NAMES = {0: "OK", 1: "DECODE_INVALID", 2: "MALFORMED_VK", 3: "VERIFY_FAILED", 4: "INPUT_NONCANONICAL"}
PROOF_BYTES, INPUT_STRIDE, GT_BYTES, R_BYTES = 192, 288, 576, 16
PREP_KIND_SPEND, PREP_KIND_OUTPUT, PREP_KIND_JOINSPLIT, PREP_KIND_JOINSPLIT_BN = 0, 1, 2, 3   # include/zg.h
PREP_FIELD_BYTES = 304

_lib = None


class ZgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("zg error %d: %s" % (code, msg))
        self.code = code


class _Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("max_batch", ctypes.c_uint32), ("seeded", ctypes.c_int),
                ("seed", ctypes.c_uint64)]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("zebra_amd/libzg.so is not built (run __graft_entry__.build()); "
                              "the GPU path has no fallback")
        L = ctypes.CDLL(LIB_PATH)
        vp, u8p, sz, i = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
        L.zg_create.restype = vp
        L.zg_create.argtypes = [ctypes.POINTER(_Config)]
        L.zg_set_priority.argtypes = [vp, i]
        L.zg_destroy.argtypes = [vp]
        L.zg_last_error.restype = ctypes.c_char_p
        L.zg_last_error.argtypes = [vp]
        L.zg_version.restype = ctypes.c_char_p
        L.zg_vk_load_builtin.argtypes = [vp, i]
        L.zg_vk_load_json.argtypes = [vp, i, u8p, sz]
        L.zg_vk_load_uncompressed.argtypes = [vp, i, u8p, u8p, u8p, u8p, u8p, u8p, sz, u8p]
        L.zg_vk_alpha_beta.argtypes = [vp, i, u8p]
        L.zg_verify_one_gt.argtypes = [vp, i, u8p, u8p, sz, u8p, u8p]
        L.zg_verify_each.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p, u8p]
        L.zg_verify_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p, u8p, u8p]
        L.zg_batch_begin.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p]
        L.zg_batch_begin_device.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        L.zg_batch_partial.argtypes = [vp, u8p]
        L.zg_batch_ready.argtypes = [vp]
        L.zg_gt_check.argtypes = [vp, sz, u8p, ctypes.POINTER(i)]
        L.zg_gt_check_many.argtypes = [vp, sz, ctypes.POINTER(sz), u8p, ctypes.POINTER(i)]
        L.zg_batch_finish.argtypes = [vp, i, u8p]
        L.zg_synth_rerandomize.argtypes = [vp, sz, u8p, u8p, sz, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, u8p]
        L.zg_last_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.zg_last_phase_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), sz]
        L.zg_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), sz]
        L.zg_bench_mad_rate.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.zg_bench_mad_rate_clock.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        L.zg_chacha20_blocks.argtypes = [vp, u8p, u8p, ctypes.c_uint32, ctypes.c_size_t, u8p]
        L.zg_redjubjub_verify.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p]
        L.zg_ed25519_verify.argtypes = [vp, sz, u8p, u8p, u8p, u8p]
        L.zg_ecdsa_verify.argtypes = [vp, sz, u8p, u8p, u8p, ctypes.POINTER(ctypes.c_uint32), u8p, u8p]
        u32p = ctypes.POINTER(ctypes.c_uint32)
        L.zg_tx_layout.argtypes = [u8p, sz, ctypes.POINTER(ctypes.c_uint64)]
        L.zg_sighash.argtypes = [vp, sz, u8p, ctypes.POINTER(ctypes.c_uint64), u32p, sz, u32p, u32p, u8p, u32p,
                                 ctypes.POINTER(ctypes.c_uint64), u32p, u8p, u8p, u8p]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        L.zg_script_class.argtypes = [u8p, sz, u8p, sz, u64p]
        L.zg_script_match.argtypes = [u8p, sz, u8p, sz, ctypes.c_uint32, u64p]
        L.zg_inputs_verify.argtypes = [vp, sz, u8p, u64p, u32p, sz, u32p, u32p, u8p, u32p, u64p, ctypes.c_uint32, u8p,
                                       u8p, u8p, u8p]
        L.zg_shielded_verify.argtypes = [vp, sz, u8p, u64p, u32p, u8p, u8p, u64p, u8p, u8p, u64p, u8p]
        L.zg_shielded_verify_flags.argtypes = [vp, sz, u8p, u64p, u32p, ctypes.c_uint32, u8p, u8p, u64p, u8p, u8p, u64p,
                                               u8p]
        L.zg_block_layout.argtypes = [u8p, sz, u64p, u64p, sz]
        L.zg_txids.argtypes = [vp, sz, u8p, u64p, u8p]
        L.zg_blocks_verify.argtypes = [vp, sz, u8p, u64p, ctypes.c_uint64, ctypes.c_uint64, sz, u8p, u8p, u64p, u8p,
                                       u64p, u8p]
        L.zg_last_sig_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.zg_equihash_verify.argtypes = [vp, ctypes.c_int, sz, u8p, sz, u8p, u8p, u8p]
        L.zg_headers_verify.argtypes = [vp, sz, u8p, ctypes.c_uint32, u8p, u8p, u8p]
        L.zg_pow_valid.argtypes = [ctypes.c_uint32, ctypes.c_uint32, u8p]
        L.zg_sapling_bvk.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), u8p,
                                     ctypes.POINTER(ctypes.c_int64), u8p, u8p]
        L.zg_jubjub_decode.argtypes = [vp, sz, u8p, u8p, u8p]
        L.zg_prep_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p]
        L.zg_merkle_combine.argtypes = [vp, i, sz, u8p, u8p, u8p, u8p]
        L.zg_pghr13_vk_load_builtin.argtypes = [vp]
        L.zg_pghr13_vk_load_json.argtypes = [vp, u8p, sz]
        L.zg_pghr13_verify.argtypes = [vp, sz, u8p, u8p, u8p, u8p, ctypes.POINTER(ctypes.c_float)]
        ip = ctypes.POINTER(ctypes.c_int)
        L.zg_pghr13_shape.argtypes = [vp, sz, ip, ip, ctypes.POINTER(ctypes.c_size_t), ip, ip]
        L.zg_bn254_pairing.argtypes = [vp, sz, u8p, u8p, u8p]
        L.zg_tree_empty_roots.argtypes = [vp, i, sz, u8p]
        L.zg_tree_state_max_bytes.restype = sz
        L.zg_tree_state_max_bytes.argtypes = [i]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        L.zg_tree_roots.argtypes = [vp, i, i, u8p, sz, sz, u8p, sz, u64p, u8p, u8p, ctypes.POINTER(sz)]
        L.zg_tree_roots_device.argtypes = [vp, i, i, u8p, sz, sz, vp, sz, u64p, u8p, u8p, ctypes.POINTER(sz),
                                           ctypes.POINTER(ctypes.c_float)]
        L.zg_prep_spend.argtypes = [u8p, u8p, u8p, u8p, u8p]
        L.zg_prep_output.argtypes = [u8p, u8p, u8p, u8p]
        L.zg_prep_joinsplit.argtypes = [u8p, u8p, u8p, u8p, u8p, ctypes.c_uint64, ctypes.c_uint64, u8p, u8p]
        L.zg_prep_joinsplit_bn.argtypes = [u8p, u8p, u8p, u8p, u8p, ctypes.c_uint64, ctypes.c_uint64, u8p, u8p]
        L.zg_hsig.argtypes = [u8p, u8p, u8p, u8p, u8p]
        L.zg_debug_field_mul.argtypes = [i, i, sz, u8p, u8p, u8p]
        _lib = L
    return _lib


# ---- host-side public-input preparation (include/zg.h zg_prep_*; CPU, no GPU needed)
PREP_ERRORS = {1: "ValueCommitment(Invalid)", 2: "ValueCommitment(SmallOrder)", 3: "Anchor",
               4: "RandomizedKey(Invalid)", 5: "RandomizedKey(SmallOrder)", 6: "NoteCommitment",
               7: "EphemeralKey(Invalid)", 8: "EphemeralKey(SmallOrder)"}


class PrepError(ValueError):
    """a description's public input failed the reference's checks (SpendError/OutputError class)"""

    def __init__(self, code):
        super().__init__(PREP_ERRORS.get(code, str(code)))
        self.code = code
        self.name = PREP_ERRORS.get(code, str(code))


def _prep(rc, out, n):
    if rc < 0:
        raise ZgError(rc, "bad argument")
    if rc:
        raise PrepError(rc)
    return [out.raw[32 * j:32 * j + 32] for j in range(n)]


def prep_fields(kind, *args):
    """one description's ZG_PREP_FIELD_BYTES row for zg_prep_batch: SPEND (cv, anchor, nullifier, rk),
    OUTPUT (cv, cmu, epk), JOINSPLIT[_BN] (anchor, random_seed, nullifiers, macs, commitments, vpub_old,
    vpub_new, pubkey) -- the arguments of prep_spend / prep_output / prep_joinsplit[_bn]"""
    if kind in (PREP_KIND_SPEND, PREP_KIND_OUTPUT):
        parts = [bytes(a) for a in args]
        if len(parts) != (4 if kind == PREP_KIND_SPEND else 3) or any(len(x) != 32 for x in parts):
            raise ZgError(-1, "bad Sapling description fields")
        row = b"".join(parts)
    else:
        anchor, seed, nfs, macs, cms, vo, vn, pk = args
        if any(len(bytes(x)) != 32 for x in [anchor, seed, pk, *nfs, *macs, *cms]) or not (
                len(nfs) == len(macs) == len(cms) == 2):
            raise ZgError(-1, "bad JoinSplit description fields")
        row = (bytes(anchor) + bytes(seed) + b"".join(map(bytes, nfs)) + b"".join(map(bytes, macs)) +
               b"".join(map(bytes, cms)) + bytes(pk) + int(vo).to_bytes(8, "little") + int(vn).to_bytes(8, "little"))
    return row.ljust(PREP_FIELD_BYTES, b"\0")


def prep_spend(cv, anchor, nullifier, rk):
    """accept_spend (verification/src/sapling.rs:101-155) -> 7 x 32-byte LE Fr"""
    out = ctypes.create_string_buffer(7 * 32)
    return _prep(lib().zg_prep_spend(bytes(cv), bytes(anchor), bytes(nullifier), bytes(rk), out), out, 7)


def prep_output(cv, cmu, epk):
    """accept_output (verification/src/sapling.rs:171-200) -> 5 x 32-byte LE Fr"""
    out = ctypes.create_string_buffer(5 * 32)
    return _prep(lib().zg_prep_output(bytes(cv), bytes(cmu), bytes(epk), out), out, 5)


def prep_joinsplit(anchor, random_seed, nullifiers, macs, commitments, vpub_old, vpub_new, pubkey):
    """sprout::verify input (verification/src/sprout.rs:34-58,86-153) -> 9 x 32-byte LE Fr"""
    out = ctypes.create_string_buffer(9 * 32)
    return _prep(lib().zg_prep_joinsplit(bytes(anchor), bytes(random_seed), b"".join(map(bytes, nullifiers)),
                                         b"".join(map(bytes, macs)), b"".join(map(bytes, commitments)),
                                         vpub_old, vpub_new, bytes(pubkey), out), out, 9)


def prep_joinsplit_bn(anchor, random_seed, nullifiers, macs, commitments, vpub_old, vpub_new, pubkey):
    """the PHGR branch's input (sprout.rs:34-67, Input::into_bn_frs: 253-bit chunks) -> 9 x
    32-byte LE BN254 Fr"""
    out = ctypes.create_string_buffer(9 * 32)
    return _prep(lib().zg_prep_joinsplit_bn(bytes(anchor), bytes(random_seed), b"".join(map(bytes, nullifiers)),
                                            b"".join(map(bytes, macs)), b"".join(map(bytes, commitments)),
                                            vpub_old, vpub_new, bytes(pubkey), out), out, 9)


def hsig(random_seed, nf0, nf1, pubkey):
    out = ctypes.create_string_buffer(32)
    rc = lib().zg_hsig(bytes(random_seed), bytes(nf0), bytes(nf1), bytes(pubkey), out)
    if rc:
        raise ZgError(rc, "bad argument")
    return out.raw


# zg_debug_field_mul operand sizes (5: a b mod 2^255 - 19, 6: (a + b 2^256) mod l: plain, canonical results)
FIELD_BYTES = {0: 48, 1: 48, 2: 96, 3: 32, 4: 32, 5: 32, 6: 32, 7: 32, 8: 32}


def debug_field_mul(field, a, b, device=0):
    """zg_debug_field_mul: the device's Montgomery product for each pair (lists of LE bytes)"""
    w = FIELD_BYTES[field]
    n = len(a)
    assert len(b) == n and all(len(x) == w for x in a) and all(len(x) == w for x in b)
    out = ctypes.create_string_buffer(max(1, w * n))
    rc = lib().zg_debug_field_mul(device, field, n, b"".join(a), b"".join(b), out)
    if rc:
        raise ZgError(rc, "zg_debug_field_mul")
    return [out.raw[w * i:w * i + w] for i in range(n)]


def pack_ecdsa(pubkeys, sigs, msgs):
    """the buffers of zg_ecdsa_verify: (pubkeys n x 65 zero-padded, pubkey_len, sigs back to back, sig_off as
    a ctypes uint32 array of n + 1, msg n x 32). A key longer than 255 bytes is sent as length 0 (any length
    other than 33 or 65 is ECDSA_PUBLIC and its bytes are not read)"""
    n = len(pubkeys)
    if not (len(sigs) == len(msgs) == n and all(len(m) == 32 for m in msgs)):
        raise ZgError(-1, "ecdsa_verify takes one signature and one 32-byte message per key")
    lens = bytes(len(k) if len(k) <= 255 else 0 for k in pubkeys)
    keys = b"".join(bytes(k)[:ECDSA_PUBKEY_STRIDE].ljust(ECDSA_PUBKEY_STRIDE, b"\0") for k in pubkeys)
    off = (ctypes.c_uint32 * (n + 1))()
    total = 0
    for i, s in enumerate(sigs):
        off[i] = total
        total += len(s)
    off[n] = total
    if total >= 1 << 32:
        raise ZgError(-1, "ecdsa_verify: the signatures exceed 4 GiB")
    return keys, lens, b"".join(map(bytes, sigs)), off, b"".join(map(bytes, msgs))


def tx_layout(raw):
    """zg_tx_layout: Transaction::deserialize (chain/src/transaction.rs:249-330) over exactly these bytes ->
    (TX_* status, [header word, inputs, outputs, JoinSplits, Sapling spends, Sapling outputs, signature version,
    bytes consumed]); the list is zero when the status is TX_MALFORMED. CPU, no context"""
    out = (ctypes.c_uint64 * 8)()
    rc = lib().zg_tx_layout(bytes(raw) + b"\0", len(raw), out)
    if rc < 0:
        raise ZgError(rc, "zg_tx_layout")
    return rc, list(out)


def pack_sighash(txs, branch_ids, items):
    """the buffers of zg_sighash. txs: serialized transactions; branch_ids: one consensus branch id per
    transaction; items: (transaction number, input index or None, script code, amount, hashtype) ->
    (arena, tx_off, branch, item_tx, input_index, scripts, script_off, amount, hashtype), the arrays as ctypes"""
    ntx, n = len(txs), len(items)
    if len(branch_ids) != ntx:
        raise ZgError(-1, "sighash takes one branch id per transaction")
    tx_off = (ctypes.c_uint64 * (ntx + 1))()
    total = 0
    for t, raw in enumerate(txs):
        tx_off[t] = total
        total += len(raw)
    tx_off[ntx] = total
    branch = (ctypes.c_uint32 * max(ntx, 1))(*[b & 0xFFFFFFFF for b in branch_ids])
    item_tx = (ctypes.c_uint32 * max(n, 1))(*[it[0] for it in items])
    index = (ctypes.c_uint32 * max(n, 1))(*[SIGHASH_NO_INPUT if it[1] is None else it[1] for it in items])
    script_off = (ctypes.c_uint32 * (n + 1))()
    stotal = 0
    for i, it in enumerate(items):
        script_off[i] = stotal
        stotal += len(it[2])
    if stotal >= 1 << 32:
        raise ZgError(-1, "sighash: the script codes exceed 4 GiB")
    script_off[n] = stotal
    amount = (ctypes.c_uint64 * max(n, 1))(*[it[3] for it in items])
    hashtype = (ctypes.c_uint32 * max(n, 1))(*[it[4] & 0xFFFFFFFF for it in items])
    return (b"".join(map(bytes, txs)), tx_off, branch, item_tx, index, b"".join(bytes(it[2]) for it in items),
            script_off, amount, hashtype)


def pack_shielded(txs, branch_ids):
    """the buffers of zg_shielded_verify. txs: serialized transactions; branch_ids: one consensus branch id per
    transaction -> (arena, tx_off, branch), the arrays as ctypes"""
    return pack_sighash(txs, branch_ids, [])[:3]


def script_class(script_sig, script_pubkey):
    """zg_script_class: the template matcher zg_inputs_verify runs -> (SCRIPT_* class, signature push offset and
    length in script_sig, key push offset and length: in script_sig for P2PKH, in script_pubkey for P2PK); all zero
    for SCRIPT_HOST. CPU, no context"""
    out = (ctypes.c_uint64 * 5)()
    rc = lib().zg_script_class(bytes(script_sig) + b"\0", len(script_sig), bytes(script_pubkey) + b"\0",
                               len(script_pubkey), out)
    if rc < 0:
        raise ZgError(rc, "zg_script_class")
    return tuple(out)


def script_match(script_sig, script_pubkey, flags=0):
    """zg_script_match: script_class, and with SCRIPT_TEMPLATE_MULTISIG in `flags` the two multisig classes -> (SCRIPT_*
    class, m, n, redeem script offset and length in script_sig (0, 0 unless P2SH), candidate pairs m (n - m + 1), where
    the first signature push instruction starts in script_sig, 0); all zero for SCRIPT_HOST. CPU, no context"""
    out = (ctypes.c_uint64 * 8)()
    rc = lib().zg_script_match(bytes(script_sig) + b"\0", len(script_sig), bytes(script_pubkey) + b"\0",
                               len(script_pubkey), flags, out)
    if rc < 0:
        raise ZgError(rc, "zg_script_match")
    return tuple(out)


def pack_inputs_verify(txs, branch_ids, items):
    """the buffers of zg_inputs_verify. items: (transaction number, input index, the spent output's script_pubkey,
    its value) -> (arena, tx_off, branch, item_tx, input_index, prev_scripts, prev_off, amount), the arrays as ctypes"""
    sh = pack_sighash(txs, branch_ids, [(t, i, s, a, 0) for t, i, s, a in items])
    return sh[:8]


def block_layout(raw):
    """zg_block_layout: Block::deserialize (chain/src/block.rs:10-14) over exactly these bytes -> (TX_* status,
    [transactions, IndexedBlock::size, sigops, 1 when transaction 0 is a coinbase, index of the first later
    coinbase or BLK_NO_INDEX, bytes consumed], the transactions' offsets); the list is zero and the offsets None
    when the status is TX_MALFORMED. CPU, no context"""
    out = (ctypes.c_uint64 * 6)()
    buf = bytes(raw) + b"\0"
    rc = lib().zg_block_layout(buf, len(raw), out, None, 0)
    if rc < 0:
        raise ZgError(rc, "zg_block_layout")
    off = None
    if rc != TX_MALFORMED:
        tx_off = (ctypes.c_uint64 * (out[0] + 1))()
        lib().zg_block_layout(buf, len(raw), out, tx_off, out[0] + 1)
        off = list(tx_off)
    return rc, list(out), off


def pack_slices(slices):
    """byte strings back to back -> (arena, their len + 1 offsets as ctypes)"""
    off = (ctypes.c_uint64 * (len(slices) + 1))()
    total = 0
    for i, b in enumerate(slices):
        off[i] = total
        total += len(b)
    off[len(slices)] = total
    return b"".join(map(bytes, slices)), off


def pow_valid(max_bits, bits, hash32):
    """is_valid_proof_of_work (verification/src/work.rs:21-34) on the CPU, the routine the header kernel
    uses: compacts as u32, the hash in H256 storage order"""
    if len(hash32) != 32:
        raise ZgError(-1, "pow_valid takes a 32-byte hash")
    return lib().zg_pow_valid(max_bits & 0xFFFFFFFF, bits & 0xFFFFFFFF, bytes(hash32)) == 1


def pack_inputs(rows):
    """list (per proof) of lists of ints / 32-byte LE values -> n x 288 bytes"""
    out = bytearray(INPUT_STRIDE * len(rows))
    for i, row in enumerate(rows):
        for j, x in enumerate(row):
            b = x if isinstance(x, (bytes, bytearray)) else int(x).to_bytes(32, "little")
            out[INPUT_STRIDE * i + 32 * j:INPUT_STRIDE * i + 32 * j + 32] = b
    return bytes(out)


class Context:
    """One zg_ctx: a HIP stream, device buffers and the prepared VKs of one GPU."""

    def __init__(self, device=0, max_batch=65536, seed=None, load_builtin=True):
        L = lib()
        self.max_batch = max_batch
        cfg = _Config(device, max_batch, 1 if seed is not None else 0, seed or 0)
        self._p = L.zg_create(ctypes.byref(cfg))
        if not self._p:
            raise ZgError(-2, "zg_create failed: %s" % (L.zg_last_error(None) or b"no GPU / HIP error").decode())
        if load_builtin:
            for k in (KIND_SPEND, KIND_OUTPUT, KIND_SPROUT):
                self.vk_load_builtin(k)

    def close(self):
        if self._p:
            lib().zg_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise ZgError(rc, lib().zg_last_error(self._p).decode())

    def vk_load_builtin(self, kind):
        self._chk(lib().zg_vk_load_builtin(self._p, kind))

    def vk_load_json(self, kind, text):
        b = text.encode() if isinstance(text, str) else text
        self._chk(lib().zg_vk_load_json(self._p, kind, b, len(b)))

    def vk_load_uncompressed(self, kind, alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1, delta_g2, ic):
        self._chk(lib().zg_vk_load_uncompressed(self._p, kind, alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1,
                                                delta_g2, len(ic), b"".join(ic) if ic else None))

    def alpha_beta(self, kind):
        out = ctypes.create_string_buffer(GT_BYTES)
        self._chk(lib().zg_vk_alpha_beta(self._p, kind, out))
        return out.raw

    def verify_one_gt(self, kind, proof, inputs):
        """bellman verify_proof for one proof -> (status, GT bytes | None)."""
        inp = pack_inputs([inputs])[:32 * len(inputs)] if inputs else b""
        st = ctypes.create_string_buffer(1)
        gt = ctypes.create_string_buffer(GT_BYTES)
        self._chk(lib().zg_verify_one_gt(self._p, kind, bytes(proof), inp or None, len(inputs), st, gt))
        s = st.raw[0]
        return s, (gt.raw if s in (STATUS_OK, STATUS_VERIFY_FAILED) else None)

    def verify_each(self, proofs, kinds, inputs, n_inputs=None, want_gt=True):
        """per-proof bellman-exact verification -> (statuses, list of GT bytes | None)"""
        n = len(kinds)
        st = ctypes.create_string_buffer(max(n, 1))
        gts = ctypes.create_string_buffer(max(GT_BYTES * n, 1)) if want_gt else None
        self._chk(lib().zg_verify_each(self._p, n, bytes(proofs), bytes(kinds), bytes(inputs),
                                       bytes(n_inputs) if n_inputs is not None else None, st, gts))
        sts = list(st.raw[:n])
        if not want_gt:
            return sts, None
        return sts, [gts.raw[GT_BYTES * i:GT_BYTES * (i + 1)] if sts[i] in (0, 3) else None for i in range(n)]

    def verify_batch(self, proofs, kinds, inputs, n_inputs=None, r=None, want_gt=False):
        """-> (list of statuses, accumulated GT bytes | None)"""
        n = len(kinds)
        st = ctypes.create_string_buffer(max(n, 1))
        gt = ctypes.create_string_buffer(GT_BYTES) if want_gt else None
        self._chk(lib().zg_verify_batch(self._p, n, bytes(proofs), bytes(kinds), bytes(inputs),
                                        bytes(n_inputs) if n_inputs is not None else None,
                                        bytes(r) if r is not None else None, st, gt))
        return list(st.raw[:n]), (gt.raw if want_gt else None)

    def batch_begin(self, proofs, kinds, inputs, n_inputs=None, r=None):
        self._chk(lib().zg_batch_begin(self._p, len(kinds), bytes(proofs), bytes(kinds), bytes(inputs),
                                       bytes(n_inputs) if n_inputs is not None else None,
                                       bytes(r) if r is not None else None))

    def batch_begin_device(self, n, d_proofs, d_kinds, d_inputs, d_n_inputs=None, d_r=None):
        """device pointers (ints, e.g. torch tensor data_ptr()) of HBM-resident inputs"""
        self._chk(lib().zg_batch_begin_device(self._p, n, d_proofs, d_kinds, d_inputs, d_n_inputs, d_r))

    def batch_partial(self):
        out = ctypes.create_string_buffer(GT_BYTES)
        self._chk(lib().zg_batch_partial(self._p, out))
        return out.raw

    def batch_ready(self):
        """True once the batch's device work is done (never blocks; zg_batch_ready)"""
        r = lib().zg_batch_ready(self._p)
        if r < 0:
            self._chk(r)
        return r == 1

    def gt_check(self, partials):
        ok = ctypes.c_int(0)
        self._chk(lib().zg_gt_check(self._p, len(partials), b"".join(partials), ctypes.byref(ok)))
        return bool(ok.value)

    GT_SETS_MAX = 16

    def gt_check_many(self, sets):
        """verdicts of several batches in one launch (zg_gt_check_many): sets = [[partial, ...], ...]
        (1..16 sets), one final exponentiation each, side by side -> [bool, ...]"""
        n = len(sets)
        if not 0 < n <= self.GT_SETS_MAX or any(len(p) == 0 for p in sets):
            raise ValueError("gt_check_many: 1..%d non-empty sets" % self.GT_SETS_MAX)
        counts = (ctypes.c_size_t * n)(*[len(p) for p in sets])
        ok = (ctypes.c_int * n)()
        self._chk(lib().zg_gt_check_many(self._p, n, counts, b"".join(b"".join(p) for p in sets), ok))
        return [bool(v) for v in ok]

    def set_priority(self, high):
        """recreate this context's streams at the highest (True) or default priority"""
        self._chk(lib().zg_set_priority(self._p, 1 if high else 0))

    def batch_finish(self, batch_ok, n):
        st = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_batch_finish(self._p, 1 if batch_ok else 0, st))
        return list(st.raw[:n])

    PHASES = ("decode", "k_batch_lines", "k_batch_fchain", "k_tree_f", "root_partial", "side_stream_vk",
              "device_pipeline", "k4_msm", "k4_bucket_phase")

    def last_timings(self):
        """[decode, lines, fchain, tree, root_partial, side_stream, device_pipeline, K4, K4 bucket
        phase] in ms (include/zg.h zg_last_phase_ms)"""
        a = (ctypes.c_float * len(self.PHASES))()
        self._chk(lib().zg_last_phase_ms(self._p, a, len(self.PHASES)))
        return list(a)

    STAT_NAMES = ("batches", "fused_launches", "fused_wait_failures", "b_subgroup_recomputes", "bisections",
                  "bisect_nodes", "k4_entries", "quad_fchain_launches", "pghr13_calls", "pghr13_batch_failures",
                  "glv_csum_batches", "line_product_batches", "affine_line_batches")

    def stats(self):
        """cumulative counters (include/zg.h zg_stats) as a dict"""
        a = (ctypes.c_uint64 * len(self.STAT_NAMES))()
        self._chk(lib().zg_stats(self._p, a, len(self.STAT_NAMES)))
        return dict(zip(self.STAT_NAMES, list(a)))

    def synth_rerandomize(self, src_proofs, src_kinds, src_index, seed):
        n = len(src_index)
        idx = (ctypes.c_uint32 * max(n, 1))(*src_index)
        out = ctypes.create_string_buffer(max(192 * n, 1))
        self._chk(lib().zg_synth_rerandomize(self._p, len(src_kinds), bytes(src_proofs), bytes(src_kinds), n, idx,
                                             seed, out))
        return out.raw[:192 * n]

    # ---- Sapling signatures / Jubjub points on the GPU (include/zg.h zg_redjubjub_verify, ...)
    def redjubjub_verify(self, vks, sigs, msgs, gens):
        """per item: redjubjub PublicKey::read(vk) + verify(msg, sig, generator) -> list of bool"""
        n = len(vks)
        assert len(sigs) == len(msgs) == len(gens) == n
        ok = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_redjubjub_verify(self._p, n, b"".join(map(bytes, vks)), b"".join(map(bytes, sigs)),
                                            b"".join(map(bytes, msgs)), bytes(gens), ok))
        return [b == 1 for b in ok.raw[:n]]

    def ed25519_verify(self, pubkeys, sigs, msgs):
        """per item: ed25519 PublicKey::from_bytes + Signature::from_bytes + verify over the 32-byte
        message -> list of ED_* statuses (0 ok, 1 key encoding, 2 signature encoding, 3 signature)"""
        n = len(pubkeys)
        assert len(sigs) == len(msgs) == n
        if not (all(len(x) == 32 for x in pubkeys) and all(len(x) == 64 for x in sigs) and
                all(len(x) == 32 for x in msgs)):
            raise ZgError(-1, "ed25519_verify takes 32-byte keys, 64-byte signatures and 32-byte messages")
        st = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_ed25519_verify(self._p, n, b"".join(map(bytes, pubkeys)), b"".join(map(bytes, sigs)),
                                          b"".join(map(bytes, msgs)), st))
        return list(st.raw[:n])

    def equihash_verify(self, params, inputs, solutions):
        """verify_equihash_solution per (input, solution) for the instance params (EQ_*): inputs of one
        common length 1..252, solutions of EQ_SOLUTION_BYTES[params] -> (ok, repeated): the reference's
        verdicts and whether some index occurs twice (lists of bool)"""
        n = len(inputs)
        assert len(solutions) == n
        if params not in EQ_SOLUTION_BYTES:
            raise ZgError(-1, "equihash_verify: unknown instance")
        ilen = len(inputs[0]) if n else 1
        if not (1 <= ilen <= 252 and all(len(x) == ilen for x in inputs) and
                all(len(x) == EQ_SOLUTION_BYTES[params] for x in solutions)):
            raise ZgError(-1, "equihash_verify takes inputs of one length 1..252 and %d-byte solutions"
                          % EQ_SOLUTION_BYTES[params])
        ok = ctypes.create_string_buffer(max(n, 1))
        rep = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_equihash_verify(self._p, params, n, b"".join(map(bytes, inputs)), ilen,
                                           b"".join(map(bytes, solutions)), ok, rep))
        return [b == 1 for b in ok.raw[:n]], [b == 1 for b in rep.raw[:n]]

    def headers_verify(self, headers, max_bits):
        """HeaderEquihashSolution::check + HeaderProofOfWork::check over serialized 1487-byte headers, ONE
        call -> (statuses HDR_*, block hashes in H256 storage order, flags HDR_F_* masks)"""
        n = len(headers)
        if not all(len(x) == HEADER_BYTES for x in headers):
            raise ZgError(-1, "headers_verify takes %d-byte headers" % HEADER_BYTES)
        st = ctypes.create_string_buffer(max(n, 1))
        hs = ctypes.create_string_buffer(max(32 * n, 1))
        fl = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_headers_verify(self._p, n, b"".join(map(bytes, headers)), max_bits & 0xFFFFFFFF, st, hs, fl))
        return list(st.raw[:n]), [hs.raw[32 * i:32 * i + 32] for i in range(n)], list(fl.raw[:n])

    def ecdsa_verify(self, pubkeys, sigs, msgs):
        """per item: keys::Public::verify -- Public::from_slice of the key (33 or 65 bytes), Signature::from_der_lax
        of the signature (DER without its hashtype byte, any length), verify over the 32-byte sighash -> list of
        ECDSA_* statuses (0 ok, 1 public key, 2 signature encoding, 3 signature)"""
        n = len(pubkeys)
        keys, lens, sg, off, msg = pack_ecdsa(pubkeys, sigs, msgs)
        st = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_ecdsa_verify(self._p, n, keys, lens, sg + b"\0", off, msg, st))
        return list(st.raw[:n])

    def sighash(self, txs, branch_ids, items):
        """TransactionInputSigner::signature_hash (script/src/sign.rs:152-329) per item over the serialized
        transactions. items: (transaction number, input index or None, script code, amount, hashtype) ->
        (TX_* per transaction, 32-byte hash per item in H256 storage order, SIGHASH_* per item); a hash is zero
        unless its status is SIGHASH_OK"""
        ntx, n = len(txs), len(items)
        arena, tx_off, branch, item_tx, index, scripts, script_off, amount, hashtype = pack_sighash(txs, branch_ids, items)
        ts = ctypes.create_string_buffer(max(ntx, 1))
        hs = ctypes.create_string_buffer(max(32 * n, 1))
        st = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_sighash(self._p, ntx, arena + b"\0", tx_off, branch, n, item_tx, index, scripts + b"\0",
                                   script_off, amount, hashtype, ts, hs, st))
        return list(ts.raw[:ntx]), [hs.raw[32 * i:32 * i + 32] for i in range(n)], list(st.raw[:n])

    def inputs_verify(self, txs, branch_ids, items, flags=SCRIPT_VERIFY_DERSIG, want_detail=True, want_hashes=True):
        """verify_script (script/src/interpreter.rs:288-360) of pay-to-pubkey-hash and pay-to-pubkey inputs over the
        serialized transactions. items: (transaction number, input index, the spent output's script_pubkey, its
        value) -> (TX_* per transaction, INPUT_* per item, the ECDSA_* detail of an EVAL_FALSE item or None, the
        32-byte signature hash that was checked or None); INPUT_HOST: not a template, the caller runs the script. With
        SCRIPT_TEMPLATE_MULTISIG in `flags`, m-of-n OP_CHECKMULTISIG inputs, bare or behind pay-to-script-hash, are
        evaluated as well (script_match names the class): detail and hash are those of the last pair the walk checked"""
        ntx, n = len(txs), len(items)
        arena, tx_off, branch, item_tx, index, prev, prev_off, amount = pack_inputs_verify(txs, branch_ids, items)
        ts = ctypes.create_string_buffer(max(ntx, 1))
        st = ctypes.create_string_buffer(max(n, 1))
        dt = ctypes.create_string_buffer(max(n, 1)) if want_detail else None
        hs = ctypes.create_string_buffer(max(32 * n, 1)) if want_hashes else None
        self._chk(lib().zg_inputs_verify(self._p, ntx, arena + b"\0", tx_off, branch, n, item_tx, index, prev + b"\0",
                                         prev_off, amount, flags, ts, st, dt, hs))
        return (list(ts.raw[:ntx]), list(st.raw[:n]), list(dt.raw[:n]) if want_detail else None,
                [hs.raw[32 * i:32 * i + 32] for i in range(n)] if want_hashes else None)

    def shielded_verify(self, txs, branch_ids, want_hashes=True, want_desc=True, phgr=False, flags=None):
        """JoinSplitVerification::check and SaplingProof::check (verification/src/accept_transaction.rs:575-596,
        649-657,707-714) of every transaction of a window from its serialized bytes, ONE call -> (TX_* per transaction,
        SHTX_* per transaction: the reference's first error, the failing description's index in its list, the SHD_*
        inner class, the 32-byte no-input signature hash of a v4 transaction (zero otherwise) or None, per
        transaction the list of its descriptions' own SHD_* classes (JoinSplits, spends, outputs) or None).
        SHTX_HOST: PHGR JoinSplits, the caller keeps pghr13_verify and ed25519_verify for it. phgr=True
        (SHIELDED_PHGR, zg_shielded_verify_flags): those transactions are checked in the call as well, the Ed25519
        signature, then Pghr13Proof::from_raw and verify per description (SHD_JOINSPLIT_ENCODING,
        SHD_JOINSPLIT_PGHR_PROOF), with their hashes and descriptions returned as a v4 transaction's. flags: the raw
        flag word instead"""
        if flags is None:
            flags = SHIELDED_PHGR if phgr else 0
        ntx = len(txs)
        arena, tx_off, branch = pack_shielded(txs, branch_ids)
        ts = ctypes.create_string_buffer(max(ntx, 1))
        st = ctypes.create_string_buffer(max(ntx, 1))
        dt = ctypes.create_string_buffer(max(ntx, 1))
        ix = (ctypes.c_uint64 * max(ntx, 1))()
        hs = ctypes.create_string_buffer(max(32 * ntx, 1)) if want_hashes else None
        doff = (ctypes.c_uint64 * (ntx + 1))() if want_desc else None
        # a description takes at least 384 bytes of its transaction
        ds = ctypes.create_string_buffer(len(arena) // 384 + 1) if want_desc else None
        if flags:
            self._chk(lib().zg_shielded_verify_flags(self._p, ntx, arena + b"\0", tx_off, branch, flags, ts, st, ix, dt, hs,
                                                     doff, ds))
        else:
            self._chk(lib().zg_shielded_verify(self._p, ntx, arena + b"\0", tx_off, branch, ts, st, ix, dt, hs, doff, ds))
        return (list(ts.raw[:ntx]), list(st.raw[:ntx]), list(ix[:ntx]), list(dt.raw[:ntx]),
                [hs.raw[32 * i:32 * i + 32] for i in range(ntx)] if want_hashes else None,
                [list(ds.raw[doff[t]:doff[t + 1]]) for t in range(ntx)] if want_desc else None)

    def txids(self, slices=None, arena=None, offsets=None):
        """dhash256 of each byte string (IndexedTransaction::hash), ONE call -> 32-byte hashes in H256 storage
        order. Either a list of byte strings, or one arena and the n + 1 offsets of its slices"""
        if arena is None:
            arena, off = pack_slices(slices)
            n = len(slices)
        else:
            n = len(offsets) - 1
            off = (ctypes.c_uint64 * (n + 1))(*offsets)
        hs = ctypes.create_string_buffer(max(32 * n, 1))
        self._chk(lib().zg_txids(self._p, n, bytes(arena) + b"\0", off, hs))
        return [hs.raw[32 * i:32 * i + 32] for i in range(n)]

    def blocks_verify(self, blocks, max_block_size, max_block_sigops, txid_cap=None, want_ids=True):
        """BlockVerifier::check (verification/src/verify_block.rs:31-40) over serialized blocks, ONE call ->
        (statuses BLK_*, flags BLK_F_* masks, details, merkle roots, cumulative transaction counts, ids per
        block). txid_cap: the capacity of the id buffer in transactions (default: sized by a first call when the
        window needs more than the blocks' bytes allow for); a window that exceeds an explicit txid_cap raises
        ZgError(E_NOMEM) whose `counts` holds the cumulative counts"""
        n = len(blocks)
        arena, off = pack_slices(blocks)
        st = ctypes.create_string_buffer(max(n, 1))
        fl = ctypes.create_string_buffer(max(n, 1))
        det = (ctypes.c_uint64 * max(n, 1))()
        roots = ctypes.create_string_buffer(max(32 * n, 1))
        cnt = (ctypes.c_uint64 * (n + 1))()
        cap = txid_cap if txid_cap is not None else len(arena) // 10 + 1   # no transaction is shorter than 10 bytes
        ids = ctypes.create_string_buffer(max(32 * cap, 1)) if want_ids else None
        rc = lib().zg_blocks_verify(self._p, n, arena + b"\0", off, max_block_size, max_block_sigops, cap, st, fl, det,
                                    roots, cnt, ids)
        if rc == E_NOMEM:
            e = ZgError(rc, "blocks_verify: %d transactions, capacity %d" % (cnt[n], cap))
            e.counts = list(cnt)
            raise e
        self._chk(rc)
        counts = list(cnt)
        per_block = [[ids.raw[32 * r:32 * r + 32] for r in range(counts[b], counts[b + 1])] for b in range(n)] \
            if want_ids else None
        return (list(st.raw[:n]), list(fl.raw[:n]), list(det)[:n], [roots.raw[32 * b:32 * b + 32] for b in range(n)],
                counts, per_block)

    def last_sig_kernel_ms(self):
        """device time of the kernel(s) of the last ed25519_verify / ecdsa_verify / redjubjub_verify /
        equihash_verify / headers_verify / sighash call"""
        ms = ctypes.c_float(0)
        self._chk(lib().zg_last_sig_kernel_ms(self._p, ctypes.byref(ms)))
        return ms.value

    def sapling_bvk(self, txs):
        """txs: list of (spend cvs, output cvs, value_balance) -> list of (status, bvk bytes)"""
        n = len(txs)
        ns = (ctypes.c_uint32 * max(n, 1))(*[len(t[0]) for t in txs])
        no = (ctypes.c_uint32 * max(n, 1))(*[len(t[1]) for t in txs])
        vb = (ctypes.c_int64 * max(n, 1))(*[t[2] for t in txs])
        cvs = b"".join(b"".join(map(bytes, t[0])) + b"".join(map(bytes, t[1])) for t in txs)
        bvk = ctypes.create_string_buffer(max(32 * n, 1))
        st = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_sapling_bvk(self._p, n, ns, no, cvs or None, vb, bvk, st))
        return [(st.raw[i], bvk.raw[32 * i:32 * i + 32]) for i in range(n)]

    def prep_batch(self, kinds, fields):
        """zg_prep_batch: a window's public-input preparation in one call. kinds: bytes (PREP_KIND_*),
        fields: n x PREP_FIELD_BYTES (prep_fields) -> (inputs n x 288 bytes, codes bytes: ZG_PREP_*)"""
        n = len(kinds)
        if len(fields) != PREP_FIELD_BYTES * n:
            raise ZgError(-1, "fields must be n x %d bytes" % PREP_FIELD_BYTES)
        inp = ctypes.create_string_buffer(max(INPUT_STRIDE * n, 1))
        codes = ctypes.create_string_buffer(max(n, 1))
        self._chk(lib().zg_prep_batch(self._p, n, bytes(kinds), bytes(fields), inp, codes))
        return inp.raw[:INPUT_STRIDE * n], codes.raw[:n]

    def jubjub_decode(self, points):
        """edwards::Point::read + small-order check -> list of (status 0/1/2, x, y ints)"""
        n = len(points)
        st = ctypes.create_string_buffer(max(n, 1))
        xy = ctypes.create_string_buffer(max(64 * n, 1))
        self._chk(lib().zg_jubjub_decode(self._p, n, b"".join(map(bytes, points)), st, xy))
        return [(st.raw[i], int.from_bytes(xy.raw[64 * i:64 * i + 32], "little"),
                 int.from_bytes(xy.raw[64 * i + 32:64 * i + 64], "little")) for i in range(n)]

    # ---- PGHR13 Sprout proofs on BN254 (include/zg.h zg_pghr13_* / zg_bn254_pairing)
    def pghr13_vk_load_json(self, text):
        """this context's PGHR13 key (other contexts keep theirs; a failed load keeps the old one)"""
        b = text.encode() if isinstance(text, str) else bytes(text)
        self._chk(lib().zg_pghr13_vk_load_json(self._p, b, len(b)))

    def pghr13_vk_load_builtin(self):
        self._chk(lib().zg_pghr13_vk_load_builtin(self._p))

    def pghr13_verify(self, proofs, inputs, n_inputs=None, with_time=False):
        """proofs: 296-byte PHGR proofs; inputs: per proof a list of <= 9 32-byte LE BN254 Fr
        (Input::into_bn_frs) -> statuses (STATUS_*). Packed form (the ABI's own buffers): proofs a
        bytes of n * 296, inputs a bytes of n * 288 (9 slots of 32 per proof) and n_inputs given."""
        if isinstance(proofs, (bytes, bytearray)):
            n = len(proofs) // 296
            assert len(proofs) == 296 * n and len(inputs) == 288 * n and n_inputs is not None and len(n_inputs) == n
            pblob, iblob, cnt = proofs, inputs, bytes(n_inputs)
        else:
            n = len(proofs)
            rows = []
            for r in inputs:
                r = [bytes(x) for x in r]
                assert len(r) <= 9
                rows.append(b"".join(r) + bytes(32 * (9 - len(r))))
            cnt = bytes(len(r) for r in inputs) if n_inputs is None else bytes(n_inputs)
            pblob, iblob = b"".join(map(bytes, proofs)), b"".join(rows)
        st = ctypes.create_string_buffer(max(n, 1))
        ms = ctypes.c_float(0)
        self._chk(lib().zg_pghr13_verify(self._p, n, pblob, iblob, cnt, st, ctypes.byref(ms)))
        out = list(st.raw[:n])
        return (out, ms.value) if with_time else out

    def pghr13_shape(self, n):
        """what pghr13_verify of n proofs would launch on this context (include/zg.h zg_pghr13_shape;
        nothing runs): {"straus_b", "bseg_k", "chunk", "halves", "p7_side"}, B / K / halves / p7_side
        of the first chunk. ZG_STRAUS_B, ZG_BSEG_K and ZG_PGHR_CHUNK are read when the context is created."""
        b, k, h, p7 = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        ch = ctypes.c_size_t(0)
        self._chk(lib().zg_pghr13_shape(self._p, n, ctypes.byref(b), ctypes.byref(k), ctypes.byref(ch),
                                        ctypes.byref(h), ctypes.byref(p7)))
        return {"straus_b": b.value, "bseg_k": k.value, "chunk": ch.value, "halves": h.value, "p7_side": p7.value}

    def bn254_pairing(self, g1s, g2s):
        """device pairing (tests): g1 (x, y) ints, g2 ((x0, x1), (y0, y1)) -> 12 ints per GT"""
        n = len(g1s)
        a = b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for x, y in g1s)
        b = b"".join(q[0][0].to_bytes(32, "little") + q[0][1].to_bytes(32, "little") +
                     q[1][0].to_bytes(32, "little") + q[1][1].to_bytes(32, "little") for q in g2s)
        out = ctypes.create_string_buffer(max(384 * n, 1))
        self._chk(lib().zg_bn254_pairing(self._p, n, a, b, out))
        return [[int.from_bytes(out.raw[384 * i + 32 * k:384 * i + 32 * k + 32], "little") for k in range(12)]
                for i in range(n)]

    # ---- note-commitment trees (include/zg.h zg_merkle_combine / zg_tree_*)
    def merkle_combine(self, kind, lefts, rights, depths=None):
        """TreeHash::combine on the GPU: [combine(l, r, depth)] as 32-byte strings"""
        n = len(lefts)
        assert len(rights) == n and (depths is None or len(depths) == n)
        out = ctypes.create_string_buffer(max(32 * n, 1))
        d = None if depths is None else bytes(depths)
        self._chk(lib().zg_merkle_combine(self._p, kind, n, b"".join(map(bytes, lefts)),
                                          b"".join(map(bytes, rights)), d, out))
        return [out.raw[32 * j:32 * j + 32] for j in range(n)]

    def tree_empty_roots(self, kind, levels=64):
        """H::empty()[0..levels)"""
        out = ctypes.create_string_buffer(32 * levels)
        self._chk(lib().zg_tree_empty_roots(self._p, kind, levels, out))
        return [out.raw[32 * j:32 * j + 32] for j in range(levels)]

    def tree_roots(self, kind, height, state, leaves, marks, want_state=True, device_leaves=None,
                   with_time=False):
        """(roots after each marks[k] appended leaves, serialized final state or None).
        state: the reference's serialized TreeState (b"" = new tree). device_leaves: a device
        pointer holding the leaves (len(leaves) is then the count, an int). Raises ZgError
        with code E_TREE_FULL past the capacity (the partial roots are on the exception)."""
        state = bytes(state or b"")
        nm = len(marks)
        mk = (ctypes.c_uint64 * max(nm, 1))(*marks)
        roots = ctypes.create_string_buffer(max(32 * nm, 1))
        cap = lib().zg_tree_state_max_bytes(height)
        so = ctypes.create_string_buffer(cap) if want_state else None
        slen = ctypes.c_size_t(cap)
        ms = ctypes.c_float(0)
        if device_leaves is None:
            n = len(leaves)
            rc = lib().zg_tree_roots(self._p, kind, height, state, len(state), n, b"".join(map(bytes, leaves)),
                                     nm, mk, roots, so, ctypes.byref(slen))
        else:
            n = int(leaves)
            rc = lib().zg_tree_roots_device(self._p, kind, height, state, len(state), n,
                                            ctypes.c_void_p(device_leaves), nm, mk, roots, so,
                                            ctypes.byref(slen), ctypes.byref(ms))
        rl = [roots.raw[32 * j:32 * j + 32] for j in range(nm)]
        if rc:
            e = ZgError(rc, lib().zg_last_error(self._p).decode(errors="replace"))
            e.roots = rl
            raise e
        st = so.raw[:slen.value] if want_state else None
        return (rl, st, ms.value) if with_time else (rl, st)

    def chacha20_blocks(self, key, nonce, counter, nblocks):
        """the device ChaCha20 keystream (the batch-scalar CSPRNG), nblocks x 64 bytes"""
        assert len(key) == 32 and len(nonce) == 12
        out = ctypes.create_string_buffer(64 * max(nblocks, 1))
        self._chk(lib().zg_chacha20_blocks(self._p, bytes(key), bytes(nonce), counter, nblocks, out))
        return out.raw[:64 * nblocks]

    def bench_mad_rate(self, with_clock=False):
        """v_mad_u64_u32 MACs/s of the probe; with_clock: (rate, shader clock in Hz)"""
        v, hz = ctypes.c_double(0), ctypes.c_double(0)
        self._chk(lib().zg_bench_mad_rate_clock(self._p, ctypes.byref(v), ctypes.byref(hz)))
        return (v.value, hz.value) if with_clock else v.value
