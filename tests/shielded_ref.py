"""Test reference (CPU) for zg_shielded_verify, independent of the library: JoinSplitVerification::check and
SaplingProof::check (verification/src/accept_transaction.rs:575-596,649-657,707-714) of serialized transactions,
composed from the parts that are already pinned on the reference's vectors:

  * tests/sighash_ref.parse and sighash: the layout and the no-input hash (accept_transaction.rs:374-387);
  * oracle.zcash spend_inputs / output_inputs / sprout_inputs: the public inputs and their error classes;
  * oracle.sapling_sig spend_auth_ok / binding_sig_ok: RedJubjub (sapling.rs:119-137,216-244);
  * tests/ed25519_ref.verify: the JoinSplit signature (crypto/src/lib.rs:298-305);
  * tests/cpulib.verify: the proofs, by the C++ restatement of bellman's verify_proof.

run(txs, branch_ids) returns what Context.shielded_verify returns. Results are cached per (transaction, branch id):
the lists of tests/shielded_cases.py repeat the same transactions many times."""
import functools

from oracle import sapling_sig, zcash
from tests import cpulib, ed25519_ref
from tests import sighash_ref as R

(SHTX_OK, SHTX_NONE, SHTX_JOINSPLIT_SIGNATURE, SHTX_INVALID_JOINSPLIT, SHTX_INVALID_SAPLING, SHTX_HOST,
 SHTX_TX_MALFORMED, SHTX_TX_NONCANONICAL) = range(8)
(SHD_OK, SHD_VALUE_COMMITMENT_INVALID, SHD_VALUE_COMMITMENT_SMALL_ORDER, SHD_ANCHOR, SHD_RANDOMIZED_KEY_INVALID,
 SHD_RANDOMIZED_KEY_SMALL_ORDER, SHD_NOTE_COMMITMENT, SHD_EPHEMERAL_KEY_INVALID, SHD_EPHEMERAL_KEY_SMALL_ORDER,
 SHD_SPEND_AUTH_SIG, SHD_PROOF_INVALID, SHD_PROOF_SYNTHESIS, SHD_PROOF_FAILED, SHD_BALANCE_VALUE,
 SHD_BINDING_SIGNATURE, SHD_JOINSPLIT_ENCODING, SHD_JOINSPLIT_PROOF, SHD_ED_PUBLIC_ENCODING,
 SHD_ED_SIGNATURE_ENCODING, SHD_ED_SIGNATURE) = range(20)
SHTX_NAMES = ("OK", "NONE", "JOINSPLIT_SIGNATURE", "INVALID_JOINSPLIT", "INVALID_SAPLING", "HOST", "TX_MALFORMED",
              "TX_NONCANONICAL")
# ProofError::Synthesis needs a key whose input count differs from the circuit's: not reachable with the built-in keys
SHD_UNREACHABLE = (SHD_PROOF_SYNTHESIS,)
PREP_CLASS = {"ValueCommitment(Invalid)": SHD_VALUE_COMMITMENT_INVALID,
              "ValueCommitment(SmallOrder)": SHD_VALUE_COMMITMENT_SMALL_ORDER, "Anchor": SHD_ANCHOR,
              "RandomizedKey(Invalid)": SHD_RANDOMIZED_KEY_INVALID,
              "RandomizedKey(SmallOrder)": SHD_RANDOMIZED_KEY_SMALL_ORDER, "NoteCommitment": SHD_NOTE_COMMITMENT,
              "EphemeralKey(Invalid)": SHD_EPHEMERAL_KEY_INVALID, "EphemeralKey(SmallOrder)": SHD_EPHEMERAL_KEY_SMALL_ORDER}
KIND_SPEND, KIND_OUTPUT, KIND_SPROUT = 0, 1, 2
ZERO = b"\x00" * 32

_cpu = None
_proofs = {}
_txs = {}


def _fr(xs):
    return b"".join(x.to_bytes(32, "little") for x in xs)


def proof_status(kind, proof, inputs):
    """ZG_STATUS_* of one proof against its public inputs (a list of integers), cached"""
    global _cpu
    key = (kind, bytes(proof), tuple(inputs))
    if key not in _proofs:
        if _cpu is None:
            _cpu = cpulib.load()
        row = _fr(inputs).ljust(288, b"\x00")
        _proofs[key] = cpulib.verify(_cpu, bytes(proof), bytes([kind]), row, bytes([len(inputs)]))[0][0]
    return _proofs[key]


def joinsplit_fields(d):
    """a serialized Groth JoinSplit description (chain/src/join_split.rs:51-66) -> (oracle.zcash desc, proof)"""
    return ({"vpub_old": int.from_bytes(d[0:8], "little"), "vpub_new": int.from_bytes(d[8:16], "little"),
             "anchor": d[16:48], "nullifiers": [d[48:80], d[80:112]], "commitments": [d[112:144], d[144:176]],
             "random_seed": d[208:240], "macs": [d[240:272], d[272:304]]}, d[304:496])


@functools.lru_cache(maxsize=None)
def joinsplit_status(d, pubkey):
    desc, proof = joinsplit_fields(d)
    st = proof_status(KIND_SPROUT, proof, zcash.sprout_inputs(desc, pubkey))
    return SHD_OK if st == 0 else SHD_JOINSPLIT_ENCODING if st == 1 else SHD_JOINSPLIT_PROOF


def _proof_class(st):
    return {0: SHD_OK, 1: SHD_PROOF_INVALID, 2: SHD_PROOF_SYNTHESIS, 3: SHD_PROOF_FAILED}[st]


@functools.lru_cache(maxsize=None)
def spend_status(s, sighash):
    """accept_spend (sapling.rs:101-169): cv, anchor, rk, spend_auth_sig, proof"""
    try:
        inputs = zcash.spend_inputs(s[0:32], s[32:64], s[64:96], s[96:128])
    except zcash.InputError as e:
        return PREP_CLASS[e.where]
    if not sapling_sig.spend_auth_ok(s[96:128], sighash, s[320:384]):
        return SHD_SPEND_AUTH_SIG
    return _proof_class(proof_status(KIND_SPEND, s[128:320], inputs))


@functools.lru_cache(maxsize=None)
def output_status(o):
    """accept_output (sapling.rs:171-214): cv, cmu, epk, proof"""
    try:
        inputs = zcash.output_inputs(o[0:32], o[32:64], o[64:96])
    except zcash.InputError as e:
        return PREP_CLASS[e.where]
    return _proof_class(proof_status(KIND_OUTPUT, o[756:948], inputs))


def verify_tx(raw, branch_id):
    """-> (TX_*, SHTX_*, index, SHD_*, hash, [SHD_* per description])"""
    key = (bytes(raw), branch_id)
    if key in _txs:
        return _txs[key]
    st, t = R.parse(raw)
    if st != R.TX_OK:
        res = (st, SHTX_TX_MALFORMED if st == R.TX_MALFORMED else SHTX_TX_NONCANONICAL, 0, 0, ZERO, [])
    elif t["sigver"] != 2:
        res = (st, SHTX_HOST if t["joinsplits"] else SHTX_NONE, 0, 0, ZERO, [])
    else:
        h = R.sighash_parsed(t, None, b"", 0, 1, branch_id)
        js = [joinsplit_status(d, t["js_pubkey"]) for d in t["joinsplits"]]
        sp = [spend_status(s, h) for s in t["spends"]]
        out = [output_status(o) for o in t["soutputs"]]
        first = (SHTX_OK, 0, SHD_OK)
        ed = ed25519_ref.verify(t["js_pubkey"], t["js_sig"], h) if t["joinsplits"] else 0
        if ed:
            first = (SHTX_JOINSPLIT_SIGNATURE, 0, SHD_ED_PUBLIC_ENCODING - 1 + ed)
        for status, lst in ((SHTX_INVALID_JOINSPLIT, js), (SHTX_INVALID_SAPLING, sp), (SHTX_INVALID_SAPLING, out)):
            for i, c in enumerate(lst):
                if c and first[0] == SHTX_OK:
                    first = (status, i, c)
        if first[0] == SHTX_OK:
            # sapling = Some for every v4 transaction (chain/src/transaction.rs:291-303): without spends and outputs
            # the binding signature is the default, 64 zero bytes
            vb = int.from_bytes(t["value_balance"], "little", signed=True)
            if vb == -(1 << 63):
                first = (SHTX_INVALID_SAPLING, 0, SHD_BALANCE_VALUE)
            elif not sapling_sig.binding_sig_ok([s[0:32] for s in t["spends"]], [o[0:32] for o in t["soutputs"]], vb, h,
                                                t.get("binding_sig", bytes(64))):
                first = (SHTX_INVALID_SAPLING, 0, SHD_BINDING_SIGNATURE)
        res = (st,) + first + (h, js + sp + out)
    _txs[key] = res
    return res


def run(txs, branch_ids):
    """the reference result of Context.shielded_verify(txs, branch_ids)"""
    rows = [verify_tx(raw, b) for raw, b in zip(txs, branch_ids)]
    return tuple([r[k] for r in rows] for k in range(6))


def parts(raw, branch_id):
    """for a v4 transaction, what the kernels around the gather and the fold compute, each from its own oracle: the
    hash, the binding key as k_sapling_bvk reports it (bytes, status 1 a cv does not decode / 2 i64::MIN), the binding
    and Ed25519 verdicts and rows, and per description (kind, proof bytes, prep class, inputs row or zeros, spend_auth
    verdict, ZG_STATUS_* of the proof with the device-written input count)"""
    st, t = R.parse(raw)
    assert st == R.TX_OK and t["sigver"] == 2
    h = R.sighash_parsed(t, None, b"", 0, 1, branch_id)
    descs, rj = [], []
    for d in t["joinsplits"]:
        desc, proof = joinsplit_fields(d)
        inputs = zcash.sprout_inputs(desc, t["js_pubkey"])
        descs.append((KIND_SPROUT, proof, 0, _fr(inputs).ljust(288, b"\x00"), 1, proof_status(KIND_SPROUT, proof, inputs)))
    for s in t["spends"]:
        ok = int(sapling_sig.spend_auth_ok(s[96:128], h, s[320:384]))
        rj.append(s[96:128] + s[320:384] + s[96:128] + h + b"\x00")
        try:
            inputs = zcash.spend_inputs(s[0:32], s[32:64], s[64:96], s[96:128])
            descs.append((KIND_SPEND, s[128:320], 0, _fr(inputs).ljust(288, b"\x00"), ok,
                          proof_status(KIND_SPEND, s[128:320], inputs)))
        except zcash.InputError as e:
            descs.append((KIND_SPEND, s[128:320], PREP_CLASS[e.where], bytes(288), ok, 2))
    for o in t["soutputs"]:
        try:
            inputs = zcash.output_inputs(o[0:32], o[32:64], o[64:96])
            descs.append((KIND_OUTPUT, o[756:948], 0, _fr(inputs).ljust(288, b"\x00"), 1,
                          proof_status(KIND_OUTPUT, o[756:948], inputs)))
        except zcash.InputError as e:
            descs.append((KIND_OUTPUT, o[756:948], PREP_CLASS[e.where], bytes(288), 1, 2))
    vb = int.from_bytes(t["value_balance"], "little", signed=True)
    try:
        p = sapling_sig.binding_verification_key([s[0:32] for s in t["spends"]], [o[0:32] for o in t["soutputs"]], vb)
        bvk, bvk_st = (bytes(32), 2) if p is None else (sapling_sig.encode(p), 0)
    except zcash.PointError:
        bvk, bvk_st = bytes(32), 1
    sig = t.get("binding_sig", bytes(64))
    bind_ok = int(bvk_st == 0 and sapling_sig.redjubjub_verify(bvk, sig, bvk + h, sapling_sig.GEN_BINDING))
    ed = ed25519_ref.verify(t["js_pubkey"], t["js_sig"], h) if t["joinsplits"] else 0
    ed_row = t["js_pubkey"] + t["js_sig"] + h if t["joinsplits"] else None
    return {"hash": h, "bvk": bvk, "bvk_st": bvk_st, "bind_ok": bind_ok, "ed": ed, "ed_row": ed_row, "descs": descs,
            "rj_spends": rj, "rj_binding": bvk + sig + bvk + h + b"\x01"}
