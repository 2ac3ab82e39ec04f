"""Test reference (CPU) for zg_shielded_verify_flags, independent of the library. With flags = 0 it is
tests/shielded_ref.run. With ZG_SHIELDED_PHGR a transaction before v4 with JoinSplits gets
JoinSplitVerification::check and JoinSplitProof::check (verification/src/accept_transaction.rs:575-596,649-657) on the
PHGR branch of sprout::verify (verification/src/sprout.rs:34-68), composed from

  * tests/sighash_ref: the layout and the no-input hash (the Sprout form, or ZIP-143 for v3);
  * tests/ed25519_ref.verify: the JoinSplit signature;
  * oracle.pghr13.joinsplit_inputs: the nine BN254 inputs (Input::into_bn_frs);
  * the oracle's verdicts recorded in tests/golden/phgr_txs.json by tests/golden/gen_phgr_txs.py, and for a
    (proof, inputs) pair that is not there oracle.pghr13.verify_raw itself (about 1.2 s for a proof that decodes).

run(txs, branch_ids, flags) returns what Context.shielded_verify(txs, branch_ids, flags=flags) returns."""
import os

from oracle import pghr13 as PG
from tests import ed25519_ref
from tests import shielded_ref as S
from tests import sighash_ref as R
from tests.conftest import ROOT, load_golden

SHIELDED_PHGR = 1
SHD_JOINSPLIT_PGHR_PROOF = 20
PROOF_AT, PROOF_BYTES = 304, 296

_verdicts = None
_vk = None
_txs = {}


def fr_hex(inputs):
    return tuple(x.to_bytes(32, "little").hex() for x in inputs)


def oracle_status(proof, inputs):
    global _vk
    if _vk is None:
        _vk = PG.load_vk_json(open(os.path.join(ROOT, "zebra_amd", "res", "sprout-verifying-key.json")).read())
    return PG.verify_raw(_vk, bytes(proof), list(inputs))


def pghr_status(proof, inputs):
    """ZG_STATUS_* of one PHGR proof against its nine inputs (integers): recorded, else by the oracle"""
    global _verdicts
    if _verdicts is None:
        try:
            _verdicts = {(v["proof"], tuple(v["inputs"])): v["status"] for v in load_golden("phgr_txs.json")["verdicts"]}
        except OSError:
            _verdicts = {}
    key = (bytes(proof).hex(), fr_hex(inputs))
    if key not in _verdicts:
        _verdicts[key] = oracle_status(proof, inputs)
    return _verdicts[key]


def fields(d):
    """a serialized PHGR JoinSplit description (chain/src/join_split.rs:51-66, 1802 bytes) -> (oracle desc, proof)"""
    return S.joinsplit_fields(d)[0], d[PROOF_AT:PROOF_AT + PROOF_BYTES]


def pairs(raw):
    """the (proof, inputs) of a transaction's PHGR descriptions"""
    st, t = R.parse(raw)
    if st != R.TX_OK or t["sigver"] == 2:
        return []
    out = []
    for d in t["joinsplits"]:
        desc, proof = fields(d)
        out.append((proof, PG.joinsplit_inputs(desc, t["js_pubkey"])))
    return out


def desc_class(st):
    """ZG_STATUS_INPUT_NONCANONICAL cannot occur (253-bit chunks): anything but OK and DECODE_INVALID is the proof's"""
    return S.SHD_OK if st == 0 else S.SHD_JOINSPLIT_ENCODING if st == 1 else SHD_JOINSPLIT_PGHR_PROOF


def parts(raw, branch_id):
    """for a transaction before v4 with JoinSplits, what the kernels around the gather and the fold compute: the hash,
    the Ed25519 verdict and row, per description (proof bytes, the 288-byte input row, ZG_STATUS_*)"""
    st, t = R.parse(raw)
    assert st == R.TX_OK and t["sigver"] != 2 and t["joinsplits"]
    h = R.sighash_parsed(t, None, b"", 0, 1, branch_id)
    descs = [(p, b"".join(x.to_bytes(32, "little") for x in inp), pghr_status(p, inp)) for p, inp in pairs(raw)]
    return {"hash": h, "ed": ed25519_ref.verify(t["js_pubkey"], t["js_sig"], h),
            "ed_row": t["js_pubkey"] + t["js_sig"] + h, "descs": descs}


def verify_tx(raw, branch_id, flags=SHIELDED_PHGR):
    """-> (TX_*, SHTX_*, index, SHD_*, hash, [SHD_* per description])"""
    if flags & ~SHIELDED_PHGR:
        raise ValueError("unknown flag")
    base = S.verify_tx(raw, branch_id)
    if not flags & SHIELDED_PHGR or base[1] != S.SHTX_HOST:
        return base
    key = (bytes(raw), branch_id)
    if key not in _txs:
        p = parts(raw, branch_id)
        js = [desc_class(d[2]) for d in p["descs"]]
        first = (S.SHTX_OK, 0, S.SHD_OK)
        if p["ed"]:
            first = (S.SHTX_JOINSPLIT_SIGNATURE, 0, S.SHD_ED_PUBLIC_ENCODING - 1 + p["ed"])
        for i, c in enumerate(js):
            if c and first[0] == S.SHTX_OK:
                first = (S.SHTX_INVALID_JOINSPLIT, i, c)
        _txs[key] = (base[0],) + first + (p["hash"], js)
    return _txs[key]


def run(txs, branch_ids, flags=SHIELDED_PHGR):
    """the reference result of Context.shielded_verify(txs, branch_ids, flags=flags)"""
    if not flags:
        return S.run(txs, branch_ids)
    rows = [verify_tx(raw, b, flags) for raw, b in zip(txs, branch_ids)]
    return tuple([r[k] for r in rows] for k in range(6))
