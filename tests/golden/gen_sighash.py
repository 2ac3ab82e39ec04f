#!/usr/bin/env python3
"""Generate tests/golden/sighash.json: the fixtures of the signature hash (zg_sighash, zg_tx_layout).

Reads the reference as TEXT only, the way gen_golden.py does. Before anything is written, all 500 vectors of
script/data/sighash_tests.json (the official ZIP-143/243 vectors, run by script/src/sign.rs:576-591) are
asserted against tests/sighash_ref.py. Kept:

  * vectors: the two smallest transactions of every (signature version, base, anyone-can-pay) class the 500
    hold (Sapling Single|ACP has none: 17 classes);
  * sapling_spends: the two real Sapling-era spends of test_sighash_cache_works_correctly (sign.rs:594-643)
    with the donor output's script and amount and input 0's public key and DER signature -- the vectors above
    all have amount 0, these two verify only with the right amount;
  * legacy: the transactions behind the `real` rows of ecdsa.json (script/src/interpreter.rs:1817-1907),
    legacy (Sprout-branch) sighash;
  * joinsplit: the transactions behind the `real` rows of ed25519.json (block 419221), the JoinSplit
    signature's message (index None);
  * sapling: the transactions behind `txs` of sapling_sigs.json (sapling.rs:303-305 and block 419221).

Every expected hash comes from tests/sighash_ref.py and is checked against the reference's own expectation
where it states one (the vectors' hashes, the signatures that must verify).

    python tests/golden/gen_sighash.py
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ecdsa_ref as E  # noqa: E402
import ed25519_ref as ED  # noqa: E402
import sighash_ref as R  # noqa: E402
from gen_ecdsa import pushes  # noqa: E402
from gen_golden import REF, extract_sources  # noqa: E402

SAPLING_BRANCH = 0x76B809BB


def vectors():
    vecs = json.load(open(os.path.join(REF, "script", "data", "sighash_tests.json")))[1:]
    assert len(vecs) == 500
    classes = {}
    for v in vecs:
        raw, script = bytes.fromhex(v[0]), bytes.fromhex(v[1])
        idx = None if v[2] == (1 << 64) - 1 else v[2]
        ht = v[3] & 0xFFFFFFFF
        got, st = R.sighash(raw, idx, script, 0, ht, v[4])
        assert st == R.SIGHASH_OK and got == bytes.fromhex(v[5])[::-1], v[5]
        sigver = R.parse(raw)[1]["sigver"]
        classes.setdefault((sigver, R._base(ht), bool(ht & 0x80)), []).append(
            {"tx": v[0], "script": v[1], "input_index": idx, "hashtype": ht, "branch_id": v[4], "amount": 0,
             "sighash": got.hex()})
    assert len(classes) == 17 and (2, 3, True) not in classes, sorted(classes)
    out = []
    for key in sorted(classes):
        out += sorted(classes[key], key=lambda e: len(e["tx"]))[:2]
    return out


def sapling_spends():
    src = open(os.path.join(REF, "script", "src", "sign.rs")).read()
    body = src[src.index("fn test_sighash_cache_works_correctly"):]
    hexes = re.findall(r'"([0-9a-f]{200,})"\.into\(\)', body)
    assert len(hexes) == 4
    out = []
    for spend_hex, donor_hex in (hexes[0:2], hexes[2:4]):
        spend, donor = bytes.fromhex(spend_hex), bytes.fromhex(donor_hex)
        st, t = R.parse(spend)
        assert st == R.TX_OK and t["sigver"] == 2
        prev = t["inputs"][0]["prevout"]
        assert E.dhash256(donor) == prev[:32]
        dout = R.parse(donor)[1]["outputs"][int.from_bytes(prev[32:], "little")]
        amount, script = int.from_bytes(dout[:8], "little"), dout[9:]
        assert dout[8] == len(script) == 25   # P2PKH
        sig, pk = pushes(t["inputs"][0]["script"])
        hashtype = sig[-1]
        sh, st = R.sighash(spend, 0, script, amount, hashtype, SAPLING_BRANCH)
        assert st == R.SIGHASH_OK and E.verify(pk, sig[:-1], sh) == E.OK
        assert E.verify(pk, sig[:-1], R.sighash(spend, 0, script, 0, hashtype, SAPLING_BRANCH)[0]) == E.SIGNATURE
        out.append({"tx": spend_hex, "input_index": 0, "script": script.hex(), "amount": amount, "hashtype": hashtype,
                    "branch_id": SAPLING_BRANCH, "pubkey": pk.hex(), "sig": sig[:-1].hex(), "sighash": sh.hex()})
    assert sorted(e["hashtype"] for e in out) == [1, 3]
    return out


def legacy():
    """the transactions of the `real` rows of ecdsa.json that come from a transaction"""
    interp = open(os.path.join(REF, "script", "src", "interpreter.rs")).read()
    rows = {r["sighash"]: r for r in json.load(open(os.path.join(HERE, "ecdsa.json")))["real"]}
    out = []
    for fn in ("test_check_transaction_signature", "test_transaction_with_high_s_signature",
               "test_transaction_from_124276", "test_check_transaction_multisig",
               "test_arithmetic_correct_arguments_order"):
        body = interp[interp.index("fn %s()" % fn):]
        body = body[:body.index("\n\t}\n")]
        tx = bytes.fromhex(re.search(r'let tx: Transaction = "(\w+)"', body).group(1))
        inp = bytes.fromhex(re.search(r'let input: Script = "(\w+)"', body).group(1))
        outp = bytes.fromhex(re.search(r'let output: Script = "(\w+)"', body).group(1))
        code = pushes(inp)[-1] if fn == "test_check_transaction_multisig" else outp   # P2SH: the redeem script
        sh, st = R.sighash(tx, 0, code, 0, 1, 0)
        assert st == R.SIGHASH_OK and sh == E.legacy_sighash_all(tx, 0, code)
        row = rows[sh.hex()]
        assert row["status"] in (E.OK, E.SIGNATURE)
        out.append({"name": fn, "tx": tx.hex(), "input_index": 0, "script": code.hex(), "hashtype": 1,
                    "sighash": sh.hex(),
                    "checks": [{"pubkey": r["pubkey"], "sig": r["sig"], "status": r["status"]}
                               for r in json.load(open(os.path.join(HERE, "ecdsa.json")))["real"]
                               if r["sighash"] == sh.hex()]})
    return out


def block_txs():
    from oracle import zcash as Z
    tx_hex, _, _, block_hex, _ = extract_sources()
    raws = [("bd4fe81c", bytes.fromhex(tx_hex))]
    rd = Z._Reader(bytes.fromhex(block_hex))
    rd.take(140)
    rd.take(rd.compact())
    for _ in range(rd.compact()):
        o0 = rd.o
        t = Z.parse_tx(rd)
        raws.append((t["txid"], rd.d[o0:rd.o]))
    return raws


def shielded():
    raws = block_txs()
    ed_rows = {r["txid"]: r for r in json.load(open(os.path.join(HERE, "ed25519.json")))["real"]}
    sap_rows = {r["name"]: r for r in json.load(open(os.path.join(HERE, "sapling_sigs.json")))["txs"]}
    joinsplit, sapling = [], []
    for name, raw in raws:
        st, t = R.parse(raw)
        assert st == R.TX_OK
        sh = R.sighash(raw, None, b"", 0, 1, SAPLING_BRANCH)[0]
        if name in ed_rows:
            row = ed_rows[name]
            assert row["sighash"] == sh.hex() and ED.verify(bytes.fromhex(row["pubkey"]), bytes.fromhex(row["sig"]), sh) == 0
            joinsplit.append({"txid": name, "tx": raw.hex(), "pubkey": row["pubkey"], "sig": row["sig"],
                              "branch_id": SAPLING_BRANCH, "sighash": sh.hex()})
        if name[:8] in sap_rows:
            assert sap_rows[name[:8]]["sighash"] == sh.hex()
            sapling.append({"name": name[:8], "tx": raw.hex(), "branch_id": SAPLING_BRANCH, "sighash": sh.hex()})
    assert len(joinsplit) == len(ed_rows) and len(sapling) == len(sap_rows)
    return joinsplit, sapling


def main():
    vec = vectors()
    joinsplit, sapling = shielded()
    doc = {"comment": "generated by tests/golden/gen_sighash.py; hashes from tests/sighash_ref.py, H256 storage order",
           "vectors": vec, "sapling_spends": sapling_spends(), "legacy": legacy(), "joinsplit": joinsplit,
           "sapling": sapling}
    path = os.path.join(HERE, "sighash.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("sighash.json: %d vectors, %d sapling spends, %d legacy, %d joinsplit, %d sapling, %d bytes" % (
        len(vec), len(doc["sapling_spends"]), len(doc["legacy"]), len(joinsplit), len(sapling), os.path.getsize(path)))


if __name__ == "__main__":
    main()
