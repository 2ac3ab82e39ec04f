#!/usr/bin/env python3
"""Generates tests/golden/phgr_txs.json: block 522's five JoinSplit transactions as they are serialized, with what the
ZG_SHIELDED_PHGR tests expect of them, so that no test spends 1.2 s per proof on the Python pairing.

Reads the reference as TEXT only, the way gen_blocks.py does: the hex of block_h522 in test-data/src/lib.rs, which is
data its tests read. Written:
  * txs: per transaction its raw bytes, its no-input signature hash by tests/sighash_ref, the tests/ed25519_ref
    verdict of its real signature under that hash, and per description the oracle.pghr13 verdict;
  * verdicts: the oracle's verdict for every (proof, inputs) pair of the transactions tests/shielded_phgr_cases.py
    derives from them (mutated proofs, re-keyed transactions).
Asserted before writing: all five signatures verify, all six proofs are accepted, and every (proof, inputs) pair equals
the matching h522_* case of tests/golden/pghr13.json.

    python tests/golden/gen_phgr_txs.py [path to the reference checkout]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import blocks_ref, ed25519_ref  # noqa: E402
from tests import shielded_phgr_cases as C  # noqa: E402
from tests import shielded_phgr_ref as P  # noqa: E402
from tests import sighash_ref as R  # noqa: E402


def block_522(ref):
    lib = open(os.path.join(ref, "test-data", "src", "lib.rs")).read()
    fn = lib[lib.index("pub fn block_h522()"):]
    return bytes.fromhex(re.search(r'"([0-9a-f]{3000,})"', fn).group(1))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ZG_REFERENCE", os.path.join(ROOT, "..", "reference"))
    raw = block_522(ref)
    _, _, off = blocks_ref.layout(raw)
    txs = [raw[a:b] for a, b in zip(off, off[1:])]
    js = [t for t in txs if R.parse(t)[1]["joinsplits"]]
    assert len(js) == 5
    known = [c for c in json.load(open(os.path.join(HERE, "pghr13.json")))["cases"] if c["name"].startswith("h522_")]
    assert len(known) == 6
    out, verdicts, n = [], {}, 0
    for t in js:
        p = R.parse(t)[1]
        assert p["sigver"] == 0
        h = R.sighash_parsed(p, None, b"", 0, 1, 0)
        ed = ed25519_ref.verify(p["js_pubkey"], p["js_sig"], h)
        assert ed == 0, "the real signature verifies under the no-input hash"
        sts = []
        for proof, inputs in P.pairs(t):
            k = known[n]
            assert (proof.hex(), list(P.fr_hex(inputs))) == (k["proof"], k["inputs"]), k["name"]
            st = P.oracle_status(proof, inputs)
            assert st == 0 == k["status"], k["name"]
            verdicts[(proof.hex(), P.fr_hex(inputs))] = st
            sts.append(st)
            n += 1
        out.append({"raw": t.hex(), "sighash": h.hex(), "ed25519": ed, "joinsplits": sts})
    assert n == 6
    C.REAL = js
    for t in C.every_tx() + [c[1] for c in C.interleaved_cases()]:
        for proof, inputs in P.pairs(t):
            key = (proof.hex(), P.fr_hex(inputs))
            if key not in verdicts:
                verdicts[key] = P.oracle_status(proof, inputs)
    doc = {"source": "test-data/src/lib.rs block_h522: its five JoinSplit transactions; verdicts by oracle/pghr13.py",
           "txs": out,
           "verdicts": [{"proof": k[0], "inputs": list(k[1]), "status": v} for k, v in verdicts.items()]}
    path = os.path.join(HERE, "phgr_txs.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d transactions, %d verdicts, %d bytes" % (path, len(out), len(verdicts), os.path.getsize(path)))


if __name__ == "__main__":
    main()
