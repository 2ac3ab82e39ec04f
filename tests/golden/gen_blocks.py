#!/usr/bin/env python3
"""Generate tests/golden/blocks.json: the fixtures of the block body checks (zg_block_layout, zg_txids,
zg_blocks_verify).

Reads the reference as TEXT only, the way gen_sighash.py does. Kept:

  * blocks: the blocks of chain/src/block.rs's test_block_parse with their stated block hash and merkle root, and
    block_h0, block_h170, block_h567 (2 transactions) and block_h522 (9 transactions: an odd row at three
    levels) of test-data/src/lib.rs, whose expectation is the header's own merkle root (bytes 36..67);
  * merkle: the two-hash vector of chain/src/merkle_root.rs:47-57;
  * sigops: the scripts of script/src/script.rs:549-583 that use sigops_count(false), with the stated counts
    (the two long ones as a recipe: a fill byte, a length, the bytes patched in).

Everything is asserted against tests/blocks_ref.py before it is written.

    python tests/golden/gen_blocks.py
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

import blocks_ref as R  # noqa: E402
from gen_golden import REF  # noqa: E402

MAX_SCRIPT_ELEMENT_SIZE = 520  # script/src/interpreter.rs / script.rs constant of the same name


def block_entry(name, raw, block_hash=None, root=None):
    st, flags, _, got_root, ids = R.verify(raw, 1 << 40, 1 << 40)
    assert st == R.BLK_OK and flags == 0, (name, st, flags)
    assert got_root == raw[36:68], name
    if root is not None:
        assert got_root == bytes.fromhex(root)[::-1], name
    if block_hash is not None:
        assert R.dhash256(raw[:R.HEADER_BYTES]) == bytes.fromhex(block_hash)[::-1], name
    _, out, off = R.layout(raw)
    return {"name": name, "raw": raw.hex(), "merkle_root": got_root.hex(), "txids": [i.hex() for i in ids],
            "layout": out, "tx_off": off}


def blocks():
    out = []
    src = open(os.path.join(REF, "chain", "src", "block.rs")).read()
    body = src[src.index("fn test_block_parse"):]
    triples = re.findall(r'"([0-9a-f]{3000,})",\s*"([0-9a-f]{64})",\s*"([0-9a-f]{64})"', body)
    assert len(triples) >= 2
    for i, (raw, h, root) in enumerate(triples):
        out.append(block_entry("block_parse_%d" % i, bytes.fromhex(raw), h, root))
    lib = open(os.path.join(REF, "test-data", "src", "lib.rs")).read()
    for name in ("block_h0", "block_h170", "block_h567", "block_h522"):
        fn = lib[lib.index("pub fn %s()" % name):]
        raw = bytes.fromhex(re.search(r'"([0-9a-f]{3000,})"', fn).group(1))
        out.append(block_entry(name, raw))
    n = {e["name"]: e["layout"][0] for e in out}
    assert n["block_h567"] == 2 and n["block_h522"] == 9, n
    sizes = [b - a for e in out if e["name"] == "block_h522" for a, b in zip(e["tx_off"], e["tx_off"][1:])]
    assert min(sizes) == 133 and max(sizes) == 3745, sizes
    return out


def merkle():
    src = open(os.path.join(REF, "chain", "src", "merkle_root.rs")).read()
    body = src[src.index("fn test_merkle_root_with_2_hashes"):]
    tx1, tx2, expected = re.findall(r'from_reversed_str\("([0-9a-f]{64})"\)', body)[:3]
    leaves = [bytes.fromhex(tx1)[::-1], bytes.fromhex(tx2)[::-1]]
    assert R.merkle_root(leaves) == bytes.fromhex(expected)[::-1]
    return [{"leaves": [x.hex() for x in leaves], "root": bytes.fromhex(expected)[::-1].hex()}]


def sigops():
    src = open(os.path.join(REF, "script", "src", "script.rs")).read()
    body = src[src.index("fn test_sigops_count()"):src.index("fn test_sigops_count_b73")]
    out = [{"hex": h, "count": int(c)}
           for c, h in re.findall(r'assert_eq!\((\d+)usize, Script::from\("([0-9a-f]+)"\)\.sigops_count\(false\)\)', body)]
    assert len(out) == 4
    cs = "ac"  # Opcode::OP_CHECKSIG
    over = MAX_SCRIPT_ELEMENT_SIZE + 1
    # test_sigops_count_b73 (:558-570) and _b74 (:573-584), max_block_sigops 20000, block_sigops 0
    out.append({"fill": cs, "len": 20000 + MAX_SCRIPT_ELEMENT_SIZE + 1 + 5 + 1,
                "patch": {"20000": "4e" + over.to_bytes(4, "little").hex()}, "count": 20001})
    out.append({"fill": cs, "len": 20000 + MAX_SCRIPT_ELEMENT_SIZE + 42, "patch": {"20001": "4efeffffff"},
                "count": 20001})
    for e in out:
        assert R.script_sigops(R.script_from_recipe(e)) == e["count"], e
    return out


def main():
    doc = {"blocks": blocks(), "merkle": merkle(), "sigops": sigops()}
    path = os.path.join(HERE, "blocks.json")
    json.dump(doc, open(path, "w"), indent=0, sort_keys=True)
    print(path, os.path.getsize(path), "bytes;", ", ".join("%s: %d transactions" % (e["name"], e["layout"][0])
                                                         for e in doc["blocks"]))


if __name__ == "__main__":
    main()
