"""Synthesized transactions and items for the signature-hash tests (tests/test_sighash.py on the host build,
tests/test_gpu_sighash.py on the GPU): a serializer for the four transaction formats and the named case lists.
A case list is (txs, branch_ids, items), items as Context.sighash takes them: (transaction number, input index
or None, script code, amount, hashtype). Expected values always come from tests/sighash_ref.py."""
import random

from tests import sighash_ref as R
from tests.conftest import load_golden

SAPLING_BRANCH, OVERWINTER_BRANCH = 0x76B809BB, 0x5BA81B19
HASHTYPE_CLASSES = (1, 2, 3, 0x81, 0x82, 0x83)
COMPACT_TAGS = ("in_count", "in_script", "out_count", "out_script", "spend_count", "sout_count", "js_count")


def long_form(form):
    """a compact-size encoder that writes every value in the 0xfd / 0xfe / 0xff form, minimal or not"""
    width = {0xFD: 2, 0xFE: 4, 0xFF: 8}[form]
    return lambda n: bytes([form]) + n.to_bytes(width, "little")


def make_tx(fmt, n_in, n_out, n_js=0, n_spend=0, n_sout=0, seed=0, enc=None, max_script=40):
    """fmt: 'v1', 'v2' (Sprout), 'overwinter', 'sapling'. enc: {tag: encoder} for the compact sizes of
    COMPACT_TAGS that are not to be minimal (the first input / output script only)."""
    rnd = random.Random("%s/%d/%d/%d/%d/%d/%d" % (fmt, n_in, n_out, n_js, n_spend, n_sout, seed))
    enc = enc or {}

    def cs(tag, n, first=True):
        return enc[tag](n) if tag in enc and first else R.compact(n)

    ow = fmt in ("overwinter", "sapling")
    s = {"v1": (1).to_bytes(4, "little"), "v2": (2).to_bytes(4, "little"),
         "overwinter": (0x80000003).to_bytes(4, "little") + R.OVERWINTER_VGID.to_bytes(4, "little"),
         "sapling": (0x80000004).to_bytes(4, "little") + R.SAPLING_VGID.to_bytes(4, "little")}[fmt]
    s += cs("in_count", n_in)
    for i in range(n_in):
        script = rnd.randbytes(rnd.randrange(max_script + 1))
        s += rnd.randbytes(36) + cs("in_script", len(script), i == 0) + script + rnd.randbytes(4)
    s += cs("out_count", n_out)
    for i in range(n_out):
        script = rnd.randbytes(rnd.randrange(max_script + 1))
        s += rnd.randbytes(8) + cs("out_script", len(script), i == 0) + script
    s += rnd.randbytes(4)
    if ow:
        s += rnd.randbytes(4)
    if fmt == "sapling":
        s += rnd.randbytes(8) + cs("spend_count", n_spend) + rnd.randbytes(384 * n_spend)
        s += cs("sout_count", n_sout) + rnd.randbytes(948 * n_sout)
    else:
        assert not (n_spend or n_sout)
    if fmt != "v1":
        s += cs("js_count", n_js) + rnd.randbytes((1698 if fmt == "sapling" else 1802) * n_js)
        if n_js:
            s += rnd.randbytes(32 + 64)
    else:
        assert not n_js
    if n_spend or n_sout:
        s += rnd.randbytes(64)
    return s


def small_txs():
    """one small transaction per signature version (Sprout, Overwinter, Sapling)"""
    return [make_tx("v2", 2, 2, seed=1), make_tx("overwinter", 2, 2, seed=1), make_tx("sapling", 2, 2, seed=1)]


def branches(txs):
    return [{0: 0, 1: OVERWINTER_BRANCH, 2: SAPLING_BRANCH}[(R.parse(t)[1] or {"sigver": 0})["sigver"]] for t in txs]


def fixture_cases():
    """every vector of tests/golden/sighash.json as one call"""
    g = load_golden("sighash.json")
    txs, br, items, seen = [], [], [], {}

    def add(tx_hex, branch, index, script_hex, amount, hashtype):
        if (tx_hex, branch) not in seen:
            seen[(tx_hex, branch)] = len(txs)
            txs.append(bytes.fromhex(tx_hex))
            br.append(branch)
        items.append((seen[(tx_hex, branch)], index, bytes.fromhex(script_hex), amount, hashtype))

    expected = []
    for v in g["vectors"] + g["sapling_spends"]:
        add(v["tx"], v["branch_id"], v["input_index"], v["script"], v["amount"], v["hashtype"])
        expected.append(bytes.fromhex(v["sighash"]))
    for v in g["legacy"]:
        add(v["tx"], 0, v["input_index"], v["script"], 0, v["hashtype"])
        expected.append(bytes.fromhex(v["sighash"]))
    for v in g["joinsplit"] + g["sapling"]:
        add(v["tx"], v["branch_id"], None, "", 0, 1)
        expected.append(bytes.fromhex(v["sighash"]))
    return txs, br, items, expected


def block_edge_sweep():
    """per signature version, every hashtype class, script codes of every length 0..300: the final stream walks
    through every residue mod 64 and mod 128, the padding edges, and the compact-size step 252 -> 253"""
    txs = small_txs()
    rnd = random.Random(300)
    code = rnd.randbytes(300)
    items = [(t, 1, code[:k], 1000 + k, ht) for t in range(3) for ht in HASHTYPE_CLASSES for k in range(301)]
    return txs, branches(txs), items


def count_edges():
    txs = [make_tx("overwinter", 0, 0), make_tx("sapling", 0, 0), make_tx("overwinter", 1, 1), make_tx("v2", 1, 1),
           make_tx("v2", 253, 253, max_script=12), make_tx("sapling", 253, 253, max_script=12), make_tx("v1", 0, 0)]
    items = [(t, None, b"", 0, ht) for t in (0, 1, 6) for ht in HASHTYPE_CLASSES]
    items += [(t, 0, b"\x51" * 25, 7, ht) for t in (2, 3) for ht in HASHTYPE_CLASSES]
    for t in (4, 5):
        items += [(t, i, bytes([i & 0xFF]) * (i % 30), i, HASHTYPE_CLASSES[i % 6]) for i in range(253)]
    return txs, branches(txs), items


def sprout_edges():
    txs = [make_tx("v2", 3, 2, seed=2), make_tx("v1", 2, 2, seed=2), make_tx("v2", 2, 2, n_js=0, seed=3),
           make_tx("v2", 2, 1, n_js=2, seed=2)]
    code = b"\x76\xa9\x14" + bytes(range(20)) + b"\x88\xac"
    items = []
    for t in range(4):
        items += [(t, None, code, 5, ht) for ht in (1, 2, 3, 0x81, 0x82, 0x83, 0, 0x1F)]      # None: the JoinSplit path
        items += [(t, 5, code, 5, ht) for ht in (1, 2, 3, 0x81, 0x82, 0x83)]                  # index >= inputs
        items += [(t, i, code, 5, ht) for i in range(2) for ht in (0, 4, 0x1F, 0x22, 0x80, 0xFFFFFF82) + HASHTYPE_CLASSES]
    items += [(0, 2, code, 0, ht) for ht in (3, 0x83, 1, 2)]          # Single with inputs > index >= outputs
    items += [(3, 1, code, 0, ht) for ht in (3, 0x83)]
    return txs, branches(txs), items


def sapling_edges():
    txs = [make_tx("sapling", 2, 2, n_spend=2, seed=4), make_tx("sapling", 2, 2, n_sout=2, seed=4),
           make_tx("sapling", 2, 2, seed=4), make_tx("sapling", 3, 1, n_js=1, n_spend=1, n_sout=1, seed=4),
           make_tx("overwinter", 3, 1, n_js=2, seed=4), make_tx("overwinter", 2, 2, seed=4)]
    code = b"\xa9\x14" + bytes(range(20)) + b"\x87"
    items = []
    for t in range(6):
        items += [(t, None, b"", 0, ht) for ht in HASHTYPE_CLASSES]
        items += [(t, i, code, 12345678901234 + i, ht) for i in range(2) for ht in HASHTYPE_CLASSES + (0, 0x1F, 0xFFFFFF82)]
    items += [(t, 2, code, 9, ht) for t in (3, 4) for ht in (3, 0x83, 1)]      # Single with index >= outputs
    items += [(t, n, code, 9, ht) for t, n in ((0, 2), (3, 3), (5, 1000), (2, 0xFFFFFFFE)) for ht in (1, 3, 0x81)]
    return txs, branches(txs), items                                          # ... and index >= inputs: status 3


def status_plumbing():
    """one malformed and one non-canonical transaction among good ones"""
    good = small_txs()
    bad = make_tx("sapling", 2, 2, n_spend=1, seed=5)[:-1]
    nonc = make_tx("v2", 2, 2, seed=5, enc={"out_script": long_form(0xFD)})
    txs = [good[0], bad, good[1], nonc, good[2]]
    code = b"\x51" * 30
    items = [(t, i, code, 3, ht) for ht in (1, 0x83) for i in (0, None, 1) for t in range(5)]
    return txs, [0, SAPLING_BRANCH, OVERWINTER_BRANCH, 0, SAPLING_BRANCH], items


SYNTHESIZED = {"block_edge_sweep": block_edge_sweep, "count_edges": count_edges, "sprout_edges": sprout_edges,
               "sapling_edges": sapling_edges, "status_plumbing": status_plumbing}
_CACHE = {}


def case(name):
    """(txs, branch_ids, items, reference result) of a synthesized case list, computed once"""
    if name not in _CACHE:
        txs, br, items = SYNTHESIZED[name]()
        _CACHE[name] = (txs, br, items, R.run(txs, br, items))
    return _CACHE[name]
