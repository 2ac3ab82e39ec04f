"""Shared inputs of tests/test_blocks.py (CPU) and tests/test_gpu_blocks.py (GPU): the fixture blocks and synthetic
blocks that fail chosen checks of BlockVerifier::check, built from a fixture header and minimal transactions."""
import itertools

from tests import blocks_ref as R
from tests.conftest import load_golden

CHECKS = {"coinbase": R.F_COINBASE, "size": R.F_SIZE, "extra": R.F_EXTRA_COINBASE, "dup": R.F_DUPLICATED,
          "sigops": R.F_SIGOPS, "merkle": R.F_MERKLE_ROOT}
BIG = 1 << 40


def fixtures():
    return [(e["name"], bytes.fromhex(e["raw"]), e) for e in load_golden("blocks.json")["blocks"]]


def header():
    return fixtures()[0][1][:R.HEADER_BYTES]


def failing(features):
    """a block that fails exactly the named checks -> (raw, max_block_size, max_block_sigops, flags)"""
    features = set(features)
    if "empty" in features:
        raw = R.make_block(header(), [])
        return raw, BIG, BIG, R.F_EMPTY | R.F_COINBASE
    txs = [R.min_tx(0, coinbase="coinbase" not in features), R.min_tx(1, out_script=b"\xae"), R.min_tx(2)]
    if "extra" in features:
        txs.append(R.min_tx(3, coinbase=True))
    if "dup" in features:
        txs.append(txs[2])
    raw = R.make_block(header(), txs, fix_root="merkle" not in features)
    flags = 0
    for f in features:
        flags |= CHECKS[f]
    return raw, len(raw) - (1 if "size" in features else 0), 19 if "sigops" in features else 20, flags


def failing_cases():
    names = [("empty",)] + [(c,) for c in CHECKS] + list(itertools.combinations(CHECKS, 2)) + [tuple(CHECKS)]
    return [(n, failing(n)) for n in [()] + names]


def synthetic(k, seed=0):
    """a good block of k minimal distinct transactions"""
    return R.make_block(header(), [R.min_tx(seed * 100000 + i, coinbase=i == 0) for i in range(k)])


def noncanonical_count(block, form):
    """the block with its (one-byte) transaction count re-encoded in a longer form: 0xfd, 0xfe or 0xff"""
    n = block[R.HEADER_BYTES]
    assert n < 0xFD
    width = {0xFD: 2, 0xFE: 4, 0xFF: 8}[form]
    return block[:R.HEADER_BYTES] + bytes([form]) + n.to_bytes(width, "little") + block[R.HEADER_BYTES + 1:]
