"""Test reference (CPU, hashlib): the block body checks (zg_block_layout, zg_txids, zg_blocks_verify), restated
independently of the library.

  * Block::deserialize (chain/src/block.rs:10-14) over one exact slice, with the statuses of the parser
    (non-minimal compact sizes are read, as the reference does, and reported);
  * dhash256 and merkle_root (chain/src/merkle_root.rs:14-38) as written: recursive, an odd row's last element
    hashed with itself, a one-element list its own root;
  * transaction_sigops(tx, NoopStore, false) (verification/src/sigops.rs:9-41) over Script::sigops_count(false)
    (script/src/script.rs:289-317), get_instruction (:199-236) and the opcode set of script/src/opcode.rs;
  * BlockVerifier::check's order (verification/src/verify_block.rs:31-40).

Hashes are the 32 bytes of the reference's H256 (storage order)."""
import hashlib

TX_OK, TX_MALFORMED, TX_NONCANONICAL = 0, 1, 2
(BLK_OK, BLK_MALFORMED, BLK_NONCANONICAL, BLK_EMPTY, BLK_COINBASE, BLK_SIZE, BLK_EXTRA_COINBASE, BLK_DUPLICATED,
 BLK_SIGOPS, BLK_MERKLE_ROOT) = range(10)
F_EMPTY, F_COINBASE, F_SIZE, F_EXTRA_COINBASE, F_DUPLICATED, F_SIGOPS, F_MERKLE_ROOT = 1, 2, 4, 8, 16, 32, 64
HEADER_BYTES = 1487
NO_INDEX = (1 << 64) - 1
OVERWINTER_VGID, SAPLING_VGID = 0x03C48270, 0x892F2085
# Opcode::from_u8: 0x00..=0xaa and 0xac..=0xb9 are Some (0xab, OP_CODESEPARATOR, is not in the table)
KNOWN_OPCODES = frozenset(range(0x00, 0xAB)) | frozenset(range(0xAC, 0xBA))


def dhash256(b):
    return hashlib.sha256(hashlib.sha256(bytes(b)).digest()).digest()


def merkle_root(hashes):
    if len(hashes) == 1:
        return hashes[0]
    row = [dhash256(hashes[i] + hashes[i + 1]) for i in range(0, len(hashes) - 1, 2)]
    if len(hashes) % 2 == 1:
        row.append(dhash256(hashes[-1] + hashes[-1]))
    return merkle_root(row)


def compact(v):
    if v < 0xFD:
        return bytes([v])
    if v <= 0xFFFF:
        return b"\xfd" + v.to_bytes(2, "little")
    if v <= 0xFFFFFFFF:
        return b"\xfe" + v.to_bytes(4, "little")
    return b"\xff" + v.to_bytes(8, "little")


class Malformed(Exception):
    pass


class Reader:
    def __init__(self, d, o=0):
        self.d, self.o, self.excess = d, o, 0

    def left(self):
        return len(self.d) - self.o

    def take(self, n):
        if n > self.left():
            raise Malformed("unexpected end")
        v = self.d[self.o:self.o + n]
        self.o += n
        return v

    def le(self, n):
        return int.from_bytes(self.take(n), "little")

    def compact(self):
        b = self.le(1)
        if b < 0xFD:
            return b
        width = {0xFD: 2, 0xFE: 4, 0xFF: 8}[b]
        v = self.le(width)
        self.excess += 1 + width - len(compact(v))
        return v

    def count(self, min_size):
        n = self.compact()
        if n * min_size > self.left():
            raise Malformed("count")
        return n


def read_tx(rd):
    """one transaction at the reader's position (Transaction::deserialize, chain/src/transaction.rs:249-330)
    -> {"raw", "inputs": [(prevout, script)], "outputs": [script]}"""
    start = rd.o
    header = rd.le(4)
    ow, version = bool(header >> 31), header & 0x7FFFFFFF
    vgid = rd.le(4) if ow else 0
    is_ow = ow and version == 3 and vgid == OVERWINTER_VGID
    is_sap = ow and version == 4 and vgid == SAPLING_VGID
    if ow and not (is_ow or is_sap):
        raise Malformed("version")
    inputs, outputs = [], []
    for _ in range(rd.count(41)):
        prev = rd.take(36)
        inputs.append((prev, rd.take(rd.compact())))
        rd.take(4)
    for _ in range(rd.count(9)):
        rd.take(8)
        outputs.append(rd.take(rd.compact()))
    rd.take(4)
    if ow:
        rd.take(4)
    n_shielded = 0
    if is_sap:
        rd.take(8)
        for size in (384, 948):
            n = rd.count(size)
            n_shielded += n
            rd.take(size * n)
    if version >= 2:
        size = 1698 if is_sap else 1802
        n = rd.count(size)
        rd.take(size * n)
        if n:
            rd.take(32 + 64)
    if is_sap and n_shielded:
        rd.take(64)
    return {"raw": rd.d[start:rd.o], "inputs": inputs, "outputs": outputs}


def is_coinbase(tx):
    return len(tx["inputs"]) == 1 and tx["inputs"][0][0] == b"\x00" * 32 + b"\xff" * 4


def script_sigops(script):
    """Script::sigops_count(false)"""
    pc, total, n = 0, 0, len(script)
    while pc < n:
        op = script[pc]
        if op not in KNOWN_OPCODES:
            return total
        if op <= 0x4B:
            step = 1 + op
        elif op <= 0x4E:
            lb = {0x4C: 1, 0x4D: 2, 0x4E: 4}[op]
            if pc + 1 + lb > n:
                return total
            step = 1 + lb + int.from_bytes(script[pc + 1:pc + 1 + lb], "little")
        else:
            step = 1
            total += 1 if op in (0xAC, 0xAD) else 20 if op in (0xAE, 0xAF) else 0
        if pc + step > n:
            return total
        pc += step
    return total


def script_from_recipe(e):
    """a script of tests/golden/blocks.json: its hex, or a fill byte, a length and the bytes patched in"""
    if "hex" in e:
        return bytes.fromhex(e["hex"])
    s = bytearray(bytes.fromhex(e["fill"]) * e["len"])
    for off, h in e["patch"].items():
        s[int(off):int(off) + len(h) // 2] = bytes.fromhex(h)
    return bytes(s)


def tx_sigops(tx):
    """transaction_sigops(tx, NoopStore, false)"""
    total = sum(script_sigops(s) for s in tx["outputs"])
    if not is_coinbase(tx):
        total += sum(script_sigops(s) for _, s in tx["inputs"])
    return total


def parse_block(raw):
    """-> (TX_* status, block dict | None): {"txs", "size"}; None when MALFORMED"""
    raw = bytes(raw)
    rd = Reader(raw)
    try:
        rd.take(140)
        if rd.take(3) != b"\xfd\x40\x05":
            raise Malformed("solution prefix")
        rd.take(HEADER_BYTES - 143)
        txs = [read_tx(rd) for _ in range(rd.count(10))]
        if rd.left():
            raise Malformed("trailing bytes")
    except Malformed:
        return TX_MALFORMED, None
    return (TX_NONCANONICAL if rd.excess else TX_OK), {"txs": txs, "size": len(raw) - rd.excess}


def layout(raw):
    """what zg_block_layout reports: (status, [transactions, size, sigops, coinbase first, first later coinbase,
    consumed], transaction offsets | None)"""
    st, b = parse_block(raw)
    if b is None:
        return st, [0] * 6, None
    txs = b["txs"]
    later = [i for i, t in enumerate(txs) if i and is_coinbase(t)]
    off = [len(raw) - sum(len(t["raw"]) for t in txs[i:]) for i in range(len(txs) + 1)]
    return st, [len(txs), b["size"], sum(map(tx_sigops, txs)), int(bool(txs) and is_coinbase(txs[0])),
                later[0] if later else NO_INDEX, len(raw)], off


def verify(raw, max_block_size, max_block_sigops):
    """BlockVerifier::check -> (BLK_* status, flags, detail, merkle root | None, [transaction ids])"""
    st, out, off = layout(raw)
    if st != TX_OK:
        return (BLK_MALFORMED if st == TX_MALFORMED else BLK_NONCANONICAL), 0, 0, None, []
    n, size, sigops, cb0, later, _ = out
    ids = [dhash256(raw[off[i]:off[i + 1]]) for i in range(n)]
    root = merkle_root(ids) if n else None
    flags = ((F_EMPTY if n == 0 else 0) | (0 if cb0 else F_COINBASE) | (F_SIZE if size > max_block_size else 0) |
             (F_EXTRA_COINBASE if later != NO_INDEX else 0) | (F_DUPLICATED if len(set(ids)) != n else 0) |
             (F_SIGOPS if sigops > max_block_sigops else 0) |
             (F_MERKLE_ROOT if n and root != raw[36:68] else 0))
    order = [(F_EMPTY, BLK_EMPTY), (F_COINBASE, BLK_COINBASE), (F_SIZE, BLK_SIZE),
             (F_EXTRA_COINBASE, BLK_EXTRA_COINBASE), (F_DUPLICATED, BLK_DUPLICATED), (F_SIGOPS, BLK_SIGOPS),
             (F_MERKLE_ROOT, BLK_MERKLE_ROOT)]
    status = next((s for f, s in order if flags & f), BLK_OK)
    detail = size if status == BLK_SIZE else later if status == BLK_EXTRA_COINBASE else 0
    return status, flags, detail, root, ids


# ---- synthetic blocks for the tests
def min_tx(tag, coinbase=False, out_script=b"\x51", in_script=b""):
    """a version-1 transaction with one input and one output, distinct per tag"""
    prev = b"\x00" * 32 + b"\xff" * 4 if coinbase else hashlib.sha256(b"prev%d" % tag).digest() + b"\x00" * 4
    in_script = in_script or (b"\x04" + tag.to_bytes(4, "little") if coinbase else b"")
    return (b"\x01\x00\x00\x00\x01" + prev + compact(len(in_script)) + in_script + b"\xff" * 4 + b"\x01" +
            (tag + 1).to_bytes(8, "little") + compact(len(out_script)) + out_script + b"\x00" * 4)


def make_block(header, txs, fix_root=True, count=None):
    """header: 1487 bytes; the root over the transactions' ids patched into bytes 36..67"""
    body = (compact(len(txs)) if count is None else count) + b"".join(txs)
    if fix_root and txs:
        header = header[:36] + merkle_root([dhash256(t) for t in txs]) + header[68:]
    return bytes(header) + body
